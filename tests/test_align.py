"""Five-point landmark alignment without a GPU: the three C-ABI entries exist in the header, the binding table and the
library; the NumPy restatements the GPU tests compare against (tests/align_ref.py) are right on cases with a known
answer; the Python entry points reject wrong shapes and dtypes before they look for a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import align_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('dif_warp_affine', 'dif_align_crop', 'dif_mtcnn_landmarks')


def test_entries_in_header_binding_table_and_library():
    from deep_insight_face import _native
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dif.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r'\bint %s\s*\(' % name, src), name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_native.SIGNATURES['dif_warp_affine'][1]) == 10
    assert len(_native.SIGNATURES['dif_align_crop'][1]) == 12


def test_template_is_the_public_arcface_one():
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112 as T
    assert T.shape == (5, 2) and T.dtype == np.float32
    assert T[0, 0] < T[1, 0] and T[3, 0] < T[4, 0]            # left before right, in x
    assert T[0, 1] < T[2, 1] < T[3, 1]                         # eyes above nose above mouth
    np.testing.assert_allclose(T.mean(0), [56.02616, 71.90078], atol=1e-4)


@pytest.mark.parametrize('scale,deg,tx,ty', [(1.0, 0.0, 0.0, 0.0), (0.15, 70.0, 300.0, 200.0), (5.0, -70.0, 40.0, 60.0),
                                             (1.3, 20.0, -5.0, 12.5)])
def test_restated_fit_inverts_an_exact_similarity(scale, deg, tx, ty):
    """Landmarks = the template under a similarity S: the fit is S itself (output pixel -> frame position)."""
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112 as T
    fwd = ar.similarity(scale, deg, tx, ty)
    m = ar.fit(ar.apply(fwd, T), T)
    np.testing.assert_allclose(m, fwd, rtol=0, atol=1e-9 * max(1.0, scale) * 640)
    np.testing.assert_allclose(ar.apply(ar.invert(m), ar.apply(fwd, T)), T.astype(np.float64), atol=1e-9)
    assert np.isnan(ar.fit(np.tile(T[:1], (5, 1)), T)).all()     # five equal points


def test_restated_warp_on_known_answers():
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    ident = np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (2, 1))
    assert np.array_equal(ar.warp_affine(frames, ident, (9, 11)), frames)
    assert np.array_equal(ar.warp_affine(frames, ident, (4, 6)), frames[:, :4, :6])
    shift = np.tile(np.array([1, 0, -2, 0, 1, 3], np.float32), (2, 1))      # out(x, y) = frame(x - 2, y + 3)
    got = ar.warp_affine(frames, shift, (9, 11))
    assert np.array_equal(got[:, :6, 2:], frames[:, 3:, :9]) and not got[:, :, :2].any() and not got[:, 6:].any()
    half = np.tile(np.array([1, 0, 0.5, 0, 1, 0], np.float32), (2, 1))      # midway between two columns: round half up
    want = np.floor((frames[:, :, :-1].astype(np.float32) + frames[:, :, 1:]) / 2 + 0.5).astype(np.uint8)
    assert np.array_equal(ar.warp_affine(frames, half, (9, 10)), want)
    k2 = ar.warp_affine(frames, np.stack([ident[0], shift[0], shift[1], ident[1]]), (9, 11), k=2)   # crop j reads frame j // k
    assert np.array_equal(k2[0], frames[0]) and np.array_equal(k2[1], got[0])
    assert np.array_equal(k2[2], got[1]) and np.array_equal(k2[3], frames[1])
    nan = ident.copy()
    nan[1, 4] = np.nan
    out = ar.warp_affine(frames, nan, (9, 11))
    assert np.array_equal(out[0], frames[0]) and not out[1].any()
    assert not ar.warp_affine(frames, np.tile(np.array([1, 0, 1e30, 0, 1, 0], np.float32), (2, 1)), (3, 3)).any()


def test_restated_landmark_decode_uses_the_clamped_rectangle():
    o = np.zeros((2, 16), np.float32)
    o[:, 6:11] = [0.0, 1.0, 0.5, 0.25, 0.75]
    o[:, 11:16] = [0.0, 0.0, 0.5, 1.0, 1.0]
    boxes = np.array([[10, 20, 50, 60], [-8.5, -3, 40.7, 130]], np.float32)     # the second overhangs a 96 x 128 frame
    lm = ar.decode_landmarks(o, boxes, 96, 128)
    assert np.array_equal(lm[0, :, 0], [10, 50, 30, 20, 40]) and np.array_equal(lm[0, :, 1], [20, 20, 40, 60, 60])
    assert np.array_equal(lm[1, :, 0], [0, 40, 20, 10, 30]) and np.array_equal(lm[1, :, 1], [0, 0, 48, 96, 96])


def test_python_entry_points_validate_before_touching_the_device():
    """ValueError for wrong shapes and dtypes with or without a device (as run.crop_faces); with well-formed arguments
    and no device the library's own error, never a host computation."""
    import torch
    from deep_insight_face import _native, api
    from deep_insight_face.detector.align import align_faces, warp_affine
    frames = np.zeros((2, 8, 10, 3), np.uint8)
    lm = np.zeros((2, 5, 2), np.float32)
    mats = np.zeros((2, 2, 3), np.float32)
    for bad in (frames.astype(np.float32), frames[..., :2], frames[0]):
        with pytest.raises(ValueError):
            warp_affine(bad, mats, (4, 4))
        with pytest.raises(ValueError):
            align_faces(bad, lm)
    for bad in (mats[:1], np.zeros((2, 3, 2), np.float32), np.zeros((2, 6), np.int32), np.zeros((4, 2, 3), np.float32)):
        with pytest.raises(ValueError):
            warp_affine(frames, bad, (4, 4))
    with pytest.raises(ValueError):
        warp_affine(frames, mats, (0, 4))
    with pytest.raises(ValueError):
        warp_affine(frames, mats, (4, 4), k=0)
    for bad in (lm[:1], np.zeros((2, 4, 2), np.float32), np.zeros((2, 5, 2), np.int64), np.zeros((2, 10), np.float32)):
        with pytest.raises(ValueError):
            align_faces(frames, bad)
    with pytest.raises(ValueError):
        align_faces(frames, lm, k=2)                              # 2 frames x 2 faces need four landmark sets
    with pytest.raises(ValueError):
        align_faces(frames, lm, template=np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError):
        align_faces(frames, lm, valid=np.zeros((3,), np.float32))
    with pytest.raises(ValueError):
        align_faces(frames, lm, size=0)
    with pytest.raises(ValueError):
        api.align_face(frames[0], lm[0, :4])
    with pytest.raises(ValueError):
        api.align_face(frames[0, :, :, 0], lm[0])
    if not torch.cuda.is_available():
        with pytest.raises(_native.DifError):
            warp_affine(frames, mats, (4, 4))
        with pytest.raises(_native.DifError):
            align_faces(frames, lm)


def test_c_entries_check_their_arguments():
    """Bad sizes and null pointers are refused before any launch (no device needed); n == 0 returns at once."""
    from deep_insight_face import _native as N
    L = N.lib
    assert L.dif_warp_affine(None, 0, 8, 8, None, 1, None, 4, 4, None) == 0
    assert L.dif_align_crop(None, 0, 8, 8, None, None, 1, None, None, 112, None, None) == 0
    assert L.dif_mtcnn_landmarks(None, 16, None, None, 0, 8, 8, 96, 128, None, None) == 0
    assert L.dif_warp_affine(None, 1, 8, 8, None, 0, None, 4, 4, None) != 0 and 'dif_warp_affine: bad sizes' in N.last_error()
    assert L.dif_warp_affine(None, 1, 8, 8, None, 1, None, 4, 4, None) != 0 and 'dif_warp_affine: null pointer' in N.last_error()
    assert L.dif_align_crop(None, 1, 8, 8, None, None, 1, None, None, 0, None, None) != 0 and 'dif_align_crop: bad sizes' in N.last_error()
    assert L.dif_align_crop(None, 1, 8, 8, None, None, 1, None, None, 112, None, None) != 0 and 'dif_align_crop: null pointer' in N.last_error()
    assert L.dif_mtcnn_landmarks(None, 8, None, None, 1, 8, 8, 96, 128, None, None) != 0 and 'dif_mtcnn_landmarks: bad sizes' in N.last_error()
    assert L.dif_mtcnn_landmarks(None, 16, None, None, 1, 8, 8, 96, 128, None, None) != 0 and 'null pointer' in N.last_error()
