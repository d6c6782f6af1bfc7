"""Every face in a frame, the part that needs no GPU: the NumPy restatement of the compaction (tests/faces_ref.py) against
plain loops, the C entry points' argument checks, and gather_faces' validation."""
import numpy as np
import pytest

import faces_ref

ENTRIES = ('dif_faces_compact', 'dif_crop_resize_list', 'dif_align_crop_list', 'dif_faces_gather')


def _loops(scores, min_score, max_faces):
    n, k = scores.shape
    offsets, frame, slot = [0], [], []
    for f in range(n):
        for s in range(k):
            v = float(scores[f, s])
            if v == v and v >= min_score:
                frame.append(f)
                slot.append(s)
        offsets.append(len(frame))
    count = len(frame)
    frame, slot = frame[:max_faces], slot[:max_faces]
    pad = [-1] * (max_faces - len(frame))
    return count, offsets, frame + pad, slot + pad


@pytest.mark.parametrize('n,k,max_faces', [(1, 1, None), (3, 5, None), (9, 7, 10), (70, 33, 100), (0, 4, None), (4, 3, 0)])
def test_reference_compaction_against_loops(n, k, max_faces):
    rng = np.random.default_rng(n * 100 + k)
    for min_score in (0.0, 0.7):
        ms = np.float32(min_score)
        pool = np.array([-1.0, np.nan, ms, np.nextafter(ms, np.float32(-np.inf)), 0.0, 0.9], np.float32)
        scores = pool[rng.integers(0, len(pool), (n, k))]
        rnd = rng.random((n, k)) < 0.3
        scores[rnd] = rng.random((n, k), dtype=np.float32)[rnd]
        count, offsets, frame, slot = faces_ref.compact(scores, ms, max_faces)
        cap = n * k if max_faces is None else max_faces
        wc, wo, wf, ws = _loops(scores, float(ms), cap)
        assert count == wc and offsets.tolist() == wo and frame.tolist() == wf and slot.tolist() == ws
        assert offsets.dtype == frame.dtype == slot.dtype == np.int32


def test_binding_table_has_the_entry_points():
    from deep_insight_face import _native
    for name in ENTRIES:
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)
    assert len(_native.SIGNATURES['dif_faces_compact'][1]) == 10
    assert len(_native.SIGNATURES['dif_crop_resize_list'][1]) == 13
    assert len(_native.SIGNATURES['dif_align_crop_list'][1]) == 14
    assert len(_native.SIGNATURES['dif_faces_gather'][1]) == 9


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """k < 1, max_faces < 0 and null pointers fail with a message; an empty list is a no-op.  (No pointer is followed.)"""
    from deep_insight_face import _native as N
    L = N.lib
    one = 0x1000                                               # never dereferenced: every call below fails, or has nothing to do
    assert L.dif_faces_compact(one, 2, 0, 0.0, 4, one, one, one, one, None) != 0 and 'dif_faces_compact: bad sizes' in N.last_error()
    assert L.dif_faces_compact(one, 2, 3, 0.0, -1, one, one, one, one, None) != 0 and 'dif_faces_compact: bad sizes' in N.last_error()
    assert L.dif_faces_compact(one, -1, 3, 0.0, 4, one, one, one, one, None) != 0 and 'dif_faces_compact: bad sizes' in N.last_error()
    for args in ((None, 2, 3, 0.0, 4, one, one, one, one), (one, 2, 3, 0.0, 4, None, one, one, one),
                 (one, 2, 3, 0.0, 4, one, None, one, one), (one, 2, 3, 0.0, 4, one, one, None, one),
                 (one, 2, 3, 0.0, 4, one, one, one, None)):
        assert L.dif_faces_compact(*args, None) != 0 and 'dif_faces_compact: null pointer' in N.last_error()
    assert L.dif_crop_resize_list(None, 1, 8, 8, None, 2, None, None, 0, 8.0, None, 112, None) == 0
    assert L.dif_crop_resize_list(one, 1, 8, 8, one, 0, one, one, 1, 8.0, one, 112, None) != 0 and 'dif_crop_resize_list: bad sizes' in N.last_error()
    assert L.dif_crop_resize_list(one, 1, 8, 8, one, 2, None, one, 1, 8.0, one, 112, None) != 0 and 'dif_crop_resize_list: null pointer' in N.last_error()
    assert L.dif_align_crop_list(None, 1, 8, 8, None, 2, None, None, 0, None, None, 112, None, None) == 0
    assert L.dif_align_crop_list(one, 1, 8, 8, one, 2, one, one, 1, None, one, 0, None, None) != 0 and 'dif_align_crop_list: bad sizes' in N.last_error()
    assert L.dif_align_crop_list(one, 1, 8, 8, None, 2, one, one, 1, None, one, 112, None, None) != 0 and 'dif_align_crop_list: null pointer' in N.last_error()
    assert L.dif_faces_gather(None, 4, 1, 2, None, None, 0, None, None) == 0
    assert L.dif_faces_gather(one, 0, 1, 2, one, one, 1, one, None) != 0 and 'dif_faces_gather: bad sizes' in N.last_error()
    assert L.dif_faces_gather(one, 4, 1, 2, one, one, 1, None, None) != 0 and 'dif_faces_gather: null pointer' in N.last_error()


def test_gather_faces_validates_its_arguments_without_a_device():
    from deep_insight_face.detector.faces import FrameFaces, gather_faces
    assert FrameFaces._fields == ('offsets', 'frame', 'boxes', 'scores', 'landmarks', 'crops', 'emb', 'idx', 'dist')
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    boxes, scores, lm = np.zeros((2, 3, 4), np.float32), np.zeros((2, 3), np.float32), np.zeros((2, 3, 5, 2), np.float32)
    with pytest.raises(ValueError, match='uint8 frames'):
        gather_faces(frames.astype(np.float32), boxes, scores)
    with pytest.raises(ValueError, match='scores'):
        gather_faces(frames, boxes, scores[:1])
    with pytest.raises(ValueError, match='scores'):
        gather_faces(frames, boxes[:, :0], scores[:, :0])
    with pytest.raises(ValueError, match='boxes'):
        gather_faces(frames, boxes[:, :2], scores)
    with pytest.raises(ValueError, match='landmarks'):
        gather_faces(frames, boxes, scores, lm[:, :, :4])
    with pytest.raises(ValueError, match='align=True needs the landmarks'):
        gather_faces(frames, boxes, scores, align=True)
    with pytest.raises(ValueError, match='max_faces'):
        gather_faces(frames, boxes, scores, max_faces=-1)
    with pytest.raises(ValueError, match='size'):
        gather_faces(frames, boxes, scores, size=0)
