"""tests/quality_ref.py on cases worked out by hand, its brute-force best row against an independent formulation, and the
layers of the feature tied to each other: header, library, binding table, module.  (No GPU.)"""
import os
import re

import numpy as np
import pytest

import quality_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gray_crops(g):
    """[M, S, S] gray values -> crops whose three channels all hold them (then g is that value)."""
    return np.repeat(np.asarray(g, np.uint8)[..., None], 3, axis=-1)


def _checkerboard(s):
    y, x = np.mgrid[:s, :s]
    return _gray_crops((((y + x) & 1) * 255)[None])


def test_gray_weights_and_channel_symmetry():
    c = np.array([[[[10, 200, 31]] * 3] * 3], np.uint8)
    assert R.gray(c)[0, 0, 0] == (10 + 400 + 31 + 2) >> 2 == 110
    assert np.array_equal(R.gray(c), R.gray(c[..., ::-1]))
    rng = np.random.default_rng(0)
    c = rng.integers(0, 256, (2, 9, 9, 3), dtype=np.uint8)
    assert np.array_equal(R.stats(c), R.stats(c[..., ::-1]))
    assert R.gray(np.full((1, 3, 3, 3), 255, np.uint8)).max() == 255


def test_size_three_has_one_interior_pixel_and_no_sharpness():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 256, (4, 3, 3, 3), dtype=np.uint8)
    st, q = R.face_quality(c)
    g = R.gray(c)
    lap = g[:, 0, 1] + g[:, 2, 1] + g[:, 1, 0] + g[:, 1, 2] - 4 * g[:, 1, 1]
    assert np.array_equal(st[:, 2], lap) and np.array_equal(st[:, 3], lap * lap)
    assert np.array_equal(q[:, 2], np.zeros(4, np.float32))              # one sample: variance 0


@pytest.mark.parametrize('s', [4, 17, 112])
def test_horizontal_ramp_has_zero_laplacian(s):
    c = _gray_crops(np.broadcast_to(np.arange(s) * 2, (1, s, s)))
    st, q = R.face_quality(c)
    assert st[0, 2] == 0 and st[0, 3] == 0 and q[0, 2] == 0
    assert st[0, 0] == s * (s * (s - 1)) and q[0, 0] == np.float32((s - 1) / 255.0)


@pytest.mark.parametrize('value', [0, 255])
def test_flat_crops_are_wholly_clipped(value):
    st, q = R.face_quality(np.full((2, 8, 8, 3), value, np.uint8))
    assert q[0, 3] == 1 and q[0, 1] == 0 and q[0, 2] == 0 and q[0, 0] == value / 255 and q[0, 9] == 0
    assert st[0].tolist() == [64 * value, 64 * value * value, 0, 0, 64 if value == 0 else 0, 64 if value == 255 else 0]
    st, q = R.face_quality(np.full((1, 8, 8, 3), 128, np.uint8), lo=15, hi=240)
    assert q[0, 3] == 0


@pytest.mark.parametrize('s', [4, 64, 224, 256])
def test_checkerboard_sharpness(s):
    st, q = R.face_quality(_checkerboard(s))
    k = (s - 2) ** 2
    assert st[0, 3] == k * 1020 * 1020 and st[0, 2] == 0                 # even s: as many +1020 as -1020
    assert q[0, 2] == np.float32(1040400.0) and q[0, 3] == 1 and q[0, 0] == np.float32(0.5)
    assert k * int(st[0, 3]) < 2 ** 53                                   # the numerator converts exactly


def _box_blur(g):
    p = np.pad(g.astype(np.float64), 1, mode='edge')
    s = g.shape[0]
    return np.round(sum(p[dy:dy + s, dx:dx + s] for dy in range(3) for dx in range(3)) / 9.0).astype(np.uint8)


def test_blur_lowers_sharpness_strictly():
    g = np.random.default_rng(2).integers(0, 256, (112, 112), dtype=np.uint8)
    sharp = []
    for _ in range(4):
        sharp.append(float(R.face_quality(_gray_crops(g[None]))[1][0, 2]))
        g = _box_blur(g)
    assert sharp[0] > sharp[1] > sharp[2] > sharp[3] > 0, sharp
    assert sharp[0] > 10 * sharp[1]


def test_arcface_template_values():
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112 as T
    q = R.columns(np.zeros((1, 6), np.int64), 112, T[None])
    # the values as they were quoted, to the digits quoted: half a unit of the last one
    assert q[0, 4] == np.float32(35.237736) and abs(float(q[0, 5]) + 0.00553102) < 5e-9
    assert q[0, 7] == np.float32(0.49495593) and abs(float(q[0, 6]) - 3.49e-5) < 5e-8
    assert np.isnan(q[0, 8])
    # scale and shift leave the ratios alone (up to the rounding of the float32 landmarks)
    q2 = R.columns(np.zeros((1, 6), np.int64), 112, (T * np.float32(3) + np.float32(100))[None])
    assert abs(q2[0, 4] - 3 * q[0, 4]) < 1e-3 and np.allclose(q2[0, 5:8], q[0, 5:8], atol=1e-5)


def test_nan_rules_of_the_geometry():
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112 as T
    lm = np.repeat(T[None], 4, 0).copy()
    lm[0] = np.nan                                       # nothing passed
    lm[1, 3, 0] = np.nan                                 # one mouth coordinate: nose_drop alone
    lm[2, 1] = lm[2, 0]                                  # coincident eyes
    lm[3, 3], lm[3, 4] = lm[3, 0], lm[3, 1]              # mouth midpoint = eye midpoint
    st = np.tile(np.array([[100, 2000, 0, 900, 0, 0]], np.int64), (4, 1))
    q = R.columns(st, 3, lm)
    assert np.isnan(q[0, 4:8]).all() and np.isnan(q[0, 9])
    assert np.isnan(q[1, 7]) and not np.isnan(q[1, 4:7]).any() and not np.isnan(q[1, 9])
    assert q[2, 4] == 0 and np.isnan(q[2, 5]) and np.isnan(q[2, 6]) and np.isnan(q[2, 9])
    assert np.isnan(q[3, 7]) and not np.isnan(q[3, 6])
    boxes = np.array([[10, 10, 50, 50], [-20, 0, 20, 40], [-50, 0, -10, 40], [5, 5, 5, 30], [np.nan, 0, 10, 10]], np.float32)
    qb = R.columns(np.tile(st[:1], (5, 1)), 3, None, boxes, (100, 100))
    assert qb[:3, 8].tolist() == [1.0, 0.5, 0.0] and np.isnan(qb[3:, 8]).all() and np.isnan(qb[3:, 9]).all()
    assert np.isnan(qb[:, 4:8]).all()
    assert qb[1, 9] == np.float32(np.float64(qb[1, 2]) * (1.0 - np.float64(qb[1, 3])) * 0.5)   # no yaw factor without landmarks


def _best_case(seed, n, n_labels):
    rng = np.random.default_rng(seed)
    labels = rng.integers(-2, n_labels, n).astype(np.int64)
    key = rng.choice(np.array([0.0, -0.0, 1.5, -3.0, np.inf, -np.inf, np.nan, 2.25, 1e-30], np.float32), n)
    return labels, key


@pytest.mark.parametrize('n,n_labels', [(1, 1), (50, 4), (400, 40), (3000, 7)])
def test_brute_force_best_against_the_sorted_formulation(n, n_labels):
    labels, key = _best_case(n, n, n_labels)
    a, b = R.best(labels, key, 17), R.best_by_sort(labels, key, 17)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        if x.dtype == np.float32:                        # bits where there is a number, NaN in the same places
            assert np.array_equal(np.isnan(x), np.isnan(y))
            x, y = x[~np.isnan(x)].view(np.uint32), y[~np.isnan(y)].view(np.uint32)
        assert np.array_equal(x, y)


def test_best_rules_by_hand():
    nan, inf = np.nan, np.inf
    labels = [3, 3, 3, -1, 5, 5, 7, 7, 9, 2, 2]
    key = np.array([1.0, 2.0, 2.0, 99.0, -0.0, 0.0, nan, -inf, nan, nan, inf], np.float32)
    tl, bk, br, cnt = R.best(labels, key, 100)
    assert tl.tolist() == [2, 3, 5, 7, 9] and cnt.tolist() == [2, 3, 2, 2, 1]
    assert br.tolist() == [110, 101, 104, 107, -1]
    assert bk[0] == inf and bk[1] == 2 and np.signbit(bk[2]) and bk[3] == -inf and np.isnan(bk[4])


def test_chunked_reference_adds_equal_one_add():
    labels, key = _best_case(5, 600, 30)
    pay = np.arange(600 * 3, dtype=np.float32).reshape(600, 3)
    one = R.RefShots()
    index = one.add(labels, key, emb=pay)
    tl, bk, br, cnt = R.best(labels, key)
    assert np.array_equal(one.labels, tl) and np.array_equal(one.row, br) and np.array_equal(one.counts, cnt)
    assert np.array_equal(one.payload['emb'][br >= 0], pay[br[br >= 0]])
    many = R.RefShots()
    cuts = [0, 1, 8, 72, 600]
    got = np.concatenate([many.add(labels[a:b], key[a:b], emb=pay[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(many.labels, one.labels) and np.array_equal(many.row, one.row) and np.array_equal(many.counts, one.counts)
    assert np.array_equal(many.key.view(np.uint32)[one.row >= 0], one.key.view(np.uint32)[one.row >= 0])
    assert np.array_equal(many.payload['emb'], one.payload['emb'])
    assert np.array_equal(got[cuts[3]:], index[cuts[3]:])


def test_header_library_and_binding_table_carry_the_feature():
    """Fails on a tree without the feature: both entries declared in include/dif.h, exported by libdif.so and bound in
    _native.SIGNATURES with the header's argument counts."""
    from deep_insight_face import _native
    raw = open(os.path.join(ROOT, 'include', 'dif.h')).read()
    header = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name, k in {'dif_face_quality': 12, 'dif_pool_best': 12}.items():
        decl = re.search(r'\bint %s\s*\(([^;]*)\);' % name, header, flags=re.S)
        assert decl and decl.group(1).count(',') + 1 == k, name
        assert hasattr(_native.lib, name) and len(_native.SIGNATURES[name][1]) == k, name
    assert re.search(r'#define DIF_QUALITY_COLS 10\b', raw)
    assert _native.lib.dif_version() == 110
    from deep_insight_face.detector import quality
    assert quality.QUALITY_COLS == 10 and quality.FaceQuality._fields[1:] == R.COLS


def test_module_checks_arguments_and_has_no_cpu_fallback():
    import torch
    from deep_insight_face import _native, templates
    from deep_insight_face.detector import quality
    from deep_insight_face.detector.faces import FrameFaces
    crops = np.zeros((2, 8, 8, 3), np.uint8)
    for bad in (crops.astype(np.float32), crops[..., :2], crops[:, :, :4], np.zeros((1, 2, 2, 3), np.uint8),
                np.zeros((1, 257, 257, 3), np.uint8)):
        with pytest.raises(ValueError):
            quality.face_quality(bad)
    with pytest.raises(ValueError):
        quality.face_quality(crops, boxes=np.zeros((2, 4), np.float32))              # boxes without frame_hw
    with pytest.raises(ValueError):
        quality.face_quality(crops, landmarks=np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError):
        quality.face_quality(crops, boxes=np.zeros((3, 4), np.float32), frame_hw=(10, 10))
    with pytest.raises(ValueError):
        quality.face_quality(crops, lo=-1)
    assert callable(FrameFaces.quality) and callable(FrameFaces.best) and callable(templates.BestShots)
    if not torch.cuda.is_available():
        with pytest.raises(_native.DifError):
            quality.face_quality(crops)
        with pytest.raises(_native.DifError):
            templates.BestShots()


def test_mask_on_host_columns():
    from deep_insight_face.detector.quality import FaceQuality
    nan = np.nan
    cols = np.array([[.5, .2, 100, 0.0, 40, 0.0, 0.1, .5, 1.0, 90],
                     [.5, .2, 10, 0.5, 10, 0.3, -0.8, .5, 0.4, 1],
                     [.5, .2, 100, 0.0, nan, nan, nan, nan, nan, nan]], np.float32)
    q = FaceQuality(np.zeros((3, 6), np.int64), *cols.T)
    assert q.mask().tolist() == [True, True, True]
    assert q.mask(min_sharpness=50).tolist() == [True, False, True]
    assert q.mask(min_eye_dist=20).tolist() == [True, False, False]
    assert q.mask(max_abs_yaw=0.5).tolist() == [True, False, False]
    assert q.mask(max_abs_roll=0.1).tolist() == [True, False, False]
    assert q.mask(min_inside=0.5).tolist() == [True, False, False]
    assert q.mask(max_clipped=0.25).tolist() == [True, False, True]
    assert q.mask(min_score=1).tolist() == [True, True, False]
