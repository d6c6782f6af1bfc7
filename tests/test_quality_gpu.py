"""Face quality and best shot on the device (csrc/quality.hip, dif_pool_best in csrc/templates.hip) against
tests/quality_ref.py: the six integer statistics exactly, the ten float columns bit for bit, the best row per label with
its key, count and payload.

"Bit for bit" compares the uint32 views; two NaNs count as equal whatever their sign and payload (0/0 is -NaN on the host
and +NaN on the device; NumPy promises neither).

A view of the crops that is not contiguous is COPIED by the wrapper (test_views_are_copied), so the kernel only ever sees
dense crops; their first byte need not be aligned, and for an odd size it is not (a crop of 63 x 63 x 3 bytes puts the next
one at an odd address), which is what sends the kernel down its byte-wise path."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import quality_ref as R

pytestmark = pytest.mark.gpu

SIZES = [3, 4, 5, 63, 64, 65, 96, 112, 160, 255, 256]
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float32:
        return np.array_equal(got, want)
    return bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def t2n(t):
    return t.cpu().numpy()


def cols_of(q):
    return np.stack([t2n(c) for c in q[1:]], axis=1)


def check_quality(q, want_stats, want_cols, what=''):
    got_stats, got_cols = t2n(q.stats), cols_of(q)
    assert got_stats.dtype == np.int64 and np.array_equal(got_stats, want_stats), \
        (what, np.argwhere(got_stats != want_stats)[:8].tolist())
    for c, name in enumerate(R.COLS):
        ok = (bits(got_cols[:, c]) == bits(want_cols[:, c])) | (np.isnan(got_cols[:, c]) & np.isnan(want_cols[:, c]))
        bad = np.nonzero(~ok)[0]
        if bad.size:
            print(what, name, 'rows', bad[:8].tolist(), 'got', got_cols[bad[:8], c].tolist(), 'want', want_cols[bad[:8], c].tolist())
        assert not bad.size, (what, name)


@functools.lru_cache(maxsize=None)
def contents(s):
    """The crops of one size, 65 of them: every content the statistics can go wrong on, then random ones."""
    rng = np.random.default_rng(s)
    y, x = np.mgrid[:s, :s]
    gray3 = lambda g: np.repeat(np.asarray(g, np.uint8)[..., None], 3, axis=-1)      # noqa: E731
    out = [rng.integers(0, 256, (s, s, 3), dtype=np.uint8), np.zeros((s, s, 3), np.uint8), np.full((s, s, 3), 255, np.uint8),
           gray3(((y + x) & 1) * 255), gray3((x * 255) // (s - 1)), gray3((y * 255) // (s - 1))]
    e, h = s - 1, s // 2                                  # one 255 pixel: corners, edges, one pixel in from each edge
    for py, px in ((0, 0), (0, e), (e, 0), (e, e), (0, h), (e, h), (h, 0), (h, e), (1, h), (e - 1, h), (h, 1), (h, e - 1)):
        c = np.zeros((s, s, 3), np.uint8)
        c[py, px] = 255
        out.append(c)
    c = rng.integers(0, 256, (s, s, 3), dtype=np.uint8)   # the three channels differ, c1 distinct: pins the weights 1, 2, 1
    c[..., 1] = 255 - c[..., 1] // 2
    out.append(c)
    for k in range(3):                                    # one channel alone
        c = np.zeros((s, s, 3), np.uint8)
        c[..., k] = rng.integers(0, 256, (s, s), dtype=np.uint8)
        out.append(c)
    while len(out) < 65:
        out.append(rng.integers(0, 256, (s, s, 3), dtype=np.uint8))
    crops = np.stack(out)
    crops.setflags(write=False)
    return crops


@functools.lru_cache(maxsize=None)
def reference(s, lo, hi):
    st, q = R.face_quality(contents(s), lo=lo, hi=hi)
    st.setflags(write=False)
    q.setflags(write=False)
    return st, q


@pytest.mark.parametrize('lo,hi', [(0, 255), (15, 240)])
@pytest.mark.parametrize('s', SIZES)
def test_statistics_and_image_columns(cuda, s, lo, hi):
    from deep_insight_face.detector.quality import face_quality
    crops = torch.from_numpy(contents(s).copy()).to(cuda)
    st, q = reference(s, lo, hi)
    if s % 2 == 0 and s >= 4:
        assert st[3, 3] == (s - 2) ** 2 * 1040400         # the checkerboard: the largest sum there is
    check_quality(face_quality(crops, lo=lo, hi=hi), st, q, 'M=65')
    for a in (0, 1, 4, 18):                               # M = 3 from an offset: for odd s an unaligned first crop
        check_quality(face_quality(crops[a:a + 3], lo=lo, hi=hi), st[a:a + 3], q[a:a + 3], 'M=3 from %d' % a)
    for a in (0, 3, 7, 19, 64):
        check_quality(face_quality(crops[a:a + 1], lo=lo, hi=hi), st[a:a + 1], q[a:a + 1], 'M=1 at %d' % a)


def test_views_are_copied(cuda):
    """Which of the two the wrapper does with a view that is not contiguous: it copies it."""
    from deep_insight_face.detector.quality import face_quality
    big = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (6, 40, 48, 3), dtype=np.uint8)).to(cuda)
    view = big[1::2, 3:36, 5:38]
    assert not view.is_contiguous()
    st, q = R.face_quality(t2n(view))
    check_quality(face_quality(view), st, q)
    flipped = big[:, :40, :40].flip(-1)                   # BGR for RGB: the same measures
    assert torch.equal(face_quality(flipped).stats, face_quality(big[:, :40, :40]).stats)


def test_numpy_in_numpy_out_and_empty(cuda):
    from deep_insight_face.detector.quality import face_quality
    crops = contents(5)[:4].copy()
    q = face_quality(crops)
    assert all(isinstance(c, np.ndarray) for c in q)
    st, want = reference(5, 0, 255)
    assert np.array_equal(q.stats, st[:4]) and same(np.stack(q[1:], 1), want[:4])
    q = face_quality(torch.empty((0, 112, 112, 3), dtype=torch.uint8, device=cuda),
                     torch.empty((0, 5, 2), device=cuda), torch.empty((0, 4), device=cuda), (480, 640))
    assert tuple(q.stats.shape) == (0, 6) and q.stats.dtype == torch.int64 and q.stats.is_cuda
    assert all(tuple(c.shape) == (0,) and c.dtype == torch.float32 for c in q[1:])
    assert q.mask(min_score=1.0).shape == (0,)


def landmark_cases():
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112 as T
    rng = np.random.default_rng(11)
    rows = [T, T * np.float32(3.7) + np.array([211.5, 97.25], np.float32)]
    rows += list(rng.uniform(0, 640, (48, 5, 2)).astype(np.float32))
    rows += list((T[None] + rng.normal(0, 6, (8, 5, 2))).astype(np.float32))
    nan_all = np.full((5, 2), NAN)
    nan_one = T.copy()
    nan_one[3, 0] = NAN
    nan_eye = T.copy()
    nan_eye[0, 1] = NAN
    eyes = T.copy()
    eyes[1] = eyes[0]
    mouth = T.copy()
    mouth[3], mouth[4] = mouth[0], mouth[1]
    rows += [nan_all, nan_one, nan_eye, eyes, mouth]
    return np.stack(rows).astype(np.float32)


def box_cases(hw):
    h, w = hw
    rng = np.random.default_rng(12)
    rows = [[10, 10, 50, 50], [-20, 0, 20, 40], [-50, 0, -10, 40], [5, 5, 5, 30], [NAN, 0, 10, 10], [0, 0, 10, NAN],
            [w - 10, h - 30, w + 30, h + 30], [0, 0, w, h], [-5, -5, w + 5, h + 5], [30, 30, 10, 10], [3, 4, 3, 4]]
    lt = rng.uniform(-60, [w, h], (52, 2))
    rows += list(np.concatenate([lt, lt + rng.uniform(1, 200, (52, 2))], axis=1))
    return np.asarray(rows, np.float32)


def test_geometry_columns(cuda):
    from deep_insight_face.detector.quality import face_quality
    hw = (480, 640)
    lm, bx = landmark_cases(), box_cases(hw)
    m = lm.shape[0]
    assert bx.shape[0] == m
    crops = contents(5)[:m].copy()
    st = reference(5, 0, 255)[0][:m]
    want = R.columns(st, 5, lm, bx, hw)
    assert want[0, 4] == np.float32(35.237736) and want[:3, 8].tolist() == [1.0, 0.5, 0.0]
    assert np.isnan(want[m - 5, 4:8]).all() and np.isnan(want[m - 4, 7]) and not np.isnan(want[m - 4, 4:7]).any()
    assert np.isnan(want[m - 2, 5:7]).all() and want[m - 2, 4] == 0 and np.isnan(want[m - 1, 7])
    assert np.isnan(want[3:6, 8]).all() and np.isnan(want[3:6, 9]).all()
    d = lambda a: torch.from_numpy(a).to(cuda)            # noqa: E731
    check_quality(face_quality(d(crops), d(lm), d(bx), hw), st, want, 'landmarks and boxes')
    check_quality(face_quality(d(crops), d(lm)), st, R.columns(st, 5, lm), 'landmarks')
    check_quality(face_quality(d(crops), None, d(bx), hw), st, R.columns(st, 5, None, bx, hw), 'boxes')
    none = R.columns(st, 5)
    assert np.isnan(none[:, 4:9]).all() and same(none[:, 9], (none[:, 2].astype(np.float64) * (1.0 - none[:, 3].astype(np.float64))).astype(np.float32))
    check_quality(face_quality(d(crops)), st, none, 'neither')
    with pytest.raises(ValueError):
        face_quality(d(crops), None, d(bx))


def test_mask_on_the_device(cuda):
    from deep_insight_face.detector.quality import face_quality
    hw = (480, 640)
    lm, bx = landmark_cases(), box_cases(hw)
    m = lm.shape[0]
    d = lambda a: torch.from_numpy(a).to(cuda)            # noqa: E731
    q = face_quality(d(contents(5)[:m].copy()), d(lm), d(bx), hw)
    c = {name: t2n(getattr(q, name)) for name in R.COLS}
    assert q.mask().dtype == torch.bool and q.mask().is_cuda and bool(q.mask().all())
    with np.errstate(invalid='ignore'):
        for kw, want in (({'min_sharpness': 2000.0}, c['sharpness'] >= 2000.0), ({'min_eye_dist': 30.0}, c['eye_dist'] >= 30.0),
                         ({'max_abs_yaw': 0.5}, np.abs(c['yaw']) <= 0.5), ({'max_abs_roll': 0.2}, np.abs(c['roll']) <= 0.2),
                         ({'min_inside': 0.75}, c['inside'] >= 0.75), ({'max_clipped': 0.01}, c['clipped'] <= 0.01),
                         ({'min_score': 100.0}, c['score'] >= 100.0)):
            got = t2n(q.mask(**kw))
            assert np.array_equal(got, want), kw
            assert 0 < got.sum() < m, kw                  # the bound tells faces apart
            col = c[next(n for n in R.COLS if list(kw)[0].endswith(n))]
            assert not got[np.isnan(col)].any(), kw       # a NaN fails an applied bound
        both = t2n(q.mask(min_eye_dist=30.0, min_inside=0.75))
    assert np.array_equal(both, (c['eye_dist'] >= 30.0) & (c['inside'] >= 0.75))


# ---------------------------------------------------------------------------------------------------- best shot

def check_shots(shots, ref, what=''):
    assert same(t2n(shots.labels), ref.labels), what
    assert same(t2n(shots.row), ref.row), what
    assert same(t2n(shots.counts), ref.counts), what
    assert same(t2n(shots.key), ref.key), what
    assert sorted(shots.payload) == sorted(ref.payload), what
    for name, v in ref.payload.items():
        got = t2n(shots.payload[name])
        assert got.dtype == v.dtype and got.shape == v.shape, (what, name)
        assert same(got, v) if v.dtype == np.float32 else np.array_equal(got, v), (what, name)


def rule_case():
    """labels and keys that hold every clause of the rule."""
    labels = np.array([3, 3, 3, -1, 5, 5, 6, 6, 7, 7, 9, 9, 2, 2, -7, 11, 11, 11, 12, 4, 4, 4], np.int64)
    key = np.array([1.0, 2.0, 2.0, 99.0, -0.0, 0.0, 0.0, -0.0, NAN, -INF, NAN, NAN, NAN, INF, 5.0, 0.5, NAN, 0.25, -INF, 7.0, 7.0, 7.0],
                   np.float32)
    return labels, key


def test_best_rules(cuda):
    from deep_insight_face.templates import BestShots
    labels, key = rule_case()
    ref = R.RefShots()
    want_index = ref.add(labels, key)
    assert ref.labels.tolist() == [2, 3, 4, 5, 6, 7, 9, 11, 12]
    assert ref.row.tolist() == [13, 1, 19, 4, 6, 9, -1, 15, 18] and ref.counts.tolist() == [2, 3, 3, 2, 2, 2, 2, 3, 1]
    assert np.signbit(ref.key[3]) and not np.signbit(ref.key[4]) and ref.key[5] == -INF and np.isnan(ref.key[6])
    shots = BestShots()
    index = shots.add(torch.from_numpy(labels).to(cuda), torch.from_numpy(key).to(cuda))
    assert same(t2n(index), want_index)
    check_shots(shots, ref)
    assert np.array_equal(bits(t2n(shots.key))[[3, 4]], bits(ref.key)[[3, 4]])          # the zero of the lower row, sign and all
    again = shots.add(labels.astype(np.int32), key)                                    # NumPy in -> NumPy out; the state goes on
    assert isinstance(again, np.ndarray) and same(again, ref.add(labels, key))
    check_shots(shots, ref, 'second add')
    assert shots.row_base == 2 * labels.size and shots.row.tolist() == ref.row.tolist()


@pytest.mark.parametrize('case', ['one_row', 'one_label_5000', 'singletons_3000', 'all_negative'])
def test_best_shapes(cuda, case):
    from deep_insight_face.templates import BestShots
    rng = np.random.default_rng(3)
    if case == 'one_row':
        labels, key = np.array([41], np.int64), np.array([-2.5], np.float32)
    elif case == 'one_label_5000':
        labels = np.full(5000, 2 ** 40 + 3, np.int64)
        key = rng.integers(0, 50, 5000).astype(np.float32)               # many exact ties: the lower row
        key[rng.integers(0, 5000, 300)] = NAN
    elif case == 'singletons_3000':
        labels = rng.permutation(3000).astype(np.int64) * 7
        key = rng.standard_normal(3000).astype(np.float32)
        key[::17] = NAN
    else:
        labels, key = np.array([-1, -5, -1], np.int64), np.array([1, 2, 3], np.float32)
    emb = rng.standard_normal((labels.size, 32)).astype(np.float32)
    ref = R.RefShots()
    want = ref.add(labels, key, emb=emb)
    shots = BestShots()
    got = shots.add(torch.from_numpy(labels).to(cuda), torch.from_numpy(key).to(cuda), emb=torch.from_numpy(emb).to(cuda))
    assert same(t2n(got), want)
    check_shots(shots, ref, case)
    if case == 'one_label_5000':
        assert ref.row[0] == int(np.nonzero(key == np.nanmax(key))[0][0])


def test_chunked_adds_equal_one_add(cuda):
    from deep_insight_face.templates import BestShots
    rng = np.random.default_rng(4)
    n = 1500
    labels = rng.integers(-1, 60, n).astype(np.int64) * 3
    labels[labels < 0] = -1
    labels[:72][labels[:72] == 90] = 87                     # label 90 first shows in the last chunk ...
    labels[100] = 90                                        # ... and sorts into the middle of the stored ones
    key = rng.choice(np.array([0.0, -0.0, 1.5, -3.0, INF, -INF, NAN, 2.25, 1e-30, 7.0], np.float32), n)
    crops = rng.integers(0, 256, (n, 4, 4, 3), dtype=np.uint8)
    emb = rng.standard_normal((n, 32)).astype(np.float32)
    d = lambda a: torch.from_numpy(a).to(cuda)              # noqa: E731
    ref = R.RefShots()
    want = ref.add(labels, key, crops=crops, emb=emb)
    assert 90 in ref.labels and ref.labels[0] < 90 < ref.labels[-1] and (ref.row == -1).sum() == 0
    one = BestShots()
    index = one.add(d(labels), d(key), crops=d(crops), emb=d(emb))
    assert same(t2n(index), want)
    check_shots(one, ref, 'one add')
    many, step = BestShots(), R.RefShots()
    cuts = [0, 1, 8, 72, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        got = many.add(d(labels[a:b]), d(key[a:b]), crops=d(crops[a:b]), emb=d(emb[a:b]))
        assert same(t2n(got), step.add(labels[a:b], key[a:b], crops=crops[a:b], emb=emb[a:b])), (a, b)
        check_shots(many, step, 'after %d rows' % b)
        assert (90 in step.labels) == (b == n)
    check_shots(many, ref, 'chunked')
    assert np.array_equal(bits(t2n(many.key)), bits(t2n(one.key))) and torch.equal(many.row, one.row)
    assert torch.equal(many.payload['crops'], one.payload['crops']) and torch.equal(many.payload['emb'].view(torch.int32),
                                                                                    one.payload['emb'].view(torch.int32))


def test_nan_only_label_turns_finite_in_a_later_chunk(cuda):
    from deep_insight_face.templates import BestShots
    shots, ref = BestShots(), R.RefShots()
    for labels, key in (([5, 8], [NAN, 1.0]), ([5, 5], [NAN, NAN]), ([5, 8, 5], [-INF, 1.0, -INF]), ([5], [NAN])):
        labels, key = np.asarray(labels, np.int64), np.asarray(key, np.float32)
        pay = np.arange(labels.size * 2, dtype=np.float32).reshape(-1, 2) + 10 * ref.row_base
        shots.add(labels, key, emb=pay)
        ref.add(labels, key, emb=pay)
        check_shots(shots, ref, str(labels))
    assert ref.row.tolist() == [4, 1] and ref.counts.tolist() == [6, 2]


def test_misuse_of_the_handle_fails_and_writes_nothing(cuda):
    from deep_insight_face import _native as N
    h = ctypes.c_void_p()
    N.check(N.lib.dif_pool_create(ctypes.byref(h), 32))
    try:
        i64 = dict(dtype=torch.int64, device=cuda)
        key = torch.tensor([1.0, 2.0, 3.0, 4.0], device=cuda)
        outs = [torch.full((8,), -77, **i64), torch.full((8,), -77.0, device=cuda), torch.full((8,), -77, **i64), torch.full((8,), -77, **i64)]
        call = lambda t: N.lib.dif_pool_best(h, None, None, None, N.ptr(key), 0, t, N.ptr(outs[0]), N.ptr(outs[1]), N.ptr(outs[2]),   # noqa: E731
                                             N.ptr(outs[3]), N.stream_ptr())
        assert call(2) != 0 and 'no dif_pool_group' in N.last_error()
        labels = torch.tensor([4, 9, 4, -1], **i64)
        index, t_dev = torch.empty((4,), **i64), torch.empty((1,), **i64)
        N.check(N.lib.dif_pool_group(h, None, 0, N.ptr(labels), 4, N.ptr(index), N.ptr(t_dev), N.stream_ptr()))
        assert call(5) != 0 and 'disagrees' in N.last_error()          # outside [t0, t0 + n]: refused whatever has run
        assert int(t_dev.item()) == 2
        assert call(3) != 0 and 'disagrees' in N.last_error()          # the group has run: the host knows T
        torch.cuda.synchronize()
        assert all(bool((o == -77).all()) for o in outs)
        N.check(call(2))
        torch.cuda.synchronize()
        assert outs[0][:2].tolist() == [4, 9] and outs[2][:2].tolist() == [2, 1] and outs[3][:2].tolist() == [2, 1]
        assert outs[1][:2].tolist() == [3.0, 2.0] and all(bool((o[2:] == -77).all()) for o in outs)
    finally:
        N.lib.dif_pool_destroy(h)


# ---------------------------------------------------------------------------------------------------- FrameFaces

def hand_made_faces(cuda, with_landmarks=True):
    from deep_insight_face.detector.faces import FrameFaces
    hw = (480, 640)
    lm, bx = landmark_cases(), box_cases(hw)
    m = lm.shape[0]
    rng = np.random.default_rng(21)
    crops = contents(64)[:m]
    emb = rng.standard_normal((m, 64)).astype(np.float32)
    scores = rng.uniform(0.5, 1.0, m).astype(np.float32)
    frame = np.sort(rng.integers(0, 9, m)).astype(np.int64)
    offsets = np.searchsorted(frame, np.arange(10)).astype(np.int64)
    labels = rng.integers(-1, 9, m).astype(np.int64)
    d = lambda a: torch.from_numpy(np.array(a)).to(cuda)                # noqa: E731
    faces = FrameFaces(d(offsets), d(frame), d(bx), d(scores), d(lm) if with_landmarks else None, d(crops), d(emb))
    return faces, labels, hw


@pytest.mark.parametrize('with_landmarks', [True, False])
def test_frame_faces_quality_and_best(cuda, with_landmarks):
    from deep_insight_face.detector.quality import face_quality
    faces, labels, hw = hand_made_faces(cuda, with_landmarks)
    for kw in ({'frame_hw': hw}, {}, {'frame_hw': hw, 'lo': 15, 'hi': 240}):
        q = faces.quality(**kw)
        direct = face_quality(faces.crops, faces.landmarks, faces.boxes if 'frame_hw' in kw else None, kw.get('frame_hw'),
                              kw.get('lo', 0), kw.get('hi', 255))
        assert torch.equal(q.stats, direct.stats) and same(cols_of(q), cols_of(direct))
        st, want = R.face_quality(t2n(faces.crops), None if faces.landmarks is None else t2n(faces.landmarks),
                                  t2n(faces.boxes) if 'frame_hw' in kw else None, kw.get('frame_hw'), kw.get('lo', 0), kw.get('hi', 255))
        check_quality(q, st, want, str(kw))
    lab = torch.from_numpy(labels).to(cuda)
    for kw in ({'frame_hw': hw}, {}):
        score = t2n(faces.quality(**kw).score)
        tl, bk, br, cnt = R.best(labels, score)
        row, got_l, got_k, got_c = faces.best(lab, **kw)
        assert same(t2n(got_l), tl) and same(t2n(row), br) and same(t2n(got_k), bk) and same(t2n(got_c), cnt)
    sharp = faces.quality().sharpness
    tl, bk, br, cnt = R.best(labels, t2n(sharp))
    row, got_l, got_k, got_c = faces.best(lab, key=sharp)
    assert same(t2n(row), br) and same(t2n(got_k), bk) and (br >= 0).all()
    empty = faces._replace(crops=faces.crops[:0], boxes=faces.boxes[:0], landmarks=None, emb=faces.emb[:0])
    assert all(t.shape == (0,) for t in empty.best(lab[:0]))


def test_frame_faces_templates_take_weights(cuda):
    from deep_insight_face.templates import pool_templates
    faces, labels, hw = hand_made_faces(cuda)
    lab = torch.from_numpy(labels).to(cuda)
    q = faces.quality()
    w = q.sharpness                                       # (zero on the flat crops: a template of those alone is NaN on both sides)
    for weights, arg in ((None, False), (faces.scores, True), (w, w)):
        want = pool_templates(faces.emb, lab, weights)[:3]
        got = faces.templates(lab, weighted=arg)
        assert all(same(t2n(a), t2n(b)) for a, b in zip(got, want)), arg is w
    assert all(same(t2n(a), t2n(b)) for a, b in zip(faces.templates(lab), pool_templates(faces.emb, lab, None)[:3]))
    assert not same(t2n(faces.templates(lab, weighted=w)[0]), t2n(faces.templates(lab, weighted=True)[0]))
    with pytest.raises(ValueError):
        faces.templates(lab, weighted=w[:-1])
    with pytest.raises(ValueError):
        faces.templates(lab, weighted=w.double())
