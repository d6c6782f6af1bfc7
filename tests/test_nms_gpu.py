"""dif_nms called directly, in all four kernel forms, against tests/nms_ref.py -- EXACTLY: nothing here depends on exp, and
box_iou rounds every product before it adds (csrc/detector.hip).  The number of boxes and classes picks the form:
    1 class,  n_boxes <= 11264          nms_reg_kernel<1024, 11, false>   boxes and scores in registers
    1 class,  11265 .. 26624            nms_reg_kernel<1024, 26, true>    scores in LDS (dynamic, behind a function attribute)
    > 1 class, n_boxes <= 12288         nms_kernel<256>                   alive bytes in the workspace
    > 12288 with > 1 class, or > 26624  nms_kernel<1024>
so the sizes below are the smallest that reach each one and sit on both sides of each boundary.  One launch per call, one
block per (image, class).  keep / count / alive_ws are pre-filled and carry a guard row behind their end."""
import numpy as np
import pytest
import torch

import nms_ref as nr

F = np.float32
SENTINEL = -7
# (n_boxes, n_classes) that reach the four forms with every register row / stride pass in use; rows of a thread are
# 1024 boxes apart in the register forms (IPT rows), NT = 256 or 1024 apart in the workspace forms
FORMS = [(11264, 1), (26624, 1), (12288, 2), (12289, 2)]


def run_nms(boxes, scores, cap, iou, thr):
    """boxes [n, K, 4], scores [n, K, C] (NumPy float32) -> keep [n, C, cap], count [n, C] from one dif_nms call; checks the
    return code, the guard rows and that nothing but -1 follows the kept indices."""
    from deep_insight_face import _native as N
    n, k, c = scores.shape
    assert boxes.shape == (n, k, 4) and boxes.dtype == F and scores.dtype == F
    pad = 1 if k == 0 else 0                                     # an empty tensor has no address; nothing of the row is read
    b = torch.from_numpy(np.ascontiguousarray(np.concatenate([boxes, np.zeros((n, pad, 4), F)], 1))).cuda()
    s = torch.from_numpy(np.ascontiguousarray(np.concatenate([scores, np.zeros((n, pad, c), F)], 1))).cuda()
    assert b.data_ptr() % 16 == 0
    row = max(k, 64)
    alive = torch.full((n * c * k + row,), 0xFF, dtype=torch.uint8, device='cuda')
    keep = torch.full((n * c + 1, cap), SENTINEL, dtype=torch.int32, device='cuda')
    count = torch.full((n * c + 1,), SENTINEL, dtype=torch.int32, device='cuda')
    rc = N.lib.dif_nms(N.ptr(b), N.ptr(s), n, k, c, cap, float(thr), float(iou), N.ptr(alive), N.ptr(keep), N.ptr(count),
                       N.stream_ptr())
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    keep, count, alive = keep.cpu().numpy(), count.cpu().numpy(), alive.cpu().numpy()
    assert (keep[-1] == SENTINEL).all() and count[-1] == SENTINEL and (alive[n * c * k:] == 0xFF).all(), 'guard row written'
    return keep[:-1].reshape(n, c, cap), count[:-1].reshape(n, c)


def check(boxes, scores, cap, iou, thr, label=''):
    want_keep, want_count = nr.nms_ref_batch(boxes, scores, cap, iou, thr)
    keep, count = run_nms(boxes, scores, cap, iou, thr)
    assert np.array_equal(count, want_count), (label, count, want_count)
    bad = np.argwhere(keep != want_keep)
    assert len(bad) == 0, (label, 'first difference at (image, class, pick)', bad[0], keep[tuple(bad[0])], want_keep[tuple(bad[0])])
    return want_keep, want_count


def grid_problem(k, n, c, seed):
    """(a) P-Net-style integer corners, 17 score levels, half the slots at -1; score_thr 0, IoU 0.5.  Every image has a
    grid of its own width, moved by whole pixels, so a wrong image stride on the boxes reads another image's geometry."""
    rng = np.random.default_rng(seed)
    gw = max(1, int(round(np.sqrt(k * 187 / 139))))            # the 139 x 187 grid's aspect, gh != gw
    boxes = np.stack([nr.pnet_grid_boxes(k, gw + 3 * i) + F(7 * i) for i in range(n)])
    assert k == 0 or n == 1 or not np.array_equal(boxes[0], boxes[1])
    scores = np.stack([nr.quantised_scores(rng, k * c).reshape(k, c) for _ in range(n)])
    return boxes, scores, 0.5, 0.0


def float_problem(k, n, c, seed):
    """(b) float boxes, reversed corners and boxes without area among them, continuous scores; score_thr 0.25, IoU 0.3."""
    rng = np.random.default_rng(seed)
    boxes = np.stack([nr.random_boxes(rng, k) for _ in range(n)])
    scores = rng.random((n, k, c)).astype(F)
    return boxes, scores, 0.3, 0.25


PROBLEMS = {'grid': grid_problem, 'float': float_problem}


def empty_one(scores, image, cls, kind):
    scores[image, :, cls] = F(-1) if kind == 'grid' else scores[image, :, cls] * F(0.2)     # all below the threshold


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['grid', 'float'])
@pytest.mark.parametrize('k', [0, 1, 63, 64, 65, 1023, 1024, 1025, 11263, 11264, 11265, 26623, 26624, 26625])
def test_form_boundaries_one_class(cuda, k, kind):
    boxes, scores, iou, thr = PROBLEMS[kind](k, 3, 1, seed=k + 1)
    empty_one(scores, 1, 0, kind)
    keep, count = check(boxes, scores, 64, iou, thr)
    assert count[1, 0] == 0 and (keep[1] == -1).all()
    if k >= 1023:
        assert count[0, 0] == 64 and count[2, 0] == 64          # the cap is reached: every pick is a full scan


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['grid', 'float'])
@pytest.mark.parametrize('k', [1025, 12288, 12289])
def test_form_boundaries_two_classes(cuda, k, kind):
    boxes, scores, iou, thr = PROBLEMS[kind](k, 3, 2, seed=k + 2)
    empty_one(scores, 2, 0, kind)
    keep, count = check(boxes, scores, 64, iou, thr)
    assert count[2, 0] == 0 and (keep[2, 0] == -1).all() and count[2, 1] == 64 and count[0, 0] == 64
    assert not np.array_equal(keep[0, 0], keep[0, 1])           # the classes' columns differ: a class stride slip shows


def _columns(scores, c):
    """[n, K] -> [n, K, c]: class 0 holds the scores; a second class holds them reversed along the boxes."""
    return np.ascontiguousarray(np.stack([scores, scores[:, ::-1]][:c], -1))


@pytest.mark.gpu
@pytest.mark.parametrize('k,c', FORMS)
def test_maximum_at_either_end_and_one_tied_list(cuda, k, c):
    rng = np.random.default_rng(k + c)
    boxes = np.stack([nr.random_boxes(rng, k) for _ in range(3)])
    s = (rng.random((3, k)) * 0.9).astype(F)
    s[0, k - 1] = F(2)                                           # the unique maximum in the last register row's last thread
    s[1, 0] = F(2)                                               # ... and in the first thread's first row
    s[2, :] = F(0.5)                                             # one tied list: the picks are the ascending survivors
    keep, count = check(boxes, _columns(s, c), 64, 0.3, 0.25)
    assert keep[0, 0, 0] == k - 1 and keep[1, 0, 0] == 0
    assert (np.diff(keep[2, 0]) > 0).all() and keep[2, 0, 0] == 0
    if c == 2:                                                   # class 1 sees the list reversed
        assert keep[0, 1, 0] == 0 and keep[1, 1, 0] == k - 1 and (np.diff(keep[2, 1]) > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('k,c', FORMS)
def test_tied_maxima_across_waves_and_rows(cuda, k, c):
    """Two equal maxima d boxes apart: d = 64 (the next wave, same row), 256 and 1024 (the same thread's next row in the
    workspace / register forms), 1024 (IPT - 1) (first against last row); the same box twice, so only the lower index is
    kept, and disjoint boxes, so both are kept in index order."""
    dists = [64, 256, 1024, 1024 * (k // 1024 - 1)]            # 1024 (IPT - 1) in the register forms
    rng = np.random.default_rng(k * 3 + c)
    n = 2 * len(dists)
    boxes = np.stack([nr.random_boxes(rng, k, flat_frac=0.0) for _ in range(n)])
    s = (rng.random((n, k)) * 0.9).astype(F)
    firsts = []
    for i in range(n):
        d = dists[i // 2]
        a = 37 + 64 * (i % 3)
        assert a + d < k
        s[i, a] = s[i, a + d] = F(1.5)
        boxes[i, a] = [10, 10, 50, 50]
        boxes[i, a + d] = [10, 10, 50, 50] if i % 2 == 0 else [500, 500, 540, 540]
        firsts.append((a, a + d))
    keep, count = check(boxes, _columns(s, c), 64, 0.3, 0.25)
    for i, (a, b) in enumerate(firsts):
        assert keep[i, 0, 0] == a and (keep[i, 0, 1] == b) == (i % 2 == 1)
        assert (b in keep[i, 0]) == (i % 2 == 1)


def clustered_problem(k, n, c, seed, centres=12):
    """Boxes jittered around a few centres: fewer survivors than 64 at IoU 0.3."""
    rng = np.random.default_rng(seed)
    mid = rng.uniform(0, 2000, (centres, 2))[rng.integers(0, centres, (n, k))]
    mid = mid + rng.uniform(-3, 3, (n, k, 2))
    half = rng.uniform(28, 32, (n, k, 2))
    boxes = np.concatenate([mid - half, mid + half], -1).astype(F)
    return boxes, rng.random((n, k, c)).astype(F)


@pytest.mark.gpu
@pytest.mark.parametrize('k,c', [(65, 1), (1025, 1), (11265, 1), (1025, 2), (12289, 2), (26625, 1)])
def test_caps(cuda, k, c):
    """Cap 1; cap 64 with fewer survivors (-1 padding and the count); a cap above n_boxes."""
    boxes, scores = clustered_problem(k, 2, c, seed=k + 7 * c)
    keep1, _ = check(boxes, scores, 1, 0.3, 0.25, 'cap 1')
    keep64, count64 = check(boxes, scores, 64, 0.3, 0.25, 'cap 64')
    assert (count64 > 1).all() and (count64 < 64).all()
    assert np.array_equal(keep64[:, :, :1], keep1)
    big, count = check(boxes, scores, k + 3, 0.3, 0.25, 'cap > n_boxes')
    assert np.array_equal(count, count64) and np.array_equal(big[:, :, :64], keep64) and (big[:, :, 64:] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize('k,c', FORMS)
def test_nan_and_infinite_scores(cuda, k, c):
    """NaN scores and NaN corners scattered through the list, several +inf scores (tied: index order), -inf scores under
    score_thr = -inf (yolov3.non_max_suppression's default): NaN and -inf never take part, in any form."""
    rng = np.random.default_rng(k + 11 * c)
    boxes = np.stack([nr.random_boxes(rng, k) for _ in range(2)])
    s = rng.random((2, k)).astype(F)
    r = rng.random((2, k))
    s[r < 0.2] = np.nan
    s[(r >= 0.2) & (r < 0.4)] = -np.inf
    s[:, [5, k // 2, k - 1]] = np.inf
    s[0, 0] = np.nan
    s[0, k - 2] = -np.inf
    nanbox = rng.random((2, k, 4)) < 0.02
    boxes[nanbox] = np.nan
    boxes[1, 5] = [0, 0, 40, 40]
    boxes[1, k - 1] = [0, 0, 40, 40]                             # +inf twice on one box: only index 5 is kept
    scores = _columns(s, c)
    for thr in (-np.inf, 0.5):
        keep, count = check(boxes, scores, 64, 0.3, thr, thr)
        assert keep[0, 0, 0] == 5 and keep[1, 0, 0] == 5 and (k - 1) not in keep[1, 0]
        for i in range(2):
            picked = s[i][keep[i, 0][keep[i, 0] >= 0]]
            assert not np.isnan(picked).any() and not (picked == -np.inf).any()
    # nothing but NaN and -inf: no survivor, all -1
    s2 = np.where(rng.random((2, k)) < 0.5, F(np.nan), F(-np.inf)).astype(F)
    keep, count = check(boxes, _columns(s2, c), 8, 0.3, -np.inf, 'all dead')
    assert (count == 0).all() and (keep == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize('k,c', FORMS + [(300, 1), (300, 2)])
def test_iou_exactly_on_the_threshold_survives(cuda, k, c):
    """Float corners whose IoU equals the threshold in the float32 statement and exceeds it when the union's subtraction
    is fused with the intersection's product: the second box survives.  One ulp lower, it is suppressed."""
    p, q, plain, fused = nr.contraction_pair()
    assert fused > plain
    boxes = np.zeros((2, k, 4), F)
    boxes[:] = [3000, 3000, 3010, 3010]
    s = np.full((2, k), -1, F)
    for i, (a, b) in enumerate([(0, k - 1), (k - 1, k // 2)]):
        boxes[i, a], boxes[i, b] = p, q
        s[i, a], s[i, b] = 0.9, 0.8
    scores = np.ascontiguousarray(np.stack([s] * c, -1))
    keep, count = check(boxes, scores, 4, plain, 0.0, 'on the threshold')
    assert (count == 2).all() and list(keep[0, 0]) == [0, k - 1, -1, -1] and list(keep[1, c - 1]) == [k - 1, k // 2, -1, -1]
    keep, count = check(boxes, scores, 4, np.nextafter(plain, F(0)), 0.0, 'one ulp below')
    assert (count == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize('k', [11264, 26624])
@pytest.mark.parametrize('kind', ['grid', 'float'])
def test_forms_agree(cuda, k, kind):
    """The one-class problem again as two classes with the score column duplicated (nms_kernel<256> / <1024>)."""
    boxes, scores, iou, thr = PROBLEMS[kind](k, 2, 1, seed=k + 3)
    keep1, count1 = check(boxes, scores, 64, iou, thr)
    two = np.ascontiguousarray(np.repeat(scores, 2, axis=2))
    keep2, count2 = run_nms(boxes, two, 64, iou, thr)
    for cls in range(2):
        assert np.array_equal(keep2[:, cls], keep1[:, 0]) and np.array_equal(count2[:, cls], count1[:, 0])


@pytest.mark.gpu
def test_same_call_twice(cuda):
    """The LDS form sets its function attribute once per device: the second call must find it set."""
    boxes, scores, iou, thr = grid_problem(26624, 2, 1, seed=99)
    first = run_nms(boxes, scores, 64, iou, thr)
    second = run_nms(boxes, scores, 64, iou, thr)
    want = nr.nms_ref_batch(boxes, scores, 64, iou, thr)
    for got in (first, second):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
