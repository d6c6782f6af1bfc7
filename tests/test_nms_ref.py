"""tests/nms_ref.py without a GPU: the vectorised float32 suppression the GPU tests compare dif_nms with equals the two
pair-by-pair oracles (oracle.mtcnn.nms_slots, oracle.detector.non_max_suppression) index for index where scores tie and
IoUs sit on the threshold, and gives the known answer on hand-made cases."""
import numpy as np
import pytest

import nms_ref as nr
from oracle import detector as odet
from oracle import mtcnn as om

F = np.float32


def _padded(idx, cap):
    out = np.full(cap, -1, np.int32)
    out[:len(idx)] = idx
    return out


@pytest.mark.parametrize('gh,gw,cap', [(30, 41, 64), (14, 21, 400), (1, 7, 3)])
def test_equals_the_oracles_on_pnet_grids(gh, gw, cap):
    """Integer corners, 17 score levels, half the slots empty: ties everywhere, IoUs of exactly 0.5."""
    rng = np.random.default_rng(gh * 100 + gw)
    boxes = nr.pnet_grid_boxes(gh * gw, gw)
    scores = nr.quantised_scores(rng, gh * gw)
    keep, count = nr.nms_ref(boxes, scores, cap, 0.5, 0.0)
    assert np.array_equal(keep, om.nms_slots(boxes, scores, cap, 0.5))
    alive = np.nonzero(scores >= 0)[0]
    want = alive[odet.non_max_suppression(boxes[alive], scores[alive], cap, F(0.5))]
    assert count == len(want) and np.array_equal(keep, _padded(want, cap))
    if cap == 400:
        assert 0 < count < cap and (keep[count:] == -1).all()    # fewer survivors than slots: -1 padding


def test_equals_the_oracles_on_random_boxes():
    rng = np.random.default_rng(11)
    k = 3000
    boxes = nr.random_boxes(rng, k, extent=300.0)
    scores = (rng.integers(0, 33, k) / F(32)).astype(F)
    scores[rng.random(k) < 0.3] = F(-1)
    for cap, iou in ((64, 0.3), (1, 0.3), (k + 5, 0.5)):
        keep, count = nr.nms_ref(boxes, scores, cap, iou, 0.0)
        assert np.array_equal(keep, om.nms_slots(boxes, scores, cap, iou))
        assert count == int((keep >= 0).sum())
    # float64 IoUs (oracle.detector) order the same picks here: no IoU of these boxes is within a rounding of 0.3
    alive = np.nonzero(scores >= 0)[0]
    want = alive[odet.non_max_suppression(boxes[alive], scores[alive], 64, 0.3)]
    assert np.array_equal(nr.nms_ref(boxes, scores, 64, 0.3, 0.0)[0], _padded(want, 64))


def test_batch_wrapper_is_nms_ref_per_image_and_class():
    rng = np.random.default_rng(5)
    boxes = np.stack([nr.random_boxes(rng, 200, extent=100.0) for _ in range(3)])
    scores = rng.random((3, 200, 2)).astype(F)
    scores[1, :, 1] = F(0.1)                                    # nothing passes the threshold
    keep, count = nr.nms_ref_batch(boxes, scores, 20, 0.3, 0.25)
    assert keep.shape == (3, 2, 20) and count.shape == (3, 2) and keep.dtype == np.int32
    for i in range(3):
        for c in range(2):
            k, m = nr.nms_ref(boxes[i], scores[i, :, c], 20, 0.3, 0.25)
            assert np.array_equal(keep[i, c], k) and count[i, c] == m
    assert count[1, 1] == 0 and (keep[1, 1] == -1).all() and count[0, 0] > 0


def test_hand_made_cases():
    box = [[0, 0, 10, 10], [1, 1, 11, 11], [20, 20, 30, 30], [0, 0, 10, 10]]
    boxes = np.array(box, dtype=F)
    scores = np.array([0.9, 0.8, 0.7, 0.9], dtype=F)
    keep, count = nr.nms_ref(boxes, scores, 10, 0.5)
    assert count == 2 and list(keep) == [0, 2] + [-1] * 8      # 3 ties with 0: the lower index wins and suppresses it
    assert list(nr.nms_ref(boxes[::-1], scores[::-1], 10, 0.5)[0][:3]) == [0, 1, -1]
    assert list(nr.nms_ref(boxes, scores, 1, 0.5)[0]) == [0]
    assert list(nr.nms_ref(boxes[:, [2, 3, 0, 1]], scores, 10, 0.5)[0][:3]) == [0, 2, -1]   # reversed corners
    assert list(nr.nms_ref(boxes[:, [2, 1, 0, 3]], scores, 10, 0.5)[0][:3]) == [0, 2, -1]   # one axis reversed
    # a box without area is picked, suppresses nothing and is never suppressed
    flat = np.array([[0, 0, 10, 10], [5, 0, 5, 10], [0, 0, 10, 10], [5, 0, 5, 10]], dtype=F)
    assert list(nr.nms_ref(flat, np.array([0.5, 0.9, 0.4, 0.3], F), 4, 0.0)[0]) == [1, 0, 3, -1]
    # NaN never takes part, whatever the threshold; neither does -inf
    s = np.array([np.nan, 0.8, 0.7, np.nan], dtype=F)
    for thr in (-np.inf, 0.0, 0.75):
        keep, count = nr.nms_ref(boxes, s, 4, 0.5, thr)
        assert list(keep) == ([1, 2, -1, -1] if thr < 0.75 else [1, -1, -1, -1])
    keep, count = nr.nms_ref(boxes, np.array([-np.inf, -5, np.inf, -np.inf], F), 4, 0.5, -np.inf)
    assert count == 2 and list(keep) == [2, 1, -1, -1]
    assert nr.nms_ref(boxes[:0], scores[:0], 3, 0.5)[1] == 0 and list(nr.nms_ref(boxes[:0], scores[:0], 3, 0.5)[0]) == [-1] * 3
    # score_thr is inclusive
    assert nr.nms_ref(boxes, scores, 4, 0.5, F(0.9))[1] == 1 and nr.nms_ref(boxes, scores, 4, 0.5, 0.95)[1] == 0


def test_iou_exactly_on_the_threshold_survives():
    # [0,0,10,10] and [0,5,10,15]: inter 50, union 150 -> 1/3 in float32 on both sides of the comparison
    boxes = np.array([[0, 0, 10, 10], [0, 5, 10, 15]], dtype=F)
    scores = np.array([0.9, 0.8], dtype=F)
    third = F(50) / F(150)
    assert list(nr.nms_ref(boxes, scores, 2, third)[0]) == [0, 1]
    assert list(nr.nms_ref(boxes, scores, 2, np.nextafter(third, F(0)))[0]) == [0, -1]
    boxes = np.array([[0, 0, 3, 10], [1, 0, 4, 10]], dtype=F)          # inter 2 x 10, union 30 + 30 - 20: 0.5 exactly
    assert list(nr.nms_ref(boxes, scores, 2, 0.5)[0]) == [0, 1]
    assert list(om.nms_slots(boxes, scores, 2, 0.5)) == [0, 1]
    # float corners whose fused union (one rounding fewer) gives a larger IoU than the statement's: the statement decides
    p, q, plain, fused = nr.contraction_pair()
    assert fused > plain
    boxes = np.array([p, q], dtype=F)
    assert list(nr.nms_ref(boxes, scores, 2, plain)[0]) == [0, 1]
    assert list(om.nms_slots(boxes, scores, 2, plain)) == [0, 1]
    assert list(nr.nms_ref(boxes, scores, 2, np.nextafter(plain, F(0)))[0]) == [0, -1]


def test_oracle_detector_drops_minus_inf_and_nan():
    boxes = np.array([[0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50], [60, 60, 70, 70]], dtype=F)
    scores = np.array([-np.inf, 0.5, np.nan, -3.0], dtype=F)
    assert list(odet.non_max_suppression(boxes, scores, 10, 0.5)) == [1, 3]
    assert list(nr.nms_ref(boxes, scores, 10, 0.5)[0][:3]) == [1, 3, -1]
