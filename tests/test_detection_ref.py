"""Detector evaluation without a device: tests/detection_ref.py (the NumPy restatement the GPU tests compare with) against
tests/golden/detection.npz -- the reference's own compute_overlap and compute_ap on seeded inputs -- and against outcomes
worked out by hand; the cases it offers make every branch of the rule happen; argument errors; operating_point."""
import functools
import os

import numpy as np
import pytest
import torch

import detection_inputs as I
import detection_ref as R


@pytest.fixture(scope='module')
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'detection.npz'))
    assert str(g['digest']) == I.digest(), 'tests/detection_inputs.py changed: run tests/gen_golden_detection.py again'
    return g


@functools.lru_cache(maxsize=None)
def _results():
    seen = set()
    return {(case['name'], len(thr)): (case, R.evaluate(case, thr, seen)) for case, thr in R.walk()}, seen


def _result(name, j=1):
    return _results()[0][(name, j)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def test_overlap_is_the_references_bit_for_bit(golden):
    a, b = I.overlap_boxes()
    got = R.overlap(a, b)
    assert got.dtype == np.float64 and np.array_equal(bits(got), bits(golden['overlap']))
    # what the inputs were built to hold: copies, touching boxes, the union clamp, an exact half
    assert (got == 1.0).sum() >= 6 and (got == 0.0).any() and ((got > 0) & (got < 1)).sum() > 1000
    assert got[-5, -9] == 0.5                                     # (0, 0, 2, 1) on (0, 0, 1, 1)
    assert got[-4, -8] == 0.0 and got[-4, -7] == 0.0              # an edge and a corner in common
    assert got[-2, -6] == 0.0 and got[-1, -5] == 0.0              # no area at all: 0 / eps


def test_a_coordinate_that_is_not_finite_gives_overlap_zero():
    a = np.array([[0, 0, np.nan, 10], [0, 0, 10, 10], [0, -np.inf, 10, np.inf]], np.float32)
    b = np.array([[0, 0, 10, 10], [0, 0, np.inf, 10]], np.float32)
    assert R.overlap(a, b).tolist() == [[0.0, 0.0], [1.0, 0.0], [0.0, 0.0]]


def test_average_precision_against_the_reference(golden):
    """Both sum the same terms, each in an order of its own: at most n non-zero terms, none negative, that sum to at most 1,
    so either order is within (n - 1) * 2^-53 of the exact sum and the two within n * 2^-52 of each other.  For a detector's
    curve n <= n_truth."""
    curves = I.ap_curves()
    assert len(curves) == len(golden['ap'])
    for (r, p), want in zip(curves, golden['ap']):
        steps = np.count_nonzero(np.diff(np.concatenate([[0.0], r])))
        assert abs(R.average_precision(r, p) - want) <= steps * 2.0 ** -52


def test_the_cases_make_every_branch_happen():
    seen = _results()[1]
    assert not set(R.EVENTS) - seen, sorted(set(R.EVENTS) - seen)
    names = [c['name'] for c in R.cases()]
    assert len(set(names)) == len(names)
    crowd = _result('crowd')[0]
    assert 700 in np.diff(crowd['det_offsets']) and 300 in np.diff(crowd['gt_offsets'])
    seeded = _result('seeded')[0]
    assert len(seeded['det_offsets']) == 38 and np.diff(seeded['det_offsets']).max() <= 40 and np.diff(seeded['gt_offsets']).max() <= 12


def test_outcomes_worked_out_by_hand():
    _, o = _result('second_best_free')
    assert o['assigned'].tolist() == [0, 0] and o['outcome'].tolist() == [[1, 0]]         # never the free second-best truth
    assert 0.5 <= R.overlap([[1, 0, 11, 10]], [[4, 0, 14, 10]])[0, 0] < o['iou'][1]
    _, o = _result('same_truth')
    assert o['outcome'].tolist() == [[0, 1, 0, 1, 0]] and o['assigned'].tolist() == [0, 0, 1, 1, 1]
    _, o = _result('duplicate_truths')
    assert o['assigned'].tolist() == [1, 1, 1] and o['outcome'].tolist() == [[1, 0, 0]]   # the lower of two equal truths, every time
    _, o = _result('at_threshold', 10)
    assert o['iou'].tolist() == [0.5, 0.75] and o['outcome'][0].tolist() == [1, 1]
    assert o['outcome'][:, 0].tolist() == [1] + [0] * 9 and o['outcome'][:, 1].tolist() == [1] * 6 + [0] * 4    # 0.75 is the sixth
    _, o = _result('ignored')
    assert o['outcome'].tolist() == [[2, 2, 1, 0, 2]] and o['n_truth'] == 1
    assert o['tp_cum'].tolist() == [[0, 0, 0, 1, 1]] and o['fp_cum'].tolist() == [[0, 0, 0, 0, 1]] and o['ap'].tolist() == [1.0]
    _, o = _result('all_ignored')
    assert o['n_truth'] == 0 and not o['recall'].any() and o['ap'].tolist() == [0.0] and o['outcome'].tolist() == [[2, 0, 2]]
    _, o = _result('bad_boxes')
    assert o['assigned'].tolist() == [0, 0, 0, 2] and o['iou'].tolist() == [0.0, 1.0, 0.0, 1.0] and o['outcome'].tolist() == [[0, 1, 0, 1]]
    _, o = _result('scores')
    # frame 1: 0.5, NaN, -inf, NaN -> 0.5, -inf, then the NaNs by row; over all rows the three 0.5 of frame 0 come before frame 1's
    assert o['order'].tolist() == [9, 0, 1, 2, 3, 7, 8, 5, 4, 6]
    for name in ('no_detections', 'no_truths', 'nothing'):
        _, o = _result(name)
        assert o['ap'].tolist() == [0.0] and not o['outcome'].any() and (o['assigned'] == -1).all()


def test_chunks_equal_one_call():
    for name in ('crowd', 'seeded', 'scores', 'empties'):
        case, one = _result(name, 10)
        n = len(case['det_offsets']) - 1
        for chunks in [[n], [1, n - 1], [n - 1, 1]] + ([[3, 1, 20, 6, 7], [1] * n] if n == 37 else []):
            got = R.evaluate(case, R.COCO, chunks=chunks)
            for k in one:
                assert np.array_equal(got[k], one[k], equal_nan=True), (name, chunks, k)


def test_sized_cases_hold_exactly_m_rows():
    for m in (R.SCAN_TILE - 1, R.SCAN_TILE, R.SCAN_TILE + 1):
        case = R.sized(m)
        assert len(case['det_scores']) == len(case['det_boxes']) == case['det_offsets'][-1] == m
        assert (np.diff(case['det_offsets']) >= 0).all() and case['gt_offsets'][-1] == len(case['gt_boxes'])


# ---- the public interface without a device ----------------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    from deep_insight_face.detector import utility as U
    from deep_insight_face.evaluation import detection as D
    with pytest.raises(ValueError, match='1 to 16'):
        D.DetectionEvaluator(())
    with pytest.raises(ValueError, match='1 to 16'):
        D.DetectionEvaluator(np.linspace(0.1, 0.9, 17))
    for bad in (0.0, 1.5, -0.5, float('nan')):
        with pytest.raises(ValueError, match=r'\(0, 1\]'):
            D.DetectionEvaluator((0.5, bad))
    assert D.DetectionEvaluator((0.5, 1.0)).iou_thresholds == (0.5, 1.0)
    boxes, scores, off = np.zeros((3, 4), np.float32), np.zeros(3, np.float32), np.array([0, 1, 3])
    gt, goff = np.zeros((2, 4), np.float32), np.array([0, 2, 2])
    ev = D.DetectionEvaluator()
    for args, what in (((boxes[:, :3], scores, off, gt, goff), 'det_boxes'), ((boxes, scores[:2], off, gt, goff), 'det_scores'),
                       ((boxes, scores, off, gt.reshape(-1), goff), 'gt_boxes'), ((boxes, scores, off[:2], gt, goff), 'det_offsets'),
                       ((boxes, scores, off, gt, np.array([0, 1, 1])), 'gt_offsets'), ((boxes, scores, np.array([0, 3, 1, 3]), gt, goff), 'det_offsets'),
                       ((boxes, scores, off.astype(np.float32), gt, goff), 'det_offsets'), ((boxes, scores, off, gt, np.array([0, 1, 2, 2])), 'same frames'),
                       ((boxes, scores, off, gt, goff, np.zeros(3, bool)), 'gt_ignore'), ((boxes, scores, off, gt, goff, np.zeros(2, np.float32)), 'gt_ignore')):
        with pytest.raises(ValueError, match=what):
            ev.add(*args)
    with pytest.raises(ValueError, match=r'boxes \[n, 4\]'):
        U.compute_overlap(np.zeros((2, 3)), np.zeros((2, 4)))
    with pytest.raises(ValueError, match='one length'):
        U.compute_ap([0.1, 0.2], [1.0])
    with pytest.raises(ValueError, match='3, 4|entries'):
        D.evaluate_detector(lambda frames: None, [(None, gt)])


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from deep_insight_face import _native
    from deep_insight_face.detector import utility as U
    from deep_insight_face.evaluation import detection as D
    with pytest.raises(_native.DifError):
        U.compute_overlap(np.zeros((2, 4)), np.zeros((2, 4)))
    with pytest.raises(_native.DifError):
        U.compute_ap([0.5], [1.0])
    with pytest.raises(_native.DifError):
        D.evaluate_detections(np.zeros((1, 4), np.float32), np.zeros(1, np.float32), [0, 1], np.zeros((1, 4), np.float32), [0, 1])


def test_operating_point_is_plain_torch_on_the_curve():
    """Scores 0.9 0.8 0.8 0.6 NaN with outcomes TP FP TP TP FP and 4 truths: precision 1, 1/2, 2/3, 3/4, 3/5.  A threshold keeps
    whole groups of equal scores, so rank 1 (the first 0.8) is no operating point, and the NaN score is none either."""
    from deep_insight_face.evaluation import detection as D
    case = dict(det_scores=np.array([0.8, 0.9, 0.6, np.nan, 0.8], np.float32))
    outcome = np.array([[0, 1, 1, 0, 1]], np.uint8)
    c = R.curve(case['det_scores'], outcome, 4)
    assert c['order'].tolist() == [1, 0, 4, 2, 3] and c['precision'][0].tolist() == [1.0, 0.5, 2 / 3, 0.75, 0.6]
    t = {k: torch.from_numpy(v) for k, v in c.items()}
    res = D.DetectionEval(None, None, torch.from_numpy(outcome), torch.tensor([4]), torch.from_numpy(case['det_scores']), t['order'],
                          t['tp_cum'], t['fp_cum'], t['recall'], t['precision'], t['ap'], (0.5,))
    for min_precision, want in ((0.7, (np.float32(0.6), 0.75, 0.75)), (0.76, (np.float32(0.9), 0.25, 1.0)), (0.5, (np.float32(0.6), 0.75, 0.75))):
        s, r, p = D.operating_point(res, min_precision)
        assert (s.item(), r.item(), p.item()) == want, min_precision
    s, r, p = D.operating_point(res, 1.01)
    assert np.isnan(s.item()) and r.item() == 0.0 and np.isnan(p.item())
    with pytest.raises(ValueError):
        D.operating_point(res, 0.5, j=1)
    empty = D.DetectionEval(*([torch.zeros((0,))] * 4), torch.zeros((0,), dtype=torch.float32), *([torch.zeros((0,))] * 6), (0.5,))
    s, r, p = D.operating_point(empty, 0.5)
    assert np.isnan(s.item()) and r.item() == 0.0
