"""Detector evaluation on the GPU (csrc/deteval.hip through deep_insight_face.evaluation.detection, detector.utility and
FrameFaces.evaluate) against tests/detection_ref.py, the sequential NumPy restatement, and tests/golden/detection.npz, the
reference's own compute_overlap / compute_ap.

Standards: assigned, iou, outcome, n_truth, order, tp_cum, fp_cum, recall and precision equal the restatement bit for bit.
ap lies within n_truth * 2^-52 of compute_ap -- the restatement's, which tests/test_detection_ref.py holds against the
reference's -- applied to the device's OWN curve: both sum the same at most n_truth non-zero terms, none negative and at most
1 in all, each in a fixed order of its own, so each is within (n_truth - 1) * 2^-53 of the exact sum.  A second call gives
the same bits."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import detection_inputs as I
import detection_ref as R

pytestmark = pytest.mark.gpu

CASES = [c['name'] for c in R.cases()]
FIELDS = ('assigned', 'iou', 'outcome', 'n_truth', 'order', 'tp_cum', 'fp_cum', 'recall', 'precision')


@functools.lru_cache(maxsize=None)
def _cases():
    return {c['name']: c for c in R.cases()}


@functools.lru_cache(maxsize=None)
def _want(name, thr):
    case = _cases()[name] if name in _cases() else _sized(int(name.split('_')[1]))
    return R.evaluate(case, thr)


@functools.lru_cache(maxsize=None)
def _sized(m):
    return R.sized(m)


@pytest.fixture(scope='module')
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'detection.npz'))
    assert str(g['digest']) == I.digest()
    return g


def _dev(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _args(case, dev):
    return [_dev(case[k], dev) for k in ('det_boxes', 'det_scores', 'det_offsets', 'gt_boxes', 'gt_offsets')]


def _evaluate(case, thr, dev):
    from deep_insight_face.evaluation import detection as D
    return D.evaluate_detections(*_args(case, dev), iou_thresholds=thr, gt_ignore=_dev(case['gt_ignore'], dev))


def _np(res):
    out = {k: getattr(res, k).cpu().numpy() for k in FIELDS + ('ap', 'scores')}
    assert all(getattr(res, k).is_cuda for k in FIELDS + ('ap', 'scores'))
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(res, want, what):
    got = _np(res)
    m, j = len(want['assigned']), len(want['ap'])
    assert got['outcome'].shape == (j, m) and got['recall'].shape == (j, m) and got['ap'].shape == (j,), what
    for k in FIELDS:
        w = np.asarray(want[k]).reshape(got[k].shape)
        assert _same_bits(got[k], w.astype(got[k].dtype) if k in ('n_truth', 'outcome') else w), (what, k)
    bound = want['n_truth'] * 2.0 ** -52
    for q in range(j):
        ref = R.average_precision(got['recall'][q], got['precision'][q])
        print('%s thr %d: ap %.17g, compute_ap of the curve %.17g, difference %.3g, bound %.3g' % (what, q, got['ap'][q], ref,
                                                                                                      abs(got['ap'][q] - ref), bound))
        assert abs(got['ap'][q] - ref) <= bound, (what, q)
    return got


@pytest.mark.parametrize('thr', [(0.5,), R.COCO], ids=['J1', 'J10'])
@pytest.mark.parametrize('name', CASES)
def test_cases(cuda, name, thr):
    """Every case of detection_ref.cases() -- frames without detections, truths or both, M = 0, T = 0, several detections on
    one truth, the free second-best truth, duplicate truths, IoU at the threshold, equal, NaN and -inf scores, boxes that are
    not finite, ignored truths, the crowd frame of 300 truths and 700 detections, 37 seeded frames -- at J = 1 and J = 10,
    twice: the second call has the bits of the first."""
    case = _cases()[name]
    first = _check(_evaluate(case, thr, cuda), _want(name, thr), name)
    again = _np(_evaluate(case, thr, cuda))
    for k in FIELDS + ('ap',):
        assert _same_bits(first[k], again[k]), (name, k)


@pytest.mark.parametrize('m', [R.SCAN_TILE - 1, R.SCAN_TILE, R.SCAN_TILE + 1, 70001])
def test_scan_sizes(cuda, m):
    """M one below, at and one above the scan tile, and 70 001 rows: 69 tiles, so the wave that scans the tiles' counts (and
    the one that carries the envelope) holds two tiles per lane, and the radix sort runs 35 blocks."""
    from deep_insight_face import _native as N
    thr = (0.5, 0.75)
    res = _evaluate(_sized(m), thr, cuda)
    got = _check(res, _want('sized_%d' % m, thr), m)
    again = _np(_evaluate(_sized(m), thr, cuda))
    assert _same_bits(got['ap'], again['ap']) and _same_bits(got['order'], again['order'])
    # dif_det_ap -- one block that walks the tiles -- on the device's curve has the bits of dif_det_curve's ap
    out = torch.empty((1,), dtype=torch.float64, device=cuda)
    for q in range(len(thr)):
        N.check(N.lib.dif_det_ap(N.ptr(res.recall[q]), N.ptr(res.precision[q]), m, N.ptr(out), N.stream_ptr()))
        assert _same_bits(out.cpu().numpy(), got['ap'][q:q + 1])


def _sort_const(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'deep-insight-face_amd', 'csrc', 'radix_sort.hip')).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, src).group(1))


SORT_SHARE = _sort_const('kSortItems') * 64                                # keys of a tile that one wave ranks, 64 per round
SORT_TILE = _sort_const('kSortThreads') * _sort_const('kSortItems')        # keys per block of the radix sort


@pytest.mark.parametrize('m', [SORT_SHARE - 1, SORT_SHARE, SORT_SHARE + 1, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1])
def test_sort_sizes(cuda, m):
    """M one below, at and one above a wave's share of the sort's tile and the tile itself (csrc/radix_sort.hip, 32-bit keys):
    the last key alone in the next wave's counters, and alone in the next block.  The order is stable only if equal scores keep
    their rows' order across every hand-off of the ranking -- a wave's rounds of 64, the waves' shares, the blocks' tiles -- so
    the input must hold equal scores on both sides of each hand-off that M reaches; that is asserted before the device is asked."""
    case, thr = _sized(m), (0.5, 0.75)
    scores = case['det_scores']
    assert len(scores) == m
    for unit in (64, SORT_SHARE, SORT_TILE):
        if m > unit:
            part = np.arange(m) // unit
            assert any(len(np.unique(part[scores == v])) > 1 for v in np.unique(scores)), (m, unit, 'no equal scores across this hand-off')
    got = _check(_evaluate(case, thr, cuda), _want('sized_%d' % m, thr), m)
    again = _np(_evaluate(case, thr, cuda))
    for k in FIELDS + ('ap',):
        assert _same_bits(got[k], again[k]), (m, k)


@pytest.mark.parametrize('name,chunks', [('seeded', [37]), ('seeded', [30, 7]), ('seeded', [3, 1, 20, 6, 7]), ('crowd', [2, 2]),
                                         ('crowd', [1, 1, 1, 1]), ('empties', [1, 2, 1, 1]), ('scores', [1, 2])])
def test_evaluator_in_chunks_equals_one_call(cuda, name, chunks):
    from deep_insight_face.evaluation import detection as D
    case = _cases()[name]
    ev = D.DetectionEvaluator(R.COCO)
    f0 = 0
    for c in chunks:
        b = R.batch(case, f0, f0 + c)
        ev.add(*_args(b, cuda), gt_ignore=_dev(b['gt_ignore'], cuda))
        f0 += c
    assert f0 == len(case['det_offsets']) - 1
    got = _check(ev.result(), _want(name, R.COCO), (name, chunks))
    one = _np(_evaluate(case, R.COCO, cuda))
    for k in FIELDS + ('ap',):
        assert _same_bits(got[k], one[k]), (name, chunks, k)


def test_an_evaluator_that_was_given_nothing(cuda):
    from deep_insight_face.evaluation import detection as D
    res = D.DetectionEvaluator((0.5, 0.75)).result()
    assert res.ap.tolist() == [0.0, 0.0] and res.n_truth.tolist() == [0] and res.outcome.shape == (2, 0) and res.order.shape == (0,)


def test_nothing_is_read_back(cuda):
    """With the inputs on the device, matching, accumulating and taking the curves synchronise nowhere on the torch side (the
    library itself has no call that could: it enqueues launches and one memset)."""
    from deep_insight_face.evaluation import detection as D
    case = _cases()['seeded']
    a, b = R.batch(case, 0, 20), R.batch(case, 20, 37)
    args = [(_args(x, cuda), _dev(x['gt_ignore'], cuda)) for x in (a, b)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        ev = D.DetectionEvaluator(R.COCO)
        for x, ign in args:
            ev.add(*x, gt_ignore=ign)
        res = ev.result()
        point = D.operating_point(res, 0.9, j=3)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    _check(res, _want('seeded', R.COCO), 'seeded, no host read')
    assert all(p.is_cuda for p in point)


def test_box_overlap_and_compute_ap_on_the_fixture(cuda, golden):
    from deep_insight_face.detector import utility as U
    a, b = I.overlap_boxes()
    got = U.compute_overlap(a, b)
    assert isinstance(got, np.ndarray) and _same_bits(got, golden['overlap'])
    dev = U.compute_overlap(_dev(a, cuda), _dev(b, cuda))
    assert dev.is_cuda and dev.dtype == torch.float64 and _same_bits(dev.cpu().numpy(), golden['overlap'])
    assert U.compute_overlap(a[:0], b).shape == (0, len(b)) and U.compute_overlap(a, b[:0]).shape == (len(a), 0)
    bad = U.compute_overlap(np.array([[0, 0, np.nan, 10], [0, 0, 10, 10]], np.float32), np.array([[0, 0, 10, 10], [0, 0, np.inf, 10]], np.float32))
    assert bad.tolist() == [[0.0, 0.0], [1.0, 0.0]]
    for (r, p), want in zip(I.ap_curves(), golden['ap']):
        steps = np.count_nonzero(np.diff(np.concatenate([[0.0], r])))
        ap = U.compute_ap(r, p)
        print('compute_ap on %d points: %.17g, the reference %.17g, bound %.3g' % (len(r), ap, want, steps * 2.0 ** -52))
        assert isinstance(ap, np.float64) and abs(ap - want) <= steps * 2.0 ** -52
        t = U.compute_ap(_dev(r, cuda), _dev(p, cuda))
        assert t.is_cuda and t.dim() == 0 and _same_bits(np.float64(t.item()), ap)
    assert U.compute_ap(list(I.ap_curves()[2][0]), list(I.ap_curves()[2][1])) == U.compute_ap(*I.ap_curves()[2])


def test_frame_faces_evaluate(cuda):
    from deep_insight_face.detector.faces import FrameFaces
    case = _cases()['seeded']
    boxes, scores, off = _dev(case['det_boxes'], cuda), _dev(case['det_scores'], cuda), _dev(case['det_offsets'], cuda)
    m = boxes.shape[0]
    frame = _dev(np.repeat(np.arange(len(case['det_offsets']) - 1), np.diff(case['det_offsets'])), cuda)
    faces = FrameFaces(off, frame, boxes, scores, None, torch.zeros((m, 1, 1, 3), dtype=torch.uint8, device=cuda))
    got = _check(faces.evaluate(_dev(case['gt_boxes'], cuda), _dev(case['gt_offsets'], cuda), R.COCO, _dev(case['gt_ignore'], cuda)),
                 _want('seeded', R.COCO), 'FrameFaces.evaluate')
    one = _np(_evaluate(case, R.COCO, cuda))
    assert all(_same_bits(got[k], one[k]) for k in FIELDS + ('ap',))
    # no faces at all, and no truths at all
    empty = FrameFaces(torch.zeros((3,), dtype=torch.int64, device=cuda), frame[:0], boxes[:0], scores[:0], None,
                       torch.zeros((0, 1, 1, 3), dtype=torch.uint8, device=cuda))
    res = empty.evaluate(np.array([[0, 0, 5, 5]], np.float32), np.array([0, 1, 1]))
    assert res.ap.tolist() == [0.0] and res.n_truth.tolist() == [1] and res.order.shape == (0,)
    res = faces.evaluate(np.zeros((0, 4), np.float32), np.zeros(len(case['det_offsets']), np.int64))
    assert res.ap.tolist() == [0.0] and res.n_truth.tolist() == [0] and (res.assigned == -1).all() and not res.outcome.any()
    assert res.fp_cum[0, -1].item() == m


def test_evaluate_detector_drives_a_pipeline(cuda):
    """faces_fn stands for a pipeline's .faces: it hands out the case's detections frame batch by frame batch."""
    import collections
    from deep_insight_face.evaluation import detection as D
    case = _cases()['seeded']
    Faces = collections.namedtuple('Faces', 'boxes scores offsets')
    spans = [(0, 10), (10, 11), (11, 37)]

    def faces_fn(frames):
        b = R.batch(case, *frames)
        return Faces(_dev(b['det_boxes'], cuda), _dev(b['det_scores'], cuda), _dev(b['det_offsets'], cuda))

    def batches(with_ignore):
        for s in spans:
            b = R.batch(case, *s)
            yield (s, b['gt_boxes'], b['gt_offsets']) + ((b['gt_ignore'],) if with_ignore else ())

    _check(D.evaluate_detector(faces_fn, batches(True), R.COCO), _want('seeded', R.COCO), 'evaluate_detector')
    plain = dict(case, gt_ignore=None)
    _check(D.evaluate_detector(faces_fn, batches(False)), R.evaluate(plain, (0.5,)), 'evaluate_detector, no ignore flags')


def test_operating_point_on_the_device_curve(cuda):
    from deep_insight_face.evaluation import detection as D
    res = _evaluate(_cases()['seeded'], R.COCO, cuda)
    host = D.DetectionEval(*(x.cpu() if torch.is_tensor(x) else x for x in res))
    for j, min_precision in ((0, 0.5), (0, 0.9), (4, 0.75), (9, 0.999), (9, 2.0)):
        got, want = D.operating_point(res, min_precision, j), D.operating_point(host, min_precision, j)
        assert all(g.is_cuda for g in got)
        assert all(_same_bits(g.cpu().numpy(), w.numpy()) for g, w in zip(got, want)), (j, min_precision)
    s, r, p = (x.item() for x in D.operating_point(res, 0.9))
    assert p >= 0.9 and 0 < r <= 1 and 0 <= s <= 1


def test_the_library_refuses_bad_arguments_before_any_launch(cuda):
    from deep_insight_face import _native as N
    one = (ctypes.c_double * 1)(0.5)
    x = torch.zeros((64,), dtype=torch.float64, device=cuda)
    for thr, j, m, ws, what in (((ctypes.c_double * 1)(0.0), 1, 1, 1 << 20, 'threshold'), ((ctypes.c_double * 1)(1.5), 1, 1, 1 << 20, 'threshold'),
                                ((ctypes.c_double * 1)(float('nan')), 1, 1, 1 << 20, 'threshold'), (one, 0, 1, 1 << 20, 'thresholds'),
                                (one, 17, 1, 1 << 20, 'thresholds'), (one, 1, -1, 1 << 20, 'sizes'), (one, 1, 1, 8, 'workspace')):
        rc = N.lib.dif_det_match(N.ptr(x), N.ptr(x), N.ptr(x), m, N.ptr(x), N.ptr(x), None, 1, 1, thr, j, N.ptr(x), N.ptr(x), N.ptr(x), N.ptr(x),
                                 N.ptr(x), ws, N.stream_ptr())
        assert rc != 0 and what in N.last_error(), (what, N.last_error())
    assert N.lib.dif_det_match(None, None, None, 1, None, None, None, 0, 0, one, 1, None, None, None, N.ptr(x), None, 0, N.stream_ptr()) != 0
    assert 'no frame' in N.last_error()
    assert N.lib.dif_det_workspace_size(-1, 0, 1) < 0 and N.lib.dif_det_workspace_size(0, 0, 17) < 0
    assert N.lib.dif_det_workspace_size(0, 0, 1) == 0 and N.lib.dif_det_workspace_size(1, 1, 1) > 0
    assert N.lib.dif_det_curve(N.ptr(x), N.ptr(x), N.ptr(x), 4, 1, N.ptr(x), N.ptr(x), N.ptr(x), N.ptr(x), N.ptr(x), N.ptr(x), N.ptr(x), 8,
                               N.stream_ptr()) != 0 and 'workspace' in N.last_error()
    assert N.lib.dif_det_ap(None, None, 3, N.ptr(x), N.stream_ptr()) != 0 and N.lib.dif_box_overlap(None, 2, None, 2, N.ptr(x), N.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert not x.any()                                                     # nothing was launched
