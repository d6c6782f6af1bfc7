"""Detector evaluation on the device (csrc/deteval.hip; include/dif.h, "detector evaluation", writes the rule out): the
detections of a detector matched to labelled boxes, and the precision / recall curve and the average precision over all
of them, at up to 16 IoU thresholds at once.

The rule is that of the consumers of the reference's ``detector/utility.py`` ``compute_overlap`` / ``compute_ap``
(keras-retinanet / keras-yolo3 ``evaluate``) with Pascal VOC's "difficult" flags: a detection's ONE candidate is the
truth of its frame it overlaps most (float64 IoU, first maximum); by descending score, the first detection that reaches
the threshold on a truth is its true positive, every later one a false positive, and a hit on an ignored truth counts as
neither.  Everything is exact and independent of the launch order, chunks of whole frames give the bits of one call, and
nothing is read back to the host.  Parity with the WIDER FACE devkit's own protocol is unpinned.

Detections and truths are CSR lists over the frames: ``offsets`` [N + 1] int64 (``FrameFaces.offsets``), boxes [M, 4]
left, top, right, bottom, scores [M].  NumPy arrays and tensors on any device are taken; results are tensors on the
device."""
import ctypes
import typing

import numpy as np
import torch

from .. import _native as N

MAX_THRESHOLDS = 16                              # DIF_DET_MAX_THRESHOLDS
FP, TP, DROPPED = 0, 1, 2                        # DIF_DET_FP, DIF_DET_TP, DIF_DET_DROPPED
COCO_THRESHOLDS = tuple(np.linspace(0.5, 0.95, 10))


class DetectionEval(typing.NamedTuple):
    """Per detection (rows in the order they were given, batches concatenated), per rank (``order``), per threshold."""
    assigned: torch.Tensor                       # [M] int64: the truth (row of all truths given) it overlaps most, -1: none
    iou: torch.Tensor                            # [M] float64: that overlap, 0 without one
    outcome: torch.Tensor                        # [J, M] uint8: FP, TP or DROPPED
    n_truth: torch.Tensor                        # [1] int64: truths that are not ignored
    scores: torch.Tensor                         # [M] float32
    order: torch.Tensor                          # [M] int64: rows by descending score, ties to the lower row, NaN last
    tp_cum: torch.Tensor                         # [J, M] int64, in that order
    fp_cum: torch.Tensor                         # [J, M] int64
    recall: torch.Tensor                         # [J, M] float64
    precision: torch.Tensor                      # [J, M] float64
    ap: torch.Tensor                             # [J] float64
    iou_thresholds: typing.Tuple[float, ...]     # on the host


def _thresholds(iou_thresholds):
    thr = tuple(float(v) for v in np.asarray(iou_thresholds, dtype=np.float64).reshape(-1))
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError('expected 1 to %d IoU thresholds, got %d' % (MAX_THRESHOLDS, len(thr)))
    for v in thr:
        if not 0.0 < v <= 1.0:
            raise ValueError('an IoU threshold must lie in (0, 1], got %r' % (v,))
    return thr


def _tensor(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def _check_csr(offsets, rows, name):
    off = _tensor(offsets)
    if off.dim() != 1 or off.shape[0] < 1 or off.dtype.is_floating_point or off.dtype == torch.bool:
        raise ValueError('%s_offsets: expected integers [N + 1], got %s %s' % (name, off.dtype, tuple(off.shape)))
    if not off.is_cuda:                          # (on the host the contents cost nothing to check; on the device nothing is read back)
        o = off.to(torch.int64)
        if int(o[0]) != 0 or int(o[-1]) != rows or bool((o[1:] < o[:-1]).any()):
            raise ValueError('%s_offsets must ascend from 0 to the %d rows of %s_boxes' % (name, rows, name))
    return off


def _check_batch(det_boxes, det_scores, det_offsets, gt_boxes, gt_offsets, gt_ignore):
    db, ds, gb = _tensor(det_boxes), _tensor(det_scores), _tensor(gt_boxes)
    if db.dim() != 2 or db.shape[1] != 4 or not db.dtype.is_floating_point:
        raise ValueError('det_boxes: expected floating-point boxes [M, 4], got %s %s' % (db.dtype, tuple(db.shape)))
    if tuple(ds.shape) != (db.shape[0],) or not ds.dtype.is_floating_point:
        raise ValueError('det_scores: expected floating-point scores [%d], got %s %s' % (db.shape[0], ds.dtype, tuple(ds.shape)))
    if gb.dim() != 2 or gb.shape[1] != 4 or not gb.dtype.is_floating_point:
        raise ValueError('gt_boxes: expected floating-point boxes [T, 4], got %s %s' % (gb.dtype, tuple(gb.shape)))
    do, go = _check_csr(det_offsets, db.shape[0], 'det'), _check_csr(gt_offsets, gb.shape[0], 'gt')
    if do.shape != go.shape:
        raise ValueError('det_offsets and gt_offsets must cover the same frames, got %d and %d entries' % (do.shape[0], go.shape[0]))
    gi = None
    if gt_ignore is not None:
        gi = _tensor(gt_ignore)
        if tuple(gi.shape) != (gb.shape[0],) or gi.dtype not in (torch.bool, torch.uint8):
            raise ValueError('gt_ignore: expected bool or uint8 [%d], got %s %s' % (gb.shape[0], gi.dtype, tuple(gi.shape)))
    return db, ds, do, gb, go, gi


class DetectionEvaluator:
    """Accumulates batches of whole frames: ``add`` matches a batch (``dif_det_match``) and keeps its scores and outcomes
    on the device, ``result`` ranks everything kept and takes the curves (``dif_det_curve``).  Chunks of any sizes give the
    bits of one call; between detections of equal score the one given earlier ranks first."""

    def __init__(self, iou_thresholds=(0.5,)):
        self.iou_thresholds = _thresholds(iou_thresholds)
        self._thr = (ctypes.c_double * len(self.iou_thresholds))(*self.iou_thresholds)
        self._parts = []                         # (assigned, iou, outcome, scores) per batch
        self._n_truth = None
        self._truths = 0                         # truths given so far: the row of the next batch's truth 0

    def add(self, det_boxes, det_scores, det_offsets, gt_boxes, gt_offsets, gt_ignore=None):
        """One batch of N whole frames -> (assigned [M] int64, iou [M] float64, outcome [J, M] uint8) of this batch, which is
        final: no later batch changes it."""
        db, ds, do, gb, go, gi = _check_batch(det_boxes, det_scores, det_offsets, gt_boxes, gt_offsets, gt_ignore)
        dev = N.require_device()
        db = db.to(device=dev, dtype=torch.float32).contiguous()
        ds = ds.to(device=dev, dtype=torch.float32).contiguous()
        gb = gb.to(device=dev, dtype=torch.float32).contiguous()
        do = do.to(device=dev, dtype=torch.int64).contiguous()
        go = go.to(device=dev, dtype=torch.int64).contiguous()
        if gi is not None:
            gi = gi.to(device=dev, dtype=torch.uint8).contiguous()
        m, t, n, j = db.shape[0], gb.shape[0], do.shape[0] - 1, len(self.iou_thresholds)
        assigned = torch.empty((m,), dtype=torch.int32, device=dev)
        iou = torch.empty((m,), dtype=torch.float64, device=dev)
        outcome = torch.empty((j, m), dtype=torch.uint8, device=dev)
        n_truth = torch.empty((1,), dtype=torch.int64, device=dev)
        size = N.lib.dif_det_workspace_size(m, t, j)
        if size < 0:
            raise N.DifError(N.last_error())
        work = torch.empty((size,), dtype=torch.uint8, device=dev)
        N.check(N.lib.dif_det_match(N.ptr(do), N.ptr(db), N.ptr(ds), m, N.ptr(go), N.ptr(gb), N.ptr(gi) if gi is not None else None, t, n,
                                    self._thr, j, N.ptr(assigned), N.ptr(iou), N.ptr(outcome), N.ptr(n_truth), N.ptr(work), size,
                                    N.stream_ptr()))
        assigned = assigned.to(torch.int64)
        if self._truths:
            assigned = torch.where(assigned >= 0, assigned + self._truths, assigned)
        self._parts.append((assigned, iou, outcome, ds))
        self._n_truth = n_truth if self._n_truth is None else self._n_truth + n_truth
        self._truths += t
        return assigned, iou, outcome

    def result(self) -> DetectionEval:
        dev = N.require_device()
        j = len(self.iou_thresholds)
        if self._parts:
            assigned, iou, outcome, scores = (torch.cat([p[i] for p in self._parts], dim=-1).contiguous() for i in range(4))
            n_truth = self._n_truth
        else:
            assigned = torch.empty((0,), dtype=torch.int64, device=dev)
            iou = torch.empty((0,), dtype=torch.float64, device=dev)
            outcome = torch.empty((j, 0), dtype=torch.uint8, device=dev)
            scores = torch.empty((0,), dtype=torch.float32, device=dev)
            n_truth = torch.zeros((1,), dtype=torch.int64, device=dev)
        m = scores.shape[0]
        order = torch.empty((m,), dtype=torch.int64, device=dev)
        tp_cum, fp_cum = (torch.empty((j, m), dtype=torch.int64, device=dev) for _ in range(2))
        recall, precision = (torch.empty((j, m), dtype=torch.float64, device=dev) for _ in range(2))
        ap = torch.empty((j,), dtype=torch.float64, device=dev)
        size = N.lib.dif_det_workspace_size(m, 0, j)
        if size < 0:
            raise N.DifError(N.last_error())
        work = torch.empty((size,), dtype=torch.uint8, device=dev)
        N.check(N.lib.dif_det_curve(N.ptr(scores), N.ptr(outcome), N.ptr(n_truth), m, j, N.ptr(order), N.ptr(tp_cum), N.ptr(fp_cum),
                                    N.ptr(recall), N.ptr(precision), N.ptr(ap), N.ptr(work), size, N.stream_ptr()))
        return DetectionEval(assigned, iou, outcome, n_truth, scores, order, tp_cum, fp_cum, recall, precision, ap, self.iou_thresholds)


def evaluate_detections(det_boxes, det_scores, det_offsets, gt_boxes, gt_offsets, iou_thresholds=(0.5,), gt_ignore=None) -> DetectionEval:
    """All frames in one call: ``DetectionEvaluator(iou_thresholds)`` with one ``add``."""
    ev = DetectionEvaluator(iou_thresholds)
    ev.add(det_boxes, det_scores, det_offsets, gt_boxes, gt_offsets, gt_ignore)
    return ev.result()


def evaluate_detector(faces_fn, batches, iou_thresholds=(0.5,)) -> DetectionEval:
    """Drives a pipeline over labelled frames: ``faces_fn(frames)`` -> a ``FrameFaces`` (``FramePipeline.faces``,
    ``MtcnnFramePipeline.faces``), ``batches`` an iterable of ``(frames, gt_boxes, gt_offsets)`` or ``(frames, gt_boxes,
    gt_offsets, gt_ignore)`` with the truths of the batch's frames as a CSR list."""
    ev = DetectionEvaluator(iou_thresholds)
    for batch in batches:
        if len(batch) not in (3, 4):
            raise ValueError('a batch is (frames, gt_boxes, gt_offsets[, gt_ignore]), got %d entries' % len(batch))
        faces = faces_fn(batch[0])
        ev.add(faces.boxes, faces.scores, faces.offsets, batch[1], batch[2], batch[3] if len(batch) == 4 else None)
    return ev.result()


def operating_point(result: DetectionEval, min_precision, j: int = 0):
    """The lowest score threshold at which the detector still holds ``min_precision`` at IoU threshold ``j`` ->
    (score, recall, precision), three 0-d tensors on the device.  Keeping the detections with a score >= s ends the curve at
    the LAST rank that carries s, so only those ranks are candidates (and none with a NaN score); among the candidates whose
    precision is >= ``min_precision`` the one furthest down the order wins.  None holds it: (NaN, 0, NaN).  Plain torch on the
    device curve; nothing is read back."""
    if not 0 <= int(j) < len(result.iou_thresholds):
        raise ValueError('j must lie in [0, %d), got %d' % (len(result.iou_thresholds), j))
    dev = result.scores.device
    nan = torch.full((), float('nan'), dtype=torch.float64, device=dev)
    if result.scores.shape[0] == 0:
        return nan.to(torch.float32), torch.zeros((), dtype=torch.float64, device=dev), nan
    s = result.scores[result.order]
    last = torch.ones_like(s, dtype=torch.bool)
    last[:-1] = s[:-1] != s[1:]                  # (a NaN differs from everything: the mask below takes it out)
    p, r = result.precision[j], result.recall[j]
    ok = last & ~torch.isnan(s) & (p >= float(min_precision))
    at = torch.where(ok, torch.arange(s.shape[0], device=dev), torch.full((), -1, dtype=torch.int64, device=dev)).max()
    found, k = at >= 0, at.clamp(min=0).reshape(1)

    def pick(x):                                 # (x[k] with a 0-d tensor k would read k back to index on the host)
        return x.index_select(0, k).reshape(())

    return (torch.where(found, pick(s), nan.to(torch.float32)), torch.where(found, pick(r), torch.zeros_like(nan)),
            torch.where(found, pick(p), nan))
