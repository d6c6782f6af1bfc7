"""The two primitives of detection evaluation, on the device (csrc/deteval.hip): the reference's ``detector/utility.py``
``compute_overlap`` (:281-306) and ``compute_ap`` (:309-334), the py-faster-rcnn pair, with its signatures.

NumPy in, NumPy out; a tensor in, a tensor on the device out.  Both compute in float64 as the reference does on float64
arrays; the boxes are float32 on the way in (the detectors' dtype), so ``compute_overlap`` equals the reference on
``boxes.astype(np.float64)`` of float32 boxes bit for bit.  ``deep_insight_face.evaluation.detection`` is their consumer.
There is no CPU fallback: without a HIP device both raise ``DifError``."""
import numpy as np
import torch

from .. import _native as N


def _boxes(x, dev, name):
    t, was_numpy = N.to_device_f32(x, dev)
    if t.dim() != 2 or t.shape[1] != 4:
        raise ValueError('%s: expected boxes [n, 4], got %s' % (name, tuple(t.shape)))
    return t, was_numpy


def compute_overlap(a, b):
    """``a`` [N, 4], ``b`` [K, 4] (x1, y1, x2, y2) -> overlaps [N, K] float64: intersection over union without the
    "+1" of pixel boxes, the union clamped below at ``np.finfo(float).eps`` (``dif_box_overlap``).  Deviation: a pair with
    a coordinate that is not finite has overlap 0, where the reference yields NaN."""
    for name, x in (('a', a), ('b', b)):
        shape = tuple(x.shape) if torch.is_tensor(x) else np.shape(x)
        if len(shape) != 2 or shape[1] != 4:
            raise ValueError('%s: expected boxes [n, 4], got %s' % (name, shape))
    dev = N.require_device()
    ta, was_numpy = _boxes(a, dev, 'a')
    tb, _ = _boxes(b, dev, 'b')
    out = torch.empty((ta.shape[0], tb.shape[0]), dtype=torch.float64, device=dev)
    N.check(N.lib.dif_box_overlap(N.ptr(ta), ta.shape[0], N.ptr(tb), tb.shape[0], N.ptr(out), N.stream_ptr()))
    return out.cpu().numpy() if was_numpy else out


def compute_ap(recall, precision):
    """The average precision of a recall and a precision curve of one length, as py-faster-rcnn computes it
    (``dif_det_ap``): sentinels, the precision envelope, the area under it where the recall changes.  Lists and arrays
    give a NumPy float64 scalar, tensors a 0-d float64 tensor on the device.  The sum runs in a fixed order of its own:
    it is within (number of terms) * 2**-52 of the reference's pairwise sum, and equal curves give equal bits."""
    was_numpy = not torch.is_tensor(recall)
    r = torch.as_tensor(np.asarray(recall, dtype=np.float64)) if was_numpy else recall
    p = precision if torch.is_tensor(precision) else torch.as_tensor(np.asarray(precision, dtype=np.float64))
    if r.dim() != 1 or r.shape != p.shape:
        raise ValueError('recall and precision must be two curves of one length, got %s and %s' % (tuple(r.shape), tuple(p.shape)))
    dev = N.require_device()
    r = r.to(device=dev, dtype=torch.float64).contiguous()
    p = p.to(device=dev, dtype=torch.float64).contiguous()
    out = torch.empty((1,), dtype=torch.float64, device=dev)
    N.check(N.lib.dif_det_ap(N.ptr(r), N.ptr(p), r.shape[0], N.ptr(out), N.stream_ptr()))
    return out.cpu().numpy()[0] if was_numpy else out[0]
