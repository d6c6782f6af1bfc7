"""Face quality (csrc/quality.hip): per-face image and pose measures from the crops, landmarks and boxes the video path
already holds on the device.

A detector's score says "this is a face", not "this is a good face".  ``face_quality`` measures every crop once -- its
brightness, contrast, sharpness (the variance of a 4-neighbour Laplacian over the interior) and clipped share -- and, from
the five landmarks and the box, the eye distance, the roll, a yaw and a nose-drop proxy and the share of the box inside
the frame; ``include/dif.h`` ("face quality") writes every column out and ``tests/quality_ref.py`` restates them in NumPy,
bit for bit.  ``score`` combines them without parameters; it is a convention that nobody has measured against recognition
accuracy.  There are no default thresholds either: ``FaceQuality.mask`` applies the bounds it is given, and ::

    q = faces.quality(frame_hw=(H, W))
    labels = torch.where(q.mask(min_eye_dist=20, max_abs_yaw=0.5), labels, -1)

keeps a bad face out of ``TemplatePool.add``, ``FrameFaces.templates`` and ``templates.BestShots`` alike: all of them leave
a negative label out.  ``FrameFaces.templates(labels, weighted=q.score)`` weighs by quality instead, and ``FrameFaces.best``
picks the one best face of every label.
"""
import typing

import numpy as np
import torch

from .. import _native as N

QUALITY_COLS = 10                                # DIF_QUALITY_COLS
MIN_SIZE, MAX_SIZE = 3, 256


class FaceQuality(typing.NamedTuple):
    """``face_quality``: ``stats`` [M, 6] int64 (sum g, sum g*g, sum L, sum L*L, #{g <= lo}, #{g >= hi}) and ten [M] float32
    columns, views of one [M, 10] tensor; on the device, or NumPy arrays for NumPy input."""
    stats: typing.Any
    brightness: typing.Any                       # mean gray / 255
    contrast: typing.Any                         # standard deviation of gray / 255
    sharpness: typing.Any                        # variance of the Laplacian over the interior pixels
    clipped: typing.Any                          # share of pixels with g <= lo or g >= hi
    eye_dist: typing.Any                         # frame pixels between the eyes; NaN without landmarks, as the next three
    roll: typing.Any                             # sine of the in-plane angle of the eye line
    yaw: typing.Any                              # 0: the nose projects onto the middle of the eye line, +-1: onto an eye
    nose_drop: typing.Any                        # the nose on the way from the eye midpoint (0) to the mouth midpoint (1)
    inside: typing.Any                           # share of the box inside the frame; NaN without boxes
    score: typing.Any                            # sharpness * (1 - clipped) * max(0, 1 - |yaw|) * inside

    def mask(self, min_sharpness=None, min_eye_dist=None, max_abs_yaw=None, max_abs_roll=None, min_inside=None,
             max_clipped=None, min_score=None):
        """-> bool [M]: the faces that meet every bound given.  A bound that is None is not applied (no bound: all true); a
        NaN fails any bound that is applied, so ``min_eye_dist`` without landmarks fails every face.  Plain comparisons,
        on the device for device tensors.  ``labels = torch.where(mask, labels, -1)`` then leaves the other faces out of
        ``TemplatePool``, ``FrameFaces.templates`` and ``BestShots``."""
        is_np = not torch.is_tensor(self.score)
        ab = np.abs if is_np else torch.abs
        keep = np.ones(self.score.shape, dtype=bool) if is_np else torch.ones_like(self.score, dtype=torch.bool)
        for col, low, high in ((self.sharpness, min_sharpness, None), (self.eye_dist, min_eye_dist, None),
                               (ab(self.yaw), None, max_abs_yaw), (ab(self.roll), None, max_abs_roll),
                               (self.inside, min_inside, None), (self.clipped, None, max_clipped),
                               (self.score, min_score, None)):
            if low is not None:
                keep = keep & (col >= low)               # (a comparison with NaN is false)
            if high is not None:
                keep = keep & (col <= high)
        return keep


def _floats(x, name, shape):
    if x is None:
        return None
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if not t.dtype.is_floating_point or tuple(t.shape) != shape:
        raise ValueError('%s must be floating point %s, got %s %s' % (name, list(shape), t.dtype, tuple(t.shape)))
    return t


def face_quality(crops, landmarks=None, boxes=None, frame_hw=None, lo: int = 0, hi: int = 255) -> FaceQuality:
    """``dif_face_quality``: ``crops`` uint8 [M, S, S, 3] (3 <= S <= 256; RGB or BGR: gray is symmetric in the two),
    optionally ``landmarks`` [M, 5, 2] (left eye, right eye, nose, mouth corners; frame pixels) and ``boxes`` [M, 4] (left,
    top, right, bottom) with ``frame_hw`` = (H, W) -> ``FaceQuality``.  A pixel is dark when g <= ``lo`` and bright when
    g >= ``hi``.  A view that is not contiguous is copied first.  NumPy in -> NumPy out; ``M == 0`` gives empty tensors and
    launches nothing; nothing is read back."""
    was_np = not torch.is_tensor(crops)
    c = torch.from_numpy(np.ascontiguousarray(crops)) if was_np else crops
    if c.dtype != torch.uint8 or c.dim() != 4 or c.shape[3] != 3 or c.shape[1] != c.shape[2]:
        raise ValueError('crops must be uint8 [M, S, S, 3], got %s %s' % (c.dtype, tuple(c.shape)))
    m, size = int(c.shape[0]), int(c.shape[1])
    if not MIN_SIZE <= size <= MAX_SIZE:
        raise ValueError('the crop size must lie in [%d, %d], got %d' % (MIN_SIZE, MAX_SIZE, size))
    lo, hi = int(lo), int(hi)
    if not (0 <= lo <= 255 and 0 <= hi <= 255):
        raise ValueError('lo and hi must lie in [0, 255], got %d and %d' % (lo, hi))
    if boxes is not None and frame_hw is None:
        raise ValueError('boxes need frame_hw = (H, W), the frame they are measured against')
    fh, fw = (float(frame_hw[0]), float(frame_hw[1])) if boxes is not None else (0.0, 0.0)
    lm = _floats(landmarks, 'landmarks', (m, 5, 2))
    bx = _floats(boxes, 'boxes', (m, 4))
    dev = c.device if c.is_cuda else N.require_device()
    c = c.to(dev).contiguous()
    if lm is not None:
        lm = lm.to(device=dev, dtype=torch.float32).contiguous()
    if bx is not None:
        bx = bx.to(device=dev, dtype=torch.float32).contiguous()
    stats = torch.empty((m, 6), dtype=torch.int64, device=dev)
    cols = torch.empty((m, QUALITY_COLS), dtype=torch.float32, device=dev)
    if m:
        with torch.cuda.device(dev):
            N.check(N.lib.dif_face_quality(N.ptr(c), m, size, N.ptr(lm) if lm is not None else None, N.ptr(bx) if bx is not None else None,
                                           fh, fw, lo, hi, N.ptr(stats), N.ptr(cols), N.stream_ptr()))
    if was_np:
        stats, cols = stats.cpu().numpy(), cols.cpu().numpy()
    return FaceQuality(stats, *(cols[:, i] for i in range(QUALITY_COLS)))
