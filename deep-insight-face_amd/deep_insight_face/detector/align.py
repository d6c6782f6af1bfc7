"""Five-point landmark alignment on the device (csrc/align.hip): landmarks -> similarity transform onto the ArcFace
template -> aligned crop, the preprocessing the public ArcFace-family embedders are trained on.

The reference aligns on the host (``api.py:132-145``, ``create_thumbnail``: ``cv2.getAffineTransform`` on three landmarks
of an external 68-point detector + ``cv2.warpAffine``); here the landmarks are MTCNN's five (``MtcnnDetector.detect(...,
return_landmarks=True)``) and the fit and the warp are one launch.  PARITY WITH ``cv2.warpAffine`` IS UNPINNED: cv2
quantises coordinates to 1/32 pixel and weighs in 15-bit fixed point; what is pinned is the float32 arithmetic
include/dif.h writes out (bilinear, integer pixel indices are sample positions, constant-zero border).
"""
import ctypes

import numpy as np
import torch

from .. import _native as N

# left eye, right eye, nose, left mouth corner, right mouth corner as (x, y) in a 112 x 112 crop: the template of the
# public ArcFace preprocessing
ARCFACE_TEMPLATE_112 = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655],
                                 [70.7299, 92.2041]], dtype=np.float32)


def _tensor(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def _frames(frames):
    t = _tensor(frames)
    if t.dim() != 4 or t.shape[3] != 3 or t.dtype != torch.uint8:
        raise ValueError('expected uint8 frames [N,H,W,3], got %s %s' % (t.dtype, tuple(t.shape)))
    return t


def _floats(x, what):
    t = _tensor(x)
    if not t.dtype.is_floating_point:
        raise ValueError('expected floating-point %s, got %s' % (what, t.dtype))
    return t


def warp_affine(frames, matrices, out_hw, k: int = 1) -> torch.Tensor:
    """Bilinear warp of uint8 frames [N,H,W,3] through ``k`` 2 x 3 matrices per frame ([N*k, 2, 3], [N, k, 2, 3] or
    [N*k, 6]) that map an OUTPUT pixel index (x, y) to a FRAME position -- the inverse of the matrix ``cv2.warpAffine``
    takes by default -> uint8 CUDA tensor [N*k, out_h, out_w, 3]; crop j reads frame j // k.  Outside the frame is zero;
    a matrix holding a NaN gives a black crop."""
    t = _frames(frames)
    m = _floats(matrices, 'matrices')
    k = int(k)
    oh, ow = (int(v) for v in out_hw)
    if k < 1 or oh < 1 or ow < 1:
        raise ValueError('k and the output size must be positive')
    if tuple(m.shape) not in ((t.shape[0] * k, 2, 3), (t.shape[0], k, 2, 3), (t.shape[0] * k, 6)):
        raise ValueError('expected %d x %d matrices of 2 x 3, got %s' % (t.shape[0], k, tuple(m.shape)))
    dev = N.require_device()
    t = t.to(dev).contiguous()
    m = m.to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty((t.shape[0] * k, oh, ow, 3), dtype=torch.uint8, device=dev)
    N.check(N.lib.dif_warp_affine(N.ptr(t), t.shape[0], t.shape[1], t.shape[2], N.ptr(m), k, N.ptr(out), oh, ow, N.stream_ptr()))
    return out


def align_faces(frames, landmarks, size: int = 112, template=None, valid=None, k: int = 1, return_matrices: bool = False):
    """Aligned ``size`` x ``size`` crops: for each of the ``k`` faces per frame the similarity transform (rotation, uniform
    scale, translation) that takes its five landmarks ([N*k, 5, 2] or [N, k, 5, 2], (x, y) in frame pixels: left eye, right
    eye, nose, left and right mouth corner) onto ``template`` ([5, 2] in output pixels; None: ARCFACE_TEMPLATE_112 scaled
    by size / 112) is fitted and the frame warped through its inverse -> uint8 CUDA tensor [N*k, size, size, 3].  ``valid``
    ([N*k] or [N, k]): negative = an empty slot.  An empty slot, a non-finite landmark or five coinciding points give a
    black crop.  ``return_matrices``: also the [N*k, 2, 3] output -> frame matrices used (NaN for a black crop)."""
    t = _frames(frames)
    lm = _floats(landmarks, 'landmarks')
    k, size = int(k), int(size)
    if k < 1 or size < 1:
        raise ValueError('k and size must be positive')
    n = t.shape[0]
    if tuple(lm.shape) not in ((n * k, 5, 2), (n, k, 5, 2)):
        raise ValueError('expected %d x %d landmark sets of 5 x 2, got %s' % (n, k, tuple(lm.shape)))
    tpl = None
    if template is not None:
        tpl = np.ascontiguousarray(np.asarray(template, dtype=np.float32))
        if tpl.shape != (5, 2):
            raise ValueError('expected a template of 5 x 2, got %s' % (tpl.shape,))
    if valid is not None:
        valid = _floats(valid, 'valid')
        if tuple(valid.shape) not in ((n * k,), (n, k)):
            raise ValueError('expected one valid value per face, got %s' % (tuple(valid.shape),))
    dev = N.require_device()
    t = t.to(dev).contiguous()
    lm = lm.to(device=dev, dtype=torch.float32).contiguous()
    if valid is not None:
        valid = valid.to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty((n * k, size, size, 3), dtype=torch.uint8, device=dev)
    mats = torch.empty((n * k, 2, 3), dtype=torch.float32, device=dev) if return_matrices else None
    N.check(N.lib.dif_align_crop(N.ptr(t), n, t.shape[1], t.shape[2], N.ptr(lm), N.ptr(valid) if valid is not None else None, k,
                                 tpl.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if tpl is not None else None, N.ptr(out),
                                 size, N.ptr(mats) if mats is not None else None, N.stream_ptr()))
    return (out, mats) if return_matrices else out
