"""Redaction (csrc/redact.hip): the faces of a batch of frames filled, pixelated or smoothed in the frames, on the device.

The video path returns numbers; a deployment that must hand on a frame stream with every face hidden -- or every face that
is NOT on a watch-list -- gets the frames back from here without taking them off the device::

    faces = pipeline.faces(frames)
    out = faces.redact(frames, select=faces.dist > tol)          # everyone the gallery does not know, pixelated

``include/dif.h`` ("redaction") writes the rule out -- the region of a box, the cell grid, the rounded cell means, the
ellipse, the integer bilinear interpolation of 'smooth', and which face a pixel under several belongs to -- and
``tests/redact_ref.py`` restates it in NumPy, bit for bit.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from .. import _native as N

MODES = {'fill': 0, 'pixelate': 1, 'smooth': 2}
SHAPES = {'box': 0, 'ellipse': 1}
MAX_CELLS, MAX_SIDE = 64, 8192                   # DIF_REDACT_MAX_CELLS, DIF_REDACT_MAX_SIDE


def _tensor(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def redact_frames(frames, offsets, boxes, select=None, mode: str = 'pixelate', cells: int = 8, min_cell: int = 4,
                  margin: float = 0.0, shape: str = 'box', fill=(0, 0, 0), out=None, workspace=None):
    """``dif_frames_redact``: ``frames`` uint8 [N, H, W, 3] (1 <= H, W <= 8192), ``offsets`` int64 [N + 1] and ``boxes``
    [M, 4] (left, top, right, bottom) as ``FrameFaces`` holds them -> ``out``, a uint8 CUDA tensor [N, H, W, 3]:
    ``frames.clone()`` unless given, with the covered pixels of the selected faces replaced and every other byte left as
    it was.  ``out`` may be ``frames`` itself (in place: the same bytes as out of place), but not a tensor that overlaps it
    in part.

    ``select`` [M] bool or uint8, ``None`` = every face; ``mode`` 'fill', 'pixelate' or 'smooth'; ``shape`` 'box' or
    'ellipse'; ``cells`` in [1, 64] cells along the longer side of a region, none smaller than ``min_cell`` pixels;
    ``margin`` grows (or, negative, shrinks) the box by that share of its size on every side; ``fill`` three bytes.
    ``workspace``: a uint8 CUDA tensor of at least ``dif_frames_redact_workspace_size(M, cells)`` bytes to use instead of a
    fresh one.  ``M == 0`` or ``N == 0`` launches nothing.  Nothing is read back; argument errors are ``ValueError``."""
    t = _tensor(frames)
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError('frames must be uint8 [N, H, W, 3], got %s %s' % (t.dtype, tuple(t.shape)))
    n, h, w = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError('H and W must lie in [1, %d], got %d and %d' % (MAX_SIDE, h, w))
    off, bx = _tensor(offsets), _tensor(boxes)
    if off.dim() != 1 or off.shape[0] != n + 1 or off.dtype.is_floating_point:
        raise ValueError('offsets must be integers [%d], got %s %s' % (n + 1, off.dtype, tuple(off.shape)))
    if bx.dim() != 2 or bx.shape[1] != 4 or not bx.dtype.is_floating_point:
        raise ValueError('boxes must be floating point [M, 4], got %s %s' % (bx.dtype, tuple(bx.shape)))
    m = int(bx.shape[0])
    sel = None
    if select is not None:
        sel = _tensor(select)
        if sel.dtype not in (torch.bool, torch.uint8) or tuple(sel.shape) != (m,):
            raise ValueError('select must be bool or uint8 [%d], got %s %s' % (m, sel.dtype, tuple(sel.shape)))
    if mode not in MODES:
        raise ValueError('mode must be one of %s, got %r' % (sorted(MODES), mode))
    if shape not in SHAPES:
        raise ValueError('shape must be one of %s, got %r' % (sorted(SHAPES), shape))
    cells, min_cell, margin = int(cells), int(min_cell), float(margin)
    if not 1 <= cells <= MAX_CELLS:
        raise ValueError('cells must lie in [1, %d], got %d' % (MAX_CELLS, cells))
    if not 1 <= min_cell <= MAX_SIDE:
        raise ValueError('min_cell must lie in [1, %d], got %d' % (MAX_SIDE, min_cell))
    if not abs(margin) <= float(np.finfo(np.float32).max):
        raise ValueError('margin must be a finite float32, got %r' % margin)
    fill = tuple(int(v) for v in fill)
    if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
        raise ValueError('fill must be three bytes, got %r' % (fill,))
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or out.shape != t.shape or not out.is_contiguous():
            raise ValueError('out must be a contiguous uint8 tensor %s' % (tuple(t.shape),))
        if out.device != t.device or (m and n and not out.is_cuda):
            raise ValueError('out must be on the device of frames, a HIP device; got %s and %s' % (out.device, t.device))
    if workspace is not None and (not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.dim() != 1
                                  or not workspace.is_contiguous()):
        raise ValueError('workspace must be a contiguous uint8 tensor [bytes]')
    if m == 0 or n == 0:
        return t.clone() if out is None else out
    dev = t.device if t.is_cuda else N.require_device()
    src = t.to(dev).contiguous()
    if out is None:
        out = src.clone()
    off = off.to(device=dev, dtype=torch.int64).contiguous()
    bx = bx.to(device=dev, dtype=torch.float32).contiguous()
    if sel is not None:
        sel = sel.to(dev).contiguous()
        if sel.dtype == torch.bool:
            sel = sel.view(torch.uint8)              # True is stored as 1
    need = N.lib.dif_frames_redact_workspace_size(m, cells)
    if need < 0:
        raise ValueError('%d faces with %d cells are more than one call takes' % (m, cells))
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif workspace.device != dev:
        raise ValueError('workspace must be on %s, got %s' % (dev, workspace.device))
    with torch.cuda.device(dev):
        N.check(N.lib.dif_frames_redact(N.ptr(src), n, h, w, N.ptr(off), N.ptr(bx), m, N.ptr(sel) if sel is not None else None,
                                        MODES[mode], SHAPES[shape], cells, min_cell, margin, (ctypes.c_uint8 * 3)(*fill), N.ptr(out),
                                        N.ptr(workspace), workspace.shape[0], N.stream_ptr()))
    return out
