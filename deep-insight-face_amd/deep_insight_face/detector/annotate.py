"""Annotation (csrc/annotate.hip): a box round every face of a batch of frames, the name the gallery gave it on a plate next
to the box and a square on every landmark, painted into the frames on the device.

What an operator is shown is the frame with its faces marked; everything the picture needs -- offsets, boxes, landmarks,
gallery rows, distances, track labels -- is on the device already, and a name table sits next to the gallery::

    table = NameTable(['ann', 'bob', ...])                        # once, next to the gallery
    faces = pipeline.faces(frames)
    out = faces.annotate(frames, names=table, known=faces.dist <= tol, values=faces.dist, colors=palette(tracks.labels))

``include/dif.h`` ("annotation") writes both rules out -- how a label is composed, and which pixels a face paints: ring,
plate, glyphs, marks, and which face a pixel under several belongs to -- and ``tests/annotate_ref.py`` restates them in
NumPy, bit for bit.  The reference draws with OpenCV on the host (``detector/utility.py:203-252``); parity with
``cv2.rectangle`` / ``cv2.putText`` is unpinned.  There is no CPU fallback.
"""
import ctypes
import functools

import numpy as np
import torch

from .. import _native as N

MAX_TEXT, MAX_THICKNESS, MAX_SCALE, MAX_MARK, MAX_SIDE = 64, 64, 8, 16, 8192       # DIF_ANNOTATE_MAX_*, DIF_REDACT_MAX_SIDE
DEFAULT_COLOR = (0, 255, 0)
# sixteen colours for labels % 16, then the grey of a negative label
PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
           (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195),
           (128, 128, 128))


def _tensor(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def _flags(x, m, what):
    """bool or uint8 [m] -> the tensor (bool still); ValueError otherwise."""
    t = _tensor(x)
    if t.dtype not in (torch.bool, torch.uint8) or tuple(t.shape) != (m,):
        raise ValueError('%s must be bool or uint8 [%d], got %s %s' % (what, m, t.dtype, tuple(t.shape)))
    return t


def _bytes_on(t, dev):
    t = t.to(dev).contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t       # True is stored as 1


class NameTable:
    """The names of the gallery rows, encoded once and kept on the device: ``names`` uint8 [G, length], NUL-padded.  ASCII;
    any other character becomes ``?``; a name longer than ``length`` is cut."""

    def __init__(self, names, length: int = 24, device=None):
        length = int(length)
        if length < 1:
            raise ValueError('length must be at least 1, got %d' % length)
        host = np.zeros((len(names), length), np.uint8)
        for row, name in enumerate(names):
            raw = str(name).encode('ascii', 'replace')[:length]
            host[row, :len(raw)] = np.frombuffer(raw, np.uint8)
        self.length = length
        self.names = torch.from_numpy(host).to(N.require_device() if device is None else device)

    def __len__(self):
        return self.names.shape[0]


def compose_text(names=None, idx=None, known=None, values=None, decimals: int = 2, unknown: str = '?', length: int = 32):
    """``dif_annotate_compose``: the label of every face -> uint8 [M, length] on the device, NUL-padded.  ``names`` a
    ``NameTable`` (or uint8 [G, Ln]) and ``idx`` [M] the gallery row of each face: the label starts with ``names[idx]`` where
    ``known`` [M] (bool or uint8, ``None`` = everywhere) holds and ``idx`` is a row of the table, and with ``unknown``
    elsewhere.  ``values`` float [M]: a space and the value with ``decimals`` digits after the point follow.  M is taken from
    ``idx``, ``known`` or ``values``, at least one of which must be given.  ``M == 0`` launches nothing.  Nothing is read
    back; argument errors are ``ValueError``."""
    given = [(k, _tensor(v)) for k, v in (('idx', idx), ('known', known), ('values', values)) if v is not None]
    if not given:
        raise ValueError('one of idx, known and values must be given: they tell the number of faces')
    if given[0][1].dim() != 1:
        raise ValueError('%s must have one dimension, got %s' % (given[0][0], tuple(given[0][1].shape)))
    m = int(given[0][1].shape[0])
    decimals, length = int(decimals), int(length)
    if not 0 <= decimals <= 4:
        raise ValueError('decimals must lie in [0, 4], got %d' % decimals)
    if not 1 <= length <= MAX_TEXT:
        raise ValueError('length must lie in [1, %d], got %d' % (MAX_TEXT, length))
    if not isinstance(unknown, str):
        raise ValueError('unknown must be a str, got %r' % (unknown,))
    unknown = unknown.encode('ascii', 'replace')
    if len(unknown) > MAX_TEXT or b'\0' in unknown:
        raise ValueError('unknown must be at most %d bytes without a NUL' % MAX_TEXT)
    table = names.names if isinstance(names, NameTable) else names
    if table is not None:
        table = _tensor(table)
        if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] < 1:
            raise ValueError('names must be a NameTable or uint8 [G, Ln], got %s %s' % (table.dtype, tuple(table.shape)))
    if idx is not None:
        idx = _tensor(idx)
        if idx.dtype.is_floating_point or idx.dtype == torch.bool or tuple(idx.shape) != (m,):
            raise ValueError('idx must be integers [%d], got %s %s' % (m, idx.dtype, tuple(idx.shape)))
    if known is not None:
        known = _flags(known, m, 'known')
    if values is not None:
        values = _tensor(values)
        if not values.dtype.is_floating_point or tuple(values.shape) != (m,):
            raise ValueError('values must be floating point [%d], got %s %s' % (m, values.dtype, tuple(values.shape)))
    tensors = [t for t in (idx, known, values, table) if t is not None]
    dev = next((t.device for t in tensors if t.is_cuda), None)
    if m == 0:
        return torch.zeros((0, length), dtype=torch.uint8, device=dev or 'cpu')
    if dev is None:
        dev = N.require_device()
    text = torch.empty((m, length), dtype=torch.uint8, device=dev)
    if table is not None:
        table = table.to(dev).contiguous()
    if idx is not None:
        idx = idx.to(device=dev, dtype=torch.int64).contiguous()
    if known is not None:
        known = _bytes_on(known, dev)
    if values is not None:
        values = values.to(device=dev, dtype=torch.float32).contiguous()
    opt = lambda t: N.ptr(t) if t is not None else None
    with torch.cuda.device(dev):
        N.check(N.lib.dif_annotate_compose(opt(table), table.shape[0] if table is not None else 0, table.shape[1] if table is not None else 1,
                                           opt(idx), opt(known), opt(values), decimals, unknown, m, N.ptr(text), length, N.stream_ptr()))
    return text


def annotate_frames(frames, offsets, boxes, landmarks=None, text=None, colors=None, select=None, margin: float = 0.0,
                    thickness: int = 2, scale: int = 2, mark: int = 1, out=None):
    """``dif_frames_annotate``: ``frames`` uint8 [N, H, W, 3] (1 <= H, W <= 8192), ``offsets`` int64 [N + 1] and ``boxes``
    [M, 4] (left, top, right, bottom) as ``FrameFaces`` holds them -> ``out``, a uint8 CUDA tensor [N, H, W, 3]:
    ``frames.clone()`` unless given, with a ring of ``thickness`` pixels round every selected face (the box grown by
    ``margin`` of its size, as in ``redact_frames``), a plate with ``text`` uint8 [M, L] (``compose_text``; L <= 64, an
    empty row has no plate) at ``scale`` pixels per font pixel above it, and a square of radius ``mark`` on each of
    ``landmarks`` [M, 5, 2] (``mark=-1``: none).  Every other byte is left as it was.  ``out=frames`` paints in place; any
    other ``out`` is painted as it is -- the paint is opaque and reads no pixel.

    ``colors``: uint8 [M, 3] per face (``palette``), three bytes for every face, or ``None`` = green; the text is black or
    white, whichever stands out.  ``select`` [M] bool or uint8, ``None`` = every face.  Where faces overlap, the lowest row
    (the best face) is on top.  ``M == 0`` or ``N == 0`` launches nothing.  Nothing is read back; argument errors are
    ``ValueError``."""
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
    lm = None
    if landmarks is not None:
        lm = _tensor(landmarks)
        if not lm.dtype.is_floating_point or tuple(lm.shape) != (m, 5, 2):
            raise ValueError('landmarks must be floating point [%d, 5, 2], got %s %s' % (m, lm.dtype, tuple(lm.shape)))
    txt = None
    if text is not None:
        txt = _tensor(text)
        if txt.dtype != torch.uint8 or txt.dim() != 2 or txt.shape[0] != m or not 1 <= txt.shape[1] <= MAX_TEXT:
            raise ValueError('text must be uint8 [%d, L] with L in [1, %d], got %s %s' % (m, MAX_TEXT, txt.dtype, tuple(txt.shape)))
    color, col = DEFAULT_COLOR, None
    if torch.is_tensor(colors) or isinstance(colors, np.ndarray):
        col = _tensor(colors)
        if col.dtype != torch.uint8 or tuple(col.shape) != (m, 3):
            raise ValueError('colors must be uint8 [%d, 3] or three bytes, got %s %s' % (m, col.dtype, tuple(col.shape)))
    elif colors is not None:
        color = tuple(int(v) for v in colors)
        if len(color) != 3 or not all(0 <= v <= 255 for v in color):
            raise ValueError('colors must be uint8 [%d, 3] or three bytes, got %r' % (m, colors))
    sel = None if select is None else _flags(select, m, 'select')
    margin, thickness, scale, mark = float(margin), int(thickness), int(scale), int(mark)
    if not abs(margin) <= float(np.finfo(np.float32).max):
        raise ValueError('margin must be a finite float32, got %r' % margin)
    if not 0 <= thickness <= MAX_THICKNESS:
        raise ValueError('thickness must lie in [0, %d], got %d' % (MAX_THICKNESS, thickness))
    if not 1 <= scale <= MAX_SCALE:
        raise ValueError('scale must lie in [1, %d], got %d' % (MAX_SCALE, scale))
    if not -1 <= mark <= MAX_MARK:
        raise ValueError('mark must lie in [-1, %d], got %d' % (MAX_MARK, mark))
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or out.shape != t.shape or not out.is_contiguous():
            raise ValueError('out must be a contiguous uint8 tensor %s' % (tuple(t.shape),))
        if out.device != t.device or (m and n and not out.is_cuda):
            raise ValueError('out must be on the device of frames, a HIP device; got %s and %s' % (out.device, t.device))
    if m == 0 or n == 0:
        return t.clone() if out is None else out
    dev = t.device if t.is_cuda else N.require_device()
    if out is None:
        out = t.to(dev).clone(memory_format=torch.contiguous_format)
    off = off.to(device=dev, dtype=torch.int64).contiguous()
    bx = bx.to(device=dev, dtype=torch.float32).contiguous()
    if lm is not None:
        lm = lm.to(device=dev, dtype=torch.float32).contiguous()
    if txt is not None:
        txt = txt.to(dev).contiguous()
    if col is not None:
        col = col.to(dev).contiguous()
    if sel is not None:
        sel = _bytes_on(sel, dev)
    opt = lambda x: N.ptr(x) if x is not None else None
    with torch.cuda.device(dev):
        N.check(N.lib.dif_frames_annotate(N.ptr(out), n, h, w, N.ptr(off), N.ptr(bx), m, opt(lm), opt(txt), txt.shape[1] if txt is not None else 1,
                                          opt(col), (ctypes.c_uint8 * 3)(*color), opt(sel), margin, thickness, scale, mark, N.stream_ptr()))
    return out


@functools.lru_cache(maxsize=None)
def _palette_on(device):
    return torch.tensor(PALETTE, dtype=torch.uint8, device=device)


def palette(labels):
    """A colour per label -> uint8 [M, 3] on the labels' device: sixteen fixed colours by ``labels % 16``, grey for a negative
    label (noise, no track).  For track, cluster or gallery labels; torch indexing, no kernel.  The table is uploaded once
    per device, so from the second call on nothing crosses to the device."""
    labels = _tensor(labels)
    if labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError('labels must be integers [M], got %s %s' % (labels.dtype, tuple(labels.shape)))
    labels = labels.to(torch.int64)
    return _palette_on(labels.device)[torch.where(labels < 0, 16, labels % 16)]
