"""Every face in a frame (csrc/faces.hip): the detectors' fixed slots -> one dense list of faces -> crops, on the device.

Both detectors fill ``k`` slots per frame (score -1 = an empty slot, best slot first).  ``gather_faces`` compacts the
slots of a batch into the list of faces that are there -- frame-major, inside a frame in the detector's pick order --
with CSR offsets that map a row back to its frame, and cuts exactly those crops; ``FramePipeline.faces`` and
``MtcnnFramePipeline.faces`` put the embedder and the gallery match behind it.  The reference's counterpart is
``detect_multiple_faces`` (``detector/run.py:63-87``), one image at a time on the host.
"""
import ctypes
import typing

import numpy as np
import torch

from .. import _native as N


class FrameFaces(typing.NamedTuple):
    """All faces of a batch of N frames, M rows in all.  Row order: frame-major; inside a frame the detector's pick order
    (descending score).  The faces of frame f are rows ``offsets[f] : offsets[f + 1]``."""
    offsets: torch.Tensor                        # [N + 1] int64, exclusive prefix sum of the faces per frame
    frame: torch.Tensor                          # [M] int64, the frame of each row
    boxes: torch.Tensor                          # [M, 4] left, top, right, bottom
    scores: torch.Tensor                         # [M]
    landmarks: typing.Optional[torch.Tensor]     # [M, 5, 2], or None
    crops: torch.Tensor                          # [M, S, S, 3] uint8, as the embedder is given them
    emb: typing.Optional[torch.Tensor] = None    # [M, d]
    idx: typing.Optional[torch.Tensor] = None    # [M] gallery row, or None without a gallery
    dist: typing.Optional[torch.Tensor] = None   # [M]

    def cluster(self, tolerance, distance_metric: int = 1) -> torch.Tensor:
        """The distinct people of the batch, without a gallery: labels [M] int64 on the device, ``labels[i]`` = the smallest
        row of this FrameFaces that a chain of pairs within ``tolerance`` joins to row i (``oneshot.Gallery.cluster`` on the M
        embeddings; exact single linkage, units of ``evaluation.utility.distance``).  ``M == 0`` gives an empty tensor."""
        if self.emb is None:
            raise ValueError('FrameFaces.cluster needs the embeddings (embed_and_match, or a pipeline\'s faces())')
        if self.emb.shape[0] == 0:
            return torch.empty((0,), dtype=torch.int64, device=self.emb.device)
        from .. import oneshot
        return oneshot.cluster(self.emb, tolerance, distance_metric)[0]

    def dbscan(self, tolerance, min_samples: int = 3, distance_metric: int = 1) -> torch.Tensor:
        """The distinct people of the batch with false detections set apart: labels [M] int64 on the device from
        ``oneshot.Gallery.dbscan`` on the M embeddings.  A face with at least ``min_samples`` faces (itself included) within
        ``tolerance`` is a core face; ``labels[i]`` = the smallest core row of i's cluster, a face that only lies next to a
        core face takes the nearest one's label and bridges nothing, and every other face is -1 (noise).  ``M == 0`` gives an
        empty tensor."""
        if self.emb is None:
            raise ValueError('FrameFaces.dbscan needs the embeddings (embed_and_match, or a pipeline\'s faces())')
        if self.emb.shape[0] == 0:
            return torch.empty((0,), dtype=torch.int64, device=self.emb.device)
        from .. import oneshot
        return oneshot.dbscan(self.emb, tolerance, min_samples, distance_metric)[0]

    def templates(self, labels, weighted: bool = False, normalize: bool = True):
        """One template per person of the batch: the embeddings pooled by ``labels`` [M] (what ``cluster`` or ``dbscan``
        returned; a negative label -- noise -- leaves the face out) -> (templates [T, d] float32, template_labels [T] int64
        ascending, counts [T] int64) on the device.  A template is the mean of its faces in row order, exact
        (``templates.pool_templates``), divided by its norm with ``normalize``; ``weighted`` weighs every face by its detection
        score.  ``M == 0`` gives empty tensors."""
        if self.emb is None:
            raise ValueError('FrameFaces.templates needs the embeddings (embed_and_match, or a pipeline\'s faces())')
        if self.emb.shape[0] == 0:
            dev = self.emb.device
            return (torch.empty((0, self.emb.shape[1]), dtype=torch.float32, device=dev),
                    torch.empty((0,), dtype=torch.int64, device=dev), torch.empty((0,), dtype=torch.int64, device=dev))
        from .. import templates
        return templates.pool_templates(self.emb, labels, self.scores if weighted else None, normalize)[:3]


def _tensor(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def _check_slots(frames, boxes, scores, landmarks):
    t, b, s = _tensor(frames), _tensor(boxes), _tensor(scores)
    if t.dim() != 4 or t.shape[3] != 3 or t.dtype != torch.uint8:
        raise ValueError('expected uint8 frames [N,H,W,3], got %s %s' % (t.dtype, tuple(t.shape)))
    n = t.shape[0]
    if s.dim() != 2 or s.shape[0] != n or s.shape[1] < 1 or not s.dtype.is_floating_point:
        raise ValueError('expected floating-point scores [%d, k], k >= 1, got %s %s' % (n, s.dtype, tuple(s.shape)))
    k = s.shape[1]
    if tuple(b.shape) != (n, k, 4) or not b.dtype.is_floating_point:
        raise ValueError('expected floating-point boxes [%d, %d, 4], got %s %s' % (n, k, b.dtype, tuple(b.shape)))
    lm = None
    if landmarks is not None:
        lm = _tensor(landmarks)
        if tuple(lm.shape) != (n, k, 5, 2) or not lm.dtype.is_floating_point:
            raise ValueError('expected floating-point landmarks [%d, %d, 5, 2], got %s %s' % (n, k, lm.dtype, tuple(lm.shape)))
    return t, b, s, lm


def compact(scores, min_score: float = 0.0, max_faces: typing.Optional[int] = None):
    """``dif_faces_compact``: scores [N, k] -> (count [1], offsets [N + 1], frame [max_faces], slot [max_faces]), int32
    CUDA tensors.  A slot is a face when score >= min_score (a NaN is none); the lists hold the first ``max_faces`` faces
    (default N * k: all), frame-major and in slot order, then -1; ``count`` and ``offsets`` are never truncated.  Nothing
    is read back to the host."""
    s = _tensor(scores)
    if s.dim() != 2 or s.shape[1] < 1 or not s.dtype.is_floating_point:
        raise ValueError('expected floating-point scores [N, k], k >= 1, got %s %s' % (s.dtype, tuple(s.shape)))
    n, k = s.shape
    max_faces = n * k if max_faces is None else int(max_faces)
    if max_faces < 0:
        raise ValueError('max_faces must not be negative')
    dev = N.require_device()
    s = s.to(device=dev, dtype=torch.float32).contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    count, offsets = torch.empty((1,), **i32), torch.empty((n + 1,), **i32)
    frame, slot = torch.empty((max_faces,), **i32), torch.empty((max_faces,), **i32)
    N.check(N.lib.dif_faces_compact(N.ptr(s), n, k, float(min_score), max_faces, N.ptr(count), N.ptr(offsets), N.ptr(frame), N.ptr(slot),
                                    N.stream_ptr()))
    return count, offsets, frame, slot


def _list(frame, slot, dev):
    f = _tensor(frame).to(device=dev, dtype=torch.int32).contiguous()
    s = _tensor(slot).to(device=dev, dtype=torch.int32).contiguous()
    if f.dim() != 1 or f.shape != s.shape:
        raise ValueError('frame and slot must be two lists of one length, got %s and %s' % (tuple(f.shape), tuple(s.shape)))
    return f, s


def gather_rows(src, frame, slot) -> torch.Tensor:
    """``dif_faces_gather``: src [N, k, ...] float -> [M, ...], row j = src[frame[j], slot[j]]; a -1 entry gives zeros."""
    dev = N.require_device()
    t = _tensor(src).to(device=dev, dtype=torch.float32).contiguous()
    if t.dim() < 2:
        raise ValueError('expected slots [N, k, ...], got %s' % (tuple(t.shape),))
    f, s = _list(frame, slot, dev)
    row = int(np.prod(t.shape[2:], dtype=np.int64))
    out = torch.empty((f.shape[0],) + tuple(t.shape[2:]), dtype=torch.float32, device=dev)
    N.check(N.lib.dif_faces_gather(N.ptr(t), row, t.shape[0], t.shape[1], N.ptr(f), N.ptr(s), f.shape[0], N.ptr(out), N.stream_ptr()))
    return out


def crop_faces_list(frames, boxes_ltrb, frame, slot, margin: int = 8, size: int = 112) -> torch.Tensor:
    """``dif_crop_resize_list``: uint8 frames [N,H,W,3], boxes [N, k, 4] -> uint8 CUDA tensor [M, size, size, 3]; crop j is
    the box of slot (frame[j], slot[j]), bit-identical to that slot's crop of ``dif_crop_resize_multi``; a -1 entry gives a
    black crop."""
    dev = N.require_device()
    t = _tensor(frames).to(dev).contiguous()
    b = _tensor(boxes_ltrb).to(device=dev, dtype=torch.float32).contiguous()
    f, s = _list(frame, slot, dev)
    out = torch.empty((f.shape[0], size, size, 3), dtype=torch.uint8, device=dev)
    N.check(N.lib.dif_crop_resize_list(N.ptr(t), t.shape[0], t.shape[1], t.shape[2], N.ptr(b), b.shape[1], N.ptr(f), N.ptr(s), f.shape[0],
                                       float(margin), N.ptr(out), int(size), N.stream_ptr()))
    return out


def align_faces_list(frames, landmarks, frame, slot, size: int = 112, template=None, return_matrices: bool = False):
    """``dif_align_crop_list``: uint8 frames [N,H,W,3], landmarks [N, k, 5, 2] -> uint8 CUDA tensor [M, size, size, 3]; crop j
    (and matrix j with ``return_matrices``: [M, 2, 3]) is that of slot (frame[j], slot[j]), bit-identical to
    ``align.align_faces``; a -1 entry gives a black crop and a NaN matrix."""
    dev = N.require_device()
    t = _tensor(frames).to(dev).contiguous()
    lm = _tensor(landmarks).to(device=dev, dtype=torch.float32).contiguous()
    f, s = _list(frame, slot, dev)
    tpl = None
    if template is not None:
        tpl = np.ascontiguousarray(np.asarray(template, dtype=np.float32))
        if tpl.shape != (5, 2):
            raise ValueError('expected a template of 5 x 2, got %s' % (tpl.shape,))
    out = torch.empty((f.shape[0], size, size, 3), dtype=torch.uint8, device=dev)
    mats = torch.empty((f.shape[0], 2, 3), dtype=torch.float32, device=dev) if return_matrices else None
    N.check(N.lib.dif_align_crop_list(N.ptr(t), t.shape[0], t.shape[1], t.shape[2], N.ptr(lm), lm.shape[1], N.ptr(f), N.ptr(s), f.shape[0],
                                      tpl.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if tpl is not None else None, N.ptr(out),
                                      int(size), N.ptr(mats) if mats is not None else None, N.stream_ptr()))
    return (out, mats) if return_matrices else out


def gather_faces(frames, boxes, scores, landmarks=None, *, min_score: float = 0.0, margin: int = 8, size: int = 112,
                 align: bool = False, max_faces: typing.Optional[int] = None) -> FrameFaces:
    """Slots -> faces: uint8 frames [N,H,W,3], boxes [N, k, 4] (left, top, right, bottom), scores [N, k], optionally
    landmarks [N, k, 5, 2] -> a ``FrameFaces`` filled up to the crops (``emb``, ``idx``, ``dist`` are None).  Any detector
    that fills slots can use it.

    A slot is a face when its score >= ``min_score`` (inclusive; NaN is none).  Rows are frame-major and keep the slot
    order inside a frame.  ``align``: the crops are aligned by the landmarks (``align.align_faces``' arithmetic) instead
    of cut from the boxes with ``margin``.  ``max_faces``: keep the first ``max_faces`` rows only; ``offsets`` is clipped to
    the rows kept, so it stays consistent with them.

    ONE host read per call: the total (4 bytes) is read back, which synchronises the stream once, and exactly M rows are
    allocated after it -- that is what lets the embedder run on the M faces and not on N * k slots, and it is
    negligible next to a detect step of tens of milliseconds.  M = 0 returns empty tensors and launches nothing more."""
    t, b, s, lm = _check_slots(frames, boxes, scores, landmarks)
    if align and lm is None:
        raise ValueError('align=True needs the landmarks of the slots')
    if max_faces is not None and int(max_faces) < 0:
        raise ValueError('max_faces must not be negative')
    size = int(size)
    if size < 1:
        raise ValueError('size must be positive')
    dev = N.require_device()
    t = t.to(dev).contiguous()
    b = b.to(device=dev, dtype=torch.float32).contiguous()
    s = s.to(device=dev, dtype=torch.float32).contiguous()
    if lm is not None:
        lm = lm.to(device=dev, dtype=torch.float32).contiguous()
    n, k = s.shape
    count, offsets, frame, slot = compact(s, min_score)
    m = int(count.item())                                  # the one host read
    offsets = offsets.long()
    if max_faces is not None and m > int(max_faces):
        m = int(max_faces)
        offsets = offsets.clamp(max=m)
    frame, slot = frame[:m], slot[:m]
    f32 = dict(dtype=torch.float32, device=dev)
    if m == 0:
        return FrameFaces(offsets, frame.long(), torch.empty((0, 4), **f32), torch.empty((0,), **f32),
                          torch.empty((0, 5, 2), **f32) if lm is not None else None,
                          torch.empty((0, size, size, 3), dtype=torch.uint8, device=dev))
    fb = gather_rows(b, frame, slot)
    fs = gather_rows(s, frame, slot)
    flm = gather_rows(lm, frame, slot) if lm is not None else None
    if align:
        crops = align_faces_list(t, lm, frame, slot, size)
    else:
        crops = crop_faces_list(t, b, frame, slot, margin, size)
    return FrameFaces(offsets, frame.long(), fb, fs, flm, crops)


def embed_and_match(faces: FrameFaces, embedder, gallery=None, distance_metric: int = 1) -> FrameFaces:
    """Fills ``emb`` (``embedder.embed`` walks the crops in chunks of ``embedder.max_batch``) and, with a gallery, ``idx`` and
    ``dist`` of its top-1 match."""
    emb = embedder.embed(faces.crops)                      # (no launch for M = 0)
    if gallery is None:
        return faces._replace(emb=emb)
    idx, dist = gallery.match(emb, distance_metric)
    return faces._replace(emb=emb, idx=idx, dist=dist)
