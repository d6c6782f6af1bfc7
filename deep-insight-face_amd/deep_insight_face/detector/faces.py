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


MAX_TRACK_FACES, MAX_TRACK_GAP = 64, 32        # DIF_TRACKS_MAX_FACES, DIF_TRACKS_MAX_GAP


class TrackState(typing.NamedTuple):
    """What ``FrameFaces.tracks`` needs to go on with the next batch of frames: the faces of the last ``max_gap`` frames in
    ``max_gap * k`` fixed slots on the device (``buf``: one buffer laid out as ``dif_tracks_link`` documents it -- the views
    below name its parts), and three host integers.  Immutable: a call returns a new one."""
    buf: typing.Optional[torch.Tensor]           # uint8 [dif_tracks_state_size(max_gap, k, d)], or None: no face stored yet
    max_gap: int
    k: int                                       # slots per frame
    d: int
    pad: int                                     # frames without a face that went by since ``buf`` was written
    row_base: int                                # faces seen so far = the global row of the next batch's row 0

    def _part(self, name):
        s = self.max_gap * self.k
        at = 0
        for part, dtype, shape in (('labels', torch.int64, (s,)), ('age', torch.int64, (s,)), ('rows', torch.int64, (s,)),
                                   ('boxes', torch.float32, (s, 4)), ('emb', torch.float32, (s, self.d)),
                                   ('closed', torch.int32, (s,)), ('count', torch.int32, (self.max_gap,))):
            size = int(np.prod(shape)) * (8 if dtype == torch.int64 else 4)
            if part == name:
                return self.buf[at:at + size].view(dtype).view(shape)
            at += size
        raise KeyError(name)

    labels = property(lambda self: self._part('labels'))      # [max_gap * k] int64: slot (t, p) = position p of the t-th
    age = property(lambda self: self._part('age'))            # of the last max_gap frames; the first count[t] slots of a
    rows = property(lambda self: self._part('rows'))          # frame are filled.  rows: the face's global row
    boxes = property(lambda self: self._part('boxes'))
    emb = property(lambda self: self._part('emb'))
    closed = property(lambda self: self._part('closed'))      # int32: 1 = has a successor already (no tail any more)
    count = property(lambda self: self._part('count'))        # [max_gap] int32 (clipped faces are not stored)


class Tracks(typing.NamedTuple):
    """``FrameFaces.tracks``: per face of the batch, on the device.  Rows are GLOBAL: ``state.row_base`` of the state handed
    in (0 without one) + the row of the batch."""
    labels: torch.Tensor                         # [M] int64: the global row of the first face of the face's track
    prev: torch.Tensor                           # [M] int64: the global row of the face it continues, -1 at a start
    link_dist: torch.Tensor                      # [M] float32: the distance to that face, NaN at a start
    age: torch.Tensor                            # [M] int64: 1 at a start, age[prev] + 1
    n_new: torch.Tensor                          # [1] int64: tracks started in this batch
    clipped: torch.Tensor                        # [1] int64: faces at a position >= max_faces_per_frame
    state: TrackState


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

    def tracks(self, tolerance, min_iou: float = 0.3, max_gap: int = 1, distance_metric: int = 1,
               state: typing.Optional[TrackState] = None, max_faces_per_frame: typing.Optional[int] = None) -> Tracks:
        """The faces of the batch -- ONE sequence of frames, in order -- linked into tracks (``dif_tracks_link``, where the
        rule is written out): a face continues the track whose last face, at most ``max_gap`` frames ago (frames without
        faces count), has a box IoU >= ``min_iou`` with it and an embedding within ``tolerance`` (units of
        ``evaluation.utility.distance``, bit for bit its values); nearest pairs first, ties to the lower rows; a track
        holds one face per frame at most.  Unlike ``cluster`` it never joins two people who are on screen at once, looks
        at neighbouring frames only, and goes on from batch to batch: hand ``state`` of the ``Tracks`` returned for the
        previous batch to the call for the next, and labels, ages and link distances are those of one call over all
        frames, bit for bit.  Labels are global rows, so ``templates(tracks.labels)`` pools a batch and
        ``TemplatePool.add(faces.emb, tracks.labels)`` pools batch after batch.

        ``max_faces_per_frame`` (at most 64): the faces of a frame beyond it (its lowest scores) are never linked and are
        counted in ``clipped``.  Given, the call reads nothing back to the host.  ``None``: the size of the largest frame
        -- at most 64 -- which is read back ONCE (8 bytes, one synchronisation of the stream).  ``M == 0`` returns empty
        tensors and launches nothing; the state still moves on by the N frames."""
        if self.emb is None:
            raise ValueError('FrameFaces.tracks needs the embeddings (embed_and_match, or a pipeline\'s faces())')
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        max_gap = int(max_gap)
        if not 1 <= max_gap <= MAX_TRACK_GAP:
            raise ValueError('max_gap must lie in [1, %d], got %d' % (MAX_TRACK_GAP, max_gap))
        if max_faces_per_frame is not None and not 1 <= int(max_faces_per_frame) <= MAX_TRACK_FACES:
            raise ValueError('max_faces_per_frame must lie in [1, %d], got %s' % (MAX_TRACK_FACES, max_faces_per_frame))
        m, d = self.emb.shape
        n = self.offsets.shape[0] - 1
        if state is None:
            state = TrackState(None, max_gap, 0, d, 0, 0)
        elif (state.max_gap, state.d) != (max_gap, d):
            raise ValueError('the state was written with max_gap %d and %d-d embeddings, this call has %d and %d'
                             % (state.max_gap, state.d, max_gap, d))
        dev = self.emb.device
        i64 = dict(dtype=torch.int64, device=dev)
        if m == 0:
            empty = torch.empty((0,), **i64)
            return Tracks(empty, empty.clone(), torch.empty((0,), dtype=torch.float32, device=dev), empty.clone(),
                          torch.zeros((1,), **i64), torch.zeros((1,), **i64), state._replace(pad=min(state.pad + n, max_gap)))
        N.require_device()
        offsets = self.offsets.to(dtype=torch.int64).contiguous()
        if max_faces_per_frame is None:
            largest = int((offsets[1:] - offsets[:-1]).max().item())          # the one host read
            kmax = min(max(largest, 1), MAX_TRACK_FACES)
        else:
            kmax = int(max_faces_per_frame)
        boxes = self.boxes.to(dtype=torch.float32).contiguous()
        emb = self.emb.to(dtype=torch.float32).contiguous()
        k_in = state.k if state.buf is not None else 0
        k_out = max(kmax, k_in)
        out_buf = torch.empty((N.lib.dif_tracks_state_size(max_gap, k_out, d),), dtype=torch.uint8, device=dev)
        work = torch.empty((N.lib.dif_tracks_workspace_size(m, max_gap, kmax, k_in),), dtype=torch.uint8, device=dev)
        labels, prev, age = torch.empty((m,), **i64), torch.empty((m,), **i64), torch.empty((m,), **i64)
        link_dist = torch.empty((m,), dtype=torch.float32, device=dev)
        n_new, clipped = torch.empty((1,), **i64), torch.empty((1,), **i64)
        N.check(N.lib.dif_tracks_link(N.ptr(offsets), N.ptr(boxes), N.ptr(emb), n, m, d, float(tolerance), float(min_iou), max_gap,
                                      distance_metric, kmax, state.row_base, N.ptr(state.buf) if k_in else None, k_in, state.pad,
                                      N.ptr(prev), N.ptr(link_dist), N.ptr(labels), N.ptr(age), N.ptr(n_new), N.ptr(clipped),
                                      N.ptr(out_buf), k_out, N.ptr(work), work.shape[0], 0, N.stream_ptr()))
        return Tracks(labels, prev, link_dist, age, n_new, clipped,
                      TrackState(out_buf, max_gap, k_out, d, 0, state.row_base + m))

    def quality(self, frame_hw=None, lo: int = 0, hi: int = 255):
        """``quality.face_quality`` on the crops, landmarks and boxes of these faces -> ``quality.FaceQuality``, on the device.
        ``frame_hw`` = (H, W) of the frames lets the boxes count (``inside``, and its factor of the score); without it they
        are left out.  Without landmarks the pose columns are NaN."""
        from . import quality
        return quality.face_quality(self.crops, self.landmarks, self.boxes if frame_hw is not None else None, frame_hw, lo, hi)

    def best(self, labels, key=None, frame_hw=None):
        """The best shot of every label: the ONE face with the greatest ``key`` [M] float32 -- default: ``quality(frame_hw)
        .score`` -- among the faces that carry it -> (best_row [T] int64, template_labels [T] int64 ascending, best_key [T]
        float32, counts [T] int64) on the device.  Ties go to the lower row, a NaN key is never chosen, and a label whose
        keys are all NaN has row -1 and key NaN (``templates.BestShots``, where the rule is written out).  A negative label
        leaves the face out; ``M == 0`` gives empty tensors."""
        dev = self.crops.device
        if self.crops.shape[0] == 0:
            i64 = dict(dtype=torch.int64, device=dev)
            return (torch.empty((0,), **i64), torch.empty((0,), **i64), torch.empty((0,), dtype=torch.float32, device=dev),
                    torch.empty((0,), **i64))
        from .. import templates
        if key is None:
            key = self.quality(frame_hw).score
        shots = templates.BestShots(device=dev if dev.type == 'cuda' else None)
        try:
            shots.add(labels, key.contiguous() if torch.is_tensor(key) else key)
            return shots.row, shots.labels, shots.key, shots.counts
        finally:
            shots.close()

    def redact(self, frames, select=None, mode: str = 'pixelate', cells: int = 8, min_cell: int = 4, margin: float = 0.0,
               shape: str = 'box', fill=(0, 0, 0), out=None):
        """The frames these faces came from with the faces hidden, on the device (``redact.redact_frames``;
        ``dif_frames_redact``, where the rule is written out): ``frames`` uint8 [N, H, W, 3] -> ``out`` (``frames.clone()``
        unless given; ``out=frames`` works in place).  ``select`` [M] bool or uint8 picks the faces to hide, ``None`` hides
        all: ``faces.redact(frames, select=faces.dist > tol)`` hides everyone the gallery does not know.  ``mode``:
        'pixelate' (``cells`` x ``cells`` means over the box grown by ``margin`` of its size), 'smooth' (the same means
        interpolated: no block edges) or 'fill'; ``shape`` 'box' or 'ellipse'.  Where faces overlap, the lowest row (the best
        face) is what shows; every value comes from ``frames``.  Nothing is read back."""
        from . import redact
        return redact.redact_frames(frames, self.offsets, self.boxes, select, mode, cells, min_cell, margin, shape, fill, out)

    def annotate(self, frames, names=None, known=None, values=None, text=None, colors=None, select=None, decimals: int = 2,
                 unknown: str = '?', length: int = 32, margin: float = 0.0, thickness: int = 2, scale: int = 2, mark: int = 1,
                 out=None):
        """The frames these faces came from with the faces marked, on the device (``annotate.annotate_frames``;
        ``dif_frames_annotate``, where the rule is written out): ``frames`` uint8 [N, H, W, 3] -> ``out`` (``frames.clone()``
        unless given; ``out=frames`` paints in place) with a ring round every selected face, a square on each of its
        landmarks and a plate with its label.  The label is ``text`` uint8 [M, L] if given; otherwise, with ``names`` (an
        ``annotate.NameTable`` over the gallery's rows) or ``values`` given, it is composed on the device from ``idx``
        (``annotate.compose_text``): the name where ``known`` holds, ``unknown`` elsewhere, then the value -- ``faces.annotate(
        frames, names=table, known=faces.dist <= tol, values=faces.dist, colors=annotate.palette(tracks.labels))``.  With
        none of the three there are no plates.  It composes with redaction: ``faces.annotate(faces.redact(frames,
        select=faces.dist > tol), ...)``.  Nothing is read back."""
        from . import annotate
        if text is None and (names is not None or values is not None):
            if names is not None and self.idx is None:
                raise ValueError('FrameFaces.annotate with names needs the gallery rows (a pipeline\'s faces() with a gallery)')
            text = annotate.compose_text(names, self.idx if names is not None else None, known, values, decimals, unknown, length)
        return annotate.annotate_frames(frames, self.offsets, self.boxes, self.landmarks, text, colors, select, margin, thickness, scale,
                                        mark, out)

    def evaluate(self, gt_boxes, gt_offsets, iou_thresholds=(0.5,), gt_ignore=None):
        """These detections against the labelled boxes of the same N frames, on the device (``evaluation.detection.
        evaluate_detections``; ``dif_det_match``, where the rule is written out): ``gt_boxes`` [T, 4] left, top, right,
        bottom with ``gt_offsets`` [N + 1] as a CSR list over the frames, ``gt_ignore`` [T] bool for truths that count for
        nobody -> a ``DetectionEval``: per face the truth it overlaps most, its float64 IoU and its outcome at each IoU
        threshold, and the precision / recall curve and average precision of the batch.  ``M == 0`` and ``T == 0`` work; over
        many batches use ``evaluation.detection.DetectionEvaluator``.  Nothing is read back."""
        from ..evaluation import detection
        return detection.evaluate_detections(self.boxes, self.scores, self.offsets, gt_boxes, gt_offsets, iou_thresholds, gt_ignore)

    def templates(self, labels, weighted=False, normalize: bool = True):
        """One template per person of the batch: the embeddings pooled by ``labels`` [M] (what ``cluster`` or ``dbscan``
        returned; a negative label -- noise -- leaves the face out) -> (templates [T, d] float32, template_labels [T] int64
        ascending, counts [T] int64) on the device.  A template is the mean of its faces in row order, exact
        (``templates.pool_templates``), divided by its norm with ``normalize``; ``weighted`` = True weighs every face by its
        detection score, a float32 tensor [M] -- ``quality().score``, say -- by that.  ``M == 0`` gives empty tensors."""
        if self.emb is None:
            raise ValueError('FrameFaces.templates needs the embeddings (embed_and_match, or a pipeline\'s faces())')
        if self.emb.shape[0] == 0:
            dev = self.emb.device
            return (torch.empty((0, self.emb.shape[1]), dtype=torch.float32, device=dev),
                    torch.empty((0,), dtype=torch.int64, device=dev), torch.empty((0,), dtype=torch.int64, device=dev))
        from .. import templates
        if torch.is_tensor(weighted):
            weights = weighted
            if weights.dtype != torch.float32 or tuple(weights.shape) != (self.emb.shape[0],):
                raise ValueError('weights must be a float32 tensor [%d], got %s %s' % (self.emb.shape[0], weights.dtype, tuple(weights.shape)))
        else:
            weights = self.scores if weighted else None
        return templates.pool_templates(self.emb, labels, weights, normalize)[:3]


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
