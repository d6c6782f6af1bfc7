"""Every face in a frame on the device (csrc/faces.hip, detector/faces.py): the compaction against tests/faces_ref.py,
the list forms of the crop and the alignment against the slot forms bit for bit, gather_faces on hand-made slots, and both
frame pipelines' faces() end to end."""
import numpy as np
import pytest
import torch

import faces_ref

pytestmark = pytest.mark.gpu


def _scores(n, k, min_score, density, seed):
    """Scores drawn from {-1, NaN, exactly min_score, just below it, random values at or above it}; `density` = the share of
    faces."""
    rng = np.random.default_rng(seed)
    ms = np.float32(min_score)
    below = np.array([-1.0, np.nan, np.nextafter(ms, np.float32(-np.inf))], np.float32)
    out = below[rng.integers(0, 3, (n, k))]
    face = rng.random((n, k)) < density
    val = (ms + rng.random((n, k), dtype=np.float32) * np.float32(0.25)).astype(np.float32)
    val[rng.random((n, k)) < 0.3] = ms                         # exactly the threshold: a face
    out[face] = val[face]
    return out


def _check_compact(scores, min_score, max_faces=None):
    from deep_insight_face.detector.faces import compact
    count, offsets, frame, slot = compact(scores, min_score, max_faces)
    wc, wo, wf, ws = faces_ref.compact(scores, min_score, max_faces)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in (count, offsets, frame, slot))
    assert count.tolist() == [wc]
    assert np.array_equal(offsets.cpu().numpy(), wo)
    assert np.array_equal(frame.cpu().numpy(), wf) and np.array_equal(slot.cpu().numpy(), ws)
    return wc


@pytest.mark.parametrize('min_score', [0.0, 0.7])
@pytest.mark.parametrize('n,k', [(1, 1), (3, 5), (70, 33)])     # 2310 slots: three passes of the 1024-thread block, and
def test_compaction_equals_the_reference(cuda, n, k, min_score):       # 33 puts the frame boundaries inside waves
    for density, seed in ((0.5, 1), (0.1, 2), (0.95, 3)):
        s = _scores(n, k, min_score, density, seed + n)
        if n * k == 1:
            s[0, 0] = (min_score, -1.0, np.nan)[seed - 1]      # (1, 1): a valid slot, an empty one, a NaN
        _check_compact(s, min_score)


def test_compaction_edge_values(cuda):
    ms = np.float32(0.7)
    s = np.array([[ms, np.nextafter(ms, np.float32(-1)), np.nan, -1.0, np.nextafter(ms, np.float32(2)), np.inf, -np.inf, -0.0]], np.float32)
    assert _check_compact(s, ms) == 3
    assert _check_compact(s, 0.0) == 5                         # -0.0 >= 0.0: a face


def test_compaction_with_every_slot_empty(cuda):
    from deep_insight_face.detector.faces import compact
    s = np.full((70, 33), -1.0, np.float32)
    s[::3] = np.nan
    count, offsets, frame, slot = compact(s, 0.0)
    assert count.item() == 0 and not offsets.any() and bool((frame == -1).all()) and bool((slot == -1).all())
    _check_compact(s, 0.0)


def test_compaction_with_fewer_list_entries_than_faces(cuda):
    s = _scores(70, 33, 0.0, 0.5, 9)
    total = _check_compact(s, 0.0, max_faces=100)              # count exact, offsets untruncated, the first 100 faces listed
    assert total > 1000
    _check_compact(s, 0.0, max_faces=0)
    _check_compact(s, 0.0, max_faces=total)
    _check_compact(s, 0.0, max_faces=total + 7)


def test_compaction_of_no_frames(cuda):
    from deep_insight_face.detector.faces import compact
    count, offsets, frame, slot = compact(np.zeros((0, 4), np.float32), 0.0)
    assert count.tolist() == [0] and offsets.tolist() == [0] and frame.numel() == 0 and slot.numel() == 0


def test_compaction_refuses_bad_arguments(cuda):
    from deep_insight_face import _native as N
    from deep_insight_face.detector.faces import compact
    with pytest.raises(ValueError):
        compact(np.zeros((2, 0), np.float32))
    with pytest.raises(ValueError):
        compact(np.zeros((2, 3), np.float32), max_faces=-1)
    with pytest.raises(ValueError):
        compact(np.zeros((2, 3), np.int32))
    s = torch.zeros((2, 3), device=cuda)
    i = torch.zeros((8,), dtype=torch.int32, device=cuda)
    for args in ((N.ptr(s), 2, 0, 0.0, 6, N.ptr(i), N.ptr(i), N.ptr(i), N.ptr(i)), (N.ptr(s), 2, 3, 0.0, -1, N.ptr(i), N.ptr(i), N.ptr(i), N.ptr(i)),
                 (N.ptr(s), 2, 3, 0.0, 6, None, N.ptr(i), N.ptr(i), N.ptr(i)), (None, 2, 3, 0.0, 6, N.ptr(i), N.ptr(i), N.ptr(i), N.ptr(i))):
        with pytest.raises(N.DifError, match='dif_faces_compact'):
            N.check(N.lib.dif_faces_compact(*args, N.stream_ptr()))


# ---- the list forms against the slot forms ---------------------------------------------------------------------------
H, W, K = 48, 64, 4


def _slots():
    rng = np.random.default_rng(31)
    frames = rng.integers(0, 256, (5, H, W, 3), dtype=np.uint8)
    boxes = np.empty((5, K, 4), np.float32)
    for f in range(5):
        for s in range(K):
            l, t = rng.uniform(0, W - 24), rng.uniform(0, H - 24)
            boxes[f, s] = (l, t, l + rng.uniform(6, 40), t + rng.uniform(6, 30))
    boxes[0, 1] = (-9.5, -4.0, 30.2, 70.0)                     # overhangs the frame on three sides
    boxes[1, 2] = (20.0, 10.0, 20.0, 30.0)                     # degenerate: no width
    boxes[2, 0] = (8.0, 4.0, 40.0, 36.0)                       # 32 x 32 at margin 0: integer ratios
    boxes[3, 3] = (0.0, 0.0, 0.0, 0.0)                         # an empty slot
    scores = rng.uniform(0.5, 1.0, (5, K)).astype(np.float32)
    scores[3, 3] = -1.0
    lm = np.empty((5, K, 5, 2), np.float32)
    shape = np.array([[-8, -6], [8, -6], [0, 2], [-6, 9], [6, 9]], np.float32)
    for f in range(5):
        for s in range(K):
            a, sc = rng.uniform(-0.6, 0.6), rng.uniform(0.6, 1.6)
            rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], np.float32) * np.float32(sc)
            lm[f, s] = shape @ rot.T + np.array([rng.uniform(4, W - 4), rng.uniform(4, H - 4)], np.float32) + rng.normal(0, 0.5, (5, 2))
    lm[4, 1, 2, 0] = np.nan                                    # a non-finite set
    lm[0, 3] = lm[0, 3, 0]                                     # five coinciding points
    lm[3, 3] = 0.0                                             # the empty slot's
    return frames, boxes, scores, lm


def _lists():
    """The natural order, and a permutation with a -1 entry in it."""
    f, s = np.divmod(np.arange(5 * K, dtype=np.int32), K)
    perm = np.random.default_rng(5).permutation(5 * K)
    pf, ps = np.insert(f[perm], 3, -1), np.insert(s[perm], 3, -1)
    return [(f.astype(np.int32), s.astype(np.int32)), (pf.astype(np.int32), ps.astype(np.int32))]


@pytest.mark.parametrize('size,margin', [(24, 8), (24, 0), (16, 0), (13, 3)])
def test_crop_list_equals_the_slot_form(cuda, size, margin):
    from deep_insight_face import _native as N
    from deep_insight_face.detector.faces import crop_faces_list
    frames, boxes, _, _ = _slots()
    t, b = torch.from_numpy(frames).to(cuda), torch.from_numpy(boxes).to(cuda)
    want = torch.empty((5 * K, size, size, 3), dtype=torch.uint8, device=cuda)
    N.check(N.lib.dif_crop_resize_multi(N.ptr(t), 5, H, W, N.ptr(b), None, K, float(margin), N.ptr(want), size, N.stream_ptr()))
    assert want.any() and (margin > 0 or not want[1 * K + 2].any())      # the degenerate box: black without a margin
    for f, s in _lists():
        got = crop_faces_list(t, b, f, s, margin, size)
        listed = f >= 0
        rows = torch.from_numpy((f * K + s)[listed].astype(np.int64)).to(cuda)
        assert torch.equal(got[torch.from_numpy(listed).to(cuda)], want[rows])
        assert not got[torch.from_numpy(~listed).to(cuda)].any()                 # a -1 entry: a black crop


@pytest.mark.parametrize('size,template', [(32, None), (15, None), (24, 'own')])        # 15 x 15: no multiple of four pixels, byte stores
def test_align_list_equals_the_slot_form(cuda, size, template):
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112, align_faces
    from deep_insight_face.detector.faces import align_faces_list
    frames, _, _, lm = _slots()
    tpl = None if template is None else ARCFACE_TEMPLATE_112[::-1] * np.float32(0.2) + np.float32(1.5)
    want, wm = align_faces(frames, lm, size, template=tpl, k=K, return_matrices=True)
    assert want.any() and not want[4 * K + 1].any() and not want[0 * K + 3].any()
    assert bool(torch.isnan(wm[4 * K + 1]).all()) and bool(torch.isfinite(wm[0]).all())
    for f, s in _lists():
        got, gm = align_faces_list(frames, lm, f, s, size, template=tpl, return_matrices=True)
        listed = torch.from_numpy(f >= 0).to(cuda)
        rows = torch.from_numpy((f * K + s)[f >= 0].astype(np.int64)).to(cuda)
        assert torch.equal(got[listed], want[rows])
        assert torch.equal(gm[listed].view(torch.int32), wm[rows].view(torch.int32))      # bit for bit, NaNs included
        assert not got[~listed].any() and bool(torch.isnan(gm[~listed]).all())
        assert torch.equal(align_faces_list(frames, lm, f, s, size, template=tpl), got)   # without the matrices


def test_gather_rows_and_out_of_range_entries(cuda):
    from deep_insight_face.detector.faces import gather_rows
    _, boxes, scores, lm = _slots()
    f = np.array([4, 0, -1, 2, 5, 1], np.int32)
    s = np.array([3, 0, -1, K, 0, 2], np.int32)                 # (2, K) and (5, 0) lie outside the slots: inert, like -1
    ok = np.array([True, True, False, False, False, True])
    for src in (boxes, scores, lm):
        got = gather_rows(src, f, s).cpu().numpy()
        assert got.shape == (6,) + src.shape[2:]
        assert np.array_equal(got[ok], src[f[ok], s[ok]], equal_nan=True) and not got[~ok].any()


# ---- gather_faces ----------------------------------------------------------------------------------------------------
def _hand_made():
    frames, boxes, _, lm = _slots()
    frames, boxes, lm = frames[:4], boxes[:4].copy(), lm[:4].copy()
    boxes[3, 3], lm[3, 3] = boxes[2, 3], lm[2, 3]
    scores = np.full((4, K), -1.0, np.float32)                 # 0, 1, 3 and k faces
    scores[1, 2] = 0.9
    scores[2, :3] = (0.95, 0.8, 0.0)
    scores[3] = (0.99, 0.9, 0.8, 0.7)
    return frames, boxes, scores, lm


@pytest.mark.parametrize('align', [False, True])
def test_gather_faces_on_hand_made_slots(cuda, align):
    from deep_insight_face.detector.align import align_faces
    from deep_insight_face.detector.faces import crop_faces_list, gather_faces
    frames, boxes, scores, lm = _hand_made()
    ff = gather_faces(frames, boxes, scores, lm, margin=4, size=20, align=align)
    wf, ws = np.nonzero(scores >= 0)
    assert ff.offsets.tolist() == [0, 0, 1, 4, 8] and ff.frame.tolist() == wf.tolist()
    assert ff.offsets.dtype == ff.frame.dtype == torch.int64
    for f in range(4):                                         # the CSR offsets and the frame of each row say the same
        assert ff.frame[ff.offsets[f]:ff.offsets[f + 1]].tolist() == [f] * int((scores[f] >= 0).sum())
    assert np.array_equal(ff.boxes.cpu().numpy(), boxes[wf, ws]) and np.array_equal(ff.scores.cpu().numpy(), scores[wf, ws])
    assert np.array_equal(ff.landmarks.cpu().numpy(), lm[wf, ws], equal_nan=True)
    rows = torch.from_numpy(wf * K + ws).to(cuda)
    want = align_faces(frames, lm, 20, k=K)[rows] if align else crop_faces_list(frames, boxes, wf, ws, 4, 20)
    assert ff.crops.dtype == torch.uint8 and torch.equal(ff.crops, want) and ff.crops.any()
    assert ff.emb is None and ff.idx is None and ff.dist is None
    if not align:
        assert gather_faces(frames, boxes, scores, margin=4, size=20).landmarks is None
        cut = gather_faces(frames, boxes, scores, lm, margin=4, size=20, max_faces=3)      # the first three rows, offsets clipped
        assert cut.offsets.tolist() == [0, 0, 1, 3, 3] and cut.frame.tolist() == [1, 2, 2]
        assert torch.equal(cut.crops, ff.crops[:3]) and torch.equal(cut.boxes, ff.boxes[:3])
        high = gather_faces(frames, boxes, scores, lm, min_score=0.8, margin=4, size=20)
        assert high.offsets.tolist() == [0, 0, 1, 3, 6] and high.scores.tolist() == scores[scores >= 0.8].tolist()


@pytest.mark.parametrize('with_landmarks', [False, True])
def test_gather_faces_without_a_face(cuda, with_landmarks):
    from deep_insight_face.detector.faces import gather_faces
    frames, boxes, scores, lm = _hand_made()
    ff = gather_faces(frames, boxes, np.full_like(scores, -1.0), lm if with_landmarks else None, size=20, align=with_landmarks)
    assert ff.offsets.tolist() == [0] * 5 and ff.offsets.dtype == torch.int64
    assert ff.frame.shape == (0,) and ff.frame.dtype == torch.int64
    assert ff.boxes.shape == (0, 4) and ff.scores.shape == (0,) and ff.boxes.dtype == ff.scores.dtype == torch.float32
    assert ff.crops.shape == (0, 20, 20, 3) and ff.crops.dtype == torch.uint8
    if with_landmarks:
        assert ff.landmarks.shape == (0, 5, 2) and ff.landmarks.dtype == torch.float32
    else:
        assert ff.landmarks is None
    assert all(t.is_cuda for t in (ff.offsets, ff.frame, ff.boxes, ff.scores, ff.crops))


# ---- end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def embedder():
    """ResNet-50V2, 512-d, as tests/test_embed_gpu.py builds it (its batch-to-batch tolerance is used below); max_batch 4, so
    that every list of more than four faces is embedded in chunks."""
    from deep_insight_face.networks.triplet import bottleneck_network
    emb = bottleneck_network('resnet', emd_size=512, input_shape=(112, 112, 3), max_batch=4)('v2')
    emb.init_synthetic(2024)
    emb.set_input_transform(scale=1 / 255.)
    yield emb
    emb.close()


def _blobs(n, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        img = np.zeros((h, w, 3), np.float32)
        for _ in range(6):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(8, 40)
            img += rng.uniform(40, 160, 3) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))[..., None]
        out[i] = np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
    return out


def _same_bits(a, b):
    """Equal bit for bit (a probe that IS a gallery row can land a hair above cosine 1, whose arccos is the reference's NaN)."""
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _chunkwise(embedder, crops):
    return torch.cat([embedder.embed(crops[lo:lo + embedder.max_batch]) for lo in range(0, crops.shape[0], embedder.max_batch)])


def _planted_gallery(emb, seed=0):
    """Random rows with the given embeddings planted at rows 10, 13, 16, ...; metric 1 puts a row at distance ~0 of itself
    (arccos near 1 loses half the digits: < 1e-3, or NaN a hair above 1) and a random 512-d row at ~0.5."""
    from deep_insight_face import oneshot
    rows = np.random.default_rng(seed).standard_normal((10 + 3 * emb.shape[0], 512)).astype(np.float32)
    rows[10::3] = emb.cpu().numpy()
    return oneshot.Gallery(rows)


def _check_pipeline(make, frames, embedder, ff, slots):
    """ff = faces() without a gallery; slots = (boxes [N, k, 4], scores [N, k], landmarks or None) of the detector."""
    sb, ss, slm = slots
    n, k = ss.shape
    keep = ss >= 0
    assert torch.equal(ff.frame, torch.nonzero(keep)[:, 0]) and ff.offsets.tolist() == [0] + torch.cumsum(keep.sum(1), 0).tolist()
    assert torch.equal(ff.boxes, sb[keep]) and torch.equal(ff.scores, ss[keep])
    if slm is not None:
        assert torch.equal(ff.landmarks, slm[keep])
    m = ff.frame.shape[0]
    assert ff.crops.shape == (m, 112, 112, 3) and ff.emb.shape == (m, 512) and ff.idx is None and ff.dist is None
    assert m > embedder.max_batch                              # the embed ran in chunks
    assert torch.equal(ff.emb, _chunkwise(embedder, ff.crops))
    per_frame = keep.sum(1)
    assert int(per_frame.max()) >= 2, per_frame.tolist()       # the point of it: some frame holds more than one face
    gal = _planted_gallery(ff.emb)
    pipe = make(gal)
    again = pipe.faces(frames)
    assert torch.equal(again.emb, ff.emb) and torch.equal(again.crops, ff.crops)
    idx, dist = gal.match(ff.emb, 1)
    assert torch.equal(again.idx, idx) and _same_bits(again.dist, dist)
    assert not bool((again.dist >= 1e-3).any())               # every face found its planted row (or an identical one)
    # row 0 of each frame that holds a face = what __call__ reports for the frame
    bx, sc, e = pipe(frames)[:3]
    has = per_frame > 0
    first = ff.offsets[:-1][has]
    assert torch.equal(ff.boxes[first], bx[has]) and torch.equal(ff.scores[first], sc[has])
    a, b = ff.emb[first].double(), e[has].double()
    assert float((1 - (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).max()) < 1e-6      # tests/test_embed_gpu.py: one row
    np.testing.assert_allclose(ff.emb[first].cpu().numpy(), e[has].cpu().numpy(), atol=2e-6)   # in batches of two sizes
    gal.close()


@pytest.mark.parametrize('align', [False, True])
def test_mtcnn_pipeline_faces(cuda, embedder, align):
    """96 x 128 frames, synthetic weights, caps (24, 12, 8) as tests/test_mtcnn.py.  Seed and logit_scale chosen on an MI355X:
    init_synthetic(2024) at logit_scale 1.0 on the blob frames of seed 11 gives 8, 7, 8, 8, 8 faces -- several per frame and
    one empty slot (seeds 7 / 2024 at logit_scale 1.0, 0.3 and 0.1 on frames of seed 5 fill all 8 slots of every frame)."""
    from deep_insight_face.detector.mtcnn import MtcnnDetector, MtcnnFramePipeline
    hw, n = (96, 128), 5
    frames = torch.from_numpy(_blobs(n, hw[0], hw[1], seed=11)).to(cuda)
    det = MtcnnDetector(hw, max_batch=2, cap=(24, 12, 8)).init_synthetic(2024, logit_scale=1.0)
    make = lambda gal: MtcnnFramePipeline(det, embedder, gal, margin=8, align=align)
    ff = make(None).faces(frames)                              # five frames through a detector of max_batch 2
    parts = [det.detect(frames[lo:lo + 2], return_landmarks=align) for lo in range(0, n, 2)]
    slots = [torch.cat([p[i] for p in parts]) for i in range(3 if align else 2)] + ([] if align else [None])
    assert (ff.landmarks is not None) == align
    _check_pipeline(make, frames, embedder, ff, slots)
    det.close()


def test_yolo_pipeline_faces(cuda, embedder):
    """YOLOv3-face at 128 x 128 on 96 x 128 frames, weights as tests/test_imageops_gpu.py makes them: every cell passes with
    about the same score, so the suppression keeps several boxes per frame."""
    from deep_insight_face.detector import run as drun
    from deep_insight_face.networks.weights import synth_params
    det = drun.yolo_v3_face(1, 128, max_batch=3)
    p = synth_params(det.param_spec(), seed=11)
    for name in p:
        if name in ('conv_58/kernel', 'conv_66/kernel', 'conv_74/kernel'):
            p[name] = p[name] * 1e-5
        if name in ('conv_58/bias', 'conv_66/bias', 'conv_74/bias'):
            p[name] = np.zeros_like(p[name])
            p[name][4::6] = 2.0
            p[name][5::6] = 2.0
    det.set_weights(p)
    det.set_input_transform(scale=1 / 255.)
    frames = torch.from_numpy(_blobs(3, 96, 128, seed=8)).to(cuda)
    kmax = 6
    make = lambda gal: _Yolo(det, embedder, gal, kmax)
    pipe = make(None)
    ff = pipe.faces(frames)
    sb, ss = pipe.detect_slots(frames, kmax)
    assert sb.shape == (3, kmax, 4) and ss.shape == (3, kmax)
    assert bool((ss[:, 1:][ss[:, 1:] >= 0] <= ss[:, :-1][ss[:, 1:] >= 0]).all())          # pick order: descending score
    assert bool((sb[ss < 0] == -1).all())
    _check_pipeline(make, frames, embedder, ff, (sb, ss, None))
    with pytest.raises(ValueError):
        pipe.pipe.faces(frames, max_faces_per_frame=0)
    det.close()


class _Yolo:
    """FramePipeline with max_faces_per_frame bound, so that one checker serves both pipelines."""

    def __init__(self, det, emb, gal, k):
        from deep_insight_face.detector.run import FramePipeline
        self.pipe, self.k = FramePipeline(det, emb, gal, margin=8, score=0.4), k

    def faces(self, frames):
        return self.pipe.faces(frames, max_faces_per_frame=self.k)

    def detect_slots(self, frames, k):
        return self.pipe.detect_slots(frames, k)

    def __call__(self, frames):
        return self.pipe(frames)


def test_embed_in_chunks_smaller_than_the_list(cuda, embedder):
    """Eight faces through an embedder of max_batch 4 (and 3: a ragged last chunk) = the chunks embedded one by one."""
    from deep_insight_face.detector.faces import embed_and_match, gather_faces
    from deep_insight_face.networks.triplet import bottleneck_network
    frames, boxes, scores, lm = _hand_made()
    found = gather_faces(frames, boxes, scores, lm, margin=4, size=112)
    assert found.crops.shape[0] == 8 > embedder.max_batch
    ff = embed_and_match(found, embedder)
    assert torch.equal(ff.emb, _chunkwise(embedder, found.crops)) and ff.idx is None
    assert torch.equal(ff.crops, found.crops) and torch.equal(ff.offsets, found.offsets)
    three = bottleneck_network('resnet', emd_size=512, input_shape=(112, 112, 3), max_batch=3)('v2')
    three.set_weights(embedder.get_weights())
    three.set_input_transform(scale=1 / 255.)
    gal = _planted_gallery(_chunkwise(three, found.crops))
    ff3 = embed_and_match(found, three, gal, 1)
    assert torch.equal(ff3.emb, _chunkwise(three, found.crops))
    assert ff3.idx.tolist() == list(range(10, 10 + 3 * 8, 3)) or torch.equal(ff3.idx, gal.match(ff3.emb, 1)[0])
    assert _same_bits(ff3.dist, gal.match(ff3.emb, 1)[1]) and not bool((ff3.dist >= 1e-3).any())
    three.close()
    gal.close()
