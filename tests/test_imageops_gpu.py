"""GPU letterbox / crop+resize kernels vs the oracle (oracle/imageops.py) and the device-resident
frames -> detect -> crop -> embed -> match pipeline (BASELINE configs[4])."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    # smooth-ish content plus noise so that resampling is exercised on gradients and on edges
    yy, xx = np.mgrid[0:h, 0:w]
    base = (127 + 100 * np.sin(xx / 17.0)[None] * np.cos(yy / 11.0)[None])[..., None]
    noise = rng.integers(-40, 40, size=(n, h, w, 3))
    return np.clip(base + noise, 0, 255).astype(np.uint8)


# (h, w, canvas) -> the reference's resized extent (nw, nh), i.e. int(w * scale), int(h * scale) with scale = min(size / w,
# size / h) in Python's floats.  At every one of these sizes the same statements in float32 give one pixel more or less on an
# axis (tests/test_letterbox_extent.py), and with it another scale, offset and grey bar: the whole frame differs from PIL's.
EXTENTS = {(360, 640, 416): (416, 234), (1280, 720, 416): (234, 416), (288, 352, 416): (416, 340), (576, 720, 416): (415, 332),
           (11, 11, 416): (416, 416), (23, 23, 416): (415, 415), (20, 41, 64): (64, 31), (20, 49, 64): (63, 26),
           (42, 56, 608): (608, 456), (20, 77, 320): (319, 83), (720, 1280, 416): (416, 234), (270, 3840, 416): (416, 29),
           (36, 64, 416): (416, 234)}


def _letterbox_gates(got, want, what):
    """The gates of the letterbox against PIL: at most one grey level per value, more than 98 % of the values equal -- what
    arithmetic in another number format than PIL's 22-bit fixed point can hold (a rounding flips by one level).  A tap short
    at a bound or the outermost tap dropped leaves at most 65 % equal, with errors of up to 81 levels; a wrong extent 49 %
    and 72 levels.  test_letterbox_equals_pil_bytes asks for PIL's bytes at a few sizes."""
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print('letterbox %s: max |diff| %d, equal %.4f %%' % (what, diff.max(), 100.0 * (diff == 0).mean()))
    assert diff.max() <= 1
    assert (diff == 0).mean() > 0.98


def _letterbox_vs_pil(frames, size):
    from deep_insight_face.detector.yolov3 import letterbox_batch, letterbox_extent
    from oracle import imageops
    h, w = frames.shape[1:3]
    if (h, w, size) in EXTENTS:
        assert letterbox_extent(h, w, size) == EXTENTS[(h, w, size)]
    got = letterbox_batch(frames, size).cpu().numpy()
    want = np.stack([imageops.letterbox(f, size) for f in frames])
    if (h, w, size) in EXTENTS:                       # PIL's picture lies where the table says: the bars are exactly grey
        nw, nh = EXTENTS[(h, w, size)]
        x0, y0 = (size - nw) // 2, (size - nh) // 2
        for a in (got, want):
            inside = np.zeros((size, size), dtype=bool)
            inside[y0:y0 + nh, x0:x0 + nw] = True
            assert (a[:, ~inside] == 128).all(), 'a grey bar is not where the extent puts it'
    _letterbox_gates(got, want, '%d x %d x %d -> %d' % (frames.shape[0], h, w, size))


@pytest.mark.parametrize('h,w,size', [(480, 640, 416), (300, 200, 416), (96, 128, 64), (416, 416, 416),
                                      # sizes at which a float32 extent is a pixel off the reference's
                                      (360, 640, 416), (1280, 720, 416), (288, 352, 416), (576, 720, 416), (11, 11, 416),
                                      (23, 23, 416), (20, 41, 64), (20, 49, 64), (42, 56, 608), (20, 77, 320)])
def test_letterbox_matches_pil(h, w, size):
    _letterbox_vs_pil(_frames(3, h, w, 5), size)


@pytest.mark.parametrize('h,w,size', [(720, 1280, 416),      # the workload's own frame size
                                      (270, 3840, 416)])     # column centres beyond 2^11 in float32
def test_letterbox_matches_pil_one_frame(h, w, size):
    _letterbox_vs_pil(_frames(1, h, w, 6), size)


@pytest.mark.parametrize('h,w,size', [(11, 11, 416), (36, 64, 416), (360, 640, 416), (300, 200, 416), (96, 128, 64),
                                      (50, 70, 101), (97, 61, 45),      # canvases that are no multiple of the 32 x 8 tile
                                      (100, 1000, 200)])                # more taps per column than the kernel tabulates
def test_letterbox_equals_pil_bytes(h, w, size):
    """The kernel restates PIL's 8-bit resampling -- double weights, 22-bit fixed-point coefficients, int32 sums, an 8-bit
    intermediate between the passes -- so enlarged, shrunk and mixed frames come out as PIL's own bytes.  (Float32 weights
    were two grey levels off PIL on a few values of the two enlarged sizes here.)"""
    from deep_insight_face.detector.yolov3 import letterbox_batch
    from oracle import imageops
    frames = _frames(26 if (h, w) == (36, 64) else 3, h, w, 12 if (h, w) == (36, 64) else 5)
    got = letterbox_batch(frames, size).cpu().numpy()
    want = np.stack([imageops.letterbox(f, size) for f in frames])
    assert np.array_equal(got, want), int((got != want).sum())


def test_letterbox_batch_matches_letterbox_image():
    """The device path and the package's own per-image path (PIL) agree at a size where float32 and double extents differ."""
    from PIL import Image
    from deep_insight_face.detector.yolov3 import letterbox_batch, letterbox_image
    frames = _frames(2, 360, 640, 8)
    got = letterbox_batch(frames, 416).cpu().numpy()
    want = np.stack([np.array(letterbox_image(Image.fromarray(f), (416, 416))) for f in frames])
    _letterbox_gates(got, want, 'letterbox_image 360 x 640')


def test_letterbox_second_trip_of_the_grid_stride_loop():
    """letterbox_kernel launches at most 16 384 blocks, each on tiles of 32 x 8 = 256 pixels: 26 canvases of 416 x 416 are
    17 576 tiles, so the last frames are written on the loop's second trip.  Every frame has its own content and is held to
    PIL."""
    n, size = 26, 416
    assert n * (size // 32) * (size // 8) > 16384 >= (n - 2) * (size // 32) * (size // 8) and size % 32 == 0
    frames = _frames(n, 36, 64, 12)
    assert len({f.tobytes() for f in frames}) == n
    _letterbox_vs_pil(frames, size)


def test_crop_second_trip_of_the_grid_stride_loop():
    """crop_resize_kernel likewise: 340 crops of 112 x 112 are 16 660 blocks' worth.  Small frames and boxes that enlarge keep
    the checker on its vectorised linear path; every crop equals the oracle's."""
    from deep_insight_face.detector.run import crop_faces
    from oracle import imageops
    n, size, H, W = 340, 112, 24, 32
    assert (n * size * size + 255) // 256 > 16384 >= ((n - 6) * size * size + 255) // 256
    rng = np.random.default_rng(13)
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    l, t = rng.uniform(0, 20, n), rng.uniform(0, 14, n)
    boxes = np.stack([l, t, l + rng.uniform(2, 14, n), t + rng.uniform(2, 12, n)], axis=1).astype(np.float32)
    got = crop_faces(frames, boxes, 8, size).cpu().numpy()
    bad = [i for i in range(n) if not np.array_equal(got[i], imageops.crop_resize(frames[i], boxes[i], 8, size))]
    assert not bad, bad[:10]
    assert got[-1].any()


def _edge_boxes(margin, H, W):
    """Boxes (left, top, right, bottom) around everything crop_pixel's rectangle does -- margin / 2 per side in float32, clamp,
    truncate to int32: coordinates on integers, one float32 step above and below an integer before and after the margin is
    applied (also where adding the margin crosses a binade and rounds), on and beyond the frame's edges, empty and inverted
    rectangles, infinities, rectangles of one and two source pixels.
    Boxes that lie wholly left of or above the frame (right + margin / 2 <= -1) are left out: the reference slices
    frame[t:b, l:r] with a negative stop there, which Python counts from the far end."""
    f32 = np.float32
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    dn = lambda v: np.nextafter(f32(v), f32(-np.inf))
    base = (10, 8, 50, 40)
    per_axis = [
        [up(10), dn(10), up(16), dn(16), 0, up(0), dn(0), -0.5, -3.25, 49, dn(50), 50, up(50), 79.5, 90],        # left
        [up(8), dn(8), up(16), dn(16), 0, -0.75, 39, dn(40), 40, up(40), 70],                                    # top
        [up(50), dn(50), up(32), dn(32), up(30), dn(30), W, up(W), dn(W), W + 5.5, 11, up(10), 10, dn(11), 5],   # right
        [up(40), dn(40), up(32), dn(32), up(30), dn(30), H, up(H), dn(H), H + 6.25, 9, up(8), 8, dn(9), 3],      # bottom
    ]
    rects = [base]
    for axis, values in enumerate(per_axis):
        for v in values:
            r = list(base)
            r[axis] = v
            rects.append(tuple(r))
    rects += [(20, 5, 21, 45), (5, 20, 70, 21),                      # 1 x N and N x 1 source pixels
              (33, 17, 34, 18), (33, 17, 35, 19),                    # 1 x 1, 2 x 2
              (W - 1, H - 1, W, H), (0, 0, 1, 1), (W - 2, H - 2, W + 5, H + 6),     # the same in the frame's corners
              (0, 0, W, H), (-4, -4, W + 4, H + 4),                  # the whole frame
              (30, 10, 30, 40), (10, 20, 50, 20),                    # left == right, top == bottom
              (50, 10, 30, 40), (10, 40, 50, 8),                     # right < left, bottom < top
              (-5, 8, -0.5, 40), (10, -5, 50, -0.25),                # ends at column / row 0: empty
              (W, 8, W + 9, 40), (10, H + 1, 50, H + 9)]             # wholly right of / below the frame
    half = f32(margin) / f32(2)
    rects = np.array(rects, dtype=np.float32)
    shrunk = rects + np.array([half, half, -half, -half], dtype=np.float32)      # the rectangle is `rects` AFTER the margin
    # infinities and 1e30 on the sides where the clamp catches them (the other way round the value reaches the cast to int32
    # unclamped, which neither NumPy nor C defines)
    inf, big = np.inf, 1e30
    wild = np.array([(-inf, 8, 50, 40), (10, -inf, 50, 40), (10, 8, inf, 40), (10, 8, 50, inf), (-inf, -inf, inf, inf),
                     (10, 8, big, big), (-big, -big, 50, 40), (-big, -inf, inf, big)], dtype=np.float32)
    boxes = np.concatenate([rects, shrunk, wild]).astype(np.float32)
    keep = (boxes[:, 2] + half > -1) & (boxes[:, 3] + half > -1)
    assert keep.all()
    return boxes


@pytest.mark.parametrize('size', [112, 16])
@pytest.mark.parametrize('margin', [0, 7, 8])
def test_crop_rectangle_edges(margin, size):
    from deep_insight_face.detector.run import crop_faces
    from oracle import imageops
    H, W = 64, 80
    frame = np.random.default_rng(21).integers(0, 256, (H, W, 3), dtype=np.uint8)
    boxes = _edge_boxes(margin, H, W)
    frames = np.ascontiguousarray(np.broadcast_to(frame, (len(boxes), H, W, 3)))
    got = crop_faces(frames, boxes, margin, size).cpu().numpy()
    bad, black = [], 0
    for i, b in enumerate(boxes):
        want = imageops.crop_resize(frame, b, margin, size)
        black += not want.any()
        if not np.array_equal(got[i], want):
            bad.append((i, b.tolist(), int(np.abs(got[i].astype(np.int32) - want).max())))
    assert not bad, (len(bad), bad[:6])
    assert 8 <= black <= len(boxes) // 2              # empty rectangles are there, and are not the rule


# crops (width, height in source pixels) of a 360 x 360 frame to 112 x 112, each with its origin inside the frame, so that
# the source pitch is not the crop's width and (left, top) != (0, 0)
PATH_CROPS = [(112, 112),      # identity
              (224, 224),      # 2 x 2 blocks
              (336, 336),      # 3 x 3: the other integer ratios
              (250, 250),      # fractional, both axes
              (112, 131), (131, 112),      # one axis exactly 1
              (224, 150), (150, 224),      # an integer ratio beside a fractional one
              (56, 56),        # exactly 2 x enlarged
              (113, 300), (300, 113),      # mixed
              (224, 100), (100, 224)]      # an integer shrink beside an enlarged axis: both take the linear path
PATH_K = 3


@functools.lru_cache(maxsize=None)
def _path_case():
    """5 frames, 3 slots each: the 13 crops above, then a slot with valid < 0 and a NaN box.  -> frames, boxes [5, 3, 4],
    valid [5, 3], and the oracle's crop of every slot's box from its frame (valid not applied; NaN: black)."""
    from oracle import imageops
    frames = _frames(5, 360, 360, 17)
    rng = np.random.default_rng(17)
    boxes = np.empty((15, 4), dtype=np.float32)
    for j, (cw, ch) in enumerate(PATH_CROPS):
        l, t = int(rng.integers(1, 360 - cw)), int(rng.integers(1, 360 - ch))
        boxes[j] = (l, t, l + cw, t + ch)
    boxes[13] = boxes[3]                              # a good box in a slot marked empty
    boxes[14] = (np.nan, 5, 100, 100)
    valid = np.linspace(0.2, 1.0, 15).astype(np.float32)
    valid[13] = -1.0
    want = np.stack([np.zeros((112, 112, 3), np.uint8) if np.isnan(boxes[j, 0]) else
                     imageops.crop_resize(frames[j // PATH_K], boxes[j], 0, 112) for j in range(15)])
    boxes, valid = boxes.reshape(5, PATH_K, 4), valid.reshape(5, PATH_K)
    for a in (frames, boxes, valid, want):            # computed once, shared by the tests below, never changed
        a.setflags(write=False)
    return frames, boxes, valid, want


def test_crop_paths_with_an_origin_inside_the_frame():
    """dif_crop_resize on every resampling path, pitch != crop width."""
    from deep_insight_face.detector.run import crop_faces
    frames, boxes, _, want = _path_case()
    flat = boxes.reshape(-1, 4)
    assert (flat[:13, :2] > 0).all() and (flat[:13, 2:] < 360).all()
    got = crop_faces(frames[np.arange(15) // PATH_K], flat, 0, 112).cpu().numpy()
    bad = [(j, int(np.abs(got[j].astype(np.int32) - want[j]).max())) for j in range(15) if not np.array_equal(got[j], want[j])]
    assert not bad, bad
    assert all(want[j].any() for j in range(14)) and not want[14].any()


def test_crop_multi_and_list_match_the_oracle(cuda):
    """dif_crop_resize_multi (frame = slot / K, the valid flag) and dif_crop_resize_list (any order, -1 entries) against the
    oracle itself, slot by slot, on every resampling path."""
    from deep_insight_face import _native as N
    from deep_insight_face.detector.faces import crop_faces_list
    frames, boxes, valid, want = _path_case()
    t, b, v = (torch.from_numpy(a.copy()).to(cuda) for a in (frames, boxes, valid))
    got = torch.full((15, 112, 112, 3), 7, dtype=torch.uint8, device=cuda)
    N.check(N.lib.dif_crop_resize_multi(N.ptr(t), 5, 360, 360, N.ptr(b), N.ptr(v), PATH_K, 0.0, N.ptr(got), 112, N.stream_ptr()))
    got = got.cpu().numpy()
    for j in range(15):
        w = np.zeros_like(want[j]) if j == 13 else want[j]             # slot 13: valid < 0 -> black
        assert np.array_equal(got[j], w), (j, int(np.abs(got[j].astype(np.int32) - w).max()))
    perm = np.random.default_rng(3).permutation(15)
    f, s = np.divmod(perm.astype(np.int32), PATH_K)
    f, s = np.insert(f, 4, -1).astype(np.int32), np.insert(s, 4, -1).astype(np.int32)
    got = crop_faces_list(t, b, f, s, 0, 112).cpu().numpy()
    for i in range(16):
        w = np.zeros_like(want[0]) if f[i] < 0 else want[f[i] * PATH_K + s[i]]     # the list form takes no valid flag
        assert np.array_equal(got[i], w), (i, int(f[i]), int(s[i]))


def test_crop_resize_matches_oracle():
    from deep_insight_face.detector.run import crop_faces
    from oracle import imageops
    frames = _frames(6, 240, 320, 7)
    boxes = np.array([[40.3, 30.9, 200.2, 180.7],      # shrink
                      [100.0, 100.0, 150.0, 160.0],    # enlarge
                      [-20.0, -10.0, 400.0, 300.0],    # clamped to the frame
                      [10.0, 20.0, 122.0, 132.0],      # 112 + margin: integer scale
                      [50.0, 50.0, 50.0, 90.0],        # zero width after margin 0 -> see below
                      [np.nan] * 4], dtype=np.float32)
    for margin in (8, 0):
        got = crop_faces(frames, boxes, margin, 112).cpu().numpy()
        for i in range(6):
            if np.isnan(boxes[i, 0]):
                assert not got[i].any()
                continue
            want = imageops.crop_resize(frames[i], boxes[i], margin, 112)
            # round 4: oracle and kernel both follow cv2's uint8 INTER_AREA paths operation by operation -> equal
            assert np.array_equal(got[i], want), (i, margin, int(np.abs(got[i].astype(np.int32) - want).max()))


@pytest.mark.parametrize('nframes,h,w', [(4, 240, 320), (96, 480, 640), (256, 480, 640)])
def test_frame_pipeline_end_to_end(nframes, h, w):
    """Device pipeline == the same stages run one by one through the host-visible API; at 4 small frames and
    at 96 and at 256 frames (= BASELINE configs[4]'s batch) of its 640x480 (the detector then runs in chunks of
    its max_batch = 64, the embedder splits its batch over two lanes...)."""
    from deep_insight_face import oneshot
    from deep_insight_face.detector import run as drun, yolov3 as yolo
    from deep_insight_face.networks.triplet import bottleneck_network
    from deep_insight_face.networks.weights import synth_params
    det = drun.yolo_v3_face(max_batch=min(nframes, 64))
    p = synth_params(det.param_spec(), seed=11)
    for k in p:                                   # keep exp() in the box decode finite
        if k in ('conv_58/kernel', 'conv_66/kernel', 'conv_74/kernel'):
            p[k] = p[k] * 1e-5
        if k in ('conv_58/bias', 'conv_66/bias', 'conv_74/bias'):
            p[k] = np.zeros_like(p[k])
            p[k][4::6] = 2.0
            p[k][5::6] = 2.0
    det.set_weights(p)
    det.set_input_transform(scale=1 / 255.)
    emb = bottleneck_network('resnet', emd_size=512, input_shape=(112, 112, 3), max_batch=nframes)('v2')
    emb.init_synthetic(3)
    emb.set_input_transform(scale=1 / 255.)
    rng = np.random.default_rng(0)
    gal = rng.standard_normal((1000, 512)).astype(np.float32)
    pipe = drun.FramePipeline(det, emb, oneshot.Gallery(gal), margin=8, score=0.4)
    frames = _frames(nframes, h, w, 9)
    boxes, scores, e, idx, dist = pipe(frames)
    boxes, scores = boxes.cpu().numpy(), scores.cpu().numpy()
    assert np.isfinite(boxes).all() and (scores >= 0.4).all()
    # stage by stage
    lb = yolo.letterbox_batch(frames, 416)
    maps = det.embed(lb)
    for i in range(0, nframes, max(1, nframes // 8)):
        b, s, c = yolo.get_yolo_output([m[i:i + 1] for m in maps], drun.ANCHORS.reshape(-1, 2), 1, (h, w),
                                       max_boxes=1, score_threshold=0.4)
        top, left, bottom, right = b[0]
        np.testing.assert_allclose(boxes[i], [left, top, right, bottom], rtol=0, atol=0)
        np.testing.assert_allclose(scores[i], s[0], rtol=0, atol=0)
    crops = drun.crop_faces(frames, boxes, 8, 112)
    e2 = emb.embed(crops)
    assert torch.equal(e, e2)
    i2, d2 = oneshot.Gallery(gal).match(e2, 1)
    assert torch.equal(idx, i2) and torch.equal(dist, d2)
