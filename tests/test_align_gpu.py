"""Five-point landmark alignment on the device (csrc/align.hip) against the NumPy restatements of tests/align_ref.py:
the warp bit for bit, the fitted matrix to 1e-3 pixel of a float64 fit, the cascade's landmarks against a restatement
assembled here from the oracle's public pieces, and the aligned pipeline end to end.  PARITY WITH cv2.warpAffine IS
UNPINNED (cv2 is not installed; its warp works on a 1/32-pixel grid with 15-bit weights): what is pinned is the float32
arithmetic include/dif.h writes out."""
import numpy as np
import pytest
import torch

import align_ref as ar
from oracle import mtcnn as om
from test_mtcnn import _frames, _synth

pytestmark = pytest.mark.gpu

H, W = 37, 53


@pytest.fixture(scope='module')
def small_frames():
    return np.random.default_rng(37).integers(0, 256, (3, H, W, 3), dtype=np.uint8)


def _rot(scale, deg, ox, oy):
    return ar.similarity(scale, deg, ox, oy).reshape(6)


def _matrices(oh, ow):
    """Output pixel -> frame position, one row per case."""
    nan, inf = float('nan'), float('inf')
    rows = [
        [1, 0, 0, 0, 1, 0],                               # 0: identity
        [1, 0, -3, 0, 1, 2],                              # integer translations: the zero border shows left / bottom
        [1, 0, 5, 0, 1, -4],
        [1, 0, W - ow, 0, 1, H - oh],                     # the last output column / row sample x0 = W - 1, y0 = H - 1
        [1, 0, W - ow + 0.5, 0, 1, H - oh + 0.25],        # ... and straddle the edge: x0 = W - 1, tap x0 + 1 outside
        [1, 0, -0.75, 0, 1, -0.5],                        # x0 = -1: only the taps at 0 are inside
        _rot(0.5, 30, 10.3, -2.6),
        _rot(2.0, 30, 20.25, -3.5),
        _rot(0.37, -112, 30.1, 30.2),
        [1, 0, 1000, 0, 1, 0],                            # wholly off the frame
        [1, 0, 0, 0, 1, -1e30],
        [1, 0, nan, 0, 1, 0],
        [1, nan, 0, 0, 1, 0],
        [inf, 0, 0, 0, 1, 0],
    ]
    return np.array(rows, dtype=np.float32)


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('out_hw', [(16, 16), (112, 112), (20, 28), (5, 7)])     # 5 x 7: no multiple of four pixels -> byte stores
def test_warp_bit_for_bit(cuda, small_frames, out_hw, k):
    from deep_insight_face.detector.align import warp_affine
    pool = _matrices(*out_hw)
    n = small_frames.shape[0]
    per = n * k
    seen = 0
    for lo in range(0, len(pool), per):
        m = pool[[(lo + i) % len(pool) for i in range(per)]]
        got = warp_affine(small_frames, m.reshape(n, k, 2, 3), out_hw, k=k)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (per,) + out_hw + (3,)
        got = got.cpu().numpy()
        want = ar.warp_affine(small_frames, m, out_hw, k=k)
        assert np.array_equal(got, want), (lo, np.argwhere(got != want)[:4])
        for i in range(per):
            case, frame = (lo + i) % len(pool), small_frames[i // k]
            if case == 0:                                  # identity: the frame's top-left block, zeros beyond the frame
                hh, ww = min(out_hw[0], H), min(out_hw[1], W)
                assert np.array_equal(got[i, :hh, :ww], frame[:hh, :ww])
                assert not got[i, hh:].any() and not got[i, :, ww:].any()
            if case == 1:
                hh, ww = min(out_hw[0], H - 2), min(out_hw[1] - 3, W)
                assert np.array_equal(got[i, :hh, 3:3 + ww], frame[2:2 + hh, :ww]) and not got[i, :, :3].any()
            if case == 3:
                assert np.array_equal(got[i, -1, -1], frame[-1, -1])
            if case >= 9:
                assert not got[i].any(), case
            elif case != 8:
                assert got[i].any(), case
            seen += 1
    assert seen >= len(pool)


def test_warp_accepts_flat_matrices_and_device_tensors(cuda, small_frames):
    from deep_insight_face.detector.align import warp_affine
    m = _matrices(16, 16)[[6, 7, 1]]
    a = warp_affine(small_frames, m, (16, 16))
    b = warp_affine(torch.from_numpy(small_frames).to(cuda), torch.from_numpy(m).to(cuda).reshape(3, 2, 3).double(), (16, 16))
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), ar.warp_affine(small_frames, m, (16, 16)))


# ------------------------------------------------------------------------------------------------ the fit
def _fit_cases(rng, count, jitter):
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112 as T
    lms = []
    for i in range(count):
        s = float(np.exp(rng.uniform(np.log(0.15), np.log(5.0))))
        if i == 0:
            s = 0.15
        if i == 1:
            s = 5.0
        deg = float(rng.uniform(-70, 70)) if i > 3 else (-70.0, 70.0, 0.0, 33.0)[i]
        tx, ty = rng.uniform(0, 640), rng.uniform(0, 480)
        p = ar.apply(ar.similarity(s, deg, tx, ty), T - T.mean(0))          # the face's centre lies inside 480 x 640
        if jitter:
            p = p + rng.normal(0, 0.03 * 35 * s, p.shape)                   # ~3 % of the eye-to-mouth distance
        lms.append(p)
    return np.asarray(lms, dtype=np.float32)


@pytest.fixture(scope='module')
def big_frames():
    return np.random.default_rng(480).integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)


@pytest.mark.parametrize('jitter', [False, True])
@pytest.mark.parametrize('size', [112, 56])
def test_fit_against_float64_and_crop_through_the_reported_matrix(cuda, big_frames, size, jitter):
    """The device's float32 closed form against the float64 fit on the output's four corners: at most 1e-3 pixel in the
    frame (a float32 NumPy evaluation of the same formula stays within 1.6e-4 over 200 000 such cases; the device's
    division may round differently; cv2 itself works on a 1/32-pixel grid).  The crop: the restated warp through the
    matrix the device reported, bit for bit."""
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112 as T, align_faces
    k = 12
    lm = _fit_cases(np.random.default_rng(size + jitter), 2 * k, jitter)
    crops, mats = align_faces(big_frames, lm, size=size, k=k, return_matrices=True)
    assert tuple(crops.shape) == (2 * k, size, size, 3) and crops.dtype == torch.uint8 and tuple(mats.shape) == (2 * k, 2, 3)
    crops, mats = crops.cpu().numpy(), mats.cpu().numpy()
    tpl = (T * np.float32(size / 112.0)).astype(np.float32)
    corners = np.array([[0, 0], [size - 1, 0], [0, size - 1], [size - 1, size - 1]], np.float64)
    worst = 0.0
    for i in range(2 * k):
        want = ar.fit(lm[i], tpl)
        worst = max(worst, float(np.abs(ar.apply(mats[i], corners) - ar.apply(want, corners)).max()))
    print('fit: worst corner difference %.3g pixel (size %d, jitter %s)' % (worst, size, jitter))
    assert worst <= 1e-3
    assert np.array_equal(crops, ar.warp_affine(big_frames, mats, (size, size), k=k))
    assert all(c.any() for c in crops[[2, 3]])                     # (scale ~1 faces around the frame's middle are not black)
    # an explicit template equal to the default one, and a device tensor of landmarks [N, k, 5, 2]: the same crops
    again = align_faces(big_frames, torch.from_numpy(lm).to(cuda).reshape(2, k, 5, 2), size=size, template=tpl, k=k)
    assert np.array_equal(again.cpu().numpy(), crops)


def test_fit_degenerate_cases_are_black(cuda, big_frames):
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112 as T, align_faces
    good = ar.apply(ar.similarity(1.4, 10, 300, 200), T - T.mean(0)).astype(np.float32)
    lm = np.stack([good] * 8)
    lm[1] = lm[1, 0]                                                # five equal points
    lm[2, 3, 1] = np.nan                                            # a NaN landmark
    lm[5, 0, 0] = np.inf
    valid = np.array([0.9, 0.9, 0.9, -1.0, 0.0, 0.9, 0.5, -1.0], np.float32)
    crops, mats = align_faces(big_frames, lm, valid=valid, k=4, return_matrices=True)
    crops, mats = crops.cpu().numpy(), mats.cpu().numpy()
    for i in range(8):
        if i in (1, 2, 3, 5, 7):
            assert not crops[i].any() and np.isnan(mats[i]).all(), i
        else:
            assert crops[i].any() and np.isfinite(mats[i]).all(), i
    assert np.array_equal(mats[0], mats[4]) and not np.array_equal(crops[0], crops[4])     # same face position, other frame
    plain = align_faces(big_frames, lm, k=4).cpu().numpy()          # without `valid` the empty slots are ordinary faces
    assert plain[3].any() and plain[7].any() and np.array_equal(plain[0], crops[0])
    assert not align_faces(big_frames, lm, template=np.tile(T[:1], (5, 1)), k=4).cpu().numpy().any()     # a one-point template


def test_white_dots_land_on_the_template(cuda):
    """Independent of the restatement's reading (a forward / inverse or x / y mix-up would be repeated there): dots drawn
    at the template's points under a known similarity come out on the template's points, each on its own."""
    from deep_insight_face import api
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112 as T, align_faces
    fwd = ar.similarity(1.3, 20, 40.0, -50.0)                       # template -> frame
    pts = ar.apply(fwd, T)
    assert (pts[:, 0] > 2).all() and (pts[:, 0] < 157).all() and (pts[:, 1] > 2).all() and (pts[:, 1] < 117).all()
    for d in range(5):
        frame = np.zeros((1, 120, 160, 3), np.uint8)
        cx, cy = int(round(pts[d, 0])), int(round(pts[d, 1]))
        frame[0, cy - 1:cy + 2, cx - 1:cx + 2] = 255
        crop = align_faces(frame, pts[None].astype(np.float32), size=112)[0].cpu().numpy()
        assert crop.shape == (112, 112, 3) and crop.max() > 100
        ys, xs = np.nonzero(crop[..., 0] == crop[..., 0].max())
        assert abs(xs.mean() - T[d, 0]) <= 1.0 and abs(ys.mean() - T[d, 1]) <= 1.0, (d, xs, ys, T[d])
        assert np.array_equal(api.align_face(frame[0], pts), crop)


# ------------------------------------------------------------------------------------------------ the cascade
CASCADE_HW, CASCADE_N, CASCADE_CAP, CASCADE_SEED = (96, 128), 3, (24, 12, 8), 12


@pytest.fixture(scope='module')
def cascade():
    """Frames, weights, the oracle's cascade and the landmarks expected of every output slot, assembled from the oracle's
    public pieces: O-Net on the stage-2 slots, its face probability and plain regression, the last suppression, and the
    landmark decode on the stage-2 boxes (the ones O-Net's crops were cut from) gathered through it."""
    p = _synth()
    h, w = CASCADE_HW
    frames = _frames(CASCADE_N, h, w, seed=CASCADE_SEED)
    ob, os_, dbg = om.detect(frames, p, cap=CASCADE_CAP)
    lms, overhang = [], 0
    for f in range(CASCADE_N):
        b2, s2 = dbg['stage2_boxes'][f], dbg['stage2_scores'][f]
        o = om.onet(om.normalise(om.crops_of(frames[f], b2, s2, 48)), p['onet'])
        pr = om.face_prob(o[:, 0:2])
        s = np.where((s2 >= 0) & (pr >= np.float32(0.7)), pr, np.float32(-1.0)).astype(np.float32)
        b = om.calibrate_plain(b2, o[:, 2:6].astype(np.float32))
        keep = om.nms_slots(b, s, CASCADE_CAP[2], 0.7)
        kb, ks, lm = om.gather_slots(keep, b, s, ar.decode_landmarks(o, b2, h, w))
        assert np.array_equal(kb, ob[f]) and np.array_equal(ks, os_[f])           # the assembly above IS the oracle's last stage
        lms.append(lm)
        overhang += sum(1 for i in keep[keep >= 0] if b2[i, 0] < 0 or b2[i, 1] < 0 or b2[i, 2] > w or b2[i, 3] > h)
    return dict(params=p, frames=frames, boxes=ob, scores=os_, dbg=dbg, landmarks=np.stack(lms), overhang=overhang)


def test_cascade_landmarks(cuda, cascade):
    from deep_insight_face.detector.mtcnn import MtcnnDetector
    det = MtcnnDetector(CASCADE_HW, max_batch=CASCADE_N, cap=CASCADE_CAP)
    det.set_weights(cascade['params'])
    b0, s0 = det.detect(cascade['frames'])
    b1, s1, lm, st = det.detect(cascade['frames'], return_stages=True, return_landmarks=True)
    b2, s2, lm2 = det.detect(cascade['frames'], return_landmarks=True)
    assert torch.equal(b0, b1) and torch.equal(s0, s1) and torch.equal(b0, b2) and torch.equal(s0, s2) and torch.equal(lm, lm2)
    assert tuple(lm.shape) == (CASCADE_N, CASCADE_CAP[2], 5, 2) and lm.dtype == torch.float32
    # the device walks the oracle's path on these frames (as test_cascade_vs_oracle asserts for its own)
    assert np.array_equal(st['stage2_boxes'].cpu().numpy(), np.stack(cascade['dbg']['stage2_boxes']))
    gs, lm = s0.cpu().numpy(), lm.cpu().numpy()
    live = cascade['scores'] >= 0
    assert np.array_equal(gs >= 0, live) and live.sum() >= CASCADE_N
    assert not lm[~live].any()                                     # an empty slot: ten zeros
    assert (~live).any() and (np.abs(lm[live]).sum((1, 2)) > 0).all()
    assert cascade['overhang'] >= 1                                # the clamped-rectangle rule is exercised
    print('cascade landmarks: worst difference %.3g pixel, %d overhanging slots' % (np.abs(lm - cascade['landmarks']).max(),
                                                                                   cascade['overhang']))
    np.testing.assert_allclose(lm, cascade['landmarks'], rtol=1e-5, atol=1e-3)
    det.close()


# ------------------------------------------------------------------------------------------------ the pipeline
def test_aligned_pipeline_and_detection_wrapper(cuda):
    from deep_insight_face import oneshot
    from deep_insight_face.detector.align import align_faces
    from deep_insight_face.detector.mtcnn import MtcnnDetection, MtcnnDetector, MtcnnFramePipeline
    from deep_insight_face.detector.run import crop_faces
    from deep_insight_face.networks.triplet import DifEmbedder
    hw, n = (96, 128), 5
    frames = _frames(n, hw[0], hw[1], seed=5)
    t = torch.from_numpy(frames).to(cuda)
    det = MtcnnDetector(hw, max_batch=2, cap=(24, 12, 8)).init_synthetic(7)
    emb = DifEmbedder('resnet', 'v2', 512, (112, 112, 3), max_batch=8).init_synthetic(3)
    emb.set_input_transform(scale=1 / 255.)
    off = MtcnnFramePipeline(det, emb, None, margin=8)
    on = MtcnnFramePipeline(det, emb, None, margin=8, align=True)
    # align=False: what the pipeline gave before (box crop with a margin through crop_faces), output by output
    bx, sc, e = off(frames)
    assert len(off.detect(t)) == 2
    want_e = emb.embed(crop_faces(t, bx, 8, 112))
    assert torch.equal(e, want_e) and torch.equal(off.crops(t)[2], crop_faces(t, bx, 8, 112))
    # align=True
    abx, asc, lm = on.detect(t)
    assert torch.equal(abx, bx) and torch.equal(asc, sc) and tuple(lm.shape) == (n, 5, 2) and bool(torch.isfinite(lm).all())
    full = torch.cat([det.detect(t[lo:lo + 2], return_landmarks=True)[2] for lo in range(0, n, 2)])
    assert torch.equal(lm, full[:, 0])
    crops = on.crops(t)[2]
    assert tuple(crops.shape) == (n, 112, 112, 3) and torch.equal(crops, align_faces(frames, lm))
    assert not torch.equal(crops, off.crops(t)[2])
    abx2, asc2, ae = on(frames)
    assert torch.equal(abx2, bx) and torch.equal(asc2, sc) and tuple(ae.shape) == (n, 512) and torch.equal(ae, emb.embed(crops))
    gal = oneshot.Gallery(ae)
    _, _, _, idx, _ = MtcnnFramePipeline(det, emb, gal, margin=8, align=True)(frames)
    assert idx.tolist() == list(range(n))
    # nothing detected: black crops, NaN landmarks, no exception
    quiet = MtcnnDetector(hw, max_batch=2, cap=(24, 12, 8), thresholds=(0.6, 0.7, 1.1))
    quiet.set_weights(det.get_weights())
    qp = MtcnnFramePipeline(quiet, emb, None, align=True)
    qb, qs, ql = qp.detect(t)
    assert bool(torch.isnan(qb).all()) and bool(torch.isnan(ql).all()) and not qs.any()
    assert not qp.crops(t)[2].any()
    assert tuple(qp(frames)[2].shape) == (n, 512)
    # the reference's detector call, aligned
    crops1, boxes1 = MtcnnDetection(model=det, margin=8, align=True)(frames[0])
    plain1, boxes0 = MtcnnDetection(model=det, margin=8)(frames[0])
    assert len(crops1) == 1 and crops1[0].shape == (112, 112, 3) and crops1[0].dtype == np.uint8
    assert np.array_equal(crops1[0], crops[0].cpu().numpy()) and np.array_equal(boxes1[0], boxes0[0])
    many, mboxes = MtcnnDetection(model=det, margin=8, detect_multiple_faces=True, align=True, size=64)(frames[0])
    assert len(many) == len(mboxes) >= 1 and all(c.shape == (64, 64, 3) for c in many)
    with pytest.raises(ValueError, match='Bounding box not found'):
        MtcnnDetection(model=quiet, align=True)(frames[0])
    for m in (det, quiet, emb, gal):
        m.close()
