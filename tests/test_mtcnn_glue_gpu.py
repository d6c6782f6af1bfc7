"""The three MTCNN glue entry points (csrc/mtcnn.hip) called directly on seeded arrays, without networks or cascade, against
oracle.mtcnn's float32 restatements: boxes, regression values and gathered scores bit for bit (mtcnn.hip is built without
FMA contraction for this), probabilities to atol 2e-6 (expf on the device, np.exp on the host; tests/test_mtcnn.py's
tolerance for the same quantity).  A slot whose probability lies within 1e-6 of the threshold could fall on either side:
the inputs are moved away from it and the reference is asserted to hold no such slot before the kernel runs."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from oracle import mtcnn as om

F = np.float32
SENT = F(777.0)
PROB_ATOL = 2e-6


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def assert_bitwise(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == F and want.dtype == F, what
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (what, 'first difference at', bad[0], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


def clear_of_threshold(logits, thr, margin=1e-4):
    """Moves every slot whose reference probability is within `margin` of thr away from it (in place), then asserts on the
    reference that none lies within 1e-6.  logits [..., >= 2]."""
    near = np.abs(om.face_prob(logits[..., 0:2]) - F(thr)) < margin
    logits[..., 1][near] += F(1)
    p = om.face_prob(logits[..., 0:2])
    assert int((np.abs(p.astype(np.float64) - float(F(thr))) <= 1e-6).sum()) == 0
    return p


def assert_scores(got, want, what):
    """-1 exactly where the reference has -1 (the alive / dead decision), probabilities to PROB_ATOL elsewhere."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == F, what
    dead = want == F(-1)
    assert np.array_equal(got == F(-1), dead), (what, int((got == F(-1)).sum()), int(dead.sum()))
    np.testing.assert_allclose(got[~dead], want[~dead], rtol=0, atol=PROB_ATOL, err_msg=what)


# ------------------------------------------------------------------------------------------------ dif_mtcnn_propose
def propose_ref(head, scale, thr):
    res = [om.propose(h, scale, thr) for h in head]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def run_propose(head, scale, thr):
    from deep_insight_face import _native as N
    n, gh, gw, ld = head.shape
    cells = n * gh * gw
    boxes = torch.full((cells + 1, 4), float(SENT), dtype=torch.float32, device='cuda')      # one guard row each
    scores = torch.full((cells + 1,), float(SENT), dtype=torch.float32, device='cuda')
    h = _dev(head)
    rc = N.lib.dif_mtcnn_propose(N.ptr(h), n, gh, gw, ld, float(scale), float(thr), N.ptr(boxes), N.ptr(scores), N.stream_ptr())
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    boxes, scores = boxes.cpu().numpy(), scores.cpu().numpy()
    assert (boxes[-1] == SENT).all() and scores[-1] == SENT, 'guard row written'
    return boxes[:-1].reshape(n, gh * gw, 4), scores[:-1].reshape(n, gh * gw)


@pytest.mark.gpu
@pytest.mark.parametrize('n,ld', [(1, 6), (3, 8), (2, 16)])
@pytest.mark.parametrize('gh,gw', [(1, 1), (1, 7), (14, 21), (139, 187)])
def test_propose(cuda, gh, gw, n, ld):
    rng = np.random.default_rng(gh * 1000 + gw * 10 + n)
    head = (rng.standard_normal((n, gh, gw, ld), dtype=F) * F(2)).astype(F)
    clear_of_threshold(head, 0.6)
    for scale in (0.6, 0.6 * 0.709 ** 3):
        want_b, want_s = propose_ref(head, scale, 0.6)
        assert gh * gw < 100 or ((want_s == -1).sum() > 50 and (want_s >= 0).sum() > 50)
        got_b, got_s = run_propose(head, scale, 0.6)
        assert_bitwise(got_b, want_b, 'boxes at scale %r' % scale)
        assert_scores(got_s, want_s, 'scores at scale %r' % scale)


@pytest.mark.gpu
def test_propose_grid_stride_second_pass(cuda):
    """81 x 139 x 187 = 2 105 433 cells, just above the 8192 x 256 the launch covers in one pass."""
    n, gh, gw, ld = 81, 139, 187, 8
    assert 8192 * 256 < n * gh * gw < 8192 * 256 + 25993        # the smallest number of such frames that is above
    rng = np.random.default_rng(81)
    head = rng.standard_normal((n, gh, gw, ld), dtype=F)
    head[..., 0:2] *= F(2)
    clear_of_threshold(head, 0.6)
    want_b, want_s = propose_ref(head, 0.6, 0.6)
    got_b, got_s = run_propose(head, 0.6, 0.6)
    assert_bitwise(got_b, want_b, 'boxes')
    assert_scores(got_s, want_s, 'scores')


# ------------------------------------------------------------------------------------------------ dif_mtcnn_gather
def gather_ref(keep, boxes, scores, reg, calibrate):
    """keep [n, k]; boxes [n, n_src, 4]; scores [n, n_src]; reg [n, n_src, 4] or None -> boxes [n, k, 4], scores, reg."""
    n, k = keep.shape
    ob, os_, orr = np.zeros((n, k, 4), F), np.full((n, k), -1, F), np.zeros((n, k, 4), F)
    for f in range(n):
        kk = np.where(keep[f] < 0, -1, keep[f])
        r = reg[f] if reg is not None else np.zeros_like(boxes[f])
        b, s, g = om.gather_slots(kk, boxes[f], scores[f], r)
        if calibrate:
            live = kk >= 0
            b[live] = om.calibrate(b[live], g[live])
        ob[f], os_[f], orr[f] = b, s, g
    return ob, os_, orr


def keep_lists(rng, n, k, n_src, pattern):
    keep = rng.integers(0, n_src, (n, k)).astype(np.int32)
    if pattern == 'front':
        keep[:, :max(1, k // 3)] = -1
    elif pattern == 'middle':
        keep[:, k // 3:max(k // 3 + 1, 2 * k // 3)] = -1
    elif pattern == 'everywhere':
        keep[:] = -1
    elif pattern == 'scattered':
        keep[rng.random((n, k)) < 0.3] = -2                       # any negative index is an empty slot
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize('n,k,n_src', [(1, 1, 1), (1, 8, 8), (3, 8, 300), (3, 1, 25993), (1, 64, 64), (3, 64, 25993)])
def test_gather(cuda, n, k, n_src):
    from deep_insight_face import _native as N
    rng = np.random.default_rng(n * 100000 + k * 1000 + n_src % 997)
    corner = rng.integers(0, 600, (n, n_src, 2)).astype(F)
    boxes = np.concatenate([corner, corner + rng.integers(10, 200, (n, n_src, 2)).astype(F)], -1)
    scores = rng.random((n, n_src)).astype(F)
    head = (rng.standard_normal((n, n_src, 8), dtype=F) * F(0.2)).astype(F)      # a P-Net map: [logits 2 | box 4 | 0 0]
    far = rng.random((n, n_src)) < 0.3
    head[far, 2:4] -= F(3)                                        # corners far below zero after the regression ...
    head[~far, 2:4] -= (boxes[~far, 0:2] / (boxes[~far, 2:4] - boxes[~far, 0:2] + 1)).astype(F)   # ... and around zero
    reg4 = np.ascontiguousarray(head[..., 2:6])
    d_boxes, d_scores, d_head, d_reg4 = _dev(boxes), _dev(scores), _dev(head), _dev(reg4)
    # the regression values: their own [n_src][4] array; columns 2..5 of the head map (ld 8, the way mtcnn.py calls it); none
    head_reg = ctypes.c_void_p(d_head.data_ptr() + 2 * 4)
    sources = [(N.ptr(d_reg4), 4, reg4, 0), (N.ptr(d_reg4), 4, reg4, 1), (head_reg, 8, reg4, 0), (head_reg, 8, reg4, 1),
               (None, 4, None, 0)]
    # destinations, allocated once and refilled before every launch: boxes, scores, reg, each with one guard image behind
    dsts = [(n_dst, off) + tuple(torch.empty((n + 1, n_dst) + tail, dtype=torch.float32, device='cuda') for tail in ((4,), (), (4,)))
            for n_dst, off in ((k, 0), (k + 9, 5))]
    untouched = np.full((n, k, 4), SENT, F)
    negative = 0
    for pattern, (reg_ptr, reg_ld, reg, calibrate) in itertools.product(('front', 'middle', 'everywhere', 'scattered', 'none'),
                                                                       sources):
        keep = keep_lists(rng, n, k, n_src, pattern)
        d_keep = _dev(keep)
        want_b, want_s, want_r = gather_ref(keep, boxes, scores, reg, calibrate)
        negative += int((want_b < 0).sum())
        for (n_dst, off, db, ds, dr), with_reg in itertools.product(dsts, (True, False)):
            what = (pattern, 'src_reg %s ld %d' % ('NULL' if reg is None else 'given', reg_ld), 'calibrate %d' % calibrate,
                    'n_dst %d dst_offset %d' % (n_dst, off), 'dst_reg %s' % ('given' if with_reg else 'NULL'))
            for t in (db, ds, dr):
                t.fill_(float(SENT))
            rc = N.lib.dif_mtcnn_gather(N.ptr(d_keep), n, k, N.ptr(d_boxes), N.ptr(d_scores), reg_ptr, reg_ld, n_src, N.ptr(db),
                                        N.ptr(ds), N.ptr(dr) if with_reg else None, n_dst, off, calibrate, N.stream_ptr())
            assert rc == 0, (N.last_error(),) + what
            torch.cuda.synchronize()
            for name, t, want in (('boxes', db, want_b), ('scores', ds, want_s), ('reg', dr, want_r if with_reg else untouched)):
                got = t.cpu().numpy()
                assert_bitwise(got[:n, off:off + k], want, (name,) + what)
                got[:n, off:off + k] = SENT
                assert (got == SENT).all(), (name, 'written outside [dst_offset, dst_offset + k)') + what
    if n * k >= 24:
        assert negative > 0                                       # trunc toward zero was exercised below zero


def test_truncation_is_toward_zero_in_the_reference():
    """What the gather test relies on: a squared box with corners in (-1, 0) truncates to -0, not to -1."""
    b = np.array([[2, 2, 11, 11]], F)
    r = np.array([[-0.25, -0.27, 0.0, 0.0]], F)                   # x1 = 2 - 2.5 = -0.5, y1 = 2 - 2.7 = -0.7
    out = om.calibrate(b, r)
    assert out[0, 0] == 0 and out[0, 1] == 0 and np.signbit(out[0, 0]) and out[0, 2] == 11


# ------------------------------------------------------------------------------------------------ dif_mtcnn_rescore
def rescore_ref(out, scores, thr, boxes, plain):
    p = om.face_prob(out[:, 0:2])
    s = np.where((scores >= 0) & (p >= F(thr)), p, F(-1)).astype(F)
    reg = np.ascontiguousarray(out[:, 2:6]).astype(F)
    return s, reg, (om.calibrate_plain(boxes, reg) if plain else boxes)


def run_rescore(out, scores, thr, boxes, plain, pass_boxes=True):
    from deep_insight_face import _native as N
    slots, ld = out.shape
    d_out = _dev(out)
    ds = _dev(np.concatenate([scores, [SENT]]).astype(F))
    db = _dev(np.concatenate([boxes, np.full((1, 4), SENT, F)]))
    dr = torch.full((slots + 1, 4), float(SENT), dtype=torch.float32, device='cuda')
    rc = N.lib.dif_mtcnn_rescore(N.ptr(d_out), slots, ld, float(thr), N.ptr(ds), N.ptr(dr), N.ptr(db) if pass_boxes else None,
                                 int(plain), N.stream_ptr())
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    gs, gr, gb = ds.cpu().numpy(), dr.cpu().numpy(), db.cpu().numpy()
    assert gs[-1] == SENT and (gr[-1] == SENT).all() and (gb[-1] == SENT).all(), 'guard row written'
    return gs[:-1], gr[:-1], gb[:-1]


def rescore_inputs(slots, ld, seed, thr):
    rng = np.random.default_rng(seed)
    out = (rng.standard_normal((slots, ld), dtype=F) * F(1.5)).astype(F)
    scores = rng.random(slots).astype(F)
    scores[rng.random(slots) < 0.4] = F(-1)                       # dead before the network saw them
    scores[rng.random(slots) < 0.1] = F(0)                        # 0 is alive
    corner = rng.uniform(-20, 500, (slots, 2))
    boxes = np.concatenate([corner, corner + rng.uniform(8, 150, (slots, 2))], -1).astype(F)
    clear_of_threshold(out, thr)
    return out, scores, boxes


@pytest.mark.gpu
@pytest.mark.parametrize('ld', [6, 8, 16])
@pytest.mark.parametrize('slots', [1, 255, 256, 257])
def test_rescore(cuda, slots, ld):
    thr = 0.7
    out, scores, boxes = rescore_inputs(slots, ld, slots * 100 + ld, thr)
    if slots > 1:
        out[0, 0:2], scores[0] = (0, 5), -1                       # dead, and its probability passes: stays dead
        out[1, 0:2], scores[1] = (5, 0), 0.9                      # alive, fails the threshold: dies
        out[2, 0:2], scores[2] = (0, 5), 0.0                      # alive at score 0, passes
        p = om.face_prob(out[:, 0:2])
        assert ((scores < 0) & (p >= F(thr))).sum() >= 1 and ((scores >= 0) & (p < F(thr))).sum() >= 1
    for plain, pass_boxes in ((0, False), (0, True), (1, True)):
        want_s, want_r, want_b = rescore_ref(out, scores, thr, boxes, plain)
        got_s, got_r, got_b = run_rescore(out, scores, thr, boxes, plain, pass_boxes)
        what = 'plain %d boxes %s' % (plain, pass_boxes)
        assert_scores(got_s, want_s, what)
        assert_bitwise(got_r, want_r, what)
        assert_bitwise(got_b, want_b, what)                       # plain 0 or no pointer: untouched
    if slots > 1:
        assert want_s[0] == -1 and want_s[1] == -1 and want_s[2] > 0.99 and not np.array_equal(want_b, boxes)


@pytest.mark.gpu
def test_rescore_probability_equal_to_the_threshold_passes(cuda):
    """Equal logits: exp(0) = 1 on the device and on the host, so P(face) is 0.5 exactly and `>=` keeps the slot under
    threshold 0.5.  These planted slots are the only ones within 1e-6 of the threshold."""
    thr = 0.5
    out, scores, boxes = rescore_inputs(300, 16, 31, thr)
    planted = np.array([0, 63, 64, 255, 256, 299])
    out[planted, 0] = out[planted, 1]
    scores[planted] = F(0.8)
    scores[planted[-1]] = F(-1)                                   # ... but not a slot that was dead
    p = om.face_prob(out[:, 0:2])
    assert (p[planted] == F(0.5)).all()
    near = np.abs(p.astype(np.float64) - 0.5) <= 1e-6
    assert sorted(np.nonzero(near)[0]) == sorted(planted)
    want_s, want_r, want_b = rescore_ref(out, scores, thr, boxes, 1)
    got_s, got_r, got_b = run_rescore(out, scores, thr, boxes, 1)
    assert (got_s[planted[:-1]] == F(0.5)).all() and got_s[planted[-1]] == -1
    assert_scores(got_s, want_s, 'scores')
    assert_bitwise(got_r, want_r, 'reg')
    assert_bitwise(got_b, want_b, 'boxes')
