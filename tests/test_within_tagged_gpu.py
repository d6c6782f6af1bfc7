"""The tagged range search (oneshot.Gallery.within with `row_tags` and `probe_masks` / dif_match_within_tagged) against
tests/tagged_queries_ref.py over the CPU oracle's distances: for every probe

    d = oracle.distance.distance(q[None, :], gallery, metric);  d[~eligible[p]] = NaN
    hits = np.flatnonzero(d <= t);  count = len(hits);  idx = hits[:K] + index_base;  dist = d[hits[:K]];  padding -1 / NaN

under tests/test_within_gpu.py's rules: metric 0 bit for bit; metric 1 exact outside the pairs whose oracle distance lies
within 2e-6 of the tolerance, distances within 1e-5.  tests/test_tagged_queries_ref.py asserts, without a GPU, the input
conditions relied on here."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import remove_ref
import tagged_queries_cases as tc
import tagged_queries_ref as tq
import tagged_ref
from test_within_gpu import NEAR, _check, _check_near, _median_t, _sparse_t

pytestmark = pytest.mark.gpu


def _np(t):
    return tuple(a.cpu().numpy() for a in t)


def _same(got, want):
    """Bit for bit, NaN where NaN."""
    assert len(got) == len(want)
    for x, y in zip(got, want):
        x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        y = y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape
        if x.dtype == np.float32:
            assert np.array_equal(np.isnan(x), np.isnan(y))
            assert np.array_equal(x[~np.isnan(x)].view(np.uint32), y[~np.isnan(y)].view(np.uint32))
        else:
            assert np.array_equal(x, y)


def _device_mask(gal, probes, t, metric, G, tags, masks):
    cnt, idx, _ = gal.within(probes, t, metric, G, tags, masks)
    mask = np.zeros((probes.shape[0], G), dtype=bool)
    for b in range(probes.shape[0]):
        assert (idx[b, :cnt[b]] >= 0).all() and (idx[b, cnt[b]:] == -1).all()
        mask[b, idx[b, :cnt[b]]] = True
    return cnt, mask


# ------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('B,G,D', tc.SHAPES)
def test_within_tagged_shapes(cuda, B, G, D, metric):
    """Tile tails in both dimensions, every probe-tile shape, more than one gallery tile; max_hits 0, 8 and G; the widest-gap
    tolerance (no pair near it: exact on both metrics) and the median one (hundreds of eligible hits per probe)."""
    from deep_insight_face import oneshot
    probes, gal_np, _, tags, masks, _ = tc.case(B, G, D)
    full, fm = tc.oracle(B, G, D, metric), tc.masked(B, G, D, metric)
    t, gap = _sparse_t(full)
    assert gap >= 1e-3, gap
    el = tagged_ref.eligible(tags, masks)
    gal = oneshot.Gallery(gal_np)
    for K in (0, 8, G):
        want = tq.within_full(full, tags, masks, t, K)
        got = gal.within(probes, t, metric, K, tags, masks)
        assert all(isinstance(a, np.ndarray) for a in got)                      # NumPy in -> NumPy out
        _check(got, want, metric)
        listed = got[1] >= 0
        assert el[np.nonzero(listed)[0], got[1][listed]].all()                  # an ineligible row is never listed
    want = tq.within_full(full, tags, masks, t, 8)
    assert (want[0][(masks == 0) | (masks == 8)] == 0).all()
    dev = gal.within(torch.from_numpy(probes).cuda(), t, metric, 8, torch.from_numpy(np.array(tags)).cuda(),
                     torch.from_numpy(np.array(masks)).cuda())
    assert all(torch.is_tensor(a) and a.is_cuda for a in dev)                   # CUDA tensors in -> CUDA tensors out
    assert dev[0].dtype == torch.int64 and dev[1].dtype == torch.int64 and dev[2].dtype == torch.float32
    _check(_np(dev), want, metric)
    _check(oneshot.within(probes, gal, t, metric, 8, tags, masks), want, metric)       # the module-level form, on a handle
    _check(oneshot.within(probes, gal_np, t, metric, 8, row_tags=tags, probe_masks=masks), want, metric)   # ... and on rows
    one = gal.within(probes, t, metric, 8, tags, 6)                             # a Python int stands for every probe
    _check(one, tq.within_full(full, tags, np.full(B, 6, dtype=np.int64), t, 8), metric)
    # the median tolerance
    tm = _median_t(full)
    if metric == 0:
        for K in (0, 8, G):
            _check(gal.within(probes, tm, 0, K, tags, masks), tq.within_full(full, tags, masks, tm, K), 0)
    else:
        near = (np.abs(full.astype(np.float64) - float(tm)) <= NEAR) & el
        assert near.sum() <= 2e-4 * el.sum()
        cnt, mask = _device_mask(gal, probes, tm, 1, G, tags, masks)
        _check_near(cnt, mask, fm, tm)
        assert not mask[~el].any()
    gal.close()


# ------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('metric', [0, 1])
def test_within_tagged_equals_the_gallery_of_the_eligible_rows(cuda, metric):
    """Per mask value: the tagged answer is the untagged answer of a gallery that holds the eligible rows alone, indices
    mapped back -- device against device, bit for bit on both metrics; with every pair eligible, the untagged call's."""
    from deep_insight_face import oneshot
    B, G, D = 130, 1000, 128
    probes, gal_np, _, tags, masks, _ = tc.case(B, G, D)
    t = _median_t(tc.oracle(B, G, D, metric))
    gal = oneshot.Gallery(gal_np)
    for K in (8, G):
        got = gal.within(probes, t, metric, K, tags, masks)
        for m in tagged_ref.MASK_CYCLE:
            who = np.flatnonzero(masks == m)
            rows = np.flatnonzero(tagged_ref.eligible(tags, np.array([m]))[0])
            if len(rows) == 0:
                assert m in (0, 8) and (got[0][who] == 0).all() and (got[1][who] == -1).all() and np.isnan(got[2][who]).all()
                continue
            sub = oneshot.Gallery(gal_np[rows])
            cnt, idx, dist = sub.within(probes[who], t, metric, K)
            sub.close()
            _same((got[0][who], got[1][who], got[2][who]), (cnt, np.where(idx >= 0, rows[np.maximum(idx, 0)], -1), dist))
        plain = gal.within(probes, t, metric, K)
        _same(gal.within(probes, t, metric, K, np.full(G, -1, dtype=np.int64), np.full(B, -1, dtype=np.int64)), plain)
        _same(gal.within(probes, t, metric, K, np.full(G, tc.TOP, dtype=np.int64), -1), plain)
        assert (plain[0] != got[0]).mean() >= 0.9
    gal.close()


# ------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('maker', [gi.match_near_tie_inputs, gi.match_tie_inputs])
def test_within_tagged_boundary_across_eligibility(cuda, maker):
    """t exactly ON an oracle distance, with exact ties and near-ties on both sides of an eligibility boundary: an ineligible
    row exactly at the tolerance is not a hit, an eligible one is; one float lower drops them all.  Metric 0, bit-exact."""
    from deep_insight_face import oneshot
    probes, gal_np = maker()
    probes = probes[:8]
    G = gal_np.shape[0]
    full = tc.distances(probes, gal_np, 0)
    order = np.argsort(full, axis=1, kind='stable')
    gal = oneshot.Gallery(gal_np)
    for b in range(8):
        t5 = full[b, order[b, 4]]
        at = np.flatnonzero(full[b] == t5)
        tags = np.ones(G, dtype=np.int64)
        tags[order[b, 4]] = 2                                                    # the row AT the tolerance: not this probe's
        tags[order[b, 1]] = 0                                                    # a nearer row: nobody's
        masks = np.array([1], dtype=np.int64)
        for t in (t5, np.nextafter(t5, np.float32(-np.inf))):
            want = tq.within_full(full[b:b + 1], tags, masks, t, 64)
            got = gal.within(probes[b:b + 1], t, 0, 64, tags, masks)
            _check(got, want, 0)
            assert order[b, 4] not in got[1][0] and order[b, 1] not in got[1][0]
        plain = gal.within(probes[b:b + 1], t5, 0, 64)
        tagged = gal.within(probes[b:b + 1], t5, 0, 64, tags, masks)
        assert plain[0][0] - tagged[0][0] == 2 and order[b, 4] in plain[1][0]
        both = gal.within(probes[b:b + 1], t5, 0, 64, tags, 3)                  # mask 3 sees the row at the tolerance again
        assert both[0][0] == plain[0][0] - 1 and order[b, 4] in both[1][0]
        assert set(at) - {order[b, 4], order[b, 1]} <= set(tagged[1][0])         # its eligible exact ties stay hits
    gal.close()


# ------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('name', [c[0] for c in gi.match_degenerate_cases()])
def test_within_tagged_degenerate(cuda, name):
    """Zero, tiny, huge and non-finite rows and probes, anti-parallel rows -- the probes that resolve every tile are among
    these -- with the odd rows eligible for every second probe only: an eligible row whose search key is NaN must still bring
    its tile in, an ineligible one is neither counted nor listed."""
    from deep_insight_face import oneshot
    probes, gal_np = [(p, g) for n, p, g in gi.match_degenerate_cases() if n == name][0]
    B = probes.shape[0]
    fulls = {metric: tc.distances(probes, gal_np, metric) for metric in (0, 1)}
    tags, masks = tc.degenerate_tags(fulls, B)
    el = tagged_ref.eligible(tags, masks)
    gal = oneshot.Gallery(gal_np)
    for metric in (0, 1):
        full = fulls[metric]
        fm = tagged_ref.masked(full, tags, masks)
        fin = full[np.isfinite(full)]
        t = np.float32(0.3) if metric == 1 else (np.float32(np.median(fin)) if fin.size else np.float32(1.0))
        want = tq.within_full(full, tags, masks, t, 16)
        cnt, idx, dist = gal.within(probes, t, metric, 16, tags, masks)
        listed = idx >= 0
        assert not np.isnan(dist[listed]).any()
        assert not np.isnan(fm[np.nonzero(listed)[0], idx[listed]]).any()        # NaN and ineligible rows are never listed
        assert el[np.nonzero(listed)[0], idx[listed]].all()
        if metric == 0:
            _check((cnt, idx, dist), want, 0)
        else:
            with np.errstate(invalid='ignore'):
                near = (np.abs(fm.astype(np.float64) - float(t)) <= NEAR).sum(1)
            clear = near == 0
            assert clear.mean() >= 0.9
            _check((cnt[clear], idx[clear], dist[clear]), tuple(w[clear] for w in want), 1)
            assert (np.abs(cnt - want[0]) <= near).all()
    gal.close()


# ------------------------------------------------------------------------------------------- 5
def test_within_tagged_skip_rule(cuda):
    """A tile without an eligible row is never evaluated row by row.  516 tiles, bit 2 on 100 rows of exactly two of them,
    nine probes with mask 4 at tolerance 1.0 on metric 1 with room in the lists: every eligible row is a sure hit, and the
    untagged rule would evaluate every tile with a sure row -- all 516 -- while the list has room; the last probe lies outside
    the bound's validity and would resolve every tile anyway.  Here: the two tiles that hold an eligible row, per probe."""
    from deep_insight_face import oneshot
    probes, gal_np, tags = tc.skip_case()
    n, G = probes.shape[0], gal_np.shape[0]
    full = tc.distances(probes, gal_np, 1)
    assert not np.isnan(full).any()
    masks = np.full(n, 4, dtype=np.int64)
    gal = oneshot.Gallery(gal_np)
    assert gal.stat('within_tagged_tiles') == 0                                  # before the first tagged call
    got = gal.within(probes, 1.0, 1, 8192, tags, masks)
    tiles = gal.stat('within_tagged_tiles')
    print('within_tagged_tiles', tiles)
    _check(got, tq.within_full(full, tags, masks, 1.0, 8192), 1)
    assert (got[0] == 100).all()
    assert 0 < tiles <= 2 * n, tiles
    c8 = gal.within(probes, 1.0, 1, 8192, tags, 8)                              # nothing carries bit 3
    assert gal.stat('within_tagged_tiles') == 0 and (c8[0] == 0).all() and (c8[1] == -1).all() and np.isnan(c8[2]).all()
    gal.within(probes, 1.0, 1, 8192, tags, masks)
    assert gal.stat('within_tagged_tiles') == tiles
    gal.within(probes[:1], 0.3, 1, 8)                                            # an untagged call leaves the stat alone
    assert gal.stat('within_tagged_tiles') == tiles
    t = _median_t(full)                                                          # a tolerance with OUT rows as well
    got = gal.within(probes, t, 1, 8192, tags, masks)
    assert gal.stat('within_tagged_tiles') <= 2 * n
    want = tq.within_full(full, tags, masks, t, 8192)
    near = (np.abs(tagged_ref.masked(full, tags, masks).astype(np.float64) - float(t)) <= NEAR).sum(1)
    clear = near == 0
    assert clear.sum() >= n - 1
    _check(tuple(a[clear] for a in got), tuple(w[clear] for w in want), 1)
    gal.close()


# ------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize('metric', [0, 1])
def test_within_tagged_rounds(cuda, metric):
    """B = 300 with "within_round" 128, then 0, on one handle: three rounds whose masks are taken at their offsets (before the
    device is asked: the oracle under the masks a dropped `+ b0` would read differs in both later rounds); the forced-round
    answer and the one after the option is taken back are equal bit for bit, and so are their tile counts -- a counter zeroed
    in every round would report the last round's alone."""
    from deep_insight_face import oneshot
    B, G, D = 300, 1000, 128
    probes, gal_np, _, tags, _, _ = tc.case(B, G, D)
    masks = tc.round_masks(B)
    full = tc.oracle(B, G, D, metric)
    t = _median_t(full) if metric == 0 else _sparse_t(full)[0]
    want = tq.within_full(full, tags, masks, t, 8)
    wrong = tq.within_full(full, tags, masks[np.arange(B) % 128], t, 8)
    for sl in (slice(128, 256), slice(256, 300)):
        assert (wrong[0][sl] != want[0][sl]).any()
    gal = oneshot.Gallery(gal_np)
    p, t_dev, m_dev = (torch.from_numpy(np.array(a)).cuda() for a in (probes, tags, masks))
    answers, tiles = [], []
    for per in (0, 128, 0):
        gal.set_option('within_round', per)
        got = _np(gal.within(p, t, metric, 8, t_dev, m_dev))
        tiles.append(gal.stat('within_tagged_tiles'))
        _check(got, want, metric)
        answers.append(got)
    _same(answers[1], answers[0])
    _same(answers[2], answers[0])
    assert tiles[0] > 0 and tiles == [tiles[0]] * 3, tiles
    gal.close()


# ------------------------------------------------------------------------------------------- 7
def test_within_tagged_handle_reuse(cuda):
    """A non-monotone batch sequence on one handle, interleaved with untagged `within`, `match`, `update` and `remove` -- the
    tags permuted by the moves `remove` reports -- against the recomputed oracle; a handle with index_base 1000."""
    from deep_insight_face import oneshot
    B, G, D = 64, 4097, 128
    probes, gal_np, _, tags, masks, _ = tc.case(B, G, D)
    gal_np, tags = gal_np.copy(), np.array(tags)
    t, gap = _sparse_t(tc.oracle(B, G, D, 0))
    assert gap >= 1e-3
    gal = oneshot.Gallery(gal_np)

    def check(n, metric=0, tol=t, K=8):
        want = tq.within_full(tc.distances(probes[:n], gal_np, metric), tags, masks[:n], tol, K)
        got = gal.within(probes[:n], tol, metric, K, tags, masks[:n])
        _check(got, want, metric)
        return got

    plain = gal.within(probes, t, 0, 8)
    first = check(64)
    check(3)
    gal.match(probes[:33], 0)
    check(33, K=0)
    _same(gal.within(probes, t, 0, 8), plain)                                   # the untagged call between tagged ones
    _same(check(64), first)
    assert masks[0] == 1 and first[0][0] >= 1
    row = gal_np[first[1][0, 0]][None]                                          # probe 0's first eligible hit, five more times:
    gal.update(np.repeat(row, 5, axis=0))                                       # three of the copies eligible for it
    gal_np = np.concatenate([gal_np, np.repeat(row, 5, axis=0)])
    tags = np.concatenate([tags, np.array([1, 0, 3, 2, tc.TOP | 1], dtype=np.int64)])
    got = check(64, K=16)
    assert got[0][0] == first[0][0] + 3 and {G, G + 2, G + 4} <= set(got[1][0]) and not {G + 1, G + 3} & set(got[1][0])
    gone = np.array([int(first[1][0, 0]), 7, 4000, G + 2], dtype=np.int64)
    moved_from, moved_to = gal.remove(gone)
    gal_np = remove_ref.remove_ref(gal_np, gone)[0]
    new_tags = tags[:gal_np.shape[0]].copy()
    new_tags[moved_to] = tags[moved_from]                                       # the caller's table follows the moves
    assert np.array_equal(new_tags, remove_ref.remove_ref(tags, gone)[0])
    tags = new_tags
    assert len(gal) == gal_np.shape[0] == G + 1
    got = check(64, K=16)
    assert got[0][0] == first[0][0] + 1
    check(33)
    check(64, metric=1, tol=_sparse_t(tc.oracle(B, G, D, 1))[0])
    gal.close()
    shifted = oneshot.Gallery(gal_np, index_base=1000)
    full = tc.distances(probes, gal_np, 0)
    got = shifted.within(probes, t, 0, 8, tags, masks)
    _check(got, tq.within_full(full, tags, masks, t, 8, index_base=1000), 0)
    assert ((got[1] == -1) | ((got[1] >= 1000) & (got[1] < 1000 + gal_np.shape[0]))).all() and (got[1] >= 1000).any()
    shifted.close()


# ------------------------------------------------------------------------------------------- 8
def test_within_tagged_arguments(cuda):
    from deep_insight_face import _native as N
    from deep_insight_face import oneshot
    B, G, D = 3, 129, 64
    probes, gal_np, _, tags, masks, _ = tc.case(B, G, D)
    full = tc.oracle(B, G, D, 1)
    t = _sparse_t(full)[0]
    want = tq.within_full(full, tags, masks, t, 4)
    gal = oneshot.Gallery(gal_np)
    for kw in (dict(row_tags=tags), dict(probe_masks=masks), dict(probe_masks=1)):        # exactly one given
        with pytest.raises(ValueError, match='go together'):
            gal.within(probes, t, 1, 4, **kw)
        with pytest.raises(ValueError, match='go together'):
            oneshot.within(probes, gal, t, 1, 4, **kw)
    for bad_t, bad_m in ((tags.astype(np.float32), masks), (tags, masks.astype(np.float64)), (tags != 0, masks),
                         (tags, masks != 0), (tags[:-1], masks), (tags, masks[:2]), (tags[None], masks), (tags, masks[:, None]),
                         (torch.from_numpy(np.array(tags)).float(), masks), (tags, torch.from_numpy(np.array(masks)) != 0),
                         (tags, 1.0), (tags, True), (tags, 1 << 64), (tags, -(1 << 63) - 1), (3, masks)):
        with pytest.raises(ValueError):
            gal.within(probes, t, 1, 4, bad_t, bad_m)
    for K in (-1, oneshot.MAX_HITS + 1):
        with pytest.raises(ValueError):
            gal.within(probes, t, 1, K, tags, masks)
    with pytest.raises(ValueError, match='NaN'):
        gal.within(probes, float('nan'), 1, 4, tags, masks)
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        gal.within(probes, t, 7, 4, tags, masks)
    # every integer width, lists, one probe as a vector with an int mask
    small = (tags & 7).astype(np.int8)                                          # without bit 63: fits every width
    ws = tq.within_full(full, small, masks & 7, t, 4)
    for dt in (np.int8, np.uint8, np.int16, np.int32, np.uint32, np.int64, np.uint64):
        _check(gal.within(probes, t, 1, 4, small.astype(dt), (masks & 7).astype(dt)), ws, 1)
    _check(gal.within(probes, t, 1, 4, small.tolist(), (masks & 7).tolist()), ws, 1)
    _check(gal.within(probes[0], t, 1, 4, tags, 1), tuple(w[:1] for w in want), 1)
    # the allocation-free form: dense int64 CUDA tensors of the right shapes, both or neither
    p = torch.from_numpy(probes).cuda()
    t_dev, m_dev = (torch.from_numpy(np.array(a)).cuda() for a in (tags, masks))
    K = 4
    cnt = torch.empty((B,), dtype=torch.int64, device='cuda')
    idx = torch.empty((B, K), dtype=torch.int64, device='cuda')
    dist = torch.empty((B, K), dtype=torch.float32, device='cuda')
    gal.within_into(p, t, 1, cnt, idx, dist, t_dev, m_dev)
    torch.cuda.synchronize()
    _check(_np((cnt, idx, dist)), want, 1)
    wide = torch.zeros((2 * G,), dtype=torch.int64, device='cuda')
    for bad in (dict(row_tags=None), dict(probe_masks=None), dict(row_tags=t_dev.to(torch.int32)), dict(probe_masks=m_dev.int()),
                dict(row_tags=t_dev.cpu()), dict(probe_masks=m_dev.cpu()), dict(row_tags=tags), dict(probe_masks=1),
                dict(row_tags=t_dev[:-1]), dict(probe_masks=m_dev[:2]), dict(row_tags=wide[::2][:G])):
        kw = dict(row_tags=t_dev, probe_masks=m_dev)
        kw.update(bad)
        with pytest.raises(ValueError):
            gal.within_into(p, t, 1, cnt, idx, dist, kw['row_tags'], kw['probe_masks'])
    # the C layer: NULL tags or masks with rows enrolled fail; n = 0 is a no-op; within's own argument errors
    h, f = gal._h, N.lib.dif_match_within_tagged
    for rt, pm in ((None, N.ptr(m_dev)), (N.ptr(t_dev), None)):
        assert f(h, N.ptr(p), B, 1, float(t), K, rt, pm, N.ptr(cnt), N.ptr(idx), N.ptr(dist), N.stream_ptr()) != 0
        assert b'null row tags or probe masks' in N.lib.dif_last_error()
    assert f(h, None, 0, 1, float(t), K, None, None, None, None, None, N.stream_ptr()) == 0
    assert f(None, N.ptr(p), B, 1, float(t), K, N.ptr(t_dev), N.ptr(m_dev), N.ptr(cnt), N.ptr(idx), N.ptr(dist), N.stream_ptr()) != 0
    for args in ((B, 7, float(t), K), (-1, 1, float(t), K), (B, 1, float('nan'), K), (B, 1, float(t), -1),
                 (B, 1, float(t), oneshot.MAX_HITS + 1)):
        n_, metric_, t_, K_ = args
        assert f(h, N.ptr(p), n_, metric_, t_, K_, N.ptr(t_dev), N.ptr(m_dev), N.ptr(cnt), N.ptr(idx), N.ptr(dist),
                 N.stream_ptr()) != 0, args
    assert f(h, N.ptr(p), B, 1, float(t), K, N.ptr(t_dev), N.ptr(m_dev), N.ptr(cnt), None, None, N.stream_ptr()) != 0
    assert f(h, N.ptr(p), B, 1, float(t), 0, N.ptr(t_dev), N.ptr(m_dev), N.ptr(cnt), None, None, N.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), want[0])
    with pytest.raises(ValueError):
        gal.stat('within_tagged')
    c0, i0, d0 = gal.within(np.zeros((0, D), dtype=np.float32), t, 1, 3, tags, np.zeros(0, dtype=np.int64))   # an empty batch
    assert c0.shape == (0,) and i0.shape == (0, 3) and d0.shape == (0, 3) and c0.dtype == np.int64 and d0.dtype == np.float32
    gal.close()
    empty = oneshot.Gallery(emd_size=D)                                         # nothing enrolled: counts 0, neither array read
    none = np.zeros(0, dtype=np.int64)
    for metric in (0, 1):
        for K in (0, 5):
            c0, i0, d0 = empty.within(probes, t, metric, K, none, masks)
            assert (c0 == 0).all() and i0.shape == (B, K) and (i0 == -1).all() and np.isnan(d0).all()
    cnt.fill_(-5)
    assert f(empty._h, N.ptr(p), B, 1, float(t), K, None, None, N.ptr(cnt), N.ptr(idx), N.ptr(dist), N.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (cnt == 0).all()
    assert empty.stat('within_tagged_tiles') == 0
    empty.close()


# ------------------------------------------------------------------------------------------- 9
def test_within_tagged_cuda_in_cuda_out_and_no_host_read(cuda):
    """CUDA tensors in give CUDA tensors out, and in steady state the call reads nothing back: under
    set_sync_debug_mode('error') any synchronising call of torch inside it raises."""
    from deep_insight_face import oneshot
    B, G, D = 65, 257, 512
    probes, gal_np, _, tags, masks, _ = tc.case(B, G, D)
    full = tc.oracle(B, G, D, 1)
    t = _sparse_t(full)[0]
    gal = oneshot.Gallery(gal_np)
    p, t_dev, m_dev = (torch.from_numpy(np.array(a)).cuda() for a in (probes, tags, masks))
    warm = gal.within(p, t, 1, 8, t_dev, m_dev)                                 # (the workspace grows on the first call)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = gal.within(p, t, 1, 8, t_dev, m_dev)
        six = gal.within(p, t, 1, 8, t_dev, 6)                                  # the broadcast mask is filled on the device
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for a, dt, shape in zip(got, (torch.int64, torch.int64, torch.float32), ((B,), (B, 8), (B, 8))):
        assert torch.is_tensor(a) and a.is_cuda and a.dtype == dt and tuple(a.shape) == shape
    _same(got, warm)
    _check(_np(got), tq.within_full(full, tags, masks, t, 8), 1)
    _check(_np(six), tq.within_full(full, tags, np.full(B, 6, dtype=np.int64), t, 8), 1)
    gal.close()
