"""Gallery range search (oneshot.Gallery.within / dif_match_within) against the CPU oracle: for every probe q

    dist  = oracle.distance.distance(q[None, :], gallery, metric)
    hits  = np.flatnonzero(dist <= t)            # NaN <= t is False
    count = len(hits);  idx = hits[:K] + index_base;  dist = dist[hits[:K]];  unused slots: idx -1, dist NaN

Metric 0: hit set, count and distances bit-identical.  Metric 1: the device evaluates arccos in double and rounds once,
NumPy's float32 arccos is within 2 ulp of that, so a pair whose oracle distance lies within 2e-6 of t may fall on the other
side; everything else must agree exactly, and distances within 1e-5 (test_match_gpu.py's rule, its _cos_ok exclusion
included)."""
import functools

import numpy as np
import pytest
import torch

import cluster_ref
import dbscan_ref
import golden_inputs as gi
import rank_ref
import topk_ids_ref
import topk_ref
from oracle import distance as od

pytestmark = pytest.mark.gpu
ATOL = 1e-5          # test_match_gpu.py
NEAR = 2e-6          # metric 1: oracle distances this close to the tolerance may differ in the arccos' last bits


def _cos_ok(sim):
    # test_match_gpu.py: arccos amplifies dot-product rounding near s -> 1
    return sim <= 0.999


@functools.lru_cache(maxsize=None)
def _inputs(B, G, D, seed=0):
    """Identities with four near-duplicate rows each; probes drawn the same way."""
    rng = np.random.default_rng(1000 * G + 10 * B + D + seed)
    nid = max(1, G // 4)
    centres = rng.standard_normal((nid, D))
    gal = (centres[np.arange(G) % nid] + 0.05 * rng.standard_normal((G, D))).astype(np.float32)
    probes = (centres[rng.integers(0, nid, B)] + 0.05 * rng.standard_normal((B, D))).astype(np.float32)
    gal.setflags(write=False)
    probes.setflags(write=False)
    return probes, gal


def _full(probes, gal, metric):
    with np.errstate(all='ignore'):
        return np.stack([od.distance(q[None, :], gal, metric) for q in probes]).astype(np.float32, copy=False)


@functools.lru_cache(maxsize=None)
def _oracle(B, G, D, metric):
    probes, gal = _inputs(B, G, D)
    full = _full(probes, gal, metric)
    full.setflags(write=False)
    return full


def _sparse_t(full):
    """Midpoint of the widest gap between adjacent sorted oracle distances; the gap itself."""
    v = np.sort(full[np.isfinite(full)].astype(np.float64))
    gaps = np.diff(v)
    k = int(np.argmax(gaps))
    return np.float32((v[k] + v[k + 1]) / 2), float(gaps[k])


def _median_t(full):
    return np.float32(np.median(full[np.isfinite(full)]))


def _expect(full, t, K, base=0):
    B = full.shape[0]
    cnt = np.zeros(B, dtype=np.int64)
    idx = np.full((B, K), -1, dtype=np.int64)
    dist = np.full((B, K), np.nan, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        for b in range(B):
            hits = np.flatnonzero(full[b] <= np.float32(t))
            cnt[b] = len(hits)
            h = hits[:K]
            idx[b, :len(h)] = h + base
            dist[b, :len(h)] = full[b, h]
    return cnt, idx, dist


def _check_dist(dist, want, metric):
    assert np.array_equal(np.isnan(dist), np.isnan(want))
    ok = ~np.isnan(want)
    if metric == 0:
        assert np.array_equal(dist[ok].view(np.uint32), want[ok].view(np.uint32))     # bit-identical
    else:
        ok &= _cos_ok(np.cos(np.where(ok, want, 0).astype(np.float64) * np.pi))
        np.testing.assert_allclose(dist[ok], want[ok], atol=ATOL, rtol=0)


def _check(got, want, metric):
    (cnt, idx, dist), (wc, wi, wd) = got, want
    assert cnt.dtype == np.int64 and idx.dtype == np.int64 and dist.dtype == np.float32
    assert cnt.shape == wc.shape and idx.shape == wi.shape and dist.shape == wd.shape
    assert np.array_equal(cnt, wc), (np.flatnonzero(cnt != wc)[:8], cnt[cnt != wc][:8], wc[cnt != wc][:8])
    assert np.array_equal(idx, wi)
    _check_dist(dist, wd, metric)


def _device_mask(gal, probes, t, metric, G):
    cnt, idx, _ = gal.within(probes, t, metric, max_hits=G)
    mask = np.zeros((probes.shape[0], G), dtype=bool)
    for b in range(probes.shape[0]):
        assert (idx[b, :cnt[b]] >= 0).all() and (idx[b, cnt[b]:] == -1).all()
        mask[b, idx[b, :cnt[b]]] = True
    return cnt, mask


def _check_near(cnt, mask, full, t):
    """Metric 1: outside the pairs within NEAR of t the hit mask is the oracle's; counts differ by at most those pairs."""
    with np.errstate(invalid='ignore'):
        want = full <= np.float32(t)
        near = np.abs(full.astype(np.float64) - float(t)) <= NEAR
    assert np.array_equal(mask[~near], want[~near])
    assert (np.abs(cnt - want.sum(1)) <= near.sum(1)).all()
    return near


# ------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('B,G,D', [(1, 1, 32), (3, 129, 64), (65, 257, 512), (130, 1000, 128), (64, 4097, 512)])
def test_within_shapes_sparse(cuda, B, G, D, metric):
    """Tile tails in both dimensions, every probe-tile shape (<= 32, <= 64, more), more than one gallery tile."""
    from deep_insight_face import oneshot
    probes, gal_np = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    if G == 1:
        d = full[0, 0]
        ts = [np.nextafter(d, np.float32(np.inf)) * np.float32(2), d / np.float32(2)]     # above and below the one distance
    else:
        t, gap = _sparse_t(full)
        assert gap >= 1e-3, gap
        ts = [t]
    gal = oneshot.Gallery(gal_np)
    for t in ts:
        want = _expect(full, t, 8)
        if G > 1:
            assert 1 <= want[0].min() and want[0].max() <= 8, (want[0].min(), want[0].max())
        got = gal.within(probes, t, metric, max_hits=8)
        assert all(isinstance(a, np.ndarray) for a in got)                      # NumPy in -> NumPy out
        _check(got, want, metric)
        tc, ti, td = gal.within(torch.from_numpy(probes).cuda(), t, metric, max_hits=8)
        assert all(torch.is_tensor(a) and a.is_cuda for a in (tc, ti, td))      # CUDA tensor in -> CUDA tensors out
        assert tc.dtype == torch.int64 and ti.dtype == torch.int64 and td.dtype == torch.float32
        _check((tc.cpu().numpy(), ti.cpu().numpy(), td.cpu().numpy()), want, metric)
        _check(oneshot.within(probes, gal, t, metric, max_hits=8), want, metric)   # the module-level form
    gal.close()


# ------------------------------------------------------------------------------------------- 2
def test_within_truncation_and_count_only(cuda):
    from deep_insight_face import oneshot
    B, G, D = 130, 1000, 128
    probes, gal_np = _inputs(B, G, D)
    full = _oracle(B, G, D, 0)
    t = _median_t(full)
    gal = oneshot.Gallery(gal_np)
    for K in (0, 1, 64):
        want = _expect(full, t, K)
        assert np.median(want[0]) > 100 and want[0].min() > 32      # hundreds of hits for the typical probe
        got = gal.within(probes, t, 0, max_hits=K)
        assert got[1].shape == (B, K) and got[2].shape == (B, K)
        _check(got, want, 0)
    gal.close()


# ------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('maker', [gi.match_near_tie_inputs, gi.match_tie_inputs])
def test_within_inclusive_boundary(cuda, maker):
    """t exactly ON an oracle distance with near-duplicates and exact ties on both sides: <= includes the tie itself and
    every exact tie, excludes the next float up; one float lower drops them all.  Metric 0, bit-exact."""
    from deep_insight_face import oneshot
    probes, gal_np = maker()
    probes = probes[:8]
    full = _full(probes, gal_np, 0)
    gal = oneshot.Gallery(gal_np)
    for b in range(8):
        t5 = np.sort(full[b])[4]                                               # the 5th-nearest row's distance
        for t in (t5, np.nextafter(t5, np.float32(-np.inf))):
            want = _expect(full[b:b + 1], t, 64)
            got = gal.within(probes[b:b + 1], t, 0, max_hits=64)
            _check(got, want, 0)
        assert _expect(full[b:b + 1], t5, 64)[0][0] >= 5
    gal.close()


# ------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('B,G,D', [(130, 1000, 128), (64, 4097, 128)])
def test_within_metric1_dense(cuda, B, G, D):
    from deep_insight_face import oneshot
    probes, gal_np = _inputs(B, G, D)
    full = _oracle(B, G, D, 1)
    t = _median_t(full)
    near = np.abs(full.astype(np.float64) - float(t)) <= NEAR
    assert near.mean() <= 2e-4, near.mean()
    gal = oneshot.Gallery(gal_np)
    cnt, mask = _device_mask(gal, probes, t, 1, G)
    _check_near(cnt, mask, full, t)
    # the device's own distances decide: the row Gallery.match reports at d_k is listed at t = d_k, not one float below
    mi, md = gal.match(probes[:8], 1)
    for k in range(8):
        assert not np.isnan(md[k])
        c1, i1, d1 = gal.within(probes[k:k + 1], md[k], 1, max_hits=G)
        assert mi[k] in i1[0, :c1[0]]
        assert d1[0, list(i1[0, :c1[0]]).index(mi[k])] == md[k]
        c2, i2, _ = gal.within(probes[k:k + 1], np.nextafter(md[k], np.float32(-np.inf)), 1, max_hits=G)
        assert mi[k] not in i2[0, :c2[0]]
    gal.close()


# ------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize('name', [c[0] for c in gi.match_degenerate_cases()])
def test_within_degenerate(cuda, name):
    """Zero, tiny, huge and non-finite rows and probes, anti-parallel rows: no special rule -- whatever IEEE arithmetic gives
    the reference, and a NaN distance is never a hit."""
    from deep_insight_face import oneshot
    probes, gal_np = [(p, g) for n, p, g in gi.match_degenerate_cases() if n == name][0]
    gal = oneshot.Gallery(gal_np)
    for metric in (0, 1):
        full = _full(probes, gal_np, metric)
        fin = full[np.isfinite(full)]
        t = np.float32(0.3) if metric == 1 else (np.float32(np.median(fin)) if fin.size else np.float32(1.0))
        want = _expect(full, t, 16)
        cnt, idx, dist = gal.within(probes, t, metric, max_hits=16)
        listed = idx >= 0
        assert not np.isnan(dist[listed]).any()                                # NaN-distance rows are never listed
        rows = np.nonzero(listed)
        assert not np.isnan(full[rows[0], idx[listed]]).any()
        if metric == 0:
            _check((cnt, idx, dist), want, 0)
        else:
            with np.errstate(invalid='ignore'):
                near = (np.abs(full.astype(np.float64) - float(t)) <= NEAR).sum(1)
            clear = near == 0
            assert clear.mean() >= 0.9
            _check((cnt[clear], idx[clear], dist[clear]), tuple(w[clear] for w in want), 1)
            assert (np.abs(cnt - want[0]) <= near).all()
    gal.close()


def test_within_identical_probe_and_clamp_nan(cuda):
    """A probe equal to an enrolled row: the reference's similarity may round above 1 and its distance is NaN then -- not a
    hit by default; with clamp_nan the clamped distance 0 is compared."""
    from deep_insight_face import oneshot
    _, gal_np = _inputs(65, 257, 512)
    rows = np.arange(0, 256, 4)
    probes = gal_np[rows].copy()
    with np.errstate(invalid='ignore'):
        sim = od.similarity(probes, gal_np[rows])
        dself = od.distance(probes, gal_np[rows], 1)
    assert (sim > 1).any() and (sim <= 1).any()                                # both outcomes occur in these 64 pairs
    t = np.float32(0.01)
    assert (dself[~np.isnan(dself)] < 1e-3).all()
    gal = oneshot.Gallery(gal_np)
    cnt, idx, dist = gal.within(probes, t, 1, max_hits=16)
    for k, r in enumerate(rows):
        assert (r in idx[k, :cnt[k]]) == (not np.isnan(dself[k])), (k, sim[k])
    gal.set_option('clamp_nan', 1)
    cnt, idx, dist = gal.within(probes, t, 1, max_hits=16)
    for k, r in enumerate(rows):
        assert r in idx[k, :cnt[k]]
        if sim[k] >= 1:
            assert dist[k, list(idx[k]).index(r)] == 0
    gal.close()


# ------------------------------------------------------------------------------------------- 6
def test_within_handle_reuse_and_workspaces(cuda):
    """A non-monotone batch sequence on one handle, interleaved with match and update: every buffer keeps its own size."""
    from deep_insight_face import oneshot
    G, D = 4097, 128
    probes, gal_np = _inputs(70, G, D)
    gal_np = gal_np.copy()
    t, gap = _sparse_t(_oracle(70, G, D, 0))
    assert gap >= 1e-3
    gal = oneshot.Gallery(gal_np)

    def check(n, metric=0, tol=t):
        want = _expect(_full(probes[:n], gal_np, metric), tol, 8)
        got = gal.within(probes[:n], tol, metric, max_hits=8)
        _check(got, want, metric)
        return got

    c70 = check(70)[0]
    check(33)
    gal.update(np.repeat(probes[:1], 5, axis=0))                               # five copies of probe 0: distance 0, all hits
    gal_np = np.concatenate([gal_np, np.repeat(probes[:1], 5, axis=0)])
    assert len(gal) == G + 5
    m_before = gal.match(probes, 0)
    c70b = check(70)[0]
    assert c70b[0] == c70[0] + 5 and np.array_equal(c70b[1:], c70[1:])
    m_after = gal.match(probes, 0)
    assert np.array_equal(m_before[0], m_after[0]) and np.array_equal(m_before[1].view(np.uint32), m_after[1].view(np.uint32))
    assert np.array_equal(m_after[0], od.match(probes, gal_np, 0)[0])
    check(70)
    t1, gap1 = _sparse_t(_full(probes, gal_np, 1)[:, :G])
    assert gap1 >= 1e-3
    check(70, 1, t1)
    gal.close()
    shifted = oneshot.Gallery(gal_np, index_base=1000)
    want = _expect(_full(probes, gal_np, 0), t, 8, base=1000)
    assert (want[1][want[1] >= 0] >= 1000).all()
    _check(shifted.within(probes, t, 0, max_hits=8), want, 0)
    shifted.close()


# ------------------------------------------------------------------------------------------- 7
def test_within_arguments(cuda):
    from deep_insight_face import oneshot
    B, G, D = 3, 129, 64
    probes, gal_np = _inputs(B, G, D)
    gal = oneshot.Gallery(gal_np)
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        gal.within(probes, 0.5, distance_metric=7)
    with pytest.raises(ValueError):
        gal.within(np.zeros((2, 32), dtype=np.float32), 0.5)
    with pytest.raises(ValueError):
        gal.within(probes, 0.5, max_hits=-1)
    with pytest.raises(ValueError):
        gal.within(probes, 0.5, max_hits=oneshot.MAX_HITS + 1)
    with pytest.raises(ValueError):
        gal.within(probes, float('nan'))
    p = torch.from_numpy(probes).cuda()
    cnt = torch.empty(B, dtype=torch.int64, device='cuda')
    idx = torch.empty((B, 4), dtype=torch.int64, device='cuda')
    dist = torch.empty((B, 4), dtype=torch.float32, device='cuda')
    gal.within_into(p, 0.5, 1, cnt, idx, dist)                                 # the well-formed call
    torch.cuda.synchronize()
    _check((cnt.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()), _expect(_oracle(B, G, D, 1), 0.5, 4), 1)
    wide = torch.empty((B, 8), dtype=torch.int64, device='cuda')
    for bad in (dict(idx=wide[:, ::2]),                                        # not contiguous
                dict(idx=idx.to(torch.int32)), dict(dist=dist.double()), dict(count=cnt.to(torch.int32)),   # wrong dtype
                dict(count=cnt[:2]), dict(dist=dist[:, :3].contiguous()), dict(idx=idx[0]),                 # wrong shape
                dict(count=cnt.cpu()), dict(idx=idx.cpu()), dict(probes=p.cpu())):                          # host tensors
        kw = dict(probes=p, count=cnt, idx=idx, dist=dist)
        kw.update(bad)
        with pytest.raises(ValueError):
            gal.within_into(kw['probes'], 0.5, 1, kw['count'], kw['idx'], kw['dist'])
    for metric in (0, 1):
        c, i, d = gal.within(probes, -1.0, metric, max_hits=4)                 # no distance is negative
        assert not c.any() and (i == -1).all() and np.isnan(d).all()
    full = _oracle(B, G, D, 1)
    c, _, _ = gal.within(probes, 2.0, 1, max_hits=4)                           # every distance that is not NaN
    assert np.array_equal(c, (~np.isnan(full)).sum(1))
    c, i, d = gal.within(np.zeros((0, D), dtype=np.float32), 0.5)
    assert c.shape == (0,) and i.shape == (0, 64) and d.shape == (0, 64)
    gal.close()
    empty = oneshot.Gallery(emd_size=D)
    c, i, d = empty.within(probes, 0.5, 1, max_hits=4)                         # np.flatnonzero of an empty array
    assert c.dtype == np.int64 and not c.any() and (i == -1).all() and np.isnan(d).all()
    empty.close()


# ------------------------------------------------------------------------------------------- 8
# Rounds of probes.  within_run splits a call into rounds of `per` probes when the census would pass its cap -- at a million
# rows from 17 153 probes up.  Gallery option "within_round" lowers `per`, so the loop and its per-round offsets run here:
# 128 + 1 probes (the last round on the 32-probe census tile), 128 + 128 + 44 (the 64-probe tile; 256 + 44 with the option at
# 256) and three full rounds.  With the option at 0 the same arrays are one launch of three probe blocks.
ROUND_SHAPES = [(129, 257, 512), (300, 1000, 128), (384, 1000, 128)]


def _round_options(B):
    """One round, forced rounds, one round again."""
    return (0, 128, 256, 0) if B == 300 else (0, 128, 0)


def _bits(a):
    """An array as integers that compare bit for bit, every NaN taken as one value."""
    if a.dtype != np.float32:
        return a
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def _identical(got, first):
    assert len(got) == len(first)
    for i, (g, f) in enumerate(zip(got, first)):
        assert g.dtype == f.dtype and g.shape == f.shape, i
        bad = np.argwhere(_bits(g) != _bits(f))
        assert bad.shape[0] == 0, (i, bad[:8])


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('B,G,D', ROUND_SHAPES)
def test_within_rounds(cuda, B, G, D, metric):
    """"within_round" 0, 128 (and 256 at B = 300), 0 on one handle: every answer passes the oracle check, and the forced-round
    answers and the one after the option is taken back equal the first one-round answer bit for bit.  The sparse tolerance with
    lists of 8 on both metrics; the dense one on metric 0 with lists of 64 and count-only (max_hits = 0: the list pointers stay
    null through the offset arithmetic), on metric 1 through the whole hit mask."""
    from deep_insight_face import oneshot
    probes, gal_np = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    t, gap = _sparse_t(full)
    assert gap >= 1e-3, gap
    sparse = _expect(full, t, 8)
    assert 1 <= sparse[0].min() and sparse[0].max() <= 8
    tm = _median_t(full)
    if metric == 1:
        assert (np.abs(full.astype(np.float64) - float(tm)) <= NEAR).mean() <= 2e-4
    gal = oneshot.Gallery(gal_np)
    first = {}
    for per in _round_options(B):
        gal.set_option('within_round', per)
        got = gal.within(probes, t, metric, max_hits=8)
        _check(got, sparse, metric)
        _identical(got, first.setdefault('sparse', got))
        if metric == 0:
            for K in (64, 0):
                got = gal.within(probes, tm, 0, max_hits=K)
                assert got[1].shape == (B, K) and got[2].shape == (B, K)
                _check(got, _expect(full, tm, K), 0)
                _identical(got, first.setdefault(K, got))
        else:
            cnt, mask = _device_mask(gal, probes, tm, 1, G)
            _check_near(cnt, mask, full, tm)
            _identical((cnt, mask), first.setdefault('mask', (cnt, mask)))
    with pytest.raises(ValueError, match='within_round'):
        gal.set_option('within_round', 100)                                    # not a multiple of 128
    with pytest.raises(ValueError, match='within_round'):
        gal.set_option('within_round', -128)
    gal.close()


# ------------------------------------------------------------------------------------------- 9
def test_shared_workspaces_survive_a_non_monotone_sequence_of_queries(cuda):
    """within, rank, cluster and dbscan share within_census / within_thr, the four top-k entries share topk_min, and each
    compares its need with a capacity another may have set.  One handle of 1000 x 128 rows through top-k at 3 probes, within at
    300, rank at 37, cluster, within in forced rounds, an append of 300 rows (8 gallery tiles become 11: the census need grows
    at the same number of probes), within in one round and in forced rounds, topk_ids at 300, dbscan, top-k at 130 -- every
    step against its oracle on metric 0, bit for bit."""
    from deep_insight_face import oneshot
    B, G, D = 300, 1000, 128
    probes, gal_np = _inputs(B, G, D)
    pick = rank_ref.distances(probes, gal_np[:G // 4], 0).argmin(1)             # each probe's identity: its nearest first copy
    extra = (gal_np[:300] + 0.05 * np.random.default_rng(5).standard_normal((300, D))).astype(np.float32)
    rows = {G: gal_np, G + 300: np.concatenate([gal_np, extra])}
    full = {n: rank_ref.distances(probes, r, 0) for n, r in rows.items()}
    assert not any(np.isnan(f).any() for f in full.values())
    lower = {n: cluster_ref.lower_distances(r, 0) for n, r in rows.items()}
    gal = oneshot.Gallery(gal_np)

    def topk(n, k):
        idx, dist = gal.topk(probes[:n], k, 0)
        want = topk_ref.topk_full(full[len(gal)][:n], k)
        assert np.array_equal(idx, want[0])
        _check_dist(dist, want[1], 0)

    def within(n):
        f = full[len(gal)][:n]
        for t, K in ((_sparse_t(f)[0], 8), (_median_t(f), 64), (_median_t(f), 0)):
            _check(gal.within(probes[:n], t, 0, max_hits=K), _expect(f, t, K), 0)

    def gap_t(inside=False):
        """The midpoint of the widest gap between the pairwise distances (identities apart); `inside`: the median distance
        within an identity, a tolerance ON a distance (metric 0 is bit-identical) that leaves core, border and noise rows."""
        v = np.sort(cluster_ref.pair_values(lower[len(gal)]))
        k = int(np.argmax(np.diff(v)))
        return np.float32(v[k // 2]) if inside else np.float32((v[k] + v[k + 1]) / 2)

    topk(3, 5)                                                                  # 1
    within(300)                                                                 # 2
    mates = (pick[:37] + (G // 4) * (np.arange(37) % 4)).astype(np.int64)       # 3
    rank, md = gal.rank(probes[:37], mates, 0)
    want = rank_ref.rank_full(full[G][:37], mates)
    assert np.array_equal(rank, want[0]) and (want[0] <= 4).all()
    _check_dist(md, want[1], 0)
    labels, n = gal.cluster(gap_t(), 0)                                         # 4
    want = cluster_ref.cluster_from(lower[G], G, gap_t())
    assert want[1] == G // 4 and int(n) == want[1] and np.array_equal(labels.cpu().numpy(), want[0])
    gal.set_option('within_round', 128)                                         # 5
    within(300)
    gal.update(extra)                                                           # 6
    assert len(gal) == G + 300
    gal.set_option('within_round', 0)                                           # 7
    within(300)
    gal.set_option('within_round', 128)
    within(300)
    gal.set_option('within_round', 0)
    row_labels = (np.arange(G + 300) % (G // 4)).astype(np.int64)               # 8
    got = gal.topk_ids(probes, 5, row_labels, 0)
    want = topk_ids_ref.topk_ids_full(full[G + 300], row_labels, 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    _check_dist(got[1], want[1], 0)
    labels, degree, counts = gal.dbscan(gap_t(True), 3, 0)                      # 9
    want = dbscan_ref.dbscan_from(lower[G + 300], G + 300, gap_t(True), 3)
    assert all(kind.sum() >= 10 for kind in dbscan_ref.kinds(want[0], want[1], 3))     # core, border and noise rows
    assert tuple(counts.cpu().tolist()) == tuple(want[2])
    assert np.array_equal(degree.cpu().numpy(), want[1]) and np.array_equal(labels.cpu().numpy(), want[0])
    topk(130, 128)                                                              # 10
    gal.close()
