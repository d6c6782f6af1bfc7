"""The k nearest rows in order (oneshot.Gallery.topk / dif_match_topk) against the CPU oracle (tests/topk_ref.py): per probe q

    d = oracle.distance.distance(q[None, :], gallery, metric);  order = np.argsort(d, kind='stable')
    keep = order[~np.isnan(d[order])][:k];  idx = keep + index_base;  dist = d[keep];  unused slots: -1 / NaN

Metric 0: idx and dist bit-identical.  Metric 1: the device evaluates arccos in double and rounds once, NumPy's float32 arccos
is within 2 ulp of that, so two rows whose oracle distances lie within NEAR = 2e-6 of each other may swap (test_within_gpu.py's
NEAR).  A list position j is CLEAR when the oracle's sorted distances at j-1, j, j+1 differ by more than NEAR: there idx
equals the oracle's; at every position the oracle distance of the device's j-th row is within NEAR of the oracle's j-th
distance and the rows of a list are distinct; dist within 1e-5 of the oracle's for that row (test_match_gpu.py's rule, its
_cos_ok exclusion included).  CLEAR positions are at least 0.9 of the listed positions of every case, asserted on the oracle
before the device is asked (tests/test_topk_ref.py holds the same caps without a GPU)."""
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
import rank_ref
import remove_ref
import topk_ref
from oracle import distance as od

pytestmark = pytest.mark.gpu
ATOL = 1e-5          # test_match_gpu.py
NEAR = 2e-6          # test_within_gpu.py
MIN_CLEAR = 0.9
NEG = np.float32(-np.inf)
SHAPES = [(1, 1, 32), (3, 129, 64), (65, 257, 512), (130, 1000, 128), (64, 4097, 512), (3, 66000, 32)]


def _cos_ok(sim):
    return sim <= 0.999


@functools.lru_cache(maxsize=None)
def _inputs(B, G, D, seed=0):
    """test_rank_gpu.py's generator (the same arrays): identities with four near-duplicate rows each, probes drawn the same
    way; also returns each probe's identity."""
    rng = np.random.default_rng(1000 * G + 10 * B + D + seed)
    nid = max(1, G // 4)
    centres = rng.standard_normal((nid, D))
    gal = (centres[np.arange(G) % nid] + 0.05 * rng.standard_normal((G, D))).astype(np.float32)
    pick = rng.integers(0, nid, B)
    probes = (centres[pick] + 0.05 * rng.standard_normal((B, D))).astype(np.float32)
    for a in (gal, probes, pick):
        a.setflags(write=False)
    return probes, gal, pick


@functools.lru_cache(maxsize=None)
def _oracle(B, G, D, metric):
    probes, gal, _ = _inputs(B, G, D)
    full = rank_ref.distances(probes, gal, metric)
    full.setflags(write=False)
    return full


def _bits_equal(a, b):
    """float32 arrays equal bit for bit, every NaN taken as one value."""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


def _cap(full, k, metric):
    """The cap on the oracle alone -- call it before the device is asked."""
    if metric == 1:
        share = topk_ref.clear_share(full, k, NEAR)
        assert share >= MIN_CLEAR, share


def _check(got, full, k, metric, base=0):
    idx, dist = got
    want_i, want_d = topk_ref.topk_full(full, k, base)
    assert idx.dtype == np.int64 and dist.dtype == np.float32
    assert idx.shape == want_i.shape and dist.shape == want_d.shape
    pad = want_i < 0
    assert np.array_equal(idx < 0, pad) and (idx[pad] == -1).all() and np.isnan(dist[pad]).all()   # padding exactly -1 / NaN
    assert not np.isnan(dist[~pad]).any()
    if metric == 0:
        bad = np.argwhere(idx != want_i)
        assert bad.shape[0] == 0, (bad[:8], idx[idx != want_i][:8], want_i[idx != want_i][:8])
        assert _bits_equal(dist, want_d)
        return
    B = full.shape[0]
    assert ((idx[~pad] >= base) & (idx[~pad] < base + full.shape[1])).all()
    clear = topk_ref.clear_positions(full, k, NEAR)
    assert clear.sum() >= MIN_CLEAR * (~pad).sum()
    bad = np.argwhere(clear & (idx != want_i))
    assert bad.shape[0] == 0, (bad[:8], idx[clear & (idx != want_i)][:8], want_i[clear & (idx != want_i)][:8])
    for b in range(B):
        n = int((~pad[b]).sum())
        rows = idx[b, :n] - base
        assert np.unique(rows).shape[0] == n                                     # the rows of a list are distinct
        mine = full[b, rows]                                                     # the oracle's distances of the device's rows
        assert not np.isnan(mine).any()
        assert (np.abs(mine.astype(np.float64) - want_d[b, :n].astype(np.float64)) <= NEAR).all(), b
        okc = _cos_ok(np.cos(mine.astype(np.float64) * np.pi))
        np.testing.assert_allclose(dist[b, :n][okc], mine[okc], atol=ATOL, rtol=0)


def _np(t):
    return tuple(a.cpu().numpy() for a in t)


# ------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('k', [1, 5, 128])
@pytest.mark.parametrize('B,G,D', SHAPES)
def test_topk_shapes(cuda, B, G, D, k, metric):
    """Tile tails in both dimensions, every probe-tile shape (<= 32, <= 64, more), k above the row count, k above the rows of
    one tile, more than 512 tiles (several rounds of words in the select kernel)."""
    from deep_insight_face import oneshot
    probes, gal_np, _ = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    _cap(full, k, metric)
    gal = oneshot.Gallery(gal_np)
    got = gal.topk(probes, k, metric)
    assert all(isinstance(a, np.ndarray) for a in got)                          # NumPy in -> NumPy out
    _check(got, full, k, metric)
    if k > G:
        assert (got[0][:, G:] == -1).all() and np.isnan(got[1][:, G:]).all() and (got[0][:, :G] >= 0).all()
    ti, td = gal.topk(torch.from_numpy(probes).cuda(), k, metric)
    assert torch.is_tensor(ti) and ti.is_cuda and torch.is_tensor(td) and td.is_cuda   # CUDA tensors in -> CUDA tensors out
    assert ti.dtype == torch.int64 and td.dtype == torch.float32 and tuple(ti.shape) == (B, k) == tuple(td.shape)
    assert np.array_equal(ti.cpu().numpy(), got[0]) and _bits_equal(td.cpu().numpy(), got[1])
    if k == 5:
        for g in (gal, gal_np):                                                 # the module-level form, on a handle and on rows
            mi, md = oneshot.topk(probes, g, k, metric)
            assert np.array_equal(mi, got[0]) and _bits_equal(md, got[1])
    gal.close()


# ------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('k', [5, 128])
@pytest.mark.parametrize('B,G,D', [(64, 4097, 512), (130, 1000, 128)])
def test_topk_both_phases(cuda, B, G, D, k, metric):
    """Option "topk_seed": 1 and 2 leave the list to the sweep (a loose tolerance, +inf where the best tile has fewer than k finite
    rows), 1000 evaluates every tile in the seed: bit-identical to the default, which is checked against the oracle."""
    from deep_insight_face import oneshot
    probes, gal_np, _ = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    _cap(full, k, metric)
    gal = oneshot.Gallery(gal_np)
    p = torch.from_numpy(probes).cuda()
    base = _np(gal.topk(p, k, metric))
    _check(base, full, k, metric)
    for seed in (1, 2, 1000, 0):
        gal.set_option('topk_seed', seed)
        idx, dist = _np(gal.topk(p, k, metric))
        assert np.array_equal(idx, base[0]), seed
        assert _bits_equal(dist, base[1]), seed
    with pytest.raises(ValueError):
        gal.set_option('topk_seed', -1)
    gal.close()


# ------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('metric', [0, 1])
def test_topk_exact_ties(cuda, metric):
    """Identical enrolled rows appear in index order at the head of the list (test_rank_exact_ties' table)."""
    from deep_insight_face import oneshot
    probes, gal_np = gi.match_tie_inputs()
    copies = {0: (100, 300, 500), 1: (105, 305, 505), 2: (119, 319, 519), 3: (120, 320), 4: (139, 339), 5: (101, 301, 501),
              6: (110, 310, 510)}
    full = rank_ref.distances(probes, gal_np, metric)
    want_i, want_d = topk_ref.topk_full(full, 4)
    for b, rows in copies.items():
        assert tuple(want_i[b, :len(rows)]) == rows
        assert (want_d[b, len(rows)] > want_d[b, 0] + 1e-3)                     # nothing else anywhere near: exact on both metrics
    gal = oneshot.Gallery(gal_np)
    for seed in (0, 1):
        gal.set_option('topk_seed', seed)
        idx, dist = gal.topk(probes, 4, metric)
        for b, rows in copies.items():
            n = len(rows)
            assert tuple(idx[b, :n]) == rows, (seed, b, idx[b])
            assert (dist[b, :n] == dist[b, 0]).all()
            if metric == 0:
                assert _bits_equal(dist[b, :n], want_d[b, :n])
            else:
                np.testing.assert_allclose(dist[b, :n], want_d[b, :n], atol=ATOL, rtol=0)
        if metric == 0:
            assert np.array_equal(idx, want_i) and _bits_equal(dist, want_d)
    gal.close()


@pytest.mark.parametrize('seed', [0, 1])
def test_topk_near_ties(cuda, seed):
    """Rows one ulp, 1e-7 and 1e-4 apart and exact duplicates at shuffled positions: metric 0, bit-identical to the stable
    argsort."""
    from deep_insight_face import oneshot
    probes, gal_np = gi.match_near_tie_inputs()
    full = rank_ref.distances(probes, gal_np, 0)
    assert not np.isnan(full).any()
    order = np.argsort(full, axis=1, kind='stable')[:, :5]
    gal = oneshot.Gallery(gal_np)
    gal.set_option('topk_seed', seed)
    idx, dist = gal.topk(probes, 5, 0)
    assert np.array_equal(idx, order), np.argwhere(idx != order)[:8]
    assert _bits_equal(dist, np.take_along_axis(full, order, axis=1))
    gal.close()


# ------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('metric', [0, 1])
def test_topk_against_rank_within_and_match(cuda, metric):
    """Device-only, exact on both metrics: the rank of the j-th listed row is j at the listed distance; the range search at
    the k-th distance counts at least k rows and just below it at most k - 1; the head of the list is the arg-min."""
    from deep_insight_face import oneshot
    B, G, D, k = 130, 1000, 128, 10
    probes, gal_np, _ = _inputs(B, G, D)
    gal = oneshot.Gallery(gal_np)
    p = torch.from_numpy(probes).cuda()
    ti, td = gal.topk(p, k, metric)
    idx, dist = _np((ti, td))
    assert (idx >= 0).all() and not np.isnan(dist).any()
    for j in range(k):
        rank, md = _np(gal.rank(p, ti[:, j].contiguous(), metric))
        assert (rank == j).all(), (j, np.flatnonzero(rank != j)[:8])
        assert np.array_equal(md.view(np.uint32), dist[:, j].view(np.uint32))
    assert (np.diff(dist.astype(np.float64), axis=1) >= 0).all()
    for b in range(B):
        hi = int(gal.within(p[b:b + 1], dist[b, k - 1], metric, max_hits=0)[0][0])
        lo = int(gal.within(p[b:b + 1], np.nextafter(dist[b, k - 1], NEG), metric, max_hits=0)[0][0])
        assert hi >= k and lo <= k - 1, (b, lo, hi)
    mi, md = _np(gal.match(p, metric))
    assert np.array_equal(mi, idx[:, 0]) and np.array_equal(md.view(np.uint32), dist[:, 0].view(np.uint32))
    gal.close()


# ------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize('name', [c[0] for c in gi.match_degenerate_cases()])
def test_topk_degenerate(cuda, name):
    """Zero, tiny, huge and non-finite rows and probes, anti-parallel rows: whatever IEEE arithmetic gives the reference; a row
    whose distance is NaN is never listed and the list is as long as the rows that are left allow.  The probes that resolve
    every tile are among these.  A list cannot be longer than 128, so k = G + 2 runs on 126 rows of the fixture (the odd ones
    among them, topk_ref.small_gallery) and the whole fixture takes k = 128 in its place."""
    from deep_insight_face import oneshot
    probes, gal_np = [(p, g) for n, p, g in gi.match_degenerate_cases() if n == name][0]
    small = topk_ref.small_gallery(probes, gal_np)
    for rows, ks in ((gal_np, (1, 3, 128)), (small, (1, 3, small.shape[0] + 2))):
        G = rows.shape[0]
        fulls = {metric: rank_ref.distances(probes, rows, metric) for metric in (0, 1)}
        for k in ks:
            _cap(fulls[1], k, 1)
        gal = oneshot.Gallery(rows)
        for metric in (0, 1):
            full = fulls[metric]
            nan = np.isnan(full)
            for k in ks:
                idx, dist = gal.topk(probes, k, metric)
                _check((idx, dist), full, k, metric)
                real = idx >= 0
                assert np.array_equal(real.sum(1), np.minimum(k, (~nan).sum(1)))
                for b in range(full.shape[0]):
                    assert not nan[b, idx[b][real[b]]].any()                    # NaN rows are never listed
        gal.close()
    assert small.shape[0] + 2 == 128


# ------------------------------------------------------------------------------------------- 6
def test_topk_identical_probe_and_clamp_nan(cuda):
    """A probe equal to an enrolled row: the reference's similarity may round above 1 and its distance is NaN then -- the row is
    absent from the list by default; with clamp_nan the clamped distance 0 is ordered and reported and the row comes first."""
    from deep_insight_face import oneshot
    _, gal_np, _ = _inputs(65, 257, 512)
    rows = np.arange(0, 256, 4).astype(np.int64)
    probes = gal_np[rows].copy()
    with np.errstate(invalid='ignore'):
        sim = od.similarity(probes, gal_np[rows])
    full = rank_ref.distances(probes, gal_np, 1)
    dself = full[np.arange(len(rows)), rows]
    assert (sim > 1).any() and (sim <= 1).any()                                # both outcomes occur in these 64 pairs
    assert np.array_equal(np.isnan(dself), sim > 1)
    k = 5
    _cap(full, k, 1)
    gal = oneshot.Gallery(gal_np)
    idx, dist = gal.topk(probes, k, 1)
    _check((idx, dist), full, k, 1)
    listed = (idx == rows[:, None]).any(1)
    assert np.array_equal(listed, sim <= 1)                                     # a self row above 1 is absent
    assert (idx[sim <= 1, 0] == rows[sim <= 1]).all()
    gal.set_option('clamp_nan', 1)
    cidx, cdist = gal.topk(probes, k, 1)
    assert (cidx[:, 0] == rows).all() and not np.isnan(cdist).any()
    assert (cdist[sim >= 1, 0] == 0).all()
    # the rest of the list is the default's, moved down by the self row where it was absent
    for b in range(len(rows)):
        rest = idx[b] if sim[b] <= 1 else np.concatenate([rows[b:b + 1], idx[b, :k - 1]])
        assert np.array_equal(cidx[b], rest), b
    rank, md = gal.rank(probes, cidx[:, 0], 1)                                  # the rank agrees under the same option
    assert (rank == 0).all() and np.array_equal(md.view(np.uint32), cdist[:, 0].view(np.uint32))
    gal.close()


# ------------------------------------------------------------------------------------------- 7
def test_topk_handle_reuse_and_workspaces(cuda):
    """A non-monotone batch and k sequence on one handle, interleaved with within, rank, match, update and remove, against
    the recomputed oracle; match unaffected; a shard with an index_base."""
    from deep_insight_face import oneshot
    G, D = 4097, 128
    probes, gal_np, _ = _inputs(70, G, D)
    gal_np = gal_np.copy()
    gal = oneshot.Gallery(gal_np)

    def check(n, k, metric=0):
        full = rank_ref.distances(probes[:n], gal_np, metric)
        _cap(full, k, metric)
        got = gal.topk(probes[:n], k, metric)
        _check(got, full, k, metric)
        return got

    m_before = gal.match(probes, 0)
    first = check(70, 5)
    gal.within(probes[:33], 0.5, 0, max_hits=8)
    check(33, 128)
    gal.rank(probes, first[0][:, 1], 0)
    again = check(70, 5)
    assert np.array_equal(first[0], again[0]) and _bits_equal(first[1], again[1])
    m_mid = gal.match(probes, 0)
    assert np.array_equal(m_before[0], m_mid[0]) and np.array_equal(m_before[1].view(np.uint32), m_mid[1].view(np.uint32))
    row = gal_np[first[0][0, 0]][None]                                          # probe 0's nearest row, appended five times:
    gal.update(np.repeat(row, 5, axis=0))                                       # ties at higher indices, listed behind it
    gal_np = np.concatenate([gal_np, np.repeat(row, 5, axis=0)])
    assert len(gal) == G + 5
    got = check(70, 5)
    assert list(got[0][0]) == [first[0][0, 0], G, G + 1, G + 2, G + 3]
    check(33, 128, 1)
    gone = np.array([int(first[0][0, 0]), 7, 4000, G + 4], dtype=np.int64)      # un-enrol it, two strangers and the last copy
    gal.remove(gone)
    gal_np = remove_ref.remove_ref(gal_np, gone)[0]
    assert len(gal) == gal_np.shape[0] == G + 1
    check(70, 5)
    check(70, 128, 1)
    gal.within(probes, 0.5, 1, max_hits=8)
    check(33, 5, 1)
    assert np.array_equal(gal.match(probes, 0)[0], od.match(probes, gal_np, 0)[0])
    gal.close()
    shifted = oneshot.Gallery(gal_np, index_base=1000)
    full = rank_ref.distances(probes, gal_np, 0)
    idx, dist = shifted.topk(probes, 5, 0)
    _check((idx, dist), full, 5, 0, base=1000)
    assert (idx >= 1000).all() and (idx < 1000 + gal_np.shape[0]).all()
    assert np.array_equal(idx[:, 0], shifted.match(probes, 0)[0])
    shifted.close()


# ------------------------------------------------------------------------------------------- 8
def test_topk_arguments(cuda):
    from deep_insight_face import oneshot
    B, G, D = 3, 129, 64
    probes, gal_np, _ = _inputs(B, G, D)
    full = _oracle(B, G, D, 1)
    gal = oneshot.Gallery(gal_np)
    for k in (0, 129, -1, -128):
        with pytest.raises(ValueError):
            gal.topk(probes, k)
        with pytest.raises(ValueError):
            oneshot.topk(probes, gal, k, 0)
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        gal.topk(probes, 3, distance_metric=7)
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        oneshot.topk(probes, gal, 3, 7)
    with pytest.raises(ValueError):
        gal.topk(np.zeros((2, 32), dtype=np.float32), 3)
    _check(gal.topk(probes[0], 3, 1), full[:1], 3, 1)                           # one probe as a vector
    p = torch.from_numpy(probes).cuda()
    k = 4
    idx = torch.empty((B, k), dtype=torch.int64, device='cuda')
    dist = torch.empty((B, k), dtype=torch.float32, device='cuda')
    gal.topk_into(p, k, 1, idx, dist)                                           # the well-formed call
    torch.cuda.synchronize()
    _check(_np((idx, dist)), full, k, 1)
    with pytest.raises(RuntimeError, match='Undefined distance metric 2'):
        gal.topk_into(p, k, 2, idx, dist)
    for bad_k in (0, 129, -3):
        with pytest.raises(ValueError):
            gal.topk_into(p, bad_k, 1, idx, dist)
    wide_i = torch.empty((B, 2 * k), dtype=torch.int64, device='cuda')
    wide_d = torch.empty((B, 2 * k), dtype=torch.float32, device='cuda')
    for bad in (dict(idx=wide_i[:, ::2]), dict(dist=wide_d[:, ::2]),                                        # not contiguous
                dict(idx=idx.to(torch.int32)), dict(dist=dist.double()), dict(probes=p.double()),           # wrong dtype
                dict(idx=idx[:2]), dict(dist=dist[:, :3]), dict(idx=wide_i), dict(idx=idx.reshape(-1)),     # wrong shape
                dict(probes=p[:, :32]), dict(probes=probes),
                dict(idx=idx.cpu()), dict(dist=dist.cpu()), dict(probes=p.cpu())):                          # host tensors
        kw = dict(probes=p, idx=idx, dist=dist)
        kw.update(bad)
        with pytest.raises(ValueError):
            gal.topk_into(kw['probes'], k, 1, kw['idx'], kw['dist'])
    i0, d0 = gal.topk(np.zeros((0, D), dtype=np.float32), 3)                    # an empty batch
    assert i0.shape == (0, 3) and d0.shape == (0, 3) and i0.dtype == np.int64 and d0.dtype == np.float32
    gal.close()
    empty = oneshot.Gallery(emd_size=D)                                         # nothing enrolled: all padding
    for metric in (0, 1):
        for k in (1, 128):
            i0, d0 = empty.topk(probes, k, metric)
            assert i0.shape == (B, k) and i0.dtype == np.int64 and (i0 == -1).all() and np.isnan(d0).all()
    empty.close()


# ------------------------------------------------------------------------------------------- 9
# Rounds of probes.  topk_run (and topk_ids_run) split a call into rounds of `per` probes when the tile words would pass their
# cap -- at a million rows from 8 577 probes up.  Gallery option "topk_round" lowers `per`, so the loop and its per-round
# offsets run here: 128 + 1 probes (the last round on the 32-probe tile), 128 + 128 + 44 (the 64-probe tile; 256 + 44 with the
# option at 256) and three full rounds.  With the option at 0 the same arrays are one launch of three probe blocks.
ROUND_SHAPES = [(129, 257, 512), (300, 1000, 128), (384, 1000, 128)]


def _round_options(B):
    """One round, forced rounds, one round again."""
    return (0, 128, 256, 0) if B == 300 else (0, 128, 0)


def _without_offset(arg, per):
    """What a launch that dropped its `+ b0` would read in rounds of `per`: probe b0 + j gets entry j."""
    return arg[np.arange(arg.shape[0]) % per]


def _later_rounds(B, per):
    return [slice(b0, min(b0 + per, B)) for b0 in range(per, B, per)]


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('k', [5, 128])
@pytest.mark.parametrize('B,G,D', ROUND_SHAPES)
def test_topk_rounds(cuda, B, G, D, k, metric):
    """"topk_round" 0, 128 (and 256 at B = 300), 0 on one handle, under the default seed and under "topk_seed" 1 (the seed and
    the sweep then both work in every round): every answer passes the oracle check, and the forced-round answers and the one
    after the option is taken back equal the first one-round answer bit for bit."""
    from deep_insight_face import oneshot
    probes, gal_np, _ = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    _cap(full, k, metric)
    gal = oneshot.Gallery(gal_np)
    p = torch.from_numpy(probes).cuda()
    first = None
    for seed in (0, 1):
        gal.set_option('topk_seed', seed)
        for per in _round_options(B):
            gal.set_option('topk_round', per)
            got = _np(gal.topk(p, k, metric))
            _check(got, full, k, metric)
            first = first or got
            assert np.array_equal(got[0], first[0]), (seed, per, np.argwhere(got[0] != first[0])[:8])
            assert _bits_equal(got[1], first[1]), (seed, per)
    with pytest.raises(ValueError, match='topk_round'):
        gal.set_option('topk_round', 100)                                       # not a multiple of 128
    with pytest.raises(ValueError, match='topk_round'):
        gal.set_option('topk_round', -128)
    gal.close()
