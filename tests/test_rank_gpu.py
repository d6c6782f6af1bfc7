"""Rank of the mate (oneshot.Gallery.rank / dif_match_rank) against the CPU oracle (tests/rank_ref.py): for every probe q

    d = oracle.distance.distance(q[None, :], gallery, metric);  dm = d[m - index_base]
    rank = count(d < dm) + count(d[:m - index_base] == dm);  mate_dist = dm        unmated: -1 / NaN;  dm NaN: G / NaN

Metric 0: rank and mate_dist bit-identical.  Metric 1: the device evaluates arccos in double and rounds once, NumPy's float32
arccos is within 2 ulp of that, so a row whose oracle distance lies within 2e-6 of dm may fall on the other side of it
(test_within_gpu.py's NEAR): a probe without such a row is CLEAR and compares exactly, the others within the number of such
rows; mate_dist within 1e-5 (test_match_gpu.py's rule, its _cos_ok exclusion included)."""
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
import rank_ref
from oracle import distance as od

pytestmark = pytest.mark.gpu
ATOL = 1e-5          # test_match_gpu.py
NEAR = 2e-6          # test_within_gpu.py
NEG = np.float32(-np.inf)


def _cos_ok(sim):
    return sim <= 0.999


@functools.lru_cache(maxsize=None)
def _inputs(B, G, D, seed=0):
    """test_within_gpu.py's generator (the same arrays): identities with four near-duplicate rows each, probes drawn the same
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


def _identity_mates(B, G, D):
    """A row of the probe's own identity (rows pick, pick + nid, ...), a different one of the four from probe to probe."""
    pick = _inputs(B, G, D)[2]
    nid = max(1, G // 4)
    return (pick + nid * (np.arange(B) % (4 if G >= 4 else 1))).astype(np.int64)


def _random_mates(B, G, seed=3):
    return np.random.default_rng(seed + G + B).integers(0, G, B).astype(np.int64)


def _near(full, mates, base=0):
    """Per probe: rows other than the mate whose oracle distance lies within NEAR of the mate's."""
    B, G = full.shape
    out = np.zeros(B, dtype=np.int64)
    for b in range(B):
        k = int(mates[b]) - base
        if 0 <= k < G and not np.isnan(full[b, k]):
            with np.errstate(invalid='ignore'):
                close = np.abs(full[b].astype(np.float64) - float(full[b, k])) <= NEAR
            close |= full[b] == full[b, k]                                       # (inf - inf is NaN)
            out[b] = int(close.sum()) - 1
    return out


def _check(got, full, mates, metric, base=0, min_clear=0.5):
    rank, dist = got
    want_r, want_d = rank_ref.rank_full(full, mates, base)
    assert rank.dtype == np.int64 and dist.dtype == np.float32
    assert rank.shape == want_r.shape and dist.shape == want_d.shape
    assert np.array_equal(np.isnan(dist), np.isnan(want_d)), (np.flatnonzero(np.isnan(dist) != np.isnan(want_d))[:8])
    ok = ~np.isnan(want_d)
    if metric == 0:
        assert np.array_equal(dist[ok].view(np.uint32), want_d[ok].view(np.uint32))              # bit-identical
        bad = np.flatnonzero(rank != want_r)
        assert bad.size == 0, (bad[:8], rank[bad[:8]], want_r[bad[:8]])
        return
    okc = ok & _cos_ok(np.cos(np.where(ok, want_d, 0).astype(np.float64) * np.pi))
    np.testing.assert_allclose(dist[okc], want_d[okc], atol=ATOL, rtol=0)
    near = _near(full, mates, base)
    clear = near == 0
    assert clear.mean() >= min_clear, clear.mean()
    bad = np.flatnonzero(clear & (rank != want_r))
    assert bad.size == 0, (bad[:8], rank[bad[:8]], want_r[bad[:8]])
    assert (np.abs(rank - want_r) <= near).all()


def _np(t):
    return tuple(a.cpu().numpy() for a in t)


# ------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('B,G,D', [(1, 1, 32), (3, 129, 64), (65, 257, 512), (130, 1000, 128), (64, 4097, 512)])
def test_rank_shapes_and_mates(cuda, B, G, D, metric):
    """Tile tails in both dimensions, every probe-tile shape (<= 32, <= 64, more), more than one gallery tile; mates of the
    probe's own identity (a sparse band), random rows (dm near the median: a dense band), -1 and rows out of range."""
    from deep_insight_face import oneshot
    probes, gal_np, _ = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    unmated = np.array([-1, G, -2, G + 5, np.iinfo(np.int64).min, np.iinfo(np.int64).max], dtype=np.int64)
    mixed = _random_mates(B, G, seed=9)
    mixed[::2] = unmated[np.arange(len(mixed[::2])) % len(unmated)]
    cases = {'identity': _identity_mates(B, G, D), 'random': _random_mates(B, G), 'mixed': mixed,
             'above': np.full(B, G, dtype=np.int64), 'none': np.full(B, -1, dtype=np.int64)}
    if metric == 1:                                            # the cap, on the oracle, before the device is asked
        for name, mates in cases.items():
            assert (_near(full, mates) == 0).mean() >= 0.5, name
    gal = oneshot.Gallery(gal_np)
    for name, mates in cases.items():
        got = gal.rank(probes, mates, metric)
        assert all(isinstance(a, np.ndarray) for a in got)                      # NumPy in -> NumPy out
        _check(got, full, mates, metric)
        if name in ('above', 'none'):
            assert (got[0] == -1).all() and np.isnan(got[1]).all()
    mates = cases['identity']
    assert (rank_ref.rank_full(full, mates)[0] <= 4).all()                      # a sparse band: the mate is among its own few rows
    tr, td = gal.rank(torch.from_numpy(probes).cuda(), torch.from_numpy(mates).cuda(), metric)
    assert torch.is_tensor(tr) and tr.is_cuda and torch.is_tensor(td) and td.is_cuda   # CUDA tensors in -> CUDA tensors out
    assert tr.dtype == torch.int64 and td.dtype == torch.float32
    _check(_np((tr, td)), full, mates, metric)
    _check(gal.rank(probes, mates.astype(np.int32), metric), full, mates, metric)      # any integer dtype
    _check(_np(gal.rank(torch.from_numpy(probes).cuda(), torch.from_numpy(mates).to(torch.int16)
                        if G < 30000 else torch.from_numpy(mates), metric)), full, mates, metric)   # ... a host tensor too
    _check(oneshot.rank(probes, gal, mates, metric), full, mates, metric)       # the module-level form, on a handle
    _check(oneshot.rank(probes, gal_np, mates, metric), full, mates, metric)    # ... and on rows
    gal.close()


# ------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('metric', [0, 1])
def test_rank_exact_ties(cuda, metric):
    """Identical enrolled rows: as mates, in turn, they rank 0, 1, 2 in index order."""
    from deep_insight_face import oneshot
    probes, gal_np = gi.match_tie_inputs()
    copies = {0: (100, 300, 500), 1: (105, 305, 505), 2: (119, 319, 519), 3: (120, 320), 4: (139, 339), 5: (101, 301, 501),
              6: (110, 310, 510)}
    full = rank_ref.distances(probes, gal_np, metric)
    gal = oneshot.Gallery(gal_np)
    for turn in range(3):
        who = np.array([b for b, rows in copies.items() if len(rows) > turn])
        mates = np.array([copies[b][turn] for b in who], dtype=np.int64)
        for b, m in zip(who, mates):
            assert np.array_equal(gal_np[m], gal_np[copies[b][0]])
            others = np.delete(full[b], list(copies[b]))
            assert (others > full[b, m] + 1e-3).all()                           # nothing else anywhere near: exact on both metrics
        want = rank_ref.rank_full(full[who], mates)
        assert (want[0] == turn).all()
        rank, dist = gal.rank(probes[who], mates, metric)
        assert np.array_equal(rank, want[0]), (turn, rank)
        if metric == 0:
            assert np.array_equal(dist.view(np.uint32), want[1].view(np.uint32))
        else:
            np.testing.assert_allclose(dist, want[1], atol=ATOL, rtol=0)
    # one call, all copies of probe 0's row and a stranger: the same distance three times, three ranks
    assert _near(full[:1], np.array([7]))[0] == 0
    rank, dist = gal.rank(np.repeat(probes[:1], 4, axis=0), np.array([500, 100, 300, 7]), metric)
    assert list(rank[:3]) == [2, 0, 1] and dist[0] == dist[1] == dist[2] and rank[3] == rank_ref.rank_row(full[0], 7)[0]
    gal.close()


def test_rank_near_ties(cuda):
    """Rows one ulp, 1e-7 and 1e-4 apart and exact duplicates at shuffled positions: the five nearest oracle rows of each
    probe as mates, metric 0, bit-exact."""
    from deep_insight_face import oneshot
    probes, gal_np = gi.match_near_tie_inputs()
    full = rank_ref.distances(probes, gal_np, 0)
    order = np.argsort(full, axis=1, kind='stable')[:, :5]
    gal = oneshot.Gallery(gal_np)
    for k in range(5):
        want = rank_ref.rank_full(full, order[:, k])
        assert (want[0] == k).all()                                             # the stable argsort position
        _check(gal.rank(probes, order[:, k], 0), full, order[:, k], 0)
    gal.close()


# ------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('metric', [0, 1])
def test_rank_against_within_and_match(cuda, metric):
    """Device-only, exact on both metrics: the rank lies between the range search's counts just below and at the mate's
    distance, and it is 0 exactly when the arg-min is the mate."""
    from deep_insight_face import oneshot
    B, G, D = 130, 1000, 128
    probes, gal_np, _ = _inputs(B, G, D)
    gal = oneshot.Gallery(gal_np)
    p = torch.from_numpy(probes).cuda()
    mi, md = gal.match(p, metric)
    for name, mates in (('identity', torch.from_numpy(_identity_mates(B, G, D)).cuda()),
                        ('random', torch.from_numpy(_random_mates(B, G)).cuda()), ('argmin', mi)):
        rank, dist = _np(gal.rank(p, mates, metric))
        assert not np.isnan(dist).any() and (rank >= 0).all()
        n_single = 0
        for b in range(B):
            lo = int(gal.within(p[b:b + 1], np.nextafter(dist[b], NEG), metric, max_hits=0)[0][0])
            hi = int(gal.within(p[b:b + 1], dist[b], metric, max_hits=0)[0][0])
            assert lo <= rank[b] <= hi - 1, (name, b, lo, rank[b], hi)
            if hi == lo + 1:
                assert rank[b] == lo
                n_single += 1
        assert n_single >= B // 2                                               # the equality was really exercised: few rows tie
        hit = mi.cpu().numpy() == mates.cpu().numpy()
        assert np.array_equal(rank == 0, hit), name
        assert np.array_equal(dist[hit].view(np.uint32), md.cpu().numpy()[hit].view(np.uint32))
        if name == 'argmin':
            assert hit.all()
        if name == 'identity':
            assert hit.any() and not hit.all()
    gal.close()


# ------------------------------------------------------------------------------------------- 4
def _degenerate_mates(full, seed):
    """Per probe: the oracle's nearest finite row, a row whose oracle distance is NaN (where there is one), a random row."""
    B, G = full.shape
    rng = np.random.default_rng(seed)
    rand = rng.integers(0, G, B).astype(np.int64)
    fin = np.isfinite(full)
    nearest = np.where(fin.any(1), np.argmin(np.where(fin, full, np.inf), axis=1), rand).astype(np.int64)
    nan = np.isnan(full)
    nanrow = np.where(nan.any(1), np.argmax(nan, axis=1), rand).astype(np.int64)
    return {'nearest': nearest, 'nan': nanrow, 'random': rand}, nan


@pytest.mark.parametrize('name', [c[0] for c in gi.match_degenerate_cases()])
def test_rank_degenerate(cuda, name):
    """Zero, tiny, huge and non-finite rows and probes, anti-parallel rows: whatever IEEE arithmetic gives the reference; a
    NaN distance is never closer, a NaN mate ranks behind every row.  The probes that resolve every tile are among these."""
    from deep_insight_face import oneshot
    probes, gal_np = [(p, g) for n, p, g in gi.match_degenerate_cases() if n == name][0]
    G = gal_np.shape[0]
    gal = oneshot.Gallery(gal_np)
    for metric in (0, 1):
        full = rank_ref.distances(probes, gal_np, metric)
        sets, nan = _degenerate_mates(full, seed=metric)
        for kind, mates in sets.items():
            rank, dist = gal.rank(probes, mates, metric)
            _check((rank, dist), full, mates, metric, min_clear=0.5)
            at_nan = nan[np.arange(len(mates)), mates]
            assert (rank[at_nan] == G).all() and np.isnan(dist[at_nan]).all()
            assert (rank[~at_nan] < G).all() and (rank >= 0).all()
    gal.close()


# ------------------------------------------------------------------------------------------- 5
def test_rank_identical_probe_and_clamp_nan(cuda):
    """A probe equal to its enrolled mate: the reference's similarity may round above 1 and its distance is NaN then -- rank
    G, a miss, by default; with clamp_nan the clamped distance 0 is compared and the mate ranks first."""
    from deep_insight_face import oneshot
    _, gal_np, _ = _inputs(65, 257, 512)
    G = gal_np.shape[0]
    rows = np.arange(0, 256, 4).astype(np.int64)
    probes = gal_np[rows].copy()
    with np.errstate(invalid='ignore'):
        sim = od.similarity(probes, gal_np[rows])
    full = rank_ref.distances(probes, gal_np, 1)
    dself = full[np.arange(len(rows)), rows]
    assert (sim > 1).any() and (sim <= 1).any()                                # both outcomes occur in these 64 pairs
    assert np.array_equal(np.isnan(dself), sim > 1)
    gal = oneshot.Gallery(gal_np)
    rank, dist = gal.rank(probes, rows, 1)
    assert (rank[sim > 1] == G).all() and np.isnan(dist[sim > 1]).all()
    assert (rank[sim <= 1] == 0).all() and not np.isnan(dist[sim <= 1]).any()
    _check((rank, dist), full, rows, 1)
    gal.set_option('clamp_nan', 1)
    rank, dist = gal.rank(probes, rows, 1)
    assert (rank == 0).all() and not np.isnan(dist).any()
    assert (dist[sim >= 1] == 0).all()
    gal.close()


# ------------------------------------------------------------------------------------------- 6
def test_rank_handle_reuse_and_workspaces(cuda):
    """A non-monotone batch sequence on one handle, interleaved with within, match and update, against the recomputed
    oracle; a shard with an index_base."""
    from deep_insight_face import oneshot
    G, D = 4097, 128
    probes, gal_np, _ = _inputs(70, G, D)
    gal_np = gal_np.copy()
    mates = _identity_mates(70, G, D)
    mates[0] = mates[0] % (G // 4) + 2 * (G // 4)                               # probe 0: not the lowest row of its identity
    gal = oneshot.Gallery(gal_np)

    def check(n, metric=0):
        full = rank_ref.distances(probes[:n], gal_np, metric)
        got = gal.rank(probes[:n], mates[:n], metric)
        _check(got, full, mates[:n], metric)
        return got[0]

    r70 = check(70)
    gal.within(probes[:33], 0.5, 0, max_hits=8)                                 # the shared workspaces, another batch size
    check(33)
    row = gal_np[mates[0]][None]
    gal.update(np.repeat(row, 5, axis=0))                                       # appended copies of probe 0's mate: ties at
    gal_np = np.concatenate([gal_np, np.repeat(row, 5, axis=0)])                # higher indices, never counted
    assert len(gal) == G + 5
    r70b = check(70)
    assert r70b[0] == r70[0]
    full0 = rank_ref.distances(probes[:1], gal_np, 0)[0]
    low = int(np.flatnonzero(full0[:mates[0]] > full0[mates[0]])[0])            # a lower row that is farther than the mate
    gal.update(row, first_row=low)                                              # ... becomes a copy of it: a tie from below
    gal_np[low] = row[0]
    r70c = check(70)
    assert r70c[0] == r70[0] + 1
    m_mid = gal.match(probes, 0)
    assert np.array_equal(m_mid[0], od.match(probes, gal_np, 0)[0])
    check(33, 1)
    check(70, 1)
    gal.within(probes, 0.5, 1, max_hits=8)
    m_after = gal.match(probes, 0)
    assert np.array_equal(m_mid[0], m_after[0]) and np.array_equal(m_mid[1].view(np.uint32), m_after[1].view(np.uint32))
    gal.close()
    shifted = oneshot.Gallery(gal_np, index_base=1000)
    full = rank_ref.distances(probes, gal_np, 0)
    for m in (mates + 1000, mates):                                             # global indices; local ones name other rows or none
        want = rank_ref.rank_full(full, m, 1000)
        _check(shifted.rank(probes, m, 0), full, m, 0, base=1000)
        assert ((m < 1000) == (want[0] == -1)).all()
    assert (rank_ref.rank_full(full, mates + 1000, 1000)[0] >= 0).all() and (mates < 1000).any() and (mates >= 1000).any()
    shifted.close()


# ------------------------------------------------------------------------------------------- 7
def test_rank_arguments(cuda):
    from deep_insight_face import oneshot
    B, G, D = 3, 129, 64
    probes, gal_np, _ = _inputs(B, G, D)
    mates = np.array([5, -1, 128], dtype=np.int64)
    full = _oracle(B, G, D, 1)
    gal = oneshot.Gallery(gal_np)
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        gal.rank(probes, mates, distance_metric=7)
    with pytest.raises(ValueError):
        gal.rank(np.zeros((2, 32), dtype=np.float32), mates[:2])
    with pytest.raises(ValueError):
        gal.rank(probes, mates.astype(np.float32))                              # a float is not an index
    with pytest.raises(ValueError):
        gal.rank(probes, torch.from_numpy(mates).double())
    with pytest.raises(ValueError):
        gal.rank(probes, mates[:2])
    with pytest.raises(ValueError):
        gal.rank(probes, mates[None, :])
    _check(gal.rank(probes[0], mates[:1], 1), full[:1], mates[:1], 1)           # one probe as a vector
    p = torch.from_numpy(probes).cuda()
    m = torch.from_numpy(mates).cuda()
    rank = torch.empty(B, dtype=torch.int64, device='cuda')
    dist = torch.empty(B, dtype=torch.float32, device='cuda')
    gal.rank_into(p, m, 1, rank, dist)                                          # the well-formed call
    torch.cuda.synchronize()
    _check(_np((rank, dist)), full, mates, 1)
    with pytest.raises(RuntimeError, match='Undefined distance metric 2'):
        gal.rank_into(p, m, 2, rank, dist)
    wide = torch.empty(2 * B, dtype=torch.int64, device='cuda')
    for bad in (dict(rank=wide[::2]), dict(mates=wide[::2]),                                                # not contiguous
                dict(rank=rank.to(torch.int32)), dict(mate_dist=dist.double()), dict(mates=m.to(torch.int32)),   # wrong dtype
                dict(rank=rank[:2]), dict(mate_dist=dist[:2]), dict(mates=m[:2]), dict(rank=rank[None, :]),      # wrong shape
                dict(probes=p[:, :32]), dict(probes=probes),
                dict(rank=rank.cpu()), dict(mate_dist=dist.cpu()), dict(mates=m.cpu()), dict(probes=p.cpu())):   # host tensors
        kw = dict(probes=p, mates=m, rank=rank, mate_dist=dist)
        kw.update(bad)
        with pytest.raises(ValueError):
            gal.rank_into(kw['probes'], kw['mates'], 1, kw['rank'], kw['mate_dist'])
    r, d = gal.rank(np.zeros((0, D), dtype=np.float32), np.zeros(0, dtype=np.int64))   # an empty batch
    assert r.shape == (0,) and d.shape == (0,) and r.dtype == np.int64 and d.dtype == np.float32
    r, d = gal.rank(np.zeros((0, D), dtype=np.float32), [])                     # ... with an empty list of mates
    assert r.shape == (0,) and d.shape == (0,)
    with pytest.raises(ValueError):
        gal.rank(probes, np.array([5, None, 128], dtype=object))
    _check(gal.rank(probes, [5, -1, 128], 1), full, mates, 1)                   # a plain list of ints
    gal.close()
    empty = oneshot.Gallery(emd_size=D)                                         # nothing enrolled: everybody is unmated
    for metric in (0, 1):
        r, d = empty.rank(probes, np.array([0, -1, 5]), metric)
        assert r.dtype == np.int64 and (r == -1).all() and np.isnan(d).all()
    empty.close()


# ------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize('kind', ['numpy', 'tensor'])
def test_evaluate_identification(cuda, kind):
    """The protocol module on the device results: one rank call, one match call on the unmated probes."""
    from deep_insight_face import oneshot
    from deep_insight_face.evaluation import identification as ident
    B, G, D = 130, 1000, 128
    probes, gal_np, _ = _inputs(B, G, D)
    mates = _identity_mates(B, G, D)
    mates[::5] = -1
    full = _oracle(B, G, D, 0)
    want_r, want_d = rank_ref.rank_full(full, mates)
    um = full[mates < 0].min(1)
    th = np.quantile(full, [0.0, 0.001, 0.002, 0.01, 0.5, 1.0])
    conv = (lambda x: torch.from_numpy(x).cuda()) if kind == 'tensor' else (lambda x: x)
    back = (lambda x: x.cpu().numpy()) if kind == 'tensor' else (lambda x: x)
    gal = oneshot.Gallery(gal_np)
    for g in (gal, gal_np):
        out = ident.evaluate_identification(g, conv(probes), conv(mates), 0, max_rank=5, thresholds=th)
        assert sorted(out) == ['cmc', 'dir', 'far', 'mate_dist', 'rank', 'thresholds']
        assert all((torch.is_tensor(v) and v.is_cuda) if kind == 'tensor' else isinstance(v, np.ndarray) for v in out.values())
        assert np.array_equal(back(out['rank']), want_r)
        assert np.array_equal(back(out['mate_dist']).view(np.uint32), want_d.view(np.uint32))
        np.testing.assert_array_equal(back(out['cmc']), ident.cmc(want_r, 5))
        wd, wf = ident.open_set_rates(want_r, want_d, um, th)
        np.testing.assert_array_equal(back(out['dir']), wd)
        np.testing.assert_array_equal(back(out['far']), wf)
        np.testing.assert_array_equal(back(out['thresholds']), th)
        assert 0 < wd[2] < wd[-1] and wf[0] == 0 and wf[-1] == 1 and back(out['cmc'])[0] > 0.2
    out = ident.evaluate_identification(gal, conv(probes), conv(mates), 1)
    assert sorted(out) == ['cmc', 'mate_dist', 'rank'] and back(out['cmc']).shape == (10,)
    gal.close()


# ------------------------------------------------------------------------------------------- 9
# Rounds of probes (test_within_gpu.py's section 8): rank_run has within_run's loop and adds `mates + b0` at three launch
# sites, `mate_dist_out + b0` and `rank_out + b0`.  Gallery option "within_round" makes it take several rounds here.
ROUND_SHAPES = [(129, 257, 512), (300, 1000, 128), (384, 1000, 128)]


def _round_options(B):
    return (0, 128, 256, 0) if B == 300 else (0, 128, 0)


def _without_offset(arg, per):
    """What a launch that dropped its `+ b0` would read in rounds of `per`: probe b0 + j gets entry j."""
    return arg[np.arange(arg.shape[0]) % per]


def _round_mates(B, G, D):
    """A row of the probe's own identity; every 7th probe unmated (-1), every 11th with a mate beyond the gallery."""
    mates = _identity_mates(B, G, D).copy()
    mates[::7] = -1
    mates[::11] = G + 5
    return mates


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('B,G,D', ROUND_SHAPES)
def test_rank_rounds(cuda, B, G, D, metric):
    """"within_round" 0, 128 (and 256 at B = 300), 0 on one handle: every answer passes the oracle check, and the forced-round
    answers and the one after the option is taken back equal the first one-round answer bit for bit.  Before the device is
    asked: the oracle on the mates a dropped `+ b0` would read differs from the true one in every round after the first."""
    from deep_insight_face import oneshot
    probes, gal_np, _ = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    mates = _round_mates(B, G, D)
    want_r, want_d = rank_ref.rank_full(full, mates)
    assert (want_r[mates == -1] == -1).all() and (want_r[mates == G + 5] == -1).all() and (want_r >= 0).sum() > B // 2
    for per in _round_options(B)[1:-1]:
        r, d = rank_ref.rank_full(full, _without_offset(mates, per))
        differs = (r != want_r) | (np.isnan(d) != np.isnan(want_d)) | (~np.isnan(d) & ~np.isnan(want_d) & (d != want_d))
        for b0 in range(per, B, per):
            assert differs[b0:b0 + per].any(), (per, b0)
    if metric == 1:
        assert (_near(full, mates) == 0).mean() >= 0.5                          # the cap, on the oracle
    gal = oneshot.Gallery(gal_np)
    first = None
    for per in _round_options(B):
        gal.set_option('within_round', per)
        got = gal.rank(probes, mates, metric)
        _check(got, full, mates, metric)
        first = first or got
        assert np.array_equal(got[0], first[0]), (per, np.flatnonzero(got[0] != first[0])[:8])
        assert np.array_equal(np.isnan(got[1]), np.isnan(first[1]))
        ok = ~np.isnan(first[1])
        assert np.array_equal(got[1][ok].view(np.uint32), first[1][ok].view(np.uint32)), per
    with pytest.raises(ValueError, match='within_round'):
        gal.set_option('within_round', 100)                                     # not a multiple of 128
    gal.close()
