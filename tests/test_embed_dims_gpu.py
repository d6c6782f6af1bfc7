"""The embedding size D is not a passive parameter of the 1:N side: it shapes the summation tree the device restates
(match_ref.hpp: SumPlan), selects the filter copy and its kernels (match.hip: one_term_fits / g1_dims / one_term_frag),
enters every copy's addressing and widens the key-error band.  These tests run dif_pairwise over every plan shape and every
gallery query at one size per class (tests/embed_dims.py), each through the query's own checker and reference."""
import numpy as np
import pytest
import torch

import cluster_ref as cr
import dbscan_ref as dr
import embed_dims as ed
import rank_ref
import remove_ref
import roc_ref
import test_cluster_gpu as cl
import test_dbscan_gpu as db
import test_rank_gpu as rk
import test_roc_gpu as rc
import test_topk_gpu as tk
import test_topk_ids_gpu as ti
import test_within_gpu as wi
from oracle import distance as od

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ dif_pairwise
def _pairwise(a, b, metric):
    from deep_insight_face import _native as N
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    n = max(a.shape[0], b.shape[0])
    out = torch.empty(n, dtype=torch.float32, device='cuda')
    N.check(N.lib.dif_pairwise(N.ptr(ta), a.shape[0], N.ptr(tb), b.shape[0], a.shape[1], metric, N.ptr(out),
                               N.stream_ptr()))
    return out.cpu().numpy()


def _pairwise_misses(a, b):
    """Names of the rules of test_reference_arithmetic_bit_exact that dif_pairwise misses on (a, b): metric 0 and the
    similarity (metric 2) bit-identical to NumPy, metric 1 within 4 ulp where NumPy is finite and NaN where it is NaN."""
    bad = []
    for metric, want in ((0, od.distance(a, b, 0)), (2, od.similarity(a, b))):
        got = _pairwise(a, b, metric)
        if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            bad.append('metric %d: %d rows' % (metric, (got.view(np.uint32) != want.view(np.uint32)).sum()))
    with np.errstate(invalid='ignore'):
        want1 = od.distance(a, b, 1)
    got1 = _pairwise(a, b, 1)
    ok = ~np.isnan(want1)
    if ok.any():
        ulps = np.abs(got1[ok].view(np.int32).astype(np.int64) - want1[ok].view(np.int32)).max()
        if ulps > 4:
            bad.append('metric 1: %d ulp' % ulps)
    if not np.all(np.isnan(got1[~ok])):
        bad.append('metric 1: a number where NumPy has NaN')
    return bad


@pytest.mark.parametrize('sizes', [ed.PAIR_SMALL, ed.PAIR_LARGE, ed.PAIR_65], ids=['1-300', 'large', '65-leaves'])
def test_pairwise_every_plan_shape(cuda, sizes):
    """dif_pairwise promises NumPy's float32 result on [1, 8192]: 64 scaled rows per size, all three metrics.  The sizes of
    the third list are the ones whose tree has 65 leaves; a plan cut off at 64 sums their last 129..135 elements as one block
    and differs from NumPy in the last bit on about one row in twenty."""
    failed = {}
    for d in sizes:
        bad = _pairwise_misses(*ed.pair_rows(d))
        if bad:
            failed[d] = bad
    assert not failed, 'sizes that differ from NumPy: %s' % failed


def test_pairwise_broadcast_at_65_leaves(cuda):
    a, b = ed.pair_rows(7690)
    for one, many in ((a[3:4], b), (b[7:8], a)):
        assert not _pairwise_misses(one, many)
        assert not _pairwise_misses(many, one)


def test_pairwise_size_out_of_range(cuda):
    a = np.ones((2, 8193), dtype=np.float32)
    for metric in (0, 1, 2):
        with pytest.raises(RuntimeError, match=r'outside \[1, 8192\]'):
            _pairwise(a, a, metric)


# ------------------------------------------------------------------------------------------------ gallery queries
# Every query at embed_dims.QUERY_SHAPES, both metrics, through the checker and the reference module of the query's own test
# file (imported, not restated) on test_topk_gpu.py's inputs: identities with four near-duplicate rows each.
shapes = pytest.mark.parametrize('B,G,D', ed.QUERY_SHAPES)
metrics = pytest.mark.parametrize('metric', [0, 1])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gallery(rows, flt=None, frag=None):
    from deep_insight_face import oneshot
    gal = oneshot.Gallery(emd_size=rows.shape[1])
    if flt is not None:
        gal.set_option('filter', flt)
    if frag is not None:
        gal.set_option('frag', frag)
    gal.set(rows)
    return gal


def _filter_terms(flt, D):
    """bf16 terms per operand the filter runs on (0: the f32 rows): the one-term copy needs D % 64 == 0 and D >= 128."""
    return 0 if flt == 0 else (2 if flt == 1 or D in ed.TWO_TERM_DIMS else 1)


@shapes
def test_match_on_every_filter(cuda, B, G, D):
    """np.argmin of the oracle under "filter" 0, 1, 2 and "frag" 0, 2; the stats say which copy the match ran on: two bf16
    terms at D % 64 != 0 even when one is asked for, one term row-major at the others -- none of these sizes has the
    fragment-order copy, "frag" 2 or not -- and every setting returns the same index, distance and key, bit for bit."""
    probes, gal_np, _ = tk._inputs(B, G, D)
    first, exact = {}, {}
    for flt in (0, 1, 2):
        for frag in (0, 2):
            gal = _gallery(gal_np, flt, frag)
            for metric in (0, 1):
                full = tk._oracle(B, G, D, metric)
                assert not np.isnan(full).any()
                idx, dist, key = gal.match(probes, metric, return_key=True)
                exact[(flt, frag, metric)] = gal.stat('exact_probes')
                tag = (flt, frag, metric, 'exact_probes', exact)
                assert gal.stat('filter_terms') == _filter_terms(flt, D) and gal.stat('frag_copy') == 0, tag
                want_i = np.argmin(full, axis=1)
                assert np.array_equal(idx, want_i), (tag, np.flatnonzero(idx != want_i)[:8])
                want_d = full[np.arange(B), want_i]
                if metric == 0:
                    assert np.array_equal(_bits(dist), _bits(want_d)), tag
                else:
                    np.testing.assert_allclose(np.cos(dist.astype(np.float64) * np.pi),
                                               np.cos(want_d.astype(np.float64) * np.pi), atol=tk.ATOL, err_msg=str(tag))
                got = (idx, _bits(dist), _bits(key))
                for a, b in zip(got, first.setdefault(metric, got)):
                    assert np.array_equal(a, b), tag
            gal.close()


@metrics
@shapes
def test_within(cuda, B, G, D, metric):
    """A tolerance in the widest gap of the oracle's distances (a probe's own identity: a few hits) and the median (half the
    gallery), listed (max_hits 64) and counted only (0).  Metric 1 at the median follows test_within_metric1_dense: outside
    the pairs within NEAR of the tolerance the hit mask is the oracle's."""
    probes, gal_np, _ = tk._inputs(B, G, D)
    full = tk._oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    t, gap = wi._sparse_t(full)
    assert gap >= 1e-3, gap
    few = wi._expect(full, t, 64)[0]
    assert 1 <= few.min() and few.max() <= 8, (few.min(), few.max())
    dense = wi._median_t(full)
    gal = _gallery(gal_np)
    for K in (0, 64):
        wi._check(gal.within(probes, t, metric, max_hits=K), wi._expect(full, t, K), metric)
        if metric == 0:
            wi._check(gal.within(probes, dense, 0, max_hits=K), wi._expect(full, dense, K), 0)
    if metric == 1:
        # The share of pairs within NEAR of the median: the strangers' distances are normal about 1/2 with sigma = 1 / (pi sqrt(D)),
        # so a window of 2 NEAR holds 4e-6 pi sqrt(D) / sqrt(2 pi) = 5e-6 sqrt(D) of them, 4.6e-4 at D = 8192 (0.3 pairs of that
        # shape's 650).  1 % leaves room for the small shapes and still has 99 % of the pairs compared exactly.
        near = np.abs(full.astype(np.float64) - float(dense)) <= wi.NEAR
        assert near.mean() <= 0.01, near.mean()
        cnt, mask = wi._device_mask(gal, probes, dense, 1, G)
        wi._check_near(cnt, mask, full, dense)
        assert np.median(cnt) >= G // 3
        c0, i0, d0 = gal.within(probes, dense, 1, max_hits=0)                    # counted only, and the first 64 of the list
        assert np.array_equal(c0, cnt) and i0.shape == (B, 0)
        c64, i64, d64 = gal.within(probes, dense, 1, max_hits=64)
        assert np.array_equal(c64, cnt)
        for b in range(B):
            n = min(64, int(cnt[b]))
            rows = np.flatnonzero(mask[b])[:n]
            assert np.array_equal(i64[b, :n], rows) and (i64[b, n:] == -1).all()
            wi._check_dist(d64[b, :n], full[b, rows], 1)
    gal.close()


@metrics
@shapes
def test_rank(cuda, B, G, D, metric):
    """The mate is a row of the probe's own identity (test_rank_shapes_and_mates' 'identity' case)."""
    probes, gal_np, pick = tk._inputs(B, G, D)
    full = tk._oracle(B, G, D, metric)
    nid = max(1, G // 4)
    mates = (pick + nid * (np.arange(B) % 4)).astype(np.int64)
    assert mates.max() < G
    if metric == 1:
        assert (rk._near(full, mates) == 0).mean() >= 0.5                        # the cap, on the oracle alone
    assert (rank_ref.rank_full(full, mates)[0] <= 4).all()
    gal = _gallery(gal_np)
    rk._check(gal.rank(probes, mates, metric), full, mates, metric)
    gal.close()


@metrics
@shapes
def test_topk(cuda, B, G, D, metric):
    probes, gal_np, _ = tk._inputs(B, G, D)
    full = tk._oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    for k in (1, 5, 128):
        tk._cap(full, k, metric)
    gal = _gallery(gal_np)
    for k in (1, 5, 128):
        tk._check(gal.topk(probes, k, metric), full, k, metric)
    gal.close()


@metrics
@shapes
def test_topk_ids(cuda, B, G, D, metric):
    """The labels are the identities ('spread' of test_topk_ids_gpu.py: row i belongs to identity i % (G // 4))."""
    probes, gal_np, _ = tk._inputs(B, G, D)
    full = tk._oracle(B, G, D, metric)
    labels = ti._labellings(G)['spread']
    for k in (1, 5):
        ti._cap(full, labels, k, metric)
    gal = _gallery(gal_np)
    for k in (1, 5):
        ti._check(gal.topk_ids(probes, k, labels, metric), full, labels, k, metric)
    gal.close()


@metrics
@shapes
def test_roc(cuda, B, G, D, metric):
    """A grid of 100 thresholds (test_roc_gpu.py's _thresholds: the grid with duplicates, infinities and actual distances among
    it): metric 0 the oracle's counts; metric 1 the counts of the library's own distances, and NumPy's within NEAR."""
    probes, gal_np, pick = tk._inputs(B, G, D)
    full = tk._oracle(B, G, D, metric)
    pl, rl = pick.astype(np.int64), (np.arange(G) % max(1, G // 4)).astype(np.int64)
    lib = rc._lib_full(probes, gal_np) if metric == 1 else full
    t = rc._thresholds(lib, 100, metric, seed=B + D)
    gal = _gallery(gal_np)
    got = rc._roc(gal, probes, pl, rl, t, metric)
    rc._same(got, roc_ref.counts_full(lib, pl, rl, t))
    if metric == 1:
        rc._within_numpy(got, full, pl, rl, t)
    assert got[1][0] > 0 and got[1][0] + got[1][1] == B * G and got[0][:, 0].max() > 0
    gal.close()


@metrics
@shapes
def test_cluster_and_dbscan(cuda, B, G, D, metric):
    """The first min(G, 515) rows at the tolerance in the widest gap of their pairwise distances (test_cluster_gpu.py's rule,
    the gap asserted on the CPU): the identities, and DBSCAN at min_samples 1 and 3."""
    _, gal_np, _ = tk._inputs(B, G, D)
    n = min(G, 515)
    rows = gal_np[:n]
    lower = cr.lower_distances(rows, metric)
    (t,) = cl._gap_t(cr.pair_values(lower))
    gal = _gallery(rows)
    cl._same(cl._run(gal, t, metric), cr.cluster_from(lower, n, t))
    for ms in (1, 3):
        db._same(db._run(gal, t, ms, metric), dr.dbscan_from(lower, n, t, ms))
    gal.close()


@pytest.mark.parametrize('B,G,D', [s for s in ed.QUERY_SHAPES if s[2] in (96, 320, 1024)])
def test_copies_follow_update_and_remove(cuda, B, G, D):
    """Half the rows set and the capacity reserved, the rest appended, ten rows in the middle overwritten, 40 scattered rows
    removed -- under every filter: match and topk then answer as a fresh handle set with the surviving rows does, index for index
    and bit for bit (the scheme of test_gallery_update_equals_set and test_remove_equals_fresh_set), and as the oracle."""
    from deep_insight_face import oneshot
    probes, gal_np, _ = tk._inputs(B, G, D)
    new = tk._inputs(B, G, D, seed=1)[1][:10]
    mid = G // 2 - 5                                                             # five rows of the set half, five of the appended
    gone = np.random.default_rng(G + D).permutation(G)[:40].astype(np.int64)
    cur = gal_np.copy()
    cur[mid:mid + 10] = new
    cur = remove_ref.remove_ref(cur, gone)[0]
    assert cur.shape[0] == G - 40

    def answers(gal):
        out = []
        for metric in (0, 1):
            i, d, k = gal.match(probes, metric, return_key=True)
            ti_, td = gal.topk(probes, 5, metric)
            out += [i, _bits(d), _bits(k), ti_, _bits(td)]
        return out

    for flt in (0, 1, 2):
        gal = oneshot.Gallery(emd_size=D)
        gal.set_option('filter', flt)
        gal.set(gal_np[:G // 2])
        gal.reserve(G)
        gal.match(probes, 1)                                                     # the filter's copy exists before the rows change
        gal.update(gal_np[G // 2:])
        gal.update(new, mid)
        assert len(gal) == G and gal.capacity == G
        gal.remove(gone)
        assert len(gal) == G - 40
        got = answers(gal)
        assert gal.stat('filter_terms') == _filter_terms(flt, D) and gal.stat('frag_copy') == 0, flt
        fresh = _gallery(cur, flt)
        for n, (a, b) in enumerate(zip(got, answers(fresh))):
            assert np.array_equal(a, b), (flt, n)
        fresh.close()
        gal.close()
        full = rank_ref.distances(probes, cur, 0)
        assert np.array_equal(got[0], np.argmin(full, axis=1)), flt
        tk._check((got[3], got[4].view(np.float32)), full, 5, 0)
