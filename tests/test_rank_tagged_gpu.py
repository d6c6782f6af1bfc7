"""The tagged rank of the mate (oneshot.Gallery.rank with `row_tags` and `probe_masks` / dif_match_rank_tagged) against
tests/tagged_queries_ref.py over the CPU oracle's distances: for every probe

    d = oracle.distance.distance(q[None, :], gallery, metric);  d[~eligible[p]] = NaN;  rank_ref.rank_row(d, mates[p], index_base)

-- the rank among the rows the probe may see; an ineligible mate ranks behind every row (G, mate_dist NaN), an unmated probe
stays -1 -- under tests/test_rank_gpu.py's rules: metric 0 bit for bit; metric 1 exact on the CLEAR probes (no eligible row
within 2e-6 of the mate's distance), the others within the number of such rows, mate_dist within 1e-5.  Also
evaluation.identification.evaluate_identification with tags.  tests/test_tagged_queries_ref.py asserts, without a GPU, the input
conditions relied on here."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import rank_ref
import remove_ref
import tagged_queries_cases as tc
import tagged_queries_ref as tq
import tagged_ref
from test_rank_gpu import ATOL, _check, _near

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
        if x.dtype.kind == 'f':
            assert np.array_equal(np.isnan(x), np.isnan(y))
            assert np.array_equal(x[~np.isnan(x)], y[~np.isnan(y)])
        else:
            assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('B,G,D', tc.SHAPES)
def test_rank_tagged_shapes_and_mates(cuda, B, G, D, metric):
    """Tile tails in both dimensions, every probe-tile shape, more than one gallery tile; the mates of
    tagged_queries_ref.case_mates: eligible and ineligible ones, of the probe's identity and random, unmated."""
    from deep_insight_face import oneshot
    probes, gal_np, pick, tags, masks, mates = tc.case(B, G, D)
    fm = tc.masked(B, G, D, metric)
    el = tagged_ref.eligible(tags, masks)
    mate_el = np.array([mates[b] >= 0 and el[b, mates[b]] for b in range(B)])
    cases = {'case': mates, 'first': (pick % max(1, G // 4)).astype(np.int64), 'none': np.full(B, -1, dtype=np.int64)}
    if metric == 1:                                            # the cap, on the oracle, before the device is asked
        for name, m in cases.items():
            assert (_near(fm, m) == 0).mean() >= 0.9, name
    gal = oneshot.Gallery(gal_np)
    for name, m in cases.items():
        got = gal.rank(probes, m, metric, tags, masks)
        assert all(isinstance(a, np.ndarray) for a in got)                      # NumPy in -> NumPy out
        _check(got, fm, m, metric, min_clear=0.9)
        if name == 'none':
            assert (got[0] == -1).all() and np.isnan(got[1]).all()
    rank, dist = gal.rank(probes, mates, metric, tags, masks)
    assert (rank[mates < 0] == -1).all()
    assert (rank[(mates >= 0) & ~mate_el] == G).all() and np.isnan(dist[~mate_el]).all()   # ineligible: behind every row
    assert (rank[mate_el] < G).all() and (rank[mate_el] >= 0).all() and not np.isnan(dist[mate_el]).any()
    dev = gal.rank(torch.from_numpy(probes).cuda(), torch.from_numpy(np.array(mates)).cuda(), metric,
                   torch.from_numpy(np.array(tags)).cuda(), torch.from_numpy(np.array(masks)).cuda())
    assert all(torch.is_tensor(a) and a.is_cuda for a in dev)                   # CUDA tensors in -> CUDA tensors out
    assert dev[0].dtype == torch.int64 and dev[1].dtype == torch.float32
    _check(_np(dev), fm, mates, metric, min_clear=0.9)
    _check(oneshot.rank(probes, gal, mates, metric, tags, masks), fm, mates, metric, min_clear=0.9)   # the module-level form
    _check(oneshot.rank(probes, gal_np, mates, metric, row_tags=tags, probe_masks=masks), fm, mates, metric, min_clear=0.9)
    six = tagged_ref.masked(tc.oracle(B, G, D, metric), tags, np.full(B, 6, dtype=np.int64))
    _check(gal.rank(probes, mates, metric, tags, 6), six, mates, metric)        # a Python int stands for every probe
    gal.close()


# ------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('metric', [0, 1])
def test_rank_tagged_equals_the_gallery_of_the_eligible_rows(cuda, metric):
    """Per mask value: the tagged rank is the untagged rank in a gallery that holds the eligible rows alone, the mate's row
    mapped -- device against device, bit for bit on both metrics; with every pair eligible, the untagged call's."""
    from deep_insight_face import oneshot
    B, G, D = 130, 1000, 128
    probes, gal_np, _, tags, masks, mates = tc.case(B, G, D)
    gal = oneshot.Gallery(gal_np)
    got = gal.rank(probes, mates, metric, tags, masks)
    for m in tagged_ref.MASK_CYCLE:
        who = np.flatnonzero(masks == m)
        ok = tagged_ref.eligible(tags, np.array([m]))[0]
        rows = np.flatnonzero(ok)
        mine = mates[who]
        seen = (mine >= 0) & ok[np.maximum(mine, 0)]
        assert (got[0][who][(mine >= 0) & ~seen] == G).all() and np.isnan(got[1][who][~seen]).all()
        if len(rows) == 0 or not seen.any():
            continue
        sub = oneshot.Gallery(gal_np[rows])
        r, d = sub.rank(probes[who][seen], np.searchsorted(rows, mine[seen]), metric)
        sub.close()
        _same((got[0][who][seen], got[1][who][seen]), (r, d))
    plain = gal.rank(probes, mates, metric)
    _same(gal.rank(probes, mates, metric, np.full(G, -1, dtype=np.int64), np.full(B, -1, dtype=np.int64)), plain)
    _same(gal.rank(probes, mates, metric, np.full(G, tc.TOP, dtype=np.int64), -1), plain)
    assert (plain[0] != got[0]).mean() >= 0.75
    gal.close()


# ------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('metric', [0, 1])
def test_rank_tagged_exact_ties_across_an_eligibility_boundary(cuda, metric):
    """Identical enrolled rows (test_rank_exact_ties' table): an ineligible copy of the mate at a lower row does not count,
    an eligible one does."""
    from deep_insight_face import oneshot
    probes, gal_np = gi.match_tie_inputs()
    G = gal_np.shape[0]
    copies = {0: (100, 300, 500), 1: (105, 305, 505), 5: (101, 301, 501), 6: (110, 310, 510)}
    full = rank_ref.distances(probes, gal_np, metric)
    who = np.array(sorted(copies))
    last = np.array([copies[b][2] for b in who], dtype=np.int64)
    for b in who:
        others = np.delete(full[b], list(copies[b]))
        assert (others > full[b, copies[b][0]] + 1e-3).all()                     # nothing else anywhere near: exact on both metrics
    gal = oneshot.Gallery(gal_np)
    assert list(gal.rank(probes[who], last, metric)[0]) == [2, 2, 2, 2]         # untagged: both lower copies tie from below
    for hidden, want in (((100, 200), 1), ((300, 400), 1), ((100, 400), 0)):
        tags = np.ones(G, dtype=np.int64)
        tags[hidden[0]:hidden[1]] = 2                                           # these copies are not mask 1's
        rank, dist = gal.rank(probes[who], last, metric, tags, 1)
        want_r, want_d = tq.rank_full(full[who], last, tags, np.ones(len(who), dtype=np.int64))
        assert list(want_r) == [want] * 4 and list(rank) == [want] * 4, (hidden, rank)
        np.testing.assert_allclose(dist, want_d, atol=0 if metric == 0 else ATOL, rtol=0)
        r3, _ = gal.rank(probes[who], last, metric, tags, 3)                    # mask 3 sees them again
        assert list(r3) == [2] * 4
        first = np.array([copies[b][0] for b in who], dtype=np.int64)           # the hidden copy as the mate: behind every row
        if hidden[0] == 100:
            rank, dist = gal.rank(probes[who], first, metric, tags, 1)
            assert (rank == G).all() and np.isnan(dist).all()
    gal.close()


def test_rank_tagged_near_ties(cuda):
    """Rows one ulp, 1e-7 and 1e-4 apart and exact duplicates at shuffled positions, a quarter of the rows nobody's: the five
    nearest eligible rows of each probe as mates rank 0 .. 4; metric 0, bit-exact."""
    from deep_insight_face import oneshot
    probes, gal_np = gi.match_near_tie_inputs()
    G, B = gal_np.shape[0], probes.shape[0]
    tags = np.random.default_rng(3).integers(0, 4, G).astype(np.int64)
    masks = np.array([1, 2, 3], dtype=np.int64)[np.arange(B) % 3]
    fm = tagged_ref.masked(rank_ref.distances(probes, gal_np, 0), tags, masks)
    order = np.argsort(fm, axis=1, kind='stable')[:, :5]                         # (NaN sorts last)
    assert not np.isnan(np.take_along_axis(fm, order, 1)).any()
    gal = oneshot.Gallery(gal_np)
    for k in range(5):
        want = rank_ref.rank_full(fm, order[:, k])
        assert (want[0] == k).all()
        _check(gal.rank(probes, order[:, k], 0, tags, masks), fm, order[:, k], 0)
    gal.close()


# ------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('name', [c[0] for c in gi.match_degenerate_cases()])
def test_rank_tagged_degenerate(cuda, name):
    """Zero, tiny, huge and non-finite rows and probes, anti-parallel rows -- the probes that resolve every tile are among
    these -- with the odd rows eligible for every second probe only; mates: the nearest eligible finite row, a row whose
    masked distance is NaN, a random row."""
    from deep_insight_face import oneshot
    probes, gal_np = [(p, g) for n, p, g in gi.match_degenerate_cases() if n == name][0]
    B, G = probes.shape[0], gal_np.shape[0]
    fulls = {metric: tc.distances(probes, gal_np, metric) for metric in (0, 1)}
    tags, masks = tc.degenerate_tags(fulls, B)
    gal = oneshot.Gallery(gal_np)
    for metric in (0, 1):
        fm = tagged_ref.masked(fulls[metric], tags, masks)
        rng = np.random.default_rng(metric)
        rand = rng.integers(0, G, B).astype(np.int64)
        fin, nan = np.isfinite(fm), np.isnan(fm)
        nearest = np.where(fin.any(1), np.argmin(np.where(fin, fm, np.inf), axis=1), rand).astype(np.int64)
        nanrow = np.where(nan.any(1), np.argmax(nan, axis=1), rand).astype(np.int64)
        for mates in (nearest, nanrow, rand):
            rank, dist = gal.rank(probes, mates, metric, tags, masks)
            _check((rank, dist), fm, mates, metric, min_clear=0.5)
            at_nan = nan[np.arange(B), mates]
            assert (rank[at_nan] == G).all() and np.isnan(dist[at_nan]).all()
            assert (rank[~at_nan] < G).all() and (rank >= 0).all()
    gal.close()


# ------------------------------------------------------------------------------------------- 5
def test_rank_tagged_skip_rule(cuda):
    """test_within_tagged_skip_rule's gallery: 516 tiles, bit 2 on 100 rows of two of them, nine probes with mask 4 -- the last
    one outside the bound's validity, for which the untagged rule resolves all 516 tiles -- and an eligible mate: at most the
    two tiles that hold an eligible row are evaluated per probe."""
    from deep_insight_face import oneshot
    probes, gal_np, tags = tc.skip_case()
    n, G = probes.shape[0], gal_np.shape[0]
    masks = np.full(n, 4, dtype=np.int64)
    fm = tagged_ref.masked(tc.distances(probes, gal_np, 1), tags, masks)
    rows = np.flatnonzero(tags & 4)
    mates = rows[(np.arange(n) * 11) % len(rows)].astype(np.int64)
    assert (_near(fm, mates) == 0).all()
    gal = oneshot.Gallery(gal_np)
    got = gal.rank(probes, mates, 1, tags, masks)
    tiles = gal.stat('within_tagged_tiles')
    print('within_tagged_tiles (rank)', tiles)
    _check(got, fm, mates, 1, min_clear=1.0)
    assert (got[0] < 100).all() and len(set(got[0])) > 1
    assert 0 < tiles <= 2 * n, tiles
    r8, d8 = gal.rank(probes, mates, 1, tags, 8)                                # nothing carries bit 3: the mate neither
    assert gal.stat('within_tagged_tiles') == 0 and (r8 == G).all() and np.isnan(d8).all()
    gal.rank(probes, mates, 1)                                                   # an untagged call leaves the stat alone
    assert gal.stat('within_tagged_tiles') == 0
    gal.close()


# ------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize('metric', [0, 1])
def test_rank_tagged_rounds(cuda, metric):
    """B = 300 with "within_round" 128, then 0, on one handle: the masks (and mates) of the second and third round are taken
    at their offsets -- before the device is asked: the oracle under the masks a dropped `+ b0` would read differs in both
    later rounds; equal answers and equal tile counts whatever the split."""
    from deep_insight_face import oneshot
    B, G, D = 300, 1000, 128
    probes, gal_np, pick, tags, _, _ = tc.case(B, G, D)
    masks = tc.round_masks(B)
    mates = tq.case_mates(B, G, pick, tags, masks)
    full = tc.oracle(B, G, D, metric)
    fm = tagged_ref.masked(full, tags, masks)
    want = rank_ref.rank_full(fm, mates)
    wrong = tq.rank_full(full, mates, tags, masks[np.arange(B) % 128])
    for sl in (slice(128, 256), slice(256, 300)):
        assert (wrong[0][sl] != want[0][sl]).any()
    gal = oneshot.Gallery(gal_np)
    p, m_, t_dev, m_dev = (torch.from_numpy(np.array(a)).cuda() for a in (probes, mates, tags, masks))
    answers, tiles = [], []
    for per in (0, 128, 0):
        gal.set_option('within_round', per)
        got = _np(gal.rank(p, m_, metric, t_dev, m_dev))
        tiles.append(gal.stat('within_tagged_tiles'))
        _check(got, fm, mates, metric, min_clear=0.9)
        answers.append(got)
    _same(answers[1], answers[0])
    _same(answers[2], answers[0])
    assert tiles[0] > 0 and tiles == [tiles[0]] * 3, tiles
    gal.close()


# ------------------------------------------------------------------------------------------- 7
def test_rank_tagged_handle_reuse(cuda):
    """A non-monotone batch sequence on one handle, interleaved with untagged `rank`, `within`, `match`, `update` and
    `remove` -- tags permuted by the reported moves -- against the recomputed oracle; a handle with index_base 1000."""
    from deep_insight_face import oneshot
    B, G, D = 64, 4097, 128
    probes, gal_np, _, tags, masks, mates = tc.case(B, G, D)
    gal_np, tags, mates = gal_np.copy(), np.array(tags), np.array(mates)
    gal = oneshot.Gallery(gal_np)

    def check(n, metric=0):
        fm = tagged_ref.masked(tc.distances(probes[:n], gal_np, metric), tags, masks[:n])
        got = gal.rank(probes[:n], mates[:n], metric, tags, masks[:n])
        _check(got, fm, mates[:n], metric, min_clear=0.9)
        return got

    plain = gal.rank(probes, mates, 0)
    first = check(64)
    check(3)
    gal.match(probes[:33], 0)
    gal.within(probes[:17], 1.0, 1, 4, tags, masks[:17])
    check(33)
    _same(gal.rank(probes, mates, 0), plain)                                    # the untagged call between tagged ones
    _same(check(64), first)
    assert masks[0] == 1 and first[0][0] >= 0 and first[0][0] < G
    row = gal_np[mates[0]][None]                                                # probe 0's mate, five more times behind it:
    gal.update(np.repeat(row, 5, axis=0))
    gal_np = np.concatenate([gal_np, np.repeat(row, 5, axis=0)])
    tags = np.concatenate([tags, np.array([1, 0, 3, 2, tc.TOP | 1], dtype=np.int64)])
    assert check(64)[0][0] == first[0][0]                                       # ties at higher rows do not count
    mates[0] = G + 4                                                            # the last copy: the mate and two eligible copies tie from below
    assert check(64)[0][0] == first[0][0] + 3
    gone = np.array([7, 4000, G + 2], dtype=np.int64)
    moved_from, moved_to = gal.remove(gone)
    gal_np = remove_ref.remove_ref(gal_np, gone)[0]
    new_tags = tags[:gal_np.shape[0]].copy()
    new_tags[moved_to] = tags[moved_from]                                       # the caller's tables follow the moves
    assert np.array_equal(new_tags, remove_ref.remove_ref(tags, gone)[0])
    tags = new_tags
    relabel = np.arange(G + 5)
    relabel[gone] = -1
    relabel[moved_from] = moved_to
    mates = np.where(mates >= 0, relabel[np.maximum(mates, 0)], -1)
    assert len(gal) == gal_np.shape[0] == G + 2
    check(64)
    check(33, 1)
    gal.close()
    shifted = oneshot.Gallery(gal_np, index_base=1000)
    fm = tagged_ref.masked(tc.distances(probes, gal_np, 0), tags, masks)
    up = np.where(mates >= 0, mates + 1000, -1)
    got = shifted.rank(probes, up, 0, tags, masks)
    _check(got, fm, up, 0, base=1000)
    assert (got[0][up < 0] == -1).all() and (got[0] >= 0).any()
    shifted.close()


# ------------------------------------------------------------------------------------------- 8
def test_rank_tagged_arguments(cuda):
    from deep_insight_face import _native as N
    from deep_insight_face import oneshot
    B, G, D = 3, 129, 64
    probes, gal_np, _, tags, masks, mates = tc.case(B, G, D)
    fm = tc.masked(B, G, D, 1)
    gal = oneshot.Gallery(gal_np)
    for kw in (dict(row_tags=tags), dict(probe_masks=masks), dict(probe_masks=1)):        # exactly one given
        with pytest.raises(ValueError, match='go together'):
            gal.rank(probes, mates, 1, **kw)
        with pytest.raises(ValueError, match='go together'):
            oneshot.rank(probes, gal, mates, 1, **kw)
    for bad_t, bad_m in ((tags.astype(np.float32), masks), (tags, masks.astype(np.float64)), (tags != 0, masks),
                         (tags, masks != 0), (tags[:-1], masks), (tags, masks[:2]), (tags[None], masks), (tags, masks[:, None]),
                         (torch.from_numpy(np.array(tags)).float(), masks), (tags, torch.from_numpy(np.array(masks)) != 0),
                         (tags, 1.0), (tags, True), (tags, 1 << 64), (tags, -(1 << 63) - 1), (3, masks)):
        with pytest.raises(ValueError):
            gal.rank(probes, mates, 1, bad_t, bad_m)
    with pytest.raises(ValueError):
        gal.rank(probes, mates.astype(np.float32), 1, tags, masks)
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        gal.rank(probes, mates, 7, tags, masks)
    small = (tags & 7).astype(np.int8)                                          # without bit 63: fits every width
    fs = tagged_ref.masked(tc.oracle(B, G, D, 1), small, masks & 7)
    for dt in (np.int8, np.uint8, np.int16, np.int32, np.uint32, np.int64, np.uint64):
        _check(gal.rank(probes, mates, 1, small.astype(dt), (masks & 7).astype(dt)), fs, mates, 1)
    _check(gal.rank(probes, mates.tolist(), 1, small.tolist(), (masks & 7).tolist()), fs, mates, 1)
    _check(gal.rank(probes[0], mates[:1], 1, tags, 1), fm[:1], mates[:1], 1)
    # the allocation-free forms: dense int64 CUDA tensors of the right shapes, both or neither
    p = torch.from_numpy(probes).cuda()
    t_dev, m_dev, mt = (torch.from_numpy(np.array(a)).cuda() for a in (tags, masks, mates))
    rank = torch.empty((B,), dtype=torch.int64, device='cuda')
    own = torch.empty((B,), dtype=torch.int64, device='cuda')
    dist = torch.empty((B,), dtype=torch.float32, device='cuda')
    gal.rank_into(p, mt, 1, rank, dist, t_dev, m_dev)
    torch.cuda.synchronize()
    _check(_np((rank, dist)), fm, mates, 1)
    wide = torch.zeros((2 * G,), dtype=torch.int64, device='cuda')
    for bad in (dict(row_tags=None), dict(probe_masks=None), dict(row_tags=t_dev.to(torch.int32)), dict(probe_masks=m_dev.int()),
                dict(row_tags=t_dev.cpu()), dict(probe_masks=m_dev.cpu()), dict(row_tags=tags), dict(probe_masks=1),
                dict(row_tags=t_dev[:-1]), dict(probe_masks=m_dev[:2]), dict(row_tags=wide[::2][:G])):
        kw = dict(row_tags=t_dev, probe_masks=m_dev)
        kw.update(bad)
        with pytest.raises(ValueError):
            gal.rank_into(p, mt, 1, rank, dist, kw['row_tags'], kw['probe_masks'])
        with pytest.raises(ValueError):
            gal.mate_dist_into(p, mt, 1, dist, own, kw['row_tags'], kw['probe_masks'])
        with pytest.raises(ValueError):
            gal.rank_at_into(p, mt, dist, 1, rank, kw['row_tags'], kw['probe_masks'])
    # the C layer: NULL tags or masks with rows enrolled fail; n = 0 is a no-op
    h, st = gal._h, N.stream_ptr()
    for rt, pm in ((None, N.ptr(m_dev)), (N.ptr(t_dev), None)):
        assert N.lib.dif_match_rank_tagged(h, N.ptr(p), B, 1, N.ptr(mt), rt, pm, N.ptr(rank), N.ptr(dist), st) != 0
        assert b'null row tags or probe masks' in N.lib.dif_last_error()
        assert N.lib.dif_match_mate_dist_tagged(h, N.ptr(p), B, 1, N.ptr(mt), rt, pm, N.ptr(dist), N.ptr(own), st) != 0
        assert b'null row tags or probe masks' in N.lib.dif_last_error()
        assert N.lib.dif_match_rank_at_tagged(h, N.ptr(p), B, 1, N.ptr(mt), N.ptr(dist), rt, pm, N.ptr(rank), st) != 0
        assert b'null row tags or probe masks' in N.lib.dif_last_error()
    assert N.lib.dif_match_rank_tagged(h, None, 0, 1, None, None, None, None, None, st) == 0
    assert N.lib.dif_match_mate_dist_tagged(h, None, 0, 1, None, None, None, None, None, st) == 0
    assert N.lib.dif_match_rank_at_tagged(h, None, 0, 1, None, None, None, None, None, st) == 0
    assert N.lib.dif_match_rank_tagged(h, N.ptr(p), B, 7, N.ptr(mt), N.ptr(t_dev), N.ptr(m_dev), N.ptr(rank), N.ptr(dist), st) != 0
    assert N.lib.dif_match_rank_tagged(h, N.ptr(p), -1, 1, N.ptr(mt), N.ptr(t_dev), N.ptr(m_dev), N.ptr(rank), N.ptr(dist), st) != 0
    assert N.lib.dif_match_rank_tagged(h, N.ptr(p), B, 1, None, N.ptr(t_dev), N.ptr(m_dev), N.ptr(rank), N.ptr(dist), st) != 0
    assert N.lib.dif_match_rank_tagged(None, N.ptr(p), B, 1, N.ptr(mt), N.ptr(t_dev), N.ptr(m_dev), N.ptr(rank), N.ptr(dist), st) != 0
    assert N.lib.dif_match_rank_tagged(h, N.ptr(p), B, 1, N.ptr(mt), N.ptr(t_dev), N.ptr(m_dev), N.ptr(rank), None, st) == 0
    torch.cuda.synchronize()
    r0, d0 = gal.rank(np.zeros((0, D), dtype=np.float32), np.zeros(0, dtype=np.int64), 1, tags, np.zeros(0, dtype=np.int64))
    assert r0.shape == (0,) and d0.shape == (0,) and r0.dtype == np.int64 and d0.dtype == np.float32   # an empty batch
    gal.close()
    empty = oneshot.Gallery(emd_size=D)                                         # nothing enrolled: every probe unmated
    none = np.zeros(0, dtype=np.int64)
    for metric in (0, 1):
        r0, d0 = empty.rank(probes, mates, metric, none, masks)
        assert (r0 == -1).all() and np.isnan(d0).all()
    rank.fill_(-5)
    assert N.lib.dif_match_rank_tagged(empty._h, N.ptr(p), B, 1, N.ptr(mt), None, None, N.ptr(rank), N.ptr(dist), st) == 0
    assert N.lib.dif_match_mate_dist_tagged(empty._h, N.ptr(p), B, 1, N.ptr(mt), None, None, N.ptr(dist), N.ptr(own), st) == 0
    torch.cuda.synchronize()
    assert (rank == -1).all() and (own == 0).all()
    assert N.lib.dif_match_rank_at_tagged(empty._h, N.ptr(p), B, 1, N.ptr(mt), N.ptr(dist), None, None, N.ptr(rank), st) == 0
    torch.cuda.synchronize()
    assert (rank == 0).all()
    assert empty.stat('within_tagged_tiles') == 0
    empty.close()


# ------------------------------------------------------------------------------------------- 9
def test_rank_tagged_cuda_in_cuda_out_and_no_host_read(cuda):
    from deep_insight_face import oneshot
    B, G, D = 65, 257, 512
    probes, gal_np, _, tags, masks, mates = tc.case(B, G, D)
    fm = tc.masked(B, G, D, 1)
    gal = oneshot.Gallery(gal_np)
    p, mt, t_dev, m_dev = (torch.from_numpy(np.array(a)).cuda() for a in (probes, mates, tags, masks))
    warm = gal.rank(p, mt, 1, t_dev, m_dev)                                     # (the workspace grows on the first call)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = gal.rank(p, mt, 1, t_dev, m_dev)
        six = gal.rank(p, mt, 1, t_dev, 6)                                      # the broadcast mask is filled on the device
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for a, dt in zip(got, (torch.int64, torch.float32)):
        assert torch.is_tensor(a) and a.is_cuda and a.dtype == dt and tuple(a.shape) == (B,)
    _same(got, warm)
    _check(_np(got), fm, mates, 1, min_clear=0.9)
    _check(_np(six), tagged_ref.masked(tc.oracle(B, G, D, 1), tags, np.full(B, 6, dtype=np.int64)), mates, 1)
    gal.close()


# ------------------------------------------------------------------------------------------- 10
def _identification_ref(fm, mates, thresholds, max_rank):
    """evaluate_identification restated in NumPy on the masked reference distances."""
    rank, md = rank_ref.rank_full(fm, mates)
    mated = rank >= 0
    cmc = np.array([((rank < k) & mated).sum() / mated.sum() for k in range(1, max_rank + 1)])
    um = fm[~mated]
    with np.errstate(all='ignore'):
        nearest = np.where(np.isnan(um).all(1), np.nan, np.nanmin(np.where(np.isnan(um), np.inf, um), axis=1))
    with np.errstate(invalid='ignore'):
        dirs = np.array([(mated & (rank < 1) & (md <= t)).sum() / mated.sum() for t in thresholds])
        far = np.array([(nearest <= t).sum() / len(nearest) for t in thresholds])
    return rank, md, cmc, dirs, far, nearest


@pytest.mark.parametrize('metric', [0, 1])
def test_evaluate_identification_with_tags(cuda, metric):
    """The tagged rank, and for the unmated probes the nearest ELIGIBLE row's distance (topk k = 1, tagged): an unmated probe
    that sees no row raises no alarm."""
    from deep_insight_face import oneshot
    from deep_insight_face.evaluation import identification as ident
    B, G, D = 130, 1000, 128
    probes, gal_np, _, tags, masks, mates = tc.case(B, G, D)
    mates = np.array(mates)
    mates[::5] = -1                                                              # unmated probes of every mask (case_mates': mask 8 alone)
    mates[_near(tc.masked(B, G, D, 1), mates) > 0] = -1                          # ... and the few that are not CLEAR on metric 1
    fm = tc.masked(B, G, D, metric)
    rank, md, cmc, _, _, nearest = _identification_ref(fm, mates, [], 10)
    assert np.isnan(nearest).any() and not np.isnan(nearest).all()               # an unmated probe with mask 8 or 0 sees no row
    fin = np.sort(nearest[~np.isnan(nearest)].astype(np.float64))
    mdf = np.sort(md[~np.isnan(md)].astype(np.float64))
    both = np.unique(np.concatenate([fin, mdf]))
    # thresholds between two adjacent values of the distances that are compared, where the gap is wide: exact on both metrics
    gaps = np.diff(both)
    pick = np.argsort(gaps)[-4:]
    assert gaps[pick].min() > 1e-4
    thresholds = np.sort((both[pick] + both[pick + 1]) / 2)
    _, _, _, dirs, far, _ = _identification_ref(fm, mates, thresholds, 10)
    assert 0 < far.max() < 1 and dirs.max() > 0
    near = _near(fm, mates)
    assert (near == 0).all()
    out = ident.evaluate_identification(gal_np, probes, mates, metric, 10, thresholds, tags, masks)
    assert np.array_equal(out['rank'], rank)
    np.testing.assert_allclose(out['cmc'], cmc, rtol=0, atol=1e-15)
    np.testing.assert_allclose(out['dir'], dirs, rtol=0, atol=1e-15)
    np.testing.assert_allclose(out['far'], far, rtol=0, atol=1e-15)
    plain = ident.evaluate_identification(gal_np, probes, mates, metric, 10, thresholds)
    assert not np.array_equal(plain['rank'], out['rank']) and (plain['far'] >= out['far']).all()
    gal = oneshot.Gallery(gal_np)
    dev = ident.evaluate_identification(gal, torch.from_numpy(probes).cuda(), torch.from_numpy(np.array(mates)).cuda(), metric, 10,
                                        thresholds, torch.from_numpy(np.array(tags)).cuda(), torch.from_numpy(np.array(masks)).cuda())
    assert all(torch.is_tensor(dev[k]) and dev[k].is_cuda for k in ('rank', 'mate_dist', 'cmc', 'dir', 'far'))
    assert np.array_equal(dev['rank'].cpu().numpy(), rank)
    np.testing.assert_allclose(dev['far'].cpu().numpy(), far, rtol=0, atol=1e-15)
    np.testing.assert_allclose(dev['dir'].cpu().numpy(), dirs, rtol=0, atol=1e-15)
    one = ident.evaluate_identification(gal, probes, mates, metric, 10, thresholds, tags, 1)    # an int mask for every probe
    assert np.array_equal(one['rank'], tq.rank_full(tc.oracle(B, G, D, metric), mates, tags, np.ones(B, dtype=np.int64))[0])
    with pytest.raises(ValueError, match='go together'):
        ident.evaluate_identification(gal, probes, mates, metric, 10, thresholds, row_tags=tags)
    gal.close()
