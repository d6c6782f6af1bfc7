"""Watch-lists: oneshot.Gallery.topk / topk_ids with `row_tags` and `probe_masks` (dif_match_topk_tagged /
dif_match_topk_ids_tagged) against the CPU statement tests/tagged_ref.py -- the untagged oracle with the distances of the
ineligible (row, probe) pairs set to NaN -- under tests/test_topk_gpu.py's rules (_check, NEAR = 2e-6, ATOL = 1e-5), and against
the device's own untagged answers, bit for bit.

Inputs: test_topk_gpu.py's _inputs on its six shapes; tags tagged_ref.case_tags(G) (bit 0 on half the rows, bit 1 on an eighth,
bit 2 on 1/128, bit 63 on half, bit 3 never, some rows tag 0); masks cycling through [1, 2, 4, 8, 1 << 63, 0, -1, 6].  The cap --
CLEAR positions at least 0.9 of the listed ones -- is asserted on the oracle before the device is asked; the smallest share of
these cases is 0.9658 at (64, 4097, 512), k = 128, metric 1 (tests/test_tagged_ref.py holds the caps without a GPU)."""
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
import rank_ref
import remove_ref
import tagged_ref
import test_topk_gpu as tg
import test_topk_ids_gpu as ti
import topk_ref

pytestmark = pytest.mark.gpu
SHAPES = tg.SHAPES
TOP = -(1 << 63)


@functools.lru_cache(maxsize=None)
def _masked(B, G, D, metric):
    fm = tagged_ref.masked(tg._oracle(B, G, D, metric), tagged_ref.case_tags(G), tagged_ref.case_masks(B))
    fm.setflags(write=False)
    return fm


def _labels(G):
    return (np.arange(G) % max(1, G // 4)).astype(np.int64)                      # _inputs' identities


def _same(got, want):
    """Bit for bit: integers equal, float32 equal as bit patterns with every NaN taken as one value."""
    got, want = tg._np(got) if torch.is_tensor(got[0]) else got, tg._np(want) if torch.is_tensor(want[0]) else want
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (i, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            assert tg._bits_equal(g, w), (i, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:8])
        else:
            assert np.array_equal(g, w), (i, np.argwhere(g != w)[:8], g[g != w][:8], w[g != w][:8])


# ------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('k', [1, 5, 128])
@pytest.mark.parametrize('B,G,D', SHAPES)
def test_tagged_against_the_oracle(cuda, B, G, D, k, metric):
    """Tile tails both ways, all three probe-tile shapes, more than 512 tiles; eligibility from one row in 128 to every tagged
    row, no row at all (masks 8 and 0) and bit 63."""
    from deep_insight_face import oneshot
    probes, gal_np, _ = tg._inputs(B, G, D)
    tags, masks = tagged_ref.case_tags(G), tagged_ref.case_masks(B)
    fm = _masked(B, G, D, metric)
    tg._cap(fm, k, metric)
    gal = oneshot.Gallery(gal_np)
    got = gal.topk(probes, k, metric, row_tags=tags, probe_masks=masks)
    assert all(isinstance(a, np.ndarray) for a in got)                          # NumPy in -> NumPy out
    tg._check(got, fm, k, metric)
    el = tagged_ref.eligible(tags, masks)
    for b in range(B):
        rows = got[0][b][got[0][b] >= 0]
        assert el[b, rows].all(), b                                             # no ineligible row is ever listed
        assert rows.shape[0] == min(k, int(el[b].sum()))
    # the identities with all-distinct labels are the rows; the module-level form; unsigned tags taken bit for bit
    ids = gal.topk_ids(probes, k, np.arange(G), metric, row_tags=tags, probe_masks=masks)
    _same(ids[:2], got)
    if k == 5:
        for g in (gal, gal_np):
            _same(oneshot.topk(probes, g, k, metric, row_tags=tags.view(np.uint64), probe_masks=masks.view(np.uint64)), got)
            _same(oneshot.topk_ids(probes, g, k, np.arange(G), metric, None, tags, masks)[:2], got)
    gal.close()


# ------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('B,G,D', [(130, 1000, 128), (64, 4097, 512)])
def test_tagged_exact_device_against_device(cuda, B, G, D, metric):
    """On the library's own distances the tagged list is exact on both metrics: per mask value it equals the untagged list of a
    gallery holding the eligible rows alone, and the tagged identities equal the untagged ones with the ineligible rows'
    labels set to -1; with every pair eligible the tagged calls equal the untagged ones."""
    from deep_insight_face import oneshot
    probes, gal_np, pick = tg._inputs(B, G, D)
    tags, masks = tagged_ref.case_tags(G), tagged_ref.case_masks(B)
    labels = _labels(G)
    gal = oneshot.Gallery(gal_np)
    p = torch.from_numpy(probes).cuda()
    t_dev, m_dev, l_dev = (torch.from_numpy(np.array(a)).cuda() for a in (tags, masks, labels))
    ex = torch.from_numpy(np.array(pick, dtype=np.int64)).cuda()                # the probe's own identity
    for k in (5, 128):
        got = tg._np(gal.topk(p, k, metric, t_dev, m_dev))
        got_ids = tg._np(gal.topk_ids(p, k, l_dev, metric, ex, t_dev, m_dev))
        for m in tagged_ref.MASK_CYCLE:
            sel = np.flatnonzero(masks == m)
            el = (tags & m) != 0
            rows = np.flatnonzero(el)
            if rows.shape[0] == 0:
                assert (got[0][sel] == -1).all() and np.isnan(got[1][sel]).all()
                assert (got_ids[0][sel] == -1).all() and np.isnan(got_ids[1][sel]).all() and (got_ids[2][sel] == -1).all()
                continue
            sub = oneshot.Gallery(gal_np[rows])
            si, sd = sub.topk(probes[sel], k, metric)
            sub.close()
            _same((got[0][sel], got[1][sel]), (np.where(si >= 0, rows[np.maximum(si, 0)], -1), sd))
            want = gal.topk_ids(probes[sel], k, np.where(el, labels, -1), metric, pick[sel])
            _same(tuple(a[sel] for a in got_ids), want)
        # every pair eligible: the untagged calls, bit for bit (a Python int stands for every probe)
        ones = torch.full((G,), -1, dtype=torch.int64, device='cuda')
        _same(gal.topk(p, k, metric, ones, -1), gal.topk(p, k, metric))
        _same(gal.topk_ids(p, k, l_dev, metric, ex, ones, -1), gal.topk_ids(p, k, l_dev, metric, ex))
        _same(gal.topk(p, k, metric, torch.full((G,), TOP, dtype=torch.int64, device='cuda'), (1 << 64) - 1),
              gal.topk(p, k, metric))
    gal.close()


# ------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('k', [5, 128])
def test_tagged_both_phases(cuda, k, metric):
    """Option "topk_seed": 1 and 2 leave the list to the sweep, 1000 evaluates every tile that holds an eligible row in the
    seed: bit-identical to the default, which is checked against the oracle."""
    from deep_insight_face import oneshot
    B, G, D = 64, 4097, 512
    probes, gal_np, pick = tg._inputs(B, G, D)
    fm = _masked(B, G, D, metric)
    tg._cap(fm, k, metric)
    gal = oneshot.Gallery(gal_np)
    p = torch.from_numpy(probes).cuda()
    t_dev = torch.from_numpy(np.array(tagged_ref.case_tags(G))).cuda()
    m_dev = torch.from_numpy(np.array(tagged_ref.case_masks(B))).cuda()
    l_dev = torch.from_numpy(_labels(G)).cuda()
    base = tg._np(gal.topk(p, k, metric, t_dev, m_dev))
    tg._check(base, fm, k, metric)
    base_ids = tg._np(gal.topk_ids(p, k, l_dev, metric, None, t_dev, m_dev))
    tiles = {}
    for seed in (1, 2, 1000, 0):
        gal.set_option('topk_seed', seed)
        _same(gal.topk(p, k, metric, t_dev, m_dev), base)
        tiles[seed] = gal.stat('topk_tagged_tiles')
        _same(gal.topk_ids(p, k, l_dev, metric, None, t_dev, m_dev), base_ids)
    # every tile holds a row with bit 0, bit 1 or bit 63; 8 of the 64 probes see bit 2 alone, 16 nothing
    gtiles = (G + 127) // 128
    # (the last tile holds one row)
    assert (gtiles - 1) * (B - 24) <= tiles[1000] <= gtiles * (B - 16) and 0 < tiles[1] <= tiles[1000]
    gal.close()


# ------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('metric', [0, 1])
def test_tagged_exact_ties_across_an_eligibility_boundary(cuda, metric):
    """Identical enrolled rows of which only the higher-indexed ones are eligible (test_topk_exact_ties' table): the list
    starts with the eligible copies in index order; where every copy is eligible, with all of them."""
    from deep_insight_face import oneshot
    probes, gal_np = gi.match_tie_inputs()
    G = gal_np.shape[0]
    tags = np.full(G, 3, dtype=np.int64)
    tags[100:140] = 2                                                            # the originals: mask 1 does not see them
    tags[300:340] = 1
    tags[500:520] = 5
    masks = np.array([1, 1, 4, 1, 2, 1, 3, 1], dtype=np.int64)
    heads = {0: (300, 500), 1: (305, 505), 2: (519,), 3: (320,), 4: (139,), 5: (301, 501), 6: (110, 310, 510)}
    fm = tagged_ref.masked(rank_ref.distances(probes, gal_np, metric), tags, masks)
    want_i, want_d = topk_ref.topk_full(fm, 4)
    for b, rows in heads.items():
        assert tuple(want_i[b, :len(rows)]) == rows
    gal = oneshot.Gallery(gal_np)
    for seed in (0, 1):
        gal.set_option('topk_seed', seed)
        idx, dist = gal.topk(probes, 4, metric, tags, masks)
        for b, rows in heads.items():
            n = len(rows)
            assert tuple(idx[b, :n]) == rows, (seed, b, idx[b])
            assert (dist[b, :n] == dist[b, 0]).all()
        if metric == 0:
            _same((idx, dist), (want_i, want_d))
        assert ((idx[2] >= 500) & (idx[2] < 520)).all()                          # mask 4 sees rows 500 .. 519 and no other
    gal.close()


@pytest.mark.parametrize('seed', [0, 1])
def test_tagged_near_ties(cuda, seed):
    """Rows one ulp, 1e-7 and 1e-4 apart and exact duplicates at shuffled positions, every second one eligible: metric 0,
    bit-identical to the stable argsort over the eligible rows."""
    from deep_insight_face import oneshot
    probes, gal_np = gi.match_near_tie_inputs()
    G, B = gal_np.shape[0], probes.shape[0]
    tags = np.random.default_rng(3).integers(0, 4, G).astype(np.int64)          # tag 0: a quarter of the rows
    masks = np.array([1, 2, 3], dtype=np.int64)[np.arange(B) % 3]
    fm = tagged_ref.masked(rank_ref.distances(probes, gal_np, 0), tags, masks)
    gal = oneshot.Gallery(gal_np)
    gal.set_option('topk_seed', seed)
    _same(gal.topk(probes, 5, 0, tags, masks), topk_ref.topk_full(fm, 5))
    _same(gal.topk(probes, 128, 0, tags, masks), topk_ref.topk_full(fm, 128))
    gal.close()


# ------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize('name', [c[0] for c in gi.match_degenerate_cases()])
def test_tagged_degenerate(cuda, name):
    """Zero, tiny, huge and non-finite rows and probes, anti-parallel rows.  The odd rows -- those with a distance that is not
    finite to some ordinary probe -- are eligible for the even probes and ineligible for the odd ones: an eligible row whose
    search key is NaN must still bring its tile in, an ineligible one must stay out of the list."""
    from deep_insight_face import oneshot
    probes, gal_np = [(p, g) for n, p, g in gi.match_degenerate_cases() if n == name][0]
    G, B = gal_np.shape[0], probes.shape[0]
    fulls = {metric: rank_ref.distances(probes, gal_np, metric) for metric in (0, 1)}
    odd = np.zeros(G, dtype=bool)
    for full in fulls.values():
        ordinary = np.isfinite(full).any(1)
        odd |= (~np.isfinite(full[ordinary])).any(0)
    tags = np.where(odd, 2, 1).astype(np.int64)
    masks = np.where(np.arange(B) % 2 == 0, 3, 1).astype(np.int64)
    gal = oneshot.Gallery(gal_np)
    for metric in (0, 1):
        fm = tagged_ref.masked(fulls[metric], tags, masks)
        nan = np.isnan(fm)
        for k in (1, 3, 128):
            tg._cap(fm, k, metric)
            idx, dist = gal.topk(probes, k, metric, tags, masks)
            tg._check((idx, dist), fm, k, metric)
            real = idx >= 0
            assert np.array_equal(real.sum(1), np.minimum(k, (~nan).sum(1)))
            for b in range(B):
                assert not nan[b, idx[b][real[b]]].any()                        # NaN and ineligible rows are never listed
    gal.close()


# ------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize('metric', [0, 1])
def test_tagged_skip_rule(cuda, metric):
    """A tile with no eligible row is never evaluated row by row.  516 tiles; bit 2 on 100 rows of exactly two tiles; probes
    with mask 4 and k = 128: the list stays short, the tolerance +inf, and the untagged rule would evaluate every tile --
    here the two that hold an eligible row.  A probe with mask 8 evaluates none."""
    from deep_insight_face import oneshot
    B, G, D = 3, 66000, 32
    probes3, gal_np, _ = tg._inputs(B, G, D)
    n = 9
    probes = np.concatenate([probes3, probes3[::-1] * np.float32(1.5), -probes3])
    tags = np.ones(G, dtype=np.int64)
    tags[128 * 7:128 * 7 + 40] = 5
    tags[128 * 300 + 5:128 * 300 + 65] = 4
    assert (G + 127) // 128 == 516 and int(((tags & 4) != 0).sum()) == 100
    assert np.unique(np.flatnonzero(tags & 4) // 128).tolist() == [7, 300]
    masks = np.full(n, 4, dtype=np.int64)
    fm = tagged_ref.masked(rank_ref.distances(probes, gal_np, metric), tags, masks)
    tg._cap(fm, 128, metric)
    gal = oneshot.Gallery(gal_np)
    assert gal.stat('topk_tagged_tiles') == 0                                    # before the first tagged call
    got = gal.topk(probes, 128, metric, tags, masks)
    tiles = gal.stat('topk_tagged_tiles')
    tg._check(got, fm, 128, metric)
    assert ((got[0] >= 0).sum(1) == 100).all()
    assert 0 < tiles <= 2 * n, tiles
    ids = gal.topk_ids(probes, 128, np.arange(G), metric, None, tags, masks)
    tiles_ids = gal.stat('topk_tagged_tiles')
    _same(ids[:2], got)
    assert 0 < tiles_ids <= 2 * n and gal.stat('topk_ids_tiles') == tiles_ids
    for seed in (1, 1000):                                                       # whatever the seed asks for
        gal.set_option('topk_seed', seed)
        _same(gal.topk(probes, 128, metric, tags, masks), got)
        assert 0 < gal.stat('topk_tagged_tiles') <= 2 * n
    gal.set_option('topk_seed', 0)
    i8, d8 = gal.topk(probes[:1], 128, metric, tags, 8)                          # nothing carries bit 3
    assert gal.stat('topk_tagged_tiles') == 0 and (i8 == -1).all() and np.isnan(d8).all()
    i8, d8, l8 = gal.topk_ids(probes[:1], 128, np.arange(G), metric, None, tags, 8)
    assert gal.stat('topk_tagged_tiles') == 0 and (i8 == -1).all() and np.isnan(d8).all() and (l8 == -1).all()
    gal.topk(probes, 5, metric)                                                  # an untagged call leaves the stat alone
    assert gal.stat('topk_tagged_tiles') == 0
    gal.close()


# ------------------------------------------------------------------------------------------- 7
def test_tagged_handle_reuse(cuda):
    """A non-monotone batch and k sequence on one handle, interleaved with untagged calls, update and remove -- the tags
    permuted by the moves `remove` reports -- against the recomputed oracle; a shard with an index_base."""
    from deep_insight_face import oneshot
    G, D = 4097, 128
    probes, gal_np, _ = tg._inputs(70, G, D)
    gal_np = gal_np.copy()
    tags = np.array(tagged_ref.case_tags(G))
    masks = tagged_ref.case_masks(70)
    gal = oneshot.Gallery(gal_np)

    def check(n, k, metric=0):
        fm = tagged_ref.masked(rank_ref.distances(probes[:n], gal_np, metric), tags, masks[:n])
        tg._cap(fm, k, metric)
        got = gal.topk(probes[:n], k, metric, tags, masks[:n])
        tg._check(got, fm, k, metric)
        return got

    plain = gal.topk(probes, 5, 0)
    first = check(70, 5)
    gal.topk_ids(probes[:33], 7, _labels(G), 0)
    check(33, 128)
    _same(gal.topk(probes, 5, 0), plain)                                        # the untagged call between tagged ones
    _same(check(70, 5), first)
    row = gal_np[first[0][0, 0]][None]                                          # probe 0's nearest eligible row, five more times:
    gal.update(np.repeat(row, 5, axis=0))                                       # three of the copies eligible for it
    gal_np = np.concatenate([gal_np, np.repeat(row, 5, axis=0)])
    tags = np.concatenate([tags, np.array([1, 0, 3, 2, TOP | 1], dtype=np.int64)])
    got = check(70, 5)
    assert masks[0] == 1 and list(got[0][0, :4]) == [first[0][0, 0], G, G + 2, G + 4]
    check(33, 128, 1)
    gone = np.array([int(first[0][0, 0]), 7, 4000, G + 2], dtype=np.int64)
    moved_from, moved_to = gal.remove(gone)
    gal_np = remove_ref.remove_ref(gal_np, gone)[0]
    new_tags = tags[:gal_np.shape[0]].copy()
    new_tags[moved_to] = tags[moved_from]                                       # the caller's table follows the moves
    assert np.array_equal(new_tags, remove_ref.remove_ref(tags, gone)[0])
    tags = new_tags
    assert len(gal) == gal_np.shape[0] == G + 1
    check(70, 5)
    check(70, 128, 1)
    check(33, 5, 1)
    gal.close()
    shifted = oneshot.Gallery(gal_np, index_base=1000)
    fm = tagged_ref.masked(rank_ref.distances(probes, gal_np, 0), tags, masks)
    idx, dist = shifted.topk(probes, 5, 0, tags, masks)
    tg._check((idx, dist), fm, 5, 0, base=1000)
    assert ((idx == -1) | ((idx >= 1000) & (idx < 1000 + gal_np.shape[0]))).all()
    ids = shifted.topk_ids(probes, 5, np.arange(gal_np.shape[0]), 0, None, tags, masks)
    _same(ids[:2], (idx, dist))
    shifted.close()


# ------------------------------------------------------------------------------------------- 8
def test_tagged_arguments(cuda):
    from deep_insight_face import _native as N
    from deep_insight_face import oneshot
    B, G, D = 3, 129, 64
    probes, gal_np, _ = tg._inputs(B, G, D)
    tags, masks = tagged_ref.case_tags(G), tagged_ref.case_masks(B)
    labels = _labels(G)
    fm = _masked(B, G, D, 1)
    gal = oneshot.Gallery(gal_np)
    for kw in (dict(row_tags=tags), dict(probe_masks=masks), dict(probe_masks=1)):        # exactly one given
        with pytest.raises(ValueError, match='go together'):
            gal.topk(probes, 3, 1, **kw)
        with pytest.raises(ValueError, match='go together'):
            gal.topk_ids(probes, 3, labels, 1, **kw)
        with pytest.raises(ValueError, match='go together'):
            oneshot.topk(probes, gal, 3, 1, **kw)
        with pytest.raises(ValueError, match='go together'):
            oneshot.topk_ids(probes, gal, 3, labels, 1, **kw)
    for bad_t, bad_m in ((tags.astype(np.float32), masks), (tags, masks.astype(np.float64)), (tags != 0, masks),
                         (tags, masks != 0), (tags[:-1], masks), (tags, masks[:2]), (tags[None], masks), (tags, masks[:, None]),
                         (torch.from_numpy(np.array(tags)).float(), masks), (tags, torch.from_numpy(np.array(masks)) != 0),
                         (tags, 1.0), (tags, True), (tags, 1 << 64), (tags, -(1 << 63) - 1), (3, masks)):
        with pytest.raises(ValueError):
            gal.topk(probes, 3, 1, bad_t, bad_m)
        with pytest.raises(ValueError):
            gal.topk_ids(probes, 3, labels, 1, None, bad_t, bad_m)
    for k in (0, 129, -1):
        with pytest.raises(ValueError):
            gal.topk(probes, k, 1, tags, masks)
        with pytest.raises(ValueError):
            gal.topk_ids(probes, k, labels, 1, None, tags, masks)
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        gal.topk(probes, 3, 7, tags, masks)
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        gal.topk_ids(probes, 3, labels, 7, None, tags, masks)
    # every integer width, lists, one probe as a vector with an int mask
    want = tg._np(gal.topk(torch.from_numpy(probes).cuda(), 3, 1, torch.from_numpy(np.array(tags)).cuda(),
                           torch.from_numpy(np.array(masks)).cuda()))
    tg._check(want, fm, 3, 1)
    small = (tags & 7).astype(np.int8)                                          # without bit 63: fits every width
    fs = tagged_ref.masked(tg._oracle(B, G, D, 1), small, masks[:3] & 7)
    for dt in (np.int8, np.uint8, np.int16, np.int32, np.uint32, np.int64, np.uint64):
        tg._check(gal.topk(probes, 3, 1, small.astype(dt), (masks & 7).astype(dt)), fs, 3, 1)
    tg._check(gal.topk(probes, 3, 1, small.tolist(), (masks & 7).tolist()), fs, 3, 1)
    one = gal.topk(probes[0], 3, 1, tags, 1)
    tg._check(one, fm[:1], 3, 1)
    # the allocation-free forms: dense int64 CUDA tensors of the right shapes, both or neither
    p = torch.from_numpy(probes).cuda()
    t_dev, m_dev, l_dev = (torch.from_numpy(np.array(a)).cuda() for a in (tags, masks, labels))
    k = 4
    idx = torch.empty((B, k), dtype=torch.int64, device='cuda')
    dist = torch.empty((B, k), dtype=torch.float32, device='cuda')
    lab = torch.empty((B, k), dtype=torch.int64, device='cuda')
    gal.topk_into(p, k, 1, idx, dist, t_dev, m_dev)
    torch.cuda.synchronize()
    tg._check(tg._np((idx, dist)), fm, k, 1)
    gal.topk_ids_into(p, k, 1, torch.arange(G, device='cuda'), None, idx, dist, lab, t_dev, m_dev)
    torch.cuda.synchronize()
    tg._check(tg._np((idx, dist)), fm, k, 1)
    wide = torch.zeros((2 * G,), dtype=torch.int64, device='cuda')
    for bad in (dict(row_tags=None), dict(probe_masks=None), dict(row_tags=t_dev.to(torch.int32)), dict(probe_masks=m_dev.int()),
                dict(row_tags=t_dev.cpu()), dict(probe_masks=m_dev.cpu()), dict(row_tags=tags), dict(probe_masks=1),
                dict(row_tags=t_dev[:-1]), dict(probe_masks=m_dev[:2]), dict(row_tags=wide[::2][:G])):
        kw = dict(row_tags=t_dev, probe_masks=m_dev)
        kw.update(bad)
        with pytest.raises(ValueError):
            gal.topk_into(p, k, 1, idx, dist, kw['row_tags'], kw['probe_masks'])
        with pytest.raises(ValueError):
            gal.topk_ids_into(p, k, 1, l_dev, None, idx, dist, lab, kw['row_tags'], kw['probe_masks'])
    # the C layer: NULL tags or masks with rows enrolled fail; n = 0 is a no-op
    h = gal._h
    for rt, pm in ((None, N.ptr(m_dev)), (N.ptr(t_dev), None)):
        assert N.lib.dif_match_topk_tagged(h, N.ptr(p), B, 1, k, rt, pm, N.ptr(idx), N.ptr(dist), N.stream_ptr()) != 0
        assert b'null row tags or probe masks' in N.lib.dif_last_error()
        assert N.lib.dif_match_topk_ids_tagged(h, N.ptr(p), B, 1, k, N.ptr(l_dev), None, rt, pm, N.ptr(idx), N.ptr(dist), None,
                                               N.stream_ptr()) != 0
        assert b'null row tags or probe masks' in N.lib.dif_last_error()
    assert N.lib.dif_match_topk_tagged(h, None, 0, 1, k, None, None, None, None, N.stream_ptr()) == 0
    assert N.lib.dif_match_topk_ids_tagged(h, None, 0, 1, k, None, None, None, None, None, None, None, N.stream_ptr()) == 0
    assert N.lib.dif_match_topk_tagged(h, N.ptr(p), B, 1, 129, N.ptr(t_dev), N.ptr(m_dev), N.ptr(idx), N.ptr(dist),
                                       N.stream_ptr()) != 0
    assert N.lib.dif_match_topk_tagged(h, N.ptr(p), -1, 1, k, N.ptr(t_dev), N.ptr(m_dev), N.ptr(idx), N.ptr(dist),
                                       N.stream_ptr()) != 0
    assert N.lib.dif_match_topk_ids_tagged(h, N.ptr(p), B, 1, k, None, None, N.ptr(t_dev), N.ptr(m_dev), N.ptr(idx), N.ptr(dist),
                                           None, N.stream_ptr()) != 0       # null row labels
    with pytest.raises(ValueError):
        gal.stat('topk_tagged')
    i0, d0 = gal.topk(np.zeros((0, D), dtype=np.float32), 3, 1, tags, np.zeros(0, dtype=np.int64))   # an empty batch
    assert i0.shape == (0, 3) and d0.shape == (0, 3) and i0.dtype == np.int64 and d0.dtype == np.float32
    gal.close()
    empty = oneshot.Gallery(emd_size=D)                                         # nothing enrolled: all padding
    none = np.zeros(0, dtype=np.int64)
    for metric in (0, 1):
        for k in (1, 128):
            i0, d0 = empty.topk(probes, k, metric, none, masks)
            assert i0.shape == (B, k) and i0.dtype == np.int64 and (i0 == -1).all() and np.isnan(d0).all()
            i0, d0, l0 = empty.topk_ids(probes, k, none, metric, None, none, -1)
            assert (i0 == -1).all() and np.isnan(d0).all() and (l0 == -1).all()
    assert empty.stat('topk_tagged_tiles') == 0
    empty.close()


# ------------------------------------------------------------------------------------------- 9
def test_tagged_cuda_in_cuda_out_and_no_host_read(cuda):
    """CUDA tensors in give CUDA tensors out, and in steady state the call reads nothing back: under
    set_sync_debug_mode('error') any synchronising call of torch inside it raises."""
    from deep_insight_face import oneshot
    B, G, D, k = 65, 257, 512, 5
    probes, gal_np, _ = tg._inputs(B, G, D)
    gal = oneshot.Gallery(gal_np)
    p = torch.from_numpy(probes).cuda()
    t_dev = torch.from_numpy(np.array(tagged_ref.case_tags(G))).cuda()
    m_dev = torch.from_numpy(np.array(tagged_ref.case_masks(B))).cuda()
    l_dev = torch.from_numpy(_labels(G)).cuda()
    warm = gal.topk(p, k, 1, t_dev, m_dev)                                      # (the workspace grows on the first call)
    warm_ids = gal.topk_ids(p, k, l_dev, 1, None, t_dev, m_dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        ti, td = gal.topk(p, k, 1, t_dev, m_dev)
        bi, bd = gal.topk(p, k, 1, t_dev, 6)                                    # the broadcast mask is filled on the device
        ii, idd, il = gal.topk_ids(p, k, l_dev, 1, None, t_dev, m_dev)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for t, dt in ((ti, torch.int64), (td, torch.float32), (ii, torch.int64), (idd, torch.float32), (il, torch.int64)):
        assert torch.is_tensor(t) and t.is_cuda and t.dtype == dt and tuple(t.shape) == (B, k)
    _same((ti, td), warm)
    _same((ii, idd, il), warm_ids)
    tg._check(tg._np((ti, td)), _masked(B, G, D, 1), k, 1)
    six = tagged_ref.masked(tg._oracle(B, G, D, 1), tagged_ref.case_tags(G), np.full(B, 6, dtype=np.int64))
    tg._check(tg._np((bi, bd)), six, k, 1)
    gal.close()


# ------------------------------------------------------------------------------------------- 10
def _round_masks(B):
    """tagged_ref.case_masks with every block of 128 probes one step further along the cycle.  The cycle's period, 8, divides
    128, so under case_masks(B) itself -- and under any rotation of the whole array -- probe 128 + j carries probe j's mask
    and a launch that dropped its `probe_masks + b0` would answer correctly."""
    i = np.arange(B)
    m = tagged_ref.case_masks(B + B // 128 + 1)[i + i // 128].copy()
    m.setflags(write=False)
    return m


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('k', [5, 128])
@pytest.mark.parametrize('B,G,D', tg.ROUND_SHAPES)
def test_tagged_rounds(cuda, B, G, D, k, metric):
    """Rounds of probes (test_topk_gpu.py's section 9), both tagged entries: "topk_round" 0, 128 (and 256 at B = 300), 0 on one
    handle; every answer passes the oracle check, and the forced-round answers and the one after the option is taken back equal
    the first one-round answer bit for bit; the identities with every probe's own identity excluded.  Rounds two and three
    hold probes whose mask admits no row: all padding.  "topk_tagged_tiles" and "topk_ids_tiles" count (probe, tile)
    evaluations, which do not depend on the split: a forced-round call reports the one-round call's number (a counter zeroed
    in every round reports the last round's alone).  Before the device is asked: the oracle under the masks a dropped `+ b0`
    would read differs from the true one in every round after the first."""
    from deep_insight_face import oneshot
    probes, gal_np, pick = tg._inputs(B, G, D)
    full = tg._oracle(B, G, D, metric)
    tags, masks, labels, ex = tagged_ref.case_tags(G), _round_masks(B), _labels(G), pick.astype(np.int64)
    fm = tagged_ref.masked(full, tags, masks)
    want = topk_ref.topk_full(fm, k)
    for per in tg._round_options(B)[1:-1]:
        wrong = topk_ref.topk_full(tagged_ref.masked(full, tags, tg._without_offset(masks, per)), k)
        for sl in tg._later_rounds(B, per):
            assert (wrong[0][sl] != want[0][sl]).any(), (per, sl)
    blind = ~tagged_ref.eligible(tags, masks).any(1)                            # probes whose mask admits no row
    assert blind[:128].any() and all(blind[sl].any() for sl in tg._later_rounds(B, 128) if sl.stop - sl.start >= 8)
    tg._cap(fm, k, metric)
    ti._cap(fm, labels, k, metric, ex)
    gal = oneshot.Gallery(gal_np)
    p = torch.from_numpy(probes).cuda()
    t_dev, m_dev, l_dev, e_dev = (torch.from_numpy(np.array(a)).cuda() for a in (tags, masks, labels, ex))
    first, first_ids, tiles = None, None, {'rows': [], 'ids': [], 'ids, topk_ids_tiles': []}
    for per in tg._round_options(B):
        gal.set_option('topk_round', per)
        got = tg._np(gal.topk(p, k, metric, t_dev, m_dev))
        tiles['rows'].append(gal.stat('topk_tagged_tiles'))
        tg._check(got, fm, k, metric)
        assert (got[0][blind] == -1).all() and np.isnan(got[1][blind]).all()
        first = first or got
        _same(got, first)
        ids = tg._np(gal.topk_ids(p, k, l_dev, metric, e_dev, t_dev, m_dev))
        tiles['ids'].append(gal.stat('topk_tagged_tiles'))
        tiles['ids, topk_ids_tiles'].append(gal.stat('topk_ids_tiles'))
        ti._check(ids, fm, labels, k, metric, ex)
        assert (ids[0][blind] == -1).all() and np.isnan(ids[1][blind]).all() and (ids[2][blind] == -1).all()
        first_ids = first_ids or ids
        _same(ids, first_ids)
    print('topk_tagged_tiles', (B, G, D), k, metric, tiles)
    gtiles = (G + 127) // 128
    for name, counts in tiles.items():
        assert 0 < counts[0] <= int((~blind).sum()) * gtiles and counts == [counts[0]] * len(counts), (name, counts)
    with pytest.raises(ValueError, match='topk_round'):
        gal.set_option('topk_round', 100)                                       # not a multiple of 128
    gal.close()
