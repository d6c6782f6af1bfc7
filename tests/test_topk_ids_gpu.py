"""The k nearest distinct identities (oneshot.Gallery.topk_ids / dif_match_topk_ids) against the CPU oracle
(tests/topk_ids_ref.py): per probe q, with row_labels [G] and an optional excluded label

    d = oracle.distance.distance(q[None, :], gallery, metric);  ok = ~isnan(d) & (row_labels >= 0) & (row_labels != exclude)
    order = np.argsort(d, kind='stable');  order = order[ok[order]];  keep = each label's first row in order, the first k
    idx = keep + index_base;  dist = d[keep];  label = row_labels[keep];  unused slots: -1 / NaN / -1

Metric 0: idx, dist and label bit-identical.  Metric 1: the device evaluates arccos in double and rounds once, NumPy's float32
arccos is within 2 ulp of that, so two identities whose best distances lie within NEAR = 2e-6 of each other may swap, and an
identity may be reported with another of its rows that close to its best (test_topk_gpu.py's NEAR).  A list position j is
CLEAR when the oracle's per-identity best distances at j-1, j, j+1 differ by more than NEAR: there the label equals the
oracle's; at every position the reported row carries the reported label, the labels of a list are distinct, the oracle
distance of the reported row is within NEAR of the oracle's j-th best, and dist is within 1e-5 of the oracle's for that row
(test_match_gpu.py's rule, its _cos_ok exclusion included).  CLEAR positions are at least 0.9 of the listed positions of
every case, asserted on the oracle before the device is asked (tests/test_topk_ids_ref.py holds the same caps without a GPU).
On the library's own distances (Gallery.within with an all-embracing tolerance) the list is exact on both metrics."""

import numpy as np
import pytest
import torch

import golden_inputs as gi
import rank_ref
import remove_ref
import topk_ids_ref as ir
from oracle import distance as od
from test_topk_gpu import ATOL, MIN_CLEAR, NEAR, ROUND_SHAPES, SHAPES, _bits_equal, _cos_ok, _inputs, _later_rounds, _np, \
    _oracle, _round_options, _without_offset

pytestmark = pytest.mark.gpu


def _labellings(G):
    nid = max(1, G // 4)
    return {'spread': np.arange(G) % nid, 'contiguous': np.arange(G) // 4, 'distinct': np.arange(G),
            'one': np.zeros(G, dtype=np.int64)}


def _cap(full, labels, k, metric, exclude=None):
    """The cap on the oracle alone -- call it before the device is asked."""
    if metric == 1:
        share = ir.clear_share(full, labels, k, NEAR, exclude)
        assert share >= MIN_CLEAR, share


def _check(got, full, labels, k, metric, exclude=None, base=0):
    idx, dist, lab = got
    labels = np.asarray(labels, dtype=np.int64)
    want_i, want_d, want_l = ir.topk_ids_full(full, labels, k, exclude, base)
    assert idx.dtype == np.int64 and dist.dtype == np.float32 and lab.dtype == np.int64
    assert idx.shape == want_i.shape and dist.shape == want_d.shape and lab.shape == want_l.shape
    pad = want_i < 0
    assert np.array_equal(idx < 0, pad) and (idx[pad] == -1).all() and np.isnan(dist[pad]).all() and (lab[pad] == -1).all()
    assert not np.isnan(dist[~pad]).any()
    assert ((idx[~pad] >= base) & (idx[~pad] < base + full.shape[1])).all()
    assert np.array_equal(labels[idx[~pad] - base], lab[~pad])                   # the reported row carries the reported label
    assert (lab[~pad] >= 0).all()
    if exclude is not None:
        assert not (lab == np.asarray(exclude, dtype=np.int64)[:, None])[~pad].any()
    if metric == 0:
        bad = np.argwhere(idx != want_i)
        assert bad.shape[0] == 0, (bad[:8], idx[idx != want_i][:8], want_i[idx != want_i][:8])
        assert _bits_equal(dist, want_d) and np.array_equal(lab, want_l)
        return
    clear = ir.clear_positions(full, labels, k, NEAR, exclude)
    assert clear.sum() >= MIN_CLEAR * (~pad).sum()
    bad = np.argwhere(clear & (lab != want_l))
    assert bad.shape[0] == 0, (bad[:8], lab[clear & (lab != want_l)][:8], want_l[clear & (lab != want_l)][:8])
    for b in range(full.shape[0]):
        n = int((~pad[b]).sum())
        assert np.unique(lab[b, :n]).shape[0] == n                               # the labels of a list are distinct
        mine = full[b, idx[b, :n] - base]                                        # the oracle's distances of the device's rows
        assert not np.isnan(mine).any()
        assert (np.abs(mine.astype(np.float64) - want_d[b, :n].astype(np.float64)) <= NEAR).all(), b
        okc = _cos_ok(np.cos(mine.astype(np.float64) * np.pi))
        np.testing.assert_allclose(dist[b, :n][okc], mine[okc], atol=ATOL, rtol=0)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and _bits_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('k', [1, 5, 128])
@pytest.mark.parametrize('B,G,D', SHAPES)
def test_topk_ids_shapes(cuda, B, G, D, k, metric):
    """test_topk_gpu.py's shapes (tile tails in both dimensions, every probe-tile shape, k above one tile's rows, more than 512
    tiles) under four labellings: identities spread over the gallery, four contiguous rows each, all distinct (Gallery.topk's
    arrays bit for bit) and one label (Gallery.match's row)."""
    from deep_insight_face import oneshot
    probes, gal_np, _ = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    labs = _labellings(G)
    for labels in labs.values():
        _cap(full, labels, k, metric)
    gal = oneshot.Gallery(gal_np)
    p = torch.from_numpy(probes).cuda()
    for name, labels in labs.items():
        got = gal.topk_ids(probes, k, labels, metric)
        assert all(isinstance(a, np.ndarray) for a in got), name                # NumPy in -> NumPy out
        _check(got, full, labels, k, metric)
        if name == 'distinct':
            ti, td = gal.topk(probes, k, metric)
            assert np.array_equal(got[0], ti) and _bits_equal(got[1], td)
        if name == 'one':
            mi, md = gal.match(probes, metric)
            assert np.array_equal(got[0][:, 0], mi) and _bits_equal(got[1][:, 0], md)
            assert (got[0][:, 1:] == -1).all() and (got[2][:, 0] == 0).all()
        if name == 'spread':
            t = gal.topk_ids(p, k, torch.from_numpy(labels).cuda(), metric)     # CUDA tensors in -> CUDA tensors out
            assert all(torch.is_tensor(a) and a.is_cuda and tuple(a.shape) == (B, k) for a in t)
            assert t[0].dtype == torch.int64 and t[1].dtype == torch.float32 and t[2].dtype == torch.int64
            assert _same(_np(t), got)
            if k == 5:
                for g in (gal, gal_np):                                         # the module-level form, on a handle and on rows
                    assert _same(oneshot.topk_ids(probes, g, k, labels.astype(np.int32), metric), got)
    gal.close()


# ------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('B,G,D', [s for s in SHAPES if s[1] <= 8192])
def test_topk_ids_exact_on_the_device_distances(cuda, B, G, D, metric):
    """Device-only, exact on both metrics: Gallery.within with a tolerance that takes in every row returns every distance that
    is not NaN as the library computes it; the NumPy reduction of those equals topk_ids bit for bit, with and without the
    probe's own identity excluded."""
    from deep_insight_face import oneshot
    probes, gal_np, pick = _inputs(B, G, D)
    gal = oneshot.Gallery(gal_np)
    count, widx, wdist = gal.within(probes, np.inf if metric == 0 else 1.0, metric, max_hits=8192)
    dev = np.full((B, G), np.nan, dtype=np.float32)
    for b in range(B):
        n = int(count[b])
        assert n <= 8192
        dev[b, widx[b, :n]] = wdist[b, :n]
    assert not np.isnan(dev).any()
    for name, labels in _labellings(G).items():
        if name in ('spread', 'contiguous'):
            for ex in (None, pick.astype(np.int64)):
                for k in (1, 5, 128):
                    got = gal.topk_ids(probes, k, labels, metric, exclude=ex)
                    assert _same(got, ir.topk_ids_full(dev, labels, k, ex)), (name, ex is not None, k)
    gal.close()


# ------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('metric', [0, 1])
def test_topk_ids_exclusion(cuda, metric):
    """With the probe's identity excluded no listed row carries it; k = 1 is the nearest row of another identity; -1 excludes
    nothing; labels offset by 2**40 give the same rows (a 32-bit compare would take every label for the excluded one)."""
    from deep_insight_face import oneshot
    B, G, D = 130, 1000, 128
    probes, gal_np, pick = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    nid = G // 4
    labels = np.arange(G) % nid
    split = np.arange(G) // nid % 2
    ex = pick.astype(np.int64)
    gal = oneshot.Gallery(gal_np)
    for k in (1, 5, 128):
        _cap(full, labels, k, metric, ex)
        got = gal.topk_ids(probes, k, labels, metric, exclude=ex)
        _check(got, full, labels, k, metric, ex)
        assert not (got[2] == ex[:, None]).any()
        base = gal.topk_ids(probes, k, labels, metric)
        assert (base[2][:, 0] == ex).all()                                      # (without it the probe's identity leads)
        assert _same(gal.topk_ids(probes, k, labels, metric, exclude=np.full(B, -1)), base)
        assert _same(gal.topk_ids(probes, k, labels, metric, exclude=np.full(B, -(2 ** 40))), base)
        big = labels + 2 ** 40
        gb = gal.topk_ids(probes, k, big, metric, exclude=ex + 2 ** 40)
        assert np.array_equal(gb[0], got[0]) and _bits_equal(gb[1], got[1])
        assert np.array_equal(gb[2], np.where(got[2] >= 0, got[2] + 2 ** 40, -1))
        # identities that differ in the HIGH word alone (rows 0, 2 and rows 1, 3 of every identity): the same lists as under
        # small labels that keep them apart
        gh = gal.topk_ids(probes, k, big + split * 2 ** 32, metric, exclude=ex + 2 ** 40)
        gl = gal.topk_ids(probes, k, labels + split * nid, metric, exclude=ex)
        assert np.array_equal(gh[0], gl[0]) and _bits_equal(gh[1], gl[1])
        assert np.array_equal(gh[2], np.where(gl[2] >= 0, gl[2] % nid + 2 ** 40 + gl[2] // nid * 2 ** 32, -1))
        assert (gl[2][:, 0] == ex + nid).all()                                  # the other half of the probe's identity leads
    one = gal.topk_ids(probes, 1, labels, metric, exclude=ex)                   # the hardest negative: the nearest other row
    other = np.where(labels[None, :] == ex[:, None], np.nan, full)
    if metric == 0:
        assert np.array_equal(one[0][:, 0], np.nanargmin(other, axis=1))
    gal.close()


# ------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('metric', [0, 1])
def test_topk_ids_negative_labels(cuda, metric):
    from deep_insight_face import oneshot
    B, G, D = 65, 257, 512
    probes, gal_np, _ = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    labels = np.arange(G) // 4
    labels[np.arange(G) % 3 == 0] = -1 - np.arange(G)[np.arange(G) % 3 == 0]   # a third of the rows out, under several negatives
    gal = oneshot.Gallery(gal_np)
    for k in (1, 5, 128):
        _cap(full, labels, k, metric)
        got = gal.topk_ids(probes, k, labels, metric)
        _check(got, full, labels, k, metric)
        assert (labels[got[0][got[0] >= 0]] >= 0).all()
        idx, dist, lab = gal.topk_ids(probes, k, np.full(G, -1), metric)        # nothing usable: all padding
        assert (idx == -1).all() and np.isnan(dist).all() and (lab == -1).all()
    gal.close()


# ------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('k', [5, 128])
@pytest.mark.parametrize('B,G,D', [(64, 4097, 512), (130, 1000, 128)])
def test_topk_ids_every_seed(cuda, B, G, D, k, metric):
    """Option "topk_seed": 1 and 2 make the seed grow from a loose first tolerance, 1000 evaluates every tile in the first
    pass: bit-identical to the default, which is checked against the oracle."""
    from deep_insight_face import oneshot
    probes, gal_np, pick = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    labels = np.arange(G) % (G // 4)
    ex = pick.astype(np.int64)
    _cap(full, labels, k, metric)
    _cap(full, labels, k, metric, ex)
    gal = oneshot.Gallery(gal_np)
    p, lab, e = torch.from_numpy(probes).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(ex).cuda()
    base = _np(gal.topk_ids(p, k, lab, metric))
    base_x = _np(gal.topk_ids(p, k, lab, metric, exclude=e))
    _check(base, full, labels, k, metric)
    _check(base_x, full, labels, k, metric, ex)
    tiles = {}
    for seed in (1, 2, 1000, 0):
        gal.set_option('topk_seed', seed)
        assert _same(_np(gal.topk_ids(p, k, lab, metric)), base), seed
        tiles[seed] = gal.stat('topk_ids_tiles')
        assert _same(_np(gal.topk_ids(p, k, lab, metric, exclude=e)), base_x), seed
    gtiles = (G + 127) // 128
    assert tiles[1000] == B * gtiles and 0 < tiles[0] <= B * gtiles              # every tile in the seed; the stat counts them
    gal.close()


# ------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize('metric', [0, 1])
def test_topk_ids_work(cuda, metric):
    """The seed that grows: at four rows per identity, and with one identity filling the six tiles nearest to every probe, the
    call evaluates at most an eighth of the (probe, tile) pairs -- a condition (the simulation of test_topk_ids_ref.py gives
    20 of 516 tiles per probe without the band E, against 229 .. 516 for a single seed of k tiles)."""
    from deep_insight_face import oneshot
    B, G, D, k = 3, 66000, 32, 5
    probes, gal_np, _ = _inputs(B, G, D)
    labels = np.arange(G) % (G // 4)
    gtiles = (G + 127) // 128
    for name, (p, g, lab) in (('natural', (probes, gal_np, labels)), ('crowd', ir.crowd_inputs(probes, gal_np, labels))):
        full = _oracle(B, G, D, metric) if name == 'natural' else rank_ref.distances(p, g, metric)
        _cap(full, lab, k, metric)
        gal = oneshot.Gallery(g)
        got = gal.topk_ids(p, k, lab, metric)
        tiles = gal.stat('topk_ids_tiles')
        print(name, metric, 'topk_ids_tiles', tiles, 'of', B * gtiles)
        _check(got, full, lab, k, metric)
        assert 0 < tiles <= B * gtiles / 8, (name, tiles)
        if name == 'crowd':
            assert (got[2][:, 0] == lab.max()).all()                           # the crowd is one entry, the nearest
        gal.close()


# ------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize('metric', [0, 1])
def test_topk_ids_exact_ties(cuda, metric):
    """Identical enrolled rows (test_topk_exact_ties' table).  Tied rows of different labels: the lower row's identity comes
    first; tied rows of one label: the lower row is reported."""
    from deep_insight_face import oneshot
    probes, gal_np = gi.match_tie_inputs()
    G = gal_np.shape[0]
    copies = {0: (100, 300, 500), 1: (105, 305, 505), 2: (119, 319, 519), 3: (120, 320), 4: (139, 339), 5: (101, 301, 501),
              6: (110, 310, 510)}
    full = rank_ref.distances(probes, gal_np, metric)
    gal = oneshot.Gallery(gal_np)
    for seed in (0, 1):
        gal.set_option('topk_seed', seed)
        idx, dist, lab = gal.topk_ids(probes, 4, np.arange(G), metric)          # every copy an identity of its own
        for b, rows in copies.items():
            assert tuple(idx[b, :len(rows)]) == rows and tuple(lab[b, :len(rows)]) == rows, (seed, b, idx[b])
            assert (dist[b, :len(rows)] == dist[b, 0]).all()
        same = np.arange(G) % 200                                               # the copies of a row share its label
        idx, dist, lab = gal.topk_ids(probes, 4, same, metric)
        for b, rows in copies.items():
            assert idx[b, 0] == rows[0] and lab[b, 0] == rows[0] % 200, (seed, b, idx[b])
            assert not np.isin(idx[b, 1:], rows).any()
        if metric == 0:
            _check((idx, dist, lab), full, same, 4, 0)
        mixed = np.arange(G)                                                    # the first two copies share a label, the third not
        mixed[300:340] = mixed[100:140]
        idx, dist, lab = gal.topk_ids(probes, 4, mixed, metric)
        for b, rows in copies.items():
            assert tuple(idx[b, :len(rows) - 1]) == (rows[0],) + rows[2:], (seed, b, idx[b])
    gal.close()


@pytest.mark.parametrize('seed', [0, 1])
def test_topk_ids_near_ties(cuda, seed):
    """Rows one ulp, 1e-7 and 1e-4 apart and exact duplicates at shuffled positions: metric 0, bit-identical."""
    from deep_insight_face import oneshot
    probes, gal_np = gi.match_near_tie_inputs()
    G = gal_np.shape[0]
    full = rank_ref.distances(probes, gal_np, 0)
    assert not np.isnan(full).any()
    gal = oneshot.Gallery(gal_np)
    gal.set_option('topk_seed', seed)
    for labels in (np.arange(G) % 1024, np.arange(G) // 4, np.arange(G) % 7):
        for k in (5, 128):
            _check(gal.topk_ids(probes, k, labels, 0), full, labels, k, 0)
    gal.close()


# ------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize('name', [c[0] for c in gi.match_degenerate_cases()])
def test_topk_ids_degenerate(cuda, name):
    """Zero, tiny, huge and non-finite rows and probes, anti-parallel rows, four contiguous rows per identity: a row whose
    distance is NaN is never listed, an identity whose rows are all NaN is absent.  The probes that resolve every tile are
    among these."""
    from deep_insight_face import oneshot
    probes, gal_np = [(p, g) for n, p, g in gi.match_degenerate_cases() if n == name][0]
    G = gal_np.shape[0]
    labels = np.arange(G) // 4
    fulls = {metric: rank_ref.distances(probes, gal_np, metric) for metric in (0, 1)}
    for k in (1, 3, 128):
        _cap(fulls[1], labels, k, 1)
    gal = oneshot.Gallery(gal_np)
    for metric in (0, 1):
        for k in (1, 3, 128):
            got = gal.topk_ids(probes, k, labels, metric)
            _check(got, fulls[metric], labels, k, metric)
            for b in range(probes.shape[0]):
                assert not np.isnan(fulls[metric][b, got[0][b][got[0][b] >= 0]]).any()   # NaN rows are never listed
    gal.close()


def test_topk_ids_identical_probe_and_clamp_nan(cuda):
    """A probe equal to an enrolled row whose similarity rounds above 1: its distance is NaN and the identity is listed with
    its next row by default; with clamp_nan the clamped distance 0 is ordered and reported and that row leads."""
    from deep_insight_face import oneshot
    _, gal_np, _ = _inputs(65, 257, 512)
    G = gal_np.shape[0]
    rows = np.arange(0, 256, 4).astype(np.int64)
    probes = gal_np[rows].copy()
    labels = np.arange(G) % (G // 4)
    with np.errstate(invalid='ignore'):
        sim = od.similarity(probes, gal_np[rows])
    full = rank_ref.distances(probes, gal_np, 1)
    assert (sim > 1).any() and (sim <= 1).any()
    k = 5
    _cap(full, labels, k, 1)
    gal = oneshot.Gallery(gal_np)
    got = gal.topk_ids(probes, k, labels, 1)
    _check(got, full, labels, k, 1)
    assert (got[2][:, 0] == labels[rows]).all()                                 # the identity leads either way ...
    assert np.array_equal(got[0][:, 0] == rows, sim <= 1)                       # ... with another of its rows where the self row is NaN
    gal.set_option('clamp_nan', 1)
    cidx, cdist, clab = gal.topk_ids(probes, k, labels, 1)
    assert (cidx[:, 0] == rows).all() and not np.isnan(cdist).any() and (cdist[sim >= 1, 0] == 0).all()
    assert np.array_equal(clab, got[2]) and np.array_equal(cidx[:, 1:], got[0][:, 1:])
    gal.close()


# ------------------------------------------------------------------------------------------- 9
def test_topk_ids_handle_reuse_and_workspaces(cuda):
    """A non-monotone batch and k sequence on one handle, interleaved with topk, within, rank, update and remove (the labels
    moved as the reported moves say), against the recomputed oracle; a shard with an index_base: idx global, labels local."""
    from deep_insight_face import oneshot
    G, D = 4097, 128
    probes, gal_np, pick = _inputs(70, G, D)
    gal_np = gal_np.copy()
    labels = np.arange(G) % (G // 4)
    gal = oneshot.Gallery(gal_np)

    def check(n, k, metric=0, ex=None):
        full = rank_ref.distances(probes[:n], gal_np, metric)
        _cap(full, labels, k, metric, ex)
        got = gal.topk_ids(probes[:n], k, labels, metric, exclude=ex)
        _check(got, full, labels, k, metric, ex)
        return got

    t_before = gal.topk(probes, 5, 0)
    first = check(70, 5)
    gal.within(probes[:33], 0.5, 0, max_hits=8)
    check(33, 128)                                                              # a second call with fewer probes
    gal.rank(probes, first[0][:, 1], 0)
    again = check(70, 5)
    assert _same(first, again)
    t_mid = gal.topk(probes, 5, 0)
    assert np.array_equal(t_before[0], t_mid[0]) and _bits_equal(t_before[1], t_mid[1])
    rank, md = gal.rank(probes, first[0][:, 2], 0)                              # dif_match_rank returns the listed distance
    assert _bits_equal(md, first[1][:, 2])
    row = gal_np[first[0][0, 0]][None]                                          # probe 0's nearest row, appended five times under
    gal.update(np.repeat(row, 5, axis=0))                                       # new labels: ties at higher rows, listed behind it
    gal_np = np.concatenate([gal_np, np.repeat(row, 5, axis=0)])
    labels = np.concatenate([labels, 5000 + np.arange(5)])
    got = check(70, 5)
    assert list(got[0][0]) == [first[0][0, 0], G, G + 1, G + 2, G + 3] and list(got[2][0, 1:]) == [5000, 5001, 5002, 5003]
    check(33, 128, 1, pick[:33].astype(np.int64))
    gone = np.array([int(first[0][0, 0]), 7, 4000, G + 4], dtype=np.int64)      # un-enrol it, two strangers and the last copy
    moved_from, moved_to = gal.remove(gone)
    gal_np = remove_ref.remove_ref(gal_np, gone)[0]
    labels[moved_to] = labels[moved_from]
    labels = labels[:gal_np.shape[0]]
    assert len(gal) == gal_np.shape[0] == G + 1
    check(70, 5)
    check(70, 128, 1)
    gal.within(probes, 0.5, 1, max_hits=8)
    check(33, 5, 1, pick[:33].astype(np.int64))
    with pytest.raises(ValueError):
        gal.topk_ids(probes, 5, labels[:-1], 0)                                 # the labels follow the gallery's size
    gal.close()
    shifted = oneshot.Gallery(gal_np, index_base=1000)
    full = rank_ref.distances(probes, gal_np, 0)
    got = shifted.topk_ids(probes, 5, labels, 0)
    _check(got, full, labels, 5, 0, base=1000)
    assert (got[0] >= 1000).all() and np.array_equal(labels[got[0] - 1000], got[2])
    shifted.close()


# ------------------------------------------------------------------------------------------- 10
def test_topk_ids_arguments(cuda):
    from deep_insight_face import _native as N
    from deep_insight_face import oneshot
    B, G, D = 3, 129, 64
    probes, gal_np, _ = _inputs(B, G, D)
    full = _oracle(B, G, D, 1)
    labels = np.arange(G) // 4
    gal = oneshot.Gallery(gal_np)
    for k in (0, 129, -1, -128):
        with pytest.raises(ValueError):
            gal.topk_ids(probes, k, labels)
        with pytest.raises(ValueError):
            oneshot.topk_ids(probes, gal, k, labels, 0)
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        gal.topk_ids(probes, 3, labels, distance_metric=7)
    with pytest.raises(ValueError):
        gal.topk_ids(np.zeros((2, 32), dtype=np.float32), 3, labels)
    for bad in (labels[:-1], np.concatenate([labels, [0]]), labels.astype(np.float32), labels[None, :]):
        with pytest.raises(ValueError):
            gal.topk_ids(probes, 3, bad)
    for bad in (np.zeros(B + 1, dtype=np.int64), np.zeros(B, dtype=np.float64)):
        with pytest.raises(ValueError):
            gal.topk_ids(probes, 3, labels, exclude=bad)
    _check(gal.topk_ids(probes[0], 3, labels, 1), full[:1], labels, 3, 1)       # one probe as a vector
    p, lab = torch.from_numpy(probes).cuda(), torch.from_numpy(labels).cuda()
    k = 4
    idx = torch.empty((B, k), dtype=torch.int64, device='cuda')
    dist = torch.empty((B, k), dtype=torch.float32, device='cuda')
    out = torch.empty((B, k), dtype=torch.int64, device='cuda')
    gal.topk_ids_into(p, k, 1, lab, None, idx, dist, out)                       # the well-formed call
    torch.cuda.synchronize()
    _check(_np((idx, dist, out)), full, labels, k, 1)
    i2, d2 = torch.empty_like(idx), torch.empty_like(dist)
    gal.topk_ids_into(p, k, 1, lab, None, i2, d2)                               # the labels are optional
    torch.cuda.synchronize()
    assert torch.equal(i2, idx) and _bits_equal(d2.cpu().numpy(), dist.cpu().numpy())
    with pytest.raises(RuntimeError, match='Undefined distance metric 2'):
        gal.topk_ids_into(p, k, 2, lab, None, idx, dist, out)
    for bad_k in (0, 129, -3):
        with pytest.raises(ValueError):
            gal.topk_ids_into(p, bad_k, 1, lab, None, idx, dist, out)
    wide_i = torch.empty((B, 2 * k), dtype=torch.int64, device='cuda')
    for bad in (dict(idx=wide_i[:, ::2]), dict(idx=idx.to(torch.int32)), dict(dist=dist.double()), dict(probes=p.double()),
                dict(idx=idx[:2]), dict(dist=dist[:, :3]), dict(label=out[:, :3]), dict(label=out.to(torch.int32)),
                dict(lab=lab[:-1]), dict(lab=lab.to(torch.int32)), dict(lab=lab.cpu()), dict(ex=lab[:B + 1]),
                dict(ex=lab[:B].to(torch.int32)), dict(probes=p[:, :32]), dict(probes=probes), dict(idx=idx.cpu())):
        kw = dict(probes=p, lab=lab, ex=None, idx=idx, dist=dist, label=out)
        kw.update(bad)
        with pytest.raises(ValueError):
            gal.topk_ids_into(kw['probes'], k, 1, kw['lab'], kw['ex'], kw['idx'], kw['dist'], kw['label'])
    # the C entry point itself: the checks of dif_match_topk, and the labels
    call = N.lib.dif_match_topk_ids
    args = [gal._h, N.ptr(p), B, 1, k, N.ptr(lab), None, N.ptr(idx), N.ptr(dist), N.ptr(out), N.stream_ptr()]
    assert call(*args) == 0
    for pos, val in ((0, None), (1, None), (2, -1), (3, 2), (4, 0), (4, 129), (5, None), (7, None), (8, None)):
        bad = list(args)
        bad[pos] = val
        assert call(*bad) != 0, (pos, val)
    bad = list(args)
    bad[2], bad[1], bad[7] = 0, None, None                                      # n = 0 is a no-op
    assert call(*bad) == 0
    torch.cuda.synchronize()
    i0, d0, l0 = gal.topk_ids(np.zeros((0, D), dtype=np.float32), 3, labels)    # an empty batch
    assert i0.shape == (0, 3) and d0.shape == (0, 3) and l0.shape == (0, 3) and l0.dtype == np.int64
    gal.close()
    empty = oneshot.Gallery(emd_size=D)                                         # nothing enrolled: all padding
    for metric in (0, 1):
        for k in (1, 128):
            i0, d0, l0 = empty.topk_ids(probes, k, np.zeros(0, dtype=np.int64), metric)
            assert i0.shape == (B, k) and (i0 == -1).all() and np.isnan(d0).all() and (l0 == -1).all()
    assert empty.stat('topk_ids_tiles') == 0
    empty.close()


# ------------------------------------------------------------------------------------------- 11
@pytest.mark.parametrize('metric', [0, 1])
def test_evaluate_identification_ids(cuda, metric):
    """Rank 1 at the identity level is the share of probes whose nearest row carries their label; the CMC does not decrease;
    the tensor form equals the NumPy form."""
    from deep_insight_face import oneshot
    from deep_insight_face.evaluation import identification as ident
    B, G, D = 65, 257, 512
    probes, gal_np, pick = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    nid = G // 4
    labels = np.arange(G) % nid
    probe_labels = pick.astype(np.int64).copy()
    probe_labels[:3] = nid + 7                                                  # three probes of nobody enrolled
    gal = oneshot.Gallery(gal_np)
    out = ident.evaluate_identification_ids(gal, probes, probe_labels, labels, metric, max_rank=10)
    mated = probe_labels < nid
    assert np.array_equal(out['rank'] >= 0, mated) and (out['rank'][mated] <= 10).all()
    mi, _ = gal.match(probes, metric)
    assert out['cmc'][0] == np.float64((labels[mi] == probe_labels)[mated].sum()) / np.float64(mated.sum())
    assert (np.diff(out['cmc']) >= 0).all() and out['cmc'].shape == (10,)
    want = gal.topk_ids(probes, 10, labels, metric)
    assert _same((out['idx'], out['dist'], out['label']), want)
    assert np.array_equal(out['rank'], ident.identity_rank(want[2], probe_labels, mated))
    t = ident.evaluate_identification_ids(gal, torch.from_numpy(probes).cuda(), torch.from_numpy(probe_labels).cuda(),
                                          torch.from_numpy(labels).cuda(), metric, max_rank=10)
    assert all(torch.is_tensor(t[key]) and t[key].is_cuda for key in ('rank', 'cmc', 'idx', 'dist', 'label'))
    assert np.array_equal(t['rank'].cpu().numpy(), out['rank']) and np.array_equal(t['cmc'].cpu().numpy(), out['cmc'])
    assert _same(_np((t['idx'], t['dist'], t['label'])), want)
    rows = ident.evaluate_identification_ids(gal_np, probes, probe_labels, labels, metric, max_rank=10)   # rows to enrol
    assert np.array_equal(rows['rank'], out['rank'])
    gal.close()


# ------------------------------------------------------------------------------------------- 12
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('k', [5, 128])
@pytest.mark.parametrize('B,G,D', ROUND_SHAPES)
def test_topk_ids_rounds(cuda, B, G, D, k, metric):
    """Rounds of probes (test_topk_gpu.py's section 9): "topk_round" 0, 128 (and 256 at B = 300), 0 on one handle, four rows per
    identity, with every probe's own identity excluded -- another label from probe to probe -- and with no exclusion: every
    answer (idx, dist and label) passes the oracle check, and the forced-round answers and the one after the option is taken
    back equal the first one-round answer bit for bit.  "topk_ids_tiles" counts (probe, tile) evaluations, which do not depend
    on the split: the forced-round call reports the one-round call's number (a counter zeroed in every round reports the last
    round's alone).  Before the device is asked: the oracle under the excluded labels a dropped `+ b0` would read differs from
    the true one in every round after the first."""
    from deep_insight_face import oneshot
    probes, gal_np, pick = _inputs(B, G, D)
    full = _oracle(B, G, D, metric)
    assert not np.isnan(full).any()
    labels = (np.arange(G) % (G // 4)).astype(np.int64)
    ex = pick.astype(np.int64)
    want = ir.topk_ids_full(full, labels, k, ex)
    for per in _round_options(B)[1:-1]:
        wrong = ir.topk_ids_full(full, labels, k, _without_offset(ex, per))
        for sl in _later_rounds(B, per):
            assert (wrong[2][sl] != want[2][sl]).any(), (per, sl)
    _cap(full, labels, k, metric)
    _cap(full, labels, k, metric, ex)
    gal = oneshot.Gallery(gal_np)
    p, lab, e = torch.from_numpy(probes).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(ex).cuda()
    tiles = {}
    for name, excl, excl_dev in (('excluded', ex, e), ('all', None, None)):
        first = None
        for per in _round_options(B):
            gal.set_option('topk_round', per)
            got = _np(gal.topk_ids(p, k, lab, metric, exclude=excl_dev))
            tiles.setdefault(name, []).append(gal.stat('topk_ids_tiles'))
            _check(got, full, labels, k, metric, excl)
            first = first or got
            assert _same(got, first), (name, per)
    print('topk_ids_tiles', (B, G, D), k, metric, tiles)
    gtiles = (G + 127) // 128
    for name, counts in tiles.items():
        assert 0 < counts[0] <= B * gtiles and counts == [counts[0]] * len(counts), (name, counts)
    with pytest.raises(ValueError, match='topk_round'):
        gal.set_option('topk_round', 100)                                       # not a multiple of 128
    gal.close()
