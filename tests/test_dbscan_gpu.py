"""Gallery.dbscan (dif_gallery_dbscan) against the CPU oracle tests/dbscan_ref.py: labels, degree and counts must equal the
oracle's exactly, for every row.

Tolerances follow test_cluster_gpu.py's rule: the midpoint of the widest gap between the oracle's pairwise distances, asserted on
the CPU to exceed 2e-5 (metric 1: the device's arccos is evaluated in double and rounded once, NumPy's float32 arccos is within
2 ulp of that, so a pair within 2e-6 of the tolerance may fall on either side; metric 0 is bit-identical and takes the same
rule).  The rows (dbscan_ref.make_rows) place that gap between the edges and the nearest non-edges of an identity, so that
core, border and noise rows all occur; the seeds below are the ones for which the widest gap lies there, found on the CPU."""
import functools

import numpy as np
import pytest
import torch

import cluster_ref as cr
import dbscan_ref as dr

pytestmark = pytest.mark.gpu
MIN_GAP = 2e-5
SHAPES = [1, 2, 127, 128, 129, 385, 1025]
DIMS = [32, 128, 512]
SEEDS = {(385, 32, 0): 1, (128, 32, 0): 2, (129, 128, 0): 1}     # (G, D, metric) -> make_rows' seed; 0 everywhere else


@functools.lru_cache(maxsize=None)
def _rows(G, D, metric):
    return dr.make_rows(G, D, metric, SEEDS.get((G, D, metric), 0))


@functools.lru_cache(maxsize=None)
def _lower(G, D, metric):
    return cr.lower_distances(_rows(G, D, metric), metric)


def _gap_t(vals):
    """test_cluster_gpu.py's rule: the midpoint of the widest gap between adjacent sorted pairwise distances, asserted wide
    enough; with fewer than two values: one tolerance above and one below the only value (or 0.5 when there is no pair)."""
    v = np.sort(np.asarray(vals, dtype=np.float64))
    if v.size == 0:
        return [np.float32(0.5)]
    if v.size == 1:
        assert v[0] > 4 * MIN_GAP
        return [np.float32(v[0] * 2), np.float32(v[0] / 2)]
    gaps = np.diff(v)
    k = int(np.argmax(gaps))
    assert gaps[k] > MIN_GAP, gaps[k]
    return [np.float32((v[k] + v[k + 1]) / 2)]


@functools.lru_cache(maxsize=None)
def _case(G, D, metric):
    """-> (rows, lower, tolerances) with the oracle's kinds at min_samples = 4 asserted: a sweep without a border row tests
    nothing."""
    rows, lower = _rows(G, D, metric), _lower(G, D, metric)
    ts = _gap_t(cr.pair_values(lower))
    if G >= 127:
        labels, degree, _ = dr.dbscan_from(lower, G, ts[0], 4)
        core, border, noise = dr.kinds(labels, degree, 4)
        assert core.sum() >= 10 and border.sum() >= 10 and noise.sum() >= 10, (core.sum(), border.sum(), noise.sum())
    return rows, lower, ts


def _run(gal, t, min_samples, metric):
    labels, degree, counts = gal.dbscan(t, min_samples, metric)
    assert labels.is_cuda and labels.dtype == torch.int64 and labels.shape == (len(gal),)
    assert degree.is_cuda and degree.dtype == torch.int32 and degree.shape == (len(gal),)
    assert counts.is_cuda and counts.dtype == torch.int64 and counts.shape == (2,)
    return labels.cpu().numpy(), degree.cpu().numpy(), tuple(counts.cpu().tolist())


def _same(got, want):
    assert tuple(got[2]) == tuple(want[2]), (got[2], want[2])
    for a, b in ((got[1], want[1]), (got[0], want[0])):
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (bad[:8], a[bad[:8]], b[bad[:8]])


# ------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('D', DIMS)
@pytest.mark.parametrize('G', SHAPES)
def test_dbscan_shapes(cuda, G, D, metric):
    """One row, one pair, a tile less one, a whole tile, a tile and one, three probe blocks and one, nine; one round and
    rounds of 128 probes (nine at 1025: a border row and its anchor lie in different rounds and tiles); min_samples 1, 2, 4.
    min_samples = 1 must also be `cluster` bit for bit, and under metric 0 the degree must be `within`'s count."""
    from deep_insight_face import oneshot
    rows, lower, ts = _case(G, D, metric)
    gal = oneshot.Gallery(rows)
    for t in ts:
        for ms in (1, 2, 4):
            want = dr.dbscan_from(lower, G, t, ms)
            _same(_run(gal, t, ms, metric), want)
            gal.set_option('cluster_round', 128)
            _same(_run(gal, t, ms, metric), want)
            gal.set_option('cluster_round', 0)
        labels, _, counts = gal.dbscan(t, 1, metric)
        cl, n = gal.cluster(t, metric)
        assert torch.equal(labels, cl) and counts.tolist() == [int(n), 0]
        if metric == 0:
            # ref_distance is bit-symmetric under metric 0 ((a - b)^2 == (b - a)^2), so the full square's count is the
            # triangle's degree once the self hit (distance 0: a hit iff t >= 0) is taken for the row itself
            count = gal.within(rows, t, 0, max_hits=0)[0]
            degree = gal.dbscan(t, 4, 0)[1].cpu().numpy()
            self_hit = 1                                      # finite rows and t >= 0
            assert t >= 0 and np.isfinite(rows).all() and np.array_equal(degree, count - self_hit + 1)
    gal.close()


@pytest.mark.parametrize('metric', [0, 1])
def test_dbscan_default_rounds(cuda, metric):
    """Above 2048 rows the default takes two rounds (2048 probes, then 152): the link sweep builds its census again; one round
    of 2304 keeps the degree sweep's."""
    from deep_insight_face import oneshot
    G, D = 2200, 32
    rows, lower, (t,) = _case(G, D, metric)
    gal = oneshot.Gallery(rows)
    for ms in (2, 4):
        want = dr.dbscan_from(lower, G, t, ms)
        for per in (0, 2304):
            gal.set_option('cluster_round', per)
            _same(_run(gal, t, ms, metric), want)
    gal.close()


# ------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('swap', [False, True])
def test_dbscan_chaining_case(cuda, swap):
    """Metric 0, exact coordinates, t = 1, min_samples = 4: `cluster` fuses the two people through the bridge row, `dbscan`
    keeps them apart; the bridge is a border row, equidistant (1.0 exactly), and goes with the lower-numbered core in both
    storage orders; moved to -0.25 it goes to A in both; the far row is noise."""
    from deep_insight_face import oneshot
    rows, at = dr.bridge_rows(0.0, swap)
    gal = oneshot.Gallery(rows)
    cl, n = gal.cluster(1.0, 0)
    cl = cl.cpu().numpy()
    assert int(n) == 2 and cl[at['cA']] == cl[at['cB']] == cl[at['bridge']] and cl[at['far']] == at['far']
    got = _run(gal, 1.0, 4, 0)
    _same(got, dr.dbscan(rows, 1.0, 4, 0))
    labels, degree, counts = got
    assert counts == (2, 1) and labels[at['far']] == -1 and degree[at['bridge']] == 3
    assert labels[at['cA']] != labels[at['cB']]
    assert labels[at['bridge']] == labels[min(at['cA'], at['cB'])]
    gal.close()
    rows, at = dr.bridge_rows(-0.25, swap)
    got = _run(oneshot.Gallery(rows), 1.0, 4, 0)
    _same(got, dr.dbscan(rows, 1.0, 4, 0))
    assert got[0][at['bridge']] == got[0][at['cA']] != got[0][at['cB']] and got[0][at['far']] == -1 and got[2] == (2, 1)


# ------------------------------------------------------------------------------------------- 3
def _degenerate_rows(metric, D=64):
    rows = _rows(160, D, metric).copy()
    rows[3] = 0
    rows[130] = 0                                             # two zero-norm rows, in different tiles
    rows[10] = np.nan
    rows[50, 5] = np.nan
    rows[20] = np.inf
    rows[60, 1] = -np.inf
    rows[70] = rows[30] * np.float32(1e-25)                   # |x|^2 underflows
    rows[139] = rows[31] * np.float32(1e-25)
    rows[80] = rows[32] * np.float32(1e25)                    # |x|^2 overflows
    rows[150] = rows[33] * np.float32(1e25)
    rows[90:100] = rows[40:50]                                # identical twins, in one tile
    rows[140:148] = rows[0:8]                                 # ... and across tiles (row 3's twin is a zero row too)
    return rows


@pytest.mark.parametrize('clamp', [0, 1])
@pytest.mark.parametrize('metric', [0, 1])
def test_dbscan_degenerate_rows(cuda, metric, clamp):
    """Zero-norm, NaN, +-inf, 1e-25- and 1e25-scaled rows and identical twins: no special rule, the oracle decides; every row
    keeps degree >= 1 whatever its distance to itself is."""
    from deep_insight_face import oneshot
    rows = _degenerate_rows(metric)
    G = len(rows)
    lower = cr.lower_distances(rows, metric, clamp=bool(clamp))
    vals = cr.pair_values(lower)
    (t,) = _gap_t(vals[(vals > 0) & ((vals < 1) | (metric == 0))])
    if metric == 1:
        assert (np.abs(vals - float(t)) > MIN_GAP).all()
    gal = oneshot.Gallery(rows)
    gal.set_option('clamp_nan', clamp)
    for ms in (1, 2, 3):
        want = dr.dbscan_from(lower, G, t, ms)
        got = _run(gal, t, ms, metric)
        _same(got, want)
        assert (got[1] >= 1).all()
    # the tolerance the rows were built for, between an identity's edges and its nearest non-edges: no pair lies near it
    t = np.float32((dr.EDGE[metric][1] + dr.NEAR[metric][0]) / 2)
    assert (np.abs(vals - float(t)) > MIN_GAP).all()
    for ms in (2, 4):
        want = dr.dbscan_from(lower, G, t, ms)
        if ms == 4:
            assert all(k.sum() >= 5 for k in dr.kinds(want[0], want[1], 4))
        _same(_run(gal, t, ms, metric), want)
    if metric == 1:
        assert (want[1][[3, 130, 10, 20]] == 1).all()         # NaN distances to everything: alone
        for ms in (2, 50):                                    # t = 1: every pair whose distance is not NaN is an edge
            want = dr.dbscan_from(lower, G, 1.0, ms)
            assert want[2][1] >= 4
            _same(_run(gal, 1.0, ms, 1), want)
    for ms, lab, cnt in ((1, np.arange(G), (G, 0)), (2, np.full(G, -1), (0, G))):   # t < 0: degree 1 everywhere
        _same(_run(gal, -1.0, ms, metric), (lab, np.ones(G, dtype=np.int32), cnt))
    gal.close()


def test_dbscan_exact_copies(cuda):
    """100 exact copies of a row (itself and 99 more) among others, metric 0, t = 0: degree 100 each; core at min_samples 100,
    noise at 101."""
    from deep_insight_face import oneshot
    base = _rows(129, 32, 0)
    rows = np.concatenate([base[:40], np.repeat(base[7:8], 99, axis=0), base[40:]])
    G = len(rows)
    lower = cr.lower_distances(rows, 0)
    gal = oneshot.Gallery(rows)
    for ms, counts in ((100, (1, G - 100)), (101, (0, G))):
        want = dr.dbscan_from(lower, G, 0.0, ms)
        assert want[2] == counts and (want[1][40:139] == 100).all() and want[1][7] == 100
        _same(_run(gal, 0.0, ms, 0), want)
    gal.close()


# ------------------------------------------------------------------------------------------- 4
def test_dbscan_handle_reuse_and_determinism(cuda):
    """dbscan interleaved with cluster, match, within (B = 70, 33, 70), update and remove on one handle -- the workspaces are
    shared -- with G growing and shrinking between calls (385 -> 1025 -> 129); index_base 1000 (noise stays -1); two calls
    give identical tensors; degree NULL through the raw entry."""
    from deep_insight_face import oneshot
    from deep_insight_face import _native as N
    D, base = 128, 1000
    rows, lower, (t,) = _case(1025, D, 0)
    probes = (rows[5:75] + np.float32(0.01) * np.random.default_rng(7).standard_normal((70, D)).astype(np.float32))

    def fresh(r, fn):
        g = oneshot.Gallery(r, index_base=base)
        try:
            return fn(g)
        finally:
            g.close()

    def same_within(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))

    G0 = 385
    want0 = dr.dbscan_from(lower[:G0], G0, t, 4, index_base=base)
    want1 = dr.dbscan_from(lower, 1025, t, 4, index_base=base)
    assert (want0[0] == -1).any() and (want1[0] == -1).any() and want1[0].max() >= base
    w70 = fresh(rows[:G0], lambda g: g.within(probes, t, 0, max_hits=8))
    w33 = fresh(rows[:G0], lambda g: g.within(probes[:33], t, 0, max_hits=8))
    m70 = fresh(rows[:G0], lambda g: g.match(probes, 0))
    gal = oneshot.Gallery(rows[:G0], index_base=base)
    same_within(gal.within(probes, t, 0, max_hits=8), w70)
    _same(_run(gal, t, 4, 0), want0)
    same_within(gal.within(probes[:33], t, 0, max_hits=8), w33)
    a, b = gal.dbscan(t, 4, 0), gal.dbscan(t, 4, 0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                        # determinism
    cl = gal.cluster(t, 0)
    want_cl = cr.cluster_from(lower[:G0], G0, t, index_base=base)
    assert np.array_equal(cl[0].cpu().numpy(), want_cl[0]) and int(cl[1]) == want_cl[1]
    _same(_run(gal, t, 4, 0), want0)                                           # cluster left nothing behind in parent
    m = gal.match(probes, 0)
    assert np.array_equal(m[0], m70[0]) and np.array_equal(m[1].view(np.uint32), m70[1].view(np.uint32))
    same_within(gal.within(probes, t, 0, max_hits=8), w70)
    gal.update(rows[G0:])                                                      # 385 -> 1025
    _same(_run(gal, t, 4, 0), want1)
    same_within(gal.within(probes, t, 0, max_hits=8), fresh(rows, lambda g: g.within(probes, t, 0, max_hits=8)))
    a, b = gal.dbscan(t, 4, 0), gal.dbscan(t, 4, 0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # degree NULL through the raw entry: the same labels and counts
    lab = torch.empty(1025, dtype=torch.int64, device='cuda')
    cnt = torch.empty(2, dtype=torch.int64, device='cuda')
    assert N.lib.dif_gallery_dbscan(gal._h, 0, float(t), 4, N.ptr(lab), None, N.ptr(cnt), N.stream_ptr()) == 0
    assert torch.equal(lab, a[0]) and torch.equal(cnt, a[2])
    gal.dbscan_into(t, 4, 0, lab, None, cnt)
    assert torch.equal(lab, a[0]) and torch.equal(cnt, a[2])
    # 1025 -> 129: the rows that `remove` leaves, in its order, decide
    gal.remove(np.arange(base + 129, base + 1025))
    assert len(gal) == 129
    left = rows[:129]
    want2 = dr.dbscan(left, t, 2, 0, index_base=base)
    _same(_run(gal, t, 2, 0), want2)
    cl = gal.cluster(t, 0)
    assert np.array_equal(cl[0].cpu().numpy(), cr.cluster(left, t, 0, index_base=base)[0])
    gal.close()


# ------------------------------------------------------------------------------------------- 5
def test_dbscan_oneshot_and_frame_faces(cuda):
    from deep_insight_face import oneshot
    from deep_insight_face.detector.faces import FrameFaces
    G, D = 129, 128
    rows, lower, (t,) = _case(G, D, 1)
    want = dr.dbscan_from(lower, G, t, 3)
    got = oneshot.dbscan(rows, t)                                              # min_samples 3 and metric 1 are the defaults
    _same((got[0].cpu().numpy(), got[1].cpu().numpy(), tuple(got[2].tolist())), want)
    got = oneshot.dbscan(torch.from_numpy(rows).cuda(), t, 4, 1)
    _same((got[0].cpu().numpy(), got[1].cpu().numpy(), tuple(got[2].tolist())), dr.dbscan_from(lower, G, t, 4))

    def faces(emb):
        m = emb.shape[0]
        z = torch.zeros
        return FrameFaces(offsets=torch.tensor([0, m]), frame=z(m, dtype=torch.int64), boxes=z((m, 4)), scores=z(m), landmarks=None,
                          crops=z((m, 8, 8, 3), dtype=torch.uint8), emb=emb)

    lab = faces(torch.from_numpy(rows).cuda()).dbscan(t)
    assert lab.is_cuda and lab.dtype == torch.int64 and np.array_equal(lab.cpu().numpy(), want[0])
    rows0, lower0, (t0,) = _case(G, D, 0)
    lab = faces(torch.from_numpy(rows0).cuda()).dbscan(t0, min_samples=4, distance_metric=0)
    assert np.array_equal(lab.cpu().numpy(), dr.dbscan_from(lower0, G, t0, 4)[0])
    none = faces(torch.zeros((0, D), device='cuda')).dbscan(t)                 # M == 0: an empty tensor
    assert none.shape == (0,) and none.dtype == torch.int64
    with pytest.raises(ValueError):
        faces(torch.zeros((0, D), device='cuda'))._replace(emb=None).dbscan(t)
    empty = oneshot.Gallery(emd_size=D)                                        # an empty gallery: counts {0, 0}
    lab, deg, cnt = empty.dbscan(0.5)
    assert lab.shape == (0,) and deg.shape == (0,) and cnt.tolist() == [0, 0]
    empty.close()
    # min_samples above the row count: all noise
    gal = oneshot.Gallery(rows)
    lab, deg, cnt = gal.dbscan(1.0, G + 1, 1)
    assert (lab == -1).all() and cnt.tolist() == [0, G]
    gal.close()


def test_dbscan_arguments(cuda):
    from deep_insight_face import oneshot
    from deep_insight_face import _native as N
    G, D = 129, 32
    gal = oneshot.Gallery(_rows(G, D, 1))
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        gal.dbscan(0.5, 3, 7)
    with pytest.raises(ValueError):
        gal.dbscan(float('nan'))
    for bad in (0, -3):
        with pytest.raises(ValueError, match='min_samples'):
            gal.dbscan(0.5, bad)
    lab = torch.empty(G, dtype=torch.int64, device='cuda')
    deg = torch.empty(G, dtype=torch.int32, device='cuda')
    cnt = torch.empty(2, dtype=torch.int64, device='cuda')
    gal.dbscan_into(0.5, 3, 1, lab, deg, cnt)                                  # the well-formed call
    for kw in (dict(labels=lab[:-1]), dict(labels=lab.to(torch.int32)), dict(labels=lab.cpu()), dict(degree=deg[:-1]),
               dict(degree=deg.to(torch.int64)), dict(degree=deg.cpu()), dict(counts=cnt.cpu()), dict(counts=cnt[:1]),
               dict(counts=cnt.to(torch.int32)), dict(counts=torch.empty(3, dtype=torch.int64, device='cuda'))):
        a = dict(labels=lab, degree=deg, counts=cnt)
        a.update(kw)
        with pytest.raises(ValueError):
            gal.dbscan_into(0.5, 3, 1, a['labels'], a['degree'], a['counts'])
    # the library's own checks, below the Python layer
    assert N.lib.dif_gallery_dbscan(gal._h, 1, 0.5, 0, N.ptr(lab), N.ptr(deg), N.ptr(cnt), None) != 0
    assert b'min_samples' in N.lib.dif_last_error()
    assert N.lib.dif_gallery_dbscan(gal._h, 7, 0.5, 3, N.ptr(lab), N.ptr(deg), N.ptr(cnt), None) != 0
    assert N.lib.dif_gallery_dbscan(gal._h, 1, float('nan'), 3, N.ptr(lab), N.ptr(deg), N.ptr(cnt), None) != 0
    assert N.lib.dif_gallery_dbscan(gal._h, 1, 0.5, 3, None, N.ptr(deg), N.ptr(cnt), None) != 0
    assert N.lib.dif_gallery_dbscan(gal._h, 1, 0.5, 3, N.ptr(lab), N.ptr(deg), None, None) != 0
    gal.close()
