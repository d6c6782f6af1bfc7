"""Gallery.cluster (dif_gallery_cluster) against the CPU oracle tests/cluster_ref.py: labels and n_clusters must equal the
oracle's exactly, for every row.

Metric 1: the device evaluates arccos in double and rounds once, NumPy's float32 arccos is within 2 ulp of that, so a pair
whose oracle distance lies within 2e-6 of the tolerance may fall on either side.  Every tolerance below is therefore the
midpoint of the widest gap between the oracle's pairwise distances (test_within_gpu.py's _sparse_t), and the gap is asserted
on the CPU to exceed 2e-5 before the device is asked anything.  Metric 0 is bit-identical and takes the same rule."""
import functools

import numpy as np
import pytest
import torch

import cluster_ref as cr

pytestmark = pytest.mark.gpu
MIN_GAP = 2e-5


@functools.lru_cache(maxsize=None)
def _rows(G, D, seed=0):
    """Identities with four near-duplicate rows each (test_within_gpu.py's _inputs): row i belongs to identity i % (G // 4),
    so a component's rows lie a quarter of the gallery apart -- across 128-row tiles and probe blocks from G = 129 up."""
    rng = np.random.default_rng(1000 * G + D + seed)
    nid = max(1, G // 4)
    centres = rng.standard_normal((nid, D))
    rows = (centres[np.arange(G) % nid] + 0.05 * rng.standard_normal((G, D))).astype(np.float32)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _lower(G, D, metric):
    return cr.lower_distances(_rows(G, D), metric)


def _gap_t(vals):
    """Midpoint of the widest gap between adjacent sorted pairwise distances, asserted wide enough; with fewer than two
    values: one tolerance above and one below the only value (or 0.5 when there is no pair at all)."""
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


def _run(gal, t, metric, **kw):
    labels, n = gal.cluster(t, metric, **kw)
    assert torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int64 and labels.shape == (len(gal),)
    assert torch.is_tensor(n) and n.is_cuda and n.dtype == torch.int64 and n.dim() == 0
    return labels.cpu().numpy(), int(n.item())


def _same(got, want):
    assert got[1] == want[1], (got[1], want[1])
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, (bad[:8], got[0][bad[:8]], want[0][bad[:8]])


# ------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('D', [32, 128, 512])
@pytest.mark.parametrize('G', [1, 2, 127, 128, 129, 385, 1025])
def test_cluster_shapes(cuda, G, D, metric):
    """One row, one pair, a tile less one, a whole tile, a tile and one, three probe blocks and one, nine; with "cluster_round"
    128 the last shape takes nine rounds, with the default one: both must give the oracle's arrays."""
    from deep_insight_face import oneshot
    rows, lower = _rows(G, D), _lower(G, D, metric)
    gal = oneshot.Gallery(rows)
    for t in _gap_t(cr.pair_values(lower)):
        want = cr.cluster_from(lower, G, t)
        if G >= 127:
            assert want[1] == G // 4                          # the identities, no more and no less
        _same(_run(gal, t, metric), want)
        gal.set_option('cluster_round', 128)
        _same(_run(gal, t, metric), want)
        gal.set_option('cluster_round', 0)
    gal.close()


@pytest.mark.parametrize('metric', [0, 1])
def test_cluster_default_rounds(cuda, metric):
    """Above 2048 rows the default takes more than one round (2048 probes, then 152); one round of 2304 and eighteen of 128
    must give the same arrays."""
    from deep_insight_face import oneshot
    G, D = 2200, 32
    rows, lower = _rows(G, D), _lower(G, D, metric)
    (t,) = _gap_t(cr.pair_values(lower))
    want = cr.cluster_from(lower, G, t)
    assert want[1] == G // 4
    gal = oneshot.Gallery(rows)
    for per in (0, 2304, 128):
        gal.set_option('cluster_round', per)
        _same(_run(gal, t, metric), want)
    gal.close()


# ------------------------------------------------------------------------------------------- 2
def test_cluster_chain(cuda):
    """300 points on a line, delta apart, stored in a fixed random order: hooks go both up and down and paths get long.
    Metric 0 (bit-identical): between delta^2 and 4 delta^2 only neighbours are edges and the chain is one component."""
    from deep_insight_face import oneshot
    n, delta = 300, np.float32(0.25)                          # k * delta and its squares are exact in float32
    perm = np.random.default_rng(300).permutation(n)
    rows = np.full((n, 32), 0.5, dtype=np.float32)
    rows[:, 0] = perm.astype(np.float32) * delta
    lower = cr.lower_distances(rows, 0)
    vals = np.unique(cr.pair_values(lower))
    assert vals[0] == delta ** 2 and vals[1] == 4 * delta ** 2
    gal = oneshot.Gallery(rows, index_base=5)
    gal.set_option('cluster_round', 128)
    t = np.float32(2 * delta ** 2)
    want = cr.cluster_from(lower, n, t, index_base=5)
    assert want[1] == 1 and (want[0] == 5).all()
    _same(_run(gal, t, 0), want)
    _same(_run(gal, np.float32(delta ** 2), 0), want)         # inclusive: t ON the neighbours' distance
    t = np.nextafter(np.float32(delta ** 2), np.float32(0))
    want = cr.cluster_from(lower, n, t, index_base=5)
    assert want[1] == n and np.array_equal(want[0], 5 + np.arange(n))
    _same(_run(gal, t, 0), want)
    gal.close()
    # exact copies of a row: one component under metric 0 with t = 0
    base = _rows(129, 32)
    rows = np.concatenate([base[:40], np.repeat(base[7:8], 100, axis=0), base[40:]])
    want = cr.cluster(rows, 0.0, 0)
    assert want[1] == len(rows) - 100 and (want[0][40:140] == 7).all()
    gal = oneshot.Gallery(rows)
    _same(_run(gal, 0.0, 0), want)
    gal.close()


# ------------------------------------------------------------------------------------------- 3
def _degenerate_rows(D=64):
    rows = _rows(160, D).copy()
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
def test_cluster_degenerate_rows(cuda, metric, clamp):
    """Zero-norm, NaN, +-inf, 1e-25- and 1e25-scaled rows and identical twins among ordinary ones: no special rule, the oracle
    decides (whatever IEEE arithmetic gives the reference; NaN is no edge), for both values of "clamp_nan"."""
    from deep_insight_face import oneshot
    rows = _degenerate_rows()
    lower = cr.lower_distances(rows, metric, clamp=bool(clamp))
    vals = cr.pair_values(lower)
    # (the twins' zeros and, under metric 1, the clamped 1s aside: the gap between mates and strangers)
    (t,) = _gap_t(vals[(vals > 0) & ((vals < 1) | (metric == 0))])
    if metric == 1:
        assert (np.abs(vals - float(t)) > MIN_GAP).all()
    want = cr.cluster_from(lower, len(rows), t)
    assert 10 < want[1] < len(rows)
    if metric == 1:
        assert want[0][10] == 10 and want[0][3] == 3 and want[0][130] == 130 and want[0][20] == 20   # NaN distances: alone
    gal = oneshot.Gallery(rows)
    gal.set_option('clamp_nan', clamp)
    _same(_run(gal, t, metric), want)
    if metric == 1:
        twins_nan = [np.isnan(lower[r][r - 50]) for r in range(90, 100)]
        if clamp:
            assert not any(twins_nan)
        # t = 1: one component of every row with a distance that is not NaN, the NaN rows alone
        want = cr.cluster_from(lower, len(rows), 1.0)
        assert 1 < want[1] < 20
        _same(_run(gal, 1.0, 1), want)
    _same(_run(gal, -1.0, metric), (np.arange(len(rows)), len(rows)))   # t < 0: all singletons
    gal.close()


# ------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('G0,G1,per', [(257, 387, 0), (130, 300, 128)])
def test_cluster_incremental_and_index_base(cuda, G0, G1, per):
    """set 257 rows, cluster, update with 130 more, cluster(first_row=257, labels=prev) == the full call on 387 rows; the
    same with first_row = G (labels copied) and 0; labels and labels_in shifted by index_base; a bad labels_in entry.
    (130, 300) with "cluster_round" 128: first_row lies inside the first round's probe block -- the blocks of rows 128 and
    129 return before the walk -- and a second round, [256, 300), follows."""
    from deep_insight_face import oneshot
    D, base = 128, 1000
    rows = _rows(G1, D)
    for metric in (0, 1):
        lower = _lower(G1, D, metric)
        (t,) = _gap_t(cr.pair_values(lower))
        want0 = cr.cluster_from(lower[:G0], G0, t, index_base=base)
        want1 = cr.cluster_from(lower, G1, t, index_base=base)
        assert want1[0].min() == base and want0[1] == want1[1] == G1 // 4   # every identity has a row among the first G0
        gal = oneshot.Gallery(rows[:G0], index_base=base)
        gal.set_option('cluster_round', per)
        prev, n0 = gal.cluster(t, metric)
        _same((prev.cpu().numpy(), int(n0)), want0)
        gal.update(rows[G0:])
        assert len(gal) == G1
        _same(_run(gal, t, metric, first_row=G0, labels=prev), want1)
        _same(_run(gal, t, metric, first_row=G0, labels=prev.cpu().numpy()), want1)       # NumPy labels are taken too
        full = gal.cluster(t, metric)
        _same((full[0].cpu().numpy(), int(full[1])), want1)
        _same(_run(gal, t, metric, first_row=G1, labels=full[0]), want1)                  # nothing to do: labels copied
        _same(_run(gal, t, metric, first_row=0, labels=None), want1)
        # the allocation-free form, in place: labels_in is the head of labels_out
        buf = torch.empty(G1, dtype=torch.int64, device='cuda')
        buf[:G0] = prev
        n = torch.empty(1, dtype=torch.int64, device='cuda')
        gal.cluster_into(t, metric, buf, n, first_row=G0, prev=buf)
        _same((buf.cpu().numpy(), int(n.item())), want1)
        # an entry that points above its own row (or below index_base) cannot come from an earlier call
        for pos, val in ((5, base + 6), (0, base - 1), (G0 - 1, base + G1 + 7)):
            bad = prev.clone()
            bad[pos] = val
            assert _run(gal, t, metric, first_row=G0, labels=bad)[1] == -1
        _same(_run(gal, t, metric, first_row=G0, labels=prev), want1)                      # ... and leaves nothing behind
        gal.close()


# ------------------------------------------------------------------------------------------- 5
def test_cluster_handle_reuse_and_determinism(cuda):
    """cluster interleaved with match, within (B = 70, 33, 70), update and a second cluster at a larger G: every answer equals
    the one from a fresh handle; two calls give bit-identical label tensors."""
    from deep_insight_face import oneshot
    D = 128
    rows = _rows(1025, D)
    G0 = 385
    probes = (rows[5:75] + np.float32(0.01) * np.random.default_rng(7).standard_normal((70, D)).astype(np.float32))

    def fresh(r, fn):
        g = oneshot.Gallery(r)
        try:
            return fn(g)
        finally:
            g.close()

    def same_within(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))

    lower = _lower(1025, D, 0)
    (t,) = _gap_t(cr.pair_values(lower))
    want0, want1 = cr.cluster_from(lower[:G0], G0, t), cr.cluster_from(lower, 1025, t)
    gal = oneshot.Gallery(rows[:G0])
    w70 = fresh(rows[:G0], lambda g: g.within(probes, t, 0, max_hits=8))
    w33 = fresh(rows[:G0], lambda g: g.within(probes[:33], t, 0, max_hits=8))
    m70 = fresh(rows[:G0], lambda g: g.match(probes, 0))
    same_within(gal.within(probes, t, 0, max_hits=8), w70)
    _same(_run(gal, t, 0), want0)
    same_within(gal.within(probes[:33], t, 0, max_hits=8), w33)
    a, b = gal.cluster(t, 0), gal.cluster(t, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                 # determinism
    _same((a[0].cpu().numpy(), int(a[1])), want0)
    m = gal.match(probes, 0)
    assert np.array_equal(m[0], m70[0]) and np.array_equal(m[1].view(np.uint32), m70[1].view(np.uint32))
    same_within(gal.within(probes, t, 0, max_hits=8), w70)
    gal.update(rows[G0:])
    _same(_run(gal, t, 0), want1)                                              # a larger G on the same handle
    same_within(gal.within(probes, t, 0, max_hits=8), fresh(rows, lambda g: g.within(probes, t, 0, max_hits=8)))
    a, b = gal.cluster(t, 0), gal.cluster(t, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _same(_run(gal, t, 0, first_row=G0, labels=torch.from_numpy(want0[0]).cuda()), want1)
    gal.close()


# ------------------------------------------------------------------------------------------- 6
def test_cluster_oneshot_and_frame_faces(cuda):
    from deep_insight_face import oneshot
    from deep_insight_face.detector.faces import FrameFaces
    G, D = 129, 128
    rows, lower = _rows(G, D), _lower(G, D, 1)
    (t,) = _gap_t(cr.pair_values(lower))
    want = cr.cluster_from(lower, G, t)
    lab, n = oneshot.cluster(rows, t)                                          # metric 1 is the default
    _same((lab.cpu().numpy(), int(n)), want)
    lab, n = oneshot.cluster(torch.from_numpy(rows).cuda(), t, 1)
    _same((lab.cpu().numpy(), int(n)), want)

    def faces(emb):
        m = emb.shape[0]
        z = torch.zeros
        return FrameFaces(offsets=torch.tensor([0, m]), frame=z(m, dtype=torch.int64), boxes=z((m, 4)), scores=z(m), landmarks=None,
                          crops=z((m, 8, 8, 3), dtype=torch.uint8), emb=emb)

    got = faces(torch.from_numpy(rows).cuda()).cluster(t)
    assert got.is_cuda and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want[0])
    want0 = cr.cluster_from(_lower(G, D, 0), G, _gap_t(cr.pair_values(_lower(G, D, 0)))[0])
    got = faces(torch.from_numpy(rows).cuda()).cluster(_gap_t(cr.pair_values(_lower(G, D, 0)))[0], distance_metric=0)
    assert np.array_equal(got.cpu().numpy(), want0[0])
    none = faces(torch.zeros((0, D), device='cuda')).cluster(t)                # M == 0: an empty tensor
    assert none.shape == (0,) and none.dtype == torch.int64
    with pytest.raises(ValueError):
        faces(torch.zeros((0, D), device='cuda'))._replace(emb=None).cluster(t)
    empty = oneshot.Gallery(emd_size=D)                                        # an empty gallery: no labels, no clusters
    lab, n = empty.cluster(0.5)
    assert lab.shape == (0,) and int(n) == 0
    empty.close()


# ------------------------------------------------------------------------------------------- 7
def test_cluster_arguments(cuda):
    from deep_insight_face import oneshot
    with pytest.raises(ValueError, match='multiple of 32'):
        oneshot.Gallery(np.zeros((4, 48), dtype=np.float32))                   # the census' own condition, at creation
    G, D = 129, 32
    gal = oneshot.Gallery(_rows(G, D))
    with pytest.raises(RuntimeError, match='Undefined distance metric 7'):
        gal.cluster(0.5, 7)
    with pytest.raises(ValueError):
        gal.cluster(float('nan'))
    for bad in (-1, G + 1):
        with pytest.raises(ValueError, match='first_row'):
            gal.cluster(0.5, 1, first_row=bad, labels=np.zeros(G + 1, dtype=np.int64))
    with pytest.raises(ValueError):
        gal.cluster(0.5, 1, first_row=5)                                       # the earlier labels are missing
    with pytest.raises(ValueError):
        gal.set_option('cluster_round', 100)                                   # not a multiple of 128
    lab = torch.empty(G, dtype=torch.int64, device='cuda')
    n = torch.empty((), dtype=torch.int64, device='cuda')
    gal.cluster_into(0.5, 1, lab, n)                                           # the well-formed call
    for kw in (dict(labels=lab[:-1]), dict(labels=lab.to(torch.int32)), dict(labels=lab.cpu()), dict(n_clusters=n.cpu()),
               dict(n_clusters=torch.empty(2, dtype=torch.int64, device='cuda')),
               dict(first_row=5, prev=lab[:4]), dict(first_row=5, prev=lab[:5].to(torch.int32))):
        a = dict(labels=lab, n_clusters=n, first_row=0, prev=None)
        a.update(kw)
        with pytest.raises(ValueError):
            gal.cluster_into(0.5, 1, a['labels'], a['n_clusters'], a['first_row'], a['prev'])
    # the library's own checks, below the Python layer
    from deep_insight_face import _native as N
    assert N.lib.dif_gallery_cluster(gal._h, 1, 0.5, G + 1, N.ptr(lab), N.ptr(lab), N.ptr(n), None) != 0
    assert b'first_row' in N.lib.dif_last_error()
    assert N.lib.dif_gallery_cluster(gal._h, 1, 0.5, 5, None, N.ptr(lab), N.ptr(n), None) != 0
    assert b'earlier labels' in N.lib.dif_last_error()
    gal.close()
