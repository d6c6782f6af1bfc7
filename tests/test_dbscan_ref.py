"""The CPU oracle of Gallery.dbscan (tests/dbscan_ref.py) against an independent brute force, and the consequences of the
definition that the GPU tests rely on.  No GPU."""
import math

import numpy as np
import pytest

import cluster_ref as cr
import dbscan_ref as dr
from oracle import distance as od


def _pair(rows, i, j, metric, clamp):
    """distance(rows[i][None, :], rows[j][None, :]): one pair, row i the probe."""
    q, g = rows[i][None, :], rows[j][None, :]
    with np.errstate(all='ignore'):
        if metric == 1 and clamp:
            return np.float32(np.arccos(np.clip(od.similarity(q, g), np.float32(-1), np.float32(1)))[0] / math.pi)
        return np.float32(od.distance(q, g, metric)[0])


def brute(rows, t, min_samples, metric, clamp=False, index_base=0):
    """The definition, with nothing shared with dbscan_ref: the full float32 matrix (row i the probe for j < i, mirrored), a
    Boolean closure over the core-core adjacency, borders by argmin over (distance, row)."""
    rows = np.asarray(rows, dtype=np.float32)
    G = rows.shape[0]
    dm = np.full((G, G), np.nan, dtype=np.float32)
    for i in range(G):
        for j in range(i):
            dm[i, j] = dm[j, i] = _pair(rows, i, j, metric, clamp)
    with np.errstate(invalid='ignore'):
        adj = dm <= np.float32(t)                                 # the diagonal is NaN: no self pair
    degree = 1 + adj.sum(axis=1)
    core = degree >= min_samples
    reach = (adj & core[:, None] & core[None, :]) | np.diag(core)
    while True:
        more = reach | ((reach.astype(np.int64) @ reach.astype(np.int64)) > 0)
        if np.array_equal(more, reach):
            break
        reach = more
    labels = np.full(G, -1, dtype=np.int64)
    for c in np.flatnonzero(core):
        labels[c] = index_base + int(np.flatnonzero(reach[c])[0])
    for b in np.flatnonzero(~core):
        cand = np.flatnonzero(adj[b] & core)
        if cand.size:
            a = cand[np.lexsort((cand, dm[b, cand]))[0]]          # smallest distance, then lowest row
            labels[b] = labels[a]
    n_clusters = len(set(labels[core].tolist()))
    return labels, degree.astype(np.int32), (n_clusters, int((labels == -1).sum()))


def _same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert tuple(got[2]) == tuple(want[2])
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32


def _blobs(G, D, seed):
    """Gaussian identities of unequal sizes and spreads: degrees of every size, chains and borders by chance."""
    rng = np.random.default_rng(seed)
    ident = rng.integers(0, max(1, G // 5), G)
    centres = rng.standard_normal((G, D))
    return (centres[ident] + 0.35 * rng.standard_normal((G, D))).astype(np.float32)


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('min_samples', [1, 2, 3, 4, 7])
def test_oracle_equals_brute_force(metric, min_samples):
    seen = np.zeros(3, dtype=np.int64)
    for rows in (dr.make_rows(64, 32, metric), _blobs(60, 8, 5), _blobs(33, 4, 6)):
        vals = np.sort(cr.pair_values(cr.lower_distances(rows, metric)))
        for t in (np.float32(sum(dr.EDGE[metric][1:] + dr.NEAR[metric][:1]) / 2), vals[len(vals) // 20], vals[len(vals) // 6]):
            for base in (0, 1000):
                got = dr.dbscan(rows, t, min_samples, metric, index_base=base)
                _same(got, brute(rows, t, min_samples, metric, index_base=base))
                seen += [k.sum() for k in dr.kinds(got[0], got[1], min_samples)]
    if min_samples >= 3:
        assert (seen > 0).all(), seen                             # core, border and noise rows were all compared


@pytest.mark.parametrize('metric', [0, 1])
def test_min_samples_one_is_cluster(metric):
    for rows in (dr.make_rows(64, 32, metric), _blobs(60, 8, 7)):
        lower = cr.lower_distances(rows, metric)
        vals = np.sort(cr.pair_values(lower))
        for t in (vals[3], vals[len(vals) // 10], vals[-1], np.float32(-1)):
            for base in (0, 77):
                labels, degree, counts = dr.dbscan_from(lower, len(rows), t, 1, index_base=base)
                want = cr.cluster_from(lower, len(rows), t, index_base=base)
                assert np.array_equal(labels, want[0]) and counts == (want[1], 0)


@pytest.mark.parametrize('metric', [0, 1])
def test_min_samples_above_the_row_count_and_negative_tolerance(metric):
    rows = _blobs(40, 8, 8)
    G = len(rows)
    labels, degree, counts = dr.dbscan(rows, 1e9 if metric == 0 else 1.0, G + 1, metric, index_base=5)
    assert (labels == -1).all() and counts == (0, G) and (degree == G).all()
    labels, degree, counts = dr.dbscan(rows, 1e9 if metric == 0 else 1.0, G, metric, index_base=5)
    assert (labels == 5).all() and counts == (1, 0)
    for ms, want in ((1, (np.arange(G) + 5, (G, 0))), (2, (np.full(G, -1), (0, G)))):
        labels, degree, counts = dr.dbscan(rows, -1.0, ms, metric, index_base=5)
        assert (degree == 1).all() and np.array_equal(labels, want[0]) and counts == want[1]


@pytest.mark.parametrize('clamp', [False, True])
def test_nan_and_zero_norm_rows_under_metric_1(clamp):
    """A zero-norm or NaN row has a NaN distance to everything, itself included: degree 1 all the same.  Identical twins whose
    similarity rounds above 1 have a NaN distance without the clamp, never with it."""
    rows = _blobs(48, 16, 9)
    rows[3] = 0
    rows[40] = 0
    rows[10] = np.nan
    rows[20, 5] = np.nan
    rows[30:36] = rows[12:18]                                     # twins
    lower = cr.lower_distances(rows, 1, clamp)
    vals = np.sort(cr.pair_values(lower))
    for t in (vals[len(vals) // 10], np.float32(0), np.float32(1)):
        for ms in (1, 2, 4):
            got = dr.dbscan_from(lower, len(rows), t, ms)
            _same(got, brute(rows, t, ms, 1, clamp))
            assert (got[1] >= 1).all() and (got[1][[3, 40, 10, 20]] == 1).all()
            if ms > 1:
                assert (got[0][[3, 40, 10, 20]] == -1).all()
            else:
                assert np.array_equal(got[0][[3, 40, 10, 20]], [3, 40, 10, 20])
    twins_nan = np.array([np.isnan(lower[r][r - 18]) for r in range(30, 36)])
    assert not (clamp and twins_nan.any())


@pytest.mark.parametrize('swap', [False, True])
def test_bridge_case(swap):
    """The row that fuses two people under single linkage is a border row here: two clusters, and on an exact tie it goes
    with whichever core has the lower row number."""
    rows, at = dr.bridge_rows(0.0, swap)
    lab, n = cr.cluster(rows, 1.0, 0)
    assert n == 2 and len(set(lab[[at['cA'], at['cB'], at['bridge']]].tolist())) == 1 and lab[at['far']] == at['far']
    labels, degree, counts = dr.dbscan(rows, 1.0, 4, 0)
    assert counts == (2, 1) and labels[at['far']] == -1
    assert degree[at['bridge']] == 3 and labels[at['cA']] != labels[at['cB']]
    assert labels[at['bridge']] == labels[at['cA'] if at['cA'] < at['cB'] else at['cB']]
    assert (labels[at['A']] == labels[at['cA']]).all() and (labels[at['B']] == labels[at['cB']]).all()
    _same((labels, degree, counts), brute(rows, 1.0, 4, 0))
    # nearer to A: A's cluster in both orders
    rows, at = dr.bridge_rows(-0.25, swap)
    labels, degree, counts = dr.dbscan(rows, 1.0, 4, 0)
    assert counts == (2, 1) and degree[at['bridge']] == 2 and labels[at['bridge']] == labels[at['cA']] != labels[at['cB']]
    _same((labels, degree, counts), brute(rows, 1.0, 4, 0))


def test_bridge_rows_put_the_tie_both_ways():
    a, b = dr.bridge_rows(0.0, False)[1], dr.bridge_rows(0.0, True)[1]
    assert (a['cA'] < a['cB']) != (b['cA'] < b['cB'])


@pytest.mark.parametrize('metric', [0, 1])
def test_against_sklearn(metric):
    """Core mask, the partition of the core rows and the noise set; sklearn's border rows depend on its visiting order."""
    sk = pytest.importorskip('sklearn.cluster')
    rows = _blobs(60, 8, 11)
    G = len(rows)
    dm = np.zeros((G, G), dtype=np.float64)
    for i in range(G):
        for j in range(i):
            dm[i, j] = dm[j, i] = _pair(rows, i, j, metric, False)
    assert np.isfinite(dm).all()
    vals = np.sort(cr.pair_values(cr.lower_distances(rows, metric)))
    for t in (vals[len(vals) // 20], vals[len(vals) // 6]):
        for ms in (2, 3, 5):
            labels, degree, counts = dr.dbscan(rows, t, ms, metric)
            fit = sk.DBSCAN(eps=float(np.float32(t)), min_samples=ms, metric='precomputed').fit(dm)
            core = np.zeros(G, dtype=bool)
            core[fit.core_sample_indices_] = True
            assert np.array_equal(core, degree >= ms)
            assert np.array_equal(fit.labels_ == -1, labels == -1)
            ours, theirs = labels[core], fit.labels_[core]
            assert np.array_equal(ours[:, None] == ours[None, :], theirs[:, None] == theirs[None, :])
