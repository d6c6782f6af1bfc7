"""The CPU oracle of Gallery.cluster (tests/cluster_ref.py) against a brute-force transitive closure, and its edge cases."""
import numpy as np
import pytest

import cluster_ref as cr
from oracle import distance as od


def _closure_labels(rows, t, metric):
    """Boolean adjacency from the full distance matrix (the lower triangle's definition, mirrored), squared until it stops
    changing; label = the smallest row reachable."""
    G = rows.shape[0]
    with np.errstate(all='ignore'):
        full = np.stack([od.distance(q[None, :], rows, metric) for q in rows])
        low = np.tril(full <= np.float32(t), -1)
    reach = low | low.T | np.eye(G, dtype=bool)
    while True:
        nxt = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
        if np.array_equal(nxt, reach):
            break
        reach = nxt
    labels = np.argmax(reach, axis=1).astype(np.int64)        # the first True of a row: the smallest row reachable
    return labels, len(np.unique(labels))


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('G,D,seed', [(1, 32, 0), (2, 32, 1), (17, 32, 2), (64, 32, 3), (64, 64, 4)])
def test_oracle_equals_bruteforce_closure(G, D, seed, metric):
    rng = np.random.default_rng(seed)
    nid = max(1, G // 4)
    centres = rng.standard_normal((nid, D))
    rows = (centres[rng.permutation(G) % nid] + 0.3 * rng.standard_normal((G, D))).astype(np.float32)
    vals = cr.pair_values(cr.lower_distances(rows, metric))
    # tolerances that give singletons, a partial clustering with chains, and one component
    for t in ([0.5] if vals.size == 0 else list(np.quantile(vals, [0.0, 0.02, 0.05, 0.1, 0.3, 1.0]).astype(np.float32)) + [-1.0]):
        want, n_want = _closure_labels(rows, t, metric)
        got, n_got = cr.cluster(rows, t, metric)
        assert got.dtype == np.int64 and np.array_equal(got, want) and n_got == n_want
    if G >= 17:
        counts = [cr.cluster(rows, t, metric)[1] for t in np.quantile(vals, [0.02, 0.05, 0.1]).astype(np.float32)]
        assert any(1 < c < G for c in counts), counts           # the middle tolerances do exercise merging


def test_singletons_chain_and_nan_rows():
    e = np.zeros((6, 32), dtype=np.float32)
    e[:, 0] = [0.0, 1.0, 2.0, 3.0, 10.0, 4.0]                   # a chain 0-1-2-3-(row 5 at 4.0) and row 4 far away
    e[:, 1] = 1.0
    lab, n = cr.cluster(e, 1.0, 0)                               # squared distance of neighbours is exactly 1: inclusive
    assert list(lab) == [0, 0, 0, 0, 4, 0] and n == 2
    lab, n = cr.cluster(e, np.nextafter(np.float32(1), np.float32(0)), 0)
    assert list(lab) == list(range(6)) and n == 6
    lab, n = cr.cluster(e, -1.0, 0)
    assert list(lab) == list(range(6)) and n == 6
    lab, n = cr.cluster(e, 1.0, 0, index_base=100)
    assert list(lab) == [100, 100, 100, 100, 104, 100] and n == 2
    # a NaN row and a zero-norm row are alone under metric 1 whatever the tolerance; every other pair joins at t = 1
    f = np.abs(np.random.default_rng(5).standard_normal((5, 32))).astype(np.float32)
    f[1] = np.nan
    f[3] = 0
    lab, n = cr.cluster(f, 1.0, 1)
    assert list(lab) == [0, 1, 0, 3, 0] and n == 3
    lab, n = cr.cluster(np.zeros((0, 32), dtype=np.float32), 0.5, 1)
    assert lab.shape == (0,) and lab.dtype == np.int64 and n == 0


def test_incremental_equals_full():
    rng = np.random.default_rng(9)
    rows = (rng.standard_normal((8, 32))[np.arange(40) % 8] + 0.3 * rng.standard_normal((40, 32))).astype(np.float32)
    t = np.float32(np.quantile(cr.pair_values(cr.lower_distances(rows, 0)), 0.05))
    full = cr.cluster(rows, t, 0, index_base=7)
    for r in (0, 1, 23, 40):
        prev = cr.cluster(rows[:r], t, 0, index_base=7)[0]
        got = cr.cluster(rows, t, 0, index_base=7, first_row=r, labels=prev)
        assert np.array_equal(got[0], full[0]) and got[1] == full[1]
    assert 1 < full[1] < 40


def test_clamp_joins_identical_twins():
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((64, 512)).astype(np.float32)
    rows = np.concatenate([rows, rows])                          # row 64 + k is row k again
    with np.errstate(invalid='ignore'):
        sim = od.similarity(rows[:64], rows[64:])
    assert (sim > 1).any()                                      # some twins' similarity rounds above 1: NaN in the reference
    lab, n = cr.cluster(rows, 0.01, 1)
    assert n == 64 + int((sim > 1).sum()) and np.array_equal(lab[64:][sim > 1], 64 + np.flatnonzero(sim > 1))
    lab, n = cr.cluster(rows, 0.01, 1, clamp=True)
    assert n == 64 and np.array_equal(lab, np.arange(128) % 64)
