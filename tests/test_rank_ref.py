"""tests/rank_ref.py -- the NumPy statement of the rank of the mate that the GPU tests compare against -- checked against
what it claims to restate: the mate's position in np.argsort(kind='stable') on rows without NaN, and the written rule
(NaN never closer, unmated -1, NaN mate G) on rows with NaN.  No GPU."""
import numpy as np

import golden_inputs as gi
import rank_ref


def _stable_pos(d, k):
    return int(np.flatnonzero(np.argsort(d, kind='stable') == k)[0])


def test_rank_is_the_stable_argsort_position():
    probes, gal = gi.match_tie_inputs()                        # exact duplicates: ties go to the lower index
    for metric in (0, 1):
        full = rank_ref.distances(probes, gal, metric)
        assert not np.isnan(full).any()
        for b in range(probes.shape[0]):
            order = np.argsort(full[b], kind='stable')
            for pos in list(range(6)) + [100, gal.shape[0] - 1]:
                r, dm = rank_ref.rank_row(full[b], order[pos])
                assert r == pos and dm == full[b, order[pos]]
    # duplicates really are met: the three copies of probe 0's row take positions 0, 1, 2 in index order
    full = rank_ref.distances(probes[:1], gal, 0)
    assert [rank_ref.rank_row(full[0], m)[0] for m in (100, 300, 500)] == [0, 1, 2]
    assert full[0, 100] == full[0, 300] == full[0, 500]


def test_rank_rules_with_nans_and_unmated():
    d = np.array([0.5, np.nan, 0.25, 0.5, np.nan, 0.75, 0.25], dtype=np.float32)
    assert rank_ref.rank_row(d, 2) == (0, np.float32(0.25))
    assert rank_ref.rank_row(d, 6) == (1, np.float32(0.25))    # the tie goes to the lower index
    assert rank_ref.rank_row(d, 0) == (2, np.float32(0.5))
    assert rank_ref.rank_row(d, 3) == (3, np.float32(0.5))
    assert rank_ref.rank_row(d, 5) == (4, np.float32(0.75))    # the NaN rows are never closer
    for m in (1, 4):                                           # the mate's own distance is NaN: behind every row
        r, dm = rank_ref.rank_row(d, m)
        assert r == 7 and np.isnan(dm)
    for m in (-1, -5, 7, 1 << 40):                             # unmated
        r, dm = rank_ref.rank_row(d, m)
        assert r == -1 and np.isnan(dm)
    # index_base shifts the mate, not the rule
    assert rank_ref.rank_row(d, 1006, index_base=1000) == (1, np.float32(0.25))
    assert rank_ref.rank_row(d, 6, index_base=1000)[0] == -1
    assert rank_ref.rank_row(d, 1007, index_base=1000)[0] == -1
    # against the argsort on the rows that are not NaN (a NaN sorts last in NumPy, so it never pushes a number back)
    fin = ~np.isnan(d)
    for m in np.flatnonzero(fin):
        assert rank_ref.rank_row(d, m)[0] == _stable_pos(d[fin], int(fin[:m].sum()))
    r, dm = rank_ref.rank_row(np.zeros(0, dtype=np.float32), 0)   # an empty gallery: everybody is unmated
    assert r == -1 and np.isnan(dm)


def test_rank_on_degenerate_rows():
    name, probes, gal = [c for c in gi.match_degenerate_cases() if c[0] == 'zero_rows'][0]
    full = rank_ref.distances(probes[:4], gal, 1)
    assert np.isnan(full[:, 417]).all()                        # a zero-norm row: 0 / 0
    rank, dist = rank_ref.rank_full(full, np.array([417, 0, -1, gal.shape[0]]))
    assert rank[0] == gal.shape[0] and np.isnan(dist[0])
    assert rank[1] == _stable_pos(np.where(np.isnan(full[1]), np.inf, full[1]), 0) and dist[1] == full[1, 0]
    assert rank[2] == -1 and rank[3] == -1 and np.isnan(dist[2:]).all()
    r2, d2 = rank_ref.rank(probes[:4], gal, np.array([417, 0, -1, gal.shape[0]]), 1)
    assert np.array_equal(r2, rank) and np.array_equal(np.isnan(d2), np.isnan(dist))
