"""What tests/test_embed_dims_gpu.py asserts on the oracle alone before it asks the device, held here without a GPU: at every
shape of embed_dims.QUERY_SHAPES the oracle has no NaN distance, the tolerances sit in gaps wide enough for metric 1 and the
shares of positions that compare exactly stay above the caps of each query's own test file.  (The top-k caps are in
test_topk_ref.py and test_topk_ids_ref.py, whose shape lists carry these shapes too.)"""
import functools

import numpy as np
import pytest

import cluster_ref as cr
import embed_dims as ed
import rank_ref
import test_cluster_gpu as cl
import test_rank_gpu as rk
import test_topk_ref as tr
import test_within_gpu as wi


@functools.lru_cache(maxsize=None)
def _full(B, G, D, metric):
    probes, gal, _ = tr._inputs(B, G, D)
    return rank_ref.distances(probes, gal, metric)


def test_the_gpu_tests_draw_the_same_rows():
    import test_topk_gpu as tk
    for shape in ed.QUERY_SHAPES[:2]:
        for a, b in zip(tr._inputs(*shape), tk._inputs(*shape)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('B,G,D', ed.QUERY_SHAPES)
def test_caps_of_the_query_shapes(B, G, D, metric):
    full = _full(B, G, D, metric)
    assert not np.isnan(full).any()
    # within: a few hits per probe inside the widest gap; at the median at most 1 % of the pairs within NEAR of it
    t, gap = wi._sparse_t(full)
    assert gap >= 1e-3, gap
    few = wi._expect(full, t, 64)[0]
    assert 1 <= few.min() and few.max() <= 8
    near = np.abs(full.astype(np.float64) - float(wi._median_t(full))) <= wi.NEAR
    assert near.mean() <= 0.01, near.mean()
    # rank: the mate among its identity's few rows, at least half of the probes clear
    pick = tr._inputs(B, G, D)[2]
    mates = (pick + max(1, G // 4) * (np.arange(B) % 4)).astype(np.int64)
    assert mates.max() < G and (rank_ref.rank_full(full, mates)[0] <= 4).all()
    assert (rk._near(full, mates) == 0).mean() >= 0.5
    # match: the arg-min is the probe's identity and no stranger is anywhere near
    assert np.array_equal(np.argmin(full, axis=1) % max(1, G // 4), pick)


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('B,G,D', ed.QUERY_SHAPES)
def test_cluster_gap_of_the_query_shapes(B, G, D, metric):
    """cluster / dbscan on the first min(G, 515) rows: the widest gap of the pairwise distances exceeds test_cluster_gpu.py's
    MIN_GAP (_gap_t asserts it) and the components at its midpoint are the identities."""
    rows = tr._inputs(B, G, D)[1][:min(G, 515)]
    lower = cr.lower_distances(rows, metric)
    (t,) = cl._gap_t(cr.pair_values(lower))
    assert cr.cluster_from(lower, rows.shape[0], t)[1] == min(rows.shape[0], max(1, G // 4))
