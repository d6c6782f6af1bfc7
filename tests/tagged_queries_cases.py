"""What tests/test_within_tagged_gpu.py, tests/test_rank_tagged_gpu.py and tests/test_shard_tagged_queries_gpu.py share: the
inputs (test_within_gpu.py's generator through test_rank_gpu.py, which also returns each probe's identity), the oracle's
distances, computed once per shape and left unchanged, tagged_ref's tags and masks, and the mates of tagged_queries_ref."""
import functools

import numpy as np

import rank_ref
import tagged_queries_ref as tq
import tagged_ref
from test_rank_gpu import _inputs, _oracle

SHAPES = [(3, 129, 64), (65, 257, 512), (130, 1000, 128), (64, 4097, 512), (64, 4097, 128)]
TOP = -(1 << 63)


def frozen(a):
    a = np.array(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(B, G, D):
    """-> (probes, gallery, pick, row_tags, probe_masks, mates)."""
    probes, gal, pick = _inputs(B, G, D)
    tags, masks = tagged_ref.case_tags(G), tagged_ref.case_masks(B)
    return probes, gal, pick, tags, masks, tq.case_mates(B, G, pick, tags, masks)


def oracle(B, G, D, metric):
    return _oracle(B, G, D, metric)


@functools.lru_cache(maxsize=None)
def masked(B, G, D, metric):
    _, _, _, tags, masks, _ = case(B, G, D)
    return frozen(tagged_ref.masked(_oracle(B, G, D, metric), tags, masks))


def round_masks(B):
    """tagged_ref.case_masks with every block of 128 probes one step further along the cycle: the cycle's period, 8, divides
    128, so under case_masks(B) itself probe 128 + j carries probe j's mask and a launch that dropped its `probe_masks + b0`
    would answer correctly."""
    i = np.arange(B)
    return frozen(tagged_ref.case_masks(B + B // 128 + 1)[i + i // 128])


def skip_case():
    """516 tiles; bit 2 on 100 rows of exactly two tiles (7 and 300); nine probes, the last one with |q|^2 below the range in
    which the census' bound holds (it resolves every tile it is not told to skip).  -> (probes [9, 32], gallery, tags)."""
    probes3, gal, _ = _inputs(3, 66000, 32)
    probes = np.concatenate([probes3, probes3[::-1] * np.float32(1.5), -probes3]).astype(np.float32)
    probes[8] = probes3[0] * np.float32(1e-16)
    assert float((probes[8].astype(np.float64) ** 2).sum()) < 1e-30               # NORM_LO of csrc/match_ref.hpp
    G = gal.shape[0]
    tags = np.ones(G, dtype=np.int64)
    tags[128 * 7:128 * 7 + 40] = 5
    tags[128 * 300 + 5:128 * 300 + 65] = 4
    assert (G + 127) // 128 == 516 and int(((tags & 4) != 0).sum()) == 100
    assert np.unique(np.flatnonzero(tags & 4) // 128).tolist() == [7, 300]
    return probes, gal, tags


def degenerate_tags(fulls, B):
    """tests/test_topk_tagged_gpu.py's rule: the odd rows -- those with a distance that is not finite to some ordinary probe --
    carry tag 2, the others tag 1; every second probe sees both kinds, the others the ordinary rows alone."""
    G = next(iter(fulls.values())).shape[1]
    odd = np.zeros(G, dtype=bool)
    for full in fulls.values():
        ordinary = np.isfinite(full).any(1)
        odd |= (~np.isfinite(full[ordinary])).any(0)
    return np.where(odd, 2, 1).astype(np.int64), np.where(np.arange(B) % 2 == 0, 3, 1).astype(np.int64)


def distances(probes, gal, metric):
    return rank_ref.distances(probes, gal, metric)
