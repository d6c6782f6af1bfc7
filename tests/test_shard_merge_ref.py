"""tests/shard_merge_ref.py -- the NumPy statements of the sharded-gallery merges and of the shard-local rank count that
tests/test_shard_queries_gpu.py holds the device against -- checked against the whole-gallery NumPy references (topk_ref,
topk_ids_ref, rank_ref, shard_merge_ref.within_full) on random and tie-laden distances: every split of a small gallery into 2,
3 and 8 ragged shards, empty shards among them, equal distances in different shards, shards out of rank order and shards that
are not contiguous.  This is the proof of the two merge arguments -- identities, rank ties -- without a kernel.  Then the C
ABI: the new entry points declared, bound and exported.  No GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import rank_ref
import shard_merge_ref as sm
import topk_ids_ref
import topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dif_shard_merge_topk', 'dif_shard_merge_topk_ids', 'dif_shard_merge_within', 'dif_shard_merge_rank',
       'dif_match_mate_dist', 'dif_match_rank_at')


def _bits(a, b):
    """Equal arrays; float32 ones bit for bit, every NaN taken as one value."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32),
                                                                       b[~np.isnan(b)].view(np.uint32))


def _same(got, want):
    return len(got) == len(want) and all(_bits(g, w) for g, w in zip(got, want))


def _splits(G, R):
    """Every way to cut rows [0, G) into R contiguous shards in rank order, empty ones included."""
    for cuts in itertools.combinations_with_replacement(range(G + 1), R - 1):
        edges = (0,) + cuts + (G,)
        yield [(edges[i], edges[i + 1]) for i in range(R)]


def _tie_laden(B, G, seed):
    rng = np.random.default_rng(seed)
    full = (rng.integers(0, 4, (B, G)) / 4).astype(np.float32)          # many exact ties, 0 among them
    full[rng.random((B, G)) < 0.15] = np.nan
    full[rng.random((B, G)) < 0.05] = np.inf
    labels = rng.integers(-1, 4, G).astype(np.int64)
    return full, labels


def _check_split(full, labels, bounds, ks=(1, 2, 3, 9), exclude=None, tol=(0.25, -1.0, 2.0), Ks=(0, 2, 9)):
    """All four merges over the contiguous shards `bounds` (any order) against the whole-gallery references."""
    B, G = full.shape
    for k in ks:
        parts = [topk_ref.topk_full(full[:, lo:hi], k, lo) for lo, hi in bounds]
        got = sm.merge_topk(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
        assert _same(got, topk_ref.topk_full(full, k)), (bounds, k)
        for ex in (None, exclude):
            parts = [topk_ids_ref.topk_ids_full(full[:, lo:hi], labels[lo:hi], k, ex, lo) for lo, hi in bounds]
            got = sm.merge_topk_ids(*[np.stack([p[i] for p in parts]) for i in range(3)])
            assert _same(got, topk_ids_ref.topk_ids_full(full, labels, k, ex)), (bounds, k, ex is None)
    for t in tol:
        for K in Ks:
            parts = [sm.within_full(full[:, lo:hi], t, K, lo) for lo, hi in bounds]
            got = sm.merge_within(*[np.stack([p[i] for p in parts]) for i in range(3)])
            assert _same(got, sm.within_full(full, t, K)), (bounds, t, K)
    for mates in (np.arange(B) % max(G, 1), np.full(B, -1), np.full(B, G), np.full(B, G - 1), np.zeros(B, dtype=np.int64)):
        mates = mates.astype(np.int64)
        assert _same(sm.sharded_rank_full(full, bounds, mates), rank_ref.rank_full(full, mates)), (bounds, mates)


@pytest.mark.parametrize('R,G', [(2, 6), (3, 6), (8, 5)])
def test_every_split_of_a_small_gallery(R, G):
    """Every cut into R ragged shards (5 rows over 8 ranks: at least three are empty), tie-laden distances with NaN and inf,
    labels with repeats and negatives: every merge equals the whole-gallery reference bit for bit."""
    full, labels = _tie_laden(3, G, seed=10 * R + G)
    exclude = np.array([0, -1, 2], dtype=np.int64)
    n = 0
    for bounds in _splits(G, R):
        if R == 8:                                                      # 792 splits: two probes, the parameters that cut lists
            _check_split(full[:2], labels, bounds, ks=(2, 9), exclude=exclude[:2], tol=(0.25,), Ks=(0, 2))
        else:
            _check_split(full, labels, bounds, exclude=exclude)
        n += 1
    assert n == {(2, 6): 7, (3, 6): 28, (8, 5): 792}[(R, G)]


@pytest.mark.parametrize('seed', range(4))
def test_random_galleries_shards_in_any_order(seed):
    """Larger random galleries (ties, NaN, inf; several rows per identity spanning shards, a label in every shard), ragged
    shards handed to the merges in a shuffled order: nothing depends on the rank order."""
    rng = np.random.default_rng(100 + seed)
    B, G = 4, int(rng.integers(20, 60))
    full, labels = _tie_laden(B, G, seed)
    labels[::3] = 1                                                     # one identity present in every shard
    for R in (1, 2, 3, 8):
        cuts = np.sort(rng.integers(0, G + 1, R - 1))
        edges = [0] + [int(c) for c in cuts] + [G]
        bounds = [(edges[i], edges[i + 1]) for i in range(R)]
        _check_split(full, labels, bounds, ks=(1, 5, G + 2), exclude=rng.integers(-1, 4, B), Ks=(0, 4, G + 2))
        _check_split(full, labels, [bounds[i] for i in rng.permutation(R)], ks=(5,), exclude=None, Ks=(4,))


def test_shards_that_are_not_contiguous():
    """Rows dealt to the shards at random (a shard's global indices interleave with the others'): the list merges still give
    the whole-gallery lists.  (A device shard is contiguous -- index_base -- but the merges do not rely on it.)"""
    rng = np.random.default_rng(7)
    B, G, R = 3, 40, 4
    full, labels = _tie_laden(B, G, 3)
    owner = rng.integers(0, R, G)
    for k in (1, 4, 50):
        ti, td, ii, idd, il, wc, wi, wd = [], [], [], [], [], [], [], []
        for r in range(R):
            rows = np.flatnonzero(owner == r)

            def glob(idx):
                return np.where(idx >= 0, rows[np.maximum(idx, 0)] if rows.size else -1, -1).astype(np.int64)
            a = topk_ref.topk_full(full[:, rows], k)
            ti.append(glob(a[0])), td.append(a[1])
            a = topk_ids_ref.topk_ids_full(full[:, rows], labels[rows], k)
            ii.append(glob(a[0])), idd.append(a[1]), il.append(a[2])
            a = sm.within_full(full[:, rows], 0.5, k)
            wc.append(a[0]), wi.append(glob(a[1])), wd.append(a[2])
        assert _same(sm.merge_topk(np.stack(ti), np.stack(td)), topk_ref.topk_full(full, k))
        assert _same(sm.merge_topk_ids(np.stack(ii), np.stack(idd), np.stack(il)), topk_ids_ref.topk_ids_full(full, labels, k))
        assert _same(sm.merge_within(np.stack(wc), np.stack(wi), np.stack(wd)), sm.within_full(full, 0.5, k))


def test_hand_made_cases():
    nan = np.float32(np.nan)
    # the same distance in two shards: the lower GLOBAL row first, whichever rank holds it
    idx = np.array([[[7, 9]], [[2, 8]]], dtype=np.int64)
    dist = np.array([[[0.5, 0.5]], [[0.5, 0.75]]], dtype=np.float32)
    assert sm.merge_topk(idx, dist)[0].tolist() == [[2, 7]]
    # a padding slot is padding whatever its distance says; an all-padding shard (an empty one) adds nothing
    idx = np.array([[[4, -1, -1]], [[-1, -1, -1]], [[1, 6, -1]]], dtype=np.int64)
    dist = np.array([[[0.25, 0.0, nan]], [[nan, nan, nan]], [[0.25, 0.5, nan]]], dtype=np.float32)
    oi, od = sm.merge_topk(idx, dist)
    assert oi.tolist() == [[1, 4, 6]] and od.tolist() == [[0.25, 0.25, 0.5]]
    # identities: label 3's best row is in shard 1; shard 0's entry of label 3 is struck, label 5 moves up
    idx = np.array([[[10, 11]], [[20, 21]]], dtype=np.int64)
    dist = np.array([[[0.3, 0.4]], [[0.1, 0.35]]], dtype=np.float32)
    lab = np.array([[[3, 5]], [[3, 9]]], dtype=np.int64)
    oi, od, ol = sm.merge_topk_ids(idx, dist, lab)
    assert oi.tolist() == [[20, 21]] and ol.tolist() == [[3, 9]]
    oi, od, ol = sm.merge_topk_ids(np.concatenate([idx, np.full((1, 1, 2), -1)]), np.concatenate([dist, np.full((1, 1, 2), nan)]),
                                   np.concatenate([lab, np.full((1, 1, 2), -1)]))
    assert oi.tolist() == [[20, 21]] and ol.tolist() == [[3, 9]]
    # within: counts add although the lists are cut; the K lowest global rows whatever the rank order
    cnt, oi, od = sm.merge_within(np.array([[5], [1]]), np.array([[[30, 31]], [[4, -1]]]),
                                  np.array([[[0.1, 0.2]], [[0.3, nan]]], dtype=np.float32))
    assert cnt.tolist() == [6] and oi.tolist() == [[4, 30]] and od.tolist() == [[np.float32(0.3), np.float32(0.1)]]
    # rank: no owner -> -1 / NaN; two owners (overlapping shards, not allowed): the lowest rank's distance
    rank, md = sm.merge_rank(np.array([[1, 2, 3], [4, 5, 6]]), np.array([[0, 0, 1], [0, 1, 1]]),
                             np.array([[nan, nan, 0.5], [nan, 0.25, 0.75]], dtype=np.float32))
    assert rank.tolist() == [-1, 7, 9] and np.isnan(md[0]) and md[1] == 0.25 and md[2] == 0.5
    # rank_at: ties count by GLOBAL row against a mate below, inside and above the shard; NaN is never closer; dm NaN: the size
    d = np.array([0.5, 0.25, nan, 0.5, 0.75], dtype=np.float32)
    assert sm.rank_at_row(d, 3, np.float32(0.5), index_base=100) == 1           # mate below the shard: no tie counts
    assert sm.rank_at_row(d, 103, np.float32(0.5), index_base=100) == 2         # row 100 ties from below the mate
    assert sm.rank_at_row(d, 10 ** 12, np.float32(0.5), index_base=100) == 3    # mate above the shard: both ties count
    assert sm.rank_at_row(d, 103, nan, index_base=100) == 5
    assert sm.rank_at_row(d[:0], 103, np.float32(0.5), index_base=100) == 0
    for m in (99, 105, -1):
        md, own = sm.mate_dist_row(d, m, 100)
        assert np.isnan(md) and own == 0
    assert sm.mate_dist_row(d, 101, 100) == (np.float32(0.25), 1) and sm.mate_dist_row(d, 102, 100)[1] == 1


def test_the_c_abi_carries_the_shard_entries():
    """Fails on a library without the feature: the entries declared in the header, bound in _native.SIGNATURES, exported by the
    built library, and the Python callables in place."""
    header = open(os.path.join(ROOT, 'include', 'dif.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    assert re.search(r'#define DIF_SHARD_MAX 64\b', header) and re.search(r'#define DIF_VERSION 110\b', header)
    lib = ctypes.CDLL(os.path.join(ROOT, 'deep-insight-face_amd', 'lib', 'libdif.so'))
    assert not [n for n in NEW if not hasattr(lib, n)]
    from deep_insight_face import _native, oneshot, parallel
    nargs = {'dif_shard_merge_topk': 8, 'dif_shard_merge_topk_ids': 10, 'dif_shard_merge_within': 10, 'dif_shard_merge_rank': 8,
             'dif_match_mate_dist': 8, 'dif_match_rank_at': 8}
    for name in NEW:
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs[name], name
    for fn in ('merge_topk', 'merge_topk_ids', 'merge_within', 'merge_rank', 'within_gather_bytes'):
        assert callable(getattr(parallel, fn)), fn
    for m in ('topk', 'topk_ids', 'within', 'rank', 'roc'):
        assert callable(getattr(parallel.ShardedGallery, m)), m
    assert callable(oneshot.Gallery.mate_dist_into) and callable(oneshot.Gallery.rank_at_into)
    # argument errors need no device: they are refused before anything is launched
    lib.dif_last_error.restype = ctypes.c_char_p
    one = ctypes.c_void_p(8)                                            # never dereferenced: the sizes are refused first
    for R in (0, -1, 65):
        assert lib.dif_shard_merge_topk(one, one, R, 1, 1, one, one, None) != 0 and b'outside [1, 64]' in lib.dif_last_error()
        assert lib.dif_shard_merge_topk_ids(one, one, one, R, 1, 1, one, one, one, None) != 0
        assert lib.dif_shard_merge_within(one, one, one, R, 1, 1, one, one, one, None) != 0
        assert lib.dif_shard_merge_rank(one, one, one, R, 1, one, one, None) != 0
    for k in (0, 129):
        assert lib.dif_shard_merge_topk(one, one, 2, 1, k, one, one, None) != 0 and b'outside [1, 128]' in lib.dif_last_error()
        assert lib.dif_shard_merge_topk_ids(one, one, one, 2, 1, k, one, one, one, None) != 0
    for K in (-1, 8193):
        assert lib.dif_shard_merge_within(one, one, one, 2, 1, K, one, one, one, None) != 0
        assert b'outside [0, 8192]' in lib.dif_last_error()
    assert lib.dif_shard_merge_topk(None, one, 2, 1, 1, one, one, None) != 0 and b'null pointer' in lib.dif_last_error()
    assert lib.dif_shard_merge_topk_ids(one, one, None, 2, 1, 1, one, one, one, None) != 0
    assert lib.dif_shard_merge_within(one, None, one, 2, 1, 1, one, one, one, None) != 0
    assert lib.dif_shard_merge_within(None, None, None, 2, 1, 0, one, None, None, None) != 0
    assert lib.dif_shard_merge_rank(one, None, one, 2, 1, one, one, None) != 0
    assert lib.dif_shard_merge_topk(one, one, 2, -1, 1, one, one, None) != 0
    for fn in (lib.dif_shard_merge_topk,):
        assert fn(None, None, 2, 0, 1, None, None, None) == 0           # n = 0: a no-op
    assert lib.dif_match_mate_dist(None, one, 1, 0, one, one, one, None) != 0 and b'null handle' in lib.dif_last_error()
    assert lib.dif_match_rank_at(None, one, 1, 0, one, one, one, None) != 0 and b'null handle' in lib.dif_last_error()
    assert parallel.within_gather_bytes(8, 512, 64) == 8 * 8 * 512 * 64 * 12


def test_record_pack_unpack_round_trip():
    """parallel._pack / _unpack, the record one all-gather moves: int64 and float32 parts of any size -- odd lengths, empty
    lists (max_hits = 0), a world of one -- come back as dense [R, ...] tensors with their bits."""
    import torch
    from deep_insight_face import parallel
    rng = np.random.default_rng(0)
    for R in (1, 2, 3):
        for B, K in ((1, 1), (3, 5), (37, 0), (5, 4), (0, 3)):
            recs, parts = [], []
            for r in range(R):
                cnt = torch.from_numpy(rng.integers(-5, 1 << 40, (B,)))
                idx = torch.from_numpy(rng.integers(-1, 1 << 40, (B, K)))
                d = torch.from_numpy(rng.random((B, K)).astype(np.float32))
                parts.append((cnt, idx, d))
                recs.append(parallel._pack([cnt, idx, d]))
                assert recs[-1].dtype == torch.float32 and recs[-1].shape == (2 * B + 3 * B * K,)
            got = parallel._unpack(torch.stack(recs), [(torch.int64, (B,)), (torch.int64, (B, K)), (torch.float32, (B, K))])
            for i in range(3):
                want = torch.stack([p[i] for p in parts])
                assert got[i].dtype == want.dtype and got[i].shape == want.shape and torch.equal(got[i], want)
                assert got[i].is_contiguous()
