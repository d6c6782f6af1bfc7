"""tests/tagged_queries_ref.py -- the NumPy statement of the tagged range search and rank that tests/test_within_tagged_gpu.py,
tests/test_rank_tagged_gpu.py and tests/test_shard_tagged_queries_gpu.py compare against -- held to a brute-force loop over the
raw bits; the input conditions those GPU cases rely on asserted on the oracle alone; and the C ABI carries the four entry
points and the stat.  No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import rank_ref
import tagged_queries_ref as tq
import tagged_ref
from test_rank_gpu import _inputs, _near, _oracle
from test_within_gpu import _median_t, _sparse_t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 2e-6          # test_within_gpu.py
SHAPES = [(3, 129, 64), (65, 257, 512), (130, 1000, 128), (64, 4097, 512), (64, 4097, 128)]


def _bits(v):
    """The 64 raw bits of a Python int given as int64 or uint64."""
    return v & ((1 << 64) - 1)


def _brute_within(d, tags, mask, t, K, base=0):
    idx, dist, count = [], [], 0
    for r, x in enumerate(d):
        if (_bits(int(tags[r])) & _bits(int(mask))) == 0 or np.isnan(x) or not float(x) <= float(np.float32(t)):
            continue
        count += 1
        if len(idx) < K:
            idx.append(r + base)
            dist.append(x)
    pad = K - len(idx)
    return count, np.array(idx + [-1] * pad, dtype=np.int64), np.array(dist + [np.nan] * pad, dtype=np.float32)


def _brute_rank(d, tags, mask, m, base=0):
    k = int(m) - base
    if k < 0 or k >= len(d):
        return -1, np.float32(np.nan)
    if (_bits(int(tags[k])) & _bits(int(mask))) == 0 or np.isnan(d[k]):
        return len(d), np.float32(np.nan)
    rank = 0
    for r, x in enumerate(d):
        if (_bits(int(tags[r])) & _bits(int(mask))) == 0 or np.isnan(x):
            continue
        if float(x) < float(d[k]) or (float(x) == float(d[k]) and r < k):
            rank += 1
    return rank, np.float32(d[k])


def _same_f32(x, y):
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    return np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~np.isnan(x)].view(np.uint32), y[~np.isnan(y)].view(np.uint32))


def test_tagged_queries_against_a_brute_force_loop():
    rng = np.random.default_rng(12)
    top = -(1 << 63)
    for trial in range(30):
        G, n = int(rng.integers(1, 60)), 8
        d = rng.integers(0, 6, (n, G)).astype(np.float32) / 4                     # many exact ties
        d[rng.random((n, G)) < 0.15] = np.nan
        tags = tagged_ref.case_tags(G) if trial % 2 else rng.integers(-4, 4, G).astype(np.int64)
        if trial % 3 == 0:
            tags = tags.copy()
            tags[rng.integers(0, G)] = top                                        # bit 63 alone
        masks = tagged_ref.case_masks(n)
        for base in (0, 1000):
            mates = rng.integers(-1, G + 1, n).astype(np.int64) + base
            mates[0] = -1
            rank, md = tq.rank_full(d, mates, tags, masks, base)
            dist_in, owned = tq.mate_dist_full(d, mates, tags, masks, base)
            count_at = tq.rank_at_full(d, mates, dist_in, tags, masks, base)
            for p in range(n):
                want = _brute_rank(d[p], tags, masks[p], mates[p], base)
                assert rank[p] == want[0] and _same_f32(md[p], want[1]), (trial, p)
                assert owned[p] == (1 if base <= mates[p] < base + G else 0)
                assert _same_f32(dist_in[p], want[1])
                # the two halves add up to the rank (one shard: the count is the rank, or G behind a NaN distance)
                assert count_at[p] == (want[0] if owned[p] else G), (trial, p)
            for t in (0.0, 0.5, 1.25):
                for K in (0, 3, G):
                    cnt, idx, dist = tq.within_full(d, tags, masks, t, K, base)
                    assert idx.shape == (n, K) and dist.shape == (n, K)
                    for p in range(n):
                        want = _brute_within(d[p], tags, masks[p], t, K, base)
                        assert cnt[p] == want[0] and np.array_equal(idx[p], want[1]) and _same_f32(dist[p], want[2])
        cnt, idx, dist = tq.within_full(d, tags, masks, 9.0, 4)
        assert cnt[5] == 0 and (idx[5] == -1).all() and np.isnan(dist[5]).all()      # mask 0: count 0, all padding
    # an ineligible row exactly at the tolerance is not a hit; foreign rows before the first permitted one take no slot
    d = np.array([[0.25, 0.25, 0.5, 0.25, 0.125]], dtype=np.float32)
    cnt, idx, _ = tq.within_full(d, np.array([2, 2, 1, 1, 0]), np.array([1]), 0.25, 1)
    assert cnt[0] == 1 and idx[0].tolist() == [3]
    # an ineligible copy of the mate at a lower row does not count; an ineligible mate is behind every row, not unmated
    r, md = tq.rank_full(d, np.array([3]), np.array([2, 2, 1, 1, 0]), np.array([1]))
    assert r[0] == 0 and md[0] == np.float32(0.25)
    assert rank_ref.rank_full(d, np.array([3]))[0][0] == 3
    r, md = tq.rank_full(d, np.array([0]), np.array([2, 2, 1, 1, 0]), np.array([1]))
    assert r[0] == 5 and np.isnan(md[0])
    assert tq.rank_full(d, np.array([-1]), np.array([2, 2, 1, 1, 0]), np.array([1]))[0][0] == -1
    # every pair eligible: the untagged answers
    full = rng.random((4, 9)).astype(np.float32)
    every, ones = np.full(9, -1), np.full(4, -1)
    m = np.array([0, 8, -1, 4])
    got, want = tq.rank_full(full, m, every, ones), rank_ref.rank_full(full, m)
    assert np.array_equal(got[0], want[0]) and _same_f32(got[1], want[1])
    cnt, idx, _ = tq.within_full(full, every, ones, 0.5, 9)
    for p in range(4):
        assert np.array_equal(idx[p, :cnt[p]], np.flatnonzero(full[p] <= np.float32(0.5)))


def test_case_mates_follow_the_rule():
    B, G, D = 130, 1000, 128
    pick = _inputs(B, G, D)[2]
    tags, masks = tagged_ref.case_tags(G), tagged_ref.case_masks(B)
    el = tagged_ref.eligible(tags, masks)
    mates = tq.case_mates(B, G, pick, tags, masks)
    nid = G // 4
    assert np.array_equal(mates, tq.case_mates(B, G, pick, tags, masks))
    for b in range(B):
        own = np.arange(pick[b], G, nid)
        if b % 4 == 0:
            assert el[b, mates[b]]                                              # masks 1 and bit 63: rows to choose from
        elif b % 4 == 1:
            ok = own[el[b, own]]
            assert mates[b] == (ok[-1] if len(ok) else own[0])
        elif b % 4 == 2:
            assert mates[b] == own[0]
        elif b % 8 == 3:
            assert mates[b] == -1
        else:
            assert mates[b] == own[-1]


@pytest.mark.parametrize('B,G,D', SHAPES)
def test_conditions_of_the_tagged_gpu_cases(B, G, D):
    """What tests/test_within_tagged_gpu.py and tests/test_rank_tagged_gpu.py rely on, on the oracle alone.  The bounds sit a
    small margin inside what these inputs give (in brackets: the range over the five shapes and both metrics)."""
    probes, gal, pick = _inputs(B, G, D)
    tags, masks = tagged_ref.case_tags(G), tagged_ref.case_masks(B)
    el = tagged_ref.eligible(tags, masks)
    mates = tq.case_mates(B, G, pick, tags, masks)
    for metric in (0, 1):
        full = _oracle(B, G, D, metric)
        assert not np.isnan(full).any()
        # the widest-gap tolerance: no pair anywhere near it, nothing left out [gap 0.355 .. 0.427 / 84.8 .. 828]
        t, gap = _sparse_t(full)
        assert gap >= 1e-3, gap
        untagged = (full <= t).sum(1)
        cnt = tq.within_full(full, tags, masks, t, 8)[0]
        assert (untagged != cnt).mean() >= 0.9, (untagged != cnt).mean()         # the tags matter [0.92 .. 1.00]
        assert cnt.max() <= 8 and (cnt[masks == 0] == 0).all() and (cnt[masks == 8] == 0).all()
        # the mates: every kind of answer occurs
        want_r, want_d = tq.rank_full(full, mates, tags, masks)
        plain_r, _ = rank_ref.rank_full(full, mates)
        mate_el = np.array([mates[b] >= 0 and el[b, mates[b]] for b in range(B)])
        assert 0.30 <= mate_el.mean() <= 0.47, mate_el.mean()                    # [0.33 .. 0.44]
        assert 0.40 <= (want_r == G).mean() <= 0.70, (want_r == G).mean()        # an ineligible mate [0.44 .. 0.67]
        unmated = (want_r == -1).mean()
        assert unmated == 0 if B == 3 else 0.11 <= unmated <= 0.13, unmated      # [0.123 .. 0.125]
        assert (plain_r != want_r).mean() >= 0.75, (plain_r != want_r).mean()    # [0.77 .. 1.00]
        if G >= 1000:
            # a quarter of the probes has a random mate among about G / 2 eligible rows: 0.25 (1 - 256 / G) >= 0.186 expected
            mid = ((want_r > 128) & (want_r < G)).mean()
            assert mid >= 0.18, mid                                              # more than one tile of closer rows [0.19 .. 0.25]
        assert np.array_equal(np.isnan(want_d), ~mate_el)
    full = _oracle(B, G, D, 1)
    fm = tagged_ref.masked(full, tags, masks)
    # the dense case: the eligible pairs within NEAR of the median tolerance are the only ones a test may leave out
    near = (np.abs(full.astype(np.float64) - float(_median_t(full))) <= NEAR) & el
    assert near.sum() <= 2e-4 * el.sum(), near.sum() / el.sum()                  # [0 .. 1.2e-4]
    # rank ties: probes with no eligible row within NEAR of the mate's distance compare exactly
    assert (_near(fm, mates) == 0).mean() >= 0.9                                 # [0.969 .. 1.0]


def test_the_c_abi_carries_the_tagged_queries():
    """Fails on a library without the feature: the four entry points declared, exported, bound and documented, the stat named
    by the header, known to the library and in Gallery.stat's docstring, the keywords on every Python form."""
    header = open(os.path.join(ROOT, 'include', 'dif.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    path = os.path.join(ROOT, 'deep-insight-face_amd', 'lib', 'libdif.so')
    lib = ctypes.CDLL(path)
    from deep_insight_face import _native, oneshot, parallel
    from deep_insight_face.evaluation import identification
    nargs = {'dif_match_within_tagged': 12, 'dif_match_rank_tagged': 10, 'dif_match_mate_dist_tagged': 10,
             'dif_match_rank_at_tagged': 10}
    doc = re.sub(r'\s+', ' ', header[header.index('watch-lists on the range search'):])
    for fn, n in nargs.items():
        assert re.search(r'\bint\s+%s\s*\(' % fn, code), fn
        assert hasattr(lib, fn), fn
        assert fn in _native.SIGNATURES and len(_native.SIGNATURES[fn][1]) == n, fn
        assert fn + ':' in doc, fn                                               # documented, not only declared
    assert '#define DIF_VERSION 110' in re.sub(r'[ \t]+', ' ', header)
    assert '"within_tagged_tiles"' in header[header.index('read-outs'):header.index('int dif_gallery_get_stat(')]
    assert b'within_tagged_tiles\x00' in open(path, 'rb').read()                 # the key the library compares against
    assert 'within_tagged_tiles' in oneshot.Gallery.stat.__doc__
    G = oneshot.Gallery
    for f in (G.within, G.within_into, G.rank, G.rank_into, G.mate_dist_into, G.rank_at_into, oneshot.within, oneshot.rank,
              parallel.ShardedGallery.within, parallel.ShardedGallery.rank, identification.evaluate_identification):
        names = list(inspect.signature(f).parameters)
        assert names[-2:] == ['row_tags', 'probe_masks'], (f, names)
        assert inspect.signature(f).parameters['row_tags'].default is None
        assert inspect.signature(f).parameters['probe_masks'].default is None
