"""tests/tagged_ref.py -- the NumPy statement of the tagged top-k searches that tests/test_topk_tagged_gpu.py and
tests/test_shard_tagged_gpu.py compare against -- held to a brute-force loop; the CLEAR-position caps of the GPU cases asserted
on the oracle alone, with the real bit 63; and the C ABI carries the two entry points and the stat.  No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import rank_ref
import tagged_ref
import topk_ids_ref
import topk_ref
from test_topk_ref import SHAPES, _inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 2e-6          # test_within_gpu.py
MIN_CLEAR = 0.9


def _bits(v):
    """The 64 raw bits of a Python int given as int64 or uint64."""
    return v & ((1 << 64) - 1)


def _brute_rows(d, tags, mask, k, base=0):
    """Selection by repeated scan over the eligible rows: the smallest remaining distance, the lowest row among equals."""
    left = [(float(x), i) for i, x in enumerate(d) if not np.isnan(x) and (_bits(int(tags[i])) & _bits(int(mask))) != 0]
    idx, dist = [], []
    while left and len(idx) < k:
        best = left[0]
        for c in left[1:]:
            if c[0] < best[0]:
                best = c
        left.remove(best)
        idx.append(best[1] + base)
        dist.append(best[0])
    pad = k - len(idx)
    return np.array(idx + [-1] * pad, dtype=np.int64), np.array(dist + [np.nan] * pad, dtype=np.float32)


def _brute_ids(d, labels, tags, mask, k, exclude=-1, base=0):
    left = [(float(x), i) for i, x in enumerate(d) if not np.isnan(x) and (_bits(int(tags[i])) & _bits(int(mask))) != 0
            and labels[i] >= 0 and labels[i] != exclude]
    idx, dist, lab = [], [], []
    while left and len(idx) < k:
        best = left[0]
        for c in left[1:]:
            if c[0] < best[0]:
                best = c
        idx.append(best[1] + base)
        dist.append(best[0])
        lab.append(int(labels[best[1]]))
        left = [c for c in left if labels[c[1]] != labels[best[1]]]
    pad = k - len(idx)
    return (np.array(idx + [-1] * pad, dtype=np.int64), np.array(dist + [np.nan] * pad, dtype=np.float32),
            np.array(lab + [-1] * pad, dtype=np.int64))


def _same(a, b):
    for x, y in zip(a, b):
        if x.dtype == np.float32:
            if not (np.array_equal(np.isnan(x), np.isnan(y)) and
                    np.array_equal(x[~np.isnan(x)].view(np.uint32), y[~np.isnan(y)].view(np.uint32))):
                return False
        elif not np.array_equal(x, y):
            return False
    return len(a) == len(b)


def test_eligibility_is_on_the_raw_64_bits():
    top = -(1 << 63)
    tags = np.array([0, 1, 2, 3, top, -1, top | 1, 1 << 62], dtype=np.int64)
    masks = np.array([0, 1, 2, top, -1, 1 << 62, 8], dtype=np.int64)
    el = tagged_ref.eligible(tags, masks)
    assert not el[0].any() and not el[:, 0].any()                                # a mask of 0, a tag of 0: never
    assert el[1].tolist() == [False, True, False, True, False, True, True, False]
    assert el[3].tolist() == [False, False, False, False, True, True, True, False]   # bit 63: the negative values
    assert el[4].tolist() == [False] + [True] * 7                                # mask -1: every row with a tag
    assert el[5].tolist() == [False] * 5 + [True, False, True]
    assert el[6].tolist() == [False] * 5 + [True, False, False]                   # bit 3: the all-ones tag alone
    for p in range(len(masks)):
        for r in range(len(tags)):
            assert bool(el[p, r]) == ((_bits(int(tags[r])) & _bits(int(masks[p]))) != 0)
    u = np.array([1 << 63, (1 << 64) - 1, 5], dtype=np.uint64)                   # uint64 is taken bit for bit
    assert tagged_ref.as_sets(u).tolist() == [top, -1, 5]
    assert np.array_equal(tagged_ref.eligible(u, u), tagged_ref.eligible(u.view(np.int64), u.view(np.int64)))
    assert tagged_ref.as_sets(np.array([-1, 3], dtype=np.int8)).tolist() == [-1, 3]      # narrower types sign-extend
    with pytest.raises(ValueError):
        tagged_ref.as_sets(np.array([1.0]))
    assert tagged_ref.MASK_CYCLE.tolist() == [1, 2, 4, 8, top, 0, -1, 6]


def test_tagged_lists_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    for trial in range(30):
        G, n = int(rng.integers(1, 60)), 8
        d = rng.integers(0, 6, (n, G)).astype(np.float32) / 4                     # many exact ties
        d[rng.random((n, G)) < 0.15] = np.nan
        tags = tagged_ref.case_tags(G) if trial % 2 else rng.integers(-4, 4, G).astype(np.int64)
        masks = tagged_ref.case_masks(n)
        labels = rng.integers(-1, 5, G).astype(np.int64)
        ex = rng.integers(-1, 5, n).astype(np.int64)
        for k in (1, 3, G, G + 2):
            for base in (0, 1000):
                rows = tagged_ref.topk_full(d, tags, masks, k, base)
                ids = tagged_ref.topk_ids_full(d, labels, tags, masks, k, ex, base)
                for p in range(n):
                    assert _same((rows[0][p], rows[1][p]), _brute_rows(d[p], tags, masks[p], k, base))
                    assert _same((ids[0][p], ids[1][p], ids[2][p]), _brute_ids(d[p], labels, tags, masks[p], k, int(ex[p]), base))
        assert (tagged_ref.topk_full(d, tags, masks, 3)[0][5] == -1).all()        # mask 0: all padding
    d = np.array([[0.5, 0.25, 0.25, 0.0]], dtype=np.float32)
    idx, dist = tagged_ref.topk_full(d, np.array([1, 2, 1, 2]), np.array([1]), 3)
    assert idx[0].tolist() == [2, 0, -1] and np.isnan(dist[0, 2])                # rows 3 and 1 are nearer and never listed
    full = np.arange(6, dtype=np.float32)[None]
    every = tagged_ref.topk_full(full, np.full(6, -1), np.array([-1]), 4, 10)     # every pair eligible: the untagged list
    assert _same(every, topk_ref.topk_full(full, 4, 10))
    lab = np.array([0, 0, 1, 1, 2, 2])
    ids = tagged_ref.topk_ids_full(full, lab, np.array([0, 1, 0, 1, 0, 0]), np.array([1]), 3)
    assert ids[0][0].tolist() == [1, 3, -1] and ids[2][0].tolist() == [0, 1, -1]  # each identity's best ELIGIBLE row
    want = topk_ids_ref.topk_ids_full(full, np.where(np.array([0, 1, 0, 1, 0, 0]) != 0, lab, -1), 3)
    assert _same(ids, want)                                                      # = the ineligible rows' labels set to -1


def test_case_tags_and_masks():
    for G in (1, 129, 4097, 66000):
        t = tagged_ref.case_tags(G)
        assert t.dtype == np.int64 and t.shape == (G,)
        assert not (t & 8).any()                                                 # bit 3 is never set
        assert (t & ~np.int64(7) & ~np.int64(-(1 << 63)) == 0).all()
        if G >= 4097:
            assert (t == 0).any() and (t < 0).any() and (t & 4).any()
            share = [float(((t >> b) & 1).mean()) for b in (0, 1, 2)] + [float((t < 0).mean())]
            assert abs(share[0] - .5) < .03 and abs(share[1] - .125) < .02 and abs(share[2] - 1 / 128) < .004 \
                and abs(share[3] - .5) < .03
        assert np.array_equal(t, tagged_ref.case_tags(G))
    assert tagged_ref.case_masks(10).tolist() == tagged_ref.MASK_CYCLE.tolist() + [1, 2]


@pytest.mark.parametrize('B,G,D', SHAPES)
def test_clear_shares_of_the_tagged_cases(B, G, D):
    """The cap tests/test_topk_tagged_gpu.py asserts per case before it asks the device, here with bit 63 itself (metric 1;
    metric 0 compares bit for bit) -- and that the tags matter: the masked list differs from the unmasked one for most probes."""
    probes, gal, _ = _inputs(B, G, D)
    tags, masks = tagged_ref.case_tags(G), tagged_ref.case_masks(B)
    full = rank_ref.distances(probes, gal, 1)
    fm = tagged_ref.masked(full, tags, masks)
    for k in (1, 5, 128):
        assert topk_ref.clear_share(fm, k, NEAR) >= MIN_CLEAR, k
    differ = int((topk_ref.topk_full(full, 5)[0] != topk_ref.topk_full(fm, 5)[0]).any(1).sum())
    assert G == 1 or differ >= (3 * B) // 4, differ                              # (masks 8 and 0 alone: a quarter of the probes)
    if G == 4097:
        assert 0.96 < topk_ref.clear_share(fm, 128, NEAR) < 0.97                # the smallest share of all the cases


def test_the_c_abi_carries_the_tagged_searches():
    """Fails on a library without the feature: both entry points declared, exported and bound, the stat named by the header
    and known to the library, the keywords on every Python form."""
    header = open(os.path.join(ROOT, 'include', 'dif.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    path = os.path.join(ROOT, 'deep-insight-face_amd', 'lib', 'libdif.so')
    lib = ctypes.CDLL(path)
    from deep_insight_face import _native, oneshot, parallel
    for fn in ('dif_match_topk_tagged', 'dif_match_topk_ids_tagged'):
        assert re.search(r'\bint\s+%s\s*\(' % fn, code), fn
        assert hasattr(lib, fn), fn
        assert fn in _native.SIGNATURES, fn
        assert fn in re.sub(r'\s+', ' ', header[header.index('watch-lists'):])   # documented, not only declared
    assert len(_native.SIGNATURES['dif_match_topk_tagged'][1]) == 10
    assert len(_native.SIGNATURES['dif_match_topk_ids_tagged'][1]) == 13
    assert '"topk_tagged_tiles"' in header[header.index('read-outs'):header.index('int dif_gallery_get_stat(')]
    assert b'topk_tagged_tiles\x00' in open(path, 'rb').read()                   # the key the library compares against
    assert 'topk_tagged_tiles' in oneshot.Gallery.stat.__doc__
    for f in (oneshot.Gallery.topk, oneshot.Gallery.topk_ids, oneshot.Gallery.topk_into, oneshot.Gallery.topk_ids_into,
              oneshot.topk, oneshot.topk_ids, parallel.ShardedGallery.topk, parallel.ShardedGallery.topk_ids):
        names = list(inspect.signature(f).parameters)
        assert names[-2:] == ['row_tags', 'probe_masks'], (f, names)
        assert inspect.signature(f).parameters['row_tags'].default is None
