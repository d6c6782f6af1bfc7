"""tests/topk_ref.py -- the NumPy statement of the top-k list that the GPU tests compare against -- checked against a
brute-force loop, against the rank of the mate (rank_ref), and for the CLEAR-position shares tests/test_topk_gpu.py asserts
before it asks the device; and the C ABI carries the entry point and its option.  No GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import embed_dims as ed
import golden_inputs as gi
import rank_ref
import topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 2e-6          # test_within_gpu.py
MIN_CLEAR = 0.9
SHAPES = [(1, 1, 32), (3, 129, 64), (65, 257, 512), (130, 1000, 128), (64, 4097, 512), (3, 66000, 32)]


def _brute(d, k, base=0):
    """Selection by repeated scan: the smallest remaining distance, the lowest row among equals, NaN never."""
    left = [(float(x), i) for i, x in enumerate(d) if not np.isnan(x)]
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


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(np.isnan(a[1]), np.isnan(b[1])) and \
        np.array_equal(a[1][~np.isnan(a[1])].view(np.uint32), b[1][~np.isnan(b[1])].view(np.uint32))


def test_topk_against_a_brute_force_loop():
    d = np.array([0.5, np.nan, 0.25, 0.5, np.nan, 0.75, 0.25, np.inf, 0.0], dtype=np.float32)
    for k in (1, 2, 3, 7, 8, 9, 12):
        assert _same(topk_ref.topk_row(d, k), _brute(d, k))
        assert _same(topk_ref.topk_row(d, k, 1000), _brute(d, k, 1000))
    idx, dist = topk_ref.topk_row(d, 9)
    assert list(idx) == [8, 2, 6, 0, 3, 5, 7, -1, -1] and np.isnan(dist[7:]).all() and dist[6] == np.inf   # ties to the lower row
    assert list(topk_ref.topk_row(d, 3, 1000)[0]) == [1008, 1002, 1006]
    idx, dist = topk_ref.topk_row(np.zeros(0, dtype=np.float32), 3)                 # an empty gallery: all padding
    assert list(idx) == [-1, -1, -1] and np.isnan(dist).all() and idx.dtype == np.int64 and dist.dtype == np.float32
    idx, dist = topk_ref.topk_row(np.full(5, np.nan, dtype=np.float32), 2)          # nothing but NaN
    assert list(idx) == [-1, -1] and np.isnan(dist).all()
    rng = np.random.default_rng(5)
    for trial in range(20):
        G = int(rng.integers(1, 40))
        d = rng.integers(0, 6, G).astype(np.float32) / 4                            # many exact ties
        d[rng.random(G) < 0.2] = np.nan
        for k in (1, 3, G, G + 2):
            assert _same(topk_ref.topk_row(d, k), _brute(d, k))
    probes, gal = gi.match_tie_inputs()
    for metric in (0, 1):
        got = topk_ref.topk(probes, gal[:64], 5, metric, index_base=7)
        full = rank_ref.distances(probes, gal[:64], metric)
        for b in range(probes.shape[0]):
            assert _same((got[0][b], got[1][b]), _brute(full[b], 5, 7))


def test_topk_agrees_with_the_rank_of_the_mate():
    cases = [gi.match_tie_inputs(), gi.match_near_tie_inputs()]
    cases += [(p, g) for n, p, g in gi.match_degenerate_cases() if n in ('zero_rows', 'odd_probes_odd_rows')]
    for probes, gal in cases:
        for metric in (0, 1):
            full = rank_ref.distances(probes[:12], gal, metric)
            idx, dist = topk_ref.topk_full(full, 6, index_base=50)
            for b in range(full.shape[0]):
                for j in range(6):
                    if idx[b, j] < 0:
                        assert np.isnan(dist[b, j]) and (idx[b, j:] == -1).all()
                        continue
                    r, dm = rank_ref.rank_row(full[b], idx[b, j], 50)
                    assert r == j and dm.view(np.uint32) == dist[b, j].view(np.uint32)


@functools.lru_cache(maxsize=None)
def _inputs(B, G, D, seed=0):
    """test_rank_gpu.py's generator (the same arrays)."""
    rng = np.random.default_rng(1000 * G + 10 * B + D + seed)
    nid = max(1, G // 4)
    centres = rng.standard_normal((nid, D))
    gal = (centres[np.arange(G) % nid] + 0.05 * rng.standard_normal((G, D))).astype(np.float32)
    pick = rng.integers(0, nid, B)
    probes = (centres[pick] + 0.05 * rng.standard_normal((B, D))).astype(np.float32)
    return probes, gal, pick


@pytest.mark.parametrize('B,G,D', SHAPES + [(70, 4097, 128)] + list(ed.QUERY_SHAPES))
def test_clear_shares_of_the_shapes(B, G, D):
    """The cap test_topk_gpu.py asserts per case, on the oracle alone (metric 1; metric 0 compares bit for bit)."""
    probes, gal, _ = _inputs(B, G, D)
    full = rank_ref.distances(probes, gal, 1)
    for k in (1, 5, 128):
        assert topk_ref.clear_share(full, k, NEAR) >= MIN_CLEAR, k


def test_clear_shares_of_the_degenerate_fixtures():
    for name, probes, gal in gi.match_degenerate_cases():
        full = rank_ref.distances(probes, gal, 1)
        for k in (1, 3, 128):
            assert topk_ref.clear_share(full, k, NEAR) >= MIN_CLEAR, (name, k)
        small = topk_ref.small_gallery(probes, gal)
        assert small.shape[0] == 126
        full = rank_ref.distances(probes, small, 1)
        for k in (1, 3, 128):
            assert topk_ref.clear_share(full, k, NEAR) >= MIN_CLEAR, (name, 'small', k)


def test_clear_positions_rule():
    d = np.array([[0.1, 0.1 + 1e-6, 0.3, 0.5, np.nan, 0.5 + 1e-6, 0.7]], dtype=np.float64).astype(np.float32)
    c = topk_ref.clear_positions(d, 8, NEAR)
    assert list(c[0]) == [False, False, True, False, False, True, False, False]     # six listed, two slots of padding
    assert list(topk_ref.clear_positions(d, 3, NEAR)[0]) == [False, False, True]
    assert list(topk_ref.clear_positions(d, 4, NEAR)[0]) == [False, False, True, False]   # the neighbour beyond k counts
    assert topk_ref.clear_share(d, 8, NEAR) == 2 / 6
    assert topk_ref.clear_share(np.full((2, 3), np.nan, dtype=np.float32), 2, NEAR) == 1.0


def test_the_c_abi_carries_topk():
    """Fails on a library without the feature: the entry point declared and exported, its limit, the option in the key table."""
    header = open(os.path.join(ROOT, 'include', 'dif.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'\bint\s+dif_match_topk\s*\(', code)
    assert re.search(r'#define DIF_TOPK_MAX 128\b', header)
    lib = ctypes.CDLL(os.path.join(ROOT, 'deep-insight-face_amd', 'lib', 'libdif.so'))
    assert hasattr(lib, 'dif_match_topk')
    fn = lib.dif_gallery_option_name
    fn.restype = ctypes.c_char_p
    fn.argtypes = [ctypes.c_int]
    keys = []
    while fn(len(keys)) is not None:
        keys.append(fn(len(keys)).decode())
        assert len(keys) < 100
    assert 'topk_seed' in keys and 'topk_round' in keys and 'within_round' in keys
    from deep_insight_face import _native, oneshot
    assert 'dif_match_topk' in _native.SIGNATURES
    assert oneshot.TOPK_MAX == 128 and callable(oneshot.topk) and callable(oneshot.Gallery.topk_into)
