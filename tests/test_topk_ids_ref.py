"""tests/topk_ids_ref.py -- the NumPy statement of the identity-level top-k list that tests/test_topk_ids_gpu.py compares
against -- checked against a brute-force loop; the CLEAR-position shares and the simulated tile counts that file asserts
before it asks the device; the C ABI carries the entry point and its stat; identity_rank / evaluate_identification_ids on
hand-made lists.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import embed_dims as ed
import golden_inputs as gi
import rank_ref
import topk_ids_ref as ir
import topk_ref
from test_topk_ref import SHAPES, _inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 2e-6          # test_within_gpu.py
MIN_CLEAR = 0.9
WORK_SHAPE = (3, 66000, 32)


def _brute(d, labels, k, exclude=-1, base=0):
    """Selection by repeated scan: the smallest remaining distance, the lowest row among equals; NaN, a negative label, the
    excluded label and a label listed already never."""
    left = [(float(x), i) for i, x in enumerate(d) if not np.isnan(x) and labels[i] >= 0 and labels[i] != exclude]
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
    return np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(np.isnan(a[1]), np.isnan(b[1])) and \
        np.array_equal(a[1][~np.isnan(a[1])].view(np.uint32), b[1][~np.isnan(b[1])].view(np.uint32))


def test_topk_ids_against_a_brute_force_loop():
    d = np.array([0.5, np.nan, 0.25, 0.5, np.nan, 0.75, 0.25, np.inf, 0.0, 0.1], dtype=np.float32)
    labels = np.array([3, 3, 7, 4, 7, 3, 9, 5, -1, 7], dtype=np.int64)
    idx, dist, lab = ir.topk_ids_row(d, labels, 6)
    # row 8 (label -1) is out; identity 7's best row is 9; rows 2 and 6 tie at 0.25: the lower row's identity (7) is listed
    # already, 9 follows; rows 0 and 3 tie at 0.5: the lower row's identity 3 comes first
    assert list(idx) == [9, 6, 0, 3, 7, -1] and list(lab) == [7, 9, 3, 4, 5, -1] and dist[4] == np.inf and np.isnan(dist[5])
    assert list(ir.topk_ids_row(d, labels, 3, exclude=7)[0]) == [6, 0, 3]
    assert list(ir.topk_ids_row(d, labels, 2, exclude=7, index_base=1000)[0]) == [1006, 1000]
    assert _same(ir.topk_ids_row(d, labels, 3, exclude=-1), ir.topk_ids_row(d, labels, 3, exclude=-5))   # negative: nothing
    for k in (1, 2, 4, 5, 6, 12):
        for ex in (-1, 3, 7, 9, 11):
            assert _same(ir.topk_ids_row(d, labels, k, ex), _brute(d, labels, k, ex))
            assert _same(ir.topk_ids_row(d, labels, k, ex, 1000), _brute(d, labels, k, ex, 1000))
    out = ir.topk_ids_row(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64), 3)       # an empty gallery: all padding
    assert list(out[0]) == [-1, -1, -1] and np.isnan(out[1]).all() and list(out[2]) == [-1, -1, -1]
    assert out[0].dtype == np.int64 and out[1].dtype == np.float32 and out[2].dtype == np.int64
    out = ir.topk_ids_row(d, np.full(10, -2, dtype=np.int64), 2)                               # every label negative
    assert list(out[0]) == [-1, -1] and np.isnan(out[1]).all()
    out = ir.topk_ids_row(d, np.full(10, 6, dtype=np.int64), 4)                                # one label: one entry, the arg-min
    assert list(out[0]) == [8, -1, -1, -1] and list(out[2]) == [6, -1, -1, -1]
    big = labels.copy()
    big[big >= 0] += 2 ** 40                                                                    # labels are full int64
    a, b = ir.topk_ids_row(d, labels, 6, exclude=7), ir.topk_ids_row(d, big, 6, exclude=7 + 2 ** 40)
    assert np.array_equal(a[0], b[0]) and np.array_equal(np.where(a[2] >= 0, a[2] + 2 ** 40, -1), b[2])
    rng = np.random.default_rng(5)
    for trial in range(30):
        G = int(rng.integers(1, 40))
        d = rng.integers(0, 6, G).astype(np.float32) / 4                                        # many exact ties
        d[rng.random(G) < 0.2] = np.nan
        labels = rng.integers(-1, 6, G).astype(np.int64)
        for k in (1, 3, 7, G + 2):                                                              # k above the identities
            for ex in (-1, 0, 2):
                assert _same(ir.topk_ids_row(d, labels, k, ex), _brute(d, labels, k, ex))
    # all-distinct labels: the row-level list
    d = rng.random(50).astype(np.float32)
    a = ir.topk_ids_row(d, np.arange(50)[::-1].copy(), 7)
    b = topk_ref.topk_row(d, 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    probes, gal = gi.match_tie_inputs()
    labels = np.arange(64) // 4
    for metric in (0, 1):
        full = rank_ref.distances(probes, gal[:64], metric)
        got = ir.topk_ids_full(full, labels, 5, exclude=np.arange(8), index_base=7)
        for b in range(probes.shape[0]):
            assert _same((got[0][b], got[1][b], got[2][b]), _brute(full[b], labels, 5, b, 7))


def test_clear_positions_rule():
    d = np.array([[0.1, 0.1 + 1e-6, 0.3, 0.5, np.nan, 0.5 + 1e-6, 0.7]], dtype=np.float64).astype(np.float32)
    distinct = np.arange(7)
    assert np.array_equal(ir.clear_positions(d, distinct, 8, NEAR), topk_ref.clear_positions(d, 8, NEAR))   # rows = identities
    assert ir.clear_share(d, distinct, 8, NEAR) == 2 / 6
    labels = np.array([0, 0, 1, 2, 2, 2, 3])          # the near pairs fall inside one identity each: the bests 0.1 0.3 0.5 0.7
    assert list(ir.clear_positions(d, labels, 5, NEAR)[0]) == [True, True, True, True, False]
    assert ir.clear_share(d, labels, 5, NEAR) == 1.0
    labels = np.array([0, 1, 1, 2, 2, 3, 4])          # bests 0.1, 0.1 + 1e-6, 0.5, 0.5 + 1e-6, 0.7
    assert list(ir.clear_positions(d, labels, 5, NEAR)[0]) == [False, False, False, False, True]
    assert list(ir.clear_positions(d, labels, 3, NEAR)[0]) == [False, False, False]           # the neighbour beyond k counts
    assert list(ir.clear_positions(d, labels, 3, NEAR, exclude=[3])[0]) == [False, False, True]
    assert ir.clear_share(np.full((2, 3), np.nan, dtype=np.float32), np.arange(3), 2, NEAR) == 1.0


def _labellings(G):
    nid = max(1, G // 4)
    return {'spread': np.arange(G) % nid, 'contiguous': np.arange(G) // 4, 'distinct': np.arange(G),
            'one': np.zeros(G, dtype=np.int64)}


@pytest.mark.parametrize('B,G,D', SHAPES + [(70, 4097, 128)] + list(ed.QUERY_SHAPES))
def test_clear_shares_of_the_shapes(B, G, D):
    """The cap test_topk_ids_gpu.py asserts per case, on the oracle alone (metric 1; metric 0 compares bit for bit): every
    labelling, with and without the probe's own identity excluded."""
    probes, gal, pick = _inputs(B, G, D)
    full = rank_ref.distances(probes, gal, 1)
    for name, labels in _labellings(G).items():
        for ex in (None, pick):
            for k in (1, 5, 128):
                assert ir.clear_share(full, labels, k, NEAR, ex) >= MIN_CLEAR, (name, ex is not None, k)


def test_clear_shares_of_the_degenerate_fixtures():
    for name, probes, gal in gi.match_degenerate_cases():
        full = rank_ref.distances(probes, gal, 1)
        labels = np.arange(gal.shape[0]) // 4
        for k in (1, 3, 128):
            assert ir.clear_share(full, labels, k, NEAR) >= MIN_CLEAR, (name, k)


def test_simulated_tiles_rule():
    """Ten tiles of two rows; identity 0 fills the three nearest tiles."""
    d = np.array([.01, .02, .03, .04, .05, .06, .5, .95, .6, .95, .7, .95, .8, .95, .91, .95, .92, .95, .93, .95],
                 dtype=np.float32)
    labels = np.array([0] * 6 + list(range(1, 15)))
    # k = 2: the seed of 2 tiles sees identity 0 alone, t = inf, 8 tiles are left > 2: s = 4 adds tiles 2 and 3 (identity 1 at
    # 0.5): t = 0.5, nothing else is within it: 4 tiles.  The single seed sweeps everything.
    assert ir.simulated_tiles(d, labels, 2, 'grow', tile=2) == 4
    assert ir.simulated_tiles(d, labels, 2, 'single', tile=2) == 10
    assert ir.simulated_tiles(d, labels, 2, 'ideal', tile=2) == 4
    assert ir.simulated_tiles(d, labels, 2, 'grow', seed=100, tile=2) == 10               # a seed above the tile count
    # identity 0 excluded: s = 2 finds nothing, s = 4 finds identities 1 (.5) and 2 (.95): t = .95 leaves 6 > 4 tiles; s = 8
    # evaluates tiles 0 .. 7: t = .6 and the last two tiles are beyond it.  The ideal schedule stops after tile 4
    assert ir.simulated_tiles(d, labels, 2, 'grow', exclude=0, tile=2) == 8
    assert ir.simulated_tiles(d, labels, 2, 'ideal', exclude=0, tile=2) == 5
    assert ir.simulated_tiles(d[:0], labels[:0], 2, 'grow', tile=2) == 0


@pytest.mark.parametrize('metric', [0, 1])
def test_simulated_tile_counts_stay_under_the_cap(metric):
    """The work test's condition stat('topk_ids_tiles') <= B * gtiles / 8, on the oracle: the growing seed stays far below
    it on the natural and on the crowd input; a single seed of k tiles does not."""
    B, G, D = WORK_SHAPE
    probes, gal, _ = _inputs(B, G, D)
    labels = np.arange(G) % (G // 4)
    gtiles = (G + 127) // 128
    cap = gtiles // 8
    for name, (p, g, lab) in (('natural', (probes, gal, labels)), ('crowd', ir.crowd_inputs(probes, gal, labels))):
        full = rank_ref.distances(p, g, metric)
        grow = [ir.simulated_tiles(full[b], lab, 5, 'grow') for b in range(B)]
        single = [ir.simulated_tiles(full[b], lab, 5, 'single') for b in range(B)]
        print(name, metric, 'grow', grow, 'single', single, 'cap', cap)
        assert max(grow) <= cap, (name, grow)       # (the simulation has no band E: the cap leaves it a factor of three)
        assert min(single) > cap, (name, single)
        if metric == 1:
            assert ir.clear_share(full, lab, 5, NEAR) >= MIN_CLEAR


def test_the_c_abi_carries_topk_ids():
    """Fails on a library without the feature: the entry point declared and exported, its signature, the Python callables,
    the stat key accepted."""
    header = open(os.path.join(ROOT, 'include', 'dif.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'\bint\s+dif_match_topk_ids\s*\(', code)
    assert '"topk_ids_tiles"' in header and '+ dif_match_topk_ids' in header
    assert re.search(r'#define DIF_VERSION 110\b', header)
    lib = ctypes.CDLL(os.path.join(ROOT, 'deep-insight-face_amd', 'lib', 'libdif.so'))
    assert hasattr(lib, 'dif_match_topk_ids')
    from deep_insight_face import _native, oneshot
    from deep_insight_face.evaluation import identification
    assert 'dif_match_topk_ids' in _native.SIGNATURES and len(_native.SIGNATURES['dif_match_topk_ids'][1]) == 11
    assert callable(oneshot.topk_ids) and callable(oneshot.Gallery.topk_ids) and callable(oneshot.Gallery.topk_ids_into)
    assert callable(identification.identity_rank) and callable(identification.evaluate_identification_ids)
    # the stat key is accepted on a handle that has made no call (no device is touched: there is no counter yet)
    lib.dif_gallery_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    lib.dif_gallery_get_stat.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    lib.dif_gallery_destroy.argtypes = [ctypes.c_void_p]
    h = ctypes.c_void_p()
    assert lib.dif_gallery_create(ctypes.byref(h), 32) == 0
    v = ctypes.c_int64(-7)
    assert lib.dif_gallery_get_stat(h, b'topk_ids_tiles', ctypes.byref(v), None) == 0 and v.value == 0
    assert lib.dif_gallery_get_stat(h, b'topk_ids_tile', ctypes.byref(v), None) != 0
    lib.dif_gallery_destroy(h)


def test_identity_rank_and_cmc_on_hand_made_lists():
    from deep_insight_face.evaluation import identification as ident
    lists = np.array([[4, 7, 9], [7, 4, -1], [9, 8, 7], [1, 2, 3], [-1, -1, -1], [5, 6, 7]], dtype=np.int64)
    probe = np.array([4, 4, 7, 9, 3, -1], dtype=np.int64)
    mated = np.array([True, True, True, True, True, False])
    rank = ident.identity_rank(lists, probe, mated)
    assert rank.dtype == np.int64 and list(rank) == [0, 1, 2, 3, 3, -1]       # k = 3: not listed; the padding matches nobody
    assert list(ident.identity_rank(lists, np.full(6, -1), np.ones(6, dtype=bool))) == [3] * 6
    cmc = ident.cmc(rank, 3)
    np.testing.assert_array_equal(cmc, np.array([1, 2, 3], dtype=np.float64) / 5)
    assert ident.identity_rank(np.zeros((2, 0), dtype=np.int64), np.array([1, 2]), np.array([True, False])).tolist() == [0, -1]


def test_evaluate_identification_ids_arithmetic():
    """On a stand-in gallery whose topk_ids is the NumPy statement: one call with k = max_rank, mated = the probe's label is
    among the non-negative row labels."""
    from deep_insight_face import oneshot
    from deep_insight_face.evaluation import identification as ident
    rng = np.random.default_rng(3)
    full = rng.random((6, 12)).astype(np.float32)
    row_labels = np.array([0, 0, 1, 1, 2, 2, 3, 3, -1, -1, 4, 4], dtype=np.int64)
    probe_labels = np.array([0, 1, 2, 3, 4, 5], dtype=np.int64)                # identity 5 is enrolled nowhere
    calls = []

    class Stub(oneshot.Gallery):
        def __init__(self):
            pass

        def topk_ids(self, probes, k, labels, distance_metric=1, exclude=None):
            calls.append((k, distance_metric, exclude))
            return ir.topk_ids_full(full, labels, k)

        def close(self):
            pass

        def __del__(self):
            pass

    out = ident.evaluate_identification_ids(Stub(), np.zeros((6, 32), dtype=np.float32), probe_labels, row_labels, 0, max_rank=3)
    assert calls == [(3, 0, None)] and sorted(out) == ['cmc', 'dist', 'idx', 'label', 'rank']
    want = ir.topk_ids_full(full, row_labels, 3)
    assert np.array_equal(out['idx'], want[0]) and np.array_equal(out['label'], want[2])
    rank = []
    for b in range(6):
        order = [int(x) for x in ir.topk_ids_row(full[b], row_labels, 5)[2]]
        rank.append(-1 if b == 5 else min(order.index(int(probe_labels[b])), 3))
    assert list(out['rank']) == rank
    np.testing.assert_array_equal(out['cmc'], ident.cmc(np.array(rank), 3))
    assert (np.diff(out['cmc']) >= 0).all()
