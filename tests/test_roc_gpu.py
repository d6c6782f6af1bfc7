"""All-pairs verification counts (oneshot.Gallery.roc / dif_match_roc, evaluation/verification.py) against the CPU statement
tests/roc_ref.py:

    accept[j] = [sum(use & same & (dist < t[j])), sum(use & ~same & (dist < t[j]))];  totals = pairs used, and their NaNs

Metric 0: accept and totals equal the oracle's.  Metric 1: equal to the same counts formed from the library's own distances
(dif_pairwise), and against NumPy the two-sided bound  count(d < t - 2e-6) <= accept <= count(d < t + 2e-6)  -- the device
evaluates arccos in double and rounds once, NumPy's float32 arccos is within 2 ulp of that (test_within_gpu.py's NEAR)."""
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
import roc_ref

pytestmark = pytest.mark.gpu
NEAR = 2e-6          # metric 1: the arccos' last bits (test_within_gpu.py)
G0 = 4097            # 33 tiles of 128 rows, the last holding one row
BMAX = 130           # two probe blocks of the widest tile, the second ragged


@functools.lru_cache(maxsize=None)
def _inputs(G, D, B=BMAX):
    """Identities with four near-duplicate rows each; probes drawn the same way -> (probes, gallery, probe and row labels)."""
    rng = np.random.default_rng(1000 * G + D)
    nid = max(1, G // 4)
    centres = rng.standard_normal((nid, D))
    rl = (np.arange(G) % nid).astype(np.int64)
    pl = rng.integers(0, nid, B).astype(np.int64)
    gal = (centres[rl] + 0.05 * rng.standard_normal((G, D))).astype(np.float32)
    probes = (centres[pl] + 0.05 * rng.standard_normal((B, D))).astype(np.float32)
    for a in (gal, probes, rl, pl):
        a.setflags(write=False)
    return probes, gal, pl, rl


@functools.lru_cache(maxsize=None)
def _oracle(G, D, metric):
    probes, gal, _, _ = _inputs(G, D)
    full = roc_ref.distances(probes, gal, metric)
    full.setflags(write=False)
    return full


def _lib_full(probes, gal, clamp=False):
    """The library's own metric-1 distances of every pair (dif_pairwise: what dif_match_within compares and reports); with
    `clamp` the rule of 'clamp_nan': a similarity rounded above 1 is distance 0, below -1 distance 1."""
    from deep_insight_face import _native as N
    dev = N.require_device()
    g, _ = N.to_device_f32(gal, dev)
    p, _ = N.to_device_f32(probes, dev)
    out = torch.empty((p.shape[0], g.shape[0]), dtype=torch.float32, device=dev)
    sim = torch.empty_like(out)
    for b in range(p.shape[0]):
        N.check(N.lib.dif_pairwise(N.ptr(p[b]), 1, N.ptr(g), g.shape[0], g.shape[1], 1, N.ptr(out[b]), N.stream_ptr()))
        if clamp:
            N.check(N.lib.dif_pairwise(N.ptr(p[b]), 1, N.ptr(g), g.shape[0], g.shape[1], N.METRIC_SIMILARITY, N.ptr(sim[b]),
                                       N.stream_ptr()))
    d = out.cpu().numpy()
    if clamp:
        s = sim.cpu().numpy()
        with np.errstate(invalid='ignore'):
            d = np.where(np.isnan(d) & (s > 1), np.float32(0), np.where(np.isnan(d) & (s < -1), np.float32(1), d))
    return d


@functools.lru_cache(maxsize=None)
def _lib_oracle(G, D):
    probes, gal, _, _ = _inputs(G, D)
    full = _lib_full(probes, gal)
    full.setflags(write=False)
    return full


def _thresholds(full, T, metric, seed=0):
    """T thresholds (float64, unsorted): a grid over the distances' range; with room, duplicates, 0, a negative, 1, +inf, -inf
    and ACTUAL distances of the input, so that the strict comparison is met at equality."""
    rng = np.random.default_rng(seed + T)
    fin = full[np.isfinite(full)].astype(np.float64)
    hi = 1.0 if metric == 1 else (float(fin.max()) * 1.05 if fin.size else 4.0)
    actual = rng.choice(fin, 8) if fin.size else np.full(8, 0.25)
    if T == 1:
        return np.array([actual[0]])
    if T == 2:
        return np.array([actual[1], actual[1]])               # a duplicate, at equality
    t = np.arange(T, dtype=np.float64) * (hi / (T - 1))        # e.g. 0 .. 1 by about 0.01
    special = np.concatenate([[-0.5, 0.0, 1.0, np.inf, -np.inf, hi * 0.37, hi * 0.37], actual, actual[:3],
                              np.nextafter(actual[:2].astype(np.float32), np.float32(np.inf)).astype(np.float64)])
    where = rng.permutation(T)[:special.size]
    t[where] = special
    return rng.permutation(t)


def _roc(gal_h, probes, pl, rl, t, metric, first_row=None):
    a, tot = gal_h.roc(probes, pl, rl, t, metric, first_row=first_row)
    assert torch.is_tensor(a) and a.is_cuda and a.dtype == torch.int64 and tuple(a.shape) == (len(t), 2)
    assert torch.is_tensor(tot) and tot.is_cuda and tot.dtype == torch.int64 and tuple(tot.shape) == (4,)
    return a.cpu().numpy(), tot.cpu().numpy()


def _same(got, want, what=''):
    (a, tot), (wa, wt) = got, want
    bad = np.flatnonzero((a != wa).any(1))
    assert bad.size == 0, (what, bad[:6], a[bad[:6]].tolist(), wa[bad[:6]].tolist())
    assert np.array_equal(tot, wt), (what, tot, wt)


def _within_numpy(got, full, pl, rl, t, first_row=None, base=0):
    """metric 1 against NumPy: an inequality that always holds, whatever the arccos' last bits do."""
    a, tot = got
    lo, wt = roc_ref.counts_full(full, pl, rl, np.asarray(t) - NEAR, first_row, base)
    hi, _ = roc_ref.counts_full(full, pl, rl, np.asarray(t) + NEAR, first_row, base)
    assert (lo <= a).all() and (a <= hi).all(), (np.flatnonzero(((lo > a) | (a > hi)).any(1))[:6])
    assert np.array_equal(tot, wt)


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('D', [128, 512])
@pytest.mark.parametrize('B', [1, 33, 70, 130])
def test_counts_at_every_tile_shape(B, D, metric):
    """G = 4097; B = 1, 33, 70, 130: every census tile shape and a ragged last probe block; T = 1, 2, 100, 1024."""
    from deep_insight_face.oneshot import Gallery
    probes, gal, pl, rl = _inputs(G0, D)
    probes, pl = probes[:B], pl[:B]
    full = _oracle(G0, D, metric)[:B]
    lib = _lib_oracle(G0, D)[:B] if metric == 1 else full
    h = Gallery(gal)
    try:
        for T in (1, 2, 100, 1024):
            # (the actual distances among the thresholds are the LIBRARY's: equality is met on the values it compares)
            t = _thresholds(lib, T, metric, seed=B + D)
            got = _roc(h, probes, pl, rl, t, metric)
            _same(got, roc_ref.counts_full(lib, pl, rl, t), 'T=%d' % T)
            if metric == 1:
                _within_numpy(got, full, pl, rl, t)
            assert got[1][0] > 0 and got[1][0] + got[1][1] == B * G0 and (T < 100 or got[0][:, 0].max() > 0)
            if T == 100:
                # The point of the kernel: most pairs are binned from the MFMA key, the few inside a band go to ref_distance.
                # A band is 2 E wide and the grid's thresholds are hi / 99 apart, so the share of pairs inside one is about
                # 2 E / spacing whatever the distribution: metric 1, E <= 650 u in similarity, <= 2.5e-5 in distance, against
                # 0.01: 0.25 %; metric 0, E <= 0.05 at |q|^2 = |g|^2 = 512 against a spacing of 11: 0.9 %.  The twenty special
                # thresholds add as much again at most.  2 % holds all of it; the thresholds AT actual distances make it > 0.
                resolved = h.stat('roc_resolved')
                assert 0 < resolved <= 0.02 * B * G0, (resolved, B * G0)
    finally:
        h.close()


@functools.lru_cache(maxsize=None)
def _degenerate():
    return gi.match_degenerate_cases()


@pytest.mark.parametrize('clamp', [0, 1])
@pytest.mark.parametrize('metric', [0, 1])
def test_ties_and_nan_inputs(metric, clamp):
    """Exact duplicates (match_tie_inputs) and every degenerate case -- zero-norm, tiny, huge, non-finite rows and probes,
    anti-parallel rows -- under 'clamp_nan' 0 and 1: the NaN pairs are in the totals and in no accept."""
    from deep_insight_face.oneshot import Gallery
    cases = [('ties',) + gi.match_tie_inputs()] + list(_degenerate())
    saw_nan = False
    for name, probes, gal in cases:
        G = gal.shape[0]
        rl = (np.arange(G) // 4).astype(np.int64)
        pl = (np.arange(probes.shape[0]) * 29 % (G // 4)).astype(np.int64)
        with np.errstate(all='ignore'):
            full = roc_ref.distances(probes, gal, metric)
        lib = _lib_full(probes, gal, clamp=bool(clamp)) if metric == 1 else full
        t = _thresholds(lib, 100, metric, seed=len(name))
        h = Gallery(gal)
        try:
            h.set_option('clamp_nan', clamp)
            got = _roc(h, probes, pl, rl, t, metric)
        finally:
            h.close()
        _same(got, roc_ref.counts_full(lib, pl, rl, t), name)
        if metric == 1 and not clamp:
            _within_numpy(got, full, pl, rl, t)
        saw_nan |= bool(got[1][2:].sum() > 0)
        fin = np.array([got[1][0] - got[1][2], got[1][1] - got[1][3]])
        assert (got[0] <= fin[None, :]).all()                  # a NaN pair is in no accept
        same = pl[:, None] == rl[None, :]
        inf = np.array([np.sum(np.isposinf(lib) & same), np.sum(np.isposinf(lib) & ~same)])   # (metric 0, a non-finite row)
        assert np.array_equal(got[0][np.flatnonzero(np.isposinf(t))[0]], fin - inf)   # +inf accepts all the others below it
    assert saw_nan


@pytest.mark.parametrize('metric', [0, 1])
def test_labels(metric):
    """All the same, all different, negatives on both sides (four-row identities are every other test's)."""
    from deep_insight_face.oneshot import Gallery
    D, B = 128, 70
    probes, gal, pl, rl = _inputs(G0, D)
    probes, pl = probes[:B], pl[:B]
    lib = (_lib_oracle(G0, D) if metric == 1 else _oracle(G0, D, 0))[:B]
    t = _thresholds(lib, 100, metric, seed=5)
    h = Gallery(gal)
    try:
        for name, p, r in (('same', np.full(B, 7), np.full(G0, 7)), ('different', np.arange(B) + G0, np.arange(G0)),
                           ('negative', np.where(np.arange(B) % 5 == 0, -1 - np.arange(B), pl),
                            np.where(np.arange(G0) % 7 == 3, -2, rl))):
            got = _roc(h, probes, p.astype(np.int32), r, t, metric)   # (any integer dtype)
            _same(got, roc_ref.counts_full(lib, p, r, t), name)
            if name == 'same':
                assert got[1][1] == 0 and got[0][:, 1].sum() == 0 and got[1][0] == B * G0
            if name == 'different':
                assert got[1][0] == 0 and got[0][:, 0].sum() == 0
            if name == 'negative':
                assert got[1][:2].sum() == (p >= 0).sum() * (r >= 0).sum() < B * G0
    finally:
        h.close()


@pytest.mark.parametrize('metric', [0, 1])
def test_first_row_and_index_base(metric):
    """A random first_row; index_base != 0 shifts first_row's meaning and nothing else."""
    from deep_insight_face.oneshot import Gallery
    D, B = 128, 70
    probes, gal, pl, rl = _inputs(G0, D)
    probes, pl = probes[:B], pl[:B]
    lib = (_lib_oracle(G0, D) if metric == 1 else _oracle(G0, D, 0))[:B]
    t = _thresholds(lib, 100, metric, seed=6)
    rng = np.random.default_rng(8)
    fr = rng.integers(-5, G0 + 5, B)
    fr[:4] = [0, G0, G0 - 1, 128]
    h = Gallery(gal)
    try:
        got0 = _roc(h, probes, pl, rl, t, metric, first_row=fr)
        _same(got0, roc_ref.counts_full(lib, pl, rl, t, fr), 'first_row')
        assert got0[1][:2].sum() == np.sum(G0 - np.clip(fr, 0, G0))
        _same(_roc(h, probes, pl, rl, t, metric, first_row=torch.from_numpy(fr)), got0, 'tensor first_row')
    finally:
        h.close()
    h = Gallery(gal, index_base=1000)
    try:
        _same(_roc(h, probes, pl, rl, t, metric, first_row=fr + 1000), got0, 'shifted')
        _same(_roc(h, probes, pl, rl, t, metric, first_row=fr), roc_ref.counts_full(lib, pl, rl, t, fr, 1000), 'not shifted')
        _same(_roc(h, probes, pl, rl, t, metric), roc_ref.counts_full(lib, pl, rl, t), 'no first_row')
    finally:
        h.close()


def test_all_pairs_counts():
    """A 700-row set against itself in blocks of 128: every unordered pair once, no row with itself."""
    from deep_insight_face.evaluation import verification as ver
    n, D = 700, 128
    _, gal, _, rl = _inputs(G0, D)
    e, lab = gal[:n], (np.arange(n) // 4).astype(np.int64)
    own = np.arange(n) + 1
    t0 = np.arange(0, 400, 1.0)
    sq = roc_ref.distances(e, e, 0)
    a, tot = ver.all_pairs_counts(e, lab, t0, distance_metric=0, block=128)
    want = roc_ref.counts_full(sq, lab, lab, t0, first_row=own)
    _same((a.cpu().numpy(), tot.cpu().numpy()), want, 'metric 0')
    assert want[1][0] + want[1][1] == n * (n - 1) // 2 and want[1][0] == (n // 4) * 6
    t1 = np.arange(0, 1, 0.01)
    a, tot = ver.all_pairs_counts(torch.from_numpy(e), torch.from_numpy(lab), t1, distance_metric=1, block=128)
    _within_numpy((a.cpu().numpy(), tot.cpu().numpy()), roc_ref.distances(e, e, 1), lab, lab, t1, first_row=own)
    _same((a.cpu().numpy(), tot.cpu().numpy()), roc_ref.counts_full(_lib_full(e, e), lab, lab, t1, first_row=own), 'metric 1')


def test_rounds_give_the_same_counts():
    """'roc_round' = 128 with B = 300: three rounds, the counts of one."""
    from deep_insight_face.oneshot import Gallery
    D, B = 128, 300
    probes, gal, pl, rl = _inputs(G0, D, B)
    h = Gallery(gal)
    try:
        for metric in (0, 1):
            t = np.arange(0, 400, 1.0) if metric == 0 else np.arange(0, 1, 0.01)
            one = _roc(h, probes, pl, rl, t, metric)
            h.set_option('roc_round', 128)
            _same(_roc(h, probes, pl, rl, t, metric), one, 'rounds')
            h.set_option('roc_round', 0)
            if metric == 0:
                _same(one, roc_ref.counts(probes, gal, pl, rl, t, 0), 'oracle')
        with pytest.raises(ValueError, match='roc_round'):
            h.set_option('roc_round', 100)                      # not a multiple of 128
    finally:
        h.close()


@pytest.mark.parametrize('metric', [0, 1])
def test_resolve_blocks_take_several_trips(metric):
    """'roc_blocks' = 1, 2, 3: 33 tiles x 300 probes are 9 900 masks, 20 trips of 512 for one block (7 for each of three);
    T = 1024 flags a few per cent of the pairs, so every trip queues masks.  The counts of the default launch and the oracle's."""
    from deep_insight_face.oneshot import Gallery
    D, B = 128, 300
    probes, gal, pl, rl = _inputs(G0, D, B)
    full = roc_ref.distances(probes, gal, metric)
    lib = _lib_full(probes, gal) if metric == 1 else full
    t = _thresholds(lib, 1024, metric, seed=9)
    want = roc_ref.counts_full(lib, pl, rl, t)
    h = Gallery(gal)
    try:
        _same(_roc(h, probes, pl, rl, t, metric), want, 'default')
        resolved = h.stat('roc_resolved')
        assert resolved > 20 * 64                               # enough flagged pairs to meet every trip
        for blocks in (1, 2, 3):
            h.set_option('roc_blocks', blocks)
            _same(_roc(h, probes, pl, rl, t, metric), want, 'blocks=%d' % blocks)
            assert h.stat('roc_resolved') == resolved
        h.set_option('roc_blocks', 0)
        with pytest.raises(ValueError, match='roc_blocks'):
            h.set_option('roc_blocks', -1)
    finally:
        h.close()


def test_handle_reuse():
    """B = 70, 33, 70 interleaved with match, within and update on one handle: the answers of fresh handles."""
    from deep_insight_face.oneshot import Gallery
    D = 128
    probes, gal, pl, rl = _inputs(G0, D)
    t = np.arange(0, 400, 1.0)

    def fresh(rows, B):
        f = Gallery(rows)
        try:
            return _roc(f, probes[:B], pl[:B], rl[:rows.shape[0]], t, 0)
        finally:
            f.close()

    first = gal[:3000]
    h = Gallery(first)
    try:
        _same(_roc(h, probes[:70], pl[:70], rl[:3000], t, 0), fresh(first, 70), 'first')
        idx, _ = h.match(probes[:40], 0)
        _same(_roc(h, probes[:33], pl[:33], rl[:3000], t, 0), fresh(first, 33), 'smaller')
        cnt, _, _ = h.within(probes[:90], 30.0, 0, max_hits=4)
        h.update(gal[3000:])                                    # 3000 -> 4097 rows: the workspace has to grow
        changed = np.array(gal)
        changed[100:110] = gal[200:210]
        h.update(changed[100:110], first_row=100)
        _same(_roc(h, probes[:70], pl[:70], rl, t, 0), fresh(changed, 70), 'after update')
        f = Gallery(changed)
        try:
            assert np.array_equal(f.match(probes[:40], 0)[0], h.match(probes[:40], 0)[0])
            assert np.array_equal(f.within(probes[:90], 30.0, 0, max_hits=4)[0], h.within(probes[:90], 30.0, 0, max_hits=4)[0])
        finally:
            f.close()
    finally:
        h.close()


def test_empty_gallery_and_no_probes():
    from deep_insight_face.oneshot import Gallery
    D = 128
    probes, gal, pl, rl = _inputs(G0, D)
    h = Gallery(emd_size=D)
    try:
        a, tot = _roc(h, probes[:5], pl[:5], np.zeros(0, np.int64), [0.1, 0.5, np.inf], 1)
        assert not a.any() and not tot.any()
        h.set(gal[:300])
        a, tot = _roc(h, probes[:0], pl[:0], rl[:300], [0.1, 0.5, np.inf], 1)   # B = 0 still zeroes the outputs
        assert not a.any() and not tot.any()
    finally:
        h.close()


def test_argument_errors():
    from deep_insight_face import _native as N
    from deep_insight_face.oneshot import Gallery
    D, B = 128, 5
    probes, gal, pl, rl = _inputs(G0, D)
    h = Gallery(gal[:300])
    try:
        with pytest.raises(ValueError, match='NaN'):
            h.roc(probes[:B], pl[:B], rl[:300], [0.1, np.nan, 0.3])
        with pytest.raises(ValueError, match=r'outside \[1, 1024\]'):
            h.roc(probes[:B], pl[:B], rl[:300], [])
        with pytest.raises(ValueError, match=r'outside \[1, 1024\]'):
            h.roc(probes[:B], pl[:B], rl[:300], np.linspace(0, 1, 1025))
        dev = N.require_device()
        p, _ = N.to_device_f32(probes[:B], dev)
        lab = torch.from_numpy(np.array(pl[:B])).to(dev)
        rows = torch.from_numpy(np.array(rl[:300])).to(dev)
        acc = torch.zeros((3, 2), dtype=torch.int64, device=dev)
        tot = torch.zeros((4,), dtype=torch.int64, device=dev)
        with pytest.raises(ValueError, match='non-decreasing'):
            h.roc_into(p, lab, rows, None, torch.tensor([0.1, 0.3, 0.2], device=dev), 1, acc, tot)
        h.roc_into(p, lab, rows, None, torch.tensor([0.1, 0.3, 0.3], device=dev), 1, acc, tot)   # duplicates are fine
        with pytest.raises(ValueError):
            h.roc(probes[:B], pl[:B], rl[:299], [0.5])          # row labels that do not cover the gallery
        with pytest.raises(ValueError):
            h.roc(probes[:B], pl[:B].astype(np.float32), rl[:300], [0.5])
        with pytest.raises(RuntimeError):
            h.roc(probes[:B], pl[:B], rl[:300], [0.5], distance_metric=2)
    finally:
        h.close()


def test_val_at_far_on_a_planted_set():
    """50 identities of two rows, 30 of them 0.1 apart and 20 of them 0.4; every impostor pair at 0.5 but three at 0.205 (and
    three more at 0.225): the FAR curve steps from 0 to 3 / n_diff between the thresholds 0.20 and 0.21, a target of half
    that step interpolates a threshold between them, and the TAR there is the planted 30 / 50."""
    from deep_insight_face.evaluation import verification as ver
    D = 128
    rows, lab = [], []
    for i in range(50):
        th = np.pi * (0.1 if i < 30 else 0.4)
        a, b = np.zeros(D), np.zeros(D)
        a[i] = 1.0
        b[i], b[64 + i] = np.cos(th), np.sin(th)
        rows += [a, b]
        lab += [i, i]
    for k in range(3):
        v = np.zeros(D)
        v[k], v[120 + k] = np.cos(0.205 * np.pi), np.sin(0.205 * np.pi)
        rows.append(v)
        lab.append(100 + k)
    e = (np.array(rows) * 3.0).astype(np.float32)
    lab = np.array(lab)
    n = e.shape[0]
    n_diff = n * (n - 1) // 2 - 50
    thresholds = np.arange(0, 1, 0.01)
    val, far, thr = ver.val_at_far(e, lab, thresholds, 1.5 / n_diff, distance_metric=1, block=64)
    assert 0.20 < thr < 0.21
    assert val == 30 / 50 and far == 3 / n_diff
    a, tot = ver.all_pairs_counts(e, lab, thresholds, distance_metric=1, block=64)
    assert tot.cpu().tolist() == [50, n_diff, 0, 0]
    t_at, tar = ver.tar_at_far(a, tot, thresholds, [1e-6, 3 / n_diff, 0.9])
    assert np.isnan(t_at[0]) and np.isnan(tar[0])              # 1 / n_diff > 1e-6: not resolvable
    assert abs(t_at[1] - 0.22) < 1e-9 and tar[1] == 0.6        # the largest threshold that lets only the three at 0.205 in
    assert tar[2] == 1.0
