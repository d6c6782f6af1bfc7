"""tests/roc_ref.py -- the NumPy statement of the all-pairs verification counts that the GPU tests compare against -- and
the array arithmetic of evaluation/verification.py, checked against what they restate: the reference's calculate_val_far on
a list of all pairs, the float64 comparison for the `up32` rule, and the written rules.  No GPU."""
import numpy as np

import golden_inputs as gi
import roc_ref
from oracle import evalproto as oe
from deep_insight_face import oneshot
from deep_insight_face.evaluation import verification as ver


def _small(metric, b=8, g=300):
    probes, gal = gi.match_tie_inputs()
    probes, gal = probes[:b], gal[:g]
    full = roc_ref.distances(probes, gal, metric)
    rng = np.random.default_rng(3)
    rl = (np.arange(g) // 4).astype(np.int64)
    pl = rng.integers(0, 8, b).astype(np.int64)
    return full, pl, rl


def test_counts_full_is_the_direct_statement():
    for metric in (0, 1):
        full, pl, rl = _small(metric)
        t = np.concatenate([np.arange(0, 2, 0.05), [-1.0, np.inf, -np.inf, 0.3, 0.3], full[0, :5].astype(np.float64)])
        fr = np.random.default_rng(4).integers(-3, 320, full.shape[0])
        for first_row, base in ((None, 0), (fr, 0), (fr + 1000, 1000)):
            a, tot = roc_ref.counts_full(full, pl, rl, t, first_row, base)
            a2, tot2 = roc_ref.counts_direct(full, pl, rl, t, first_row, base)
            assert np.array_equal(a, a2) and np.array_equal(tot, tot2)
        tot = roc_ref.counts_full(full, pl, rl, t)[1]
        assert tot[0] > 0 and tot[1] > 0 and tot[0] + tot[1] == full.size


def test_val_far_is_the_reference_on_a_list_of_all_pairs():
    for metric in (0, 1):
        full, pl, rl = _small(metric)
        issame = (pl[:, None] == rl[None, :]).reshape(-1)
        thresholds = np.arange(0, 4, 0.01) if metric == 0 else np.arange(0, 1.2, 0.01)
        accept, totals = roc_ref.counts_full(full, pl, rl, thresholds)
        val, far = ver.val_far(accept, totals)
        for j, t in enumerate(thresholds):
            assert (val[j], far[j]) == oe.calculate_val_far(t, full.reshape(-1), issame)
    # the zero-denominator rule: no genuine pair, or no impostor pair
    accept, totals = roc_ref.counts_full(full, np.full(full.shape[0], 10 ** 6), rl, [0.5])
    assert ver.val_far(accept, totals)[0][0] == 0 == oe.calculate_val_far(0.5, full.reshape(-1), np.zeros(full.size, bool))[0]
    accept, totals = roc_ref.counts_full(full, np.zeros(full.shape[0], np.int64), np.zeros(full.shape[1], np.int64), [0.5])
    assert ver.val_far(accept, totals)[1][0] == 0 == oe.calculate_val_far(0.5, full.reshape(-1), np.ones(full.size, bool))[1]


def test_up32_is_the_float64_comparison():
    for up32 in (roc_ref.up32, oneshot.up32):
        for t64 in (0.01, 0.3, 0.7, 1.0, 0.0, -0.25, 1e-50, 1e30, -1e30, np.inf, -np.inf):
            t32 = np.float32(t64)
            d = np.array([np.nextafter(t32, np.float32(-np.inf)), t32, np.nextafter(t32, np.float32(np.inf))], dtype=np.float32)
            want = d.astype(np.float64) < np.float64(t64)
            u = up32(np.array([t64]))[0]
            assert u.dtype == np.float32
            assert np.array_equal(d < u, want), (t64, u)
            assert np.float64(u) >= t64 and (np.isinf(u) or np.float64(np.nextafter(u, np.float32(-np.inf))) < t64)
        assert np.isnan(up32(np.array([np.nan]))[0])
        # rounding to nearest would differ: float32(0.01) < 0.01 and float32(0.7) < 0.7 in double
        assert up32(np.array([0.01]))[0] > np.float32(0.01) and up32(np.array([0.7]))[0] > np.float32(0.7)
        assert up32(np.array([0.3]))[0] == np.float32(0.3)     # float32(0.3) > 0.3


def test_rules():
    full, pl, rl = _small(1)
    B, G = full.shape
    # duplicate thresholds give equal rows
    a, _ = roc_ref.counts_full(full, pl, rl, [0.4, 0.5, 0.4, 0.5])
    assert np.array_equal(a[0], a[2]) and np.array_equal(a[1], a[3]) and not np.array_equal(a[0], a[1])
    # negative labels remove pairs from counts and totals
    pl2, rl2 = pl.copy(), rl.copy()
    pl2[[1, 5]] = -1
    rl2[10:50] = -7
    a2, t2 = roc_ref.counts_full(full, pl2, rl2, [0.5, np.inf])
    keep_p, keep_r = pl2 >= 0, rl2 >= 0
    a3, t3 = roc_ref.counts_full(full[keep_p][:, keep_r], pl2[keep_p], rl2[keep_r], [0.5, np.inf])
    assert np.array_equal(a2, a3) and np.array_equal(t2, t3) and t2[:2].sum() == keep_p.sum() * keep_r.sum()
    # first_row = own + 1 over a whole set: n (n - 1) / 2 pairs
    _, gal = gi.match_tie_inputs()
    gal = gal[:97]
    sq = roc_ref.distances(gal, gal, 0)
    lab = np.arange(97) // 3
    a, t = roc_ref.counts_full(sq, lab, lab, [np.inf], first_row=np.arange(97) + 1)
    assert t[0] + t[1] == 97 * 96 // 2 == a[0].sum() and t[0] == 32 * 3 + 0
    iu = np.triu_indices(97, 1)
    assert a[0, 0] == np.sum(lab[iu[0]] == lab[iu[1]])


def test_nan_rows_are_in_the_totals_and_in_no_accept():
    name, probes, gal = [c for c in gi.match_degenerate_cases() if c[0] == 'zero_rows'][0]
    full = roc_ref.distances(probes[:6], gal, 1)
    assert np.isnan(full[:, 417]).all()
    rl = np.arange(gal.shape[0]) // 4
    pl = np.array([417 // 4, 1500 // 4, 0, 1, 2, 3])
    a, t = roc_ref.counts_full(full, pl, rl, [0.5, 1.0, 2.0, np.inf])
    nan = np.isnan(full)
    same = pl[:, None] == rl[None, :]
    assert t[2] == np.sum(nan & same) >= 3 and t[3] == np.sum(nan & ~same) >= 5 * 6 - 3
    assert np.array_equal(a[-1], [t[0] - t[2], t[1] - t[3]])    # +inf accepts every distance that is not NaN, and no NaN


def test_tar_at_far():
    # 10 genuine pairs, 1000 impostor pairs; FAR at the four thresholds: 0, 1e-3, 5e-3, 0.1
    accept = np.array([[2, 0], [5, 1], [7, 5], [10, 100]])
    totals = np.array([10, 1000, 0, 0])
    thresholds = [0.1, 0.2, 0.3, 0.4]
    thr, tar = ver.tar_at_far(accept, totals, thresholds, [1e-4, 1e-3, 2e-3, 5e-3, 0.5])
    assert np.isnan(thr[0]) and np.isnan(tar[0])               # 1 / 1000 > 1e-4: not resolvable
    assert np.array_equal(thr[1:], [0.2, 0.2, 0.3, 0.4]) and np.array_equal(tar[1:], [0.5, 0.5, 0.7, 1.0])
    thr, tar = ver.tar_at_far(accept[1:], totals, thresholds[1:], [1e-3 - 1e-9, 1e-3])
    assert np.isnan(thr[0]) and thr[1] == 0.2
    thr, tar = ver.tar_at_far(accept[2:], totals, thresholds[2:], [2e-3])   # resolvable, but no listed threshold reaches it
    assert np.isnan(thr[0]) and np.isnan(tar[0])
    thr, tar = ver.tar_at_far(accept, np.array([10, 0, 0, 0]), thresholds, [0.1])   # no impostor pair at all
    assert np.isnan(thr[0])
