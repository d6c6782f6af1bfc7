"""Error bounds of the ArcMargin logits against the float64 oracle (oracle.nets.arcmargin_logits), derived from the kernel's
operations (csrc/arcmargin.hip), and the cases tests/test_embed_gpu.py runs the device on.  tests/test_arcmargin_bounds.py
holds the float32 NumPy evaluation of the oracle to the same bounds without a GPU: a bound that plain float32 arithmetic in
another order misses would be fitted to the device, not derived.

u = 2^-24, the unit roundoff of float32.  For embedding e, class centre w, c = e.w / (|e| |w|):

  dot     a D-term chain of float32 multiply-adds on the matrix unit: a term meets at most D additions and one product
          rounding, |dot' - e.w| <= (D + 2) u sum_k |e_k w_k|  (<= (D + 2) u |e| |w|; the sum is evaluated here, in float64)
  1/|x|   |x|^2 by one multiply-add chain per lane (D / 64 terms) and six butterfly additions, every term positive: relative
          error <= (D / 64 + 6) u; halved by the square root, plus its rounding and the division's: <= (D / 128 + 4) u each
  c'      dot' * einv * winv: two products, u / 2 each
  =>      |c' - c| <= u ((D + 2) A + (D / 64 + 9) |c|) (1 + 1e-3),   A = sum_k |e_k w_k| / (|e| |w|) <= 1

and the plain logit s c' adds the rounding of the last product, s |c| u / 2 (none when s is a power of two).

The label column evaluates f(c') = c' cm - sqrt(clamp(1 - c'^2, 0, 1)) sm where c' > th = cos(pi - m), c' - mm otherwise.
Given c' (with s a power of two it IS plain / s), the float32 evaluation is within

  E(c') = sm (sqrt(x + 4u) - sqrt(max(x - 4u, 0))) + |cm| u + 8u,   x = max(1 - c'^2, 0)

of f(c') in float64: 4u covers the float32 evaluation of 1 - c'c' (a product and a difference, fused or not), |cm| u the
product c' cm with cm rounded to float32, 8u the square root's rounding, the product with sm, the difference and the scale.
Against the oracle's c the column also carries f's change over [c - d, c + d], d the bound on |c' - c|; f increases with c on
both branches and across the threshold (f jumps from th - mm = -1.117 to -1 there), so the change is taken at the ends."""
import math

import numpy as np

U = 2.0 ** -24
TOL = 1e-5                 # test_embed_gpu.py: the plain logits' gate is s TOL, the label column's s 2e-5, where the bounds are smaller
SHAPES = ((5, 100, 32), (67, 333, 96), (130, 257, 1024), (3, 4097, 2048))       # (B, C, D): tails in both tile dimensions
HEADS = ((64.0, 0.5), (30.0, 0.3))                                              # (s, m); the second head runs on the second shape only


def general_case(B, C, D):
    rng = np.random.default_rng(100 * B + C + D)
    e = rng.standard_normal((B, D)).astype(np.float32)
    w = rng.standard_normal((C, D)).astype(np.float32)
    return e, w, rng.integers(0, C, (B,))


def cos_bound(e, w):
    """-> (c, d): the float64 cosines [B, C] and the bound on |c' - c| of every one."""
    e, w = e.astype(np.float64), w.astype(np.float64)
    D = e.shape[1]
    eh = e / np.sqrt(np.maximum((e * e).sum(1, keepdims=True), 1e-12))
    wh = w / np.sqrt(np.maximum((w * w).sum(1, keepdims=True), 1e-12))
    c = eh @ wh.T
    A = np.abs(eh) @ np.abs(wh).T
    return c, U * ((D + 2) * A + (D / 64 + 9) * np.abs(c)) * (1 + 1e-3)


def margin(c, m):
    """f(c) in float64: the oracle's formula for the label column, before the scale."""
    c = np.asarray(c, dtype=np.float64)
    phi = c * math.cos(m) - np.sqrt(np.clip(1.0 - c * c, 0.0, 1.0)) * math.sin(m)
    return np.where(c > math.cos(math.pi - m), phi, c - math.sin(math.pi - m) * m)


def eval_bound(c, m):
    """E(c): the float32 evaluation of f at a given float32 c against f(c) in float64."""
    x = np.maximum(1.0 - np.asarray(c, dtype=np.float64) ** 2, 0.0)
    return math.sin(m) * (np.sqrt(x + 4 * U) - np.sqrt(np.maximum(x - 4 * U, 0.0))) + abs(math.cos(m)) * U + 8 * U


def plain_gate(e, w, s):
    """-> (want, gate) of the plain logits: the float64 oracle's and the bound per element, s TOL where that is larger."""
    c, d = cos_bound(e, w)
    return s * c, np.maximum(s * TOL, s * (d + np.abs(c) * U))


def label_gate(e, w, labels, s, m):
    """-> (want, gate) of the label column [B]."""
    c, d = cos_bound(e, w)
    rows = np.arange(e.shape[0])
    c, d = c[rows, labels], d[rows, labels]
    lo, hi = np.clip(c - d, -1, 1), np.clip(c + d, -1, 1)
    f = margin(c, m)
    move = np.maximum(margin(hi, m) - f, f - margin(lo, m))
    ev = np.maximum(eval_bound(c, m), np.maximum(eval_bound(lo, m), eval_bound(hi, m)))
    return s * f, np.maximum(s * 2 * TOL, s * (move + ev + U))


def check_general(plain, labelled, e, w, labels, s, m):
    """The gates of one general case on the logits without and with labels (any implementation's)."""
    want, gate = plain_gate(e, w, s)
    assert plain.dtype == np.float32 and plain.shape == want.shape and np.isfinite(plain).all()
    over = np.abs(plain - want) - gate
    assert over.max() <= 0, (over.max(), np.unravel_index(np.argmax(over), over.shape))
    # the arg-max wherever the oracle's best two logits are further apart than twice the bound
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 2 * gate.max(1)
    assert clear.mean() >= 0.9 and np.array_equal(np.argmax(plain, 1)[clear], np.argmax(want, 1)[clear])
    rows = np.arange(e.shape[0])
    lw, lg = label_gate(e, w, labels, s, m)
    over = np.abs(labelled[rows, labels] - lw) - lg
    assert over.max() <= 0, (over.max(), int(np.argmax(over)))
    assert lg.max() <= s * 1e-3                                  # no label cosine sits at the threshold or at +-1
    other = np.ones(want.shape, dtype=bool)
    other[rows, labels] = False
    assert np.array_equal(labelled[other].view(np.uint32), plain[other].view(np.uint32))   # no other column moves


# ------------------------------------------------------------------------------------------------ planted label columns
PLANT_D, PLANT_C, PLANT_S, PLANT_M = 128, 70, 64.0, 0.5
PLANT_ROWS = ('aligned', 'opposed', 'above_th', 'below_th', 'zero_embedding', 'zero_centre', 'label_-1', 'label_C') + \
    ('aligned', 'opposed') * 12      # |c'| rounds above 1 on some of these only: 1 - c'c' < 0 is the clamp's lower end


def planted_case():
    """-> (e [32, 128], w [70, 128], labels [32]): the rows PLANT_ROWS names, one or more per branch of the label column's
    epilogue."""
    rng = np.random.default_rng(7)
    w = rng.standard_normal((PLANT_C, PLANT_D))
    w[33] = 0.0                                                   # a class centre of zeros
    e = rng.standard_normal((len(PLANT_ROWS), PLANT_D))
    labels = np.array([3, 11, 20, 47, 5, 33, -1, PLANT_C] + list(range(34, 58)), dtype=np.int64)
    e[0] = 3.0 * w[3]                                             # c = 1: 1 - c c rounds to either side of 0
    e[1] = -2.0 * w[11]                                           # c = -1: below the threshold, and the same clamp
    for row in range(8, len(PLANT_ROWS)):
        e[row] = (1.0 if PLANT_ROWS[row] == 'aligned' else -1.0) * rng.uniform(0.5, 4.0) * w[labels[row]]
    th = math.cos(math.pi - PLANT_M)
    for row, c in ((2, th + 1e-3), (3, th - 1e-3)):               # a unit vector at cosine c to its label's centre
        wh = w[labels[row]] / np.linalg.norm(w[labels[row]])
        v = e[row] - (e[row] @ wh) * wh
        e[row] = 1.7 * (c * wh + math.sqrt(1.0 - c * c) * v / np.linalg.norm(v))
    e[4] = 0.0
    return e.astype(np.float32), w.astype(np.float32), labels


def check_planted(plain, labelled, e, w, labels):
    """plain / s is the implementation's own cosine (s = 64: the scale is exact); the label column is f of it within E."""
    s, m, C = PLANT_S, PLANT_M, PLANT_C
    want, gate = plain_gate(e, w, s)
    assert np.isfinite(plain).all() and np.isfinite(labelled).all()
    assert (np.abs(plain - want) <= gate).all()
    assert (plain[4] == 0).all() and (plain[:, 33] == 0).all() and (want[4] == 0).all() and (want[:, 33] == 0).all()
    th, mm = math.cos(math.pi - m), math.sin(math.pi - m) * m
    beyond = {'aligned': 0, 'opposed': 0}
    for row, name in enumerate(PLANT_ROWS):
        lab = int(labels[row])
        other = np.ones(C, dtype=bool)
        if not 0 <= lab < C:                                      # no column may move
            assert np.array_equal(labelled[row].view(np.uint32), plain[row].view(np.uint32)), name
            continue
        other[lab] = False
        assert np.array_equal(labelled[row, other].view(np.uint32), plain[row, other].view(np.uint32)), name
        c = float(plain[row, lab]) / s
        got = float(labelled[row, lab])
        phi = c * math.cos(m) - math.sqrt(min(max(1.0 - c * c, 0.0), 1.0)) * math.sin(m)
        fall = c - mm
        takes_phi = name not in ('opposed', 'below_th')
        assert (c > th) == takes_phi, (name, c)
        f, wrong = (phi, fall) if takes_phi else (fall, phi)
        assert abs(got - s * f) <= s * float(eval_bound(c, m)), (name, c, got, s * f)
        assert abs(got - s * wrong) > s * 0.1, (name, c, got)     # the branch, by value: the two are 0.117 apart at th and more elsewhere
        if name in ('aligned', 'opposed'):                        # (D + 2 + D / 64 + 9) u = 8.4e-6: the sine is at the clamp's edge
            assert abs(abs(c) - 1) <= 1e-5, (name, c)
            beyond[name] += abs(c) > 1
        if name in ('above_th', 'below_th'):
            assert 5e-4 < abs(c - th) < 2e-3, (name, c - th)
        if name in ('zero_embedding', 'zero_centre'):             # the oracle's max(sum, 1e-12): cosine 0, the column s cos(pi/2 + m)
            assert c == 0 and abs(got + s * math.sin(m)) <= s * float(eval_bound(0.0, m)), name
    # the lower end of the sine's clamp was met on both branches (its upper end, 1 - 0 = 1, by the zero rows)
    assert beyond['aligned'] >= 1 and beyond['opposed'] >= 1, beyond
