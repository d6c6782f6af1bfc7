"""The bounds tests/test_embed_gpu.py holds the ArcMargin kernel to (tests/arcmargin_bounds.py derives them from the kernel's
operations) are met by the oracle's own formula evaluated in float32 by NumPy -- other summation orders, no fused operations --
on every case the device is run on.  Runs without a GPU."""
import numpy as np
import pytest

import arcmargin_bounds as ab
from oracle import nets


def _f32_logits(e, w, labels, s, m):
    assert e.dtype == np.float32 and w.dtype == np.float32
    plain = nets.arcmargin_logits(e, w, s=s, m=m)
    ok = (labels >= 0) & (labels < w.shape[0])
    labelled = plain.copy()                                    # a label outside [0, C) names no column
    labelled[ok] = nets.arcmargin_logits(e[ok], w, labels[ok], s=s, m=m)
    assert plain.dtype == np.float32 and labelled.dtype == np.float32
    return plain, labelled


@pytest.mark.parametrize('B,C,D,s,m', [shape + ab.HEADS[0] for shape in ab.SHAPES] + [ab.SHAPES[1] + ab.HEADS[1]])
def test_float32_numpy_meets_the_general_gates(B, C, D, s, m):
    e, w, labels = ab.general_case(B, C, D)
    plain, labelled = _f32_logits(e, w, labels, s, m)
    ab.check_general(plain, labelled, e, w, labels, s, m)
    # the float64 values the gates are centred on are the oracle's
    want = nets.arcmargin_logits(e.astype(np.float64), w.astype(np.float64), labels, s=s, m=m)
    rows = np.arange(B)
    np.testing.assert_allclose(ab.label_gate(e, w, labels, s, m)[0], want[rows, labels], rtol=0, atol=1e-9)
    want[rows, labels] = nets.arcmargin_logits(e.astype(np.float64), w.astype(np.float64), s=s, m=m)[rows, labels]
    np.testing.assert_allclose(ab.plain_gate(e, w, s)[0], want, rtol=0, atol=1e-9)


def test_float32_numpy_meets_the_planted_gates():
    e, w, labels = ab.planted_case()
    plain, labelled = _f32_logits(e, w, labels, ab.PLANT_S, ab.PLANT_M)
    ab.check_planted(plain, labelled, e, w, labels)
