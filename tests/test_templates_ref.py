"""tests/templates_ref.py is NumPy's arithmetic: the sequential float32 loop equals np.mean over the label's rows, its
normalisation equals np.linalg.norm's, and chunked adds equal one add -- bit for bit.  (No GPU.)  The last two tests tie the
feature's layers to each other: header, library, binding table, module."""
import os
import re

import numpy as np
import pytest

import templates_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 9, 129, 4097]


def _case(n, d, seed, n_labels=None):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    labels = rng.integers(-1, n_labels if n_labels else max(1, n // 40) + 1, n).astype(np.int64)
    return x, labels


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('d', [32, 96, 512])
@pytest.mark.parametrize('n', SIZES)
def test_reference_loop_is_np_mean(n, d):
    x, labels = _case(n, d, 100 + n + d)
    labels[0] = 0
    if n == 4097:
        labels[:] = 0                                   # one 4097-row template: the longest sum the issue checked
    tpl, tl, counts, index = R.pool_templates(x, labels, normalize=False)
    assert np.array_equal(tl, np.unique(labels[labels >= 0])) and tl.dtype == np.int64
    assert np.array_equal(index, np.where(labels >= 0, np.searchsorted(tl, np.maximum(labels, 0)), -1))
    for t, l in enumerate(tl):
        rows = x[labels == l]
        assert counts[t] == rows.shape[0]
        assert np.array_equal(_bits(tpl[t]), _bits(np.mean(rows, axis=0))), (n, d, l)
        assert np.array_equal(_bits(tpl[t] * np.float32(1)), _bits(np.add.reduce(rows, axis=0) / np.float32(rows.shape[0])))


@pytest.mark.parametrize('d', [32, 96, 512])
@pytest.mark.parametrize('n', SIZES)
def test_reference_normalisation_is_np_linalg_norm(n, d):
    x, labels = _case(n, d, 200 + n + d)
    labels[0] = 0
    m = R.pool_templates(x, labels, normalize=False)[0]
    got = R.pool_templates(x, labels, normalize=True)[0]
    assert np.array_equal(_bits(got), _bits(m / np.linalg.norm(m, axis=1, keepdims=True)))
    w = np.random.default_rng(n).uniform(0.01, 1.0, n).astype(np.float32)
    m = R.pool_templates(x, labels, w, normalize=False)[0]
    got = R.pool_templates(x, labels, w, normalize=True)[0]
    assert np.array_equal(_bits(got), _bits(m / np.linalg.norm(m, axis=1, keepdims=True)))


def test_zero_mean_template_is_a_nan_row():
    x = np.ones((2, 32), np.float32)
    x[1] = -1
    tpl, tl, counts, _ = R.pool_templates(x, [5, 5])
    assert tl.tolist() == [5] and counts.tolist() == [2] and np.isnan(tpl).all()


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_three_chunked_adds_equal_one_add(n, weighted):
    d = 96
    x, labels = _case(n, d, 300 + n, n_labels=7)
    w = np.random.default_rng(n).uniform(0.01, 1.0, n).astype(np.float32) if weighted else None
    one = R.RefPool(d, weighted)
    index = one.add(x, labels, w)
    three = R.RefPool(d, weighted)
    cuts = [0, n // 3, (2 * n + 2) // 3, n]
    last = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        last = three.add(x[a:b], labels[a:b], None if w is None else w[a:b])
        assert np.array_equal(three.labels[last[last >= 0]], labels[a:b][last >= 0])
    assert np.array_equal(three.labels, one.labels) and np.array_equal(three.counts, one.counts)
    assert np.array_equal(_bits(three.sums), _bits(one.sums))
    if weighted:
        assert np.array_equal(_bits(three.wsum), _bits(one.wsum))
    assert np.array_equal(_bits(three.templates()), _bits(one.templates()))
    assert np.array_equal(last, index[cuts[2]:])


def test_weighted_reference_rounds_the_product_first():
    x, labels = _case(129, 32, 7, n_labels=3)
    w = np.random.default_rng(7).uniform(0.01, 1.0, 129).astype(np.float32)
    pool = R.RefPool(32, True)
    pool.add(x, labels, w)
    for t, l in enumerate(pool.labels):
        rows, ws = x[labels == l], w[labels == l]
        acc, tot = ws[0] * rows[0], ws[0]
        for r in range(1, rows.shape[0]):
            acc, tot = acc + ws[r] * rows[r], tot + ws[r]
        assert np.array_equal(_bits(pool.sums[t]), _bits(acc)) and pool.wsum[t] == tot
    fused = R.pool_templates(x, labels, w, normalize=False, contracted=True)[0]
    assert not np.array_equal(_bits(fused), _bits(pool.means()))


def test_header_library_and_binding_table_carry_the_pool():
    """Fails on a tree without the feature: the five entries declared in include/dif.h, exported by libdif.so and bound in
    _native.SIGNATURES with the header's argument counts."""
    from deep_insight_face import _native
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dif.h')).read(), flags=re.S)
    nargs = {'dif_pool_create': 2, 'dif_pool_destroy': 1, 'dif_pool_group': 8, 'dif_pool_reduce': 12, 'dif_pool_finish': 8}
    for name, k in nargs.items():
        decl = re.search(r'\bint %s\s*\(([^;]*)\);' % name, header, flags=re.S)
        assert decl and decl.group(1).count(',') + 1 == k, name
        assert hasattr(_native.lib, name) and len(_native.SIGNATURES[name][1]) == k, name
    assert re.search(r'typedef struct dif_pool dif_pool;', header)
    assert _native.lib.dif_version() == 110


def test_module_checks_arguments_before_it_needs_a_device():
    from deep_insight_face import templates
    from deep_insight_face.detector.faces import FrameFaces
    with pytest.raises(ValueError):
        templates.TemplatePool(48)
    with pytest.raises(ValueError):
        templates.pool_templates(np.zeros((4,), np.float32), [0, 1, 2, 3])
    assert callable(FrameFaces.templates)
