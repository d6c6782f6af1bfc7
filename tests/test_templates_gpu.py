"""Template pooling on the device (csrc/templates.hip, deep_insight_face.templates) against tests/templates_ref.py, bit for
bit: labels, counts, index, sums, wsum, the raw means and the normalised templates.

"Bit for bit" compares the uint32 views; two NaNs count as equal whatever their sign and payload (0/0 is -NaN on the host
and +NaN on the device; NumPy promises neither).

Every case asserts on the CPU, before the device is asked, that its input can tell a wrong evaluation from the right one:
the reference summed in REVERSED row order differs in bits on at least half of the templates of three rows or more, and
for weighted cases an FMA-contracted evaluation differs from the reference somewhere.

The sizes follow the code: the sort's tile (kSortThreads * kSortItems keys per block) and the reduction's look-ahead
(kLookAhead rows per chunk behind a segment's first row) are read from the source."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import templates_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, 'deep-insight-face_amd', 'csrc', 'templates.hip')).read()


def _const(name):
    return int(re.search(r'constexpr int %s = (\d+);' % name, _SRC).group(1))


TILE = _const('kSortThreads') * _const('kSortItems')
LOOK = _const('kLookAhead')
I64MAX = np.iinfo(np.int64).max


def rows_of(rng, n, d):
    """The issue's draw: randn * 10 ** uniform(-3, 3) per row."""
    return (rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float32:
        return np.array_equal(got, want)
    return bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def reference(x, labels, w=None):
    """The reference pool of one add, after the input conditions have been asserted."""
    d = x.shape[1]
    ref = R.RefPool(d, w is not None)
    ref.add(x, labels, w)
    rev = R.RefPool(d, w is not None)
    rev.add(x, labels, w, reverse=True)
    long = ref.counts >= 3
    differ = np.any(bits(ref.sums) != bits(rev.sums), axis=1)
    assert 2 * int(differ[long].sum()) >= int(long.sum()), 'a reversed sum would pass on this input'
    if w is not None:
        fused = R.RefPool(d, True)
        fused.add(x, labels, w, contracted=True)
        assert np.any(bits(fused.sums) != bits(ref.sums)), 'a contracted multiply-add would pass on this input'
    return ref


def t2n(t):
    return t.cpu().numpy()


def check_pool(pool, ref, what=''):
    assert same(t2n(pool.labels), ref.labels), what
    assert same(t2n(pool.counts), ref.counts), what
    assert same(t2n(pool.sums), ref.sums), what
    if ref.weighted:
        assert same(t2n(pool.wsum), ref.wsum), what
    assert len(pool) == ref.labels.shape[0]
    assert same(t2n(pool.templates(normalize=False)), ref.templates(False)), what
    assert same(t2n(pool.templates()), ref.templates(True)), what


def run_case(cuda, x, labels, w=None):
    from deep_insight_face.templates import TemplatePool
    ref = reference(x, labels, w)
    want_index = np.where(labels >= 0, np.searchsorted(ref.labels, np.maximum(labels, 0)), -1).astype(np.int64)
    pool = TemplatePool(x.shape[1], weighted=w is not None)
    try:
        index = pool.add(x, labels, w)
        assert isinstance(index, np.ndarray) and same(index, want_index)
        check_pool(pool, ref)
    finally:
        pool.close()
    return ref


def interleaved(rng, n, n_labels, negatives=True):
    labels = rng.integers(0, max(n_labels, 1), n).astype(np.int64) * 3 + 1
    if negatives and n > 4:
        labels[rng.random(n) < 0.1] = -rng.integers(1, 5)
    return labels


@pytest.mark.parametrize('d', [32, 96, 512])
@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 70001])
def test_sizes(cuda, n, d):
    rng = np.random.default_rng(1000 + n + d)
    run_case(cuda, rows_of(rng, n, d), interleaved(rng, n, n // 5 + 1))


def test_all_distinct_labels(cuda):
    rng = np.random.default_rng(1)
    n = 70001
    ref = run_case(cuda, rows_of(rng, n, 32), rng.permutation(n).astype(np.int64) * 5 + 2)
    assert ref.labels.shape[0] == n


def test_one_label_one_long_segment(cuda):
    rng = np.random.default_rng(2)
    ref = run_case(cuda, rows_of(rng, 70001, 96), np.full((70001,), 12345, np.int64))
    assert ref.counts.tolist() == [70001]


@pytest.mark.parametrize('n', [1, 257, TILE + 1])
def test_all_negative_labels(cuda, n):
    rng = np.random.default_rng(3)
    ref = run_case(cuda, rows_of(rng, n, 32), -rng.integers(1, 1 << 40, n).astype(np.int64))
    assert ref.labels.shape[0] == 0


@pytest.mark.parametrize('d', [32, 96, 512])
def test_segment_lengths_around_the_look_ahead(cuda, d):
    """A segment's first row starts the sum; the rest goes in chunks of LOOK rows."""
    rng = np.random.default_rng(4 + d)
    lengths = [1, 2, 3, LOOK - 1, LOOK, LOOK + 1, LOOK + 2, 2 * LOOK - 1, 2 * LOOK, 2 * LOOK + 1, 2 * LOOK + 2, 3 * LOOK + 1] * 3
    labels = np.repeat(rng.permutation(len(lengths)).astype(np.int64) * 7, lengths)
    labels = labels[rng.permutation(labels.shape[0])]
    ref = run_case(cuda, rows_of(rng, labels.shape[0], d), labels)
    assert sorted(ref.counts.tolist()) == sorted(lengths)


def test_one_long_segment_among_singletons(cuda):
    rng = np.random.default_rng(5)
    labels = np.concatenate([np.full((3000,), 77, np.int64), 100 + np.arange(500, dtype=np.int64)])
    labels = labels[rng.permutation(labels.shape[0])]
    ref = run_case(cuda, rows_of(rng, labels.shape[0], 512), labels)
    assert ref.counts.max() == 3000 and ref.labels.shape[0] == 501


def test_wide_labels_mixed_with_negatives(cuda):
    rng = np.random.default_rng(6)
    pick = np.array([0, 1, 255, 256, 2 ** 31, 2 ** 40 + 3, I64MAX, -1, -2 ** 40, np.iinfo(np.int64).min], np.int64)
    labels = pick[rng.integers(0, pick.shape[0], 700)]
    ref = run_case(cuda, rows_of(rng, 700, 96), labels)
    assert ref.labels.tolist() == [0, 1, 255, 256, 2 ** 31, 2 ** 40 + 3, I64MAX]


@pytest.mark.parametrize('negatives', [False, True])
def test_labels_that_differ_in_byte_five_only(cuda, negatives):
    """Seven of the eight digits are constant over the labels: their passes are skipped."""
    rng = np.random.default_rng(7)
    labels = (rng.integers(0, 256, 3000).astype(np.int64) << 40) + 0x0301000000A7
    if negatives:
        labels[rng.random(3000) < 0.2] = -1
    ref = run_case(cuda, rows_of(rng, 3000, 32), labels)
    assert ref.labels.shape[0] == 256


@pytest.mark.parametrize('d', [32, 96, 512])
def test_weighted(cuda, d):
    rng = np.random.default_rng(8 + d)
    n = 2500
    labels = interleaved(rng, n, 200)
    w = (1.0 - rng.random(n)).astype(np.float32)                 # (0, 1]
    assert w.min() > 0 and w.max() <= 1
    kept = np.unique(labels[labels >= 0])
    for label, bad in zip(kept[[3, 50, 120]], [0.0, np.nan, np.inf]):
        w[np.flatnonzero(labels == label)[1]] = bad              # three templates, one planted weight each
    ref = run_case(cuda, rows_of(rng, n, d), labels, w)
    assert np.isnan(ref.wsum).sum() == 1 and np.isinf(ref.wsum).sum() == 1


def test_weights_that_sum_to_zero(cuda):
    rng = np.random.default_rng(9)
    labels = np.array([4, 9, 4, 9, 9, 9, 9], np.int64)
    w = np.array([0, 0.3, 0, 0.7, 0.9, 0.11, 0.6], np.float32)
    ref = run_case(cuda, rows_of(rng, 7, 32), labels, w)
    assert np.isnan(ref.templates(False)[0]).all()


def test_special_rows(cuda):
    rng = np.random.default_rng(10)
    n, d = 1200, 96
    x = rows_of(rng, n, d)
    labels = interleaved(rng, n, 100)
    kept = np.unique(labels[labels >= 0])
    x[np.flatnonzero(labels == kept[2])[0], 5] = np.nan
    x[np.flatnonzero(labels == kept[7])[1], ::3] = np.inf
    x[np.flatnonzero(labels == kept[9])[0], 1] = -np.inf
    both = np.flatnonzero(labels == kept[11])[:2]
    x[both[0], 0], x[both[1], 0] = np.inf, -np.inf                # Inf - Inf inside a sum
    x[labels == kept[20]] = -0.0                                  # a sum that starts at its first row stays -0
    x = np.concatenate([x, x[:1] * 3, x[:1] * -3])                # a template of v and -v: mean exactly zero
    labels = np.concatenate([labels, [2 ** 33, 2 ** 33]]).astype(np.int64)
    ref = run_case(cuda, x, labels)
    assert np.all(ref.sums[-1] == 0) and np.isnan(ref.templates()[-1]).all()
    assert np.all(bits(ref.templates(False)[20]) == 0x80000000) and np.isnan(ref.templates()[20]).all()


@pytest.mark.parametrize('weighted', [False, True])
def test_three_adds_equal_one_add(cuda, weighted):
    from deep_insight_face.templates import TemplatePool
    rng = np.random.default_rng(11)
    d = 96
    first = rng.integers(10, 20, 900).astype(np.int64) * 10                      # stored: 100, 110, .. 190
    second = np.concatenate([rng.integers(10, 20, 300) * 10 + 5,                  # between the stored ones
                             rng.integers(0, 5, 200), rng.integers(1000, 1005, 200),   # before and after them
                             rng.integers(10, 20, 300) * 10, np.full((60,), -1)]).astype(np.int64)
    second = second[rng.permutation(second.shape[0])]
    first[rng.random(900) < 0.05] = -3
    labels = [first, second, None]
    ref, pool = R.RefPool(d, weighted), TemplatePool(d, weighted=weighted)
    xs, ws = [], []
    try:
        for k in range(3):
            if k == 2:                                                          # the third add touches stored labels only
                labels[2] = ref.labels[rng.integers(0, ref.labels.shape[0], 2100)]
            n = labels[k].shape[0]
            xs.append(rows_of(rng, n, d))
            ws.append((1.0 - rng.random(n)).astype(np.float32) if weighted else None)
            t_before = ref.labels.shape[0]
            want = ref.add(xs[k], labels[k], ws[k])
            got = pool.add(torch.from_numpy(xs[k]).to(cuda), torch.from_numpy(labels[k]).to(cuda),
                           torch.from_numpy(ws[k]).to(cuda) if weighted else None)
            assert torch.is_tensor(got) and same(t2n(got), want), k
            live = labels[k] >= 0
            assert np.array_equal(t2n(pool.labels)[t2n(got)[live]], labels[k][live])     # index names the post-add rows
            assert (ref.labels.shape[0] > t_before) == (k < 2)
            check_pool(pool, ref, 'after add %d' % k)
        x, lab = np.concatenate(xs), np.concatenate(labels)
        w = np.concatenate(ws) if weighted else None
        one = reference(x, lab, w)
        check_pool(pool, one, 'against one add of the concatenation')
    finally:
        pool.close()


def test_two_identical_calls_give_identical_tensors(cuda):
    from deep_insight_face.templates import pool_templates
    rng = np.random.default_rng(12)
    n = 3 * TILE + 77
    x = torch.from_numpy(rows_of(rng, n, 512)).to(cuda)
    labels = torch.from_numpy(interleaved(rng, n, 300)).to(cuda)
    w = torch.from_numpy((1.0 - rng.random(n)).astype(np.float32)).to(cuda)
    a = pool_templates(x, labels, w)
    b = pool_templates(x, labels, w)
    for p, q in zip(a, b):
        assert p.dtype == q.dtype and same(t2n(p), t2n(q))


def test_element_offsets_beyond_two_to_the_31(cuda):
    """4.3 M rows of 512 floats: the rows' and the sums' element offsets pass 2^31.  All labels distinct but the last three
    rows', so the expectation needs no sum but one and is a gather on the device."""
    from deep_insight_face.templates import TemplatePool
    n, d = (1 << 22) + (1 << 17), 512
    assert (n - 3) * d > 2 ** 31
    g = torch.Generator(device=cuda).manual_seed(17)
    x = torch.randn((n, d), device=cuda, generator=g)
    labels = torch.randperm(n, device=cuda, generator=g)
    labels[-3:] = n + 5
    pool = TemplatePool(d)
    try:
        index = pool.add(x, labels)
        order = torch.argsort(labels[:-3])
        assert len(pool) == n - 2
        assert torch.equal(pool.labels[:-1], labels[:-3][order]) and pool.labels[-1].item() == n + 5
        assert torch.equal(index[:-3][order], torch.arange(n - 3, device=cuda)) and index[-3:].tolist() == [n - 3] * 3
        assert bool((pool.counts[:-1] == 1).all()) and pool.counts[-1].item() == 3
        assert torch.equal(pool.sums[:-1].view(torch.int32), x[:-3][order].view(torch.int32))
        last = (x[-3] + x[-2]) + x[-1]
        assert torch.equal(pool.sums[-1].view(torch.int32), last.view(torch.int32))
        means = pool.templates(normalize=False)
        assert same(t2n(means[-1]), t2n(last) / np.float32(3))
        assert torch.equal(means[n - 100:-1].view(torch.int32), pool.sums[n - 100:-1].view(torch.int32))
    finally:
        pool.close()


def test_one_add_is_one_host_read(cuda, monkeypatch):
    from deep_insight_face.templates import TemplatePool
    rng = np.random.default_rng(13)
    n = TILE + 300
    xh, lh = rows_of(rng, n, 32), interleaved(rng, n, 60)
    x, labels = torch.from_numpy(xh).to(cuda), torch.from_numpy(lh).to(cuda)
    reads = []
    read = TemplatePool._read_total

    def counted(t_dev):
        torch.cuda.set_sync_debug_mode('default')
        try:
            reads.append(read(t_dev))
        finally:
            torch.cuda.set_sync_debug_mode('error')
        return reads[-1]

    monkeypatch.setattr(TemplatePool, '_read_total', staticmethod(counted))
    pool = TemplatePool(32)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')          # any other synchronising call of torch raises from here on
    try:
        index = pool.add(x[:n // 2], labels[:n // 2])
        index2 = pool.add(x[n // 2:], labels[n // 2:])
        tpl = pool.templates()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    ref = reference(xh, lh)
    assert reads == [np.unique(lh[:n // 2][lh[:n // 2] >= 0]).shape[0], ref.labels.shape[0]]
    assert same(t2n(tpl), ref.templates()) and index.shape[0] + index2.shape[0] == n
    pool.close()


def _frame_faces(cuda, rng, m, d):
    from deep_insight_face.detector.faces import FrameFaces
    emb = rows_of(rng, m, d)
    scores = (1.0 - rng.random(m)).astype(np.float32)
    z = torch.zeros
    faces = FrameFaces(offsets=torch.tensor([0, m], device=cuda), frame=z((m,), dtype=torch.int64, device=cuda),
                       boxes=z((m, 4), device=cuda), scores=torch.from_numpy(scores).to(cuda), landmarks=None,
                       crops=z((m, 8, 8, 3), dtype=torch.uint8, device=cuda), emb=torch.from_numpy(emb).to(cuda))
    return faces, emb, scores


@pytest.mark.parametrize('weighted', [False, True])
def test_frame_faces_templates(cuda, weighted):
    rng = np.random.default_rng(14)
    m, d = 90, 512
    faces, emb, scores = _frame_faces(cuda, rng, m, d)
    labels = rng.choice(np.array([-1, 0, 4, 5, 17, 40], np.int64), m)        # dbscan's: the smallest core row, -1 = noise
    ref = reference(emb, labels, scores if weighted else None)
    for normalize in (True, False):
        tpl, tl, counts = faces.templates(torch.from_numpy(labels).to(cuda), weighted=weighted, normalize=normalize)
        assert tpl.is_cuda and same(t2n(tpl), ref.templates(normalize))
        assert same(t2n(tl), ref.labels) and same(t2n(counts), ref.counts)
    tpl, tl, counts = faces.templates(labels)                                 # labels from the host are taken too
    assert same(t2n(tpl), R.pool_templates(emb, labels)[0])


def test_frame_faces_templates_without_faces(cuda):
    faces, _, _ = _frame_faces(cuda, np.random.default_rng(15), 0, 128)
    tpl, tl, counts = faces.templates(torch.empty((0,), dtype=torch.int64, device=cuda))
    assert tuple(tpl.shape) == (0, 128) and tpl.dtype == torch.float32 and tpl.is_cuda
    assert tuple(tl.shape) == (0,) and tl.dtype == torch.int64 and tuple(counts.shape) == (0,) and counts.dtype == torch.int64
    with pytest.raises(ValueError):
        faces._replace(emb=None).templates(torch.empty((0,), dtype=torch.int64))


def test_gallery_of_templates(cuda):
    from deep_insight_face import oneshot
    from deep_insight_face.templates import pool_templates
    rng = np.random.default_rng(16)
    n, d, ids = 4000, 128, 400
    centres = rng.standard_normal((ids, d)).astype(np.float32)
    labels = rng.integers(0, ids, n).astype(np.int64)
    x = (centres[labels] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    ref = reference(x, labels)
    tpl, tl, counts, index = pool_templates(x, labels)
    assert isinstance(tpl, np.ndarray) and same(tpl, ref.templates()) and same(tl, ref.labels) and same(counts, ref.counts)
    probes = (centres[::7] + 0.3 * rng.standard_normal(centres[::7].shape)).astype(np.float32)
    for metric in (0, 1):
        got = oneshot.Gallery(tpl).match(probes, metric)
        want = oneshot.Gallery(ref.templates()).match(probes, metric)
        assert np.array_equal(got[0], want[0]) and same(got[1], want[1])
    assert np.mean(tl[got[0]] == np.arange(ids)[::7]) > 0.95                 # and the templates are the identities


def test_python_argument_errors(cuda):
    from deep_insight_face.templates import TemplatePool, pool_templates
    x = np.zeros((6, 32), np.float32)
    labels = np.arange(6)
    w = np.ones((6,), np.float32)
    with pytest.raises(ValueError):
        TemplatePool(33)
    plain, weighted = TemplatePool(32), TemplatePool(32, weighted=True)
    for pool, args in ((plain, (x, labels, w)),                              # weights given to an unweighted pool
                       (weighted, (x, labels)),                              # weights missing on a weighted pool
                       (plain, (x[:, :16], labels)),                         # wrong width
                       (plain, (x[0], labels[:1])),                          # not a matrix
                       (plain, (x, labels[:5])),                             # one label short
                       (plain, (x, labels[None, :])),
                       (plain, (x, labels.astype(np.float32))),              # labels that are no integers
                       (plain, (x, labels > 2)),
                       (plain, (x.astype(np.float64), labels)),              # rows that are not float32
                       (plain, (torch.zeros((6, 32), dtype=torch.float16), labels)),
                       (weighted, (x, labels, w[:5])),
                       (weighted, (x, labels, w.astype(np.float64)))):
        with pytest.raises(ValueError):
            pool.add(*args)
    assert len(plain) == 0 and len(weighted) == 0
    assert plain.add(x, labels.astype(np.int16)).tolist() == list(range(6))  # any integer dtype
    assert plain.add(x, torch.arange(6, dtype=torch.uint8)).tolist() == list(range(6)) and plain.counts.tolist() == [2] * 6
    plain.close()
    weighted.close()
    with pytest.raises(ValueError):
        plain.add(x, labels)
    with pytest.raises(ValueError):
        pool_templates(x[0], labels)


def test_c_abi_argument_errors(cuda):
    from deep_insight_face import _native as N
    i64, f32 = dict(dtype=torch.int64, device=cuda), dict(dtype=torch.float32, device=cuda)
    stream = N.stream_ptr()

    def fails(rc):
        assert rc == -1 and N.last_error()

    h = ctypes.c_void_p()
    fails(N.lib.dif_pool_create(None, 32))
    for d in (0, -32, 48):
        fails(N.lib.dif_pool_create(ctypes.byref(h), d))
    assert N.lib.dif_pool_create(ctypes.byref(h), 32) == 0
    n = 10
    labels = torch.tensor([5, 5, 9, -1, 9, 9, 2, 2, 5, 7], **i64)
    rows = torch.ones((n, 32), **f32)
    index, t_dev = torch.empty((n,), **i64), torch.empty((1,), **i64)
    out = dict(labels=torch.empty((n,), **i64), sums=torch.full((n, 32), -7.0, **f32), counts=torch.empty((n,), **i64))
    p = N.ptr

    def reduce(t, rows_=rows, sums=out['sums'], handle=h):
        return N.lib.dif_pool_reduce(handle, None, None, None, p(rows_) if rows_ is not None else None, None, t, p(out['labels']),
                                     p(sums) if sums is not None else None, None, p(out['counts']), stream)

    fails(reduce(4))                                                         # no group before it
    fails(N.lib.dif_pool_group(None, None, 0, p(labels), n, p(index), p(t_dev), stream))
    fails(N.lib.dif_pool_group(h, None, 0, p(labels), -1, p(index), p(t_dev), stream))
    fails(N.lib.dif_pool_group(h, None, -1, p(labels), n, p(index), p(t_dev), stream))
    fails(N.lib.dif_pool_group(h, None, 0, p(labels), 2 ** 31, p(index), p(t_dev), stream))
    fails(N.lib.dif_pool_group(h, p(labels), 2 ** 30, p(labels), 2 ** 30, p(index), p(t_dev), stream))
    fails(N.lib.dif_pool_group(h, None, 0, None, n, p(index), p(t_dev), stream))
    fails(N.lib.dif_pool_group(h, None, 0, p(labels), n, None, p(t_dev), stream))
    fails(N.lib.dif_pool_group(h, None, 0, p(labels), n, p(index), None, stream))
    fails(N.lib.dif_pool_group(h, None, 3, p(labels), n, p(index), p(t_dev), stream))      # a state without its labels
    fails(reduce(4))                                                         # still none that succeeded
    assert N.lib.dif_pool_group(h, None, 0, p(labels), n, p(index), p(t_dev), stream) == 0
    assert t_dev.item() == 4 and index.tolist() == [1, 1, 3, -1, 3, 3, 0, 0, 1, 2]
    fails(reduce(-1))
    fails(reduce(n + 1))
    fails(reduce(3))                                                         # not what the group wrote
    fails(reduce(5))
    fails(reduce(4, rows_=None))
    fails(reduce(4, sums=None))
    fails(reduce(4, handle=None))
    fails(N.lib.dif_pool_reduce(h, None, None, None, p(rows), p(rows), 4, p(out['labels']), p(out['sums']), None, p(out['counts']),
                                stream))                                     # weights without a place for their sums
    fails(N.lib.dif_pool_reduce(h, None, None, None, ctypes.c_void_p(rows.data_ptr() + 4), None, 4, p(out['labels']), p(out['sums']),
                                None, p(out['counts']), stream))             # rows off the 16-byte grid
    assert bool((out['sums'] == -7.0).all())                                 # nothing was written by the refused calls
    assert reduce(4) == 0
    assert out['labels'][:4].tolist() == [2, 5, 7, 9] and out['counts'][:4].tolist() == [2, 3, 1, 3]
    assert out['sums'][:4, 0].tolist() == [2.0, 3.0, 1.0, 3.0] and bool((out['sums'][4:] == -7.0).all())
    tpl = torch.empty((4, 32), **f32)
    finish = N.lib.dif_pool_finish
    fails(finish(p(out['sums']), None, p(out['counts']), 4, 48, 1, p(tpl), stream))
    fails(finish(p(out['sums']), None, p(out['counts']), -1, 32, 1, p(tpl), stream))
    fails(finish(None, None, p(out['counts']), 4, 32, 1, p(tpl), stream))
    fails(finish(p(out['sums']), None, None, 4, 32, 1, p(tpl), stream))
    fails(finish(p(out['sums']), None, p(out['counts']), 4, 32, 1, None, stream))
    assert finish(p(out['sums']), None, p(out['counts']), 4, 32, 0, p(tpl), stream) == 0
    assert bool((tpl == 1.0).all())
    assert finish(None, None, None, 0, 32, 1, None, stream) == 0             # no template, nothing to do
    assert N.lib.dif_pool_destroy(h) == 0 and N.lib.dif_pool_destroy(None) == 0
