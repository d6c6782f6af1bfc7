"""FrameFaces.tracks / dif_tracks_link on the GPU against tests/tracks_ref.py, bit for bit.  The reference takes its distances
from the library's own evaluation.utility.distance (dif_pairwise: existing code with tests of its own), so link_dist must
carry the same bits; boxes and the rule are the reference's float32 NumPy."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
import tracks_ref as R

pytestmark = pytest.mark.gpu


def _ff(off, boxes, emb, dev):
    from deep_insight_face.detector.faces import FrameFaces
    off = np.asarray(off, np.int64)
    m = int(off[-1])
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return FrameFaces(torch.from_numpy(off).to(dev), torch.from_numpy(frame).to(dev),
                      torch.from_numpy(np.asarray(boxes, np.float32).reshape(m, 4)).to(dev), torch.ones((m,), device=dev), None,
                      torch.zeros((m, 1, 1, 3), dtype=torch.uint8, device=dev),
                      emb=torch.from_numpy(np.ascontiguousarray(emb, np.float32)).to(dev))


def _lib_dist(emb, metric, dev):
    """The library's distances of the pairs (emb_j, emb_i) over the rows of the whole sequence."""
    from deep_insight_face.evaluation import utility
    t = torch.from_numpy(np.ascontiguousarray(emb, np.float32)).to(dev)

    def fn(j, i):
        if len(j) == 0:
            return np.zeros((0,), np.float32)
        jj, ii = torch.as_tensor(j, device=dev), torch.as_tensor(i, device=dev)
        return utility.distance(t[jj], t[ii], metric).cpu().numpy()
    return fn


def _same_floats(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


def _check(got, want, what=''):
    prev, dist, labels, age, n_new, clipped = want[:6]
    assert got.prev.is_cuda and got.labels.dtype == torch.int64 and got.link_dist.dtype == torch.float32
    assert np.array_equal(got.prev.cpu().numpy(), prev), what
    assert _same_floats(got.link_dist.cpu().numpy(), dist), what
    assert np.array_equal(got.labels.cpu().numpy(), labels) and np.array_equal(got.age.cpu().numpy(), age), what
    assert int(got.n_new) == n_new and int(got.clipped) == clipped, what


def _run(dev, off, boxes, emb, tol, min_iou, max_gap, metric, kmax):
    got = _ff(off, boxes, emb, dev).tracks(tol, min_iou, max_gap, metric, max_faces_per_frame=kmax)
    want = R.link(off, boxes, _lib_dist(emb, metric, dev), tol, min_iou, max_gap, kmax)
    _check(got, want)
    return got, want


# ---- shapes ----------------------------------------------------------------------------------------------------------
_shape_case = R.shape_case


SHAPES = ['one', 'two', 'sparse_first', 'sparse_last', 'long_gaps', 'street', 'crowd', 'crowd16']


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('max_gap', [1, 2, 8])
@pytest.mark.parametrize('name', SHAPES)
def test_tracks_equal_the_reference(cuda, name, max_gap, metric):
    (off, boxes, emb), tols, min_iou, kmax = _shape_case(name)
    got, want = _run(cuda, off, boxes, emb, tols[metric], min_iou, max_gap, metric, kmax)
    counts = np.diff(off)
    if name == 'one':
        assert want[0].tolist() == [-1]
    if name == 'two':
        assert want[0].tolist() == [-1, 0] and want[3].tolist() == [1, 2]
    if name.startswith('sparse') or name == 'long_gaps':
        assert counts.max() <= 3 and (counts == 0).sum() >= 3
        frame = np.repeat(np.arange(len(counts)), counts)
        gaps = (frame - frame[np.maximum(want[0], 0)])[want[0] >= 0]
        assert max_gap < 8 or (gaps > 1).any()              # a link across empty frames, where the gap admits one
        assert (want[0] >= 0).any() or name != 'long_gaps'
    if name == 'crowd16':
        assert int(got.clipped) == int(np.maximum(counts - 16, 0).sum()) > 100
        posn = np.arange(off[-1]) - np.repeat(off[:-1], counts)
        assert (want[0][posn >= 16] == -1).all() and not np.isin(np.nonzero(posn >= 16)[0], want[0]).any()
    if name in ('street', 'crowd'):
        assert (want[0] >= 0).sum() > 100 and int(got.clipped) == 0


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('d', sorted(R.DIM_SEEDS))
def test_every_size_class_of_the_embedding(cuda, d, metric):
    """One size per class of tests/embed_dims.py that dif_pairwise admits: n < 8, the 8-wide body with a tail, the first
    splits, a large size, a 65-leaf tree and the largest."""
    off, boxes, emb = R.dim_case(d)
    tols, min_iou, max_gap, kmax = R.DIM_PARAMS
    got, want = _run(cuda, off, boxes, emb, tols[metric], min_iou, max_gap, metric, kmax)
    assert (want[0] >= 0).sum() >= 2 and (want[0] < 0).sum() >= 2


@pytest.mark.parametrize('metric', [0, 1])
def test_the_caps_max_gap_32_and_64_positions(cuda, metric):
    """What the walk's LDS arrays are sized for: 32 ring frames of 64 slots, links across 32 frames, a tail at position 63,
    the first and the last slot range of a face's table row, and the ring wrapping."""
    (off, boxes, emb), tols, min_iou, max_gap, kmax = R.cap_case()
    assert (max_gap, kmax) == (32, 64) and len(off) - 1 > 32 and np.diff(off).max() == 64
    got, want = _run(cuda, off, boxes, emb, tols[metric], min_iou, max_gap, metric, kmax)
    prev = want[0]
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    posn = np.arange(off[-1]) - off[frame]
    gaps = (frame - frame[np.maximum(prev, 0)])[prev >= 0]
    assert (gaps == 32).sum() > 5 and (gaps == 31).sum() > 5 and (gaps == 1).sum() > 50
    assert posn[prev[prev >= 0]].max() == 63 and posn[prev >= 0].max() == 63


# ---- edges -----------------------------------------------------------------------------------------------------------
def _rows(d, n, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


@pytest.mark.parametrize('metric', [0, 1])
def test_tolerance_exactly_on_a_distance(cuda, metric):
    """Two tails, two faces; the tolerance is the larger of the two link distances, bit for bit from utility.distance: both
    link.  One ulp below it the farther pair does not."""
    e = _rows(128, 2, 1)
    emb = np.concatenate([e, e + 0.2 * _rows(128, 2, 2), ])
    emb[3] = e[1] + 0.4 * _rows(128, 1, 3)[0]
    boxes = np.array([[0, 0, 40, 40], [100, 0, 140, 40]] * 2, np.float32)
    off = [0, 2, 4]
    fn = _lib_dist(emb, metric, cuda)
    dd = fn([2, 3], [0, 1])
    assert dd[1] > dd[0] > 0
    got, want = _run(cuda, off, boxes, emb, dd[1], 0.3, 1, metric, 2)
    assert want[0].tolist() == [-1, -1, 0, 1] and _same_floats(want[1][2:], dd)
    got, want = _run(cuda, off, boxes, emb, np.nextafter(dd[1], np.float32(0)), 0.3, 1, metric, 2)
    assert want[0].tolist() == [-1, -1, 0, -1]
    got, want = _run(cuda, off, boxes, emb, float('nan'), 0.3, 1, metric, 2)
    assert want[0].tolist() == [-1] * 4


def test_iou_exactly_on_min_iou(cuda):
    emb = np.tile(_rows(128, 1, 4), (2, 1)) + 0.01 * _rows(128, 2, 5)
    boxes = np.array([[0, 0, 2, 2], [0, 0, 2, 1]], np.float32)
    got, want = _run(cuda, [0, 1, 2], boxes, emb, 10.0, 0.5, 1, 0, 1)
    assert want[0].tolist() == [-1, 0]                      # 0.5 >= 0.5
    got, want = _run(cuda, [0, 1, 2], boxes, emb, 10.0, np.nextafter(np.float32(0.5), np.float32(1)), 1, 0, 1)
    assert want[0].tolist() == [-1, -1]
    # an IoU whose float32 statement differs from the contracted one would move here: ordinary boxes, threshold on the value
    boxes = np.array([[0.1, 0.2, 40.3, 41.7], [3.3, 1.9, 44.1, 40.2]], np.float32)
    v = np.float32(R.iou32(boxes[0], boxes[1]))
    assert _run(cuda, [0, 1, 2], boxes, emb, 10.0, v, 1, 0, 1)[1][0].tolist() == [-1, 0]
    assert _run(cuda, [0, 1, 2], boxes, emb, 10.0, np.nextafter(v, np.float32(1)), 1, 0, 1)[1][0].tolist() == [-1, -1]


def test_min_iou_zero_and_odd_boxes(cuda):
    """min_iou 0 links disjoint boxes, boxes without area (IoU 0) and a box whose NaN corner fminf / fmaxf drop; an area of
    inf - inf makes the IoU NaN, which never links; min_iou above 0 links none of them."""
    inf, nan = np.inf, np.nan
    tails = np.array([[0, 0, 10, 10], [50, 50, 50, 60], [nan, 0, 2, 2], [inf, 0, inf, 2], [0, 0, inf, inf], [5, 5, 1, 1]], np.float32)
    faces = np.array([[200, 200, 210, 210], [50, 50, 50, 60], [0, 0, 2, 2], [0, 0, 2, 2], [0, 0, 2, 2], [1, 1, 5, 5]], np.float32)
    base = _rows(64, 6, 6)
    emb = np.concatenate([base, base + 0.05 * _rows(64, 6, 7)])
    boxes = np.concatenate([tails, faces])
    for min_iou, metric in ((0.0, 0), (0.0, 1), (-0.0, 0), (1e-6, 0)):
        got, want = _run(cuda, [0, 6, 12], boxes, emb, (2.0, 0.2)[metric], min_iou, 1, metric, 6)
        if min_iou > 0:
            assert want[0][6:].tolist() == [-1, -1, -1, -1, -1, 5]        # (5,5,1,1) is (1,1,5,5) with its corners swapped
        else:
            assert (want[0][6:] >= 0).sum() == 5 and 3 not in want[0]     # the NaN tail stays alone


@functools.lru_cache(maxsize=None)
def _degenerate_rows():
    cases = {n: (p, g) for n, p, g in gi.match_degenerate_cases()}
    probes, gal = cases['odd_probes']
    tiny = cases['tiny_huge_rows'][1]
    return np.concatenate([probes[:14], tiny[[50, 700, 2600, 2000, 2500]], gal[:5]]).astype(np.float32)


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('max_gap', [1, 2])
def test_degenerate_embeddings_and_exact_ties(cuda, metric, max_gap):
    """The zero-norm, NaN, inf, tiny and huge rows of the top-k tests, 24 to a frame and the same 24 in every frame, all in
    ONE box: every pair passes the gate, identical rows tie exactly (metric 0: distance 0; inf distances tie too under an
    infinite tolerance) and (i, j) decides; metric 1 of a row with itself follows the reference, NaN above cosine 1 or not."""
    rows = _degenerate_rows()
    emb = np.concatenate([rows, rows[::-1], rows])
    boxes = np.tile(np.array([[10, 10, 50, 50]], np.float32), (len(emb), 1))
    off = np.arange(4) * len(rows)
    tol = np.inf if metric == 0 else 0.6
    got, want = _run(cuda, off, boxes, emb, tol, 0.3, max_gap, metric, len(rows))
    d = want[1][want[0] >= 0]
    assert len(d) > 10 and len(np.unique(d)) < len(d)                  # exact ties among the accepted links
    assert np.isnan(want[1]).sum() > len(rows)                         # rows that nothing may link to


def test_ties_go_to_the_lower_tail_then_the_lower_face(cuda):
    a, b = _rows(128, 1, 8), _rows(128, 1, 9)
    box = np.array([[0, 0, 30, 30]], np.float32)
    for n0, n1 in ((2, 3), (3, 2)):
        emb = np.concatenate([np.tile(a, (n0, 1)), np.tile(a + 0.1 * b, (n1, 1))])
        got, want = _run(cuda, [0, n0, n0 + n1], np.tile(box, (n0 + n1, 1)), emb, 5.0, 0.5, 1, 0, 4)
        assert want[0].tolist() == ([-1, -1, 0, 1, -1] if n0 == 2 else [-1, -1, -1, 0, 1])


# ---- state -----------------------------------------------------------------------------------------------------------
_twelve = R.twelve


def _chunked(dev, cuts, off, boxes, emb, tol, min_iou, max_gap, metric, kmax):
    state, parts, n_new, clipped = None, [], 0, 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = int(off[a]), int(off[b])
        t = _ff(off[a:b + 1] - lo, boxes[lo:hi], emb[lo:hi], dev).tracks(tol, min_iou, max_gap, metric, state, kmax)
        assert t.state.row_base == hi and t.labels.shape == (hi - lo,)
        state = t.state
        parts.append(t)
        n_new, clipped = n_new + int(t.n_new), clipped + int(t.clipped)
    return [torch.cat([getattr(p, k) for p in parts]).cpu().numpy() for k in ('prev', 'link_dist', 'labels', 'age')] + [n_new, clipped]


@pytest.mark.parametrize('kmax', [4, None])
@pytest.mark.parametrize('metric', [0, 1])
def test_chunked_calls_equal_one_call(cuda, metric, kmax):
    """Twelve frames (4 and 5 empty) at max_gap 3: every two-way split, chunks of one frame, a chunk without frames and a
    chunk of nothing but empty frames, each call given the state of the one before, equal one call bit for bit.  kmax None:
    every call sizes its own slots, so the stored frames and the new ones differ in theirs."""
    off, boxes, emb = _twelve()
    tol = (0.6, 0.3)[metric]
    whole = _ff(off, boxes, emb, cuda).tracks(tol, 0.2, 3, metric, max_faces_per_frame=kmax)
    ref = R.link(off, boxes, _lib_dist(emb, metric, cuda), tol, 0.2, 3, kmax or 64)
    _check(whole, ref)
    assert whole.state.row_base == len(boxes)
    frame = np.repeat(np.arange(12), np.diff(off))
    far = (ref[0] >= 0) & (frame - frame[np.maximum(ref[0], 0)] > 1)
    assert far.any() and ref[5] == (0 if kmax is None else int(np.maximum(np.diff(off) - 4, 0).sum()))
    crossing = 0
    for cuts in [[0, s, 12] for s in range(13)] + [list(range(13)), [0, 3, 3, 7, 12], [0, 4, 6, 12], [0, 4, 5, 6, 12]]:
        got = _chunked(cuda, cuts, off, boxes, emb, tol, 0.2, 3, metric, kmax)
        assert np.array_equal(got[0], ref[0]) and _same_floats(got[1], ref[1]), cuts
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]) and got[4:] == [ref[4], ref[5]], cuts
        if len(cuts) == 3:
            crossing += int((far & (frame >= cuts[1]) & (frame[np.maximum(ref[0], 0)] < cuts[1])).sum())
    assert crossing > 0                                     # tracks that survive a gap across a chunk boundary


def test_state_is_not_modified_and_names_its_parts(cuda):
    off, boxes, emb = _twelve()
    first = _ff(off[:7], boxes[:off[6]], emb[:off[6]], cuda).tracks(0.3, 0.2, 3, 1, max_faces_per_frame=4)
    st = first.state
    assert (st.max_gap, st.k, st.d, st.pad, st.row_base) == (3, 4, 32, 0, int(off[6]))
    count = st.count.cpu().numpy()
    assert count.tolist() == np.minimum(np.diff(off)[3:6], 4).tolist()           # frames 3, 4, 5
    lo = int(off[3])
    assert torch.equal(st.emb[:count[0]].cpu(), torch.from_numpy(emb[lo:lo + count[0]]))
    assert st.rows[:count[0]].tolist() == list(range(lo, lo + count[0])) and st.labels[:count[0]].tolist() == first.labels[lo:lo + count[0]].tolist()
    before = st.buf.clone()
    rest = _ff(off[6:] - off[6], boxes[off[6]:], emb[off[6]:], cuda)
    a = rest.tracks(0.3, 0.2, 3, 1, st, 4)
    b = rest.tracks(0.3, 0.2, 3, 1, st, 4)
    assert torch.equal(st.buf, before) and torch.equal(a.labels, b.labels) and torch.equal(a.state.buf, b.state.buf)
    with pytest.raises(ValueError):
        rest.tracks(0.3, 0.2, 2, 1, st, 4)                  # another max_gap than the state's


# ---- plumbing --------------------------------------------------------------------------------------------------------
def test_no_host_read_with_max_faces_given(cuda):
    off, boxes, emb = _twelve()
    ff = _ff(off[:7], boxes[:off[6]], emb[:off[6]], cuda)
    rest = _ff(off[6:] - off[6], boxes[off[6]:], emb[off[6]:], cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        first = ff.tracks(0.3, 0.2, 3, 1, max_faces_per_frame=4)
        second = rest.tracks(0.3, 0.2, 3, 1, first.state, 4)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    ref = R.link(off, boxes, _lib_dist(emb, 1, cuda), 0.3, 0.2, 3, 4)
    assert np.array_equal(torch.cat([first.labels, second.labels]).cpu().numpy(), ref[2])


def test_no_faces_and_no_frames(cuda):
    off, boxes, emb = _twelve()
    none = _ff([0], np.zeros((0, 4)), np.zeros((0, 32)), cuda).tracks(0.3)
    assert none.labels.shape == (0,) and none.labels.is_cuda and none.state.pad == 0 and int(none.n_new) == 0
    # an empty batch of five frames between two halves = five more empty frames in one call
    cut = int(off[6])
    first = _ff(off[:7], boxes[:cut], emb[:cut], cuda).tracks(0.3, 0.2, 8, 1, max_faces_per_frame=4)
    gap = _ff(np.zeros(6, np.int64), np.zeros((0, 4)), np.zeros((0, 32)), cuda).tracks(0.3, 0.2, 8, 1, first.state, 4)
    assert gap.prev.shape == (0,) and gap.state.pad == 5 and gap.state.row_base == cut
    second = _ff(off[6:] - cut, boxes[cut:], emb[cut:], cuda).tracks(0.3, 0.2, 8, 1, gap.state, 4)
    off2 = np.concatenate([off[:7], np.full(5, cut), off[7:]])
    ref = R.link(off2, boxes, _lib_dist(emb, 1, cuda), 0.3, 0.2, 8, 4)
    assert np.array_equal(torch.cat([first.prev, second.prev]).cpu().numpy(), ref[0]) and (ref[0][cut:] >= 0).sum() > 3
    assert np.array_equal(torch.cat([first.age, second.age]).cpu().numpy(), ref[3])
    # the C entry with m = 0: the state moves on, the counts are written
    from deep_insight_face import _native as N
    cnt = torch.full((2,), -1, dtype=torch.int64, device=cuda)
    size = N.lib.dif_tracks_state_size(8, 4, 32)
    out = torch.zeros((size,), dtype=torch.uint8, device=cuda)
    work = torch.empty((N.lib.dif_tracks_workspace_size(0, 8, 4, 4),), dtype=torch.uint8, device=cuda)
    o5 = torch.zeros((6,), dtype=torch.int64, device=cuda)
    N.check(N.lib.dif_tracks_link(N.ptr(o5), None, None, 5, 0, 32, 0.3, 0.2, 8, 1, 4, cut, N.ptr(first.state.buf), 4, 0, None, None, None,
                                  None, N.ptr(cnt), N.ptr(cnt[1:]), N.ptr(out), 4, N.ptr(work), work.shape[0], 0, N.stream_ptr()))
    assert cnt.tolist() == [0, 0]
    moved = first.state._replace(buf=out)
    assert moved.count.tolist() == first.state.count[5:].tolist() + [0] * 5
    third = _ff(off[6:] - cut, boxes[cut:], emb[cut:], cuda).tracks(0.3, 0.2, 8, 1, moved, 4)
    assert torch.equal(third.prev, second.prev) and torch.equal(third.link_dist.view(torch.int32), second.link_dist.view(torch.int32))


def _c_link(N, dev, seq, params, work, /, **over):
    """dif_tracks_link on seq = (offsets, boxes, emb) and params = (tolerance, min_iou, max_gap, metric, kmax) without a state;
    `over` replaces arguments by name (`work` among them, hence the positional-only parameters)."""
    off, boxes, emb = seq
    m, d = emb.shape
    t = dict(off=torch.from_numpy(np.asarray(off, np.int64)).to(dev), boxes=torch.from_numpy(boxes).to(dev), emb=torch.from_numpy(emb).to(dev))
    i64 = dict(dtype=torch.int64, device=dev)
    out = dict(prev=torch.empty((m,), **i64), dist=torch.empty((m,), dtype=torch.float32, device=dev), labels=torch.empty((m,), **i64),
               age=torch.empty((m,), **i64), cnt=torch.empty((2,), **i64))
    a = dict(off=N.ptr(t['off']), boxes=N.ptr(t['boxes']), emb=N.ptr(t['emb']), n=len(off) - 1, m=m, d=d, tol=params[0], min_iou=params[1],
             max_gap=params[2], metric=params[3], kmax=params[4], row_base=0, st=None, st_k=0, pad=0, prev=N.ptr(out['prev']),
             dist=N.ptr(out['dist']), labels=N.ptr(out['labels']), age=N.ptr(out['age']), n_new=N.ptr(out['cnt']),
             clipped=N.ptr(out['cnt'][1:]), so=None, so_k=0, work=N.ptr(work), bytes=work.shape[0], passes=0)
    assert set(over) <= set(a)
    a.update(over)
    rc = N.lib.dif_tracks_link(*a.values(), N.stream_ptr())
    return rc, out


def test_c_entry_argument_errors_and_workspace_reuse(cuda):
    from deep_insight_face import _native as N
    (off, boxes, emb), tols, min_iou, kmax = _shape_case('street')
    (off2, boxes2, emb2), _, _, _ = _shape_case('two')
    need = N.lib.dif_tracks_workspace_size(len(boxes), 8, kmax, 0)
    assert need >= len(boxes) * 8 * kmax * 4 + len(boxes) * 4
    work = torch.empty((need + 8,), dtype=torch.uint8, device=cuda)
    refs = {}
    for which in ('large', 'small', 'large', 'small'):                  # one workspace: large, small, large again
        o, b, e, k = (off, boxes, emb, kmax) if which == 'large' else (off2, boxes2, emb2, 1)
        rc, out = _c_link(N, cuda, (o, b, e), (tols[1], min_iou, 8, 1, k), work)
        assert rc == 0, N.last_error()
        if which not in refs:
            refs[which] = R.link(o, b, _lib_dist(e, 1, cuda), tols[1], min_iou, 8, k)
        want = refs[which]
        assert np.array_equal(out['prev'].cpu().numpy(), want[0]) and _same_floats(out['dist'].cpu().numpy(), want[1])
        assert np.array_equal(out['labels'].cpu().numpy(), want[2]) and out['cnt'].tolist() == [want[4], want[5]]
    bad = [dict(kmax=0), dict(kmax=65), dict(max_gap=0), dict(max_gap=33), dict(metric=2), dict(metric=-1), dict(d=0), dict(d=8193),
           dict(off=None), dict(boxes=None), dict(emb=None), dict(prev=None), dict(dist=None), dict(labels=None), dict(age=None),
           dict(n_new=None), dict(clipped=None), dict(work=None), dict(bytes=need - 256), dict(work=ctypes.c_void_p(work.data_ptr() + 4)),
           dict(m=-1), dict(n=-1), dict(n=0), dict(row_base=-1), dict(pad=-1), dict(passes=8), dict(so=N.ptr(work), so_k=kmax - 1),
           dict(st=N.ptr(work), st_k=0), dict(st=N.ptr(work), st_k=65)]
    for over in bad:
        rc, _ = _c_link(N, cuda, (off, boxes, emb), (tols[1], min_iou, 8, 1, kmax), work, **over)
        assert rc != 0 and N.last_error().startswith('dif_tracks_link'), over
    rc, _ = _c_link(N, cuda, (off, boxes, emb), (tols[1], min_iou, 8, 1, kmax), work)
    assert rc == 0                                          # (and the refused calls left nothing behind that hinders this one)
    torch.cuda.synchronize()


def test_python_argument_errors(cuda):
    off, boxes, emb = _twelve()
    ff = _ff(off, boxes, emb, cuda)
    for bad in (dict(max_gap=0), dict(max_gap=33), dict(max_faces_per_frame=65), dict(max_faces_per_frame=0)):
        with pytest.raises(ValueError):
            ff.tracks(0.3, **bad)
    with pytest.raises(RuntimeError):
        ff.tracks(0.3, distance_metric=2)
    with pytest.raises(ValueError):
        ff._replace(emb=None).tracks(0.3)


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_one_frame_four_times_through_the_pipeline(cuda):
    """The MTCNN pipeline of tests/test_faces_gpu.py on one frame repeated four times: under tolerance 0, min_iou 1 every face
    of frame 0 heads a track of age 4, and templates(labels) pools one template per face of frame 0."""
    from deep_insight_face.detector.mtcnn import MtcnnDetector, MtcnnFramePipeline
    from deep_insight_face.networks.triplet import bottleneck_network
    from test_faces_gpu import _blobs
    emb = bottleneck_network('resnet', emd_size=512, input_shape=(112, 112, 3), max_batch=4)('v2')
    emb.init_synthetic(2024)
    emb.set_input_transform(scale=1 / 255.)
    det = MtcnnDetector((96, 128), max_batch=2, cap=(24, 12, 8)).init_synthetic(2024, logit_scale=1.0)
    frame = torch.from_numpy(_blobs(1, 96, 128, seed=11)).to(cuda)
    ff = MtcnnFramePipeline(det, emb, None, margin=8).faces(frame.repeat(4, 1, 1, 1))
    k = int(ff.offsets[1])
    assert k >= 2 and ff.offsets.tolist() == [0, k, 2 * k, 3 * k, 4 * k]
    t = ff.tracks(tolerance=0, min_iou=1.0, max_gap=1, distance_metric=0)
    assert t.labels.tolist() == list(range(k)) * 4
    assert t.age.tolist() == [a for a in (1, 2, 3, 4) for _ in range(k)]
    assert t.prev.tolist() == [-1] * k + list(range(3 * k)) and int(t.n_new) == k and int(t.clipped) == 0
    assert bool((t.link_dist[k:] == 0).all()) and bool(torch.isnan(t.link_dist[:k]).all())
    tpl, labels, counts = ff.templates(t.labels)
    assert tpl.shape == (k, 512) and labels.tolist() == list(range(k)) and counts.tolist() == [4] * k
    det.close()
    emb.close()
