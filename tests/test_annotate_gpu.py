"""FrameFaces.annotate / annotate_frames / dif_frames_annotate and compose_text / dif_annotate_compose on the GPU against
tests/annotate_ref.py: every comparison is array_equal on the whole output."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import annotate_ref as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _cases():
    return A.cases()


def _dev(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _ff(off, boxes, landmarks, dev, idx=None, dist=None):
    from deep_insight_face.detector.faces import FrameFaces
    off = np.asarray(off, np.int64)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    m = len(boxes)
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return FrameFaces(_dev(off, dev), _dev(frame, dev), _dev(boxes, dev), torch.ones((m,), device=dev), _dev(landmarks, dev),
                      torch.zeros((m, 1, 1, 3), dtype=torch.uint8, device=dev), None, _dev(idx, dev), _dev(dist, dev))


def _run(dev, frames, off, boxes, landmarks=None, text=None, colors=None, select=None, margin=0.0, t=2, s=2, r=1, what=''):
    """One call through FrameFaces.annotate, out of place, against the restatement; -> (got, frames on the device)."""
    fr = _dev(frames, dev)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    per_face = isinstance(colors, np.ndarray)
    got = _ff(off, boxes, landmarks, dev).annotate(fr, text=_dev(text, dev), colors=_dev(colors, dev) if per_face else colors,
                                                   select=_dev(select, dev), margin=margin, thickness=t, scale=s, mark=r)
    assert got.is_cuda and got.dtype == torch.uint8 and got.data_ptr() != fr.data_ptr()
    want = A.annotate(frames, off, boxes, landmarks, text, colors if per_face else None, A.COLOR if colors is None or per_face else colors,
                      select, margin, t, s, r)
    assert np.array_equal(got.cpu().numpy(), want), what
    assert np.array_equal(fr.cpu().numpy(), frames), what                      # the frames are unchanged
    return got, fr


# ---- the generated cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thickness', A.THICKNESSES)
def test_generated_cases(cuda, thickness):
    """Every call of annotate_ref.walk() at one thickness: 8 cases x (scale 1, 2 x mark -1, 0, 2 x margin 0, 0.25, -0.2), with and
    without select and colours in turn, and the margins that empty every region."""
    calls = 0
    for case, t, s, r, margin, use_select, use_colors in A.walk():
        if t != thickness:
            continue
        select, colors = A.call_args(case, use_select, use_colors)
        _run(cuda, case['frames'], case['offsets'], case['boxes'], case['landmarks'], case['text'], colors, select, margin, t, s, r,
             what=(case['name'], t, s, r, margin, use_select, use_colors))
        calls += 1
    assert calls == 8 * (18 + (thickness > 0))


def test_a_frame_of_one_pixel(cuda):
    fr = np.array([[[[10, 200, 31]]]], np.uint8)
    lm = np.zeros((2, 5, 2), np.float32)
    for boxes, text, r, want in (([[-3.0, -2.0, 5.0, 9.0], [0.0, 0.0, 1.0, 1.0]], None, -1, [10, 200, 31]),      # inside both boxes: no paint
                                 ([[1.0, 0.0, 4.0, 1.0], [0.0, 0.0, 1.0, 1.0]], None, -1, [1, 2, 3]),            # the first face's ring
                                 ([[0.0, 0.0, 1.0, 1.0], [0.0, 10.0, 1.0, 11.0]], A.texts([b'', b'8']), -1, [1, 2, 3]),   # a plate's corner
                                 ([[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]], None, 0, [1, 2, 3])):            # a mark
        got, _ = _run(cuda, fr, [0, 2], boxes, lm, text, (1, 2, 3), None, 0.0, 1, 1, r)
        assert got.cpu().numpy().tolist() == [[[want]]]


def test_a_frame_8192_wide_with_a_plate_at_scale_8(cuda):
    rng = np.random.default_rng(9)
    fr = rng.integers(0, 256, (1, 2, 8192, 3), dtype=np.uint8)
    text = A.texts([bytes(rng.integers(0x21, 0x7F, 64).astype(np.uint8).tolist()), b'Wide', b'edge'], 64)
    boxes = [[5000.5, -80.0, 5100.0, -60.0], [-5.0, 0.5, 8200.0, 1.5], [8100.0, -80.0, 8180.0, -60.0]]
    lm = np.array([[[3.2, 0.4], [8191.4, 1.2], [8191.6, 0.0], [-20.0, 1.0], [4000.0, 5.0]]] * 3, np.float32)
    colors = np.array([[255, 255, 255], [0, 0, 0], [90, 200, 30]], np.uint8)
    got, _ = _run(cuda, fr, [0, 3], boxes, lm, text, colors, None, 0.0, 3, 8, 2)
    assert (got.cpu().numpy() != fr).any(3).sum() > 3000                       # the plate of 3080 x 72 reaches down into both rows
    tall = np.ascontiguousarray(fr.transpose(0, 2, 1, 3))
    _run(cuda, tall, [0, 2], [[0.2, 100.0, 1.9, 8000.0], [-9.0, 4000.0, -4.0, 4100.0]], None, A.texts([b'tall', b'left']), None, None, 0.0, 2, 8, -1)


def test_thickness_64(cuda):
    for case in _cases()[:3]:
        for s, margin in ((1, 0.0), (2, -0.2)):
            _run(cuda, case['frames'], case['offsets'], case['boxes'], case['landmarks'], case['text'], case['colors'], case['select'], margin, 64,
                 s, 1, what=case['name'])


def test_more_lower_faces_than_one_block_lists(cuda):
    """One frame whose faces outnumber the block's LDS list by one and by many: the rows beyond it test their lower faces one by one."""
    src = open(os.path.join(ROOT, 'deep-insight-face_amd', 'csrc', 'annotate.hip')).read()
    consts = dict(re.findall(r'constexpr int (kAnn\w+) = (\w+);', src))
    cap = int(consts[consts['kAnnListFaces']]) if not consts['kAnnListFaces'].isdigit() else int(consts['kAnnListFaces'])
    assert cap >= 64
    h, w = 80, 100
    fr = np.random.default_rng(5).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    for m in (cap + 2, cap + 2 + 343):                                          # the last row has cap + 1 lower faces; hundreds of rows have more
        rng = np.random.default_rng(m)
        x, y = rng.uniform(-2, w - 3, m), rng.uniform(-2, h - 3, m)
        boxes = np.stack([x, y, x + rng.uniform(1, 6, m), y + rng.uniform(1, 6, m)], 1).astype(np.float32)
        text = A.texts([bytes(rng.integers(0x21, 0x7F, rng.choice([0, 0, 0, 1, 2])).astype(np.uint8).tolist()) for _ in range(m)], 2)
        lm = A._centre_marks(boxes)
        select = (rng.integers(0, 4, m) == 0).astype(np.uint8)
        select[-1] = select[cap + 1] = 1
        colors = rng.integers(0, 256, (m, 3)).astype(np.uint8)
        _run(cuda, fr, [0, m], boxes, lm, text, colors, select, 0.0, 1, 1, 0)
        own, _, depth = A.owners([0, m], boxes, lm, text, select, 0.0, 1, 1, 0, 1, h, w)
        assert depth.max() >= 3 and (own > cap).any() and (m == cap + 2 or ((own > cap).sum() > 100 and depth[own > cap].max() >= 2))


# ---- in place, out, offsets, nothing to do -------------------------------------------------------------------------------
def test_in_place_equals_out_of_place(cuda):
    for case in _cases()[:3]:
        got, fr = _run(cuda, case['frames'], case['offsets'], case['boxes'], case['landmarks'], case['text'], case['colors'], case['select'], 0.25, 3,
                       1, 2)
        ff = _ff(case['offsets'], case['boxes'], case['landmarks'], cuda)
        same = ff.annotate(fr, text=_dev(case['text'], cuda), colors=_dev(case['colors'], cuda), select=_dev(case['select'], cuda), margin=0.25,
                           thickness=3, scale=1, mark=2, out=fr)
        assert same is fr and torch.equal(fr, got)


def test_out_given_keeps_its_other_bytes(cuda):
    """`out` need not start as a copy of the frames: only the painted pixels are written, and the frames are not read."""
    case = _cases()[1]
    fr = _dev(case['frames'], cuda)
    out = torch.full_like(fr, 99)
    ff = _ff(case['offsets'], case['boxes'], case['landmarks'], cuda)
    assert ff.annotate(fr, text=_dev(case['text'], cuda), select=_dev(case['select'], cuda), out=out) is out
    want = A.annotate(case['frames'], case['offsets'], case['boxes'], case['landmarks'], case['text'], None, A.COLOR, case['select'],
                      out=np.full_like(case['frames'], 99))
    assert np.array_equal(out.cpu().numpy(), want) and (want == 99).any() and (want != 99).any()
    assert np.array_equal(fr.cpu().numpy(), case['frames'])


def test_select_none_all_ones_any_non_zero_all_zeros_and_bool(cuda):
    case = _cases()[1]
    args = (case['frames'], case['offsets'], case['boxes'], case['landmarks'], case['text'], case['colors'])
    m = len(case['boxes'])
    none, fr = _run(cuda, *args, None)
    ones, _ = _run(cuda, *args, np.ones(m, np.uint8))
    many, _ = _run(cuda, *args, np.full(m, 200, np.uint8))
    zeros, _ = _run(cuda, *args, np.zeros(m, np.uint8))
    assert torch.equal(none, ones) and torch.equal(none, many) and torch.equal(zeros, fr)
    pick = np.arange(m) % 2 == 0
    _run(cuda, *args, pick)


def test_offsets_that_cover_only_some_rows(cuda):
    """offsets[n] < m and offsets[0] > 0: the rows outside are in no frame and are left out."""
    from deep_insight_face.detector.annotate import annotate_frames
    case = _cases()[1]
    fr = _dev(case['frames'], cuda)
    off = case['offsets'].copy()
    off[-1] -= 2
    off[0] += 1
    got = annotate_frames(fr, off, case['boxes'], case['landmarks'], case['text'], _dev(case['colors'], cuda), _dev(case['select'], cuda))
    want = A.annotate(case['frames'], off, case['boxes'], case['landmarks'], case['text'], case['colors'], A.COLOR, case['select'])
    assert np.array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(want, A.annotate(case['frames'], case['offsets'], case['boxes'], case['landmarks'], case['text'], case['colors'],
                                               A.COLOR, case['select']))


def _entry(dev, out, off, boxes, landmarks=None, text=None, colors=None, color=(1, 2, 3), select=None, margin=0.0, t=2, s=2, r=1, null=(),
           **sizes):
    """dif_frames_annotate itself -> rc; `null` names the pointers to pass as NULL, `sizes` replaces n, h, w, m or l."""
    from deep_insight_face import _native as N
    n, h, w = out.shape[:3]
    off = torch.as_tensor(np.asarray(off, np.int64)).to(dev)
    bx = torch.as_tensor(np.asarray(boxes, np.float32).reshape(-1, 4)).to(dev)
    lm, tx, cl, se = _dev(landmarks, dev), _dev(text, dev), _dev(colors, dev), _dev(select, dev)
    opt = lambda x: None if x is None else N.ptr(x)
    a = dict(out=N.ptr(out), n=n, h=h, w=w, offsets=N.ptr(off), boxes=N.ptr(bx), m=bx.shape[0], landmarks=opt(lm), text=opt(tx),
             l=1 if tx is None else tx.shape[1], colors=opt(cl), color=(ctypes.c_uint8 * 3)(*color), select=opt(se), margin=margin, t=t, s=s, r=r)
    a.update(sizes)
    a.update({k: None for k in null})
    assert list(a)[:4] == ['out', 'n', 'h', 'w'] and len(a) == 17
    rc = N.lib.dif_frames_annotate(*a.values(), N.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_no_faces_and_no_frames_in_both_layers(cuda):
    from deep_insight_face import _native as N
    from deep_insight_face.detector.annotate import annotate_frames, compose_text
    fr = _dev(_cases()[0]['frames'], cuda)
    i64 = dict(dtype=torch.int64, device=cuda)
    got = annotate_frames(fr, torch.zeros((4,), **i64), torch.zeros((0, 4), device=cuda), text=torch.zeros((0, 8), dtype=torch.uint8, device=cuda))
    assert got.data_ptr() != fr.data_ptr() and torch.equal(got, fr)
    assert annotate_frames(fr, torch.zeros((4,), dtype=torch.int64), torch.zeros((0, 4)), out=fr) is fr
    assert annotate_frames(fr[:0], torch.zeros((1,), **i64), torch.zeros((0, 4), device=cuda)).shape == (0, A.H, A.W, 3)
    empty = _ff([0, 0, 0, 0], [], None, cuda, idx=np.zeros((0,), np.int64), dist=np.zeros((0,), np.float32))
    assert torch.equal(empty.annotate(fr, values=empty.dist), fr)
    text = compose_text(idx=torch.zeros((0,), **i64), length=5)
    assert text.shape == (0, 5) and text.is_cuda and text.dtype == torch.uint8
    marker = torch.full_like(fr, 77)
    assert _entry(cuda, marker, [0, 0, 0, 0], []) == 0 and int(marker.min()) == 77 and int(marker.max()) == 77
    color = (ctypes.c_uint8 * 3)(1, 2, 3)
    assert N.lib.dif_frames_annotate(None, 0, A.H, A.W, None, None, 0, None, None, 1, None, color, None, 0.0, 2, 2, 1, N.stream_ptr()) == 0
    assert N.lib.dif_frames_annotate(N.ptr(marker), 3, A.H, A.W, None, None, 0, None, None, 1, None, color, None, 0.0, 2, 2, 1, N.stream_ptr()) == 0
    assert N.lib.dif_annotate_compose(None, 0, 1, None, None, None, 2, b'?', 0, None, 8, N.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(marker.min()) == 77 and int(marker.max()) == 77


# ---- the label text ------------------------------------------------------------------------------------------------------
def test_compose_on_the_device_equals_the_restatement(cuda):
    from deep_insight_face.detector.annotate import NameTable, compose_text
    rng = np.random.default_rng(31)
    m = 120
    people = ['ann', 'bob', 'christopher', '', 'Zoë Q.']
    values = rng.uniform(-3, 3, m).astype(np.float32)
    values[:12] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 0.005, -0.004, 0.125, -0.125, 99999.5, 1e-9, -123456.0]
    values[12:24] *= 1e4
    known = rng.integers(0, 3, m) > 0
    calls = 0
    for g, ln in ((5, 7), (1, 1), (5, 64)):
        table = NameTable(people[:g], length=ln, device=cuda)
        names = table.names.cpu().numpy()
        assert names.shape == (g, ln)
        idx = rng.integers(-1, g + 1, m)
        for l in (1, 5, 32, 64):
            for decimals, unknown in ((2, '?'), (0, ''), (4, 'x' * 64), (1, 'who')):
                for use in ((1, 1, 1, 1), (1, 1, 0, 1), (1, 1, 0, 0), (0, 1, 0, 1), (0, 0, 1, 1), (0, 0, 0, 1), (1, 0, 1, 0)):
                    if not any(use[1:]):
                        continue
                    n_, i_, k_, v_ = (x if u else None for x, u in zip((names, idx, known, values), use))
                    got = compose_text(table if use[0] else None, _dev(i_, cuda), _dev(k_, cuda), _dev(v_, cuda), decimals, unknown, l)
                    want = A.compose(m, n_, i_, k_, v_, decimals, unknown.encode(), l)
                    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want), (g, ln, l, decimals, unknown, use)
                    calls += 1
    assert calls == 3 * 4 * 4 * 7
    by_bytes = compose_text(table, _dev(idx, cuda), _dev(known.astype(np.uint8) * 200, cuda), length=9)       # any non-zero value is known
    assert np.array_equal(by_bytes.cpu().numpy(), A.compose(m, names, idx, known, l=9))


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_frame_faces_annotate_reads_nothing_back(cuda):
    """names, known = dist <= tol, values = dist and palette colours, composed and drawn under sync debug mode 'error'."""
    from deep_insight_face.detector.annotate import PALETTE, NameTable, palette
    case = _cases()[1]
    m = len(case['boxes'])
    rng = np.random.default_rng(3)
    idx, dist = rng.integers(0, 4, m), rng.uniform(0.05, 0.9, m).astype(np.float32)
    labels = rng.integers(-1, 40, m)
    fr = _dev(case['frames'], cuda)
    ff = _ff(case['offsets'], case['boxes'], case['landmarks'], cuda, idx, dist)
    table = NameTable(['ann', 'bob', 'cy', 'dee'], length=6, device=cuda)
    lab, sel = _dev(labels, cuda), _dev(case['select'], cuda)
    ff.annotate(fr, names=table, known=ff.dist <= 0.5, values=ff.dist, colors=palette(lab), select=sel, length=8)   # (the allocator has its blocks)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = ff.annotate(fr, names=table, known=ff.dist <= 0.5, values=ff.dist, colors=palette(lab), select=sel, length=8, scale=1)
        same = ff.annotate(fr, names=table, values=ff.dist, decimals=1, out=fr.clone())
        boxes_only = ff.annotate(fr)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    names = table.names.cpu().numpy()
    colors = np.asarray(PALETTE, np.uint8)[np.where(labels < 0, 16, labels % 16)]
    text = A.compose(m, names, idx, dist <= 0.5, dist, 2, b'?', 8)
    assert (text[:, 0] == ord('?')).any() and (text[:, 0] != ord('?')).any()
    want = A.annotate(case['frames'], case['offsets'], case['boxes'], case['landmarks'], text, colors, A.COLOR, case['select'], scale=1)
    assert np.array_equal(got.cpu().numpy(), want) and not np.array_equal(want, case['frames'])
    text = A.compose(m, names, idx, None, dist, 1, b'?', 32)
    assert np.array_equal(same.cpu().numpy(), A.annotate(case['frames'], case['offsets'], case['boxes'], case['landmarks'], text))
    assert np.array_equal(boxes_only.cpu().numpy(), A.annotate(case['frames'], case['offsets'], case['boxes'], case['landmarks']))
    assert np.array_equal(fr.cpu().numpy(), case['frames'])


# ---- argument errors -----------------------------------------------------------------------------------------------------
def test_the_entries_argument_errors(cuda):
    """Each is an error return with a dif_last_error text, and nothing is launched: the output stays as it was."""
    from deep_insight_face import _native as N
    case = _cases()[1]
    fr = _dev(case['frames'], cuda)
    good = dict(off=case['offsets'], boxes=case['boxes'], landmarks=case['landmarks'], text=case['text'], colors=case['colors'])
    out = fr.clone()
    assert _entry(cuda, out, **good) == 0 and not torch.equal(out, fr)          # the arguments below differ from a good call in one thing
    bad = [dict(null=('out',)), dict(null=('offsets',)), dict(null=('boxes',)), dict(null=('colors', 'color')), dict(h=0), dict(h=8193), dict(w=0),
           dict(w=8193), dict(t=-1), dict(t=65), dict(s=0), dict(s=9), dict(r=-2), dict(r=17), dict(margin=float('nan')), dict(margin=float('inf')),
           dict(margin=float('-inf')), dict(n=-1), dict(m=-1), dict(n=1 << 31), dict(m=1 << 29), dict(l=0), dict(l=65)]
    for over in bad:
        marker = torch.full_like(fr, 77)
        assert _entry(cuda, marker, **{**good, **over}) != 0 and N.last_error().startswith('dif_frames_annotate'), over
        assert int(marker.min()) == 77 and int(marker.max()) == 77, over
    assert _entry(cuda, fr.clone(), **{**good, 'text': None}, l=0) == 0         # l is not looked at without text
    assert _entry(cuda, fr.clone(), **good, null=('color',)) == 0               # colours per face need no host colour
    m = len(case['boxes'])
    idx, values = _dev(np.arange(m) % 3, cuda), _dev(np.linspace(0, 1, m).astype(np.float32), cuda)
    names = _dev(A.texts([b'a', b'bc', b'def'], 4), cuda)

    def compose(text, names_ptr=N.ptr(names), g=3, ln=4, decimals=2, unknown=b'?', m=m, l=8, text_null=False):
        rc = N.lib.dif_annotate_compose(names_ptr, g, ln, N.ptr(idx), None, N.ptr(values), decimals, unknown, m, None if text_null else N.ptr(text), l,
                                        N.stream_ptr())
        torch.cuda.synchronize()
        return rc
    text = torch.full((m, 8), 77, dtype=torch.uint8, device=cuda)
    assert compose(text) == 0 and not (text == 77).any()                        # every byte of text is written: no label holds an 'M'
    for over in (dict(decimals=-1), dict(decimals=5), dict(unknown=None), dict(unknown=b'x' * 65), dict(m=-1), dict(m=1 << 31), dict(l=0),
                 dict(l=65), dict(g=-1), dict(ln=0), dict(text_null=True)):
        marker = torch.full((m, 8), 77, dtype=torch.uint8, device=cuda)
        assert compose(marker, **over) != 0 and N.last_error().startswith('dif_annotate_compose'), over
        assert int(marker.min()) == 77 and int(marker.max()) == 77, over
    assert compose(text, names_ptr=None, g=-1, ln=0) == 0                        # g and ln are not looked at without names
