"""FrameFaces.redact / redact_frames / dif_frames_redact on the GPU against tests/redact_ref.py: every comparison is
array_equal on the whole `out`."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import redact_ref as R

pytestmark = pytest.mark.gpu

MODE_NAMES = {v: k for k, v in R.MODES.items()}
SHAPE_NAMES = {v: k for k, v in R.SHAPES.items()}
FILL = (7, 130, 255)


@functools.lru_cache(maxsize=None)
def _cases():
    return R.cases()


def _ff(off, boxes, dev):
    from deep_insight_face.detector.faces import FrameFaces
    off = np.asarray(off, np.int64)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    m = len(boxes)
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return FrameFaces(torch.from_numpy(off).to(dev), torch.from_numpy(frame).to(dev), torch.from_numpy(boxes).to(dev),
                      torch.ones((m,), device=dev), None, torch.zeros((m, 1, 1, 3), dtype=torch.uint8, device=dev))


def _run(dev, frames, off, boxes, select=None, mode=1, shape=0, cells=8, min_cell=4, margin=0.0, fill=FILL, want=None, what=''):
    """One call through FrameFaces.redact, out of place, against the restatement (or `want`); -> (got, frames on the device)."""
    fr = torch.from_numpy(frames).to(dev)
    sel = None if select is None else torch.from_numpy(np.asarray(select, np.uint8)).to(dev)
    got = _ff(off, boxes, dev).redact(fr, sel, MODE_NAMES[mode], cells, min_cell, margin, SHAPE_NAMES[shape], fill)
    assert got.is_cuda and got.dtype == torch.uint8 and got.data_ptr() != fr.data_ptr()
    if want is None:
        want = R.redact(frames, off, boxes, select, mode, shape, cells, min_cell, margin, fill)
    assert np.array_equal(got.cpu().numpy(), want), what
    assert np.array_equal(fr.cpu().numpy(), frames), what                      # the frames are unchanged
    return got, fr


# ---- the generated cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [0, 1])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_generated_cases(cuda, mode, shape):
    """Every call of redact_ref.walk(): 8 cases x (cells 1, 2, 8, 64 x min_cell 1, 4 x margin 0, 0.25, -0.2, and two margins
    that empty every region)."""
    calls = 0
    for case, cells, min_cell, margin in R.walk():
        _run(cuda, case['frames'], case['offsets'], case['boxes'], case['select'], mode, shape, cells, min_cell, margin,
             what=(case['name'], cells, min_cell, margin))
        calls += 1
    assert calls == 8 * 26


def test_one_frame_one_face(cuda):
    fr = _cases()[0]['frames'][:1]
    for mode, shape in itertools.product((0, 1, 2), (0, 1)):
        _run(cuda, fr, [0, 1], [[4.3, 5.1, 40.2, 30.9]], None, mode, shape)


def test_a_frame_of_one_pixel(cuda):
    fr = np.array([[[[10, 200, 31]]]], np.uint8)
    for mode, shape in itertools.product((0, 1, 2), (0, 1)):
        got, _ = _run(cuda, fr, [0, 2], [[-3.0, -2.0, 5.0, 9.0], [0.0, 0.0, 1.0, 1.0]], None, mode, shape, cells=2, min_cell=1)
        assert got.cpu().numpy().tolist() == [[[list(FILL) if mode == 0 else [10, 200, 31]]]]


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_in_place_equals_out_of_place(cuda, mode):
    for case in _cases()[:2]:
        for shape in (0, 1):
            got, fr = _run(cuda, case['frames'], case['offsets'], case['boxes'], case['select'], mode, shape, 8, 4, 0.25)
            sel = None if case['select'] is None else torch.from_numpy(case['select']).to(cuda)
            same = _ff(case['offsets'], case['boxes'], cuda).redact(fr, sel, MODE_NAMES[mode], 8, 4, 0.25, SHAPE_NAMES[shape], FILL, out=fr)
            assert same is fr and torch.equal(fr, got)


def test_out_given_keeps_its_other_bytes(cuda):
    """`out` need not start as a copy of the frames: only the covered pixels are written."""
    case = _cases()[1]
    fr = torch.from_numpy(case['frames']).to(cuda)
    out = torch.full_like(fr, 99)
    sel = torch.from_numpy(case['select']).to(cuda)
    assert _ff(case['offsets'], case['boxes'], cuda).redact(fr, sel, 'smooth', out=out) is out
    want = R.redact(case['frames'], case['offsets'], case['boxes'], case['select'], 2, 0, 8, 4, 0.0, out=np.full_like(case['frames'], 99))
    assert np.array_equal(out.cpu().numpy(), want) and (want == 99).any() and (want != 99).any()
    assert np.array_equal(fr.cpu().numpy(), case['frames'])


def test_select_none_all_ones_all_zeros_and_bool(cuda):
    case = _cases()[0]
    fr, off, boxes = case['frames'], case['offsets'], case['boxes']
    m = len(boxes)
    for mode in (0, 1, 2):
        none, _ = _run(cuda, fr, off, boxes, None, mode, 1)
        ones, _ = _run(cuda, fr, off, boxes, np.ones(m, np.uint8), mode, 1)
        assert torch.equal(none, ones)
        _run(cuda, fr, off, boxes, np.full(m, 200, np.uint8), mode, 1, want=none.cpu().numpy())           # any non-zero value
        _run(cuda, fr, off, boxes, np.zeros(m, np.uint8), mode, 1, want=fr)
    pick = np.arange(m) % 2 == 0
    by_bool = _ff(off, boxes, cuda).redact(torch.from_numpy(fr).to(cuda), torch.from_numpy(pick).to(cuda), 'pixelate')
    assert np.array_equal(by_bool.cpu().numpy(), R.redact(fr, off, boxes, pick))


def test_edges_on_integers_and_half_integers(cuda):
    fr = _cases()[2]['frames'][:2]
    boxes = [[3.0, 4.0, 20.0, 18.0], [10.5, 2.5, 30.5, 20.5], [0.0, 0.0, 53.0, 37.0], [52.0, 36.0, 53.0, 37.0],
             [5.0, 6.5, 25.5, 30.0], [-0.5, -0.5, 8.0, 8.5], [44.5, 30.0, 53.5, 37.5], [20.0, 10.0, 21.0, 30.0]]
    for mode, shape, margin in itertools.product((0, 1, 2), (0, 1), (0.0, 0.5)):
        _run(cuda, fr, [0, 4, 8], boxes, None, mode, shape, 4, 1, margin)


def test_edges_beyond_the_clamp(cuda):
    fr = _cases()[3]['frames'][:1]
    big = [[-1e6, -1e6, 1e6, 1e6], [10.0, 5.0, 1e6, 20.0], [-1e6, 8.0, 30.0, 1e6], [5.0, 5.0, 3e38, 3e38], [-3e38, -3e38, 20.0, 20.0],
           [-3e38, -3e38, 3e38, 3e38]]
    for row in big[:-1]:
        assert R.region(row, 0.0, R.H, R.W) is not None
    assert R.region(big[-1], 0.0, R.H, R.W) is None                            # r - l overflows, 0 * inf is not finite
    for mode, shape in itertools.product((0, 1, 2), (0, 1)):
        for row in big:
            _run(cuda, fr, [0, 1], [row], None, mode, shape, 8, 4, 0.0, what=row)
        _run(cuda, fr, [0, 6], big[::-1], None, mode, shape, 64, 1, 0.0)
    _run(cuda, fr, [0, 3], big[:3], None, 2, 1, 8, 4, 0.25)                    # +-1e6 with a margin


def test_more_lower_faces_than_one_block_lists(cuda):
    """A frame with 300 faces: from row 257 on the lower faces are tested one by one from the boxes, not from the list."""
    rng = np.random.default_rng(5)
    fr = _cases()[0]['frames'][:1]
    x, y = rng.uniform(-2, R.W - 3, 300), rng.uniform(-2, R.H - 3, 300)
    boxes = np.stack([x, y, x + rng.uniform(1, 5, 300), y + rng.uniform(1, 5, 300)], 1)
    select = rng.integers(0, 3, 300) == 0
    for mode, shape in ((1, 0), (2, 1)):
        _run(cuda, fr, [0, 300], boxes, select, mode, shape, 2, 1, 0.0)
    own, depth = R.owners([0, 300], np.asarray(boxes, np.float32), select, 0, 0.0, 1, R.H, R.W)
    assert (own > 256).sum() > 100 and depth[own > 256].max() >= 2 and depth.max() >= 3


# ---- the size caps -------------------------------------------------------------------------------------------------------
def test_a_frame_8192_wide(cuda):
    rng = np.random.default_rng(9)
    fr = rng.integers(0, 256, (1, 16, 8192, 3), dtype=np.uint8)
    for mode, shape, cells in ((1, 0, 64), (2, 1, 64), (1, 1, 3), (0, 0, 1)):
        _run(cuda, fr, [0, 2], [[-5.0, 2.0, 8200.0, 13.0], [100.0, -4.0, 300.0, 40.0]], None, mode, shape, cells, 4, 0.0)
    tall = np.ascontiguousarray(fr.transpose(0, 2, 1, 3))
    _run(cuda, tall, [0, 1], [[1.0, -9.0, 15.5, 9000.0]], None, 2, 0, 64, 1, 0.0)


def test_sums_beyond_32_bits(cuda):
    """One 4112 x 4112 frame of all 255, one box over it, one cell: S = 255 * 16 908 544 > 2^32, and smooth's V = 255 * 4 c^2 >
    2^32.  The answer is all 255; a border of the box is left out so that the test sees what was written."""
    side = 4112
    fr = torch.full((1, side, side, 3), 255, dtype=torch.uint8, device=cuda)
    ff = _ff([0, 1], [[0.0, 0.0, float(side), float(side)]], cuda)
    for mode in ('pixelate', 'smooth'):
        out = torch.zeros_like(fr)
        assert ff.redact(fr, None, mode, cells=1, min_cell=1, out=out) is out
        assert int(out.min()) == 255, mode
    part = _ff([0, 1], [[8.0, 8.0, float(side), float(side)]], cuda).redact(fr, None, 'smooth', cells=1, min_cell=1, out=torch.zeros_like(fr))
    assert int(part[0, 8:, 8:].min()) == 255 and not part[0, :8].any() and not part[0, :, :8].any()


# ---- nothing to do, no host read, the workspace --------------------------------------------------------------------------
def _entry(dev, frames, off, boxes, select=None, mode=1, shape=0, cells=8, min_cell=4, margin=0.0, fill=FILL, out=None, work=None,
           work_bytes=None, null=(), **sizes):
    """dif_frames_redact itself -> (rc, out); `null` names the pointers to pass as NULL, `sizes` replaces n, h, w or m."""
    from deep_insight_face import _native as N
    n, h, w = frames.shape[:3]
    off = torch.as_tensor(np.asarray(off, np.int64)).to(dev)
    bx = torch.as_tensor(np.asarray(boxes, np.float32).reshape(-1, 4)).to(dev)
    m = bx.shape[0]
    out = frames.clone() if out is None else out
    if work is None:
        work = torch.empty((max(N.lib.dif_frames_redact_workspace_size(m, min(max(cells, 1), 64)), 4),), dtype=torch.uint8, device=dev)
    a = dict(frames=N.ptr(frames), n=n, h=h, w=w, offsets=N.ptr(off), boxes=N.ptr(bx), m=m, select=None if select is None else N.ptr(select),
             mode=mode, shape=shape, cells=cells, min_cell=min_cell, margin=margin, fill=(ctypes.c_uint8 * 3)(*fill), out=N.ptr(out),
             work=N.ptr(work), work_bytes=work.shape[0] if work_bytes is None else work_bytes)
    a.update(sizes)
    a.update({k: None for k in null})
    assert list(a)[:4] == ['frames', 'n', 'h', 'w'] and len(a) == 17
    rc = N.lib.dif_frames_redact(*a.values(), N.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def test_no_faces_and_no_frames_in_both_layers(cuda):
    from deep_insight_face import _native as N
    from deep_insight_face.detector.redact import redact_frames
    fr = torch.from_numpy(_cases()[0]['frames']).to(cuda)
    got = redact_frames(fr, torch.zeros((4,), dtype=torch.int64, device=cuda), torch.zeros((0, 4), device=cuda))
    assert got.data_ptr() != fr.data_ptr() and torch.equal(got, fr)
    assert redact_frames(fr, torch.zeros((4,), dtype=torch.int64), torch.zeros((0, 4)), out=fr) is fr
    assert redact_frames(fr[:0], torch.zeros((1,), dtype=torch.int64, device=cuda), torch.zeros((0, 4), device=cuda)).shape == (0, R.H, R.W, 3)
    assert torch.equal(_ff([0, 0, 0, 0], [], cuda).redact(fr, mode='fill'), fr)
    rc, out = _entry(cuda, fr, [0, 0, 0, 0], [])
    assert rc == 0 and torch.equal(out, fr)
    assert N.lib.dif_frames_redact(None, 0, R.H, R.W, None, None, 0, None, 1, 0, 8, 4, 0.0, None, None, None, 0, N.stream_ptr()) == 0
    assert N.lib.dif_frames_redact(N.ptr(fr), 3, R.H, R.W, None, None, 0, None, 1, 0, 8, 4, 0.0, None, None, None, 0, N.stream_ptr()) == 0


def test_nothing_is_read_back(cuda):
    case = _cases()[1]
    fr = torch.from_numpy(case['frames']).to(cuda)
    ff = _ff(case['offsets'], case['boxes'], cuda)
    sel = torch.from_numpy(case['select']).to(cuda)
    dist = torch.where(sel > 0, 0.9, 0.1)
    ff.redact(fr, sel)                                                          # (the allocator has its blocks)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = [ff.redact(fr, dist > 0.5, mode, shape='ellipse', margin=0.25) for mode in ('fill', 'pixelate', 'smooth')]
        same = ff.redact(fr, sel, 'smooth', out=fr.clone())
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for mode, g in zip((0, 1, 2), got):
        assert np.array_equal(g.cpu().numpy(), R.redact(case['frames'], case['offsets'], case['boxes'], case['select'], mode, 1, 8, 4, 0.25))
    assert np.array_equal(same.cpu().numpy(), R.redact(case['frames'], case['offsets'], case['boxes'], case['select'], 2, 0, 8, 4, 0.0))


def test_one_workspace_used_large_small_large(cuda):
    from deep_insight_face import _native as N
    from deep_insight_face.detector.redact import redact_frames
    big, small = _cases()[1], _cases()[2]
    work = torch.empty((N.lib.dif_frames_redact_workspace_size(len(big['boxes']), 64),), dtype=torch.uint8, device=cuda)
    for case, cells in ((big, 64), (small, 2), (big, 64), (small, 8), (big, 3)):
        work.fill_(0xAB)
        fr = torch.from_numpy(case['frames']).to(cuda)
        sel = None if case['select'] is None else torch.from_numpy(case['select']).to(cuda)
        got = redact_frames(fr, case['offsets'], case['boxes'], sel, 'smooth', cells, 1, 0.25, 'box', workspace=work)
        assert np.array_equal(got.cpu().numpy(), R.redact(case['frames'], case['offsets'], case['boxes'], case['select'], 2, 0, cells, 1, 0.25))
    with pytest.raises(N.DifError, match='workspace'):
        redact_frames(fr, big['offsets'], big['boxes'], None, workspace=work[:len(big['boxes']) * 64 * 4 - 1])


def test_the_entrys_argument_errors(cuda):
    """Each is an error return with a dif_last_error text, and nothing is launched: out stays as it was."""
    from deep_insight_face import _native as N
    case = _cases()[1]
    fr = torch.from_numpy(case['frames']).to(cuda)
    off, boxes = case['offsets'], case['boxes']
    rc, out = _entry(cuda, fr, off, boxes, mode=0)
    assert rc == 0 and not torch.equal(out, fr)                                 # the arguments below differ from a good call in one thing
    flat = torch.zeros((2 * fr.numel(),), dtype=torch.uint8, device=cuda)
    lo = flat[:fr.numel()].view(fr.shape)
    lo.copy_(fr)
    bad = [dict(null=('frames',)), dict(null=('offsets',)), dict(null=('boxes',)), dict(null=('fill',)), dict(null=('out',)), dict(null=('work',)),
           dict(h=0), dict(h=8193), dict(w=0), dict(w=8193), dict(cells=0), dict(cells=65), dict(min_cell=0), dict(min_cell=8193),
           dict(mode=-1), dict(mode=3), dict(shape=-1), dict(shape=2), dict(margin=float('nan')), dict(margin=float('inf')),
           dict(margin=float('-inf')), dict(n=-1), dict(m=-1), dict(work_bytes=len(boxes) * 64 * 4 - 1), dict(work_bytes=0)]
    for over in bad:
        marker = torch.full_like(fr, 77)
        rc, out = _entry(cuda, fr, off, boxes, **{'mode': 0, 'out': marker, **over})
        assert rc != 0 and N.last_error().startswith('dif_frames_redact'), over
        assert int(marker.min()) == 77 and int(marker.max()) == 77, over
    work = torch.empty((len(boxes) * 64 * 4 + 4,), dtype=torch.uint8, device=cuda)
    rc, _ = _entry(cuda, fr, off, boxes, work=work[1:])
    assert rc != 0 and 'aligned' in N.last_error()
    for shift in (3, fr.numel() // 2, fr.numel() - 1):                          # out overlaps the frames in part
        over_out = flat[shift:shift + fr.numel()].view(fr.shape)
        before = flat.clone()
        rc, _ = _entry(cuda, lo, off, boxes, mode=0, out=over_out)
        assert rc != 0 and 'overlaps' in N.last_error() and torch.equal(flat, before), shift
        rc, _ = _entry(cuda, over_out, off, boxes, mode=0, out=lo)
        assert rc != 0 and 'overlaps' in N.last_error() and torch.equal(flat, before), shift
    rc, out = _entry(cuda, lo, off, boxes, mode=0, out=flat[fr.numel():].view(fr.shape))   # adjacent is no overlap
    assert rc == 0
    assert N.lib.dif_frames_redact_workspace_size(-1, 8) == -1 and N.lib.dif_frames_redact_workspace_size(4, 65) == -1


def test_offsets_that_cover_only_some_rows(cuda):
    """offsets[n] < m: the rows beyond are in no frame and are left out; nothing outside the buffers is touched."""
    case = _cases()[1]
    fr = torch.from_numpy(case['frames']).to(cuda)
    off = case['offsets'].copy()
    off[-1] -= 2
    from deep_insight_face.detector.redact import redact_frames
    got = redact_frames(fr, off, case['boxes'], torch.from_numpy(case['select']).to(cuda), 'pixelate')
    want = R.redact(case['frames'], off, case['boxes'][:off[-1]], case['select'][:off[-1]], 1)
    assert np.array_equal(got.cpu().numpy(), want)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_the_pipelines_faces_redacted(cuda):
    """MtcnnFramePipeline.faces on one seeded frame, then redact: the restatement on the boxes the pipeline returned."""
    from deep_insight_face.detector.mtcnn import MtcnnDetector, MtcnnFramePipeline
    from deep_insight_face.networks.triplet import bottleneck_network
    from test_faces_gpu import _blobs
    emb = bottleneck_network('resnet', emd_size=512, input_shape=(112, 112, 3), max_batch=4)('v2')
    emb.init_synthetic(2024)
    emb.set_input_transform(scale=1 / 255.)
    det = MtcnnDetector((96, 128), max_batch=2, cap=(24, 12, 8)).init_synthetic(2024, logit_scale=1.0)
    frames = _blobs(1, 96, 128, seed=11)
    fr = torch.from_numpy(frames).to(cuda)
    ff = MtcnnFramePipeline(det, emb, None, margin=8).faces(fr)
    m = int(ff.offsets[-1])
    assert m >= 2
    off, boxes = ff.offsets.cpu().numpy(), ff.boxes.cpu().numpy()
    select = np.arange(m) % 2 == 0
    for mode, shape in itertools.product((0, 1, 2), (0, 1)):
        got = ff.redact(fr, torch.from_numpy(select).to(cuda), MODE_NAMES[mode], shape=SHAPE_NAMES[shape], margin=0.1, fill=FILL)
        want = R.redact(frames, off, boxes, select, mode, shape, 8, 4, 0.1, FILL)
        assert np.array_equal(got.cpu().numpy(), want) and not np.array_equal(want, frames)
    det.close()
    emb.close()
