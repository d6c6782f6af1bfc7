"""The redaction rule (tests/redact_ref.py) on hand cases, the coverage of the cases the GPU file walks, and the layers that
carry FrameFaces.redact / dif_frames_redact.  No GPU."""
import os
import re

import numpy as np
import pytest

import redact_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(frame, box, **kw):
    """redact() of one frame [h][w][3] with one box -> [h][w][3]."""
    return R.redact(frame[None], np.array([0, 1]), np.asarray([box], np.float32), **kw)[0]


def _ramp(h, w):
    return (np.arange(h * w * 3, dtype=np.int64).reshape(h, w, 3) * 7 % 256).astype(np.uint8)


# ---- hand cases ----------------------------------------------------------------------------------------------------------
def test_means_round_half_up_on_a_4x4_box():
    f = np.zeros((4, 4, 3), np.uint8)
    f[0, 0] = (1, 1, 0)                              # cell (0, 0): 0, 0, 0, 1 -> 1/4 -> 0;  channel 2 all 0
    f[0, 2], f[1, 3] = (1, 0, 0), (1, 0, 0)          # cell (0, 1), channel 0: 1, 1, 0, 0 -> 2/4 = exactly one half -> 1
    f[2:, :2] = (200, 201, 255)
    f[2, 0] = (201, 201, 254)                        # 801 / 4 = 200.25 -> 200;  1019 / 4 = 254.75 -> 255
    got = _one(f, (0, 0, 4, 4), mode=1, cells=2, min_cell=1)
    assert got[:2, :2].tolist() == [[[0, 0, 0]] * 2] * 2
    assert got[:2, 2:, 0].tolist() == [[1, 1], [1, 1]] and not got[:2, 2:, 1:].any()
    assert got[2:, :2].tolist() == [[[200, 201, 255]] * 2] * 2
    two = np.zeros((1, 2, 3), np.uint8)
    two[0, 1] = 1                                    # values 0 and 1 give 1
    assert _one(two, (0, 0, 2, 1), mode=1, cells=1, min_cell=1).tolist() == [[[1, 1, 1]] * 2]


def test_the_4x4_ellipse_covers_twelve_pixels():
    cov = R.covered(R.region((0, 0, 4, 4), 0.0, 4, 4), 1)
    want = np.ones((4, 4), bool)
    want[[0, 0, 3, 3], [0, 3, 0, 3]] = False
    assert cov.sum() == 12 and np.array_equal(cov, want)
    got = _one(_ramp(4, 4), (0, 0, 4, 4), mode=0, shape=1, fill=(9, 8, 7))
    assert np.array_equal(got[want], np.broadcast_to(np.uint8([9, 8, 7]), (12, 3))) and np.array_equal(got[~want], _ramp(4, 4)[~want])


def test_a_region_one_pixel_wide_is_covered():
    for box, shape in (((3.2, 1.0, 3.9, 8.0), (7, 1)), ((1.0, 2.5, 9.0, 2.75), (1, 8))):
        reg = R.region(box, 0.0, 10, 10)
        assert (reg[3] - reg[1], reg[2] - reg[0]) == shape
        assert R.covered(reg, 1).all() and R.covered(reg, 0).all()


def test_smooth_at_an_odd_cells_centre_is_the_cell_mean():
    f = _ramp(15, 15)
    reg = R.region((0, 0, 15, 15), 0.0, 15, 15)
    assert R.cell_size(reg, 3, 1) == 5
    v = R.cell_means(f, reg, 5, 3)
    got = _one(f, (0, 0, 15, 15), mode=2, cells=3, min_cell=1)
    for j in range(3):
        for i in range(3):
            assert got[5 * j + 2, 5 * i + 2].tolist() == v[j, i].tolist()
    assert not np.array_equal(got, _one(f, (0, 0, 15, 15), mode=1, cells=3, min_cell=1))


def test_smooth_with_one_cell_is_pixelate():
    f = _ramp(11, 13)
    for shape in (0, 1):
        a = _one(f, (1.5, 2.0, 12.0, 10.5), mode=2, cells=1, min_cell=1, shape=shape)
        assert np.array_equal(a, _one(f, (1.5, 2.0, 12.0, 10.5), mode=1, cells=1, min_cell=1, shape=shape))


def test_min_cell_raises_the_cell_size():
    reg = R.region((2, 2, 8, 7), 0.0, 20, 20)       # 6 x 5 pixels, 8 cells: c = 1 without min_cell
    assert R.cell_size(reg, 8, 1) == 1 and R.cell_size(reg, 8, 4) == 4 and R.cell_size(reg, 2, 1) == 3
    f = _ramp(20, 20)
    assert np.array_equal(_one(f, (2, 2, 8, 7), mode=1, cells=8, min_cell=1), f)       # a mean of one pixel: untouched
    assert not np.array_equal(_one(f, (2, 2, 8, 7), mode=1, cells=8, min_cell=4), f)


def test_a_negative_margin_empties_a_region():
    assert R.region((2, 2, 10, 10), -0.25, 20, 20) == (4, 4, 8, 8, 4, 4, 8, 8)
    assert R.region((2, 2, 10, 10), -0.5, 20, 20) is None and R.region((2, 2, 10, 10), -0.75, 20, 20) is None
    assert R.region((2, 2, 10, 10), 0.5, 12, 20) == (-2, -2, 14, 14, 0, 0, 14, 12)
    f = _ramp(20, 20)
    assert np.array_equal(_one(f, (2, 2, 10, 10), mode=0, margin=-0.5, fill=(1, 1, 1)), f)


def test_regions_clamp_and_reject():
    assert R.region((-1e6, -1e6, 1e6, 1e6), 0.0, 30, 40) == (-4096, -4096, 12288, 12288, 0, 0, 40, 30)
    assert R.region((5, 5, 3e38, 3e38), 0.0, 30, 40) == (5, 5, 12288, 12288, 5, 5, 40, 30)
    assert R.region((-3e38, 0, 3e38, 9), 0.0, 30, 40) is None          # bw = inf, and 0 * inf is not finite
    assert R.region((0.0, 0.5, 3.0, 2.5), 0.0, 30, 40) == (0, 0, 3, 3, 0, 0, 3, 3)
    assert R.region((50, 5, 60, 9), 0.0, 30, 40) is None and R.unclipped((50, 5, 60, 9), 0.0) == (50, 5, 60, 9)


# ---- overlap -------------------------------------------------------------------------------------------------------------
def test_the_lowest_row_wins_and_swapping_rows_changes_the_answer():
    f = _ramp(20, 24)[None]
    boxes = np.asarray([[2, 2, 14, 14], [8, 6, 22, 18]], np.float32)
    off = np.array([0, 2])
    for mode in (1, 2):
        both = R.redact(f, off, boxes, mode=mode, cells=2, min_cell=1)
        first = R.redact(f, np.array([0, 1]), boxes[:1], mode=mode, cells=2, min_cell=1)
        second = R.redact(f, np.array([0, 1]), boxes[1:], mode=mode, cells=2, min_cell=1)
        assert np.array_equal(both[0, 2:14, 2:14], first[0, 2:14, 2:14])                # row 0 shows whole
        rest = np.ones((20, 24), bool)
        rest[2:14, 2:14] = False
        assert np.array_equal(both[0][rest], second[0][rest])                           # row 1 where row 0 is not
        swapped = R.redact(f, off, boxes[::-1], mode=mode, cells=2, min_cell=1)
        assert not np.array_equal(swapped, both)
        assert np.array_equal(swapped[0, 6:18, 8:22], second[0, 6:18, 8:22])


def test_painting_order_equals_the_rule_stated_pixel_by_pixel():
    """owners() names the face of every pixel without painting; the value of that face alone must be what redact() left."""
    for case in R.cases()[:5]:
        fr, off, boxes, sel = case['frames'], case['offsets'], case['boxes'], case['select']
        for shape in (0, 1):
            got = R.redact(fr, off, boxes, sel, 1, shape, 2, 1, 0.25)
            own, _ = R.owners(off, boxes, sel, shape, 0.25, *fr.shape[:3])
            want = fr.copy()
            frame = np.repeat(np.arange(R.N), np.diff(off))
            for i in np.unique(own[own >= 0]):
                alone = R.redact(fr, np.where(np.arange(R.N + 1) > frame[i], 1, 0), boxes[i:i + 1], None, 1, shape, 2, 1, 0.25)
                want[own == i] = alone[own == i]
            assert np.array_equal(got, want), case['name']


def test_in_place_equals_out_of_place_in_the_restatement():
    case = R.cases()[1]
    for mode in (0, 1, 2):
        want = R.redact(case['frames'], case['offsets'], case['boxes'], case['select'], mode, 1, 8, 4, 0.25, (4, 5, 6))
        buf = case['frames'].copy()
        assert R.redact(buf, case['offsets'], case['boxes'], case['select'], mode, 1, 8, 4, 0.25, (4, 5, 6), out=buf) is buf
        assert np.array_equal(buf, want)


# ---- coverage of the generated cases -------------------------------------------------------------------------------------
def test_the_walk_shows_every_coverage_event():
    """Frames hold at most six faces and the first and the last are to be empty in some case, so no single case can show all
    fourteen events: each hand-built case must show its own at every margin of the grid, and the walk as a whole all of them."""
    seen = {}
    for case, cells, min_cell, margin in R.walk():
        assert case['frames'].shape == (R.N, R.H, R.W, 3) and (np.diff(case['offsets']) <= 6).all()
        seen.setdefault((case['name'], margin), R.events(case, margin))
    for margin in R.MARGINS:
        assert {'cut_left', 'cut_top', 'cut_right', 'cut_bottom', 'outside', 'whole_frame'} <= seen[('edges', margin)], margin
        assert {'three_deep', 'unselected_under_selected'} <= seen[('stack', margin)], margin
        assert {'empty_first_frame', 'empty_last_frame'} <= seen[('gaps', margin)], margin
        assert {'no_region_nan', 'no_region_inf', 'no_region_zero_area'} <= seen[('bad', margin)], margin
    assert 'no_region_margin' in seen[('bad', -0.5)] and 'no_region_margin' in seen[('stack', -0.75)]
    assert set().union(*seen.values()) == set(R.EVENTS)
    assert len(R.cases()) == 8 and [c['name'] for c in R.cases()][:4] == ['edges', 'stack', 'gaps', 'bad']


def test_the_generator_is_seeded():
    a, b = R.cases(), R.cases()
    for x, y in zip(a, b):
        assert np.array_equal(x['frames'], y['frames']) and np.array_equal(x['boxes'], y['boxes'], equal_nan=True)
    assert any(c['select'] is not None and 0 < c['select'].sum() < len(c['select']) for c in a)


def test_every_walked_call_stays_in_range():
    """Every call of the walk in every mode and shape: face_values asserts 0 .. 255, cell indices below `cells` and no cell
    without pixels inside the index clamp."""
    calls = 0
    for case, cells, min_cell, margin in R.walk():
        for mode in (0, 1, 2):
            for shape in (0, 1):
                out = R.redact(case['frames'], case['offsets'], case['boxes'], case['select'], mode, shape, cells, min_cell, margin, (1, 2, 3))
                assert out.dtype == np.uint8 and out.shape == case['frames'].shape
                calls += 1
    assert calls == 8 * 26 * 6


# ---- layers --------------------------------------------------------------------------------------------------------------
def test_header_library_binding_table_module_and_method_carry_redaction():
    """Fails on a tree without the feature."""
    from deep_insight_face import _native
    from deep_insight_face.detector import redact
    from deep_insight_face.detector.faces import FrameFaces
    raw = open(os.path.join(ROOT, 'include', 'dif.h')).read()
    header = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name, k in {'dif_frames_redact': 18, 'dif_frames_redact_workspace_size': 2}.items():
        decl = re.search(r'\b(?:int|int64_t) %s\s*\(([^;]*)\);' % name, header, flags=re.S)
        assert decl and decl.group(1).count(',') + 1 == k, name
        assert hasattr(_native.lib, name), name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == k, name
    assert re.search(r'#define DIF_REDACT_MAX_CELLS 64\b', raw) and re.search(r'#define DIF_REDACT_MAX_SIDE 8192\b', raw)
    assert (redact.MAX_CELLS, redact.MAX_SIDE) == (64, 8192) and redact.MODES == R.MODES and redact.SHAPES == R.SHAPES
    assert callable(redact.redact_frames) and callable(getattr(FrameFaces, 'redact', None))
    assert _native.lib.dif_version() == 110
    src = open(os.path.join(ROOT, 'deep-insight-face_amd', 'csrc', 'redact.hip')).read()
    assert src.startswith('// hipcc-flags: -ffp-contract=off') and 'atomic' not in src.replace('no atomics', '').replace('No atomics', '')


def test_workspace_size_and_entry_errors_without_a_device():
    from deep_insight_face import _native as N
    size = N.lib.dif_frames_redact_workspace_size
    assert size(0, 8) == 0 and size(5, 8) == 5 * 64 * 4 and size(3, 64) == 3 * 4096 * 4 and size(7, 1) == 28
    assert size(-1, 8) == -1 and size(1, 0) == -1 and size(1, 65) == -1 and size(1 << 31, 1) == -1 and size(1 << 26, 64) == -1
    assert N.lib.dif_frames_redact(None, 1, 0, 4, None, None, 1, None, 1, 0, 8, 4, 0.0, None, None, None, 0, None) != 0
    assert N.last_error().startswith('dif_frames_redact')
    assert N.lib.dif_frames_redact(None, 0, 4, 4, None, None, 0, None, 1, 0, 8, 4, 0.0, None, None, None, 0, None) == 0    # nothing to do


def _args(**over):
    import torch
    a = dict(frames=torch.zeros((2, 6, 7, 3), dtype=torch.uint8), offsets=torch.tensor([0, 1, 3]), boxes=torch.zeros((3, 4)))
    a.update(over)
    return a


def test_the_modules_argument_errors():
    import torch
    from deep_insight_face.detector.redact import redact_frames
    z = torch.zeros
    bad = [dict(frames=z((2, 6, 7, 3))), dict(frames=z((2, 6, 7), dtype=torch.uint8)), dict(frames=z((2, 6, 7, 4), dtype=torch.uint8)),
           dict(frames=z((2, 0, 7, 3), dtype=torch.uint8)), dict(frames=z((1, 1, 8193, 3), dtype=torch.uint8), offsets=torch.tensor([0, 3])),
           dict(offsets=torch.tensor([0, 3])), dict(offsets=torch.tensor([0.0, 1.0, 3.0])), dict(boxes=z((3, 5))),
           dict(boxes=z((3, 4), dtype=torch.int64)), dict(select=z((2,), dtype=torch.bool)), dict(select=z((3,))),
           dict(mode='blur'), dict(mode=1), dict(shape='circle'), dict(cells=0), dict(cells=65), dict(min_cell=0), dict(min_cell=8193),
           dict(margin=float('nan')), dict(margin=float('inf')), dict(margin=1e39), dict(fill=(0, 0)), dict(fill=(0, 0, 256)),
           dict(out=z((2, 6, 7, 3))), dict(out=z((2, 6, 8, 3), dtype=torch.uint8)), dict(out=z((2, 7, 6, 3), dtype=torch.uint8).transpose(1, 2)),
           dict(out=np.zeros((2, 6, 7, 3), np.uint8)), dict(workspace=z((4, 4), dtype=torch.uint8)), dict(workspace=z((64,)))]
    for over in bad:
        with pytest.raises(ValueError):
            redact_frames(**_args(**over))
    if not torch.cuda.is_available():
        with pytest.raises(ValueError):                                      # out on the host
            redact_frames(**_args(out=z((2, 6, 7, 3), dtype=torch.uint8)))


def test_nothing_to_do_needs_no_device():
    import torch
    from deep_insight_face.detector.faces import FrameFaces
    from deep_insight_face.detector.redact import redact_frames
    fr = torch.arange(2 * 6 * 7 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(2, 6, 7, 3)
    got = redact_frames(fr, torch.tensor([0, 0, 0]), torch.zeros((0, 4)))
    assert got is not fr and torch.equal(got, fr)
    out = torch.zeros_like(fr)
    assert redact_frames(fr, torch.tensor([0, 0, 0]), torch.zeros((0, 4)), out=out) is out and not out.any()       # out is left as it was
    assert redact_frames(fr[:0], torch.tensor([0]), torch.zeros((0, 4))).shape == (0, 6, 7, 3)
    z = torch.zeros((0,))
    ff = FrameFaces(torch.zeros((3,), dtype=torch.int64), z.long(), torch.zeros((0, 4)), z, None, torch.zeros((0, 8, 8, 3), dtype=torch.uint8))
    assert torch.equal(ff.redact(fr, mode='smooth', shape='ellipse'), fr)
    with pytest.raises(ValueError):
        ff.redact(fr, cells=65)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a HIP device is visible')
    from deep_insight_face import _native
    from deep_insight_face.detector.redact import redact_frames
    with pytest.raises(_native.DifError):
        redact_frames(**_args(boxes=torch.tensor([[1.0, 1.0, 5.0, 5.0]] * 3)))
