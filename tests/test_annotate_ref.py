"""The annotation rules (tests/annotate_ref.py) on hand cases, the coverage of the cases the GPU file walks, the font, and the
layers that carry FrameFaces.annotate / dif_frames_annotate / dif_annotate_compose.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import annotate_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(case, t, s, r, margin, use_select=True, use_colors=True, **kw):
    select, colors = A.call_args(case, use_select, use_colors)
    return A.annotate(case['frames'], case['offsets'], case['boxes'], case['landmarks'], case['text'], colors, A.COLOR, select, margin, t, s, r,
                      **kw)


# ---- the drawing on hand cases -------------------------------------------------------------------------------------------
def test_a_ring_lies_round_the_box_and_never_over_it():
    fr = np.full((1, 20, 24, 3), 9, np.uint8)
    got = A.annotate(fr, [0, 1], [[6.0, 7.0, 14.0, 13.0]], color=(1, 2, 3), thickness=2, mark=-1)[0]
    want = fr[0].copy()
    want[5:15, 4:16] = (1, 2, 3)
    want[7:13, 6:14] = 9
    assert np.array_equal(got, want)
    assert np.array_equal(A.annotate(fr, [0, 1], [[6.0, 7.0, 14.0, 13.0]], thickness=0, mark=-1), fr)      # no ring, nothing else


def test_a_plate_with_one_glyph_pixel_for_pixel():
    """'I' at scale 2 on a light colour: a plate of (6 - 1) * 2 + 4 = 14 by 18 above the box, black text one scale in."""
    fr = np.zeros((1, 40, 30, 3), np.uint8)
    got = A.annotate(fr, [0, 1], [[5.0, 25.0, 15.0, 35.0]], text=A.texts([b'I'], 4), color=(250, 250, 250), thickness=1, scale=2, mark=-1)[0]
    plate = got[6:24, 4:18]
    assert (got[:6] == 0).all() and (got[6:24, :4] == 0).all() and (got[6:24, 18:] == 0).all()
    glyph = np.array([[0, 1, 1, 1, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 1, 1, 1, 0]], bool)
    want = np.full((18, 14, 3), 250, np.uint8)
    want[2:16, 2:12][np.kron(glyph, np.ones((2, 2), bool))] = 0
    assert np.array_equal(plate, want)
    dark = A.annotate(fr, [0, 1], [[5.0, 25.0, 15.0, 35.0]], text=A.texts([b'I'], 4), color=(0, 0, 200), thickness=1, scale=2, mark=-1)[0]
    assert np.array_equal(dark[6:24, 4:18] == 255, want == 0)                                              # white text: all channels 255


def test_the_plate_moves_below_left_and_to_zero():
    fp = A.footprint([30.0, 3.0, 40.0, 12.0], A.texts([b'abc'])[0], None, 0.0, 1, 1, -1, 53)
    assert fp['plate'] == (29, 13, 29 + 19, 13 + 9)                            # no room above: below the ring
    fp = A.footprint([45.0, 20.0, 52.0, 30.0], A.texts([b'abc'])[0], None, 0.0, 1, 1, -1, 53)
    assert fp['plate'] == (53 - 19, 10, 53, 19)                                # pushed left at the right edge
    fp = A.footprint([45.0, 20.0, 52.0, 30.0], A.texts([b'abcdefgh'])[0], None, 0.0, 1, 2, -1, 53)
    assert fp['plate'] == (0, 1, 98, 19)                                       # wider than the frame: starts at 0
    assert A.footprint([45.0, 20.0, 52.0, 30.0], A.texts([b''])[0], None, 0.0, 1, 2, -1, 53)['plate'] is None
    assert A.footprint([45.0, 20.0, 45.0, 30.0], A.texts([b'x'])[0], None, 0.0, 1, 2, -1, 53) is None


def test_marks_round_half_up_and_skip_what_is_not_finite():
    lm = np.array([[2.5, 3.49], [np.nan, 1.0], [4.0, np.inf], [-0.5, -0.51], [1e9, 7.0]], np.float32)
    fp = A.footprint([0.0, 0.0, 9.0, 9.0], None, lm, 0.0, 1, 1, 1, 53)
    assert fp['marks'] == [(3, 3), (0, -1), (12288, 7)]
    assert A.footprint([0.0, 0.0, 9.0, 9.0], None, lm, 0.0, 1, 1, -1, 53)['marks'] == []
    fr = np.zeros((1, 12, 12, 3), np.uint8)
    got = A.annotate(fr, [0, 1], [[0.0, 0.0, 9.0, 9.0]], lm[None], color=(7, 7, 7), thickness=0, mark=1)[0]
    want = np.zeros((12, 12, 3), np.uint8)
    want[2:5, 2:5] = 7
    want[0:1, 0:2] = 7
    assert np.array_equal(got, want)


def test_the_lowest_row_wins_and_its_plate_is_opaque():
    fr = np.zeros((1, 37, 53, 3), np.uint8)
    boxes = [[10.0, 14.0, 30.0, 30.0], [12.0, 5.0, 32.0, 31.0]]
    text = A.texts([b'a', b'b'])
    colors = np.array([[200, 0, 0], [0, 0, 200]], np.uint8)
    both = A.annotate(fr, [0, 2], boxes, text=text, colors=colors, thickness=1, scale=1, mark=-1)[0]
    first = A.annotate(fr, [0, 1], boxes[:1], text=text[:1], colors=colors[:1], thickness=1, scale=1, mark=-1)[0]
    assert np.array_equal(both[first.any(2)], first[first.any(2)])             # row 0 shows whole: ring, plate, glyph
    plate = A.footprint(boxes[0], text[0], None, 0.0, 1, 1, -1, 53)['plate']
    assert (both[plate[1]:plate[3], plate[0]:plate[2], 2] != 200).all()        # row 1's ring crosses the plate and is hidden
    swapped = A.annotate(fr, [0, 2], boxes[::-1], text=text[::-1], colors=colors[::-1], thickness=1, scale=1, mark=-1)[0]
    assert not np.array_equal(swapped, both)
    off = A.annotate(fr, [0, 2], boxes, text=text, colors=colors, select=[0, 1], thickness=1, scale=1, mark=-1)[0]
    assert (off[..., 0] != 200).all() and (off[..., 2] == 200).any()           # an unselected face paints and shields nothing


# ---- the two statements of the drawing, and the cases --------------------------------------------------------------------
def test_painting_order_equals_the_rule_stated_pixel_by_pixel_and_other_bytes_stay():
    calls = 0
    for case, t, s, r, margin, use_select, use_colors in A.walk():
        select, colors = A.call_args(case, use_select, use_colors)
        got = _run(case, t, s, r, margin, use_select, use_colors)
        own, element, depth = A.owners(case['offsets'], case['boxes'], case['landmarks'], case['text'], select, margin, t, s, r, A.N, A.H, A.W)
        assert np.array_equal(got, A.from_owners(case['frames'], own, element, colors)), (case['name'], t, s, r, margin)
        assert np.array_equal(got[own < 0], case['frames'][own < 0]) and ((own >= 0) == (depth > 0)).all()
        calls += 1
    assert calls == 8 * (54 + 2)


def test_the_walk_shows_every_coverage_event():
    seen = {}
    for case, t, s, r, margin, use_select, use_colors in A.walk():
        assert case['frames'].shape == (A.N, A.H, A.W, 3) and (np.diff(case['offsets']) <= 6).all() and case['text'].shape[1] == A.L
        seen[(case['name'], t, s, r, margin, use_select, use_colors)] = A.events(case, t, s, r, margin, use_select, use_colors)

    def at(name):
        return set().union(*(v for k, v in seen.items() if k[0] == name))
    assert {'ring_cut_left', 'ring_cut_top', 'ring_cut_right', 'ring_cut_bottom', 'box_outside_paint_inside', 'plate_above', 'plate_below',
            'plate_shifted_left', 'plate_wider_than_frame', 'empty_text', 'full_length_text', 'no_landmarks', 'text_black',
            'text_white'} <= at('edges')
    assert {'three_deep', 'unselected_under_selected', 'plate_over_ring', 'byte_outside_ascii'} <= at('stack')
    assert {'empty_first_frame', 'empty_last_frame', 'nan_landmark', 'mark_outside_frame'} <= at('gaps')
    assert {'no_region_nan', 'no_region_inf', 'no_region_zero_area', 'no_region_margin'} <= at('bad')
    assert set().union(*seen.values()) == set(A.EVENTS)
    assert len(A.cases()) == 8 and [c['name'] for c in A.cases()][:4] == ['edges', 'stack', 'gaps', 'bad']


def test_the_generator_is_seeded():
    for x, y in zip(A.cases(), A.cases()):
        assert all(np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == 'f') for k in x if isinstance(x[k], np.ndarray))
    assert any(0 < c['select'].sum() < len(c['select']) for c in A.cases())


def test_in_place_and_an_out_of_other_bytes():
    case = A.cases()[1]
    want = _run(case, 1, 1, 2, 0.25)
    buf = case['frames'].copy()
    assert _run(dict(case, frames=buf), 1, 1, 2, 0.25, out=buf) is buf and np.array_equal(buf, want)
    other = _run(case, 1, 1, 2, 0.25, out=np.full_like(case['frames'], 99))
    own, _, _ = A.owners(case['offsets'], case['boxes'], case['landmarks'], case['text'], case['select'], 0.25, 1, 1, 2, A.N, A.H, A.W)
    assert np.array_equal(other[own >= 0], want[own >= 0]) and (other[own < 0] == 99).all() and (own < 0).any()


# ---- the label text ------------------------------------------------------------------------------------------------------
def _labels(**kw):
    m = len(kw['values']) if kw.get('values') is not None else len(kw['idx'])
    return [bytes(r.tolist()).rstrip(b'\0') for r in A.compose(m, **kw)]


def test_compose_on_hand_written_expectations():
    names = A.texts([b'ann', b'bob', b'christopher'], 11)
    # 0.005 -> 0.01: the value is float32, and float32(0.005) is 0.00499999989 -- below one half of a hundredth, 0.00 by the
    # rule -- so the half-way case is the least float32 that is not below 0.005, and halves that float32 holds exactly
    half = np.nextafter(np.float32(0.005), np.float32(1))
    assert float(half) >= 0.005 > float(np.float32(0.005))
    assert _labels(values=np.array([0.005, 0.125, 0.375, -0.125], np.float32), unknown=b'') == [b'0.00', b'0.13', b'0.38', b'-0.13']
    v = np.array([half, -0.004, np.nan, np.inf, -np.inf, 12.345, -half, 0.0, 99999.5, -1.0], np.float32)
    assert _labels(values=v) == [b'? 0.01', b'? 0.00', b'? nan', b'? 99999.00', b'? -99999.00', b'? 12.35', b'? -0.01', b'? 0.00',
                                 b'? 99999.00', b'? -1.00']
    assert _labels(values=v[:6], decimals=0) == [b'? 0', b'? 0', b'? nan', b'? 99999', b'? -99999', b'? 12']
    assert _labels(values=np.array([0.5, 1.5, 2.5, -0.5], np.float32), decimals=0, unknown=b'') == [b'1', b'2', b'3', b'-1']   # half up in |v|
    assert _labels(values=v[:2], decimals=4, unknown=b'') == [b'0.0050', b'-0.0040']
    idx = np.array([1, 0, 2, 3, -1, 2])
    assert _labels(names=names, idx=idx) == [b'bob', b'ann', b'christopher', b'?', b'?', b'christopher']      # idx out of range: unknown
    assert _labels(names=names, idx=idx, known=[1, 0, 1, 1, 1, 0], unknown=b'who') == [b'bob', b'who', b'christopher', b'who', b'who', b'who']
    assert _labels(names=names, idx=idx, values=np.arange(6, dtype=np.float32) / 4, l=8) == [b'bob 0.00', b'ann 0.25', b'christop', b'? 0.75',
                                                                                            b'? 1.00', b'christop']             # cut at l
    assert _labels(names=names, idx=idx[:2], unknown=b'', known=[0, 0]) == [b'', b'']
    assert _labels(idx=idx[:2]) == [b'?', b'?'] and _labels(names=names, idx=idx[:1], l=1) == [b'b']
    assert A.compose(2, names=names, idx=idx[:2], l=3).tolist() == [[98, 111, 98], [97, 110, 110]]                # l bytes: no NUL


# ---- the font ------------------------------------------------------------------------------------------------------------
def test_the_font():
    font = A.font()
    printable = font[0x20:0x7F]
    assert len(printable) == 95 and (printable < 32).all()                     # five columns
    assert len({tuple(g) for g in printable.tolist()}) == 95                   # pairwise distinct
    assert not printable[0].any() and all(g.any() for g in printable[1:])      # only the space is blank
    other = [c for c in range(256) if not 0x20 <= c <= 0x7E]
    assert (font[other] == 31).all() and len(other) == 161
    literal = {'I': [0b01110, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110],
               '0': [0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110],
               '-': [0, 0, 0, 0b11111, 0, 0, 0],
               '.': [0, 0, 0, 0, 0, 0b00110, 0b00110],
               '?': [0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b00000, 0b00100]}
    for ch, rows in literal.items():
        assert font[ord(ch)].tolist() == rows, ch
    from deep_insight_face import _native as N
    assert N.lib.dif_annotate_glyph(65, None) != 0 and N.last_error().startswith('dif_annotate_glyph')
    rows = (ctypes.c_uint8 * 7)()
    assert N.lib.dif_annotate_glyph(-5, rows) == 0 and list(rows) == [31] * 7 and N.lib.dif_annotate_glyph(1 << 20, rows) == 0


# ---- layers --------------------------------------------------------------------------------------------------------------
def test_header_library_binding_table_module_and_method_carry_annotation():
    """Fails on a tree without the feature."""
    from deep_insight_face import _native
    from deep_insight_face.detector import annotate
    from deep_insight_face.detector.faces import FrameFaces
    raw = open(os.path.join(ROOT, 'include', 'dif.h')).read()
    header = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name, k in {'dif_frames_annotate': 18, 'dif_annotate_compose': 12, 'dif_annotate_glyph': 2}.items():
        decl = re.search(r'\bint %s\s*\(([^;]*)\);' % name, header, flags=re.S)
        assert decl and decl.group(1).count(',') + 1 == k, name
        assert hasattr(_native.lib, name), name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == k, name
    for name, value in (('TEXT', 64), ('THICKNESS', 64), ('SCALE', 8), ('MARK', 16)):
        assert re.search(r'#define DIF_ANNOTATE_MAX_%s %d\b' % (name, value), raw) and getattr(annotate, 'MAX_' + name) == value
    assert all(callable(f) for f in (annotate.compose_text, annotate.annotate_frames, annotate.palette, annotate.NameTable,
                                     getattr(FrameFaces, 'annotate', None)))
    assert _native.lib.dif_version() == 110
    src = open(os.path.join(ROOT, 'deep-insight-face_amd', 'csrc', 'annotate.hip')).read()
    assert src.startswith('// hipcc-flags: -ffp-contract=off') and 'atomic' not in src.replace('no atomics', '').replace('No atomics', '')


def test_the_entries_argument_errors_without_a_device():
    from deep_insight_face import _native as N
    ann, comp = N.lib.dif_frames_annotate, N.lib.dif_annotate_compose
    color = (ctypes.c_uint8 * 3)(1, 2, 3)
    assert ann(None, 0, 4, 4, None, None, 0, None, None, 1, None, color, None, 0.0, 2, 2, 1, None) == 0           # nothing to do
    for h, w, t, s, r, margin in ((0, 4, 2, 2, 1, 0.0), (4, 8193, 2, 2, 1, 0.0), (4, 4, -1, 2, 1, 0.0), (4, 4, 65, 2, 1, 0.0), (4, 4, 2, 0, 1, 0.0),
                                  (4, 4, 2, 9, 1, 0.0), (4, 4, 2, 2, -2, 0.0), (4, 4, 2, 2, 17, 0.0), (4, 4, 2, 2, 1, float('nan'))):
        assert ann(None, 0, h, w, None, None, 0, None, None, 1, None, color, None, margin, t, s, r, None) != 0
        assert N.last_error().startswith('dif_frames_annotate')
    assert ann(None, 1, 4, 4, None, None, 1, None, None, 1, None, color, None, 0.0, 2, 2, 1, None) != 0 and 'null' in N.last_error()
    assert comp(None, 0, 1, None, None, None, 2, b'?', 0, None, 8, None) == 0
    for decimals, unknown, m, l in ((-1, b'?', 0, 8), (5, b'?', 0, 8), (2, None, 0, 8), (2, b'x' * 65, 0, 8), (2, b'?', -1, 8), (2, b'?', 0, 0),
                                    (2, b'?', 0, 65), (2, b'?', 1, 8)):
        assert comp(None, 0, 1, None, None, None, decimals, unknown, m, None, l, None) != 0
        assert N.last_error().startswith('dif_annotate_compose')
    assert comp(None, 0, 1, None, None, None, 2, b'x' * 64, 0, None, 8, None) == 0


def _args(**over):
    import torch
    a = dict(frames=torch.zeros((2, 6, 7, 3), dtype=torch.uint8), offsets=torch.tensor([0, 1, 3]), boxes=torch.zeros((3, 4)))
    a.update(over)
    return a


def test_the_modules_argument_errors():
    import torch
    from deep_insight_face.detector.annotate import annotate_frames, compose_text, palette
    z = torch.zeros
    u8 = dict(dtype=torch.uint8)
    bad = [dict(frames=z((2, 6, 7, 3))), dict(frames=z((2, 6, 7), **u8)), dict(frames=z((2, 6, 7, 4), **u8)), dict(frames=z((2, 0, 7, 3), **u8)),
           dict(frames=z((1, 1, 8193, 3), **u8), offsets=torch.tensor([0, 3])), dict(offsets=torch.tensor([0, 3])),
           dict(offsets=torch.tensor([0.0, 1.0, 3.0])), dict(boxes=z((3, 5))), dict(boxes=z((3, 4), dtype=torch.int64)),
           dict(landmarks=z((3, 5))), dict(landmarks=z((2, 5, 2))), dict(landmarks=z((3, 5, 2), dtype=torch.int64)),
           dict(text=z((3, 8))), dict(text=z((2, 8), **u8)), dict(text=z((3, 65), **u8)), dict(text=z((3, 0), **u8)), dict(text=z((3,), **u8)),
           dict(colors=z((3, 3))), dict(colors=z((2, 3), **u8)), dict(colors=(0, 0)), dict(colors=(0, 0, 256)),
           dict(select=z((2,), dtype=torch.bool)), dict(select=z((3,))), dict(margin=float('nan')), dict(margin=float('inf')), dict(margin=1e39),
           dict(thickness=-1), dict(thickness=65), dict(scale=0), dict(scale=9), dict(mark=-2), dict(mark=17),
           dict(out=z((2, 6, 7, 3))), dict(out=z((2, 6, 8, 3), **u8)), dict(out=z((2, 7, 6, 3), **u8).transpose(1, 2)),
           dict(out=np.zeros((2, 6, 7, 3), np.uint8))]
    for over in bad:
        with pytest.raises(ValueError):
            annotate_frames(**_args(**over))
    if not torch.cuda.is_available():
        with pytest.raises(ValueError):                                      # out on the host
            annotate_frames(**_args(out=z((2, 6, 7, 3), **u8)))
    ok = dict(idx=torch.tensor([0, 1]))
    for over in (dict(idx=None), dict(idx=z((2, 2), dtype=torch.int64)), dict(idx=z((2,))), dict(known=z((3,), **u8)), dict(known=z((2,))),
                 dict(values=z((3,))), dict(values=z((2,), dtype=torch.int64)), dict(decimals=-1), dict(decimals=5), dict(length=0),
                 dict(length=65), dict(unknown=b'?'), dict(unknown='x' * 65), dict(unknown='a\0b'), dict(names=z((2, 4))), dict(names=z((4,), **u8))):
        with pytest.raises(ValueError):
            compose_text(**{**ok, **over})
    for labels in (z((2, 2), dtype=torch.int64), z((2,))):
        with pytest.raises(ValueError):
            palette(labels)


def test_nothing_to_do_needs_no_device_and_the_host_helpers():
    import torch
    from deep_insight_face.detector.annotate import PALETTE, NameTable, annotate_frames, compose_text, palette
    from deep_insight_face.detector.faces import FrameFaces
    fr = torch.arange(2 * 6 * 7 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(2, 6, 7, 3)
    got = annotate_frames(fr, torch.tensor([0, 0, 0]), torch.zeros((0, 4)))
    assert got is not fr and torch.equal(got, fr)
    out = torch.zeros_like(fr)
    assert annotate_frames(fr, torch.tensor([0, 0, 0]), torch.zeros((0, 4)), out=out) is out and not out.any()
    assert annotate_frames(fr[:0], torch.tensor([0]), torch.zeros((0, 4))).shape == (0, 6, 7, 3)
    z = torch.zeros((0,))
    ff = FrameFaces(torch.zeros((3,), dtype=torch.int64), z.long(), torch.zeros((0, 4)), z, None, torch.zeros((0, 8, 8, 3), dtype=torch.uint8),
                    idx=z.long(), dist=z)
    table = NameTable(['ann', 'Zoë', 'a name that is far too long'], length=6, device='cpu')
    assert len(table) == 3 and table.names.tolist() == [[97, 110, 110, 0, 0, 0], [90, 111, 63, 0, 0, 0], list(b'a name')]
    assert torch.equal(ff.annotate(fr, names=table, values=ff.dist), fr) and torch.equal(ff.annotate(fr), fr)
    assert compose_text(table, torch.zeros((0,), dtype=torch.int64), length=9).shape == (0, 9)
    with pytest.raises(ValueError):
        ff.annotate(fr, scale=9)
    with pytest.raises(ValueError):
        ff._replace(idx=None).annotate(fr, names=table)
    colors = palette(torch.tensor([0, 1, 15, 16, 33, -1, -7]))
    assert colors.dtype == torch.uint8 and colors.tolist() == [list(PALETTE[k]) for k in (0, 1, 15, 0, 1, 16, 16)]
    assert len(set(PALETTE)) == 17 and palette(torch.zeros((0,), dtype=torch.int64)).shape == (0, 3)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a HIP device is visible')
    from deep_insight_face import _native
    from deep_insight_face.detector.annotate import annotate_frames, compose_text
    with pytest.raises(_native.DifError):
        annotate_frames(**_args(boxes=torch.tensor([[1.0, 1.0, 5.0, 5.0]] * 3)))
    with pytest.raises(_native.DifError):
        compose_text(idx=torch.tensor([0, 1]))
