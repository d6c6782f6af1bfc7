"""The two rules of FrameFaces.annotate (include/dif.h, "annotation") in plain NumPy, and the seeded cases their tests walk:
`compose` is dif_annotate_compose's label text; `annotate` is dif_frames_annotate's drawing, painted face by face, and
`owners` the same drawing decided pixel by pixel.  Box and landmark arithmetic is np.float32, one operation per statement
(the box's region is redact_ref.unclipped); everything on pixels is integer.  The font is data and comes from the library
(dif_annotate_glyph)."""
import ctypes
import functools
import itertools

import numpy as np

from redact_ref import CLAMP_HI, CLAMP_LO, F, unclipped

MAX_TEXT = 64
COLOR = (0, 255, 0)                                  # the colour of every face when no colours are given
NONE, PLATE, GLYPH, MARK, RING = 0, 1, 2, 3, 4       # the element that paints a pixel


@functools.lru_cache(maxsize=None)
def font():
    """-> uint8 [256][7]: the seven rows of the glyph of every byte, bit 4 = the left column."""
    from deep_insight_face import _native as N
    out = np.zeros((256, 7), np.uint8)
    rows = (ctypes.c_uint8 * 7)()
    for code in range(256):
        assert N.lib.dif_annotate_glyph(code, rows) == 0
        out[code] = list(rows)
    return out


# ---- the label text --------------------------------------------------------------------------------------------------------
def number(v, decimals):
    v = F(v)
    if np.isnan(v):
        return b'nan'
    a = min(abs(v), F(99999))
    p = 10 ** decimals
    scaled = np.float64(a) * np.float64(p)
    c = int(np.floor(scaled + np.float64(0.5)))
    s = ('-' if v < 0 and c > 0 else '') + str(c // p)
    if decimals > 0:
        s += '.' + str(c % p).zfill(decimals)
    return s.encode()


def compose(m, names=None, idx=None, known=None, values=None, decimals=2, unknown=b'?', l=32):
    """names uint8 [g][ln] or None, unknown bytes -> uint8 [m][l]."""
    out = np.zeros((m, l), np.uint8)
    for i in range(m):
        s = unknown
        if names is not None and idx is not None and (known is None or known[i]) and 0 <= int(idx[i]) < len(names):
            s = bytes(names[int(idx[i])].tolist()).split(b'\0')[0]
        if values is not None:
            s = s + (b' ' if s else b'') + number(values[i], decimals)
        s = s[:l]
        out[i, :len(s)] = list(s)
    return out


# ---- the drawing -----------------------------------------------------------------------------------------------------------
def text_length(row):
    nul = np.flatnonzero(np.asarray(row) == 0)
    return int(nul[0]) if len(nul) else len(row)


def footprint(box, text_row, lm, margin, t, s, r, w):
    """-> dict(box=(X0, Y0, X1, Y1), plate=(PX0, PY0, PX1, PY1) or None, marks=[(mx, my)], len), or None without a region."""
    u = unclipped(box, margin)
    if u is None:
        return None
    X0, Y0, X1, Y1 = u
    ln = 0 if text_row is None else text_length(text_row)
    plate = None
    if ln > 0:
        tw = (6 * ln - 1) * s
        pw, ph = tw + 2 * s, 9 * s
        px0 = X0 - t
        if px0 + pw > w:
            px0 = w - pw
        if px0 < 0:
            px0 = 0
        py0 = Y0 - t - ph
        if py0 < 0:
            py0 = Y1 + t
        plate = (px0, py0, px0 + pw, py0 + ph)
    marks = []
    if lm is not None and r >= 0:
        for k in range(5):
            px, py = F(lm[k][0]), F(lm[k][1])
            if not (np.isfinite(px) and np.isfinite(py)):
                continue
            px, py = min(max(px, CLAMP_LO), CLAMP_HI), min(max(py, CLAMP_LO), CLAMP_HI)
            sx, sy = F(px + F(0.5)), F(py + F(0.5))
            marks.append((int(np.floor(sx)), int(np.floor(sy))))
    return dict(box=u, plate=plate, marks=marks, len=ln)


def ink(c):
    return (0, 0, 0) if 299 * int(c[0]) + 587 * int(c[1]) + 114 * int(c[2]) >= 128000 else (255, 255, 255)


def _fill(img, x0, y0, x1, y1, c):
    h, w = img.shape[:2]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
    if x1 > x0 and y1 > y0:
        img[y0:y1, x0:x1] = c


def _paint_face(img, fp, text_row, c, t, s, r):
    """One face in full, lowest priority first: ring, marks, plate, glyphs."""
    X0, Y0, X1, Y1 = fp['box']
    _fill(img, X0 - t, Y0 - t, X1 + t, Y0, c)
    _fill(img, X0 - t, Y1, X1 + t, Y1 + t, c)
    _fill(img, X0 - t, Y0, X0, Y1, c)
    _fill(img, X1, Y0, X1 + t, Y1, c)
    for mx, my in fp['marks']:
        _fill(img, mx - r, my - r, mx + r + 1, my + r + 1, c)
    if fp['plate'] is None:
        return
    px0, py0, px1, py1 = fp['plate']
    _fill(img, px0, py0, px1, py1, c)
    bits = np.zeros((7, 6 * fp['len'] - 1), bool)
    for k in range(fp['len']):
        rows = font()[int(text_row[k])]
        bits[:, 6 * k:6 * k + 5] = (rows[:, None] >> (4 - np.arange(5))[None, :]) & 1
    big = np.kron(bits, np.ones((s, s), bool))       # every font pixel s x s
    h, w = img.shape[:2]
    gx0, gy0 = px0 + s, py0 + s
    x0, y0, x1, y1 = max(gx0, 0), max(gy0, 0), min(gx0 + big.shape[1], w), min(gy0 + big.shape[0], h)
    if x1 > x0 and y1 > y0:
        img[y0:y1, x0:x1][big[y0 - gy0:y1 - gy0, x0 - gx0:x1 - gx0]] = ink(c)


def _face_args(i, landmarks, text, colors, color):
    return (None if landmarks is None else landmarks[i], None if text is None else text[i], color if colors is None else tuple(colors[i]))


def annotate(frames, offsets, boxes, landmarks=None, text=None, colors=None, color=COLOR, select=None, margin=0.0, thickness=2,
             scale=2, mark=1, out=None):
    """The rule as a painter: the selected faces of a frame from its last row to its first, each in full, so the lowest row
    is what stays.  -> out (a copy of frames unless given; painted in place)."""
    frames = np.asarray(frames)
    n, h, w, _ = frames.shape
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    if out is None:
        out = frames.copy()
    for f in range(n):
        for i in range(int(offsets[f + 1]) - 1, int(offsets[f]) - 1, -1):
            if select is not None and not select[i]:
                continue
            lm, row, c = _face_args(i, landmarks, text, colors, color)
            fp = footprint(boxes[i], row, lm, margin, thickness, scale, mark, w)
            if fp is not None:
                _paint_face(out[f], fp, row, c, thickness, scale, mark)
    return out


def element_masks(fp, text_row, t, s, r, h, w):
    """-> (plate, glyph, marks, ring) bool [h][w], each from its own inequality on the pixel's coordinates."""
    xs, ys = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    X0, Y0, X1, Y1 = fp['box']
    inside = (xs >= X0) & (xs < X1) & (ys >= Y0) & (ys < Y1)
    ring = (xs >= X0 - t) & (xs < X1 + t) & (ys >= Y0 - t) & (ys < Y1 + t) & ~inside
    marks = np.zeros((h, w), bool)
    for mx, my in fp['marks']:
        marks |= (abs(xs - mx) <= r) & (abs(ys - my) <= r)
    plate, glyph = np.zeros((h, w), bool), np.zeros((h, w), bool)
    if fp['plate'] is not None:
        px0, py0, px1, py1 = fp['plate']
        plate = (xs >= px0) & (xs < px1) & (ys >= py0) & (ys < py1)
        u, v = xs - px0 - s, ys - py0 - s
        tw, th = (6 * fp['len'] - 1) * s, 7 * s
        field = (u >= 0) & (u < tw) & (v >= 0) & (v < th)
        k = np.clip(u // (6 * s), 0, fp['len'] - 1)
        col = (u % (6 * s)) // s
        row = np.clip(v // s, 0, 6)
        codes = np.asarray(text_row[:fp['len']], np.int64)[k]                   # [1][w]
        rows = font()[codes, row]                                               # [h][w]
        glyph = field & (col < 5) & (((rows >> np.clip(4 - col, 0, 4)) & 1) > 0)
    return plate, glyph, marks, ring


def owners(offsets, boxes, landmarks, text, select, margin, thickness, scale, mark, n, h, w):
    """-> own int64 [n][h][w], the row that paints a pixel (-1: none); element [n][h][w], with which of its elements; depth, how
    many selected faces paint it.  Decided pixel by pixel, apart from `annotate`'s painting order."""
    own = np.full((n, h, w), -1, np.int64)
    element = np.zeros((n, h, w), np.int64)
    depth = np.zeros((n, h, w), np.int64)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    for f in range(n):
        for i in range(int(offsets[f]), int(offsets[f + 1])):
            if select is not None and not select[i]:
                continue
            lm, row, _ = _face_args(i, landmarks, text, None, None)
            fp = footprint(boxes[i], row, lm, margin, thickness, scale, mark, w)
            if fp is None:
                continue
            plate, glyph, marks, ring = element_masks(fp, row, thickness, scale, mark, h, w)
            el = np.where(plate, np.where(glyph, GLYPH, PLATE), np.where(marks, MARK, np.where(ring, RING, NONE)))
            free = (own[f] < 0) & (el > 0)
            own[f][free] = i
            element[f][free] = el[free]
            depth[f] += el > 0
    return own, element, depth


def from_owners(frames, own, element, colors=None, color=COLOR):
    """The picture that `owners` describes."""
    out = np.asarray(frames).copy()
    for i in np.unique(own[own >= 0]):
        c = color if colors is None else tuple(colors[i])
        out[(own == i) & (element != GLYPH)] = c
        out[(own == i) & (element == GLYPH)] = ink(c)
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------
N, H, W, L = 3, 37, 53, 8
EVENTS = ('ring_cut_left', 'ring_cut_top', 'ring_cut_right', 'ring_cut_bottom', 'box_outside_paint_inside', 'plate_above',
          'plate_below', 'plate_shifted_left', 'plate_wider_than_frame', 'empty_text', 'full_length_text', 'byte_outside_ascii',
          'mark_outside_frame', 'nan_landmark', 'no_landmarks', 'no_region_nan', 'no_region_inf', 'no_region_zero_area',
          'no_region_margin', 'three_deep', 'unselected_under_selected', 'plate_over_ring', 'empty_first_frame', 'empty_last_frame',
          'text_black', 'text_white')


def texts(rows, l=L):
    out = np.zeros((len(rows), l), np.uint8)
    for i, s in enumerate(rows):
        assert len(s) <= l
        out[i, :len(s)] = list(s)
    return out


def _centre_marks(boxes):
    """Five landmarks inside every box: the usual eyes, nose, mouth corners."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    with np.errstate(all='ignore'):
        fx = np.array([0.3, 0.7, 0.5, 0.35, 0.65], np.float32)
        fy = np.array([0.35, 0.35, 0.55, 0.75, 0.75], np.float32)
        x = b[:, :1] + (b[:, 2:3] - b[:, :1]) * fx[None, :]
        y = b[:, 1:2] + (b[:, 3:4] - b[:, 1:2]) * fy[None, :]
    return np.stack([x, y], 2).astype(np.float32)


def _case(name, frames, per_frame, text, select, colors, landmarks):
    counts = [len(b) for b in per_frame]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    boxes = np.asarray([b for fr in per_frame for b in fr], np.float32).reshape(-1, 4)
    m = len(boxes)
    text = texts(text)
    select, colors = np.asarray(select, np.uint8), np.asarray(colors, np.uint8).reshape(-1, 3)
    assert len(text) == m and len(select) == m and len(colors) == m and (landmarks is None or landmarks.shape == (m, 5, 2))
    return dict(name=name, frames=frames, offsets=offsets, boxes=boxes, text=text, select=select, colors=colors, landmarks=landmarks)


DARK, LIGHT = (20, 20, 120), (255, 255, 0)


def _random_box(rng):
    kind = rng.integers(0, 8)
    cx, cy = rng.uniform(0, W), rng.uniform(0, H)
    bw, bh = rng.uniform(2, 24), rng.uniform(2, 20)
    if kind == 0:                                    # snapped to integers and half integers
        return [np.floor(cx - bw / 2), np.floor(cy - bh / 2) + 0.5, np.floor(cx + bw / 2) + 0.5, np.floor(cy + bh / 2) + 1]
    if kind == 1:                                    # hangs over an edge, or lies beyond it
        cx, cy = rng.choice([-3.0, cx, W + 2.0]), rng.choice([-2.0, cy, H + 3.0])
    if kind == 2:                                    # small
        bw, bh = rng.uniform(0.2, 3), rng.uniform(0.2, 3)
    return [cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]


def _random_text(rng):
    ln = int(rng.choice([0, 1, 2, 3, 5, L]))
    s = rng.integers(0x20, 0x7F, ln).astype(np.uint8)
    if ln and rng.integers(0, 5) == 0:
        s[rng.integers(0, ln)] = rng.choice([1, 0x7F, 0xE9])
    return bytes(s.tolist())


def cases(seed=2027, n_random=4):
    """The cases both test files walk: hand-built ones that carry the coverage events, then seeded random ones.  Frames are
    3 x 37 x 53 with 0 .. 6 faces each; text rows are 8 bytes."""
    rng = np.random.default_rng(seed)

    def frames():
        return rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)

    nan, inf = float('nan'), float('inf')
    out = []
    out.append(_case('edges', frames(), [
        [[0.5, 12.0, 11.0, 24.0], [20.0, 0.5, 32.0, 9.0], [42.0, 11.0, 52.5, 22.0], [20.0, 26.0, 31.0, 36.5], [-12.0, 26.0, -0.5, 35.0],
         [60.0, 5.0, 80.0, 20.0]],
        [[-40.0, -30.0, 95.0, 70.0]],
        [[10.0, 14.0, 30.0, 30.0], [40.5, 20.5, 41.5, 21.5]]],
        [b'ab', b'Top', b'xyz', b'', b'Q', b'far', b'big', b'ABCDEFGH', b''],
        [1] * 9, [LIGHT, DARK, LIGHT, DARK, LIGHT, DARK, LIGHT, DARK, LIGHT], None))
    stack = [
        [[5.0, 12.0, 30.0, 30.0], [12.5, 14.0, 40.0, 33.5], [18.0, 11.0, 36.0, 22.0], [8.0, 13.0, 48.0, 31.0], [20.0, 14.0, 27.0, 21.0]],
        [[10.0, 14.0, 30.0, 30.0], [11.0, 15.0, 31.0, 31.0], [12.0, 16.0, 32.0, 32.0], [9.0, 13.0, 29.0, 29.0]],
        [[4.0, 12.0, 20.0, 24.0], [15.0, 18.0, 40.0, 35.0], [6.0, 22.0, 14.0, 30.0]]]
    out.append(_case('stack', frames(), stack,
                     [b'ann', b'bob 0.41', b'?', b'', b'e', b'one', b'two', b'three', b'zero', b'p', b'\xe9t\x01', b'r 1'],
                     [1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 0], [DARK, LIGHT] * 6, _centre_marks([b for fr in stack for b in fr])))
    gaps = [[], [[6.2, 13.7, 31.4, 29.9], [25.0, 12.0, 50.0, 24.0], [44.0, 2.0, 58.0, 12.0]], []]
    lm = _centre_marks([b for fr in gaps for b in fr])
    lm[0, 1] = (nan, 20.0)
    lm[0, 3] = (8.0, inf)
    lm[1, 0] = (-9.0, 14.0)                                                     # a mark outside the frame
    lm[1, 4] = (49.6, 38.2)                                                     # ... and one that reaches in from below
    lm[2, 2] = (1e6, -1e6)
    out.append(_case('gaps', frames(), gaps, [b'gap', b'', b'edge'], [1, 1, 1], [LIGHT, DARK, LIGHT], lm))
    bad = [
        [[nan, 2.0, 20.0, 20.0], [3.0, 3.0, inf, 20.0], [10.0, 10.0, 10.0, 20.0], [8.0, 12.0, 30.0, 25.0]],
        [[20.0, 5.0, 10.0, 25.0], [-inf, 0.0, 5.0, 5.0], [4.0, 14.0, 24.0, nan]],
        [[2.0, 30.0, 40.0, 30.0], [30.0, 13.0, 45.0, 33.0]]]
    out.append(_case('bad', frames(), bad, [b'nan', b'inf', b'flat', b'ok', b'neg', b'-inf', b'nan2', b'flat2', b'ok2'], [1] * 9,
                     [LIGHT, DARK, LIGHT] * 3, _centre_marks([b for fr in bad for b in fr])))
    for r in range(n_random):
        per_frame = [[_random_box(rng) for _ in range(rng.integers(0, 7))] for _ in range(N)]
        flat = [b for fr in per_frame for b in fr]
        m = len(flat)
        lm = _centre_marks(flat) + rng.uniform(-2, 2, (m, 5, 2)).astype(np.float32) if m else np.zeros((0, 5, 2), np.float32)
        lm[rng.integers(0, 6, (m, 5)) == 0] = nan
        out.append(_case('random%d' % r, frames(), per_frame, [_random_text(rng) for _ in range(m)],
                         rng.integers(0, 4, m) > 0 if r % 2 == 0 else np.ones(m, np.uint8), rng.integers(0, 256, (m, 3)),
                         lm if r != 1 else None))
    return out


THICKNESSES, SCALES, MARKS, MARGINS = (0, 1, 3), (1, 2), (-1, 0, 2), (0.0, 0.25, -0.2)


def walk():
    """(case, thickness, scale, mark, margin, use_select, use_colors) of every generated call the GPU file makes: the full grid
    on every case, with and without the case's select and colours in turn, and two margins that empty every region."""
    k = 0
    for case in cases():
        for t, s, r, margin in itertools.product(THICKNESSES, SCALES, MARKS, MARGINS):
            yield case, t, s, r, margin, bool(k & 1), bool(k & 2)
            k += 1
        yield case, 3, 1, 1, -0.5, True, True
        yield case, 1, 2, 0, -0.75, True, True


def call_args(case, use_select, use_colors):
    """-> (select, colors) of one walked call."""
    return (case['select'] if use_select else None), (case['colors'] if use_colors else None)


def events(case, t, s, r, margin, use_select=True, use_colors=True):
    """The coverage events one case shows at one setting."""
    seen = set()
    off, boxes, text, lms = case['offsets'], case['boxes'], case['text'], case['landmarks']
    select, colors = call_args(case, use_select, use_colors)
    sel = np.ones(len(boxes), bool) if select is None else select.astype(bool)
    if off[1] == off[0]:
        seen.add('empty_first_frame')
    if off[-1] == off[-2]:
        seen.add('empty_last_frame')
    if lms is None:
        seen.add('no_landmarks')
    own, element, depth = owners(off, boxes, lms, text, sel, margin, t, s, r, N, H, W)
    if depth.max() >= 3:
        seen.add('three_deep')
    frame = np.repeat(np.arange(N), np.diff(off))
    masks = {}
    for i, b in enumerate(boxes):
        fp = footprint(b, text[i], None if lms is None else lms[i], margin, t, s, r, W)
        if fp is None:
            with np.errstate(all='ignore'):
                if np.isnan(b).any():
                    seen.add('no_region_nan')
                elif np.isinf(b).any():
                    seen.add('no_region_inf')
                elif not (b[2] - b[0] > 0) or not (b[3] - b[1] > 0):
                    seen.add('no_region_zero_area')
                elif unclipped(b, 0.0) is not None:
                    seen.add('no_region_margin')
            continue
        masks[i] = element_masks(fp, text[i], t, s, r, H, W)
        plate, glyph, marks, ring = masks[i]
        if not sel[i]:
            if ((plate | marks | ring) & (own[frame[i]] >= 0)).any():
                seen.add('unselected_under_selected')
            continue
        X0, Y0, X1, Y1 = fp['box']
        if t > 0:
            seen |= {k for k, hit in (('ring_cut_left', X0 - t < 0 <= X1 + t), ('ring_cut_top', Y0 - t < 0 <= Y1 + t),
                                      ('ring_cut_right', X1 + t > W >= X0 - t), ('ring_cut_bottom', Y1 + t > H >= Y0 - t)) if hit and ring.any()}
        if (X1 <= 0 or Y1 <= 0 or X0 >= W or Y0 >= H) and (plate | ring).any():
            seen.add('box_outside_paint_inside')
        if fp['len'] == 0:
            seen.add('empty_text')
        else:
            px0, py0, px1, py1 = fp['plate']
            if fp['len'] == text.shape[1]:
                seen.add('full_length_text')
            if any(c < 0x20 or c > 0x7E for c in text[i, :fp['len']]) and glyph.any():
                seen.add('byte_outside_ascii')
            if plate.any():
                seen.add('plate_above' if py0 < Y0 else 'plate_below')
                if px1 - px0 > W:
                    seen.add('plate_wider_than_frame')
                elif px0 < X0 - t and px1 == W:
                    seen.add('plate_shifted_left')
                if glyph.any():
                    seen.add('text_black' if ink(COLOR if colors is None else colors[i]) == (0, 0, 0) else 'text_white')
        if lms is not None and r >= 0:
            if not np.isfinite(lms[i]).all():
                seen.add('nan_landmark')
            if any(mx + r < 0 or mx - r >= W or my + r < 0 or my - r >= H for mx, my in fp['marks']):
                seen.add('mark_outside_frame')
    for i, (plate, _, _, _) in masks.items():
        if sel[i]:
            mine = plate & (own[frame[i]] == i)
            if any(sel[j] and j != i and frame[j] == frame[i] and (masks[j][3] & mine).any() for j in masks):
                seen.add('plate_over_ring')
    return seen
