"""The redaction rule of FrameFaces.redact / dif_frames_redact (include/dif.h, "redaction") in plain NumPy, and the seeded
cases its tests walk.  Box arithmetic is np.float32, one operation per statement; everything on pixels is int64."""
import itertools

import numpy as np

F = np.float32
CLAMP_LO, CLAMP_HI = F(-4096), F(12288)
MODES = {'fill': 0, 'pixelate': 1, 'smooth': 2}
SHAPES = {'box': 0, 'ellipse': 1}


def _finite(*v):
    return all(bool(np.isfinite(x)) for x in v)


def unclipped(box, margin):
    """-> (X0, Y0, X1, Y1), steps 1 to 8 of the rule, or None."""
    l, t, r, b = F(box[0]), F(box[1]), F(box[2]), F(box[3])
    margin = F(margin)
    with np.errstate(all='ignore'):
        bw = F(r - l)
        bh = F(b - t)
        if not _finite(l, t, r, b) or not (bw > 0) or not (bh > 0):
            return None
        mw = F(margin * bw)
        mh = F(margin * bh)
        le = F(l - mw)
        re = F(r + mw)
        te = F(t - mh)
        be = F(b + mh)
        if not _finite(le, re, te, be) or not (re > le) or not (be > te):
            return None
    le, re, te, be = (min(max(v, CLAMP_LO), CLAMP_HI) for v in (le, re, te, be))
    X0, X1, Y0, Y1 = int(np.floor(le)), int(np.ceil(re)), int(np.floor(te)), int(np.ceil(be))
    if X1 <= X0 or Y1 <= Y0:
        return None
    return X0, Y0, X1, Y1


def region(box, margin, h, w):
    """-> (X0, Y0, X1, Y1, cx0, cy0, cx1, cy1): the unclipped and the clipped region of one face, or None."""
    u = unclipped(box, margin)
    if u is None:
        return None
    X0, Y0, X1, Y1 = u
    cx0, cy0, cx1, cy1 = max(X0, 0), max(Y0, 0), min(X1, w), min(Y1, h)
    if cx1 <= cx0 or cy1 <= cy0:
        return None
    return X0, Y0, X1, Y1, cx0, cy0, cx1, cy1


def cell_size(reg, cells, min_cell):
    rw, rh = reg[2] - reg[0], reg[3] - reg[1]
    return max(-(-max(rw, rh) // cells), min_cell)


def cell_means(src, reg, c, cells):
    """src uint8 [h][w][3] -> v int64 [cells][cells][3], the rounded means of the cells that meet the frame, -1 elsewhere."""
    X0, Y0, _, _, cx0, cy0, cx1, cy1 = reg
    ix = (np.arange(cx0, cx1, dtype=np.int64) - X0) // c
    jy = (np.arange(cy0, cy1, dtype=np.int64) - Y0) // c
    assert ix.max() < cells and jy.max() < cells
    S = np.zeros((cells, cells, 3), np.int64)
    K = np.zeros((cells, cells), np.int64)
    np.add.at(S, (jy[:, None], ix[None, :]), src[cy0:cy1, cx0:cx1].astype(np.int64))
    np.add.at(K, (jy[:, None], ix[None, :]), 1)
    v = np.full((cells, cells, 3), -1, np.int64)
    nz = K > 0
    v[nz] = (2 * S[nz] + K[nz][:, None]) // (2 * K[nz][:, None])
    return v


def covered(reg, shape):
    """-> bool [cy1 - cy0][cx1 - cx0]: the pixels of the clipped region that the shape covers."""
    X0, Y0, X1, Y1, cx0, cy0, cx1, cy1 = reg
    if shape == 0:
        return np.ones((cy1 - cy0, cx1 - cx0), bool)
    rw, rh = np.int64(X1 - X0), np.int64(Y1 - Y0)
    dx = np.arange(cx0, cx1, dtype=np.int64) - X0
    dy = np.arange(cy0, cy1, dtype=np.int64) - Y0
    ex = rh * rh * (2 * dx + 1 - rw) ** 2
    ey = rw * rw * (2 * dy + 1 - rh) ** 2
    return ex[None, :] + ey[:, None] <= rw * rw * rh * rh


def face_values(src, reg, mode, cells, min_cell, fill):
    """-> uint8 [cy1 - cy0][cx1 - cx0][3]: the value of every pixel of the clipped region, from the source frame."""
    X0, Y0, _, _, cx0, cy0, cx1, cy1 = reg
    ch, cw = cy1 - cy0, cx1 - cx0
    if mode == 0:
        return np.broadcast_to(np.asarray(fill, np.uint8), (ch, cw, 3)).copy()
    c = cell_size(reg, cells, min_cell)
    v = cell_means(src, reg, c, cells)
    dx = np.arange(cx0, cx1, dtype=np.int64) - X0
    dy = np.arange(cy0, cy1, dtype=np.int64) - Y0
    if mode == 1:
        vals = v[(dy // c)[:, None], (dx // c)[None, :]]
    else:
        a = 2 * dx + 1 - c
        i0 = a // (2 * c)
        fa = a - 2 * c * i0
        b = 2 * dy + 1 - c
        j0 = b // (2 * c)
        fb = b - 2 * c * j0
        assert fa.min() >= 0 and fa.max() < 2 * c and fb.min() >= 0 and fb.max() < 2 * c
        ilo, ihi = (cx0 - X0) // c, (cx1 - 1 - X0) // c
        jlo, jhi = (cy0 - Y0) // c, (cy1 - 1 - Y0) // c
        i0c, i1c = np.clip(i0, ilo, ihi), np.clip(i0 + 1, ilo, ihi)
        j0c, j1c = np.clip(j0, jlo, jhi), np.clip(j0 + 1, jlo, jhi)
        ga, gb = (2 * c - fa)[None, :, None], (2 * c - fb)[:, None, None]
        fa, fb = fa[None, :, None], fb[:, None, None]
        v00, v01 = v[j0c[:, None], i0c[None, :]], v[j0c[:, None], i1c[None, :]]
        v10, v11 = v[j1c[:, None], i0c[None, :]], v[j1c[:, None], i1c[None, :]]
        assert min(v00.min(), v01.min(), v10.min(), v11.min()) >= 0           # never a cell without pixels
        V = ga * gb * v00 + fa * gb * v01 + ga * fb * v10 + fa * fb * v11
        vals = (V + 2 * c * c) // (4 * c * c)
    assert vals.min() >= 0 and vals.max() <= 255
    return vals.astype(np.uint8)


def redact(frames, offsets, boxes, select=None, mode=1, shape=0, cells=8, min_cell=4, margin=0.0, fill=(0, 0, 0), out=None):
    """The rule.  frames uint8 [n][h][w][3] -> out (a copy of frames unless given; `out is frames` is in place).  Every value
    comes from `frames`; the faces of a frame are painted from its last row to its first, so the lowest row is what stays."""
    frames = np.asarray(frames)
    n, h, w, _ = frames.shape
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    src_all = frames.copy() if out is frames else frames
    if out is None:
        out = frames.copy()
    for f in range(n):
        for i in range(int(offsets[f + 1]) - 1, int(offsets[f]) - 1, -1):
            if select is not None and not select[i]:
                continue
            reg = region(boxes[i], margin, h, w)
            if reg is None:
                continue
            cx0, cy0, cx1, cy1 = reg[4:]
            vals = face_values(src_all[f], reg, mode, cells, min_cell, fill)
            cov = covered(reg, shape)
            out[f, cy0:cy1, cx0:cx1][cov] = vals[cov]
    return out


def owners(offsets, boxes, select, shape, margin, n, h, w):
    """-> int64 [n][h][w]: the row whose value a pixel takes, -1 where no selected face covers it; and depth, the number of
    selected faces that cover it.  Stated pixel by pixel, apart from `redact`'s painting order."""
    own = np.full((n, h, w), -1, np.int64)
    depth = np.zeros((n, h, w), np.int64)
    for f in range(n):
        for i in range(int(offsets[f]), int(offsets[f + 1])):
            if select is not None and not select[i]:
                continue
            reg = region(boxes[i], margin, h, w)
            if reg is None:
                continue
            cx0, cy0, cx1, cy1 = reg[4:]
            cov = covered(reg, shape)
            o = own[f, cy0:cy1, cx0:cx1]
            o[cov & (o < 0)] = i
            depth[f, cy0:cy1, cx0:cx1] += cov
    return own, depth


# ---- cases ---------------------------------------------------------------------------------------------------------------
N, H, W = 3, 37, 53
EVENTS = ('cut_left', 'cut_top', 'cut_right', 'cut_bottom', 'outside', 'whole_frame', 'three_deep', 'unselected_under_selected',
          'empty_first_frame', 'empty_last_frame', 'no_region_nan', 'no_region_inf', 'no_region_zero_area', 'no_region_margin')


def _case(name, frames, per_frame, select):
    counts = [len(b) for b in per_frame]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    boxes = np.asarray([b for fr in per_frame for b in fr], np.float32).reshape(-1, 4)
    select = None if select is None else np.asarray(select, np.uint8)
    assert select is None or len(select) == len(boxes)
    return dict(name=name, frames=frames, offsets=offsets, boxes=boxes, select=select)


def _random_box(rng):
    kind = rng.integers(0, 8)
    cx, cy = rng.uniform(0, W), rng.uniform(0, H)
    bw, bh = rng.uniform(2, 30), rng.uniform(2, 30)
    if kind == 0:                                    # snapped to integers and half integers
        return [np.floor(cx - bw / 2), np.floor(cy - bh / 2) + 0.5, np.floor(cx + bw / 2) + 0.5, np.floor(cy + bh / 2) + 1]
    if kind == 1:                                    # hangs over an edge
        cx, cy = rng.choice([-3.0, cx, W + 2.0]), rng.choice([-2.0, cy, H + 3.0])
    if kind == 2:                                    # small
        bw, bh = rng.uniform(0.2, 3), rng.uniform(0.2, 3)
    return [cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]


def cases(seed=2026, n_random=4):
    """The cases both test files walk: hand-built ones that carry the coverage events, then seeded random ones.  Frames are
    3 x 37 x 53 with 0 .. 6 faces each."""
    rng = np.random.default_rng(seed)

    def frames():
        f = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        f[:, ::2, ::2] //= 4                         # some structure, so that means differ from cell to cell
        return f

    out = []
    out.append(_case('edges', frames(), [
        [[-4.5, 5.2, 9.7, 20.1], [10.3, -6.0, 25.5, 8.8], [44.2, 12.0, 60.9, 30.3], [20.0, 28.5, 39.5, 45.0], [60.0, 5.0, 80.0, 20.0],
         [-30.0, -30.0, -2.0, -1.0]],
        [[-40.0, -30.0, 95.0, 70.0]],
        [[0.0, 0.0, 53.0, 37.0], [5.5, 5.5, 6.5, 6.5]]], None))
    out.append(_case('stack', frames(), [
        [[5.0, 4.0, 30.0, 28.0], [12.5, 9.0, 40.0, 33.5], [18.0, 2.0, 36.0, 20.0], [8.0, 12.0, 48.0, 30.0], [20.0, 14.0, 27.0, 21.0]],
        [[10.0, 10.0, 30.0, 30.0], [12.0, 12.0, 28.0, 28.0]],
        [[1.0, 1.0, 20.0, 20.0], [15.0, 15.0, 40.0, 35.0], [3.0, 3.0, 10.0, 10.0]]],
        [1, 1, 1, 0, 1, 0, 1, 1, 0, 1]))
    out.append(_case('gaps', frames(), [[], [[6.2, 7.7, 31.4, 29.9], [25.0, 3.0, 50.0, 22.0], [26.0, 4.0, 33.0, 9.0]], []], [1, 1, 1]))
    nan, inf = float('nan'), float('inf')
    out.append(_case('bad', frames(), [
        [[nan, 2.0, 20.0, 20.0], [3.0, 3.0, inf, 20.0], [10.0, 10.0, 10.0, 20.0], [8.0, 9.0, 30.0, 25.0]],
        [[20.0, 5.0, 10.0, 25.0], [-inf, 0.0, 5.0, 5.0], [4.0, 4.0, 24.0, nan]],
        [[2.0, 30.0, 40.0, 30.0], [30.0, 3.0, 45.0, 33.0]]], None))
    for r in range(n_random):
        per_frame = [[_random_box(rng) for _ in range(rng.integers(0, 7))] for _ in range(N)]
        m = sum(len(b) for b in per_frame)
        out.append(_case('random%d' % r, frames(), per_frame, rng.integers(0, 4, m) > 0 if r % 2 == 0 else None))
    return out


CELLS, MIN_CELLS, MARGINS = (1, 2, 8, 64), (1, 4), (0.0, 0.25, -0.2)


def walk():
    """(case, cells, min_cell, margin) of every generated call the GPU file makes, for each mode and shape: the full grid on
    every case, and the cases once more at a margin that empties every region."""
    for case in cases():
        for cells, min_cell, margin in itertools.product(CELLS, MIN_CELLS, MARGINS):
            yield case, cells, min_cell, margin
        yield case, 8, 4, -0.5
        yield case, 8, 1, -0.75


def events(case, margin):
    """The coverage events one case shows at one margin."""
    seen = set()
    off, boxes, select = case['offsets'], case['boxes'], case['select']
    sel = np.ones(len(boxes), bool) if select is None else select.astype(bool)
    if off[1] == off[0]:
        seen.add('empty_first_frame')
    if off[-1] == off[-2]:
        seen.add('empty_last_frame')
    for i, b in enumerate(boxes):
        reg = region(b, margin, H, W)
        if reg is None:
            with np.errstate(all='ignore'):
                if unclipped(b, margin) is not None:
                    seen.add('outside')
                elif np.isnan(b).any():
                    seen.add('no_region_nan')
                elif np.isinf(b).any():
                    seen.add('no_region_inf')
                elif not (b[2] - b[0] > 0) or not (b[3] - b[1] > 0):
                    seen.add('no_region_zero_area')
                elif unclipped(b, 0.0) is not None:
                    seen.add('no_region_margin')
            continue
        X0, Y0, X1, Y1 = reg[:4]
        if sel[i]:
            seen |= {k for k, hit in (('cut_left', X0 < 0), ('cut_top', Y0 < 0), ('cut_right', X1 > W), ('cut_bottom', Y1 > H)) if hit}
            if X0 <= 0 and Y0 <= 0 and X1 >= W and Y1 >= H:
                seen.add('whole_frame')
    own, depth = owners(off, boxes, sel, 0, margin, N, H, W)
    if depth.max() >= 3:
        seen.add('three_deep')
    frame = np.repeat(np.arange(N), np.diff(off))
    for i in np.flatnonzero(~sel):
        reg = region(boxes[i], margin, H, W)
        if reg is not None and (own[frame[i], reg[5]:reg[7], reg[4]:reg[6]] >= 0).any():
            seen.add('unselected_under_selected')
    return seen
