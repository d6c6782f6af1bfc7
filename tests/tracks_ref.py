"""The tracking rule of FrameFaces.tracks / dif_tracks_link in plain NumPy, and the seeded sequences its tests walk.

A face continues the track whose last face, at most ``max_gap`` frames ago, overlaps it (IoU >= min_iou) and lies within the
embedding tolerance; candidates are taken in ascending (dist, i, j) order; a track holds one face per frame at most.  The
distances come from a callable, so that the GPU tests can hand over the library's own ``evaluation.utility.distance`` values
(dif_pairwise: existing, tested code) and compare ``link_dist`` bit for bit; ``np_distance`` is the reference's formula in
NumPy for the tests without a GPU.  Rows are GLOBAL everywhere: ``row_base`` + the row of the call.
"""
import functools
import math

import numpy as np

F = np.float32


def iou32(p, q):
    """box_iou of csrc/detector.hip in float32, one operation per statement (np.fmin / np.fmax drop a NaN operand as fminf /
    fmaxf do).  Corners are normalised per axis, so left / top / right / bottom serves as y0 / x0 / y1 / x1 does.  p, q:
    boxes [..., 4] that broadcast against each other."""
    p, q = np.asarray(p, F), np.asarray(q, F)
    with np.errstate(all='ignore'):
        py0, py1 = np.fmin(p[..., 0], p[..., 2]), np.fmax(p[..., 0], p[..., 2])
        px0, px1 = np.fmin(p[..., 1], p[..., 3]), np.fmax(p[..., 1], p[..., 3])
        qy0, qy1 = np.fmin(q[..., 0], q[..., 2]), np.fmax(q[..., 0], q[..., 2])
        qx0, qx1 = np.fmin(q[..., 1], q[..., 3]), np.fmax(q[..., 1], q[..., 3])
        ph = py1 - py0
        pw = px1 - px0
        ap = ph * pw
        qh = qy1 - qy0
        qw = qx1 - qx0
        aq = qh * qw
        ih = np.fmin(py1, qy1) - np.fmax(py0, qy0)
        ih = np.fmax(ih, F(0))
        iw = np.fmin(px1, qx1) - np.fmax(px0, qx0)
        iw = np.fmax(iw, F(0))
        inter = ih * iw
        union = ap + aq
        union = union - inter
        out = inter / union
        assert out.dtype == F                                   # every statement above is one float32 operation
        return np.where((ap <= 0) | (aq <= 0), F(0), out)


def np_distance(a, b, metric):
    """evaluation/utility.py:54-62 of the reference on float32 rows (what dif_pairwise restates)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all='ignore'):
        if metric == 0:
            return np.sum(np.square(np.subtract(a, b)), 1)
        dot = np.sum(np.multiply(a, b), axis=1)
        norm = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
        return (np.arccos(dot / norm) / math.pi).astype(F)


def dist_of(emb, metric):
    """A distance callable over the global rows of ``emb`` [rows, d] (the whole sequence): (j rows, i rows) -> float32."""
    def fn(j, i):
        if len(j) == 0:
            return np.zeros((0,), F)
        return np.asarray(np_distance(emb[np.asarray(j)], emb[np.asarray(i)], metric), F)
    return fn


class Face:
    __slots__ = ('row', 'box', 'label', 'age', 'closed', 'clipped')

    def __init__(self, row, box, clipped):
        self.row, self.box, self.clipped = row, box, clipped
        self.label, self.age, self.closed = row, 1, clipped


def new_state():
    return {'frames': [], 'row_base': 0}


def link(offsets, boxes, dist_fn, tolerance, min_iou, max_gap, kmax, state=None, events=None):
    """-> (prev, link_dist, labels, age, n_new, clipped, state).  offsets [N + 1], boxes [M, 4]; dist_fn(j_rows, i_rows) ->
    float32 distances of the pairs (emb_j, emb_i), rows global; ``state``: what an earlier call returned (not modified).
    ``events`` (a dict, or None) counts what the tests' coverage conditions ask for; it then evaluates the distance of the
    pairs the IoU rejects too."""
    offsets = np.asarray(offsets, np.int64)
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    n, m = len(offsets) - 1, int(offsets[-1]) if len(offsets) else 0
    state = state or new_state()
    base = state['row_base']
    hist = [list(fr) for fr in state['frames']]                 # the Face objects are copied before they are changed
    hist = [[_copy(f) for f in fr] for fr in hist]
    tol, miou = F(tolerance), F(min_iou)
    prev = np.full(m, -1, np.int64)
    link_dist = np.full(m, np.nan, F)
    labels = np.zeros(m, np.int64)
    age = np.zeros(m, np.int64)
    clipped = 0
    for f in range(n):
        lo, hi = int(offsets[f]), int(offsets[f + 1])
        faces = [Face(base + r, boxes[r], r - lo >= kmax) for r in range(lo, hi)]
        clipped += sum(fc.clipped for fc in faces)
        window = hist[-max_gap:]
        tails = [(len(window) - w, t) for w, fr in enumerate(window) for t in fr if not t.closed]
        live = [fc for fc in faces if not fc.clipped]
        gate = np.zeros((len(live), len(tails)), bool)
        if live and tails:
            gate = iou32(np.stack([t.box for _, t in tails])[None], np.stack([fc.box for fc in live])[:, None]) >= miou
        pairs = [(t, fc, gap, bool(gate[a, b])) for a, fc in enumerate(live) for b, (gap, t) in enumerate(tails)]
        want = [pr for pr in pairs if pr[3] or events is not None]
        dist = dist_fn([pr[1].row for pr in want], [pr[0].row for pr in want])
        cands = []
        for (t, fc, gap, gate), dd in zip(want, dist):
            near = bool(F(dd) <= tol)                            # (a NaN compares false)
            if gate and near:
                cands.append((float(dd), t.row, fc.row, t, fc, gap, F(dd)))
            elif events is not None:
                events['iou_only'] += (not gate) and near
                events['tol_only'] += gate and not near
        cands.sort(key=lambda c: c[:3])
        used_i, used_j = set(), set()
        lost = set()
        for _, ti, fj, t, fc, gap, dd in cands:
            if ti in used_i or fj in used_j:
                if ti in used_i and fj not in used_j:
                    lost.add(fj)
                continue
            used_i.add(ti)
            used_j.add(fj)
            r = fj - base
            prev[r], link_dist[r] = ti, dd
            fc.label, fc.age = t.label, t.age + 1
            t.closed = True
            if events is not None:
                events['gap_link'] += gap > 1
        if events is not None:
            events['conflict'] += len(lost - used_j)
            if len(hist) >= max_gap:
                events['gap_out'] += sum(not t.closed for t in hist[-max_gap])   # leaves the window with this frame
        for fc in faces:
            labels[fc.row - base], age[fc.row - base] = fc.label, fc.age
        hist.append(faces)
        hist = hist[-max_gap:]
    n_new = int((prev < 0).sum())
    out = {'frames': [[fc for fc in fr] for fr in hist], 'row_base': base + m}
    return prev, link_dist, labels, age, n_new, clipped, out


def _copy(f):
    g = Face(f.row, f.box, f.clipped)
    g.label, g.age, g.closed = f.label, f.age, f.closed
    return g


def new_events():
    return {'gap_link': 0, 'iou_only': 0, 'tol_only': 0, 'conflict': 0, 'gap_out': 0}


def walk_chunks(cuts, offsets, boxes, dist_fn, tolerance, min_iou, max_gap, kmax):
    """The sequence in chunks: frames [cuts[c], cuts[c + 1]) per call, each given the state of the call before -> the
    outputs of the calls joined (prev is global already)."""
    offsets = np.asarray(offsets, np.int64)
    state, parts = None, []
    n_new = clipped = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = int(offsets[a]), int(offsets[b])
        out = link(offsets[a:b + 1] - lo, boxes[lo:hi], dist_fn, tolerance, min_iou, max_gap, kmax, state)
        state = out[6]
        parts.append(out[:4])
        n_new += out[4]
        clipped += out[5]
    joined = [np.concatenate([p[k] for p in parts]) if parts else np.zeros(0) for k in range(4)]
    return joined[0], joined[1], joined[2], joined[3], n_new, clipped, state


# ------------------------------------------------------------------------------------------------ sequences
def sequence(seed, n_frames, people, d, canvas=(640, 480), speed=6.0, box=40.0, noise=0.3, miss=0.15, false_rate=0.5,
             per_frame=None, blank=()):
    """People on straight lines with boxes of about ``box`` px, embeddings = a unit direction per person + noise of
    about ``noise`` in length (four times that for one face in four); a detection is
    missed with probability ``miss``; ``false_rate`` false detections per frame on average, half of them a second, shifted
    detection of a real face (the same person's embedding with more noise), half a box somewhere with an embedding of its
    own.  People 0 and 1 walk towards each other on one line and cross in the middle of the sequence;
    every fifth person runs.  ``per_frame``: the
    faces of a frame are cut to at most that many (after a shuffle: the detector's order is by score, not by person);
    ``blank``: frames that are left without any face.  -> offsets [N + 1] int64, boxes [M, 4] float32 (l, t, r, b),
    emb [M, d] float32, who [M] int64 (-1: a false detection)."""
    rng = np.random.default_rng(seed)
    w, h = canvas
    dirs = rng.standard_normal((people, d))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    pos = np.stack([rng.uniform(0, w, people), rng.uniform(0, h, people)], 1)
    ang = rng.uniform(0, 2 * np.pi, people)
    vel = np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(0.3, 1.0, (people, 1)) * speed
    vel[4::5] *= 6.0                                        # runners: the same face, too far away a frame later
    if people >= 2:
        reach = speed * (n_frames - 1) / 2.0
        pos[0], vel[0] = (w / 2 - reach, h / 2), (speed, 0.0)
        pos[1], vel[1] = (w / 2 + reach, h / 2 + 4.0), (-speed, 0.0)
    size = rng.uniform(0.85, 1.15, people) * box
    offsets, boxes, emb, who = [0], [], [], []

    def face(c, s, e, p):
        boxes.append([c[0] - s / 2, c[1] - s / 2, c[0] + s / 2, c[1] + s / 2])
        emb.append(e)
        who.append(p)

    for f in range(n_frames):
        first = len(boxes)
        if f not in blank:
            for p in range(people):
                c = pos[p] + vel[p] * f + rng.normal(0, 1.0, 2)
                e = dirs[p] + noise / np.sqrt(d) * rng.standard_normal(d) * rng.choice([1.0, 1.0, 1.0, 4.0])
                if rng.uniform() < miss:
                    continue
                face(c, size[p] * rng.uniform(0.95, 1.05), e, p)
                if rng.uniform() < false_rate / people:
                    face(c + rng.normal(0, 4.0, 2), size[p], dirs[p] + 1.5 * noise / np.sqrt(d) * rng.standard_normal(d), -1)
            for _ in range(rng.poisson(false_rate / 2)):
                near = pos[rng.integers(people)] + vel[rng.integers(people)] * f if people else np.array([w / 2, h / 2])
                face(near + rng.normal(0, 8.0, 2), box, rng.standard_normal(d) / np.sqrt(d), -1)
            order = first + rng.permutation(len(boxes) - first)
            keep = order[:per_frame] if per_frame is not None else order
            for arr in (boxes, emb, who):
                arr[first:] = [arr[i] for i in keep]
        offsets.append(len(boxes))
    return (np.asarray(offsets, np.int64), np.asarray(boxes, F).reshape(-1, 4), np.asarray(emb, F).reshape(-1, d),
            np.asarray(who, np.int64))


# The generated cases the GPU tests walk (tests/test_tracks_ref.py asserts the coverage conditions on exactly these):
# name -> (arguments of sequence(), {metric: tolerance}, min_iou, kmax)
CASES = {
    # 40 frames with 0 .. 17 faces, d = 512: frame boundaries fall inside waves, 17 is odd against every tile
    'street': (dict(seed=3, n_frames=40, people=14, d=512, per_frame=17, blank=(7, 8, 9, 21), false_rate=1.5, miss=0.2),
               {0: 0.5, 1: 0.2}, 0.3, 17),
    # 9 frames with up to 64 faces, d = 128 (and the same clipped to 16 positions)
    'crowd': (dict(seed=5, n_frames=9, people=60, d=128, per_frame=64, canvas=(1280, 960), false_rate=6.0, miss=0.1, speed=10.0),
              {0: 0.5, 1: 0.2}, 0.3, 64),
}


def case(name):
    kw, tols, min_iou, kmax = CASES[name]
    return sequence(**kw), tols, min_iou, kmax


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """Every sequence of the GPU tests' shape list by name -> (offsets, boxes, emb), {metric: tolerance}, min_iou, kmax."""
    slow = dict(speed=1.0, canvas=(160, 120), false_rate=0.4, miss=0.1)      # people who stay where a face may find them
    if name in CASES:
        seq, tols, min_iou, kmax = case(name)
        return seq[:3], tols, min_iou, kmax
    if name == 'crowd16':                                   # the clip rule: positions 16 .. 63 of 'crowd' are never linked
        seq, tols, min_iou, _ = case('crowd')
        return seq[:3], tols, min_iou, 16
    seq = {'one': lambda: sequence(1, 1, 1, 128, miss=0.0, false_rate=0.0),
           'two': lambda: sequence(2, 2, 1, 128, miss=0.0, false_rate=0.0, speed=1.0),
           # 5 frames of 0 .. 3 faces: empty frames first, last, and in a run (longer than max_gap 1 and 2)
           'sparse_first': lambda: sequence(4, 5, 3, 128, per_frame=3, blank=(0, 2, 3), **slow),
           'sparse_last': lambda: sequence(6, 5, 3, 128, per_frame=3, blank=(1, 2, 4), **slow),
           # faces in frames 0, 4, 14, 22, 23 only: runs of empty frames longer than max_gap 2 and 8, and one that 8 just spans
           'long_gaps': lambda: sequence(10, 24, 3, 128, per_frame=3, blank=LONG_GAPS_BLANK, **slow)}[name]()
    return seq[:3], {0: 0.5, 1: 0.2}, 0.3, 3


LONG_GAPS_BLANK = tuple(f for f in range(24) if f not in (0, 4, 14, 22, 23))


# One embedding size per class of tests/embed_dims.py that dif_pairwise admits (n < 8, the 8-wide body with a tail, the first
# splits, a large size, a 65-leaf tree, the largest) -> the seed at which the six-frame case below holds all five coverage
# events on both metrics (found on the CPU; tests/test_tracks_ref.py asserts them).
DIM_SEEDS = {5: 111, 100: 216, 129: 256, 257: 406, 1000: 1148, 7689: 7913, 8192: 8322}
DIM_PARAMS = ({0: 0.5, 1: 0.25}, 0.3, 2, 8)                 # {metric: tolerance}, min_iou, max_gap, kmax


@functools.lru_cache(maxsize=None)
def dim_case(d):
    """Six frames of four people with embeddings of d floats -> offsets, boxes, emb (walked with DIM_PARAMS)."""
    return sequence(DIM_SEEDS[d], 6, 4, d, canvas=(160, 120), speed=2.0, miss=0.2, false_rate=1.0)[:3]


TWELVE_PARAMS = ({0: 0.6, 1: 0.3}, 0.2, 3)                  # {metric: tolerance}, min_iou, max_gap; kmax 4 and 64


@functools.lru_cache(maxsize=None)
def twelve():
    """The twelve frames (4 and 5 empty, d = 32) that the chunked walks split -> offsets, boxes, emb."""
    return sequence(14, 12, 5, 32, canvas=(200, 150), noise=0.2, miss=0.3, false_rate=1.0, blank=(4, 5))[:3]


CAP_BLANK = tuple(range(2, 32))


@functools.lru_cache(maxsize=None)
def cap_case():
    """The caps: max_gap 32 with 64 positions.  36 frames, faces in frames 0, 1 and 32 .. 35 only, 64 to a frame (nearly),
    people who hardly move: frame 32 links frames 0 and 1 across gaps of 32 and 31 frames (the first slots of
    its table), frame 33 continues frame 32 through the last ones (up to 31 * 64 + 63), and frames 32 .. 35 take over ring
    frames 0 .. 3 again.
    -> (offsets, boxes, emb), {metric: tolerance}, min_iou, max_gap, kmax"""
    seq = sequence(21, 36, 60, 64, canvas=(1280, 960), speed=0.25, miss=0.05, false_rate=8.0, per_frame=64, blank=CAP_BLANK)
    return seq[:3], {0: 0.5, 1: 0.2}, 0.3, 32, 64
