"""Seeded inputs of tests/golden/detection.npz (tests/gen_golden_detection.py writes it from the reference's
detector/utility.py; tests/test_detection_ref.py and tests/test_detection_gpu.py read it).  The fixture carries `digest()` of
these arrays, so a change here without a new fixture fails loudly."""
import hashlib

import numpy as np


def overlap_boxes():
    """a [97, 4], b [69, 4] float32 (x1, y1, x2, y2): seeded boxes on a 640 x 480 frame with fractional coordinates, copies of
    one another (overlap 1), jittered copies, boxes that touch along an edge or in a corner, boxes of no width, of no area at
    all (the union clamp) and with right < left (a negative "area").  All finite: the reference yields NaN otherwise."""
    rng = np.random.default_rng(20240611)

    def boxes(n):
        xy = rng.random((n, 2)) * np.array([560.0, 400.0])
        wh = 4.0 + rng.random((n, 2)) * 360.0
        return np.concatenate([xy, xy + wh], axis=1)

    b = boxes(60)
    a = boxes(80)
    a = np.concatenate([a, b[:6], b[6:12] + rng.normal(0.0, 3.0, (6, 4))])
    special_a = [[0, 0, 2, 1], [10, 10, 20, 20], [10, 10, 20, 20], [5, 5, 5, 9], [7, 7, 7, 7]]
    special_b = [[0, 0, 1, 1], [20, 10, 30, 20], [20, 20, 30, 30], [5, 5, 5, 9], [7, 7, 7, 7], [30, 30, 20, 40], [12, 12, 18, 18],
                 [0.1, 0.2, 0.30000001, 0.7], [1e-12, 0, 2e-12, 1e-12]]
    a = np.concatenate([a, np.asarray(special_a, np.float64)]).astype(np.float32)
    b = np.concatenate([b, np.asarray(special_b, np.float64)]).astype(np.float32)
    return a, b


def ap_curves():
    """(recall, precision) float64 pairs: empty, one point, a clean staircase, a curve whose recall stalls, one that ends at
    recall 1, one whose precision rises late (the envelope at work), and two seeded detector-like curves of 300 and 5 000 points."""
    rng = np.random.default_rng(977)
    out = [(np.zeros(0), np.zeros(0)), (np.array([0.25]), np.array([1.0])),
           (np.array([0.2, 0.4, 0.6, 0.8]), np.array([1.0, 1.0, 0.75, 0.8])),
           (np.array([0.0, 0.0, 0.5, 0.5, 0.5]), np.array([0.0, 0.0, 1 / 3, 0.25, 0.2])),
           (np.array([0.5, 0.5, 1.0]), np.array([1.0, 0.5, 2 / 3])),
           (np.array([0.1, 0.1, 0.1, 0.2, 0.3]), np.array([1.0, 0.5, 1 / 3, 0.5, 0.6]))]
    for m, n_truth, p_hit in ((300, 41, 0.3), (5000, 1200, 0.22)):
        hit = rng.random(m) < p_hit * np.linspace(1.6, 0.2, m)
        tp = np.minimum(np.cumsum(hit), n_truth)
        hit = np.diff(np.concatenate([[0], tp])) > 0
        tp, fp = np.cumsum(hit), np.cumsum(~hit)
        out.append((tp / np.float64(n_truth), tp / np.maximum((tp + fp).astype(np.float64), np.finfo(float).eps)))
    return [(np.ascontiguousarray(r, dtype=np.float64), np.ascontiguousarray(p, dtype=np.float64)) for r, p in out]


def digest():
    h = hashlib.sha256()
    for x in overlap_boxes():
        h.update(x.tobytes())
    for r, p in ap_curves():
        h.update(r.tobytes())
        h.update(p.tobytes())
    return h.hexdigest()
