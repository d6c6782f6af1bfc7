"""NumPy restatement of dif_nms for the tests (test infrastructure only): the greedy suppression of csrc/detector.hip in
float32, operation by operation as box_iou evaluates it, vectorised over the boxes so that a 26 625-box list with 64 picks
takes tens of milliseconds (oracle.mtcnn.nms_slots and oracle.detector.non_max_suppression state the same rule pair by pair
in pure Python; tests/test_nms_ref.py holds the three together index for index)."""
import numpy as np

F = np.float32
NEG_INF = F(-np.inf)


def nms_ref(boxes, scores, cap, iou, score_thr=-np.inf):
    """boxes [K, 4] (two corners, either order), scores [K] -> (keep [cap] int32, -1 padded, pick order; count).
    A box takes part when score >= score_thr and score > -inf (NaN fails both).  Every pick is the highest live score,
    the lowest index among equals; it clears every live box whose IoU with it is > iou, and itself."""
    b = np.ascontiguousarray(boxes, dtype=F).reshape(-1, 4)
    s = np.ascontiguousarray(scores, dtype=F).reshape(-1)
    assert len(b) == len(s)
    keep = np.full(cap, -1, np.int32)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        idx = np.nonzero((s >= F(score_thr)) & (s > NEG_INF))[0]
        s, b = s[idx], b[idx]
        # fminf / fmaxf return the other operand when one is NaN: np.fmin / np.fmax, not np.minimum / np.maximum
        y0, y1 = np.fmin(b[:, 0], b[:, 2]), np.fmax(b[:, 0], b[:, 2])
        x0, x1 = np.fmin(b[:, 1], b[:, 3]), np.fmax(b[:, 1], b[:, 3])
        area = (y1 - y0) * (x1 - x0)
        thr = F(iou)
        count = 0
        while count < cap and len(s):
            k = int(np.argmax(s))                                # the first maximum = the lowest index
            keep[count] = idx[k]
            count += 1
            ih = np.fmax(np.fmin(y1, y1[k]) - np.fmax(y0, y0[k]), F(0))
            iw = np.fmax(np.fmin(x1, x1[k]) - np.fmax(x0, x0[k]), F(0))
            inter = ih * iw
            val = inter / ((area + area[k]) - inter)
            val = np.where((area <= 0) | (area[k] <= 0), F(0), val)
            live = ~(val > thr)
            live[k] = False
            idx, s, y0, y1, x0, x1, area = idx[live], s[live], y0[live], y1[live], x0[live], x1[live], area[live]
    return keep, count


def nms_ref_batch(boxes, scores, cap, iou, score_thr=-np.inf):
    """boxes [n, K, 4], scores [n, K, C] -> keep [n, C, cap] int32, count [n, C] int32: nms_ref per (image, class)."""
    boxes = np.asarray(boxes, dtype=F)
    scores = np.asarray(scores, dtype=F)
    n, k, c = scores.shape
    assert boxes.shape == (n, k, 4)
    keep = np.full((n, c, cap), -1, np.int32)
    count = np.zeros((n, c), np.int32)
    for i in range(n):
        for j in range(c):
            keep[i, j], count[i, j] = nms_ref(boxes[i], scores[i, :, j], cap, iou, score_thr)
    return keep, count


# The two helpers below only CHOOSE INPUTS for the threshold tests: they model a contracted union so that a pair of boxes
# can be found on which it would differ.  The reference is nms_ref alone; nothing is ever compared with the fused value.
def iou_plain_and_fused(p, q):
    """The IoU of two boxes as float32 twice: every operation rounded (box_iou's statement), and with the union's
    subtraction fused with the intersection's product, fma(-ih, iw, ap + aq), as a contracting compiler would emit it."""
    p, q = np.asarray(p, dtype=F), np.asarray(q, dtype=F)
    py0, py1, px0, px1 = min(p[0], p[2]), max(p[0], p[2]), min(p[1], p[3]), max(p[1], p[3])
    qy0, qy1, qx0, qx1 = min(q[0], q[2]), max(q[0], q[2]), min(q[1], q[3]), max(q[1], q[3])
    ap, aq = F(F(py1 - py0) * F(px1 - px0)), F(F(qy1 - qy0) * F(qx1 - qx0))
    ih = max(F(min(py1, qy1) - max(py0, qy0)), F(0))
    iw = max(F(min(px1, qx1) - max(px0, qx0)), F(0))
    inter = F(ih * iw)
    plain = F(inter / F(F(ap + aq) - inter))
    fused = F(inter / F(np.float64(F(ap + aq)) - np.float64(ih) * np.float64(iw)))   # the product is exact in float64
    return plain, fused


def contraction_pair(seed=7):
    """Two overlapping float boxes whose IoU with a fused multiply-subtract in the union is above the float32 statement's."""
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        p = np.concatenate([rng.uniform(0, 40, 2), rng.uniform(60, 100, 2)]).astype(F)
        q = np.concatenate([rng.uniform(20, 50, 2), rng.uniform(70, 130, 2)]).astype(F)
        plain, fused = iou_plain_and_fused(p, q)
        if fused > plain:
            return p, q, plain, fused
    raise AssertionError('no such pair')


def pnet_grid_boxes(count, gw, scale=0.6):
    """The first `count` cells (row-major) of a P-Net grid gw cells wide as dif_mtcnn_propose boxes them: integer corners
    trunc((2 g + 1) / scale), trunc((2 g + 12) / scale), so that many IoUs equal 0.5 in exact arithmetic."""
    g = np.arange(count)
    gx, gy = (g % gw).astype(F), (g // gw).astype(F)
    inv = F(1) / F(scale)
    return np.stack([np.trunc((F(2) * gx + F(1)) * inv), np.trunc((F(2) * gy + F(1)) * inv),
                     np.trunc((F(2) * gx + F(12)) * inv), np.trunc((F(2) * gy + F(12)) * inv)], -1).astype(F)


def quantised_scores(rng, count, levels=17, dead=0.5):
    """`levels` score values k / (levels - 1) (0 and 1 among them: many ties), a fraction `dead` of the slots at -1."""
    s = (rng.integers(0, levels, count) / F(levels - 1)).astype(F)
    s[rng.random(count) < dead] = F(-1)
    return s


def random_boxes(rng, count, extent=400.0, reversed_frac=0.25, flat_frac=0.05):
    """Float boxes of 5 .. 60 pixels in an extent x extent frame; some with their corners swapped (on one axis or both),
    some without area (a line or a point)."""
    c = rng.uniform(0, extent, (count, 2))
    half = rng.uniform(2.5, 30.0, (count, 2))
    b = np.concatenate([c - half, c + half], 1).astype(F)
    r = rng.random(count)
    sw = r < reversed_frac
    b[sw] = b[sw][:, [2, 1, 0, 3]]
    sw = r < reversed_frac / 2
    b[sw] = b[sw][:, [0, 3, 2, 1]]
    flat = rng.random(count) < flat_frac
    b[flat, 2] = b[flat, 0]
    point = rng.random(count) < flat_frac / 4
    b[point, 2:] = b[point, :2]
    return b
