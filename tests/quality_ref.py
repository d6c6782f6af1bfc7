"""NumPy restatement of dif_face_quality and dif_pool_best (include/dif.h): int64 and float64 exactly as the header writes
them, np.minimum / np.maximum, and a brute-force best row per label.  The GPU tests compare against this bit for bit."""
import numpy as np

COLS = ('brightness', 'contrast', 'sharpness', 'clipped', 'eye_dist', 'roll', 'yaw', 'nose_drop', 'inside', 'score')


def gray(crops):
    c = np.asarray(crops).astype(np.int64)
    return (c[..., 0] + 2 * c[..., 1] + c[..., 2] + 2) >> 2


def laplacian(g):
    """[M, S-2, S-2]: the interior only."""
    return g[:, :-2, 1:-1] + g[:, 2:, 1:-1] + g[:, 1:-1, :-2] + g[:, 1:-1, 2:] - 4 * g[:, 1:-1, 1:-1]


def stats(crops, lo=0, hi=255):
    crops = np.asarray(crops)
    m = crops.shape[0]
    g = gray(crops)
    lap = laplacian(g)
    out = np.empty((m, 6), np.int64)
    out[:, 0] = g.reshape(m, -1).sum(1)
    out[:, 1] = (g * g).reshape(m, -1).sum(1)
    out[:, 2] = lap.reshape(m, -1).sum(1)
    out[:, 3] = (lap * lap).reshape(m, -1).sum(1)
    out[:, 4] = (g <= lo).reshape(m, -1).sum(1)
    out[:, 5] = (g >= hi).reshape(m, -1).sum(1)
    return out


def columns(st, size, landmarks=None, boxes=None, frame_hw=None):
    """float32 [M, 10] from the integer statistics: every value in float64 as written, rounded once."""
    st = np.asarray(st, np.int64)
    m = st.shape[0]
    n, k = size * size, (size - 2) * (size - 2)
    out = np.full((m, 10), np.nan, np.float32)
    f64 = lambda a: np.asarray(a).astype(np.float64)      # noqa: E731
    with np.errstate(all='ignore'):
        out[:, 0] = f64(st[:, 0]) / np.float64(n * 255)
        out[:, 1] = np.sqrt(f64(n * st[:, 1] - st[:, 0] * st[:, 0]) / np.float64(n * n)) / 255.0
        out[:, 2] = f64(k * st[:, 3] - st[:, 2] * st[:, 2]) / np.float64(k * k)
        out[:, 3] = f64(st[:, 4] + st[:, 5]) / np.float64(n)
        if landmarks is not None:
            lm = f64(np.asarray(landmarks, np.float32)).reshape(m, 5, 2)
            le, re, nose, ml, mr = (lm[:, i] for i in range(5))
            ex, ey = re[:, 0] - le[:, 0], re[:, 1] - le[:, 1]
            e2 = ex * ex + ey * ey
            ed = np.sqrt(e2)
            out[:, 4] = ed
            out[:, 5] = ey / ed
            t = ((nose[:, 0] - le[:, 0]) * ex + (nose[:, 1] - le[:, 1]) * ey) / e2
            out[:, 6] = 2.0 * t - 1.0
            cx, cy = (le[:, 0] + re[:, 0]) * 0.5, (le[:, 1] + re[:, 1]) * 0.5
            vx, vy = (ml[:, 0] + mr[:, 0]) * 0.5 - cx, (ml[:, 1] + mr[:, 1]) * 0.5 - cy
            out[:, 7] = ((nose[:, 0] - cx) * vx + (nose[:, 1] - cy) * vy) / (vx * vx + vy * vy)
        if boxes is not None:
            b = f64(np.asarray(boxes, np.float32)).reshape(m, 4)
            H, W = np.float64(np.float32(frame_hw[0])), np.float64(np.float32(frame_hw[1]))
            left, top, right, bottom = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
            iw = np.maximum(np.minimum(right, W) - np.maximum(left, 0.0), 0.0)
            ih = np.maximum(np.minimum(bottom, H) - np.maximum(top, 0.0), 0.0)
            out[:, 8] = (iw * ih) / ((right - left) * (bottom - top))
        score = f64(out[:, 2]) * (1.0 - f64(out[:, 3]))
        if landmarks is not None:
            score = score * np.maximum(0.0, 1.0 - np.abs(f64(out[:, 6])))
        if boxes is not None:
            score = score * f64(out[:, 8])
        out[:, 9] = score
    return out


def face_quality(crops, landmarks=None, boxes=None, frame_hw=None, lo=0, hi=255):
    """-> (stats int64 [M, 6], columns float32 [M, 10])"""
    crops = np.asarray(crops)
    st = stats(crops, lo, hi)
    return st, columns(st, crops.shape[1], landmarks, boxes, frame_hw)


def best(labels, key, row_base=0):
    """Brute force over one batch -> (labels [T], key [T] float32, row [T], counts [T]): per distinct non-negative label the
    greatest non-NaN key, ties to the lower row; all NaN: row -1, key NaN."""
    labels, key = np.asarray(labels, np.int64), np.asarray(key, np.float32)
    tl = np.unique(labels[labels >= 0])
    bk, br, cnt = np.full(tl.shape, np.nan, np.float32), np.full(tl.shape, -1, np.int64), np.zeros(tl.shape, np.int64)
    for t, l in enumerate(tl):
        rows = np.nonzero(labels == l)[0]
        cnt[t] = rows.size
        for r in rows:
            if not np.isnan(key[r]) and (br[t] < 0 or key[r] > bk[t]):
                bk[t], br[t] = key[r], row_base + r
    return tl, bk, br, cnt


def best_by_sort(labels, key, row_base=0):
    """The same answer formulated independently: one lexicographic sort by (label, NaN last, key descending, row)."""
    labels, key = np.asarray(labels, np.int64), np.asarray(key, np.float32)
    keep = np.nonzero(labels >= 0)[0]
    nan = np.isnan(key[keep])
    k64 = np.where(nan, 0.0, key[keep].astype(np.float64)) + 0.0           # (-0.0 + 0.0 = +0.0: the two zeros tie)
    order = np.lexsort((keep, -k64, nan, labels[keep]))
    sl = labels[keep][order]
    head = np.ones(sl.shape, bool)
    head[1:] = sl[1:] != sl[:-1]
    first = order[head]
    tl = sl[head]
    won = ~nan[first]
    bk = np.where(won, key[keep][first], np.float32(np.nan)).astype(np.float32)
    br = np.where(won, keep[first] + row_base, -1).astype(np.int64)
    cnt = np.diff(np.append(np.nonzero(head)[0], sl.size)).astype(np.int64)
    return tl, bk, br, cnt


class RefShots:
    """templates.BestShots on the host: the state merged add by add."""

    def __init__(self):
        self.labels, self.key = np.empty((0,), np.int64), np.empty((0,), np.float32)
        self.row, self.counts = np.empty((0,), np.int64), np.empty((0,), np.int64)
        self.payload, self.row_base = {}, 0

    def add(self, labels, key, **payload):
        labels, key = np.asarray(labels, np.int64), np.asarray(key, np.float32)
        tl, bk, br, cnt = best(labels, key, self.row_base)
        all_l = np.union1d(self.labels, tl)
        nk, nr = np.full(all_l.shape, np.nan, np.float32), np.full(all_l.shape, -1, np.int64)
        nc = np.zeros(all_l.shape, np.int64)
        npay = {name: np.zeros((all_l.size,) + np.asarray(v).shape[1:], np.asarray(v).dtype) for name, v in payload.items()}
        old, new = np.searchsorted(all_l, self.labels), np.searchsorted(all_l, tl)
        nk[old], nr[old], nc[old] = self.key, self.row, self.counts
        for name in npay:
            if self.labels.size:
                npay[name][old] = self.payload[name]
        for j, t in enumerate(new):
            nc[t] += cnt[j]
            if br[j] >= 0 and (nr[t] < 0 or bk[j] > nk[t]):
                nk[t], nr[t] = bk[j], br[j]
                for name, v in payload.items():
                    npay[name][t] = np.asarray(v)[br[j] - self.row_base]
        self.labels, self.key, self.row, self.counts, self.payload = all_l, nk, nr, nc, npay
        self.row_base += labels.size
        return np.where(labels >= 0, np.searchsorted(all_l, np.maximum(labels, 0)), -1)
