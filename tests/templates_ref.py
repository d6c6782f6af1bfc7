"""Template pooling, restated in NumPy: the contract of deep_insight_face.templates and of dif_pool_* (include/dif.h).

One template per distinct non-negative label, in ascending label order.  A template's sum runs over its rows in ascending
row number, one float32 add after the other, starting AT the first row (np.add.reduce(x[labels == l], axis=0), bit for
bit: tests/test_templates_ref.py); with weights the product w_r * x_r is rounded to float32 before it is added.  The mean
divides by float32(count), or by the float32 sum of the weights; the normalised template divides the mean by
np.linalg.norm(mean, axis=1, keepdims=True).  Rows with a negative label are left out (index -1).

``RefPool`` keeps the state of an incremental pool; adding in chunks continues every stored sum, so the result equals one
add of the concatenation.  ``reverse`` and ``contracted`` give the two WRONG evaluations a test wants to tell from the
right one: the rows of a template in descending row number, and the multiply-add fused
(float32(float64(w) * float64(x) + float64(acc))).
"""
import numpy as np


class RefPool:
    def __init__(self, d, weighted=False):
        self.d, self.weighted = int(d), bool(weighted)
        self.labels = np.zeros((0,), np.int64)
        self.sums = np.zeros((0, self.d), np.float32)
        self.wsum = np.zeros((0,), np.float32) if weighted else None
        self.counts = np.zeros((0,), np.int64)

    def add(self, x, labels, weights=None, reverse=False, contracted=False):
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, self.d)
        labels = np.asarray(labels).astype(np.int64).reshape(-1)
        assert x.shape[0] == labels.shape[0] and (weights is not None) == self.weighted
        w = None if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
        merged = np.union1d(self.labels, labels[labels >= 0]).astype(np.int64)
        T = merged.shape[0]
        sums = np.zeros((T, self.d), np.float32)
        wsum = np.zeros((T,), np.float32)
        counts = np.zeros((T,), np.int64)
        started = np.zeros((T,), bool)
        old = np.searchsorted(merged, self.labels)
        sums[old], counts[old], started[old] = self.sums, self.counts, True
        if self.weighted:
            wsum[old] = self.wsum
        index = np.where(labels >= 0, np.searchsorted(merged, np.maximum(labels, 0)), -1).astype(np.int64)
        rows = range(x.shape[0] - 1, -1, -1) if reverse else range(x.shape[0])
        with np.errstate(all='ignore'):
            for r in rows:
                t = index[r]
                if t < 0:
                    continue
                if not started[t]:
                    sums[t] = x[r] if w is None else w[r] * x[r]
                    if w is not None:
                        wsum[t] = w[r]
                    started[t] = True
                elif w is None:
                    np.add(sums[t], x[r], out=sums[t])
                else:
                    if contracted:
                        sums[t] = (np.float64(w[r]) * x[r].astype(np.float64) + sums[t].astype(np.float64)).astype(np.float32)
                    else:
                        np.add(sums[t], w[r] * x[r], out=sums[t])
                    wsum[t] = wsum[t] + w[r]
                counts[t] += 1
        self.labels, self.sums, self.counts = merged, sums, counts
        if self.weighted:
            self.wsum = wsum
        return index

    def means(self):
        with np.errstate(all='ignore'):
            if self.weighted:
                return self.sums / self.wsum[:, None]
            return self.sums / self.counts.astype(np.float32)[:, None]

    def templates(self, normalize=True):
        m = self.means()
        if not normalize:
            return m
        with np.errstate(all='ignore'):
            return m / np.sqrt(np.add.reduce(m * m, axis=1, keepdims=True))


def pool_templates(x, labels, weights=None, normalize=True, reverse=False, contracted=False):
    """-> (templates [T, d], template_labels [T], counts [T], index [N]), as deep_insight_face.templates.pool_templates."""
    x = np.asarray(x, dtype=np.float32)
    pool = RefPool(x.shape[1], weights is not None)
    index = pool.add(x, labels, weights, reverse=reverse, contracted=contracted)
    return pool.templates(normalize), pool.labels, pool.counts, index
