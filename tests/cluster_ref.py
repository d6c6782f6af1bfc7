"""CPU oracle of Gallery.cluster (dif_gallery_cluster): oracle.distance plus a NumPy union-find.  TEST INFRASTRUCTURE ONLY.

    for i in range(G):                                   # every enrolled row is a probe
        d = distance(rows[i][None, :], rows[:i + 1], metric)      # reference float32 values, rows 0..i only
        for j in np.flatnonzero(d <= t):                 # inclusive; NaN <= t is False
            unite(i, j)
    label[i] = index_base + min(row numbers of i's component);  n_clusters = number of components

`clamp` restates the gallery option "clamp_nan" 1: under metric 1 a similarity that rounding pushed beyond +-1 is compared as
the distance of the clamped similarity (0 or 1) instead of the reference's NaN; a NaN similarity stays NaN."""
import math

import numpy as np

from oracle import distance as od


def lower_distances(rows, metric, clamp=False, first_row=0):
    """-> list over i in [first_row, G) of distance(rows[i], rows[:i + 1]) (float32 [i + 1])."""
    out = []
    with np.errstate(all='ignore'):
        for i in range(first_row, rows.shape[0]):
            q, g = rows[i][None, :], rows[:i + 1]
            if metric == 1 and clamp:
                d = np.arccos(np.clip(od.similarity(q, g), np.float32(-1), np.float32(1))) / math.pi
            else:
                d = od.distance(q, g, metric)
            out.append(np.asarray(d, dtype=np.float32))
    return out


def pair_values(lower):
    """The distances of the pairs j < i (no self pairs) that are finite, as one float64 array."""
    v = np.concatenate([d[:-1] for d in lower]) if lower else np.zeros(0, dtype=np.float32)
    return v[np.isfinite(v)].astype(np.float64)


def cluster_from(lower, G, t, index_base=0, first_row=0, labels=None):
    """The union-find over the edges of `lower` (lower_distances(..., first_row)) at tolerance t -> (labels [G] int64, n_clusters)."""
    parent = np.arange(G, dtype=np.int64)
    if first_row:
        parent[:first_row] = np.asarray(labels[:first_row], dtype=np.int64) - index_base

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    t = np.float32(t)
    with np.errstate(invalid='ignore'):
        for i, d in zip(range(first_row, G), lower):
            for j in np.flatnonzero(d <= t):
                a, b = find(i), find(int(j))
                if a != b:
                    parent[max(a, b)] = min(a, b)            # (any rule would do: the labels below are canonical)
    root = np.array([find(i) for i in range(G)], dtype=np.int64)
    low = np.full(G, G, dtype=np.int64)
    np.minimum.at(low, root, np.arange(G, dtype=np.int64))   # the smallest row of every component
    return index_base + low[root] if G else np.zeros(0, dtype=np.int64), int(len(np.unique(root)))


def cluster(rows, t, metric, clamp=False, index_base=0, first_row=0, labels=None):
    rows = np.asarray(rows, dtype=np.float32)
    return cluster_from(lower_distances(rows, metric, clamp, first_row), rows.shape[0], t, index_base, first_row, labels)
