"""NumPy statement of the identity-level top-k list (oneshot.Gallery.topk_ids / dif_match_topk_ids), over the oracle's
distances (rank_ref.distances).

For probe q with `row_labels` [G] int64, an excluded label (negative: none) and `index_base` the global index of row 0:

    d     = oracle.distance.distance(q[None, :], gallery, metric)
    ok    = ~isnan(d) & (row_labels >= 0) & (row_labels != exclude)
    order = np.argsort(d, kind='stable');  order = order[ok[order]]
    first = order[np.sort(np.unique(row_labels[order], return_index=True)[1])]   # each identity's first, i.e. best, row
    keep  = first[:k]
    idx = keep + index_base;  dist = d[keep];  label = row_labels[keep];  unused slots: idx -1, dist NaN, label -1

Also the CLEAR positions of the per-identity best distances (where metric 1 must agree with NumPy row for row), the select
stage's tile schedule simulated on the oracle's distances, and the crowd input of the work test."""
import numpy as np


def firsts(d, labels, exclude=-1):
    """Every usable identity's best row of one probe's distances d [G], in list order (ascending distance, ties to the lower
    row)."""
    labels = np.asarray(labels, dtype=np.int64)
    ok = ~np.isnan(d) & (labels >= 0) & (labels != exclude)
    order = np.argsort(d, kind='stable')
    order = order[ok[order]]
    return order[np.sort(np.unique(labels[order], return_index=True)[1])]


def topk_ids_row(d, labels, k, exclude=-1, index_base=0):
    """(idx [k] int64, dist [k] float32, label [k] int64) of one probe's row of distances d [G]."""
    labels = np.asarray(labels, dtype=np.int64)
    keep = firsts(d, labels, exclude)[:k]
    idx = np.full(k, -1, dtype=np.int64)
    dist = np.full(k, np.nan, dtype=np.float32)
    lab = np.full(k, -1, dtype=np.int64)
    idx[:len(keep)] = keep + index_base
    dist[:len(keep)] = d[keep]
    lab[:len(keep)] = labels[keep]
    return idx, dist, lab


def _excl(exclude, B):
    return np.full(B, -1, dtype=np.int64) if exclude is None else np.asarray(exclude, dtype=np.int64).reshape(B)


def topk_ids_full(full, labels, k, exclude=None, index_base=0):
    """The same over precomputed distances full [B, G] -> (idx, dist, label), each [B, k]."""
    B = full.shape[0]
    ex = _excl(exclude, B)
    idx = np.empty((B, k), dtype=np.int64)
    dist = np.empty((B, k), dtype=np.float32)
    lab = np.empty((B, k), dtype=np.int64)
    for b in range(B):
        idx[b], dist[b], lab[b] = topk_ids_row(full[b], labels, k, int(ex[b]), index_base)
    return idx, dist, lab


def clear_positions(full, labels, k, near, exclude=None):
    """[B, k] bool: list position j is CLEAR when the per-identity best distances at j-1, j, j+1 of that sequence differ by
    more than `near` (a neighbour that does not exist does not count); False at the padding."""
    B = full.shape[0]
    ex = _excl(exclude, B)
    out = np.zeros((B, k), dtype=bool)
    for b in range(B):
        sd = full[b][firsts(full[b], labels, int(ex[b]))].astype(np.float64)
        n = min(k, sd.shape[0])
        if n == 0:
            continue
        with np.errstate(invalid='ignore'):                    # (inf - inf is NaN: not clear)
            gap = np.diff(sd[:n + 1]) > near                   # gap[j]: between positions j and j + 1
        left = np.concatenate([[True], gap[:n - 1]])
        right = np.concatenate([gap, [True]])[:n]              # (the last identity of all has no right neighbour)
        out[b, :n] = left & right
    return out


def clear_share(full, labels, k, near, exclude=None):
    """CLEAR positions as a share of all listed positions of the case (1.0 when nothing is listed)."""
    B = full.shape[0]
    ex = _excl(exclude, B)
    listed = sum(min(k, firsts(full[b], labels, int(ex[b])).shape[0]) for b in range(B))
    return 1.0 if listed == 0 else float(clear_positions(full, labels, k, near, exclude).sum()) / float(listed)


def simulated_tiles(d, labels, k, rule='grow', exclude=-1, seed=0, tile=128):
    """How many 128-row tiles the select stage evaluates for one probe's distances d [G], with the words formed from the
    oracle's distances (the minimum over ALL rows of the tile, -inf when one is NaN) and the band E taken as 0, so that "word
    > thr_out" reads "word > t".  Rules:
      'grow'    the kernel's: s = seed or k; loop { kappa = the s-th smallest word; evaluate the tiles with word <= kappa;
                t = the k-th kept distance or +inf; left = the tiles not evaluated that are not > t; leave when left <= s or
                every tile is evaluated; s *= 2 }; then the sweep over `left`
      'single'  one seed of s tiles, then the sweep (dif_match_topk's schedule)
      'ideal'   tiles in ascending word order, stop when the next word is above the current t"""
    labels = np.asarray(labels, dtype=np.int64)
    G = d.shape[0]
    gt = (G + tile - 1) // tile
    if gt == 0:
        return 0
    pad = np.full(gt * tile, np.inf, dtype=np.float64)
    pad[:G] = d
    pad = pad.reshape(gt, tile)
    words = np.where(np.isnan(pad).any(1), -np.inf, np.nanmin(np.where(np.isnan(pad), np.inf, pad), axis=1))
    done = np.zeros(gt, dtype=bool)

    def kth():
        seen = np.repeat(done, tile)[:G]
        best = d[firsts(np.where(seen, d, np.nan), labels, exclude)]
        return np.inf if best.shape[0] < k else float(best[k - 1])

    if rule == 'ideal':
        for n, t in enumerate(np.argsort(words, kind='stable')):
            if words[t] > kth():
                return n
            done[t] = True
        return gt
    s = seed if seed > 0 else k
    ranked = np.sort(words)
    while True:
        if s >= gt:
            return gt
        done |= words <= ranked[s - 1]
        t = kth()
        left = ~done & ~(words > t)
        if rule == 'single' or int(left.sum()) <= s:
            break
        s *= 2
    return int((done | left).sum())


def crowd_inputs(probes, gallery, labels, lo=1280, hi=2048, noise=0.02, seed=5):
    """The crowd input of the work test: rows [lo, hi) overwritten by near-copies of probe 0 under ONE extra label, and every
    probe a near-copy of probe 0 -- one identity fills the six tiles nearest to every probe.
    -> (probes, gallery, labels), new arrays."""
    rng = np.random.default_rng(seed)
    D = gallery.shape[1]
    gal = gallery.copy()
    gal[lo:hi] = (probes[0][None, :] + noise * rng.standard_normal((hi - lo, D))).astype(np.float32)
    lab = np.asarray(labels, dtype=np.int64).copy()
    lab[lo:hi] = lab.max() + 1
    pr = (probes[0][None, :] + noise * rng.standard_normal(probes.shape)).astype(np.float32)
    return pr, gal, lab
