"""NumPy statement of the top-k list (oneshot.Gallery.topk / dif_match_topk), over the oracle's distances (rank_ref.distances).

For probe q (`index_base` is the global index of gallery row 0):

    d     = oracle.distance.distance(q[None, :], gallery, metric)
    order = np.argsort(d, kind='stable')                       # ascending distance, ties to the lower row
    keep  = order[~np.isnan(d[order])][:k]                     # a NaN distance is never listed
    idx[:len(keep)] = keep + index_base;  dist[:len(keep)] = d[keep];  unused slots: idx -1, dist NaN"""
import numpy as np

import rank_ref


def topk_row(d, k, index_base=0):
    """(idx [k] int64, dist [k] float32) of one probe's row of distances d [G]."""
    order = np.argsort(d, kind='stable')
    keep = order[~np.isnan(d[order])][:k]
    idx = np.full(k, -1, dtype=np.int64)
    dist = np.full(k, np.nan, dtype=np.float32)
    idx[:len(keep)] = keep + index_base
    dist[:len(keep)] = d[keep]
    return idx, dist


def topk_full(full, k, index_base=0):
    """The same over precomputed distances full [B, G] -> (idx [B, k] int64, dist [B, k] float32)."""
    B = full.shape[0]
    idx = np.empty((B, k), dtype=np.int64)
    dist = np.empty((B, k), dtype=np.float32)
    for b in range(B):
        idx[b], dist[b] = topk_row(full[b], k, index_base)
    return idx, dist


def topk(probes, gallery, k, metric=1, index_base=0):
    return topk_full(rank_ref.distances(probes, gallery, metric), k, index_base)


def clear_positions(full, k, near):
    """[B, k] bool: list position j is CLEAR when the oracle's sorted distances at j-1, j, j+1 differ by more than `near`
    (a neighbour that does not exist does not count); False at the padding."""
    B = full.shape[0]
    out = np.zeros((B, k), dtype=bool)
    for b in range(B):
        sd = np.sort(full[b][~np.isnan(full[b])], kind='stable').astype(np.float64)
        n = min(k, sd.shape[0])
        if n == 0:
            continue
        with np.errstate(invalid='ignore'):                    # (inf - inf is NaN: not clear)
            gap = np.diff(sd[:n + 1]) > near                   # gap[j]: between positions j and j + 1
        left = np.concatenate([[True], gap[:n - 1]])
        right = np.concatenate([gap, [True]])[:n]              # (the last row of all has no right neighbour)
        out[b, :n] = left & right
    return out


def clear_share(full, k, near):
    """CLEAR positions as a share of all listed positions of the case (1.0 when nothing is listed)."""
    listed = np.minimum(k, (~np.isnan(full)).sum(1)).sum()
    return 1.0 if listed == 0 else float(clear_positions(full, k, near).sum()) / float(listed)


def small_gallery(probes, gallery, rows=126):
    """`rows` rows of a (degenerate) fixture gallery, in index order: up to half of them rows with a distance that is not
    finite to some ordinary probe under either metric, the rest the lowest other rows -- small enough for a list longer than the
    gallery (k = rows + 2 <= 128)."""
    odd = np.zeros(gallery.shape[0], dtype=bool)
    for metric in (0, 1):
        full = rank_ref.distances(probes, gallery, metric)
        ordinary = np.isfinite(full).any(1)                     # probes that are not degenerate themselves
        odd |= (~np.isfinite(full[ordinary])).any(0)
    pick = np.flatnonzero(odd)[:rows // 2]
    rest = np.setdiff1d(np.arange(gallery.shape[0]), pick)[:rows - pick.shape[0]]
    return gallery[np.sort(np.concatenate([pick, rest]))]
