"""NumPy statement of the rank of the mate (oneshot.Gallery.rank / dif_match_rank), over the oracle's distances.

For probe q with mate row m (a global index; `index_base` is the global index of gallery row 0):

    d    = oracle.distance.distance(q[None, :], gallery, metric)
    dm   = d[m - index_base]
    rank = count(d < dm) + count(d[:m - index_base] == dm)          # NaN compares False: a NaN distance is never closer

m outside [index_base, index_base + G) -- -1 by convention -- is an unmated probe: rank -1, mate_dist NaN.
dm NaN with the mate given: rank G ("behind every row"), mate_dist NaN."""
import numpy as np

from oracle import distance as od


def rank_row(d, m, index_base=0):
    """(rank, mate_dist) of global row m in one probe's row of distances d [G]."""
    G = d.shape[0]
    k = int(m) - int(index_base)
    if k < 0 or k >= G:
        return -1, np.float32(np.nan)
    dm = d[k]
    if np.isnan(dm):
        return G, np.float32(np.nan)
    with np.errstate(invalid='ignore'):
        return int(np.count_nonzero(d < dm)) + int(np.count_nonzero(d[:k] == dm)), np.float32(dm)


def rank_full(full, mates, index_base=0):
    """The same over precomputed distances full [B, G] -> (rank [B] int64, mate_dist [B] float32)."""
    B = full.shape[0]
    rank = np.empty(B, dtype=np.int64)
    dist = np.empty(B, dtype=np.float32)
    for b in range(B):
        rank[b], dist[b] = rank_row(full[b], mates[b], index_base)
    return rank, dist


def distances(probes, gallery, metric):
    with np.errstate(all='ignore'):
        if gallery.shape[0] == 0:
            return np.zeros((probes.shape[0], 0), dtype=np.float32)
        return np.stack([od.distance(q[None, :], gallery, metric) for q in probes]).astype(np.float32, copy=False)


def rank(probes, gallery, mates, metric=1, index_base=0):
    return rank_full(distances(probes, gallery, metric), mates, index_base)
