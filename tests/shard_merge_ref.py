"""NumPy statements of the sharded-gallery merges (parallel.merge_topk / merge_topk_ids / merge_within / merge_rank, i.e.
dif_shard_merge_*) and of the shard-local rank count (dif_match_mate_dist / dif_match_rank_at).

Every merge takes the R per-shard results stacked [R, n, ...] and returns what ONE gallery holding all the rows answers.  A slot
with idx < 0 is padding whatever its distance says; distances of live slots are never NaN.

    merge_topk      live entries of the R lists sorted by (dist, global idx), the first k; padding -1 / NaN
    merge_topk_ids  the same order, of every label its first entry only, the first k; padding -1 / NaN / -1
    merge_within    counts summed; the K lowest global indices of the union, ascending; padding -1 / NaN
    merge_rank      counts summed and the distance of the LOWEST rank that owns the mate; -1 / NaN without an owner
    rank_at_row     count(d < dm) + count((d == dm) & (index_base + row < m)); dm NaN: the shard's size

TEST INFRASTRUCTURE ONLY."""
import numpy as np


def _ord(d):
    """The order-preserving integer image of float32 distances that are not NaN (bit patterns, so -0 < +0 as on the device)."""
    u = np.asarray(d, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def _sorted_live(idx, dist, by_dist):
    """Positions (r, j) of the live entries of idx [R, L] in merge order: (dist, idx) or idx alone, exact ties to the lower r."""
    R, L = idx.shape
    rr, jj = np.nonzero(idx >= 0)
    keys = (rr, idx[rr, jj]) + ((_ord(dist[rr, jj]),) if by_dist else ())     # np.lexsort: the LAST key is the primary one
    o = np.lexsort(keys)
    return rr[o], jj[o]


def merge_topk(idx, dist):
    idx, dist = np.asarray(idx, dtype=np.int64), np.asarray(dist, dtype=np.float32)
    R, n, k = idx.shape
    oi = np.full((n, k), -1, dtype=np.int64)
    od = np.full((n, k), np.nan, dtype=np.float32)
    for p in range(n):
        rr, jj = _sorted_live(idx[:, p], dist[:, p], True)
        m = min(k, rr.shape[0])
        oi[p, :m], od[p, :m] = idx[rr[:m], p, jj[:m]], dist[rr[:m], p, jj[:m]]
    return oi, od


def merge_topk_ids(idx, dist, label):
    idx, dist, label = np.asarray(idx, dtype=np.int64), np.asarray(dist, dtype=np.float32), np.asarray(label, dtype=np.int64)
    R, n, k = idx.shape
    oi = np.full((n, k), -1, dtype=np.int64)
    od = np.full((n, k), np.nan, dtype=np.float32)
    ol = np.full((n, k), -1, dtype=np.int64)
    for p in range(n):
        rr, jj = _sorted_live(idx[:, p], dist[:, p], True)
        seen, m = set(), 0
        for r, j in zip(rr, jj):
            lab = int(label[r, p, j])
            if lab in seen:
                continue
            seen.add(lab)
            if m < k:
                oi[p, m], od[p, m], ol[p, m] = idx[r, p, j], dist[r, p, j], lab
                m += 1
    return oi, od, ol


def merge_within(count, idx, dist):
    count, idx, dist = np.asarray(count, dtype=np.int64), np.asarray(idx, dtype=np.int64), np.asarray(dist, dtype=np.float32)
    R, n, K = idx.shape
    oi = np.full((n, K), -1, dtype=np.int64)
    od = np.full((n, K), np.nan, dtype=np.float32)
    for p in range(n):
        rr, jj = _sorted_live(idx[:, p], dist[:, p], False)
        m = min(K, rr.shape[0])
        oi[p, :m], od[p, :m] = idx[rr[:m], p, jj[:m]], dist[rr[:m], p, jj[:m]]
    return count.sum(0), oi, od


def merge_rank(count, owned, mate_dist):
    count, owned = np.asarray(count, dtype=np.int64), np.asarray(owned, dtype=np.int64)
    mate_dist = np.asarray(mate_dist, dtype=np.float32)
    R, n = count.shape
    any_owner = (owned != 0).any(0)
    owner = np.argmax(owned != 0, axis=0)                        # the first, i.e. lowest, rank
    rank = np.where(any_owner, count.sum(0), -1).astype(np.int64)
    md = np.where(any_owner, mate_dist[owner, np.arange(n)], np.float32(np.nan)).astype(np.float32)
    return rank, md


def mate_dist_row(d, m, index_base=0):
    """(mate_dist, owned) of global row m for one probe's distances d [G] of a shard whose row 0 is global row index_base."""
    k = int(m) - int(index_base)
    if k < 0 or k >= d.shape[0]:
        return np.float32(np.nan), 0
    return np.float32(d[k]), 1


def rank_at_row(d, m, dm, index_base=0):
    """The shard's share of the rank: d [G] its distances, m the mate's GLOBAL index (anywhere), dm the mate's distance."""
    if np.isnan(dm):
        return int(d.shape[0])
    rows = int(index_base) + np.arange(d.shape[0], dtype=np.int64)
    with np.errstate(invalid='ignore'):
        return int(np.count_nonzero(d < dm)) + int(np.count_nonzero((d == dm) & (rows < int(m))))


def mate_dist_full(full, mates, index_base=0):
    B = full.shape[0]
    md, own = np.empty(B, dtype=np.float32), np.empty(B, dtype=np.int64)
    for b in range(B):
        md[b], own[b] = mate_dist_row(full[b], mates[b], index_base)
    return md, own


def rank_at_full(full, mates, dm, index_base=0):
    return np.array([rank_at_row(full[b], mates[b], dm[b], index_base) for b in range(full.shape[0])], dtype=np.int64).reshape(-1)


def sharded_rank_full(full, bounds, mates):
    """dif_match_rank over the whole gallery, formed the sharded way from distances full [B, G] and shard row ranges
    [(lo, hi), ...] (global indices; any order): mate_dist per shard, the owner's distance, rank_at per shard, merge_rank."""
    parts = [mate_dist_full(full[:, lo:hi], mates, lo) for lo, hi in bounds]
    md, own = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    _, dm = merge_rank(np.zeros_like(own), own, md)
    cnt = np.stack([rank_at_full(full[:, lo:hi], mates, dm, lo) for lo, hi in bounds])
    return merge_rank(cnt, own, md)


def within_full(full, tolerance, K, index_base=0):
    """oneshot.Gallery.within over precomputed distances full [B, G]: (count [B], idx [B, K], dist [B, K])."""
    B = full.shape[0]
    count = np.zeros(B, dtype=np.int64)
    idx = np.full((B, K), -1, dtype=np.int64)
    dist = np.full((B, K), np.nan, dtype=np.float32)
    for b in range(B):
        with np.errstate(invalid='ignore'):
            hits = np.flatnonzero(full[b] <= tolerance)
        count[b] = hits.shape[0]
        m = min(K, hits.shape[0])
        idx[b, :m], dist[b, :m] = hits[:m] + index_base, full[b, hits[:m]]
    return count, idx, dist
