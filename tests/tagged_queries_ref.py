"""NumPy statement of the tagged (watch-list) range search and rank: oneshot.Gallery.within / rank with `row_tags` and
`probe_masks` (dif_match_within_tagged / dif_match_rank_tagged, and the shard-local halves dif_match_mate_dist_tagged /
dif_match_rank_at_tagged), over the oracle's distances (rank_ref.distances).

`row_tags` int64 [G] and `probe_masks` int64 [n] are tagged_ref's: eligible[p, r] = (row_tags[r] & probe_masks[p]) != 0 on the
raw 64 bits.  For probe p with query q:

    d = oracle.distance.distance(q[None, :], gallery, metric);  d[~eligible[p]] = NaN
    within:  hits = np.flatnonzero(d <= t);  count = len(hits);  idx = hits[:K] + index_base;  dist = d[hits[:K]]
             unused slots: idx -1, dist NaN                          (the three-line rule of include/dif.h)
    rank:    rank_ref.rank_row(d, mates[p], index_base)

so an ineligible row is never counted, never listed, never closer and never a tie; a mask of 0 gives count 0 and all padding;
an ineligible mate is a mate whose distance is NaN: rank G, mate_dist NaN (unmated stays -1 / NaN).  NumPy only."""
import numpy as np

import rank_ref
import tagged_ref


def within_row(d, t, K, index_base=0):
    """(count, idx [K], dist [K]) of one probe's row of distances d [G]; NaN is never a hit."""
    with np.errstate(invalid='ignore'):
        hits = np.flatnonzero(d <= np.float32(t))
    idx = np.full(K, -1, dtype=np.int64)
    dist = np.full(K, np.nan, dtype=np.float32)
    h = hits[:K]
    idx[:len(h)] = h + index_base
    dist[:len(h)] = d[h]
    return len(hits), idx, dist


def within_full(full, row_tags, probe_masks, t, K, index_base=0):
    """-> (count [n] int64, idx [n, K] int64, dist [n, K] float32) over precomputed distances full [n, G]."""
    fm = tagged_ref.masked(full, row_tags, probe_masks)
    n = fm.shape[0]
    cnt = np.zeros(n, dtype=np.int64)
    idx = np.full((n, K), -1, dtype=np.int64)
    dist = np.full((n, K), np.nan, dtype=np.float32)
    for p in range(n):
        cnt[p], idx[p], dist[p] = within_row(fm[p], t, K, index_base)
    return cnt, idx, dist


def rank_full(full, mates, row_tags, probe_masks, index_base=0):
    """-> (rank [n] int64, mate_dist [n] float32)."""
    return rank_ref.rank_full(tagged_ref.masked(full, row_tags, probe_masks), mates, index_base)


def mate_dist_full(full, mates, row_tags, probe_masks, index_base=0):
    """The first shard-local half -> (mate_dist [n] float32, owned [n] int64): owned says the shard holds the row, whatever
    its tag; the distance is NaN for a mate the probe is not eligible for."""
    fm = tagged_ref.masked(full, row_tags, probe_masks)
    n, G = fm.shape
    k = np.asarray(mates, dtype=np.int64) - index_base
    owned = ((k >= 0) & (k < G)).astype(np.int64)
    md = np.full(n, np.nan, dtype=np.float32)
    for p in np.flatnonzero(owned):
        md[p] = fm[p, k[p]]
    return md, owned


def rank_at_full(full, mates, dm, row_tags, probe_masks, index_base=0):
    """The second half -> count [n] int64: eligible rows closer than dm, or tied with it at a global index below the mate's;
    dm NaN gives G."""
    fm = tagged_ref.masked(full, row_tags, probe_masks)
    n, G = fm.shape
    rows = np.arange(G, dtype=np.int64) + index_base
    out = np.empty(n, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for p in range(n):
            out[p] = G if np.isnan(dm[p]) else int(np.count_nonzero(fm[p] < dm[p])) + \
                int(np.count_nonzero((fm[p] == dm[p]) & (rows < int(mates[p]))))
    return out


def case_mates(B, G, pick, row_tags, probe_masks, seed=1):
    """The GPU tests' mates.  `pick` [B] is each probe's identity (rows pick, pick + nid, ... with nid = max(1, G // 4)).
    Probe b:  b % 4 == 0: a random eligible row, if any (else -1);  b % 4 == 1: the highest eligible row of its own identity,
    else the identity's first row;  b % 4 == 2: the identity's first row, whatever its tag;  b % 8 == 3: -1;  b % 8 == 7: the
    identity's last row."""
    rng = np.random.default_rng(seed + G + B)
    nid = max(1, G // 4)
    el = tagged_ref.eligible(row_tags, probe_masks)
    mates = np.full(B, -1, dtype=np.int64)
    for b in range(B):
        own = np.arange(int(pick[b]), G, nid)
        u = rng.random()                                                           # (drawn for every probe: one stream)
        if b % 4 == 0:
            rows = np.flatnonzero(el[b])
            mates[b] = rows[int(u * len(rows))] if len(rows) else -1
        elif b % 4 == 1:
            ok = own[el[b, own]]
            mates[b] = ok[-1] if len(ok) else own[0]
        elif b % 4 == 2:
            mates[b] = own[0]
        elif b % 8 == 7:
            mates[b] = own[-1]
    mates.setflags(write=False)
    return mates
