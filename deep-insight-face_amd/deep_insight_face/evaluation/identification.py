"""1:N identification protocol on top of the rank of the mate (oneshot.Gallery.rank): rank-k identification rates, the CMC
curve and the open-set detection-and-identification rate (DIR) at a false-alarm rate (FAR).

The reference has no counterpart: its evaluation speaks the 1:1 LFW protocol only (evaluation/utility.py calculate_roc /
calculate_val; here evals.py, utility.py and csrc/evalproto.hip).  `cmc` and `open_set_rates` are plain array arithmetic
on whatever they are given -- NumPy in, NumPy out; a tensor in, a tensor on its device out, without a kernel of this
library and without a host round trip.  Conventions (oneshot.Gallery.rank): rank is 0-based, -1 marks an unmated probe
(nobody enrolled), a mate whose own distance is NaN has rank len(gallery) and a NaN mate_dist.  NaN compares False
everywhere: a NaN distance passes no threshold.

With several rows per identity the honest rank-k rate counts identities, not rows: `identity_rank` reads a probe's rank off
the identity-level lists of oneshot.Gallery.topk_ids and feeds `cmc` unchanged; `evaluate_identification_ids` is the run."""
import numpy as np
import torch


def _f64(x, like):
    """`x` as a float64 array of the kind of `like`."""
    if torch.is_tensor(like):
        return torch.as_tensor(x, device=like.device).to(torch.float64)
    return np.asarray(x, dtype=np.float64)


def cmc(rank, max_rank):
    """Cumulative match characteristic -> [max_rank] float64: entry k-1 is the share of MATED probes (rank >= 0) whose
    mate ranks among the k nearest rows (rank < k); entry 0 is the rank-1 identification rate.  No mated probe: NaN."""
    max_rank = int(max_rank)
    if max_rank < 0:
        raise ValueError('max_rank must not be negative, got %d' % max_rank)
    if torch.is_tensor(rank):
        r = rank.reshape(-1)
        ks = torch.arange(1, max_rank + 1, device=r.device, dtype=r.dtype if not r.dtype.is_floating_point else torch.int64)
        mated = r >= 0
        hits = ((r[None, :] < ks[:, None]) & mated[None, :]).sum(1).to(torch.float64)
        return hits / mated.sum().to(torch.float64)
    r = np.asarray(rank).reshape(-1)
    ks = np.arange(1, max_rank + 1)
    mated = r >= 0
    hits = ((r[None, :] < ks[:, None]) & mated[None, :]).sum(1).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return hits / np.float64(mated.sum())


def open_set_rates(rank, mate_dist, unmated_min_dist, thresholds, k=1):
    """Open-set identification at each of `thresholds` [T] -> (dir [T], far [T]) float64.

    dir[t]: share of mated probes (rank >= 0) whose mate ranks among the k nearest rows AND lies within the threshold
            (rank < k and mate_dist <= thresholds[t]);
    far[t]: share of unmated probes that raise an alarm all the same -- their nearest enrolled row lies within the threshold
            (unmated_min_dist <= thresholds[t]); `unmated_min_dist` [U] holds the nearest-row distance of the unmated probes
            alone (Gallery.match on them).
    No mated probe: dir is NaN; no unmated probe: far is NaN."""
    if torch.is_tensor(rank):
        r = rank.reshape(-1)
        md = mate_dist.reshape(-1).to(torch.float64)
        um = torch.as_tensor(unmated_min_dist, device=r.device).reshape(-1).to(torch.float64)
        th = _f64(thresholds, r).reshape(-1)
        mated = r >= 0
        ok = mated & (r < int(k))
        dirs = (ok[None, :] & (md[None, :] <= th[:, None])).sum(1).to(torch.float64) / mated.sum().to(torch.float64)
        # (a device tensor as the divisor: by a Python number torch multiplies with the reciprocal, one ulp off the quotient)
        far = (um[None, :] <= th[:, None]).sum(1).to(torch.float64) / torch.full((), um.shape[0], dtype=torch.float64,
                                                                                 device=r.device)
        return dirs, far
    r = np.asarray(rank).reshape(-1)
    md = np.asarray(mate_dist, dtype=np.float64).reshape(-1)
    um = np.asarray(unmated_min_dist, dtype=np.float64).reshape(-1)
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    mated = r >= 0
    ok = mated & (r < int(k))
    with np.errstate(invalid='ignore', divide='ignore'):
        dirs = (ok[None, :] & (md[None, :] <= th[:, None])).sum(1).astype(np.float64) / np.float64(mated.sum())
        far = (um[None, :] <= th[:, None]).sum(1).astype(np.float64) / np.float64(um.shape[0])
    return dirs, far


def evaluate_identification(gallery, probes, mates, distance_metric=1, max_rank=10, thresholds=None, row_tags=None,
                            probe_masks=None):
    """One 1:N evaluation run: `gallery` an oneshot.Gallery (or the rows to enrol), `probes` [B, d], `mates` [B] the
    global row of each probe's enrolled mate, -1 for a probe of nobody enrolled.

    One Gallery.rank call on all probes and -- when thresholds are given -- one Gallery.match call on the unmated ones.
    -> {'rank', 'mate_dist', 'cmc'} and, with thresholds, {'dir', 'far', 'thresholds'} (rank-1 DIR).  NumPy probes give
    NumPy results, CUDA tensors give CUDA tensors.

    Watch-lists: with `row_tags` [len(gallery)] and `probe_masks` [B] (oneshot.Gallery.rank's; both or neither) the run is
    the one of a gallery that holds, for every probe, only the rows it is eligible for: the tagged rank -- a mate the probe
    may not see is a miss at every rank (rank len(gallery), mate_dist NaN) --, and for the unmated probes the distance of
    the nearest ELIGIBLE row, ``Gallery.topk(k=1, row_tags=, probe_masks=)``'s dist[:, 0]: NaN where the probe sees no row,
    which raises no alarm at any threshold."""
    from .. import oneshot
    g = gallery if isinstance(gallery, oneshot.Gallery) else oneshot.Gallery(gallery)
    try:
        if (row_tags is None) != (probe_masks is None):
            raise ValueError('row_tags and probe_masks go together: give both or neither')
        tagged = row_tags is not None
        rank, mate_dist = g.rank(probes, mates, distance_metric, row_tags, probe_masks)
        out = {'rank': rank, 'mate_dist': mate_dist, 'cmc': cmc(rank, max_rank)}
        if thresholds is not None:
            unmated = rank < 0
            p = probes if torch.is_tensor(probes) else np.asarray(probes, dtype=np.float32)
            if p.ndim == 1:
                p = p[None, :]
            pu = p[unmated]
            if pu.shape[0] and len(g) and tagged:
                pm = oneshot._bit_sets(probe_masks, 'probe_masks', p.shape[0], g._dev, scalar=True)
                _, um = g.topk(pu, 1, distance_metric, row_tags, pm[torch.as_tensor(unmated, device=g._dev)])
                um = um[:, 0]
            elif pu.shape[0] and len(g):
                _, um = g.match(pu, distance_metric)
            else:                                            # nobody unmated, or nothing enrolled: no alarm can be raised
                um = mate_dist[unmated]                      # (NaN for every unmated probe)
            out['thresholds'] = _f64(thresholds, rank).reshape(-1)
            out['dir'], out['far'] = open_set_rates(rank, mate_dist, um, out['thresholds'], k=1)
        return out
    finally:
        if g is not gallery:
            g.close()


def identity_rank(label_lists, probe_labels, mated):
    """Rank of the probe's identity in its identity-level list -> [B] int64: the position of probe_labels[b] in
    label_lists[b] ([B, k], the `label` of Gallery.topk_ids: distinct per row, -1 padding), k when a mated probe's identity
    is not listed (a miss at every rank the list covers), -1 for an unmated probe (mated[b] False).  Feeds `cmc`."""
    if torch.is_tensor(label_lists):
        ll = label_lists
        pl = torch.as_tensor(probe_labels, device=ll.device).reshape(-1).to(ll.dtype)
        m = torch.as_tensor(mated, device=ll.device).reshape(-1).to(torch.bool)
        k = ll.shape[1]
        hit = (ll == pl[:, None]) & (ll >= 0)
        pos = torch.arange(k, device=ll.device, dtype=torch.int64)[None, :].expand(ll.shape[0], k)
        first = torch.where(hit, pos, torch.full_like(pos, k)).amin(1) if k else torch.zeros(ll.shape[0], dtype=torch.int64,
                                                                                             device=ll.device)
        return torch.where(m, first, torch.full_like(first, -1))
    ll = np.asarray(label_lists)
    pl = np.asarray(probe_labels).reshape(-1)
    m = np.asarray(mated, dtype=bool).reshape(-1)
    k = ll.shape[1]
    hit = (ll == pl[:, None]) & (ll >= 0)
    first = np.where(hit, np.arange(k, dtype=np.int64)[None, :], k).min(1, initial=k).astype(np.int64)
    return np.where(m, first, np.int64(-1))


def evaluate_identification_ids(gallery, probes, probe_labels, row_labels, distance_metric=1, max_rank=10):
    """One identity-level 1:N evaluation run: `gallery` an oneshot.Gallery (or the rows to enrol), `probes` [B, d],
    `probe_labels` [B] and `row_labels` [len(gallery)] integer identities (a negative row label takes the row out).

    One Gallery.topk_ids call with k = max_rank; a probe is mated when its label is among the non-negative row labels.
    -> {'rank', 'cmc', 'idx', 'dist', 'label'}: rank [B] from `identity_rank` (max_rank: not among the max_rank nearest
    identities), cmc [max_rank] over the mated probes, and the lists.  NumPy probes give NumPy results, CUDA tensors give
    CUDA tensors."""
    from .. import oneshot
    g = gallery if isinstance(gallery, oneshot.Gallery) else oneshot.Gallery(gallery)
    try:
        idx, dist, label = g.topk_ids(probes, max_rank, row_labels, distance_metric)
        if torch.is_tensor(label):
            rl = torch.as_tensor(row_labels, device=label.device).reshape(-1).to(torch.int64)
            pl = torch.as_tensor(probe_labels, device=label.device).reshape(-1).to(torch.int64)
            mated = torch.isin(pl, rl[rl >= 0])
        else:
            rl = np.asarray(row_labels).reshape(-1)
            pl = np.asarray(probe_labels).reshape(-1)
            mated = np.isin(pl, rl[rl >= 0])
        rank = identity_rank(label, pl, mated)
        return {'rank': rank, 'cmc': cmc(rank, max_rank), 'idx': idx, 'dist': dist, 'label': label}
    finally:
        if g is not gallery:
            g.close()
