"""Data-parallel embed + gallery-sharded match across the GPUs of one node.

The reference is single-process (SURVEY.md section 5 "distributed communication backend:
none"); this is new work named by north_star.  One process per GPU, torch.distributed
for the exchange (backend "nccl" is RCCL over xGMI on ROCm; "gloo" on CPU for tests):

  1. every rank embeds its own slice of the batch                    [b, d]
  2. ONE all-gather of the per-rank embeddings                       [R*b, d]   (8 MiB at B=4096)
  3. every rank matches ALL probes against ITS gallery shard         (key, idx, dist)[R*b]
  4. ONE all-gather of the packed per-rank results                   [R][{key, dist, idx}[R*b]] (tiny)
  5. merge: lowest key (= the reference distance), then lowest GLOBAL index == np.argmin over the whole gallery

There is no other collective on the data path.  The local compute (steps 1, 3, 5) is the
HIP library; tests on CPU inject stand-ins for it to exercise steps 2 and 4.

The other gallery queries follow the same pattern -- ShardedGallery.topk, topk_ids, within, rank and roc: all-gather the
probes (and the per-probe arrays), run the local query on all R*b probes, ONE all-gather of the packed per-rank results,
merge on the device (merge_topk, merge_topk_ids, merge_within, merge_rank; roc's int64 counts add).  `rank` takes two result
exchanges: the mate's distance has to reach the shards that do not hold the mate before they can count.  Every answer equals,
bit for bit, that of one oneshot.Gallery holding all the rows (DESIGN.md has the arguments).  `cluster` and `dbscan` do not
merge (their edges cross shards); `update` / `remove` need a policy for which rank owns a row: neither is offered here.
"""
import numpy as np
import torch
import torch.distributed as dist

WITHIN_GATHER_MAX = 1 << 30   # bytes of gathered lists ShardedGallery.within accepts (see within_gather_bytes)


def shard_bounds(n_rows, world_size, rank):
    """Contiguous row range [lo, hi) of `rank`: the first n % R ranks hold one extra row."""
    base, extra = divmod(int(n_rows), int(world_size))
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


class _StepBuffers:
    """Device buffers of one (B, d) step shape, allocated once: the gathered probes, this rank's packed
    partial result and the gathered partial results, the merged output."""

    def __init__(self, world, b, d, dev):
        B = world * b
        self.probes = torch.empty((B, d), dtype=torch.float32, device=dev)
        # one rank's record = { float key[B]; float dist[B]; int64 idx[B]; } (include/dif.h: dif_match_merge_packed)
        self.packed = torch.empty((world, 4 * B), dtype=torch.float32, device=dev)
        self.local = torch.empty((4 * B,), dtype=torch.float32, device=dev)      # this rank's record (not aliasing `packed`)
        self.out_idx = torch.empty((B,), dtype=torch.int64, device=dev)
        self.out_dist = torch.empty((B,), dtype=torch.float32, device=dev)

    def record(self, B):
        rec = self.local
        return rec[0:B], rec[B:2 * B], rec[2 * B:4 * B].view(torch.int64)


def _hip_match(gallery, probes, metric):
    idx, d, key = gallery.match(probes, metric, return_key=True)
    return key, idx, d


def _hip_merge(keys, idx, dists):
    from . import _native as N
    R, B = keys.shape
    oi = torch.empty((B,), dtype=torch.int64, device=keys.device)
    od = torch.empty((B,), dtype=torch.float32, device=keys.device)
    N.check(N.lib.dif_match_merge(N.ptr(keys), N.ptr(idx), N.ptr(dists), R, B, N.ptr(oi), N.ptr(od), N.stream_ptr()))
    return oi, od


def _merge_args(fn, parts):
    """The stacked per-shard results of a merge: CUDA tensors, dense, of the library's dtypes, and of one leading shape."""
    first = parts[0][1]
    for name, t, dt, shape in parts:
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise ValueError('%s: %s must be a contiguous %s CUDA tensor' % (fn, name, dt))
        if t.device != first.device:
            raise ValueError('%s: %s is on %s, %s on %s' % (fn, name, t.device, parts[0][0], first.device))
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError('%s: %s must have shape %s, got %s' % (fn, name, list(shape), tuple(t.shape)))


def merge_topk(idx, dist_):
    """R per-shard `topk` results stacked [R, n, k] (int64 global indices, float32 distances, -1 / NaN padding behind) -> the
    whole gallery's (idx [n, k], dist [n, k]): the first k of the union by (distance, global index).  On the device
    (dif_shard_merge_topk); an R outside [1, 64] or a k outside [1, 128] raises ValueError."""
    from . import _native as N
    if not torch.is_tensor(idx) or idx.dim() != 3:
        raise ValueError('merge_topk: idx must be [R, n, k]')
    _merge_args('merge_topk', (('idx', idx, torch.int64, None), ('dist', dist_, torch.float32, idx.shape)))
    R, n, k = idx.shape
    oi = torch.empty((n, k), dtype=torch.int64, device=idx.device)
    od = torch.empty((n, k), dtype=torch.float32, device=idx.device)
    N.check(N.lib.dif_shard_merge_topk(N.ptr(idx), N.ptr(dist_), R, n, k, N.ptr(oi), N.ptr(od), N.stream_ptr()), ValueError)
    return oi, od


def merge_topk_ids(idx, dist_, label):
    """R per-shard `topk_ids` results stacked [R, n, k] -> (idx, dist, label), each [n, k]: the union by (distance, global
    index), of every label its first entry, the first k of those; padding -1 / NaN / -1 (dif_shard_merge_topk_ids)."""
    from . import _native as N
    if not torch.is_tensor(idx) or idx.dim() != 3:
        raise ValueError('merge_topk_ids: idx must be [R, n, k]')
    _merge_args('merge_topk_ids', (('idx', idx, torch.int64, None), ('dist', dist_, torch.float32, idx.shape),
                                   ('label', label, torch.int64, idx.shape)))
    R, n, k = idx.shape
    oi = torch.empty((n, k), dtype=torch.int64, device=idx.device)
    od = torch.empty((n, k), dtype=torch.float32, device=idx.device)
    ol = torch.empty((n, k), dtype=torch.int64, device=idx.device)
    N.check(N.lib.dif_shard_merge_topk_ids(N.ptr(idx), N.ptr(dist_), N.ptr(label), R, n, k, N.ptr(oi), N.ptr(od), N.ptr(ol),
                                           N.stream_ptr()), ValueError)
    return oi, od, ol


def merge_within(count, idx, dist_):
    """R per-shard `within` results stacked -- count [R, n], idx and dist [R, n, K] -> (count [n], idx [n, K], dist [n, K]):
    the counts summed, the K lowest global indices of the union in ascending order, padding -1 / NaN
    (dif_shard_merge_within).  K may be 0."""
    from . import _native as N
    if not torch.is_tensor(idx) or idx.dim() != 3:
        raise ValueError('merge_within: idx must be [R, n, K]')
    _merge_args('merge_within', (('idx', idx, torch.int64, None), ('dist', dist_, torch.float32, idx.shape),
                                 ('count', count, torch.int64, idx.shape[:2])))
    R, n, K = idx.shape
    oc = torch.empty((n,), dtype=torch.int64, device=idx.device)
    oi = torch.empty((n, K), dtype=torch.int64, device=idx.device)
    od = torch.empty((n, K), dtype=torch.float32, device=idx.device)
    N.check(N.lib.dif_shard_merge_within(N.ptr(count), N.ptr(idx) if K else None, N.ptr(dist_) if K else None, R, n, K,
                                         N.ptr(oc), N.ptr(oi) if K else None, N.ptr(od) if K else None, N.stream_ptr()),
            ValueError)
    return oc, oi, od


def merge_rank(count, owned, mate_dist):
    """R per-shard results of Gallery.mate_dist_into / rank_at_into stacked [R, n] (int64 counts, int64 0 / 1 owned, float32
    mate_dist) -> (rank [n] int64, mate_dist [n] float32): the counts summed and the owner's distance, or -1 / NaN where no
    shard owns the mate.  Were two shards to own it (overlapping shards: not allowed) the lowest rank wins
    (dif_shard_merge_rank)."""
    from . import _native as N
    if not torch.is_tensor(count) or count.dim() != 2:
        raise ValueError('merge_rank: count must be [R, n]')
    _merge_args('merge_rank', (('count', count, torch.int64, None), ('owned', owned, torch.int64, count.shape),
                               ('mate_dist', mate_dist, torch.float32, count.shape)))
    R, n = count.shape
    rk = torch.empty((n,), dtype=torch.int64, device=count.device)
    md = torch.empty((n,), dtype=torch.float32, device=count.device)
    N.check(N.lib.dif_shard_merge_rank(N.ptr(count), N.ptr(owned), N.ptr(mate_dist), R, n, N.ptr(rk), N.ptr(md),
                                       N.stream_ptr()), ValueError)
    return rk, md


def within_gather_bytes(world, b, max_hits):
    """Bytes of the lists ShardedGallery.within gathers on every rank: R records of R*b probes x max_hits slots x 12 bytes."""
    return int(world) * int(world) * int(b) * int(max_hits) * 12


def _pack(parts):
    """One rank's record: the results of a local query as ONE dense float32 buffer (int64 parts first: they stay 8-byte aligned)."""
    flat = [t.contiguous().view(-1).view(torch.float32) for t in parts if t.numel()]      # (an empty part has no bytes to view)
    return torch.cat(flat) if flat else torch.empty((0,), dtype=torch.float32, device=parts[0].device)


def _unpack(gathered, specs):
    """[R, record] float32 -> one dense [R, *shape] tensor per (dtype, shape) of the record."""
    out, at = [], 0
    R = gathered.shape[0]
    for dt, shape in specs:
        n = int(np.prod(shape, dtype=np.int64)) * (2 if dt == torch.int64 else 1)
        if n == 0:
            out.append(torch.empty((R,) + tuple(shape), dtype=dt, device=gathered.device))
            continue
        part = torch.empty((R * n,), dtype=torch.float32, device=gathered.device)  # a fresh, aligned block: int64 is viewed on it
        part.view(R, n).copy_(gathered[:, at:at + n])
        out.append(part.view(dt).view((R,) + tuple(shape)))
        at += n
    return out


class ShardedGallery:
    """Row shard of a gallery plus the two collectives around the local match."""

    def __init__(self, shard_rows, index_base, group=None, match_fn=None, merge_fn=None, gallery=None,
                 force_collectives=False, check_batch='always'):
        """`force_collectives`: with a world of ONE rank the two all-gathers and the merge are short-cut (they
        would move a rank's data to itself); True runs them all the same -- the whole N > 1 branch over the real
        backend on a single GPU (tests/test_parallel_gpu.py::test_rccl_single_rank_runs_the_sharded_branch).
        Needs an initialised process group.
        `check_batch`: every rank must bring the SAME number of probes b to a step (all_gather_into_tensor sizes its
        buffers from this rank's b: a ragged last batch on one rank would otherwise hang or gather garbage).
        'always' (default) compares the ranks' b before every step -- one 8-byte all-gather and a host read, raising
        ValueError on EVERY rank when they differ; 'first' only when this rank meets a (b, d) shape for the first
        time (no host read in a steady serving loop: what bench.py times; a rank whose shape is cached does not take
        part, so it protects the first step of a shape only); 'never' trusts the caller."""
        if check_batch not in ('always', 'first', 'never'):
            raise ValueError("check_batch must be 'always', 'first' or 'never'")
        self.check_batch = check_batch
        self.phase_events = None      # bench.py: a list to which every step appends its five CUDA events (see match)
        self.group = group
        self.force = bool(force_collectives)
        if self.force and not dist.is_initialized():
            raise RuntimeError('force_collectives needs torch.distributed.init_process_group first')
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        # (this rank's number; `rank` itself is the query, as on oneshot.Gallery)
        self.rank_index = dist.get_rank(group) if dist.is_initialized() else 0
        self._match = match_fn
        self._merge = merge_fn
        self._bufs = {}
        self._seen = set()            # (query, b, d) shapes topk / topk_ids / within / rank / roc have met (check_batch 'first')
        if gallery is not None:
            self.gallery = gallery
        elif match_fn is None:
            from .oneshot import Gallery
            self.gallery = Gallery(shard_rows, index_base=index_base)
        else:
            self.gallery = (shard_rows, index_base)     # stand-in compute gets the raw shard

    def all_gather_embeddings(self, local, out=None):
        """Step 2.  `local` is [b, d] on every rank (same b); returns [R*b, d]."""
        if self.world == 1 and not self.force:
            return local
        if out is None:
            out = torch.empty((self.world * local.shape[0], local.shape[1]), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(out, local.contiguous(), group=self.group)
        return out

    def _check_same_batch(self, b, device, first_time):
        """Raises ValueError on every rank when the ranks' probe counts differ (see __init__: check_batch)."""
        if self.world == 1 or self.check_batch == 'never' or (self.check_batch == 'first' and not first_time):
            return
        mine = torch.tensor([int(b)], dtype=torch.int64, device=device)
        sizes = torch.empty((self.world,), dtype=torch.int64, device=device)
        dist.all_gather_into_tensor(sizes, mine, group=self.group)
        sizes = [int(v) for v in sizes.cpu().tolist()]
        if any(v != sizes[0] for v in sizes):
            raise ValueError('ShardedGallery.match: every rank must bring the same number of probes per step, got %s '
                             '(pad the ragged last batch, or drop it, on all ranks alike)' % sizes)

    def match(self, local_embeddings, distance_metric=1, copy=True):
        """Steps 2-5: returns (idx[R*b] int64 global, dist[R*b] float32), identical on every rank.
        `local_embeddings`: [b, emd_size], NumPy or torch on any device / float dtype / strides (converted to a
        dense float32 tensor on this rank's GPU, like Gallery.match; a wrong width raises ValueError).
        On the HIP path the match writes its (key, dist, idx) straight into this rank's record of one packed,
        preallocated buffer, ONE all-gather moves the records, dif_match_merge_packed reduces them.
        copy=True (default) returns fresh tensors; copy=False returns the step buffers themselves, which the
        NEXT call of the same shape overwrites -- the allocation-free form for a serving loop."""
        if self._match is not None:
            return self._match_injected(local_embeddings, distance_metric)
        from . import _native as N
        local_embeddings, _ = N.to_device_f32(local_embeddings, self.gallery._dev)
        if local_embeddings.dim() != 2 or local_embeddings.shape[1] != self.gallery.emd_size:
            raise ValueError('embeddings must be [b, %d], got %s' % (self.gallery.emd_size,
                                                                      tuple(local_embeddings.shape)))
        b, d = local_embeddings.shape
        key = (b, d, local_embeddings.device)
        buf = self._bufs.get(key)
        self._check_same_batch(b, local_embeddings.device, buf is None)
        if buf is None:
            buf = self._bufs[key] = _StepBuffers(self.world, b, d, local_embeddings.device)
        B = self.world * b
        evs = None
        if self.phase_events is not None:                     # [start, embeddings gathered, matched, records gathered, merged]
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            self.phase_events.append(evs)
            evs[0].record()
        probes = self.all_gather_embeddings(local_embeddings, buf.probes)
        if evs:
            evs[1].record()
        k, dd, ix = buf.record(B)
        if self.world == 1 and not self.force:
            self.gallery.match_into(probes, distance_metric, buf.out_idx, buf.out_dist)
            if evs:
                for e in evs[2:]:
                    e.record()
        else:
            self.gallery.match_into(probes, distance_metric, ix, dd, k)
            if evs:
                evs[2].record()
            dist.all_gather_into_tensor(buf.packed.view(-1), buf.local, group=self.group)
            if evs:
                evs[3].record()
            N.check(N.lib.dif_match_merge_packed(N.ptr(buf.packed), self.world, B, N.ptr(buf.out_idx),
                                                 N.ptr(buf.out_dist), N.stream_ptr()))
            if evs:
                evs[4].record()
        if copy:
            return buf.out_idx.clone(), buf.out_dist.clone()
        return buf.out_idx, buf.out_dist

    def _match_injected(self, local_embeddings, distance_metric):
        """The same exchange with stand-in compute (CPU tests over gloo: the HIP kernels need a GPU)."""
        shape = tuple(local_embeddings.shape)
        self._check_same_batch(shape[0], local_embeddings.device, shape not in self._bufs)
        self._bufs.setdefault(shape, True)
        probes = self.all_gather_embeddings(local_embeddings)
        key, idx, d = self._match(self.gallery, probes, distance_metric)
        if self.world == 1 and not self.force:
            return idx, d
        B = probes.shape[0]
        rec = torch.cat([key.to(torch.float32), d.to(torch.float32), idx.to(torch.int64).view(torch.float32)])   # [4B]
        allrec = torch.empty((self.world * 4 * B,), dtype=torch.float32, device=rec.device)
        dist.all_gather_into_tensor(allrec, rec.contiguous(), group=self.group)
        allrec = allrec.view(self.world, 4 * B)
        keys, dists = allrec[:, 0:B].contiguous(), allrec[:, B:2 * B].contiguous()
        ix = allrec[:, 2 * B:4 * B].contiguous().view(torch.int64)
        return (self._merge or _hip_merge)(keys, ix, dists)

    # ---- the other gallery queries: gather the probes, query the shard with all of them, gather the records, merge

    def _local(self):
        return self.world == 1 and not self.force

    def _begin(self, what, local_probes):
        """-> (probes [b, d] float32 on the shard's device, NumPy in?, b), the ranks' b compared as `match` does."""
        if self._match is not None:
            raise RuntimeError('ShardedGallery.%s needs the HIP gallery (match_fn stand-ins serve `match` only)' % what)
        from . import _native as N
        p, was_np = N.to_device_f32(local_probes, self.gallery._dev)
        if p.dim() == 1:
            p = p[None, :]
        if p.dim() != 2 or p.shape[1] != self.gallery.emd_size:
            raise ValueError('probes must be [b, %d], got %s' % (self.gallery.emd_size, tuple(p.shape)))
        key = (what, p.shape[0], p.shape[1])
        self._check_same_batch(p.shape[0], p.device, key not in self._seen)
        self._seen.add(key)
        return p, was_np, p.shape[0]

    def _ints(self, x, name, n):
        """A per-probe (or per-row) integer array, NumPy or torch -> int64 [n] on the shard's device."""
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        if t.numel() == 0:
            t = t.to(torch.int64)
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError('%s must be integers, got %s' % (name, t.dtype))
        if tuple(t.shape) != (n,):
            raise ValueError('%s must have shape [%d], got %s' % (name, n, tuple(t.shape)))
        return t.to(device=self.gallery._dev, dtype=torch.int64).contiguous()

    def _gather(self, local):
        """all_gather_into_tensor of one dense tensor per rank -> [R, *local.shape]."""
        out = torch.empty((self.world,) + tuple(local.shape), dtype=local.dtype, device=local.device)
        if local.numel():
            dist.all_gather_into_tensor(out.view(-1), local.contiguous().view(-1), group=self.group)
        return out

    @staticmethod
    def _back(was_np, *ts):
        return tuple(t.cpu().numpy() for t in ts) if was_np else ts

    def _tags(self, row_tags, probe_masks, b):
        """The watch-list pair of `topk` / `topk_ids` / `within` / `rank`: -> (this shard's row tags [len(shard)], the masks of ALL ranks' probes
        [R*b]) as int64 on the shard's device, or (None, None); exactly one given raises ValueError."""
        if row_tags is None and probe_masks is None:
            return None, None
        if row_tags is None or probe_masks is None:
            raise ValueError('row_tags and probe_masks go together: give both or neither')
        from .oneshot import _bit_sets
        dev = self.gallery._dev
        rt = _bit_sets(row_tags, 'row_tags', len(self.gallery), dev)
        return rt, self._gather(_bit_sets(probe_masks, 'probe_masks', b, dev, scalar=True)).view(-1)

    def topk(self, local_probes, k, distance_metric=1, row_tags=None, probe_masks=None):
        """oneshot.Gallery.topk over the whole sharded gallery: -> (idx [R*b, k] int64 global, dist [R*b, k] float32) for the
        probes of ALL ranks in rank order, identical on every rank and equal, bit for bit, to one Gallery holding every row.
        Every rank brings its own [b, d] probes (same b).  Exchange: the probes, then one gather of R records of
        R*b*k*12 bytes; merged on the device (merge_topk).
        `row_tags` [len(shard)] are THIS shard's tags in its local row order, as `row_labels` are; `probe_masks` [b] (or a
        Python int; None on every rank alike) belong to this rank's probes and are gathered with them (oneshot.Gallery.topk).
        The merge is unchanged: a row among the k nearest eligible rows of all shards is among those of its own shard."""
        if self._local():
            return self.gallery.topk(local_probes, k, distance_metric, row_tags, probe_masks)
        p, was_np, b = self._begin('topk', local_probes)
        rt, pm = self._tags(row_tags, probe_masks, b)
        probes = self.all_gather_embeddings(p)
        B = probes.shape[0]
        idx, d = self.gallery.topk(probes, k, distance_metric, rt, pm)
        gi, gd = _unpack(self._gather(_pack([idx, d])), [(torch.int64, (B, k)), (torch.float32, (B, k))])
        return self._back(was_np, *merge_topk(gi, gd))

    def topk_ids(self, local_probes, k, row_labels, distance_metric=1, exclude=None, row_tags=None, probe_masks=None):
        """oneshot.Gallery.topk_ids over the whole sharded gallery: -> (idx, dist, label), each [R*b, k], identical on every
        rank and equal to one Gallery holding every row.  `row_labels` [len(shard)] are THIS shard's labels in its local row
        order; `exclude` [b] (or None -- on every rank alike) belongs to this rank's probes and is gathered with them.
        Exchange: the probes, exclude, then one gather of R records of R*b*k*20 bytes (merge_topk_ids).
        `row_tags` (this shard's) and `probe_masks` (this rank's probes', gathered with them) as in `topk`."""
        if self._local():
            return self.gallery.topk_ids(local_probes, k, row_labels, distance_metric, exclude, row_tags, probe_masks)
        p, was_np, b = self._begin('topk_ids', local_probes)
        ex = None if exclude is None else self._gather(self._ints(exclude, 'exclude', b)).view(-1)
        rt, pm = self._tags(row_tags, probe_masks, b)
        probes = self.all_gather_embeddings(p)
        B = probes.shape[0]
        idx, d, lab = self.gallery.topk_ids(probes, k, self._ints(row_labels, 'row_labels', len(self.gallery)),
                                            distance_metric, ex, rt, pm)
        gi, gl, gd = _unpack(self._gather(_pack([idx, lab, d])),
                             [(torch.int64, (B, k)), (torch.int64, (B, k)), (torch.float32, (B, k))])
        return self._back(was_np, *merge_topk_ids(gi, gd, gl))

    def within(self, local_probes, tolerance, distance_metric=1, max_hits=64, row_tags=None, probe_masks=None):
        """oneshot.Gallery.within over the whole sharded gallery: -> (count [R*b] int64, idx [R*b, K] int64, dist [R*b, K]
        float32), K = max_hits, identical on every rank and equal to one Gallery holding every row: the counts are exact, the
        lists hold the K lowest global rows.  Exchange: the probes, then one gather of R records of R*b*(8 + 12 K) bytes.
        Every rank receives every shard's lists: R * R*b * max_hits * 12 bytes.  Above 2^30 bytes the call raises ValueError
        before it allocates anything -- lower max_hits (0 gives the counts alone), or bring fewer probes per step.
        `row_tags` [len(shard)] are THIS shard's tags in its local row order; `probe_masks` [b] (or a Python int; None on
        every rank alike) belong to this rank's probes and are gathered with them (oneshot.Gallery.within).  The merge is
        unchanged: counts over the eligible rows of disjoint shards add, and the K lowest eligible hits of all shards are
        among each shard's K lowest."""
        if self._local():
            return self.gallery.within(local_probes, tolerance, distance_metric, max_hits, row_tags, probe_masks)
        p, was_np, b = self._begin('within', local_probes)
        rt, pm = self._tags(row_tags, probe_masks, b)
        K = int(max_hits)
        need = within_gather_bytes(self.world, b, K)
        if need > WITHIN_GATHER_MAX:
            raise ValueError('ShardedGallery.within: the gathered lists would take %d bytes (%d ranks x %d probes x %d hits x '
                             '12) > 2^30: lower max_hits' % (need, self.world, self.world * b, K))
        probes = self.all_gather_embeddings(p)
        B = probes.shape[0]
        cnt, idx, d = self.gallery.within(probes, tolerance, distance_metric, K, rt, pm)
        gc, gi, gd = _unpack(self._gather(_pack([cnt, idx, d])),
                             [(torch.int64, (B,)), (torch.int64, (B, K)), (torch.float32, (B, K))])
        return self._back(was_np, *merge_within(gc, gi, gd))

    def rank(self, local_probes, mates, distance_metric=1, row_tags=None, probe_masks=None):
        """oneshot.Gallery.rank over the whole sharded gallery: -> (rank [R*b] int64, mate_dist [R*b] float32), identical on
        every rank and equal to one Gallery holding every row.  `mates` [b] are global indices (any shard's; -1 or an index
        no shard holds: unmated, rank -1).  Two result exchanges, because a shard cannot count against a mate it does not
        hold: the probes and mates; every shard's (owned, mate_dist) -- R records of R*b*12 bytes -- from which every rank
        takes the owner's distance; then every shard's count against that distance -- R records of R*b*8 bytes -- summed
        (merge_rank).
        `row_tags` (this shard's) and `probe_masks` (this rank's probes', gathered with them) as in `within`: the rank among
        the rows each probe is eligible for.  The merge is unchanged: the owning shard reports owned = 1 and a NaN distance
        for a mate the probe may not see (rank = the size of every shard, summed: len of the whole gallery), and counts over
        the eligible rows of disjoint shards add."""
        if self._local():
            return self.gallery.rank(local_probes, mates, distance_metric, row_tags, probe_masks)
        p, was_np, b = self._begin('rank', local_probes)
        rt, pm = self._tags(row_tags, probe_masks, b)
        m = self._gather(self._ints(mates, 'mates', b)).view(-1)
        probes = self.all_gather_embeddings(p)
        B = probes.shape[0]
        dev = probes.device
        md = torch.empty((B,), dtype=torch.float32, device=dev)
        own = torch.empty((B,), dtype=torch.int64, device=dev)
        self.gallery.mate_dist_into(probes, m, distance_metric, md, own, rt, pm)
        g_own, g_md = _unpack(self._gather(_pack([own, md])), [(torch.int64, (B,)), (torch.float32, (B,))])
        _, dm = merge_rank(torch.zeros_like(g_own), g_own, g_md)        # the owner's distance, on every rank
        cnt = torch.empty((B,), dtype=torch.int64, device=dev)
        self.gallery.rank_at_into(probes, m, dm, distance_metric, cnt, rt, pm)
        return self._back(was_np, *merge_rank(self._gather(cnt), g_own, g_md))

    def roc(self, local_probes, probe_labels, row_labels, thresholds, distance_metric=1, first_row=None):
        """oneshot.Gallery.roc over the whole sharded gallery and the probes of ALL ranks: -> (accept [T, 2] int64, totals [4]
        int64) on the device, identical on every rank and equal to one Gallery holding every row queried with all R*b probes.
        `probe_labels` and `first_row` [b] (or None -- on every rank alike) belong to this rank's probes, `row_labels`
        [len(shard)] to this shard's rows; `first_row` is a global row index.  `thresholds` must be EQUAL on all ranks: this is
        not checked, and unequal thresholds add counts that do not belong together.  Exchange: the probes, their labels and
        first rows, then one gather of R records of (2 T + 4) * 8 bytes; the counts of row shards add."""
        if self._local():
            return self.gallery.roc(local_probes, probe_labels, row_labels, thresholds, distance_metric, first_row)
        p, _, b = self._begin('roc', local_probes)
        pl = self._gather(self._ints(probe_labels, 'probe_labels', b)).view(-1)
        fr = None if first_row is None else self._gather(self._ints(first_row, 'first_row', b)).view(-1)
        probes = self.all_gather_embeddings(p)
        acc, tot = self.gallery.roc(probes, pl, self._ints(row_labels, 'row_labels', len(self.gallery)), thresholds,
                                    distance_metric, fr)
        T = acc.shape[0]
        s = self._gather(torch.cat([acc.reshape(-1), tot])).sum(0)
        return s[:2 * T].view(T, 2), s[2 * T:]
