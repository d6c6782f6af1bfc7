"""1:N gallery match ("one shot" identification) on the MI355X.

The reference's oneshot.py is an unfinished Omniglot stub with no distance code
(deep_insight_face/oneshot.py:8 "TODO: FIX THIS MODULE"); north_star houses the
pairwise cosine-distance gallery match under this module name.  Semantics: for every
probe row q, ``np.argmin(evaluation.utility.distance(q[None, :], gallery, metric))``
(evaluation/utility.py:52-66 broadcast over the gallery; first minimum wins).
"""
import ctypes
import os

import numpy as np
import torch

from . import _native as N


MAX_HITS = 8192   # DIF_WITHIN_MAX_HITS (include/dif.h): the longest list `within` returns per probe
TOPK_MAX = 128    # DIF_TOPK_MAX: the longest list `topk` returns per probe
ROC_MAX_THRESHOLDS = 1024   # DIF_ROC_MAX_THRESHOLDS: the most thresholds one `roc` call takes


def up32(thresholds):
    """float64 thresholds -> the float32 thresholds that compare the same way with a float32 distance: for a float32 d,
    ``d < t64`` (NumPy compares in double) holds exactly when ``d < up32(t64)``, the smallest float32 >= t64.  Rounding to
    nearest would move a threshold below a distance that equals the rounded value.  NaN stays NaN."""
    t64 = np.asarray(thresholds, dtype=np.float64)
    with np.errstate(over='ignore'):
        t32 = t64.astype(np.float32)
    low = t32.astype(np.float64) < t64
    return np.where(low, np.nextafter(t32, np.float32(np.inf)), t32).astype(np.float32)


def _bit_sets(x, name, n, dev, scalar=False):
    """`row_tags` / `probe_masks` of the tagged searches -> int64 [n] on `dev`, one 64-bit set per entry.  NumPy or torch
    integers of any width (a negative value has bit 63 set; NumPy uint64 is taken bit for bit); floats and bools are rejected,
    the shape must be [n].  With `scalar` a Python int stands for every entry: -2^63 .. 2^64 - 1, the same 64 bits."""
    if scalar and isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)):
        v = int(x)
        if not -(1 << 63) <= v < (1 << 64):
            raise ValueError('%s %d does not fit 64 bits' % (name, v))
        return torch.full((n,), v - (1 << 64) if v >= (1 << 63) else v, dtype=torch.int64, device=dev)
    if torch.is_tensor(x):
        t = x
    else:
        a = np.asarray(x)
        if a.size == 0 and a.dtype.kind == 'f':                 # np.asarray([]) is float64: an empty list holds no set
            a = a.astype(np.int64)
        if a.dtype.kind not in 'iu':
            raise ValueError('%s must be integers, got %s' % (name, a.dtype))
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.int64).copy() if a.dtype == np.uint64 else a.astype(np.int64))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError('%s must be integers, got %s' % (name, t.dtype))
    if tuple(t.shape) != (n,):
        raise ValueError('%s must have shape [%d], got %s' % (name, n, tuple(t.shape)))
    return t.to(device=dev, dtype=torch.int64).contiguous()


def _tag_pair(row_tags, probe_masks, G, B, dev):
    """Both None -> (None, None); exactly one given -> ValueError; else the two int64 device tensors."""
    if row_tags is None and probe_masks is None:
        return None, None
    if row_tags is None or probe_masks is None:
        raise ValueError('row_tags and probe_masks go together: give both or neither')
    return _bit_sets(row_tags, 'row_tags', G, dev), _bit_sets(probe_masks, 'probe_masks', B, dev, scalar=True)


class Gallery:
    """Device-resident gallery of enrolled embeddings, [G, d] float32.

    One instance per process/GPU.  With ``index_base`` the rows are a shard of a larger
    gallery (see deep_insight_face.parallel.ShardedGallery)."""

    def __init__(self, embeddings=None, emd_size=None, index_base=0):
        self._h = ctypes.c_void_p()
        self._dev = N.require_device()
        if embeddings is not None and emd_size is None:
            emd_size = int(embeddings.shape[1])
        if emd_size is None:
            raise ValueError('Gallery needs embeddings or emd_size')
        N.check(N.lib.dif_gallery_create(ctypes.byref(self._h), int(emd_size)), ValueError)
        self.emd_size = int(emd_size)
        # development hook (A/B runs of bench.py and the tools, like DIF_OPTIONS for the networks): "key=value,..." applied to
        # every gallery of the process at creation
        for kv in os.environ.get('DIF_GALLERY_OPTIONS', '').split(','):
            if '=' in kv:
                self.set_option(kv.split('=')[0].strip(), int(kv.split('=')[1]))
        if embeddings is not None:
            self.set(embeddings, index_base)

    def set(self, embeddings, index_base=0):
        g, _ = N.to_device_f32(embeddings, self._dev)
        if g.dim() != 2 or g.shape[1] != self.emd_size:
            raise ValueError('gallery must be [G, %d], got %s' % (self.emd_size, tuple(g.shape)))
        N.check(N.lib.dif_gallery_set(self._h, N.ptr(g), g.shape[0], int(index_base), N.stream_ptr()))
        torch.cuda.current_stream().synchronize()   # g may be a temporary: the copy must have landed

    def update(self, embeddings, first_row=None):
        """Enrol incrementally: overwrite rows [first_row, first_row + k) or, with first_row None (or == len(self)),
        append -- O(k) on the device (`set` is a pass over the whole gallery).  Appending beyond the capacity grows it
        by half (one reallocation + copy)."""
        g, _ = N.to_device_f32(embeddings, self._dev)
        if g.dim() == 1:
            g = g[None, :]
        if g.dim() != 2 or g.shape[1] != self.emd_size:
            raise ValueError('rows must be [k, %d], got %s' % (self.emd_size, tuple(g.shape)))
        n = len(self)
        first_row = n if first_row is None else int(first_row)
        if first_row < 0 or first_row > n:
            raise ValueError('first_row %d outside [0, %d]' % (first_row, n))
        need = first_row + g.shape[0]
        if need > self.capacity:
            self.reserve(max(need, self.capacity + self.capacity // 2))
        N.check(N.lib.dif_gallery_update(self._h, N.ptr(g), g.shape[0], first_row, N.stream_ptr()), ValueError)
        torch.cuda.current_stream().synchronize()   # g may be a temporary: the copy must have landed

    def remove(self, rows):
        """Un-enrol: take the rows named in `rows` (global indices, any integer dtype, shape [k], any order; duplicates
        collapse as in np.delete) out of the gallery -- O(k) on the device, the capacity stays.
        -> (moved_from[m], moved_to[m]) int64, m <= k; NumPy in -> NumPy out, tensor in -> tensors on the device.

        Swap-remove: with new_n = len(self) - k, rows below new_n that are not named keep their indices; the surviving rows of
        the tail [new_n, len) fill the holes the named rows leave below new_n, the i-th survivor the i-th hole, both in
        ascending order: row moved_from[i] is now row moved_to[i] (fix the name table with it).  Afterwards `match`, `within`
        and `rank` answer exactly as a gallery `set` with the resulting rows; the removed rows' slots are zeroed on the device.
        An index outside the gallery raises ValueError and leaves the gallery as it was."""
        was_np = not torch.is_tensor(rows)
        if was_np:
            r = np.asarray(rows)
            if r.size == 0 and r.dtype.kind == 'f':          # np.asarray([]) is float64: an empty list names no row
                r = r.astype(np.int64)
            if r.dtype.kind not in 'iu':
                raise ValueError('rows must be integers, got %s' % r.dtype)
            if r.dtype.kind == 'u' and r.size and int(r.max()) > np.iinfo(np.int64).max:
                raise ValueError('rows must fit int64')
            if r.ndim != 1:
                raise ValueError('rows must have shape [k], got %s' % (r.shape,))
            r = torch.from_numpy(np.ascontiguousarray(r.astype(np.int64)))
        else:
            r = rows
            if r.dtype.is_floating_point or r.dtype.is_complex or r.dtype == torch.bool:
                raise ValueError('rows must be integers, got %s' % r.dtype)
            if r.dim() != 1:
                raise ValueError('rows must have shape [k], got %s' % (tuple(r.shape),))
        r = torch.unique(r.to(device=self._dev, dtype=torch.int64))   # sorted, distinct: what dif_gallery_remove takes
        k = r.shape[0]
        moved_from = torch.empty((k,), dtype=torch.int64, device=self._dev)
        moved_to = torch.empty((k,), dtype=torch.int64, device=self._dev)
        m = ctypes.c_int64(0)
        if k:
            N.check(N.lib.dif_gallery_remove(self._h, N.ptr(r), k, N.ptr(moved_from), N.ptr(moved_to), ctypes.byref(m),
                                             N.stream_ptr()), ValueError)
        moved_from, moved_to = moved_from[:m.value], moved_to[:m.value]
        if was_np:
            moved_from, moved_to = moved_from.cpu().numpy(), moved_to.cpu().numpy()
        return moved_from, moved_to

    def reserve(self, capacity):
        N.check(N.lib.dif_gallery_reserve(self._h, int(capacity), N.stream_ptr()))

    @property
    def capacity(self):
        return int(N.lib.dif_gallery_capacity(self._h))

    def __len__(self):
        return int(N.lib.dif_gallery_size(self._h))

    def set_option(self, key, value):
        """'filter': 2 (default) runs the MFMA filter stage on operands rounded to bf16 once, 1 on two-term split-bf16
        operands, 0 in float32: the same results (the filter only proposes candidates), different speed and memory.
        'frag': layout of the one-term filter's copy -- 1 (default) MFMA-fragment order from 2^18 rows up (embedding sizes that
        are multiples of 128 up to 512), 2 always, 0 row-major; same results (include/dif.h).
        'clamp_nan': 1 reports distance 0 / 1 where the reference's distance is NaN (a similarity rounded
        beyond +-1); the default 0 reports NaN like the reference.  The arg-min is unaffected.
        'topk_seed': tiles of 128 rows the seed stage of `topk` evaluates per probe -- 0 (default): k of them; same results
        for every value (include/dif.h).  `topk_ids` starts its growing seed there.
        'cluster_round': probes per round of `cluster` and `dbscan`, a multiple of 128 -- 0 (default): a sixteenth of the rows, at least 2048; same
        results for every value (include/dif.h).
        'roc_round': probes per round of `roc`, a multiple of 128 -- 0 (default): what its workspace allows; same results for
        every value (include/dif.h).
        'within_round': probes per round of `within`, `rank` and `rank_at`, plain and tagged, a multiple of 128 -- 0 (default): what the census
        workspace allows; same results for every value (include/dif.h).
        'topk_round': probes per round of `topk` and `topk_ids`, plain and tagged, a multiple of 128 -- 0 (default): what the
        tile-word workspace allows; same results for every value (include/dif.h).
        'roc_blocks': most blocks of `roc`'s resolve stage -- 0 (default): 2048; same results for every value (include/dif.h)."""
        N.check(N.lib.dif_gallery_set_option(self._h, key.encode(), int(value)), ValueError)

    def stat(self, key):
        """'split_copy': 1 when the filter's bf16 copy of the rows exists (+ 50 % device memory for the one-term
        filter, + 100 % for the two-term one; when it cannot be allocated the float32 filter serves);
        'filter_terms': bf16 terms per operand the next match's filter runs on (0: float32 rows);
        'frag_copy': 1 when the one-term copy is held in MFMA-fragment order (option 'frag': match_g1_kernel serves);
        'row_bytes': device bytes per row;
        'exact_probes': probes the last match sent to the exact whole-gallery search (synchronises);
        'roc_resolved': pairs the last `roc` evaluated one by one, too close to a threshold to call (synchronises);
        'topk_ids_tiles': (probe, 128-row tile) pairs the last `topk_ids` evaluated row by row (synchronises);
        'topk_tagged_tiles': the same for the last `topk` or `topk_ids` given `row_tags` and `probe_masks` -- a tile without
        a row eligible for the probe is never among them (synchronises);
        'within_tagged_tiles': the same for the last `within`, `rank` or `rank_at_into` given `row_tags` and `probe_masks`
        -- a tile without an eligible row that could be a hit (resp. closer or tied) is never among them (synchronises)."""
        v = ctypes.c_int64(0)
        N.check(N.lib.dif_gallery_get_stat(self._h, key.encode(), ctypes.byref(v), N.stream_ptr()), ValueError)
        return int(v.value)

    def _tags_into(self, fn, row_tags, probe_masks, B):
        """The checks of the `_into` forms of the tagged range search and rank: both None -> False; else both dense int64
        CUDA tensors, [len(self)] and [B] -> True."""
        if (row_tags is None) != (probe_masks is None):
            raise ValueError('row_tags and probe_masks go together: give both or neither')
        if row_tags is None:
            return False
        for name, t, shape in (('row_tags', row_tags, (len(self),)), ('probe_masks', probe_masks, (B,))):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or t.device != self._dev or not t.is_contiguous():
                raise ValueError('%s: %s must be a contiguous %s tensor on %s' % (fn, name, torch.int64, self._dev))
            if tuple(t.shape) != shape:
                raise ValueError('%s: %s must have shape %s, got %s' % (fn, name, list(shape), tuple(t.shape)))
        return True

    def match_into(self, probes, distance_metric, idx, dist, key=None):
        """Allocation-free form for a serving loop: `probes` [B, d] float32 CUDA, results written into the
        caller's CUDA tensors idx [B] int64, dist [B] float32 and (optional) key [B] float32 -- which may be
        slices of one packed buffer (see ShardedGallery)."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        # the library reads `probes` as dense float32 [B, emd_size] and writes B results: anything else would be
        # read out of bounds or reinterpreted silently, so it is refused here (no conversion: this form allocates nothing)
        if not torch.is_tensor(probes) or probes.dim() != 2 or probes.shape[1] != self.emd_size:
            raise ValueError('probes must be a [B, %d] tensor, got %s' % (
                self.emd_size, tuple(probes.shape) if hasattr(probes, 'shape') else type(probes).__name__))
        B = probes.shape[0]
        for name, t, dt in (('probes', probes, torch.float32), ('idx', idx, torch.int64), ('dist', dist, torch.float32),
                            ('key', key, torch.float32)):
            if t is None and name == 'key':
                continue
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self._dev or not t.is_contiguous():
                raise ValueError('match_into: %s must be a contiguous %s tensor on %s' % (name, dt, self._dev))
            if name != 'probes' and (t.dim() != 1 or t.shape[0] != B):
                raise ValueError('match_into: %s must have shape [%d], got %s' % (name, B, tuple(t.shape)))
        if B:
            if len(self) == 0:
                raise ValueError('attempt to get argmin of an empty sequence')
            N.check(N.lib.dif_match(self._h, N.ptr(probes), B, distance_metric, N.ptr(idx), N.ptr(dist),
                                    N.ptr(key) if key is not None else None, N.stream_ptr()))

    def match(self, probes, distance_metric=1, return_key=False):
        """-> (idx[B] int64, dist[B] float32) [, key[B]]; NumPy in -> NumPy out."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        p, was_np = N.to_device_f32(probes, self._dev)
        if p.dim() == 1:
            p = p[None, :]
        if p.dim() != 2 or p.shape[1] != self.emd_size:
            raise ValueError('probes must be [B, %d], got %s' % (self.emd_size, tuple(p.shape)))
        B = p.shape[0]
        idx = torch.empty((B,), dtype=torch.int64, device=self._dev)
        dist = torch.empty((B,), dtype=torch.float32, device=self._dev)
        key = torch.empty((B,), dtype=torch.float32, device=self._dev)
        if B:
            if len(self) == 0:
                raise ValueError('attempt to get argmin of an empty sequence')   # what np.argmin raises
            N.check(N.lib.dif_match(self._h, N.ptr(p), B, distance_metric, N.ptr(idx), N.ptr(dist),
                                    N.ptr(key), N.stream_ptr()))
        if was_np:
            idx, dist, key = idx.cpu().numpy(), dist.cpu().numpy(), key.cpu().numpy()
        return (idx, dist, key) if return_key else (idx, dist)

    def within_into(self, probes, tolerance, distance_metric, count, idx, dist, row_tags=None, probe_masks=None):
        """Allocation-free form of `within`: `probes` [B, d] float32 CUDA, results written into the caller's CUDA tensors
        count [B] int64, idx [B, K] int64 and dist [B, K] float32 (K = max_hits, taken from idx; K may be 0).  `row_tags`
        [len(self)] and `probe_masks` [B], both int64 CUDA or both None, restrict every probe to its eligible rows (`within`)."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        tolerance = float(tolerance)
        if tolerance != tolerance:
            raise ValueError('within: the tolerance is NaN')
        if not torch.is_tensor(probes) or probes.dim() != 2 or probes.shape[1] != self.emd_size:
            raise ValueError('probes must be a [B, %d] tensor, got %s' % (
                self.emd_size, tuple(probes.shape) if hasattr(probes, 'shape') else type(probes).__name__))
        B = probes.shape[0]
        for name, t, dt in (('probes', probes, torch.float32), ('count', count, torch.int64), ('idx', idx, torch.int64),
                            ('dist', dist, torch.float32)):
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self._dev or not t.is_contiguous():
                raise ValueError('within_into: %s must be a contiguous %s tensor on %s' % (name, dt, self._dev))
        if count.dim() != 1 or count.shape[0] != B:
            raise ValueError('within_into: count must have shape [%d], got %s' % (B, tuple(count.shape)))
        if idx.dim() != 2 or idx.shape[0] != B or idx.shape[1] > MAX_HITS:
            raise ValueError('within_into: idx must have shape [%d, K] with K <= %d, got %s' % (B, MAX_HITS, tuple(idx.shape)))
        if tuple(dist.shape) != tuple(idx.shape):
            raise ValueError('within_into: dist must have shape %s, got %s' % (tuple(idx.shape), tuple(dist.shape)))
        K = idx.shape[1]
        if self._tags_into('within_into', row_tags, probe_masks, B):
            if B:
                N.check(N.lib.dif_match_within_tagged(self._h, N.ptr(probes), B, distance_metric, tolerance, K,
                                                      N.ptr(row_tags) if len(self) else None, N.ptr(probe_masks), N.ptr(count),
                                                      N.ptr(idx) if K else None, N.ptr(dist) if K else None, N.stream_ptr()))
            return
        if B:
            N.check(N.lib.dif_match_within(self._h, N.ptr(probes), B, distance_metric, tolerance, K, N.ptr(count),
                                           N.ptr(idx) if K else None, N.ptr(dist) if K else None, N.stream_ptr()))

    def within(self, probes, tolerance, distance_metric=1, max_hits=64, row_tags=None, probe_masks=None):
        """Range search: every enrolled row whose distance to a probe is <= `tolerance`, exact.
        -> (count[B] int64, idx[B, K] int64, dist[B, K] float32) with K = max_hits; NumPy in -> NumPy out.

        Per probe q: ``d = evaluation.utility.distance(q[None, :], gallery, metric)``, ``hits = np.flatnonzero(d <= tolerance)``;
        count = len(hits) (exact, however large), idx = the K lowest hit rows in ascending order (+ index_base), dist their
        distances; unused slots hold idx -1 and dist NaN.  max_hits=0 returns the counts alone ([B, 0] lists).
        The tolerance is in the units of utility.distance: metric 0 is the SQUARED L2 distance, metric 1 arccos(sim)/pi.
        A NaN distance is never a hit: with the default 'clamp_nan' 0 a similarity that rounding pushes beyond +-1 is NaN in
        the reference -- a probe identical to an enrolled row can miss it this way; set_option('clamp_nan', 1) compares
        the clamped distance (0 or 1) instead.  An empty gallery gives counts of 0.

        Watch-lists: `row_tags` [len(self)] and `probe_masks` [B] (a Python int stands for every probe) are `topk`'s -- row r
        is eligible for probe b iff ``(row_tags[r] & probe_masks[b]) != 0`` on the raw 64 bits -- and the answer is the one
        above with ``d[~eligible[b]] = NaN``: an ineligible row is never counted and never listed, however many of them
        precede the first permitted hit; a tag of 0 is never eligible, a mask of 0 gives count 0 and all padding.  Give both
        or neither (ValueError otherwise).  `stat('within_tagged_tiles')` tells how many tiles the call evaluated row by row."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        max_hits = int(max_hits)
        if max_hits < 0 or max_hits > MAX_HITS:
            raise ValueError('max_hits %d outside [0, %d]' % (max_hits, MAX_HITS))
        p, was_np = N.to_device_f32(probes, self._dev)
        if p.dim() == 1:
            p = p[None, :]
        if p.dim() != 2 or p.shape[1] != self.emd_size:
            raise ValueError('probes must be [B, %d], got %s' % (self.emd_size, tuple(p.shape)))
        B = p.shape[0]
        count = torch.empty((B,), dtype=torch.int64, device=self._dev)
        idx = torch.empty((B, max_hits), dtype=torch.int64, device=self._dev)
        dist = torch.empty((B, max_hits), dtype=torch.float32, device=self._dev)
        rt, pm = _tag_pair(row_tags, probe_masks, len(self), B, self._dev)
        self.within_into(p, tolerance, distance_metric, count, idx, dist, rt, pm)
        if was_np:
            count, idx, dist = count.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
        return count, idx, dist

    def rank_into(self, probes, mates, distance_metric, rank, mate_dist, row_tags=None, probe_masks=None):
        """Allocation-free form of `rank`: `probes` [B, d] float32 and `mates` [B] int64 CUDA, results written into the
        caller's CUDA tensors rank [B] int64 and mate_dist [B] float32.  `row_tags` [len(self)] and `probe_masks` [B], both
        int64 CUDA or both None: the rank among the rows each probe is eligible for (`rank`)."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        if not torch.is_tensor(probes) or probes.dim() != 2 or probes.shape[1] != self.emd_size:
            raise ValueError('probes must be a [B, %d] tensor, got %s' % (
                self.emd_size, tuple(probes.shape) if hasattr(probes, 'shape') else type(probes).__name__))
        B = probes.shape[0]
        for name, t, dt in (('probes', probes, torch.float32), ('mates', mates, torch.int64), ('rank', rank, torch.int64),
                            ('mate_dist', mate_dist, torch.float32)):
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self._dev or not t.is_contiguous():
                raise ValueError('rank_into: %s must be a contiguous %s tensor on %s' % (name, dt, self._dev))
            if name != 'probes' and (t.dim() != 1 or t.shape[0] != B):
                raise ValueError('rank_into: %s must have shape [%d], got %s' % (name, B, tuple(t.shape)))
        if self._tags_into('rank_into', row_tags, probe_masks, B):
            if B:
                N.check(N.lib.dif_match_rank_tagged(self._h, N.ptr(probes), B, distance_metric, N.ptr(mates),
                                                    N.ptr(row_tags) if len(self) else None, N.ptr(probe_masks), N.ptr(rank),
                                                    N.ptr(mate_dist), N.stream_ptr()))
            return
        if B:
            N.check(N.lib.dif_match_rank(self._h, N.ptr(probes), B, distance_metric, N.ptr(mates), N.ptr(rank),
                                         N.ptr(mate_dist), N.stream_ptr()))

    def rank(self, probes, mates, distance_metric=1, row_tags=None, probe_masks=None):
        """Rank of the mate: where row `mates[b]` (global index, any integer dtype, shape [B]) ranks among ALL enrolled rows
        by distance to probe b, exact.  -> (rank[B] int64, mate_dist[B] float32); NumPy in -> NumPy out.

        Per probe q: ``d = evaluation.utility.distance(q[None, :], gallery, metric)``, ``dm = d[m - index_base]``,
        ``rank = count(d < dm) + count(d[:m - index_base] == dm)`` -- 0-based, the mate's position in
        ``np.argsort(d, kind='stable')`` when no distance is NaN; ``mate_dist = dm``.  A NaN distance is never closer.
        A mate of -1 (or any index outside the gallery) marks an unmated probe: rank -1, mate_dist NaN.  A mate whose own
        distance is NaN gets rank len(self), a miss at every k.  Without NaNs rank == 0 exactly when `match` returns the mate.
        Rows of the mate's identity count like any other row.

        Watch-lists: with `row_tags` [len(self)] and `probe_masks` [B] (as in `topk` and `within`; a Python int stands for
        every probe) the rank is the one among the rows the probe is eligible for -- the formula above with
        ``d[~eligible[b]] = NaN``: ineligible rows are never closer and never tie.  A mate the probe is NOT eligible for is a
        mate whose distance is NaN: rank len(self), mate_dist NaN -- distinct from an unmated probe (rank -1).  Give both or
        neither (ValueError otherwise)."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        p, was_np = N.to_device_f32(probes, self._dev)
        if p.dim() == 1:
            p = p[None, :]
        if p.dim() != 2 or p.shape[1] != self.emd_size:
            raise ValueError('probes must be [B, %d], got %s' % (self.emd_size, tuple(p.shape)))
        B = p.shape[0]
        if torch.is_tensor(mates):
            m = mates
            if m.dtype.is_floating_point or m.dtype.is_complex or m.dtype == torch.bool:
                raise ValueError('mates must be integers, got %s' % m.dtype)
        else:
            m = np.asarray(mates)
            if m.size == 0 and m.dtype.kind == 'f':          # np.asarray([]) is float64: an empty list names no row
                m = m.astype(np.int64)
            if m.dtype.kind not in 'iu':
                raise ValueError('mates must be integers, got %s' % m.dtype)
            if m.dtype.kind == 'u' and m.size and int(m.max()) > np.iinfo(np.int64).max:
                raise ValueError('mates must fit int64')
            m = torch.from_numpy(np.ascontiguousarray(m.astype(np.int64)))
        if tuple(m.shape) != (B,):
            raise ValueError('mates must have shape [%d], got %s' % (B, tuple(m.shape)))
        m = m.to(device=self._dev, dtype=torch.int64).contiguous()
        rank = torch.empty((B,), dtype=torch.int64, device=self._dev)
        mate_dist = torch.empty((B,), dtype=torch.float32, device=self._dev)
        rt, pm = _tag_pair(row_tags, probe_masks, len(self), B, self._dev)
        self.rank_into(p, m, distance_metric, rank, mate_dist, rt, pm)
        if was_np:
            rank, mate_dist = rank.cpu().numpy(), mate_dist.cpu().numpy()
        return rank, mate_dist

    def _rank_args(self, fn, probes, arrays):
        """The checks of the two shard-local rank forms: dense CUDA tensors of the library's own dtypes, [B] each."""
        if not torch.is_tensor(probes) or probes.dim() != 2 or probes.shape[1] != self.emd_size:
            raise ValueError('probes must be a [B, %d] tensor, got %s' % (
                self.emd_size, tuple(probes.shape) if hasattr(probes, 'shape') else type(probes).__name__))
        B = probes.shape[0]
        for name, t, dt in (('probes', probes, torch.float32),) + tuple(arrays):
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self._dev or not t.is_contiguous():
                raise ValueError('%s: %s must be a contiguous %s tensor on %s' % (fn, name, dt, self._dev))
            if name != 'probes' and (t.dim() != 1 or t.shape[0] != B):
                raise ValueError('%s: %s must have shape [%d], got %s' % (fn, name, B, tuple(t.shape)))
        return B

    def mate_dist_into(self, probes, mates, distance_metric, mate_dist, owned, row_tags=None, probe_masks=None):
        """The first shard-local half of a sharded `rank` (parallel.ShardedGallery.rank): for `probes` [B, d] float32 and
        `mates` [B] int64 (global indices) CUDA, writes mate_dist [B] float32 -- the distance to the mate where THIS gallery
        holds it, NaN where it does not -- and owned [B] int64 (1 / 0).  O(B d): no pass over the gallery.
        With `row_tags` [len(self)] and `probe_masks` [B] (int64 CUDA, both or neither) a mate this gallery holds but the
        probe is not eligible for is owned (1) with the distance NaN."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        B = self._rank_args('mate_dist_into', probes, (('mates', mates, torch.int64), ('mate_dist', mate_dist, torch.float32),
                                                       ('owned', owned, torch.int64)))
        if self._tags_into('mate_dist_into', row_tags, probe_masks, B):
            if B:
                N.check(N.lib.dif_match_mate_dist_tagged(self._h, N.ptr(probes), B, distance_metric, N.ptr(mates),
                                                         N.ptr(row_tags) if len(self) else None, N.ptr(probe_masks),
                                                         N.ptr(mate_dist), N.ptr(owned), N.stream_ptr()))
            return
        if B:
            N.check(N.lib.dif_match_mate_dist(self._h, N.ptr(probes), B, distance_metric, N.ptr(mates), N.ptr(mate_dist),
                                              N.ptr(owned), N.stream_ptr()))

    def rank_at_into(self, probes, mates, mate_dist, distance_metric, count, row_tags=None, probe_masks=None):
        """The second half: this gallery's share of the rank of a mate it need not hold.  `mate_dist` [B] float32 is the
        mate's distance dm, from whichever shard owns it; count [B] int64 receives
        ``count(d < dm) + count((d == dm) & (index_base + row < mates))`` over this gallery's rows (NaN is never closer;
        dm NaN gives len(self)).  The counts of disjoint shards add up to `rank` over all their rows.
        With `row_tags` [len(self)] and `probe_masks` [B] (int64 CUDA, both or neither) only the rows the probe is eligible
        for are counted (dm NaN still gives len(self))."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        B = self._rank_args('rank_at_into', probes, (('mates', mates, torch.int64), ('mate_dist', mate_dist, torch.float32),
                                                     ('count', count, torch.int64)))
        if self._tags_into('rank_at_into', row_tags, probe_masks, B):
            if B:
                N.check(N.lib.dif_match_rank_at_tagged(self._h, N.ptr(probes), B, distance_metric, N.ptr(mates), N.ptr(mate_dist),
                                                       N.ptr(row_tags) if len(self) else None, N.ptr(probe_masks), N.ptr(count),
                                                       N.stream_ptr()))
            return
        if B:
            N.check(N.lib.dif_match_rank_at(self._h, N.ptr(probes), B, distance_metric, N.ptr(mates), N.ptr(mate_dist),
                                            N.ptr(count), N.stream_ptr()))

    def topk_into(self, probes, k, distance_metric, idx, dist, row_tags=None, probe_masks=None):
        """Allocation-free form of `topk`: `probes` [B, d] float32 CUDA, results written into the caller's CUDA tensors
        idx [B, k] int64 and dist [B, k] float32.  `row_tags` [len(self)] and `probe_masks` [B], both int64 CUDA or both
        None, restrict every probe to its eligible rows (`topk`)."""
        if (row_tags is None) != (probe_masks is None):
            raise ValueError('row_tags and probe_masks go together: give both or neither')
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        k = int(k)
        if k < 1 or k > TOPK_MAX:
            raise ValueError('k %d outside [1, %d]' % (k, TOPK_MAX))
        if not torch.is_tensor(probes) or probes.dim() != 2 or probes.shape[1] != self.emd_size:
            raise ValueError('probes must be a [B, %d] tensor, got %s' % (
                self.emd_size, tuple(probes.shape) if hasattr(probes, 'shape') else type(probes).__name__))
        B = probes.shape[0]
        for name, t, dt in (('probes', probes, torch.float32), ('idx', idx, torch.int64), ('dist', dist, torch.float32)):
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self._dev or not t.is_contiguous():
                raise ValueError('topk_into: %s must be a contiguous %s tensor on %s' % (name, dt, self._dev))
            if name != 'probes' and tuple(t.shape) != (B, k):
                raise ValueError('topk_into: %s must have shape [%d, %d], got %s' % (name, B, k, tuple(t.shape)))
        if row_tags is not None:
            G = len(self)
            for name, t, shape in (('row_tags', row_tags, (G,)), ('probe_masks', probe_masks, (B,))):
                if not torch.is_tensor(t) or t.dtype != torch.int64 or t.device != self._dev or not t.is_contiguous():
                    raise ValueError('topk_into: %s must be a contiguous %s tensor on %s' % (name, torch.int64, self._dev))
                if tuple(t.shape) != shape:
                    raise ValueError('topk_into: %s must have shape %s, got %s' % (name, list(shape), tuple(t.shape)))
            if B:
                N.check(N.lib.dif_match_topk_tagged(self._h, N.ptr(probes), B, distance_metric, k, N.ptr(row_tags) if G else None,
                                                    N.ptr(probe_masks), N.ptr(idx), N.ptr(dist), N.stream_ptr()))
            return
        if B:
            N.check(N.lib.dif_match_topk(self._h, N.ptr(probes), B, distance_metric, k, N.ptr(idx), N.ptr(dist),
                                         N.stream_ptr()))

    def topk(self, probes, k, distance_metric=1, row_tags=None, probe_masks=None):
        """The k nearest enrolled rows of each probe, in order, exact.  -> (idx[B, k] int64, dist[B, k] float32); NumPy in ->
        NumPy out.  1 <= k <= 128.

        Per probe q: ``d = evaluation.utility.distance(q[None, :], gallery, metric)``, ``order = np.argsort(d, kind='stable')``
        (ascending distance, exact ties to the lower row), ``keep = order[~np.isnan(d[order])][:k]``; idx = keep + index_base,
        dist = d[keep].  A NaN distance is never listed (set_option('clamp_nan', 1) orders and reports the clamped 0 / 1
        instead); k above len(self), or fewer than k rows with a distance that is not NaN, pads with idx -1 and dist NaN, and
        an empty gallery gives all padding.  `rank(q, idx[:, j])` returns `(j, dist[:, j])`; where no distance is NaN idx[:, 0]
        is `match`'s row.

        Watch-lists: `row_tags` [len(self)] holds one 64-bit set per enrolled row in the gallery's row order (any integer
        dtype, NumPy uint64 taken bit for bit; the gallery stores none -- keep it as `row_labels` is kept, permuted by the moves
        `remove` reports) and `probe_masks` [B] one per probe (a Python int stands for every probe).  Row r is eligible for
        probe b iff ``(row_tags[r] & probe_masks[b]) != 0`` on the raw 64 bits, and the list is the one above with
        ``d[~eligible[b]] = NaN``: an ineligible row is never listed, however near; a tag of 0 is never eligible, a mask of 0
        gives all padding.  Give both or neither (ValueError otherwise).  `stat('topk_tagged_tiles')` tells how many tiles
        the call evaluated row by row; a tile without an eligible row is never one."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        k = int(k)
        if k < 1 or k > TOPK_MAX:
            raise ValueError('k %d outside [1, %d]' % (k, TOPK_MAX))
        p, was_np = N.to_device_f32(probes, self._dev)
        if p.dim() == 1:
            p = p[None, :]
        if p.dim() != 2 or p.shape[1] != self.emd_size:
            raise ValueError('probes must be [B, %d], got %s' % (self.emd_size, tuple(p.shape)))
        B = p.shape[0]
        rt, pm = _tag_pair(row_tags, probe_masks, len(self), B, self._dev)
        idx = torch.empty((B, k), dtype=torch.int64, device=self._dev)
        dist = torch.empty((B, k), dtype=torch.float32, device=self._dev)
        self.topk_into(p, k, distance_metric, idx, dist, rt, pm)
        if was_np:
            idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        return idx, dist

    def topk_ids_into(self, probes, k, distance_metric, row_labels, exclude, idx, dist, label=None, row_tags=None,
                      probe_masks=None):
        """Allocation-free form of `topk_ids`: `probes` [B, d] float32, `row_labels` [len(self)] int64 and `exclude` [B] int64
        (or None) CUDA, results written into the caller's CUDA tensors idx [B, k] int64, dist [B, k] float32 and (optional)
        label [B, k] int64.  `row_tags` [len(self)] and `probe_masks` [B], both int64 CUDA or both None, as in `topk_into`."""
        if (row_tags is None) != (probe_masks is None):
            raise ValueError('row_tags and probe_masks go together: give both or neither')
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        k = int(k)
        if k < 1 or k > TOPK_MAX:
            raise ValueError('k %d outside [1, %d]' % (k, TOPK_MAX))
        if not torch.is_tensor(probes) or probes.dim() != 2 or probes.shape[1] != self.emd_size:
            raise ValueError('probes must be a [B, %d] tensor, got %s' % (
                self.emd_size, tuple(probes.shape) if hasattr(probes, 'shape') else type(probes).__name__))
        B, G = probes.shape[0], len(self)
        for name, t, dt, shape in (('probes', probes, torch.float32, None), ('row_labels', row_labels, torch.int64, (G,)),
                                   ('exclude', exclude, torch.int64, (B,)), ('idx', idx, torch.int64, (B, k)),
                                   ('dist', dist, torch.float32, (B, k)), ('label', label, torch.int64, (B, k)),
                                   ('row_tags', row_tags, torch.int64, (G,)), ('probe_masks', probe_masks, torch.int64, (B,))):
            if t is None and name in ('exclude', 'label', 'row_tags', 'probe_masks'):
                continue
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self._dev or not t.is_contiguous():
                raise ValueError('topk_ids_into: %s must be a contiguous %s tensor on %s' % (name, dt, self._dev))
            if shape is not None and tuple(t.shape) != shape:
                raise ValueError('topk_ids_into: %s must have shape %s, got %s' % (name, list(shape), tuple(t.shape)))
        if B and row_tags is not None:
            N.check(N.lib.dif_match_topk_ids_tagged(
                self._h, N.ptr(probes), B, distance_metric, k, N.ptr(row_labels) if G else None,
                N.ptr(exclude) if exclude is not None else None, N.ptr(row_tags) if G else None, N.ptr(probe_masks),
                N.ptr(idx), N.ptr(dist), N.ptr(label) if label is not None else None, N.stream_ptr()))
        elif B:
            N.check(N.lib.dif_match_topk_ids(self._h, N.ptr(probes), B, distance_metric, k, N.ptr(row_labels) if G else None,
                                             N.ptr(exclude) if exclude is not None else None, N.ptr(idx), N.ptr(dist),
                                             N.ptr(label) if label is not None else None, N.stream_ptr()))

    def topk_ids(self, probes, k, row_labels, distance_metric=1, exclude=None, row_tags=None, probe_masks=None):
        """The k nearest distinct IDENTITIES of each probe, each with its best row, in order, exact.
        -> (idx[B, k] int64, dist[B, k] float32, label[B, k] int64); NumPy in -> NumPy out.  1 <= k <= 128.

        `row_labels` [len(self)] holds the identity of every enrolled row in the gallery's row order (any integer dtype; the
        gallery stores none; a negative label takes the row out, as in `roc`); `exclude` [B] (optional) names one identity
        per probe to leave out, a negative entry none.  Per probe q: ``d = evaluation.utility.distance(q[None, :], gallery,
        metric)``, the rows with a NaN distance, a negative label or the excluded label dropped, the rest in the order of
        ``np.argsort(d, kind='stable')``; of every identity only its first -- nearest, on exact ties lowest -- row stays, and
        the first k of those are listed: idx = row + index_base, dist = d[row], label = row_labels[row].  Fewer than k
        identities pad with idx -1, dist NaN and label -1.  Distances, units and 'clamp_nan' are `topk`'s.

        With ``exclude`` the probe's own identity the list holds the k nearest OTHER identities (k = 1: the hardest negative).
        With all-distinct labels idx and dist are `topk`'s bit for bit; with one label the list has one entry, `match`'s row
        where no distance is NaN.  `stat('topk_ids_tiles')` tells how many tiles the call evaluated row by row.

        `row_tags` and `probe_masks` are `topk`'s: a row that is not eligible for the probe is dropped like one with a
        negative label, so an identity is listed with its best ELIGIBLE row."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        k = int(k)
        if k < 1 or k > TOPK_MAX:
            raise ValueError('k %d outside [1, %d]' % (k, TOPK_MAX))
        p, was_np = N.to_device_f32(probes, self._dev)
        if p.dim() == 1:
            p = p[None, :]
        if p.dim() != 2 or p.shape[1] != self.emd_size:
            raise ValueError('probes must be [B, %d], got %s' % (self.emd_size, tuple(p.shape)))
        B, G = p.shape[0], len(self)

        def ints(x, name, n):                                   # as `roc` converts its labels
            t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
            if t.numel() == 0:
                t = t.to(torch.int64)
            if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
                raise ValueError('%s must be integers, got %s' % (name, t.dtype))
            if tuple(t.shape) != (n,):
                raise ValueError('%s must have shape [%d], got %s' % (name, n, tuple(t.shape)))
            return t.to(device=self._dev, dtype=torch.int64).contiguous()

        rl = ints(row_labels, 'row_labels', G)
        ex = None if exclude is None else ints(exclude, 'exclude', B)
        rt, pm = _tag_pair(row_tags, probe_masks, G, B, self._dev)
        idx = torch.empty((B, k), dtype=torch.int64, device=self._dev)
        dist = torch.empty((B, k), dtype=torch.float32, device=self._dev)
        label = torch.empty((B, k), dtype=torch.int64, device=self._dev)
        self.topk_ids_into(p, k, distance_metric, rl, ex, idx, dist, label, rt, pm)
        if was_np:
            idx, dist, label = idx.cpu().numpy(), dist.cpu().numpy(), label.cpu().numpy()
        return idx, dist, label

    def cluster_into(self, tolerance, distance_metric, labels, n_clusters, first_row=0, prev=None):
        """Allocation-free form of `cluster`: results written into the caller's CUDA tensors labels [G] int64 and n_clusters
        (one int64 element, 0-d or [1]); `prev` [first_row] int64 CUDA holds the earlier labels when first_row > 0 (it may
        be `labels` itself or a slice of it)."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        tolerance = float(tolerance)
        if tolerance != tolerance:
            raise ValueError('cluster: the tolerance is NaN')
        G, first_row = len(self), int(first_row)
        if first_row < 0 or first_row > G:
            raise ValueError('first_row %d outside [0, %d]' % (first_row, G))
        if first_row > 0 and prev is None:
            raise ValueError('cluster: first_row > 0 needs the labels of the earlier call')
        for name, t in (('labels', labels), ('n_clusters', n_clusters), ('prev', prev)):
            if t is None and name == 'prev':
                continue
            if not torch.is_tensor(t) or t.dtype != torch.int64 or t.device != self._dev or not t.is_contiguous():
                raise ValueError('cluster_into: %s must be a contiguous %s tensor on %s' % (name, torch.int64, self._dev))
        if tuple(labels.shape) != (G,):
            raise ValueError('cluster_into: labels must have shape [%d], got %s' % (G, tuple(labels.shape)))
        if n_clusters.numel() != 1:
            raise ValueError('cluster_into: n_clusters must hold one element, got %s' % (tuple(n_clusters.shape),))
        if first_row > 0 and (prev.dim() != 1 or prev.shape[0] < first_row):
            raise ValueError('cluster_into: prev must hold the labels of rows [0, %d), got %s' % (first_row, tuple(prev.shape)))
        N.check(N.lib.dif_gallery_cluster(self._h, distance_metric, tolerance, first_row,
                                          N.ptr(prev) if first_row > 0 else None, N.ptr(labels) if G else None,
                                          N.ptr(n_clusters), N.stream_ptr()), ValueError)

    def cluster(self, tolerance, distance_metric=1, first_row=0, labels=None):
        """Which enrolled rows are the same person: exact single-linkage clustering at `tolerance`, i.e. the connected
        components of the graph whose edges are the pairs of rows within it.  -> (labels [G] int64, n_clusters 0-d int64),
        both on the device; nothing of size G x G is kept and nothing is read back.

        Every row i is a probe against rows[:i + 1]: ``d = evaluation.utility.distance(rows[i][None, :], rows[:i + 1], metric)``
        and every ``j`` with ``d[j] <= tolerance`` (inclusive; NaN is no edge) joins i's component.  labels[i] = index_base +
        the smallest row number of i's component -- canonical: two calls give identical tensors -- and n_clusters the number
        of components.  A row whose distances are all NaN or above the tolerance is a component of its own.  The tolerance
        has `within`'s units and edge cases: metric 0 is the SQUARED L2 distance; tolerance < 0 gives G singletons; under metric
        1 a tolerance >= 1 joins every pair whose distance is not NaN.  'clamp_nan' is honoured as `within` honours it: with the
        default 0 two identical rows whose similarity rounds above 1 have a NaN distance under metric 1 and are NOT joined, so
        de-duplicating exact copies under metric 1 wants set_option('clamp_nan', 1).

        Incremental form (enrolment): ``cluster(t, metric, first_row=r, labels=prev)`` with ``prev`` the labels of a call over
        rows [0, r) with the same tolerance and metric (a tensor or an array of at least r entries) probes rows [r, G) only and
        returns what the full call returns, at O((G - r) * G) cost.  A `prev` entry that no such call can have produced (outside
        [index_base, index_base + its own row]) gives n_clusters == -1.  After `remove` row numbers have moved and earlier
        labels are void: run the full call."""
        G, first_row = len(self), int(first_row)
        if first_row < 0 or first_row > G:
            raise ValueError('first_row %d outside [0, %d]' % (first_row, G))
        prev = None
        if first_row > 0:
            if labels is None:
                raise ValueError('cluster: first_row > 0 needs the labels of the earlier call')
            prev = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels, dtype=np.int64)))
            prev = prev.to(device=self._dev, dtype=torch.int64).contiguous()
        out = torch.empty((G,), dtype=torch.int64, device=self._dev)
        n = torch.empty((), dtype=torch.int64, device=self._dev)
        self.cluster_into(tolerance, distance_metric, out, n, first_row, prev)
        return out, n

    def dbscan_into(self, tolerance, min_samples, distance_metric, labels, degree, counts):
        """Allocation-free form of `dbscan`: results written into the caller's CUDA tensors labels [G] int64, degree [G] int32
        (or None: not wanted) and counts [2] int64."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        tolerance = float(tolerance)
        if tolerance != tolerance:
            raise ValueError('dbscan: the tolerance is NaN')
        min_samples = int(min_samples)
        if min_samples < 1:
            raise ValueError('dbscan: min_samples must be at least 1, got %d' % min_samples)
        G = len(self)
        for name, t, dt in (('labels', labels, torch.int64), ('degree', degree, torch.int32), ('counts', counts, torch.int64)):
            if t is None and name == 'degree':
                continue
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self._dev or not t.is_contiguous():
                raise ValueError('dbscan_into: %s must be a contiguous %s tensor on %s' % (name, dt, self._dev))
        if tuple(labels.shape) != (G,):
            raise ValueError('dbscan_into: labels must have shape [%d], got %s' % (G, tuple(labels.shape)))
        if degree is not None and tuple(degree.shape) != (G,):
            raise ValueError('dbscan_into: degree must have shape [%d], got %s' % (G, tuple(degree.shape)))
        if tuple(counts.shape) != (2,):
            raise ValueError('dbscan_into: counts must have shape [2], got %s' % (tuple(counts.shape),))
        N.check(N.lib.dif_gallery_dbscan(self._h, distance_metric, tolerance, min_samples, N.ptr(labels) if G else None,
                                         N.ptr(degree) if degree is not None and G else None, N.ptr(counts), N.stream_ptr()),
                ValueError)

    def dbscan(self, tolerance, min_samples=3, distance_metric=1):
        """Which enrolled rows are the same person, and which are nobody: exact density clustering with noise (DBSCAN) at
        `tolerance`.  -> (labels [G] int64, degree [G] int32, counts [2] int64), all on the device; nothing of size G x G is
        kept and nothing is read back.

        The edges are `cluster`'s: rows i > j with ``evaluation.utility.distance(rows[i][None, :], rows[j][None, :], metric) <=
        tolerance`` (row i is the probe; inclusive; NaN is no edge; same units, edge cases and 'clamp_nan' rule as `cluster`).
        degree[i] = 1 + the number of edges at row i (the row itself always counts).  A row is a CORE row when degree[i] >=
        min_samples.  Clusters are the connected components of the core rows under the edges between two core rows, and
        labels[c] = index_base + the smallest row of c's component.  A row that is no core but has a core row within the
        tolerance is a BORDER row: it takes the label of the nearest such core row (the edge's float32 distance; exact ties
        go to the lower row number) and joins nothing else, so it cannot bridge two people the way it does under `cluster`.
        Every other row is NOISE: labels[x] = -1, whatever index_base is.  counts = (number of clusters, number of noise rows).

        The result is canonical: two calls, or other 'cluster_round' values, give identical tensors.  min_samples = 1 gives
        `cluster`'s labels bit for bit and no noise; min_samples > G gives G noise rows.

        There is no incremental form and `first_row` is not offered: enrolling a row changes the degrees of the rows already
        there, and with them which rows are core.  Costs two sweeps of `cluster`'s lower triangle."""
        G = len(self)
        labels = torch.empty((G,), dtype=torch.int64, device=self._dev)
        degree = torch.empty((G,), dtype=torch.int32, device=self._dev)
        counts = torch.empty((2,), dtype=torch.int64, device=self._dev)
        self.dbscan_into(tolerance, min_samples, distance_metric, labels, degree, counts)
        return labels, degree, counts

    def roc_into(self, probes, probe_labels, row_labels, first_row, thresholds, distance_metric, accept, totals):
        """Allocation-free form of `roc`, the library's own terms: `probes` [B, d] float32, `probe_labels` [B] int64,
        `row_labels` [len(self)] int64, `first_row` [B] int64 or None, `thresholds` [T] float32 NON-DECREASING -- all CUDA;
        results written into the caller's CUDA tensors accept [T, 2] int64 and totals [4] int64.  The thresholds are checked
        by the library (one 4 KB read; ValueError with its message); the counts are not read back."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        if not torch.is_tensor(probes) or probes.dim() != 2 or probes.shape[1] != self.emd_size:
            raise ValueError('probes must be a [B, %d] tensor, got %s' % (
                self.emd_size, tuple(probes.shape) if hasattr(probes, 'shape') else type(probes).__name__))
        B, G = probes.shape[0], len(self)
        for name, t, dt, shape in (('probes', probes, torch.float32, None), ('probe_labels', probe_labels, torch.int64, (B,)),
                                   ('row_labels', row_labels, torch.int64, (G,)), ('first_row', first_row, torch.int64, (B,)),
                                   ('thresholds', thresholds, torch.float32, None), ('accept', accept, torch.int64, None),
                                   ('totals', totals, torch.int64, (4,))):
            if t is None and name == 'first_row':
                continue
            if not torch.is_tensor(t) or t.dtype != dt or t.device != self._dev or not t.is_contiguous():
                raise ValueError('roc_into: %s must be a contiguous %s tensor on %s' % (name, dt, self._dev))
            if shape is not None and tuple(t.shape) != shape:
                raise ValueError('roc_into: %s must have shape %s, got %s' % (name, list(shape), tuple(t.shape)))
        if thresholds.dim() != 1:
            raise ValueError('roc_into: thresholds must have shape [T], got %s' % (tuple(thresholds.shape),))
        T = thresholds.shape[0]
        if tuple(accept.shape) != (T, 2):
            raise ValueError('roc_into: accept must have shape [%d, 2], got %s' % (T, tuple(accept.shape)))
        N.check(N.lib.dif_match_roc(self._h, N.ptr(probes) if B else None, B, distance_metric,
                                    N.ptr(probe_labels) if B else None, N.ptr(row_labels) if G else None,
                                    N.ptr(first_row) if first_row is not None and B else None,
                                    N.ptr(thresholds) if T else None, T, N.ptr(accept) if T else None, N.ptr(totals),
                                    N.stream_ptr()), ValueError)

    def roc(self, probes, probe_labels, row_labels, thresholds, distance_metric=1, first_row=None):
        """All-pairs verification counts: how many genuine and impostor (probe, enrolled row) pairs lie below each threshold,
        exact, in one pass over the gallery whatever the number of thresholds.
        -> (accept [T, 2] int64, totals [4] int64), both on the device and in the caller's threshold order.

        With ``dist = evaluation.utility.distance(q[:, None], gallery[None, :], metric)`` (never materialised),
        ``use = (probe_labels[:, None] >= 0) & (row_labels[None, :] >= 0) & (index_base + arange(G)[None, :] >= first_row[:, None])``
        and ``same = probe_labels[:, None] == row_labels[None, :]``:
        accept[j] = [sum(use & same & (dist < thresholds[j])), sum(use & ~same & (dist < thresholds[j]))] -- strict, as
        calculate_val_far's np.less; NaN < t is False -- and totals = [sum(use & same), sum(use & ~same), and of each the pairs
        whose dist is NaN].  Labels are integers (any integer dtype; a negative one takes the probe or row out of every pair),
        `row_labels` in the gallery's row order; the gallery stores none.  `first_row` [B] (default: zeros) is a global row
        index: a labelled set against itself passes its own row + 1 and gets every unordered pair once
        (evaluation.verification.all_pairs_counts).  `thresholds`: up to 1024 numbers in any order, float64 welcome -- they are
        converted with `up32`, the rule under which a float32 distance compares with them as NumPy compares it in double, and
        sorted for the library; duplicates, values <= 0 or > 1 and +-inf are fine, a NaN raises ValueError.  Distances, units
        and the NaN rule ('clamp_nan') are `within`'s; an empty gallery gives zeros."""
        if distance_metric not in (0, 1):
            raise RuntimeError('Undefined distance metric %d' % distance_metric)
        p, _ = N.to_device_f32(probes, self._dev)
        if p.dim() == 1:
            p = p[None, :]
        if p.dim() != 2 or p.shape[1] != self.emd_size:
            raise ValueError('probes must be [B, %d], got %s' % (self.emd_size, tuple(p.shape)))
        B, G = p.shape[0], len(self)

        def ints(x, name, n):
            t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
            if t.numel() == 0:
                t = t.to(torch.int64)
            if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
                raise ValueError('%s must be integers, got %s' % (name, t.dtype))
            if tuple(t.shape) != (n,):
                raise ValueError('%s must have shape [%d], got %s' % (name, n, tuple(t.shape)))
            return t.to(device=self._dev, dtype=torch.int64).contiguous()

        pl, rl = ints(probe_labels, 'probe_labels', B), ints(row_labels, 'row_labels', G)
        fr = None if first_row is None else ints(first_row, 'first_row', B)
        th = thresholds.detach().cpu().numpy() if torch.is_tensor(thresholds) else np.asarray(thresholds)
        t32 = up32(th.astype(np.float64).reshape(-1))
        order = np.argsort(t32, kind='stable')                  # (a NaN sorts last and the library names it)
        ts = torch.from_numpy(np.ascontiguousarray(t32[order])).to(self._dev)
        T = ts.shape[0]
        acc = torch.empty((T, 2), dtype=torch.int64, device=self._dev)
        totals = torch.empty((4,), dtype=torch.int64, device=self._dev)
        self.roc_into(p, pl, rl, fr, ts, distance_metric, acc, totals)
        accept = torch.empty_like(acc)
        accept[torch.from_numpy(order).to(self._dev)] = acc     # back to the caller's order, on the device
        return accept, totals

    def close(self):
        if self._h:
            N.lib.dif_gallery_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def match(probes, gallery, distance_metric=1):
    """One-call form: top-1 gallery index and distance for each probe row."""
    g = gallery if isinstance(gallery, Gallery) else Gallery(gallery)
    try:
        return g.match(probes, distance_metric)
    finally:
        if g is not gallery:
            g.close()


def within(probes, gallery, tolerance, distance_metric=1, max_hits=64, row_tags=None, probe_masks=None):
    """One-call form of Gallery.within: per probe, how many gallery rows lie within `tolerance` and the first
    `max_hits` of them -> (count[B], idx[B, K], dist[B, K]); with `row_tags` and `probe_masks`, among the rows the probe is
    eligible for."""
    g = gallery if isinstance(gallery, Gallery) else Gallery(gallery)
    try:
        return g.within(probes, tolerance, distance_metric, max_hits, row_tags, probe_masks)
    finally:
        if g is not gallery:
            g.close()


def rank(probes, gallery, mates, distance_metric=1, row_tags=None, probe_masks=None):
    """One-call form of Gallery.rank: per probe, the rank of its mate row among all gallery rows and the mate's distance
    -> (rank[B], mate_dist[B]); with `row_tags` and `probe_masks`, among the rows the probe is eligible for."""
    g = gallery if isinstance(gallery, Gallery) else Gallery(gallery)
    try:
        return g.rank(probes, mates, distance_metric, row_tags, probe_masks)
    finally:
        if g is not gallery:
            g.close()


def topk(probes, gallery, k, distance_metric=1, row_tags=None, probe_masks=None):
    """One-call form of Gallery.topk: per probe, the k nearest gallery rows in order -> (idx[B, k], dist[B, k]); with
    `row_tags` and `probe_masks`, the k nearest rows the probe is eligible for."""
    g = gallery if isinstance(gallery, Gallery) else Gallery(gallery)
    try:
        return g.topk(probes, k, distance_metric, row_tags, probe_masks)
    finally:
        if g is not gallery:
            g.close()


def topk_ids(probes, gallery, k, row_labels, distance_metric=1, exclude=None, row_tags=None, probe_masks=None):
    """One-call form of Gallery.topk_ids: per probe, the k nearest distinct identities, each with its best row
    -> (idx[B, k], dist[B, k], label[B, k]); `row_tags` and `probe_masks` as in Gallery.topk."""
    g = gallery if isinstance(gallery, Gallery) else Gallery(gallery)
    try:
        return g.topk_ids(probes, k, row_labels, distance_metric, exclude, row_tags, probe_masks)
    finally:
        if g is not gallery:
            g.close()


def cluster(embeddings, tolerance, distance_metric=1):
    """One-call form of Gallery.cluster on a temporary gallery of `embeddings` [M, d]: which rows are the same person
    -> (labels[M] int64, n_clusters 0-d int64), on the device."""
    g = embeddings if isinstance(embeddings, Gallery) else Gallery(embeddings)
    try:
        labels, n = g.cluster(tolerance, distance_metric)
        torch.cuda.current_stream().synchronize()   # the temporary gallery is freed below: the work must have ended
        return labels, n
    finally:
        if g is not embeddings:
            g.close()


def dbscan(embeddings, tolerance, min_samples=3, distance_metric=1):
    """One-call form of Gallery.dbscan on a temporary gallery of `embeddings` [M, d]: density clustering with noise
    -> (labels[M] int64, -1 = noise; degree[M] int32; counts[2] int64: clusters, noise rows), on the device."""
    g = embeddings if isinstance(embeddings, Gallery) else Gallery(embeddings)
    try:
        out = g.dbscan(tolerance, min_samples, distance_metric)
        torch.cuda.current_stream().synchronize()   # the temporary gallery is freed below: the work must have ended
        return out
    finally:
        if g is not embeddings:
            g.close()


def one_shot_clf(probe, gallery, distance_metric=1):
    """Identify one face: index of the nearest enrolled embedding and its distance
    (name kept from the reference stub, deep_insight_face/oneshot.py:110)."""
    idx, dist = match(probe, gallery, distance_metric)
    return int(idx[0]), float(dist[0])


def cosine_similarity_matrix(embeddings1, embeddings2=None):
    """All-pairs cosine similarity ``l2norm(E1) @ l2norm(E2).T`` -> [B, G] float32 (E2 defaults to E1):
    the reference's own "cosine = matmul of normalised rows" (common/losses.py:39-40, :137-138), as one
    MFMA GEMM with both normalisations in its epilogue (csrc/arcmargin.hip with scale 1, no margin).
    NumPy in -> NumPy out."""
    from .networks.arcmargin import ArcMarginHead
    if embeddings2 is None:
        embeddings2 = embeddings1
    head = ArcMarginHead(embeddings2, s=1.0, m=0.0)
    try:
        return head.logits(embeddings1)
    finally:
        head.close()
