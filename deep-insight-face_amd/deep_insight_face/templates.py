"""Template pooling (csrc/templates.hip): one exact mean embedding per identity, on the device.

A 1:N system enrols one row per person: the several images of a person, or the frames of a track, pooled into a mean
embedding that is usually re-normalised.  ``TemplatePool`` turns rows and labels -- a directory's identities, or the labels
of ``oneshot.Gallery.cluster`` / ``dbscan`` -- into those rows, and keeps doing so as more rows arrive::

    pool = TemplatePool(512)
    index = pool.add(embeddings, labels)         # index[i]: the template of row i, -1 for a negative label
    gallery = oneshot.Gallery(pool.templates())  # row t is the template of pool.labels[t]

The arithmetic is NumPy's float32, bit for bit: a template's sum is ``np.add.reduce(x[labels == l], axis=0)`` -- its rows
in ascending row number, one rounded add after the other --, the mean divides by ``float32(count)`` and the normalised
template by ``np.linalg.norm(mean, axis=1, keepdims=True)``.  With weights the sum is ``(... + fl(w_r * x_r))`` and the mean
divides by the float32 sum of the weights; weights are used as given.  A zero-norm template is a NaN row, as NumPy gives
it, and the gallery ranks such rows as the reference does.  Rows with a negative label are left out (``roc``'s and
``topk_ids``' convention; ``dbscan``'s noise).  The templates are the distinct non-negative labels in ascending order.

Sequential sums make enrolment incremental: ``add`` continues every stored sum over the new rows, and the result is
bit-identical to one ``add`` of all rows ever added, in order.  A new label takes its ascending position, so the templates
behind it shift: rebuild a live gallery with ``Gallery.set`` after an add that inserts labels.

One ``add`` reads 8 bytes back -- the number of templates, to size its buffers -- and that is its one synchronisation.

``BestShots`` keeps, on the same grouping, the ONE best row of every label instead of their mean: the face with the
greatest key (``detector.quality``'s score, say) and whatever payload rows -- crops, embeddings, boxes -- come with it.
"""
import ctypes

import numpy as np
import torch

from . import _native as N


def _ints(x, name, n, dev):                                     # as oneshot.Gallery.topk_ids converts its labels
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.numel() == 0:
        t = t.to(torch.int64)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError('%s must be integers, got %s' % (name, t.dtype))
    if tuple(t.shape) != (n,):
        raise ValueError('%s must have shape [%d], got %s' % (name, n, tuple(t.shape)))
    return t.to(device=dev, dtype=torch.int64).contiguous()


class TemplatePool:
    """The templates of every label seen so far: ``labels`` [T] int64 ascending, ``sums`` [T, emd_size] float32, ``counts`` [T]
    int64 (rows per template) and, in a weighted pool, ``wsum`` [T] float32, all on the device."""

    def __init__(self, emd_size, weighted=False, device=None):
        emd_size = int(emd_size)
        if emd_size <= 0 or emd_size % 32 != 0:
            raise ValueError('emd_size must be a positive multiple of 32, got %d' % emd_size)
        self._dev = N.require_device() if device is None else torch.device(device)
        self.emd_size, self.weighted = emd_size, bool(weighted)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self._dev):
            N.check(N.lib.dif_pool_create(ctypes.byref(self._h), emd_size))
        self.labels = torch.empty((0,), dtype=torch.int64, device=self._dev)
        self.sums = torch.empty((0, emd_size), dtype=torch.float32, device=self._dev)
        self.wsum = torch.empty((0,), dtype=torch.float32, device=self._dev) if self.weighted else None
        self.counts = torch.empty((0,), dtype=torch.int64, device=self._dev)

    def close(self):
        if self._h:
            N.lib.dif_pool_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self.labels.shape[0])

    @staticmethod
    def _read_total(t_dev):
        """The one host read of an ``add``: the number of templates after it."""
        return int(t_dev.item())

    def add(self, embeddings, labels, weights=None):
        """Pools ``embeddings`` [N, emd_size] float32 under ``labels`` [N] (any integer dtype; a negative label leaves the row
        out) and, in a weighted pool, ``weights`` [N] float32 into the templates.  -> index [N] int64: the position of each
        row's template among ``self.labels`` AFTER this add, -1 for a negative label; NumPy in -> NumPy out."""
        if not self._h:
            raise ValueError('the pool is closed')
        if self.weighted and weights is None:
            raise ValueError('a weighted pool needs the weights of the rows')
        if not self.weighted and weights is not None:
            raise ValueError('weights given to an unweighted pool (TemplatePool(..., weighted=True))')
        for name, v in (('embeddings', embeddings), ('weights', weights)):
            dt = getattr(v, 'dtype', None)
            if v is not None and dt is not None and dt not in (torch.float32, np.dtype(np.float32)):
                raise ValueError('%s must be float32, got %s' % (name, dt))
        x, was_np = N.to_device_f32(embeddings, self._dev)
        if x.dim() != 2 or x.shape[1] != self.emd_size:
            raise ValueError('embeddings must be [N, %d], got %s' % (self.emd_size, tuple(x.shape)))
        n, t0 = int(x.shape[0]), len(self)
        lab = _ints(labels, 'labels', n, self._dev)
        w = None
        if weights is not None:
            w, _ = N.to_device_f32(weights, self._dev)
            if tuple(w.shape) != (n,):
                raise ValueError('weights must have shape [%d], got %s' % (n, tuple(w.shape)))
        if n + t0 >= 2 ** 31:
            raise ValueError('rows and templates together must stay below 2^31')
        opt = lambda t: N.ptr(t) if t is not None and t.numel() else None   # noqa: E731
        with torch.cuda.device(self._dev):
            index = torch.empty((n,), dtype=torch.int64, device=self._dev)
            t_dev = torch.empty((1,), dtype=torch.int64, device=self._dev)
            N.check(N.lib.dif_pool_group(self._h, opt(self.labels), t0, opt(lab), n, opt(index), N.ptr(t_dev), N.stream_ptr()))
            t = self._read_total(t_dev)
            new_labels = torch.empty((t,), dtype=torch.int64, device=self._dev)
            new_sums = torch.empty((t, self.emd_size), dtype=torch.float32, device=self._dev)
            new_wsum = torch.empty((t,), dtype=torch.float32, device=self._dev) if self.weighted else None
            new_counts = torch.empty((t,), dtype=torch.int64, device=self._dev)
            N.check(N.lib.dif_pool_reduce(self._h, opt(self.sums), opt(self.wsum), opt(self.counts), opt(x), opt(w), t, opt(new_labels),
                                          opt(new_sums), opt(new_wsum), opt(new_counts), N.stream_ptr()))
        self.labels, self.sums, self.wsum, self.counts = new_labels, new_sums, new_wsum, new_counts
        return index.cpu().numpy() if was_np else index

    def templates(self, normalize=True):
        """-> [T, emd_size] float32 on the device: the mean of every template, divided by its norm with ``normalize``; row t
        belongs to ``self.labels[t]``."""
        if not self._h:
            raise ValueError('the pool is closed')
        t = len(self)
        out = torch.empty((t, self.emd_size), dtype=torch.float32, device=self._dev)
        if t:
            with torch.cuda.device(self._dev):
                N.check(N.lib.dif_pool_finish(N.ptr(self.sums), N.ptr(self.wsum) if self.weighted else None, N.ptr(self.counts), t,
                                              self.emd_size, 1 if normalize else 0, N.ptr(out), N.stream_ptr()))
        return out


class BestShots:
    """The best shot of every label seen so far -- the ONE row with the greatest key, a face quality say -- next to
    ``TemplatePool``::

        shots = BestShots()
        index = shots.add(tracks.labels, q.score, crops=faces.crops, emb=faces.emb)
        shots.payload['crops']                   # [T, S, S, 3]: the thumbnail of shots.labels[t]

    ``labels`` [T] int64 ascending, ``key`` [T] float32, ``row`` [T] int64 (rows count on from add to add: row i of an add is
    ``row_base + i``), ``counts`` [T] int64 (rows seen, NaN keys included) and ``payload``, a dict of [T, ...] tensors, stay
    in step, on the device.  The rule is ``dif_pool_best``'s: the greatest key, exact ties to the lower row, -0.0 ties with
    +0.0, a NaN key is never chosen and -inf is an ordinary key; a label that has shown NaN keys only has row -1, key NaN
    and a zero payload.  A negative label leaves the row out.  Adding in chunks equals adding at once, bit for bit,
    payloads included; a new label takes its ascending position, as in ``TemplatePool``.  One ``add`` reads 8 bytes back."""

    def __init__(self, device=None):
        self._dev = N.require_device() if device is None else torch.device(device)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self._dev):
            N.check(N.lib.dif_pool_create(ctypes.byref(self._h), 32))     # (the embedding size is dif_pool_reduce's alone)
        i64 = dict(dtype=torch.int64, device=self._dev)
        self.labels, self.row, self.counts = torch.empty((0,), **i64), torch.empty((0,), **i64), torch.empty((0,), **i64)
        self.key = torch.empty((0,), dtype=torch.float32, device=self._dev)
        self.payload = {}
        self.row_base = 0

    def close(self):
        if self._h:
            N.lib.dif_pool_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self.labels.shape[0])

    def add(self, labels, key, **payload):
        """``labels`` [N] integers, ``key`` [N] float32, every payload [N, ...] (the same names on every add) -> index [N] int64:
        the position of each row's label among ``self.labels`` AFTER this add, -1 for a negative label; NumPy in -> NumPy
        out."""
        if not self._h:
            raise ValueError('the shots are closed')
        dt = getattr(key, 'dtype', None)
        if dt is not None and dt not in (torch.float32, np.dtype(np.float32)):
            raise ValueError('key must be float32, got %s' % dt)
        k, was_np = N.to_device_f32(key, self._dev)
        if k.dim() != 1:
            raise ValueError('key must be [N], got %s' % (tuple(k.shape),))
        n, t0 = int(k.shape[0]), len(self)
        lab = _ints(labels, 'labels', n, self._dev)
        if (self.row_base or t0) and set(payload) != set(self.payload):
            raise ValueError('payloads %s given, %s kept' % (sorted(payload), sorted(self.payload)))
        rows = {}
        for name, v in payload.items():
            v = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))
            if v.dim() < 1 or v.shape[0] != n:
                raise ValueError('payload %s must be [%d, ...], got %s' % (name, n, tuple(v.shape)))
            kept = self.payload.get(name)
            if kept is not None and (kept.shape[1:] != v.shape[1:] or kept.dtype != v.dtype):
                raise ValueError('payload %s was %s %s per row, now %s %s' % (name, kept.dtype, tuple(kept.shape[1:]), v.dtype,
                                                                             tuple(v.shape[1:])))
            rows[name] = v.to(self._dev)
        if n + t0 >= 2 ** 31:
            raise ValueError('rows and labels together must stay below 2^31')
        opt = lambda t: N.ptr(t) if t is not None and t.numel() else None   # noqa: E731
        i64 = dict(dtype=torch.int64, device=self._dev)
        with torch.cuda.device(self._dev):
            index, t_dev = torch.empty((n,), **i64), torch.empty((1,), **i64)
            N.check(N.lib.dif_pool_group(self._h, opt(self.labels), t0, opt(lab), n, opt(index), N.ptr(t_dev), N.stream_ptr()))
            t = TemplatePool._read_total(t_dev)
            new_labels, new_row, new_counts = torch.empty((t,), **i64), torch.empty((t,), **i64), torch.empty((t,), **i64)
            new_key = torch.empty((t,), dtype=torch.float32, device=self._dev)
            N.check(N.lib.dif_pool_best(self._h, opt(self.key), opt(self.row), opt(self.counts), opt(k), self.row_base, t, opt(new_labels),
                                        opt(new_key), opt(new_row), opt(new_counts), N.stream_ptr()))
            # the winner's payload: of this add where its row is new, else the stored one (a label new to this add with
            # NaN keys only has neither: zeros)
            fresh = new_row >= self.row_base
            src_new = (new_row - self.row_base).clamp(min=0)
            at = torch.searchsorted(self.labels, new_labels).clamp(max=max(t0 - 1, 0))
            stored = ~fresh & (self.labels[at] == new_labels) if t0 else torch.zeros_like(fresh)
            merged = {}
            for name, v in rows.items():
                shape = (t,) + (1,) * (v.dim() - 1)
                out = torch.zeros((t,) + tuple(v.shape[1:]), dtype=v.dtype, device=self._dev)
                if n:
                    out = torch.where(fresh.view(shape), v[src_new], out)
                if t0:
                    out = torch.where(stored.view(shape), self.payload[name][at], out)
                merged[name] = out
        self.labels, self.key, self.row, self.counts, self.payload = new_labels, new_key, new_row, new_counts, merged
        self.row_base += n
        return index.cpu().numpy() if was_np else index


def pool_templates(embeddings, labels, weights=None, normalize=True):
    """One call: ``embeddings`` [N, d] float32 (d a multiple of 32), ``labels`` [N] integers, optional ``weights`` [N] float32
    -> (templates [T, d], template_labels [T] int64, counts [T] int64, index [N] int64); NumPy in -> NumPy out."""
    shape = tuple(getattr(embeddings, 'shape', ()))
    if len(shape) != 2:
        raise ValueError('embeddings must be [N, d], got %s' % (shape,))
    pool = TemplatePool(shape[1], weighted=weights is not None,
                        device=embeddings.device if torch.is_tensor(embeddings) and embeddings.is_cuda else None)
    try:
        index = pool.add(embeddings, labels, weights)
        out = pool.templates(normalize), pool.labels, pool.counts
    finally:
        pool.close()
    if not torch.is_tensor(index):
        out = tuple(t.cpu().numpy() for t in out)
    return out + (index,)
