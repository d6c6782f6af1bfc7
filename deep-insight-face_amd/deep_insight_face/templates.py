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
