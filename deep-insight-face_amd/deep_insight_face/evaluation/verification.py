"""1:1 verification over EVERY pair of a labelled set, on top of oneshot.Gallery.roc: the accept counts of genuine and
impostor pairs at each threshold, and VAL / TAR at a false-accept rate from them.

The reference's verification protocol (evaluation/utility.py calculate_val_far / calculate_val / calculate_roc; here
utility.py and csrc/evalproto.hip) works on a caller-made list of pairs, LFW's 6 000.  An operating point such as TAR at
FAR = 1e-6 needs of the order of 1e8 impostor pairs to resolve: all pairs of a labelled set (the IJB / MegaFace style).
`all_pairs_counts` produces those counts on the device in one pass of the gallery per block of probes, whatever the number
of thresholds; the rest is array arithmetic on [T, 2] integers -- NumPy arrays or tensors in, NumPy out.  Conventions
(oneshot.Gallery.roc): the comparison is strict (`dist < threshold`, calculate_val_far's np.less), a NaN distance passes
no threshold but is part of the totals, a negative label takes a row out of every pair."""
import numpy as np
import torch


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def all_pairs_counts(embeddings, labels, thresholds, distance_metric=1, block=512):
    """Every unordered pair of rows of `embeddings` [n, d] once, no row with itself: enrols the set, walks it in blocks of
    `block` probes with first_row = own row + 1 and sums.  `labels` [n] integers (negative: the row is in no pair).
    -> (accept [T, 2] int64, totals [4] int64) on the device, as oneshot.Gallery.roc; totals[0] + totals[1] is
    n (n - 1) / 2 when no label is negative."""
    from .. import _native as N
    from ..oneshot import Gallery
    block = int(block)
    if block < 1:
        raise ValueError('block must be positive, got %d' % block)
    gal = Gallery(embeddings)
    try:
        dev = gal._dev
        e, _ = N.to_device_f32(embeddings, dev)
        n = e.shape[0]
        lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
        if lab.dtype.is_floating_point or lab.dtype.is_complex or lab.dtype == torch.bool:
            raise ValueError('labels must be integers, got %s' % lab.dtype)
        if tuple(lab.shape) != (n,):
            raise ValueError('labels must have shape [%d], got %s' % (n, tuple(lab.shape)))
        lab = lab.to(device=dev, dtype=torch.int64).contiguous()
        T = int(np.asarray(_np(thresholds)).size)
        accept = torch.zeros((T, 2), dtype=torch.int64, device=dev)
        totals = torch.zeros((4,), dtype=torch.int64, device=dev)
        own = torch.arange(1, n + 1, dtype=torch.int64, device=dev)
        for b0 in range(0, max(n, 1), block):
            b1 = min(n, b0 + block)
            a, t = gal.roc(e[b0:b1], lab[b0:b1], lab, thresholds, distance_metric, first_row=own[b0:b1])
            accept += a
            totals += t
        torch.cuda.current_stream().synchronize()   # the temporary gallery is freed below: the work must have ended
        return accept, totals
    finally:
        gal.close()


def val_far(accept, totals):
    """The reference's val / far at every threshold -> (val [T], far [T]) float64: accepted genuine pairs over all genuine
    pairs, accepted impostor pairs over all impostor pairs, and calculate_val_far's rule for an empty denominator: 0."""
    a = _np(accept).astype(np.int64).reshape(-1, 2)
    t = _np(totals).astype(np.int64).reshape(-1)
    n_same, n_diff = int(t[0]), int(t[1])
    val = np.zeros(a.shape[0]) if n_same == 0 else a[:, 0].astype(np.float64) / float(n_same)
    far = np.zeros(a.shape[0]) if n_diff == 0 else a[:, 1].astype(np.float64) / float(n_diff)
    return val, far


def tar_at_far(accept, totals, thresholds, far_targets):
    """The operating points a verification system is quoted at -> (threshold [K], tar [K]) float64, one per entry of
    `far_targets`: the LARGEST listed threshold whose FAR is <= the target, and the TAR (val) there.  No interpolation: both
    numbers are ones the counts support.  NaN where the impostor count cannot resolve the target (1 / n_diff > target: one
    false accept already exceeds it), and where no listed threshold reaches down to it."""
    th = np.asarray(_np(thresholds), dtype=np.float64).reshape(-1)
    val, far = val_far(accept, totals)
    n_diff = int(_np(totals).reshape(-1)[1])
    targets = np.asarray(far_targets, dtype=np.float64).reshape(-1)
    thr_out = np.full(targets.shape, np.nan)
    tar_out = np.full(targets.shape, np.nan)
    for k, target in enumerate(targets):
        if n_diff == 0 or 1.0 / n_diff > target:
            continue
        ok = np.flatnonzero((far <= target) & ~np.isnan(th))
        if ok.size == 0:
            continue
        j = ok[np.argmax(th[ok])]
        thr_out[k], tar_out[k] = th[j], val[j]
    return thr_out, tar_out


def val_at_far(embeddings, labels, thresholds, far_target, distance_metric=1, block=512):
    """The reference's two steps of calculate_val over all pairs, without folds -> (val, far, threshold).
    1. the FAR curve at `thresholds` picks the threshold at `far_target` by np.interp (piecewise linear, as this package's
       calculate_val and for the reason stated there); a curve that never reaches the target picks 0.0, as the reference;
    2. a second pass with that one threshold gives val and far -- counted, not interpolated."""
    th = np.sort(np.asarray(_np(thresholds), dtype=np.float64).reshape(-1))
    accept, totals = all_pairs_counts(embeddings, labels, th, distance_metric, block)
    _, far = val_far(accept, totals)
    if far.size and np.max(far) >= far_target:
        threshold = float(np.interp(far_target, far, th))
    else:
        threshold = 0.0
    accept, totals = all_pairs_counts(embeddings, labels, [threshold], distance_metric, block)
    val, far = val_far(accept, totals)
    return float(val[0]), float(far[0]), threshold
