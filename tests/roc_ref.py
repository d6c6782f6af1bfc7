"""NumPy statement of the all-pairs verification counts (oneshot.Gallery.roc / dif_match_roc), over the oracle's distances.

    dist  = oracle.distance.distance(q[:, None], gallery[None, :], metric)          float32, B x G
    use   = (probe_labels[:, None] >= 0) & (row_labels[None, :] >= 0) & (index_base + arange(G)[None, :] >= first_row[:, None])
    same  = probe_labels[:, None] == row_labels[None, :]
    accept[j] = [sum(use & same & (dist < t[j])), sum(use & ~same & (dist < t[j]))]  np.less in DOUBLE; NaN < t is False
    totals    = [sum(use & same), sum(use & ~same), sum(use & same & isnan(dist)), sum(use & ~same & isnan(dist))]

`counts_full` forms the counts from sorted distances (np.searchsorted); `counts_direct` is the statement above word for
word, for small shapes -- tests/test_roc_ref.py holds the one against the other.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from rank_ref import distances   # noqa: F401  (the B x G float32 distances of the oracle)


def up32(thresholds):
    """The smallest float32 >= each float64 threshold: for a float32 d,  d < t64  iff  d < up32(t64)."""
    t64 = np.asarray(thresholds, dtype=np.float64)
    with np.errstate(over='ignore'):
        t32 = t64.astype(np.float32)
    return np.where(t32.astype(np.float64) < t64, np.nextafter(t32, np.float32(np.inf)), t32).astype(np.float32)


def _use_same(B, G, probe_labels, row_labels, first_row, index_base):
    pl = np.asarray(probe_labels, dtype=np.int64).reshape(B)
    rl = np.asarray(row_labels, dtype=np.int64).reshape(G)
    fr = np.zeros(B, dtype=np.int64) if first_row is None else np.asarray(first_row, dtype=np.int64).reshape(B)
    use = (pl[:, None] >= 0) & (rl[None, :] >= 0) & ((int(index_base) + np.arange(G, dtype=np.int64))[None, :] >= fr[:, None])
    return use, pl[:, None] == rl[None, :]


def counts_direct(full, probe_labels, row_labels, thresholds, first_row=None, index_base=0):
    B, G = full.shape
    use, same = _use_same(B, G, probe_labels, row_labels, first_row, index_base)
    d = full.astype(np.float64)
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    accept = np.zeros((t.size, 2), dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for j in range(t.size):
            accept[j, 0] = np.sum(use & same & np.less(d, t[j]))
            accept[j, 1] = np.sum(use & ~same & np.less(d, t[j]))
    nan = np.isnan(full)
    totals = np.array([np.sum(use & same), np.sum(use & ~same), np.sum(use & same & nan), np.sum(use & ~same & nan)],
                      dtype=np.int64)
    return accept, totals


def counts_full(full, probe_labels, row_labels, thresholds, first_row=None, index_base=0):
    """-> (accept [T, 2] int64, totals [4] int64) from precomputed float32 distances full [B, G]; thresholds in any order,
    compared in double."""
    B, G = full.shape
    use, same = _use_same(B, G, probe_labels, row_labels, first_row, index_base)
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    accept = np.zeros((t.size, 2), dtype=np.int64)
    totals = np.zeros(4, dtype=np.int64)
    for c, sel in enumerate((use & same, use & ~same)):
        v = full[sel].astype(np.float64)
        nan = np.isnan(v)
        accept[:, c] = np.searchsorted(np.sort(v[~nan]), t, side='left')   # the number of distances < t
        totals[c], totals[2 + c] = v.size, int(nan.sum())
    return accept, totals


def counts(probes, gallery, probe_labels, row_labels, thresholds, metric=1, first_row=None, index_base=0):
    return counts_full(distances(probes, gallery, metric), probe_labels, row_labels, thresholds, first_row, index_base)
