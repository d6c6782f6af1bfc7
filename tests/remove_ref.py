"""Swap-remove from the tail, the statement Gallery.remove / dif_gallery_remove is held to.

`rows` [n, ...] and the distinct LOCAL indices `R` (k of them) -> the new_n = n - k rows that remain: rows below new_n
that are not in R keep their index, the i-th surviving row of the tail [new_n, n) fills the i-th hole below new_n, both in
ascending order.  Returns (out, moved_from, moved_to), local indices."""
import numpy as np


def remove_ref(rows, R):
    rows = np.asarray(rows)
    n = rows.shape[0]
    R = np.unique(np.asarray(R, dtype=np.int64))
    new_n = n - R.shape[0]
    keep = np.ones(n, bool); keep[R] = False
    holes = np.flatnonzero(~keep[:new_n]);  surv = new_n + np.flatnonzero(keep[new_n:])   # same length m
    out = rows[:new_n].copy();  out[holes] = rows[surv]            # i-th surviving tail row -> i-th hole, both ascending
    return out, surv.astype(np.int64), holes.astype(np.int64)


def relocate(index, R, moved_from, moved_to):
    """Where the rows `index` (local, before the removal) are afterwards: -1 for a removed row."""
    index = np.asarray(index, dtype=np.int64)
    new = index.copy()
    new[np.isin(index, np.asarray(R, dtype=np.int64))] = -1
    for f, t in zip(moved_from, moved_to):
        new[index == f] = t
    return new
