"""NumPy statement of the tagged (watch-list) top-k searches: oneshot.Gallery.topk / topk_ids with `row_tags` and `probe_masks`
(dif_match_topk_tagged / dif_match_topk_ids_tagged), over the oracle's distances (rank_ref.distances).

`row_tags` is int64 [G], one 64-bit set per enrolled row in local row order; `probe_masks` is int64 [n], one per probe.

    eligible[p, r] = (row_tags[r] & probe_masks[p]) != 0       the raw 64 bits: a negative value has bit 63 set;
                                                               a tag of 0 is never eligible, a mask of 0 sees no row

For probe p with query q:

    d = oracle.distance.distance(q[None, :], gallery, metric);  d[~eligible[p]] = NaN
    rows:        exactly topk_ref.topk_row(d, k, index_base)
    identities:  topk_ids_ref.topk_ids_row with  ok &= eligible[p]  -- the same d serves: a NaN distance is never usable

Everything else -- stable order with ties to the lower row, NaN never listed, the -1 / NaN (and label -1) padding, clamp_nan,
index_base, k in [1, 128] -- is the untagged searches'.  NumPy only."""
import numpy as np

import topk_ids_ref
import topk_ref

MASK_CYCLE = np.array([1, 2, 4, 8, -(1 << 63), 0, -1, 6], dtype=np.int64)   # per probe: the GPU tests' eight masks


def as_sets(x):
    """Any integer array -> int64 with the same low 64 bits (uint64 reinterpreted, narrower types sign-extended)."""
    a = np.asarray(x)
    if a.dtype.kind not in 'iu':
        raise ValueError('bit sets must be integers, got %s' % a.dtype)
    return a.view(np.int64) if a.dtype == np.uint64 else a.astype(np.int64)


def eligible(row_tags, probe_masks):
    """[n, G] bool."""
    t, m = as_sets(row_tags), as_sets(probe_masks)
    return (t[None, :] & m[:, None]) != 0


def masked(full, row_tags, probe_masks):
    """The oracle's distances full [n, G] with the ineligible pairs set to NaN (a new float32 array)."""
    out = np.array(full, dtype=np.float32)
    out[~eligible(row_tags, probe_masks)] = np.nan
    return out


def topk_full(full, row_tags, probe_masks, k, index_base=0):
    """-> (idx [n, k] int64, dist [n, k] float32)."""
    return topk_ref.topk_full(masked(full, row_tags, probe_masks), k, index_base)


def topk_ids_full(full, labels, row_tags, probe_masks, k, exclude=None, index_base=0):
    """-> (idx, dist, label), each [n, k]."""
    return topk_ids_ref.topk_ids_full(masked(full, row_tags, probe_masks), labels, k, exclude, index_base)


def case_tags(G):
    """The GPU tests' row tags for a gallery of G rows: bit 0 on half the rows, bit 1 on an eighth, bit 2 on 1/128, bit 63 on
    half, bit 3 never; some rows end with tag 0."""
    u = np.random.default_rng(7 + G).random((G, 4))
    t = (u[:, 0] < .5).astype(np.uint64) | ((u[:, 1] < .125).astype(np.uint64) << np.uint64(1)) \
        | ((u[:, 2] < 1 / 128).astype(np.uint64) << np.uint64(2)) | ((u[:, 3] < .5).astype(np.uint64) << np.uint64(63))
    t = t.view(np.int64).copy()
    t.setflags(write=False)
    return t


def case_masks(B):
    m = MASK_CYCLE[np.arange(B) % len(MASK_CYCLE)].copy()
    m.setflags(write=False)
    return m
