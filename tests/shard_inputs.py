"""Seeded inputs of the sharded-gallery tests (tests/test_shard_queries_gpu.py, its two-rank workers and its RCCL child): a
gallery of identities with four near-duplicate rows each, exact copies planted so that they fall into different shards and twice
into one shard, labels whose identities span the shards, probes that are near-copies of enrolled rows -- the copied ones first,
so exact ties stand at the head of the lists.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(B, G, D, seed=0):
    """Rows 0, 1 and G - 1 are one row three times (rows 0 and 1 share every shard of at least two rows; row G - 1 is in the last
    shard that holds rows), rows 2 and 3 one row twice.  labels: identity i % nid, so every identity has rows G // nid apart
    (several shards); identity 0 is also given every 16th row (a label present in every shard of 16 rows or more); negative
    labels (rows taken out) at every 13th row from 7.  labels_same / labels_diff: the copies under one label / under labels of
    their own.  probes[b] is a noisy copy of row pick[b]; pick starts 0, 2, G - 1."""
    assert G >= 5
    rng = np.random.default_rng(1000 * G + 10 * B + D + seed)
    nid = max(1, G // 4)
    centres = rng.standard_normal((nid, D))
    gal = (centres[np.arange(G) % nid] + 0.05 * rng.standard_normal((G, D))).astype(np.float32)
    gal[1] = gal[0]
    gal[G - 1] = gal[0]
    gal[3] = gal[2]
    labels = (np.arange(G) % nid).astype(np.int64)
    labels[::16] = 0
    labels[7::13] = -1 - (np.arange(len(labels[7::13])) % 3)
    same, diff = labels.copy(), labels.copy()
    same[[0, 1, G - 1]] = 0
    same[[2, 3]] = 2 % nid
    diff[[0, 1, G - 1, 2, 3]] = nid + 1 + np.arange(5)
    pick = rng.integers(0, G, B)
    pick[:3] = np.array([0, 2, G - 1])[:min(B, 3)]
    probes = (gal[pick] + 0.05 * rng.standard_normal((B, D))).astype(np.float32)
    c = Case()
    c.B, c.G, c.D, c.nid = B, G, D, nid
    c.gal, c.probes, c.pick, c.labels, c.labels_same, c.labels_diff = gal, probes, pick.astype(np.int64), labels, same, diff
    for a in (c.gal, c.probes, c.pick, c.labels, c.labels_same, c.labels_diff):
        a.setflags(write=False)
    return c


def mates(bounds, G, B, seed=0):
    """[B] int64 global mate indices that visit every position relative to a shard: the first and last row of the first,
    a middle and the last shard that holds rows, the copied rows, -1, a row beyond the total (G, and far beyond), then random
    rows.  B = 1 gets the first only: the tripled row 1, whose tie with row 0 crosses no shard but with row G - 1 does."""
    held = [(lo, hi) for lo, hi in bounds if hi > lo]
    pos = [1, G - 1, 0, 2, 3, -1, G, G + 10 ** 12]
    for lo, hi in (held[0], held[len(held) // 2], held[-1]):
        pos += [lo, hi - 1]
    rng = np.random.default_rng(G + seed)
    m = np.concatenate([np.array(pos, dtype=np.int64), rng.integers(0, G, max(0, B - len(pos)))])
    return m[:B].astype(np.int64)


def to_numpy(ts):
    return tuple(t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t) for t in ts)


ROC_THRESHOLDS = np.linspace(0.0, 1.0, 7)


def five_queries(q, probes, c, lo, hi, first, metric, all_mates):
    """topk, topk_ids (with and without an excluded identity), within (lists and counts alone), rank and roc on `q` -- a
    parallel.ShardedGallery holding rows [lo, hi) of case `c`, or a oneshot.Gallery holding all of them (lo, hi = 0, G) -- for
    the probes [first, first + len(probes)) of the case: the same signatures serve both.  -> {name: array}."""
    res = {}
    sl = slice(first, first + probes.shape[0])
    pl, ex = c.labels[c.pick][sl].copy(), c.labels_same[c.pick][sl].copy()
    res['topk_i'], res['topk_d'] = to_numpy(q.topk(probes, 5, metric))
    res['ids_i'], res['ids_d'], res['ids_l'] = to_numpy(q.topk_ids(probes, 5, c.labels_same[lo:hi].copy(), metric, ex))
    res['nox_i'], res['nox_d'], res['nox_l'] = to_numpy(q.topk_ids(probes, 128, c.labels[lo:hi].copy(), metric))
    res['within_c'], res['within_i'], res['within_d'] = to_numpy(q.within(probes, 0.3 if metric == 1 else 20.0, metric, 4))
    res['count_c'] = to_numpy(q.within(probes, 0.45 if metric == 1 else 200.0, metric, 0))[0]
    res['rank_r'], res['rank_d'] = to_numpy(q.rank(probes, all_mates[sl].copy(), metric))
    res['roc_a'], res['roc_t'] = to_numpy(q.roc(probes, pl, c.labels[lo:hi].copy(),
                                                ROC_THRESHOLDS * (1.0 if metric == 1 else 300.0), metric,
                                                first_row=c.pick[sl] + 1))
    return res
