"""The sharded gallery's other queries -- topk, topk_ids, within, rank, roc -- against ONE oneshot.Gallery holding all the rows.

In-process form: R Gallery handles with their index_base on one device (parallel.shard_bounds: ragged, and empty where there are
fewer rows than ranks), every handle queried with all the probes, the results stacked [R, ...] and merged on the device by
parallel.merge_topk / merge_topk_ids / merge_within / merge_rank (roc's int64 counts are summed).  The outcome must equal the
whole-gallery handle's BIT FOR BIT -- indices, counts, labels and the bit patterns of the distances, NaN padding included -- on
both metrics; on metric 0, where the library is bit-identical to the reference, also the NumPy statements (tests/topk_ref.py,
topk_ids_ref.py, rank_ref.py, roc_ref.py, shard_merge_ref.within_full), NaN taken as one value.  Then the two local entries of
the sharded rank directly, the argument errors, two ranks over gloo on one GPU and one rank over RCCL with force_collectives,
both through parallel.ShardedGallery's methods."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import golden_inputs as gi
import rank_ref
import roc_ref
import shard_inputs as si
import shard_merge_ref as sm
import topk_ids_ref
import topk_ref

pytestmark = pytest.mark.gpu

# (total rows, ranks, probes, embedding size): every total over every R; shards of 0 rows (5 over 8), of 1 row, of 125 .. 129
# rows around the 128-row census tile (257 / 2, 1001 / 8) and ragged ones; B of 1, 37 and 130 (one probe block and two)
_B = {5: {1: 1, 2: 37, 3: 130, 8: 1}, 257: {1: 37, 2: 130, 3: 1, 8: 37}, 1001: {1: 130, 2: 1, 3: 37, 8: 130},
      3001: {1: 1, 2: 37, 3: 130, 8: 37}}
CASES = [(G, R, _B[G][R], 128) for G in (5, 257, 1001, 3001) for R in (1, 2, 3, 8)] + [(257, 3, 37, 512)]
KS = (1, 5, 128)


_np = si.to_numpy


def _t(a):
    return torch.from_numpy(np.array(a)).cuda()                 # (a copy: the cached inputs are read-only)


def _raw(got, want):
    """Bit for bit: integers equal, float32 equal as bit patterns (the padding's NaN included)."""
    got, want = _np(got), _np(want)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (i, g.dtype, w.dtype, g.shape, w.shape)
        a, b = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        assert np.array_equal(a, b), (i, np.argwhere(a != b)[:8], g[a != b][:8], w[a != b][:8])


def _ref(got, want):
    """Against NumPy: integers equal, float32 bit for bit with every NaN taken as one value."""
    got, want = _np(got), _np(want)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (i, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            assert np.array_equal(np.isnan(g), np.isnan(w)), (i, np.argwhere(np.isnan(g) != np.isnan(w))[:8])
            g, w = g[~np.isnan(g)].view(np.uint32), w[~np.isnan(w)].view(np.uint32)
        assert np.array_equal(g, w), (i, np.argwhere(g != w)[:8])


@functools.lru_cache(maxsize=None)
def _full(B, G, D, metric):
    c = si.case(B, G, D)
    full = rank_ref.distances(c.probes, c.gal, metric)
    full.setflags(write=False)
    return full


class Handles:
    """The whole-gallery handle and the R shard handles of one gallery, and every query the sharded way."""

    def __init__(self, gal, R, clamp=0):
        from deep_insight_face import oneshot
        from deep_insight_face.parallel import shard_bounds
        gal = np.array(gal)                                      # (a copy: the cached inputs are read-only)
        G, D = gal.shape
        self.R, self.G = R, G
        self.bounds = [shard_bounds(G, R, r) for r in range(R)]
        assert self.bounds[0][0] == 0 and self.bounds[-1][1] == G
        self.whole = oneshot.Gallery(gal)
        self.shards = []
        for lo, hi in self.bounds:
            g = oneshot.Gallery(emd_size=D)
            g.set(gal[lo:hi], lo)                                # (an empty shard too: index_base is kept)
            assert len(g) == hi - lo
            self.shards.append(g)
        for g in [self.whole] + self.shards:
            g.set_option('clamp_nan', clamp)

    def close(self):
        for g in [self.whole] + self.shards:
            g.close()

    def topk(self, p, k, metric):
        from deep_insight_face import parallel
        parts = [g.topk(p, k, metric) for g in self.shards]
        return parallel.merge_topk(torch.stack([a[0] for a in parts]), torch.stack([a[1] for a in parts]))

    def topk_ids(self, p, k, labels, metric, exclude=None):
        from deep_insight_face import parallel
        parts = [g.topk_ids(p, k, _t(labels[lo:hi]), metric, exclude) for g, (lo, hi) in zip(self.shards, self.bounds)]
        return parallel.merge_topk_ids(*[torch.stack([a[i] for a in parts]) for i in range(3)])

    def within(self, p, tolerance, metric, max_hits):
        from deep_insight_face import parallel
        parts = [g.within(p, tolerance, metric, max_hits) for g in self.shards]
        return parallel.merge_within(*[torch.stack([a[i] for a in parts]) for i in range(3)])

    def rank_parts(self, p, m, metric):
        """-> (count [R, B], owned [R, B], mate_dist [R, B], dm [B]) as ShardedGallery.rank forms them."""
        from deep_insight_face import parallel
        B = p.shape[0]
        md = torch.empty((self.R, B), dtype=torch.float32, device='cuda')
        own = torch.empty((self.R, B), dtype=torch.int64, device='cuda')
        cnt = torch.empty((self.R, B), dtype=torch.int64, device='cuda')
        for r, g in enumerate(self.shards):
            g.mate_dist_into(p, m, metric, md[r], own[r])
        _, dm = parallel.merge_rank(torch.zeros_like(own), own, md)
        for r, g in enumerate(self.shards):
            g.rank_at_into(p, m, dm, metric, cnt[r])
        return cnt, own, md, dm

    def rank(self, p, m, metric):
        from deep_insight_face import parallel
        cnt, own, md, _ = self.rank_parts(p, m, metric)
        return parallel.merge_rank(cnt, own, md)

    def roc(self, p, probe_labels, labels, thresholds, metric, first_row=None):
        parts = [g.roc(p, probe_labels, _t(labels[lo:hi]), thresholds, metric, first_row)
                 for g, (lo, hi) in zip(self.shards, self.bounds)]
        return torch.stack([a[0] for a in parts]).sum(0), torch.stack([a[1] for a in parts]).sum(0)


# ------------------------------------------------------------------------------------------- the five queries, every case
@pytest.mark.parametrize('G,R,B,D', CASES)
def test_topk(cuda, G, R, B, D):
    """k = 1, 5 and 128: above a shard's size the shard lists carry padding, above the total (G = 5) the merged list does.
    Probes 0 .. 2 are noisy copies of the copied rows: their lists start with exact ties within and across shards, which go to
    the lower global row."""
    c = si.case(B, G, D)
    h = Handles(c.gal, R)
    p = _t(c.probes)
    for metric in (0, 1):
        for k in KS:
            got = h.topk(p, k, metric)
            _raw(got, h.whole.topk(p, k, metric))
            if metric == 0:
                _ref(got, topk_ref.topk_full(_full(B, G, D, 0), k))
    idx = h.topk(p, 5, 0)[0].cpu().numpy()
    assert idx[0, :3].tolist() == [0, 1, G - 1]                                 # the tripled row, ties in index order
    if B >= 3:
        assert idx[1, :2].tolist() == [2, 3] and idx[2, :3].tolist() == [0, 1, G - 1]
    h.close()


@pytest.mark.parametrize('G,R,B,D', CASES)
def test_topk_ids(cuda, G, R, B, D):
    """Identities with rows in several shards, identity 0 in every shard, negative labels; the copied rows under one label and
    under labels of their own; the probe's identity excluded or not; all-distinct labels give merge_topk's lists."""
    c = si.case(B, G, D)
    h = Handles(c.gal, R)
    p = _t(c.probes)
    for metric in (0, 1):
        for name in ('labels', 'labels_same', 'labels_diff'):
            labels = getattr(c, name)
            for exclude in (None, labels[c.pick]):
                ex = None if exclude is None else _t(exclude)
                for k in KS:
                    got = h.topk_ids(p, k, labels, metric, ex)
                    _raw(got, h.whole.topk_ids(p, k, _t(labels), metric, ex))
                    if metric == 0:
                        _ref(got, topk_ids_ref.topk_ids_full(_full(B, G, D, 0), labels, k, exclude))
        distinct = np.arange(G, dtype=np.int64)[::-1].copy()
        for k in KS:
            got = h.topk_ids(p, k, distinct, metric)
            _raw(got[:2], h.topk(p, k, metric))
    lab = h.topk_ids(p, 5, c.labels_same, 0)[2].cpu().numpy()
    assert lab[0, 0] == 0 and (lab[0, 1:] != 0).all()                            # the three copies are one entry
    lab = h.topk_ids(p, 5, c.labels_diff, 0)
    assert lab[0][0, :3].tolist() == [0, 1, G - 1] and lab[2][0, :3].tolist() == [c.nid + 1, c.nid + 2, c.nid + 3]
    h.close()


def _tolerances(full):
    """From the oracle's distances of probe 0: below every distance (zero hits), its third smallest (a few hits), its 100th
    smallest or its largest (more than 64 hits where there are that many rows; more than 4 always) -- and the extremes."""
    row = np.sort(full[0][~np.isnan(full[0])])
    return [np.float32(row[0] / 2), row[min(2, row.size - 1)], row[min(99, row.size - 1)], np.float32(-1.0), np.float32(np.inf)]


@pytest.mark.parametrize('G,R,B,D', CASES)
def test_within(cuda, G, R, B, D):
    c = si.case(B, G, D)
    h = Handles(c.gal, R)
    p = _t(c.probes)
    for metric in (0, 1):
        full = _full(B, G, D, metric)
        tols = _tolerances(full)
        if metric == 0:
            hits = [int((full[0] <= t).sum()) for t in tols[:3]]
            assert hits[0] == 0 and hits[1] >= 3 and hits[2] > 4 and (G < 100 or hits[2] > 64), hits
        for t in tols:
            for K in (0, 4, 64):
                got = h.within(p, t, metric, K)
                _raw(got, h.whole.within(p, t, metric, K))
                if metric == 0:
                    _ref(got, sm.within_full(full, t, K))
    cnt, idx, _ = _np(h.within(p, _tolerances(_full(B, G, D, 0))[1], 0, 4))
    assert cnt[0] >= 3 and idx[0, :2].tolist() == [0, 1]                         # the lowest global rows first
    h.close()


@pytest.mark.parametrize('G,R,B,D', CASES)
def test_rank(cuda, G, R, B, D):
    """Mates in the first, a middle and the last shard, in the first and last row of a shard, the copied rows (ties count by
    the global row, across shards), -1 and beyond the total (unmated)."""
    c = si.case(B, G, D)
    h = Handles(c.gal, R)
    p = _t(c.probes)
    for seed in (0, 1):
        mates = si.mates(h.bounds, G, B, seed) if seed == 0 else np.roll(si.mates(h.bounds, G, max(B, 16), 1), 5)[:B]
        m = _t(mates)
        for metric in (0, 1):
            got = h.rank(p, m, metric)
            _raw(got, h.whole.rank(p, m, metric))
            if metric == 0:
                _ref(got, rank_ref.rank_full(_full(B, G, D, 0), mates))
    rank, md = _np(h.rank(p[:1], _t(np.array([G - 1])), 0))                      # probe 0 is a copy of rows 0, 1, G - 1
    assert rank.tolist() == [2] and md[0] == _full(B, G, D, 0)[0, 0]
    h.close()


@functools.lru_cache(maxsize=None)
def _self_full(B, G, D, n):
    c = si.case(B, G, D)
    return rank_ref.distances(c.gal[:n], c.gal, 0)


@pytest.mark.parametrize('T', [1, 7, 1024])
@pytest.mark.parametrize('G,R,B,D', CASES)
def test_roc(cuda, G, R, B, D, T):
    """A labelled set against itself (the first rows of the gallery as probes, first_row = own row + 1: every unordered pair
    once), split over the shards, negative labels among them; then the case's probes against all rows."""
    c = si.case(B, G, D)
    h = Handles(c.gal, R)
    n = min(G, 130)
    own = np.arange(n, dtype=np.int64) + 1
    for metric in (0, 1):
        hi = 1.0 if metric == 1 else 2.5 * D
        thr = {1: np.array([hi / 3]), 7: np.linspace(-0.1, hi, 7), 1024: np.linspace(0.0, hi, 1024)}[T]
        for probes, pl, fr in ((c.gal[:n], c.labels[:n], own), (c.probes, c.labels[c.pick], None)):
            frt = None if fr is None else _t(fr)
            got = h.roc(_t(probes), _t(pl), c.labels, thr, metric, frt)
            _raw(got, h.whole.roc(_t(probes), _t(pl), _t(c.labels), thr, metric, frt))
            if metric == 0:
                full = _self_full(B, G, D, n) if fr is not None else _full(B, G, D, 0)
                _ref(got, roc_ref.counts_full(full, pl, c.labels, thr, fr))
    h.close()


# ------------------------------------------------------------------------------------------- planted fixtures
def test_near_ties(cuda):
    """Rows one ulp, 1e-7 and 1e-4 apart and exact duplicates at shuffled positions (tests/test_topk_gpu.py::
    test_topk_near_ties), over three shards: the merged lists are the stable argsort's, and the sharded rank of the j-th listed
    row is j at the listed distance."""
    probes, gal = gi.match_near_tie_inputs(b=16, g=1024)
    h = Handles(gal, 3)
    p = _t(probes)
    labels = (np.arange(1024) % 300).astype(np.int64)
    for metric in (0, 1):
        for k in (5, 128):
            got = h.topk(p, k, metric)
            _raw(got, h.whole.topk(p, k, metric))
            _raw(h.topk_ids(p, k, labels, metric), h.whole.topk_ids(p, k, _t(labels), metric))
        ti, td = h.topk(p, 5, metric)
        for j in range(5):
            rank, md = h.rank(p, ti[:, j].contiguous(), metric)
            assert (rank == j).all()
            _raw((md,), (td[:, j].contiguous(),))
        t = float(td[:, 4].max())
        _raw(h.within(p, t, metric, 64), h.whole.within(p, t, metric, 64))
    full = rank_ref.distances(probes, gal, 0)
    assert not np.isnan(full).any()
    order = np.argsort(full, axis=1, kind='stable')[:, :5]
    _ref(h.topk(p, 5, 0), (order.astype(np.int64), np.take_along_axis(full, order, axis=1)))
    _ref(h.topk_ids(p, 5, labels, 0), topk_ids_ref.topk_ids_full(full, labels, 5))
    h.close()


@functools.lru_cache(maxsize=None)
def _degenerate(name):
    probes, gal = [(p, g) for n, p, g in gi.match_degenerate_cases() if n == name][0]
    return probes[:24], topk_ref.small_gallery(probes, gal)      # 126 rows, up to half of them the fixture's odd rows


@pytest.mark.parametrize('clamp', [0, 1])
@pytest.mark.parametrize('name', [c[0] for c in gi.match_degenerate_cases()])
def test_degenerate(cuda, name, clamp):
    """The rows tests/golden/match_degenerate.npz was recorded on -- zero-norm, tiny, huge and non-finite rows and probes,
    similarities that round beyond +-1 -- spread over 3 and over 8 shards, under clamp_nan 0 and 1: a NaN distance is never
    listed and never a hit in any shard, and a mate whose own distance is NaN ranks at the TOTAL size, the sum of the shards'."""
    probes, gal = _degenerate(name)
    G, B = gal.shape[0], probes.shape[0]
    full0 = rank_ref.distances(probes, gal, 0)
    labels = (np.arange(G) % 40).astype(np.int64)
    labels[5::9] = -2
    mates = (np.arange(B) * 5 % G).astype(np.int64)
    p, m = _t(probes), _t(mates)
    for R in (3, 8):
        h = Handles(gal, R, clamp)
        for metric in (0, 1):
            for k in (1, 128):
                got = h.topk(p, k, metric)
                _raw(got, h.whole.topk(p, k, metric))
                ids = h.topk_ids(p, k, labels, metric)
                _raw(ids, h.whole.topk_ids(p, k, _t(labels), metric))
                if metric == 0:
                    _ref(got, topk_ref.topk_full(full0, k))
                    _ref(ids, topk_ids_ref.topk_ids_full(full0, labels, k))
            for t in ((0.5, 1.0) if metric == 1 else (1.0, np.inf)):
                for K in (0, 64):
                    got = h.within(p, t, metric, K)
                    _raw(got, h.whole.within(p, t, metric, K))
                    if metric == 0:
                        _ref(got, sm.within_full(full0, t, K))
            got = h.rank(p, m, metric)
            want = h.whole.rank(p, m, metric)
            _raw(got, want)
            rank, md = _np(want)
            assert (rank[np.isnan(md)] == G).all()                               # the NaN mate: behind every row of every shard
            if metric == 0:
                _ref(got, rank_ref.rank_full(full0, mates))
            thr = np.linspace(0.0, 1.0 if metric == 1 else 4.0, 7)
            got = h.roc(p, _t(labels[mates]), labels, thr, metric)
            _raw(got, h.whole.roc(p, _t(labels[mates]), _t(labels), thr, metric))
            if metric == 0:
                _ref(got, roc_ref.counts_full(full0, labels[mates], labels, thr))
        h.close()


# ------------------------------------------------------------------------------------------- the two local entries of rank
@pytest.mark.parametrize('G,R,B', [(257, 2, 37), (1001, 8, 130), (5, 8, 37)])
def test_rank_at_direct(cuda, G, R, B):
    """dif_match_mate_dist and dif_match_rank_at shard by shard against the NumPy count; the counts of the shards add up to
    dif_match_rank over the whole gallery; and dif_match_rank on a handle that has served rank_at calls -- they share the
    census, its thresholds and the mate record -- still equals its reference."""
    D = 128
    c = si.case(B, G, D)
    h = Handles(c.gal, R)
    p = _t(c.probes)
    mates = si.mates(h.bounds, G, B)
    m = _t(mates)
    full = _full(B, G, D, 0)
    for metric in (0, 1):
        cnt, own, md, dm = h.rank_parts(p, m, metric)
        want_rank, want_md = h.whole.rank(p, m, metric)
        mated = (mates >= 0) & (mates < G)
        assert np.array_equal(own.sum(0).cpu().numpy(), mated.astype(np.int64))  # exactly one owner, or none
        _raw((dm,), (want_md,))
        assert torch.equal(cnt.sum(0)[_t(mated)], want_rank[_t(mated)])
        if metric == 0:
            for r, (lo, hi) in enumerate(h.bounds):
                want = sm.mate_dist_full(full[:, lo:hi], mates, lo)
                _ref((md[r], own[r]), want)
                _ref((cnt[r],), (sm.rank_at_full(full[:, lo:hi], mates, dm.cpu().numpy(), lo),))
    # a mate's distance the shard never computed: any float, a NaN and an infinity among them; mates of -1 are legal here
    dm = full[np.arange(B), (np.arange(B) * 7) % G].copy()
    dm[::5] = np.nan
    dm[1::5] = np.inf
    far = np.where(np.arange(B) % 2 == 0, -1, mates).astype(np.int64)
    for r, (g, (lo, hi)) in enumerate(zip(h.shards, h.bounds)):
        cnt = torch.empty((B,), dtype=torch.int64, device='cuda')
        g.rank_at_into(p, _t(far), _t(dm), 0, cnt)
        _ref((cnt,), (sm.rank_at_full(full[:, lo:hi], far, dm, lo),))
        assert (cnt.cpu().numpy()[np.isnan(dm)] == hi - lo).all()
    # the whole handle: rank, rank_at, rank again
    cnt = torch.empty((B,), dtype=torch.int64, device='cuda')
    for metric in (0, 1):
        first = h.whole.rank(p, m, metric)
        h.whole.rank_at_into(p, _t(far), _t(dm), metric, cnt)
        again = h.whole.rank(p, m, metric)
        _raw(again, first)
        if metric == 0:
            _ref((cnt,), (sm.rank_at_full(full, far, dm, 0),))
            _ref(again, rank_ref.rank_full(full, mates))
    h.close()


# ------------------------------------------------------------------------------------------- rounds of probes in every shard
def test_forced_rounds_in_every_shard(cuda):
    """Every shard is queried with the gathered probes of all ranks, so the shards are where the round loops of within_run,
    rank_run, topk_run and topk_ids_run are met first.  300 probes over three shards of 1001 rows with "within_round" and
    "topk_round" at 128 on every shard (128 + 128 + 44 probes): the merged rank -- dif_match_rank_at in rounds, its mates
    global, owned by other shards or by none, its `dm` handed in per probe --, top-k, identities and range search equal the
    whole handle's one-round answers and the shards' own one-round answers bit for bit, and NumPy on metric 0.  Before the
    device is asked: the oracle on the mates a dropped `+ b0` would read differs in both later rounds."""
    B, G, R, D = 300, 1001, 3, 128
    c = si.case(B, G, D)
    h = Handles(c.gal, R)
    assert all(lo > 0 for lo, _ in h.bounds[1:])                                 # index_base != 0
    p = _t(c.probes)
    mates = si.mates(h.bounds, G, B)
    owner = np.array([next((r for r, (lo, hi) in enumerate(h.bounds) if lo <= m < hi), -1) for m in mates])
    assert all((owner == r).sum() >= 32 for r in range(R)) and (owner == -1).sum() >= 3
    m = _t(mates)
    labels, exclude = c.labels, c.labels[c.pick]
    ex = _t(exclude)
    want_r, want_d = rank_ref.rank_full(_full(B, G, D, 0), mates)
    wrong_r, wrong_d = rank_ref.rank_full(_full(B, G, D, 0), mates[np.arange(B) % 128])
    for b0 in (128, 256):
        assert ((wrong_r != want_r) | (wrong_d.view(np.uint32) != want_d.view(np.uint32)))[b0:b0 + 128].any()

    def queries(metric):
        full = _full(B, G, D, metric)
        tols = _tolerances(full)
        out = {'rank': h.rank(p, m, metric)}
        for k in (5, 128):
            out['topk %d' % k] = h.topk(p, k, metric)
            out['ids %d' % k] = h.topk_ids(p, k, labels, metric, ex)
        for K in (4, 0):
            out['within %d' % K] = h.within(p, tols[2], metric, K)
        return out, tols

    for metric in (0, 1):
        base, tols = queries(metric)
        for g in h.shards:
            g.set_option('within_round', 128)
            g.set_option('topk_round', 128)
        forced, _ = queries(metric)
        for g in h.shards:
            g.set_option('within_round', 0)
            g.set_option('topk_round', 0)
        again, _ = queries(metric)
        whole = {'rank': h.whole.rank(p, m, metric)}
        for k in (5, 128):
            whole['topk %d' % k] = h.whole.topk(p, k, metric)
            whole['ids %d' % k] = h.whole.topk_ids(p, k, _t(labels), metric, ex)
        for K in (4, 0):
            whole['within %d' % K] = h.whole.within(p, tols[2], metric, K)
        for name in whole:
            _raw(forced[name], whole[name])
            _raw(forced[name], base[name])
            _raw(again[name], base[name])
        if metric == 0:
            full = _full(B, G, D, 0)
            _ref(forced['rank'], (want_r, want_d))
            for k in (5, 128):
                _ref(forced['topk %d' % k], topk_ref.topk_full(full, k))
                _ref(forced['ids %d' % k], topk_ids_ref.topk_ids_full(full, labels, k, exclude))
            for K in (4, 0):
                _ref(forced['within %d' % K], sm.within_full(full, tols[2], K))
    h.close()


# ------------------------------------------------------------------------------------------- argument errors
def test_argument_errors(cuda):
    """Every one returns an error (ValueError from the wrappers, a non-zero code from the library) and launches nothing."""
    from deep_insight_face import _native as N
    from deep_insight_face import oneshot, parallel
    i3 = torch.full((2, 3, 4), -1, dtype=torch.int64, device='cuda')
    d3 = torch.full((2, 3, 4), float('nan'), dtype=torch.float32, device='cuda')
    c2 = torch.zeros((2, 3), dtype=torch.int64, device='cuda')
    f2 = torch.zeros((2, 3), dtype=torch.float32, device='cuda')
    assert [tuple(t.shape) for t in parallel.merge_topk(i3, d3)] == [(3, 4), (3, 4)]
    # R outside [1, 64]

    def ints(*shape):
        return torch.full(shape, -1, dtype=torch.int64, device='cuda')

    def flts(*shape):
        return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')

    for R in (0, 65):
        with pytest.raises(ValueError, match=r'outside \[1, 64\]'):
            parallel.merge_topk(ints(R, 3, 4), flts(R, 3, 4))
        with pytest.raises(ValueError, match=r'outside \[1, 64\]'):
            parallel.merge_topk_ids(ints(R, 3, 4), flts(R, 3, 4), ints(R, 3, 4))
        with pytest.raises(ValueError, match=r'outside \[1, 64\]'):
            parallel.merge_within(ints(R, 3), ints(R, 3, 4), flts(R, 3, 4))
        with pytest.raises(ValueError, match=r'outside \[1, 64\]'):
            parallel.merge_rank(ints(R, 3), ints(R, 3) + 1, flts(R, 3))
    ok = parallel.merge_rank(ints(64, 3), ints(64, 3) + 1, flts(64, 3))      # 64 itself is fine: nobody owns the mate
    assert ok[0].tolist() == [-1, -1, -1]
    # k outside [1, 128], max_hits outside [0, 8192]
    for k in (0, 129):
        with pytest.raises(ValueError, match=r'outside \[1, 128\]'):
            parallel.merge_topk(ints(2, 3, k), flts(2, 3, k))
        with pytest.raises(ValueError, match=r'outside \[1, 128\]'):
            parallel.merge_topk_ids(ints(2, 3, k), flts(2, 3, k), ints(2, 3, k))
    with pytest.raises(ValueError, match=r'outside \[0, 8192\]'):
        parallel.merge_within(c2, ints(2, 3, 8193), flts(2, 3, 8193))
    assert N.lib.dif_shard_merge_within(N.ptr(c2), None, None, 2, 3, -1, N.ptr(c2), None, None, N.stream_ptr()) != 0
    # shapes, dtypes and devices the wrappers refuse
    for bad in ((i3, d3[:, :, :2].contiguous()), (i3.int(), d3), (i3, d3.double()), (i3.cpu(), d3.cpu()), (i3[0], d3[0]),
                (i3.transpose(1, 2), d3.transpose(1, 2))):
        with pytest.raises(ValueError):
            parallel.merge_topk(*bad)
    with pytest.raises(ValueError):
        parallel.merge_within(c2[:, :2].contiguous(), i3, d3)
    with pytest.raises(ValueError):
        parallel.merge_rank(c2, c2, f2[:1])
    # null pointers
    s = N.stream_ptr()
    one = N.ptr(i3)
    assert N.lib.dif_shard_merge_topk(None, N.ptr(d3), 2, 3, 4, one, N.ptr(d3), s) != 0 and 'null pointer' in N.last_error()
    assert N.lib.dif_shard_merge_topk(one, N.ptr(d3), 2, 3, 4, None, N.ptr(d3), s) != 0
    assert N.lib.dif_shard_merge_topk_ids(one, N.ptr(d3), None, 2, 3, 4, one, N.ptr(d3), one, s) != 0
    assert N.lib.dif_shard_merge_within(None, one, N.ptr(d3), 2, 3, 4, N.ptr(c2), one, N.ptr(d3), s) != 0
    assert N.lib.dif_shard_merge_within(N.ptr(c2), one, None, 2, 3, 4, N.ptr(c2), one, N.ptr(d3), s) != 0
    assert N.lib.dif_shard_merge_rank(N.ptr(c2), None, N.ptr(f2), 2, 3, N.ptr(c2), N.ptr(f2), s) != 0
    assert N.lib.dif_shard_merge_rank(N.ptr(c2), N.ptr(c2), N.ptr(f2), 2, 3, None, N.ptr(f2), s) != 0
    assert N.lib.dif_shard_merge_rank(N.ptr(c2), N.ptr(c2), N.ptr(f2), 2, -1, N.ptr(c2), N.ptr(f2), s) != 0
    g = oneshot.Gallery(np.array(si.case(37, 257, 128).gal))
    assert N.lib.dif_match_mate_dist(g._h, None, 3, 0, N.ptr(c2), N.ptr(f2), N.ptr(c2), s) != 0
    assert N.lib.dif_match_mate_dist(g._h, N.ptr(f2), 3, 2, N.ptr(c2), N.ptr(f2), N.ptr(c2), s) != 0      # the metric
    assert N.lib.dif_match_rank_at(g._h, N.ptr(f2), 3, 0, N.ptr(c2), None, N.ptr(c2), s) != 0
    assert N.lib.dif_match_rank_at(g._h, N.ptr(f2), -1, 0, N.ptr(c2), N.ptr(f2), N.ptr(c2), s) != 0
    p = torch.zeros((3, 128), device='cuda')
    with pytest.raises(ValueError):
        g.rank_at_into(p, c2[0], f2[0].double(), 0, c2[1])
    with pytest.raises(ValueError):
        g.mate_dist_into(p, c2[0, :2], 0, f2[0], c2[1])
    with pytest.raises(RuntimeError, match='Undefined distance metric'):
        g.rank_at_into(p, c2[0], f2[0], 2, c2[1])
    # n = 0 and K = 0
    e = parallel.merge_topk(i3[:, :0].contiguous(), d3[:, :0].contiguous())
    assert tuple(e[0].shape) == (0, 4)
    cnt, ei, ed = parallel.merge_within(c2 + 2, i3[:, :, :0].contiguous(), d3[:, :, :0].contiguous())
    assert cnt.tolist() == [4, 4, 4] and tuple(ei.shape) == (3, 0)
    # the size refusal of ShardedGallery.within: 2 ranks x 2 * 2731 probes x 8192 hits x 12 bytes > 2^30, refused before the
    # first collective or allocation (the world is made up: nothing is gathered)
    sg = parallel.ShardedGallery(None, 0, gallery=g, check_batch='never')
    sg.world = 2
    assert parallel.within_gather_bytes(2, 2731, 8192) > 2 ** 30 >= parallel.within_gather_bytes(2, 2730, 8192)
    with pytest.raises(ValueError, match='lower max_hits'):
        sg.within(torch.zeros((2731, 128), device='cuda'), 0.5, 1, max_hits=8192)
    with pytest.raises(ValueError, match='outside'):
        parallel.ShardedGallery(None, 0, gallery=g).within(p, 0.5, 1, max_hits=8193)
    g.close()


# ------------------------------------------------------------------------------------------- two ranks over gloo, one over RCCL
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _CpuCollectives:
    """all_gather_into_tensor for CUDA tensors over gloo: stage through the host."""

    def __init__(self):
        self._orig = dist.all_gather_into_tensor

    def __call__(self, out, inp, group=None):
        o = torch.empty(out.shape, dtype=out.dtype)
        self._orig(o, inp.cpu(), group=group)
        out.copy_(o)


def _worker(rank, world, port, G, b, out_dir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dist.all_gather_into_tensor = _CpuCollectives()
        from deep_insight_face.parallel import ShardedGallery, shard_bounds
        c = si.case(world * b, G, 128)
        bounds = [shard_bounds(G, world, r) for r in range(world)]
        lo, hi = bounds[rank]
        sg = ShardedGallery(torch.from_numpy(c.gal[lo:hi].copy()).cuda(), lo)
        mates = si.mates(bounds, G, world * b)
        res = {}
        for metric in (0, 1):
            mine = torch.from_numpy(c.probes[rank * b:(rank + 1) * b].copy()).cuda()
            for k, v in si.five_queries(sg, mine, c, lo, hi, rank * b, metric, mates).items():
                res['%s%d' % (k, metric)] = v
        try:                                                      # the size refusal, on every rank alike, before any collective
            sg.within(torch.zeros((2731, 128), device='cuda'), 0.5, 1, max_hits=8192)
            res['refused'] = np.array(False)
        except ValueError as e:
            res['refused'] = np.array('lower max_hits' in str(e))
        np.savez(os.path.join(out_dir, 'r%d.npz' % rank), **res)
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_gpu_all_queries(cuda, tmp_path):
    """ShardedGallery.topk, topk_ids, within, rank and roc on two ranks that share the one GPU (gloo carries
    all_gather_into_tensor, as in tests/test_parallel_gpu.py), ragged shards of 3001 rows, 37 probes per rank: both ranks'
    results equal each other and the whole-gallery handle's, bit for bit.  One spawn: with this process three have the GPU open."""
    from deep_insight_face import oneshot
    from deep_insight_face.parallel import shard_bounds
    world, G, b = 2, 3001, 37
    mp.spawn(_worker, args=(world, _free_port(), G, b, str(tmp_path)), nprocs=world, join=True)
    c = si.case(world * b, G, 128)
    mates = si.mates([shard_bounds(G, world, r) for r in range(world)], G, world * b)
    whole = oneshot.Gallery(np.array(c.gal))
    z = [np.load(os.path.join(str(tmp_path), 'r%d.npz' % r)) for r in range(world)]
    assert bool(z[0]['refused']) and bool(z[1]['refused'])
    for metric in (0, 1):
        want = si.five_queries(whole, torch.from_numpy(c.probes.copy()).cuda(), c, 0, G, 0, metric, mates)
        for k, v in want.items():
            for r in range(world):
                _raw((z[r]['%s%d' % (k, metric)],), (v,))
    whole.close()


def test_rccl_single_rank_all_queries(cuda, tmp_path):
    """RCCL itself carries the gathers of the five methods: a FRESH child process (tests/shard_rccl_single_rank_child.py)
    initialises backend "nccl" with a world of one before any other GPU call and runs them with force_collectives=True -- the
    whole gather-and-merge branch -- beside the plain Gallery's calls."""
    out = os.path.join(str(tmp_path), 'rccl.npz')
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'shard_rccl_single_rank_child.py')
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    r = subprocess.run([sys.executable, child, str(_free_port()), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)
    assert str(z['backend']) == 'nccl' and int(z['world']) == 1 and bool(z['forced']) and bool(z['refused'])
    names = sorted(k[len('plain_'):] for k in z.files if k.startswith('plain_'))
    assert len(names) == 2 * 16
    for k in names:
        _raw((z['sharded_' + k],), (z['plain_' + k],))
