"""The tagged range search and rank over a sharded gallery against ONE oneshot.Gallery holding all the rows and all the tags
(tests/test_shard_tagged_gpu.py's pattern).

In-process form: the rows and their tags split over 3 Gallery handles of unequal size with their index_base on one device,
every handle queried with all the probes and all the masks -- the rank through its two shard-local halves, mate_dist_into and
rank_at_into, both tagged --, the results stacked [3, ...] and merged on the device by parallel.merge_within / merge_rank,
unchanged: counts over the eligible rows of disjoint shards add, the K lowest eligible hits of all shards are among each
shard's K lowest, and the owning shard reports owned = 1 with a NaN distance for a mate the probe may not see.  The outcome
equals the whole-gallery handle's BIT FOR BIT on both metrics and, on metric 0, the NumPy statement
(tests/tagged_queries_ref.py), the two halves per shard included.  Then parallel.ShardedGallery's own methods on one rank over
RCCL with force_collectives."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rank_ref
import shard_inputs as si
import tagged_queries_ref as tq
import tagged_ref
from test_shard_queries_gpu import _free_port, _raw, _ref, _t
from test_shard_tagged_gpu import BOUNDS

pytestmark = pytest.mark.gpu


class Shards:
    def __init__(self, gal, bounds):
        from deep_insight_face import oneshot
        gal = np.array(gal)
        self.bounds = bounds
        self.whole = oneshot.Gallery(gal)
        self.shards = [oneshot.Gallery(gal[lo:hi], index_base=lo) for lo, hi in bounds]

    def close(self):
        for g in [self.whole] + self.shards:
            g.close()

    def within(self, p, t, metric, K, tags, masks):
        from deep_insight_face import parallel
        parts = [g.within(p, t, metric, K, _t(tags[lo:hi]), masks) for g, (lo, hi) in zip(self.shards, self.bounds)]
        return parallel.merge_within(*[torch.stack([a[i] for a in parts]) for i in range(3)])

    def rank_parts(self, p, m, metric, tags, masks):
        """-> (count [R, B], owned [R, B], mate_dist [R, B], dm [B]) as ShardedGallery.rank forms them."""
        from deep_insight_face import parallel
        R, B = len(self.shards), p.shape[0]
        md = torch.empty((R, B), dtype=torch.float32, device='cuda')
        own = torch.empty((R, B), dtype=torch.int64, device='cuda')
        cnt = torch.empty((R, B), dtype=torch.int64, device='cuda')
        for r, (g, (lo, hi)) in enumerate(zip(self.shards, self.bounds)):
            g.mate_dist_into(p, m, metric, md[r], own[r], _t(tags[lo:hi]), masks)
        _, dm = parallel.merge_rank(torch.zeros_like(own), own, md)
        for r, (g, (lo, hi)) in enumerate(zip(self.shards, self.bounds)):
            g.rank_at_into(p, m, dm, metric, cnt[r], _t(tags[lo:hi]), masks)
        return cnt, own, md, dm


@pytest.mark.parametrize('G,B', [(1001, 37), (3001, 130)])
def test_three_unequal_shards(cuda, G, B):
    """Shards of 130, 1 and 870 rows, and of 1500, 129 and 1372: tile tails in every shard, a shard of one row.  Rows 0, 1 and
    G - 1 are one row three times (shard_inputs.case): of rows 0 and 1 only the second is eligible for the probes with mask 1,
    so with row G - 1 as the mate one tie counts, from another shard."""
    from deep_insight_face import parallel
    c = si.case(B, G, 128)
    tags = np.array(tagged_ref.case_tags(G))
    tags[[0, 1, 2, 3, G - 1]] = [2, 1, 4, 1, 1]
    masks = np.array(tagged_ref.case_masks(B))
    el = tagged_ref.eligible(tags, masks)
    mates = np.array(si.mates(BOUNDS[G], G, B))
    mates[0] = G - 1
    seen = np.array([0 <= m < G and el[b, m] for b, m in enumerate(mates)])
    assert seen.sum() >= B // 8 and ((mates >= 0) & (mates < G) & ~seen).sum() >= B // 8
    h = Shards(c.gal, BOUNDS[G])
    p, m_dev, t_dev, mt = _t(c.probes), _t(masks), _t(tags), _t(mates)
    for metric in (0, 1):
        full = rank_ref.distances(c.probes, c.gal, metric)
        t = np.float32(np.median(full))
        for K in (0, 8, 64):
            got = h.within(p, t, metric, K, tags, m_dev)
            _raw(got, h.whole.within(p, t, metric, K, t_dev, m_dev))
            if metric == 0:
                _ref(got, tq.within_full(full, tags, masks, t, K))
        cnt, own, md, dm = h.rank_parts(p, mt, metric, tags, m_dev)
        want = h.whole.rank(p, mt, metric, t_dev, m_dev)
        _raw(parallel.merge_rank(cnt, own, md), want)
        assert np.array_equal(own.sum(0).cpu().numpy(), ((mates >= 0) & (mates < G)).astype(np.int64))   # owned whatever the tag
        rank = want[0].cpu().numpy()
        real = seen & ~np.isnan(full[np.arange(B), np.clip(mates, 0, G - 1)])  # (metric 1: a probe equal to its mate may be NaN)
        assert (rank[(mates >= 0) & (mates < G) & ~seen] == G).all() and (rank[real] < G).all()
        assert masks[0] == 1 and (rank[0] == 1 or not real[0])                  # row 1 ties from below, row 0 is not the probe's
        assert metric == 1 or real[0]
        if metric == 0:
            _ref(want, tq.rank_full(full, mates, tags, masks))
            for r, (lo, hi) in enumerate(h.bounds):
                _ref((md[r], own[r]), tq.mate_dist_full(full[:, lo:hi], mates, tags[lo:hi], masks, lo))
                _ref((cnt[r],), (tq.rank_at_full(full[:, lo:hi], mates, dm.cpu().numpy(), tags[lo:hi], masks, lo),))
        one = h.within(p, t, metric, 8, tags, -1)                               # a Python int for every probe, on every shard
        _raw(one, h.whole.within(p, t, metric, 8, t_dev, -1))
    h.close()


def test_rccl_single_rank_tagged_queries(cuda, tmp_path):
    """ShardedGallery.within / rank with row_tags and probe_masks through the whole gather-and-merge branch: a FRESH child
    process (tests/shard_tagged_queries_single_rank_child.py) initialises backend "nccl" with a world of one before any other
    GPU call and runs them with force_collectives=True beside the plain Gallery's calls; and the argument errors."""
    out = os.path.join(str(tmp_path), 'tagged_queries.npz')
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'shard_tagged_queries_single_rank_child.py')
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    r = subprocess.run([sys.executable, child, str(_free_port()), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)
    assert str(z['backend']) == 'nccl' and int(z['world']) == 1 and bool(z['forced'])
    assert bool(z['one_given_within']) and bool(z['one_given_rank']) and bool(z['float_masks'])
    names = sorted(k[len('plain_'):] for k in z.files if k.startswith('plain_'))
    assert len(names) == 2 * 10
    for k in names:
        _raw((z['sharded_' + k],), (z['plain_' + k],))
    assert (z['plain_w_c0'] != z['plain_int_c0']).any() and (z['plain_rank_r0'] != z['plain_int_r0']).any()   # the masks matter
