"""The tagged top-k searches over a sharded gallery against ONE oneshot.Gallery holding all the rows and all the tags
(tests/test_shard_queries_gpu.py's pattern).

In-process form: the rows and their tags split over 3 Gallery handles of unequal size with their index_base on one device,
every handle queried with all the probes and all the masks, the results stacked [3, ...] and merged on the device by
parallel.merge_topk / merge_topk_ids: the outcome equals the whole-gallery handle's BIT FOR BIT on both metrics -- a row among
the k nearest eligible rows of all shards is among the k nearest eligible rows of its own shard -- and, on metric 0, the NumPy
statement (tests/tagged_ref.py).  Then parallel.ShardedGallery's own methods on one rank over RCCL with force_collectives: the
gathers of the probes and their masks, the local tagged queries, the merges."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rank_ref
import shard_inputs as si
import tagged_ref
from test_shard_queries_gpu import _free_port, _raw, _ref, _t

pytestmark = pytest.mark.gpu
KS = (1, 5, 128)
BOUNDS = {1001: [(0, 130), (130, 131), (131, 1001)], 3001: [(0, 1500), (1500, 1629), (1629, 3001)]}   # 130 + 1 + 870; 1500 + 129 + 1372


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

    def topk(self, p, k, metric, tags, masks):
        from deep_insight_face import parallel
        parts = [g.topk(p, k, metric, _t(tags[lo:hi]), masks) for g, (lo, hi) in zip(self.shards, self.bounds)]
        return parallel.merge_topk(torch.stack([a[0] for a in parts]), torch.stack([a[1] for a in parts]))

    def topk_ids(self, p, k, labels, metric, exclude, tags, masks):
        from deep_insight_face import parallel
        parts = [g.topk_ids(p, k, _t(labels[lo:hi]), metric, exclude, _t(tags[lo:hi]), masks)
                 for g, (lo, hi) in zip(self.shards, self.bounds)]
        return parallel.merge_topk_ids(*[torch.stack([a[i] for a in parts]) for i in range(3)])


@pytest.mark.parametrize('G,B', [(1001, 37), (3001, 130)])
def test_three_unequal_shards(cuda, G, B):
    """Shards of 130, 1 and 870 rows, and of 1500, 129 and 1372: tile tails in every shard, a shard of one row.  The copied
    rows 0, 1 and G - 1 (shard_inputs.case) lie in the first and the last shard; of rows 0 and 1 only the second is eligible
    for the probes with mask 1, so the head of probe 0's list is [1, G - 1] -- a tie across two shards."""
    c = si.case(B, G, 128)
    tags = np.array(tagged_ref.case_tags(G))
    tags[[0, 1, 2, 3, G - 1]] = [2, 1, 4, 1, 1]
    masks = np.array(tagged_ref.case_masks(B))
    h = Shards(c.gal, BOUNDS[G])
    p, m_dev, t_dev = _t(c.probes), _t(masks), _t(tags)
    for metric in (0, 1):
        full = rank_ref.distances(c.probes, c.gal, metric) if metric == 0 else None
        for k in KS:
            got = h.topk(p, k, metric, tags, m_dev)
            _raw(got, h.whole.topk(p, k, metric, t_dev, m_dev))
            if metric == 0:
                _ref(got, tagged_ref.topk_full(full, tags, masks, k))
            for labels in (c.labels, c.labels_same):
                for exclude in (None, labels[c.pick]):
                    ex = None if exclude is None else _t(exclude)
                    got = h.topk_ids(p, k, labels, metric, ex, tags, m_dev)
                    _raw(got, h.whole.topk_ids(p, k, _t(labels), metric, ex, t_dev, m_dev))
                    if metric == 0:
                        _ref(got, tagged_ref.topk_ids_full(full, labels, tags, masks, k, exclude))
        idx = h.topk(p, 5, metric, tags, m_dev)[0].cpu().numpy()
        assert masks[0] == 1 and idx[0, :2].tolist() == [1, G - 1]
        one = h.topk(p, 5, metric, tags, -1)                                    # a Python int for every probe, on every shard
        _raw(one, h.whole.topk(p, 5, metric, t_dev, -1))
    h.close()


def test_rccl_single_rank_tagged(cuda, tmp_path):
    """ShardedGallery.topk / topk_ids with row_tags and probe_masks through the whole gather-and-merge branch: a FRESH child
    process (tests/shard_tagged_single_rank_child.py) initialises backend "nccl" with a world of one before any other GPU
    call and runs them with force_collectives=True beside the plain Gallery's calls; and the argument errors."""
    out = os.path.join(str(tmp_path), 'tagged.npz')
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'shard_tagged_single_rank_child.py')
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    r = subprocess.run([sys.executable, child, str(_free_port()), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)
    assert str(z['backend']) == 'nccl' and int(z['world']) == 1 and bool(z['forced'])
    assert bool(z['one_given_topk']) and bool(z['one_given_ids']) and bool(z['float_masks'])
    names = sorted(k[len('plain_'):] for k in z.files if k.startswith('plain_'))
    assert len(names) == 2 * 10
    for k in names:
        _raw((z['sharded_' + k],), (z['plain_' + k],))
    assert (z['plain_int_i0'][:, :5] != z['plain_topk_i0']).any()                     # the masks matter
