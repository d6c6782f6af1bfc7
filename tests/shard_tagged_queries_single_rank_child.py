"""Child process of tests/test_shard_tagged_queries_gpu.py::test_rccl_single_rank_tagged_queries.

Started fresh (no GPU call before the process group exists), it initialises torch.distributed with backend "nccl" -- RCCL on
ROCm -- for a world of ONE rank bound to cuda:0 and runs ShardedGallery.within and rank with row_tags and probe_masks and
force_collectives=True: the gathers of the probes, the mates and the masks, the local tagged queries (the rank through
mate_dist_into and rank_at_into), the gathers of the records, the merges on the device.  The results go to an .npz beside the
plain Gallery's for the parent to compare.

    python shard_tagged_queries_single_rank_child.py <port> <out.npz>
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, 'deep-insight-face_amd'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def queries(q, probes, mates, tags, masks, metric, t):
    """The same signatures serve parallel.ShardedGallery and oneshot.Gallery.  -> {name: array}."""
    import shard_inputs as si
    res = {}
    res['w_c'], res['w_i'], res['w_d'] = si.to_numpy(q.within(probes, t, metric, 8, row_tags=tags, probe_masks=masks))
    res['int_c'], res['int_i'], res['int_d'] = si.to_numpy(q.within(probes, t, metric, 64, row_tags=tags, probe_masks=6))
    res['rank_r'], res['rank_d'] = si.to_numpy(q.rank(probes, mates, metric, row_tags=tags, probe_masks=masks))
    res['int_r'], res['int_m'] = si.to_numpy(q.rank(probes, mates, metric, row_tags=tags.numpy(), probe_masks=-1))
    return res


def main():
    port, out_path = sys.argv[1], sys.argv[2]
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = port
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import numpy as np
    import torch
    import torch.distributed as dist
    dev = torch.device('cuda', 0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)      # before any other GPU call
    try:
        torch.cuda.set_device(dev)
        import rank_ref
        import shard_inputs as si
        import tagged_ref
        from deep_insight_face import oneshot
        from deep_insight_face.parallel import ShardedGallery
        B, G = 37, 1001
        c = si.case(B, G, 128)
        tags = torch.from_numpy(np.array(tagged_ref.case_tags(G)))             # the shard's tags from the host ...
        masks = torch.from_numpy(np.array(tagged_ref.case_masks(B))).to(dev)    # ... this rank's masks on the device
        mates = torch.from_numpy(np.array(si.mates([(0, G)], G, B))).to(dev)
        res = {'backend': np.array(dist.get_backend()), 'world': np.array(dist.get_world_size())}
        sg = ShardedGallery(torch.from_numpy(c.gal.copy()).to(dev), 0, force_collectives=True)
        res['forced'] = np.array(not sg._local())
        plain = oneshot.Gallery(c.gal.copy())
        p_t = torch.from_numpy(c.probes.copy()).to(dev)
        for metric in (0, 1):
            t = float(np.median(rank_ref.distances(c.probes, c.gal, metric)))
            for k, v in queries(sg, p_t, mates, tags, masks, metric, t).items():
                res['sharded_%s%d' % (k, metric)] = v
            for k, v in queries(plain, p_t, mates, tags, masks, metric, t).items():
                res['plain_%s%d' % (k, metric)] = v
        for name, call in (('one_given_within', lambda: sg.within(p_t, 0.5, 1, 8, row_tags=tags)),
                           ('one_given_rank', lambda: sg.rank(p_t, mates, 1, probe_masks=masks)),
                           ('float_masks', lambda: sg.within(p_t, 0.5, 1, 8, tags, masks.float()))):
            try:                                                  # refused on every rank alike, before any collective
                call()
                res[name] = np.array(False)
            except ValueError:
                res[name] = np.array(True)
        torch.cuda.synchronize()
        np.savez(out_path, **res)
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
