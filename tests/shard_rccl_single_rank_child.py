"""Child process of tests/test_shard_queries_gpu.py::test_rccl_single_rank_all_queries.

Started fresh (no GPU call before the process group exists), it initialises torch.distributed with backend "nccl" -- RCCL on
ROCm -- for a world of ONE rank bound to cuda:0 and runs ShardedGallery.topk, topk_ids, within, rank and roc with
force_collectives=True: the gathers of the probes and the per-probe arrays, the local queries, the gather of the packed
records, the merges on the device.  The results go to an .npz beside the plain Gallery's for the parent to compare.

    python shard_rccl_single_rank_child.py <port> <out.npz>
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, 'deep-insight-face_amd'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


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
        import shard_inputs as si
        from deep_insight_face import oneshot
        from deep_insight_face.parallel import ShardedGallery
        B, G = 37, 1001
        c = si.case(B, G, 128)
        mates = si.mates([(0, G)], G, B)
        res = {'backend': np.array(dist.get_backend()), 'world': np.array(dist.get_world_size())}
        sg = ShardedGallery(torch.from_numpy(c.gal.copy()).to(dev), 0, force_collectives=True)
        res['forced'] = np.array(not sg._local())
        plain = oneshot.Gallery(c.gal.copy())
        p_t = torch.from_numpy(c.probes.copy()).to(dev)
        for metric in (0, 1):
            for k, v in si.five_queries(sg, p_t, c, 0, G, 0, metric, mates).items():
                res['sharded_%s%d' % (k, metric)] = v
            for k, v in si.five_queries(plain, p_t, c, 0, G, 0, metric, mates).items():
                res['plain_%s%d' % (k, metric)] = v
        try:                                                      # 1 rank x 10923 probes x 8192 hits x 12 bytes > 2^30
            sg.within(torch.zeros((10923, 128), device=dev), 0.5, 1, max_hits=8192)
            res['refused'] = np.array(False)
        except ValueError as e:
            res['refused'] = np.array('lower max_hits' in str(e))
        torch.cuda.synchronize()
        np.savez(out_path, **res)
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
