"""Times the identity-level top-k list (Gallery.topk_ids at k = 1, 10, 128, with and without the probe's own identity excluded)
next to the row-level list at the same k (Gallery.topk, whose kernels the identity-level entry point leaves untouched: the
yardstick of the same run), with HIP events, and writes profiles/topk_ids_bench.json.

    python tools/topk_ids_bench.py [--out profiles/topk_ids_bench.json] [--shape all|big|small] [--repeats 5] [--iters N]

tools/topk_bench.py's protocol: shapes 512 probes x 1 M rows x 512-d and 1 probe x 100 k rows x 512-d, metric 1; gallery of
identities of four near-duplicate rows (centre + 0.05 noise, label = row % (rows // 4)), probes drawn the same way; the calls
timed in alternation, `repeats` windows of `iters` calls each after a warm-up of the same calls; median / min / max per call.
After the windows every topk_ids form is called once more and `stat('topk_ids_tiles')` per probe is recorded.  Under
`rocprofv3 --kernel-trace --stats -- python tools/topk_ids_bench.py --shape big --repeats 1 --iters 3` the per-kernel split
(topk_tilemin_kernel / topk_select_kernel / topk_ids_select_kernel) comes from the profiler."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deep_insight_face import oneshot  # noqa: E402
from topk_bench import D, KS, make, stats, window  # noqa: E402


def run_shape(B, G, repeats, iters, seed_option):
    probes, gal_rows, genuine = make(G, B, seed=G + B)
    nid = max(1, G // 4)
    labels = (torch.arange(G, device='cuda') % nid).contiguous()
    own = (genuine % nid).contiguous()                                # the probe's identity
    gal = oneshot.Gallery(gal_rows)
    del gal_rows
    if seed_option:
        gal.set_option('topk_seed', seed_option)
    out_i = {k: torch.empty((B, k), dtype=torch.int64, device='cuda') for k in KS}
    out_d = {k: torch.empty((B, k), dtype=torch.float32, device='cuda') for k in KS}
    out_l = {k: torch.empty((B, k), dtype=torch.int64, device='cuda') for k in KS}
    calls = {}
    for k in KS:
        calls['topk_%d' % k] = (lambda k=k: gal.topk_into(probes, k, 1, out_i[k], out_d[k]))
        calls['topk_ids_%d' % k] = (lambda k=k: gal.topk_ids_into(probes, k, 1, labels, None, out_i[k], out_d[k], out_l[k]))
        calls['topk_ids_excl_%d' % k] = (lambda k=k: gal.topk_ids_into(probes, k, 1, labels, own, out_i[k], out_d[k], out_l[k]))
    for name, fn in calls.items():                                   # warm-up: every shape the timed windows use
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():                               # alternated: drifts of clock and neighbours hit all calls
            times[name].append(window(fn, iters))
    out = {'probes': B, 'rows': G, 'd': D, 'metric': 1, 'rows_per_identity': 4, 'topk_seed': seed_option,
           'iters_per_window': iters, 'windows': repeats, 'tiles_per_probe_of': (G + 127) // 128}
    for name, fn in calls.items():
        out[name] = stats(times[name])
        if name.startswith('topk_ids'):
            k = int(name.rsplit('_', 1)[1])
            base = out['topk_%d' % k]
            out[name]['ratio_to_topk_same_k'] = out[name]['median_ms'] / base['median_ms']
            out[name]['beyond_the_windows_spread'] = bool(out[name]['min_ms'] > base['max_ms'])
            fn()
            out[name]['tiles_per_probe'] = gal.stat('topk_ids_tiles') / B
            if 'excl' in name:
                out[name]['own_identity_listed'] = bool((out_l[k] == own[:, None]).any())
            else:
                out[name]['head_is_own_identity'] = float((out_l[k][:, 0] == own).float().mean())
    gal.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'topk_ids_bench.json'))
    ap.add_argument('--shape', default='all', choices=('all', 'big', 'small'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=0, help='calls per window (default: 10 at 1 M rows, 200 at 100 k)')
    ap.add_argument('--seed', type=int, default=0, help='gallery option "topk_seed" (0: the default, k tiles)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'topk_ids_bench needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'shapes': []}
    if a.shape in ('all', 'big'):
        res['shapes'].append(run_shape(512, 1_000_000, a.repeats, a.iters or 10, a.seed))
    if a.shape in ('all', 'small'):
        res['shapes'].append(run_shape(1, 100_000, a.repeats, a.iters or 200, a.seed))
    for s in res['shapes']:
        print(json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
