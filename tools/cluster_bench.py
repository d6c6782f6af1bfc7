"""Times Gallery.cluster (connected components of the gallery's own rows under a tolerance, one call) next to the loop a user
had to write without it -- Gallery.within over the whole gallery in blocks of 512 probes, device time only, the host
union-find that loop still needs NOT counted -- with HIP events, and writes profiles/cluster_bench.json.

    python tools/cluster_bench.py [--out profiles/cluster_bench.json] [--rows 100000] [--big] [--repeats 5]

Workload: 512-d, metric 1, identities of four near-duplicate rows (centre + 0.05 noise, tools/within_bench.py's gallery),
tolerance 0.2: a row's own identity.  One process, a warm-up of both calls, then `repeats` windows of one call each, the two
calls in alternation; median / min / max.  --big adds 1 M rows as a single window.  Under
`rocprofv3 --kernel-trace --stats -- python tools/cluster_bench.py --repeats 1` the per-kernel split (within_census_kernel /
cluster_resolve_kernel / within_resolve_kernel) comes from the profiler."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
from deep_insight_face import oneshot  # noqa: E402

D, K, BLOCK, T = 512, 64, 512, 0.2


def make(G, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    nid = max(1, G // 4)
    centres = torch.randn(nid, D, device='cuda', generator=gen)
    gal = centres[torch.arange(G, device='cuda') % nid] + 0.05 * torch.randn(G, D, device='cuda', generator=gen)
    return gal.contiguous()


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    v = sorted(v)
    return {'median_ms': v[len(v) // 2], 'min_ms': v[0], 'max_ms': v[-1]}


def run_shape(G, repeats, warmup):
    rows = make(G, seed=G)
    gal = oneshot.Gallery(rows)
    labels = torch.empty(G, dtype=torch.int64, device='cuda')
    n = torch.empty((), dtype=torch.int64, device='cuda')
    count = torch.empty(BLOCK, dtype=torch.int64, device='cuda')
    idx = torch.empty((BLOCK, K), dtype=torch.int64, device='cuda')
    dist = torch.empty((BLOCK, K), dtype=torch.float32, device='cuda')
    hits = torch.zeros((), dtype=torch.int64, device='cuda')

    def within_loop():
        hits.zero_()
        for b0 in range(0, G, BLOCK):
            nb = min(BLOCK, G - b0)
            gal.within_into(rows[b0:b0 + nb], T, 1, count[:nb], idx[:nb], dist[:nb])
            hits.add_(count[:nb].sum())

    calls = {'cluster': lambda: gal.cluster_into(T, 1, labels, n), 'within_loop': within_loop}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():                               # alternated: drifts of clock and neighbours hit both
            times[name].append(window(fn))
    out = {'rows': G, 'd': D, 'metric': 1, 'tolerance': T, 'windows': repeats, 'warmup_calls': warmup,
           'n_clusters': int(n), 'identities': max(1, G // 4), 'within_block': BLOCK, 'within_max_hits': K,
           'within_hits_per_row': float(hits) / G}
    for name in calls:
        out[name] = stats(times[name])
    out['ratio_cluster_to_within_loop'] = out['cluster']['median_ms'] / out['within_loop']['median_ms']
    gal.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cluster_bench.json'))
    ap.add_argument('--rows', type=int, default=100_000)
    ap.add_argument('--big', action='store_true', help='add 1 M rows, one window after one warm-up call')
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'cluster_bench needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'shapes': [run_shape(a.rows, a.repeats, 2)]}
    print(json.dumps(res['shapes'][-1]), flush=True)
    if a.big:
        res['shapes'].append(run_shape(1_000_000, 1, 1))
        print(json.dumps(res['shapes'][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
