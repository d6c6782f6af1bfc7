"""Times Gallery.dbscan (density clustering with noise, two sweeps of the lower triangle) next to Gallery.cluster (one sweep, the
same census and the same reference arithmetic) on the same rows in the same process, with HIP events, and writes
profiles/dbscan_bench.json.

    python tools/dbscan_bench.py [--out profiles/dbscan_bench.json] [--rows 100000] [--big] [--repeats 5]

Workload: 512-d, metric 1, identities of four near-duplicate rows (centre + 0.05 noise, tools/cluster_bench.py's gallery) plus
10 % isolated rows (a centre of their own), tolerance 0.2, min_samples 3: the identities are clusters of four core rows, the
isolated rows are noise.  One process, a warm-up of both calls, then `repeats` windows of one call each, the two calls in
alternation; median / min / max.  --big adds 1 M rows as a single window.  Under
`rocprofv3 --kernel-trace --stats -- python tools/dbscan_bench.py --repeats 1` the per-kernel split (within_census_kernel /
dbscan_degree_kernel / dbscan_link_kernel / cluster_resolve_kernel) comes from the profiler."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
from deep_insight_face import oneshot  # noqa: E402

D, T, MIN_SAMPLES = 512, 0.2, 3


def make(G, seed):
    """-> (rows [G, D], isolated rows): 10 % of the rows are their own centre, the rest identities of four; shuffled."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    lone = G // 10
    nid = max(1, (G - lone) // 4)
    centres = torch.randn(nid + lone, D, device='cuda', generator=gen)
    owner = torch.cat([torch.arange(G - lone, device='cuda') % nid, nid + torch.arange(lone, device='cuda')])
    gal = centres[owner] + 0.05 * torch.randn(G, D, device='cuda', generator=gen)
    return gal[torch.randperm(G, device='cuda', generator=gen)].contiguous(), lone


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
    rows, lone = make(G, seed=G)
    gal = oneshot.Gallery(rows)
    labels = torch.empty(G, dtype=torch.int64, device='cuda')
    degree = torch.empty(G, dtype=torch.int32, device='cuda')
    counts = torch.empty(2, dtype=torch.int64, device='cuda')
    cl_labels = torch.empty(G, dtype=torch.int64, device='cuda')
    n = torch.empty((), dtype=torch.int64, device='cuda')
    calls = {'dbscan': lambda: gal.dbscan_into(T, MIN_SAMPLES, 1, labels, degree, counts),
             'cluster': lambda: gal.cluster_into(T, 1, cl_labels, n)}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():                               # alternated: drifts of clock and neighbours hit both
            times[name].append(window(fn))
    out = {'rows': G, 'd': D, 'metric': 1, 'tolerance': T, 'min_samples': MIN_SAMPLES, 'windows': repeats, 'warmup_calls': warmup,
           'isolated_rows': lone, 'identities': max(1, (G - lone) // 4), 'clusters': int(counts[0]), 'noise_rows': int(counts[1]),
           'core_rows': int((degree >= MIN_SAMPLES).sum()), 'mean_degree': float(degree.double().mean()),
           'cluster_n_clusters': int(n)}
    for name in calls:
        out[name] = stats(times[name])
    out['ratio_dbscan_to_cluster'] = out['dbscan']['median_ms'] / out['cluster']['median_ms']
    gal.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dbscan_bench.json'))
    ap.add_argument('--rows', type=int, default=100_000)
    ap.add_argument('--big', action='store_true', help='add 1 M rows, one window after one warm-up call')
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'dbscan_bench needs a HIP device'
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
