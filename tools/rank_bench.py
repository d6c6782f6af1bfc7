"""Times the rank of the mate (Gallery.rank) next to the top-1 match on the f32 filter (Gallery.match, "filter" = 0 -- the same
f32 MFMA main loop over the same rows) and the sparse range search (Gallery.within), with HIP events, and writes
profiles/rank_bench.json.

    python tools/rank_bench.py [--out profiles/rank_bench.json] [--shape all|big|small] [--repeats 5] [--iters N]

Shapes: 512 probes x 1 M rows x 512-d and 1 probe x 100 k rows x 512-d, metric 1.  Gallery: identities of four near-duplicate
rows (centre + 0.05 noise), probes drawn the same way.  Two kinds of mate: GENUINE (a row of the probe's own identity: a
handful of rows are closer, the band around the mate's distance is almost empty) and RANDOM (any row: half the gallery is
closer, and every tile with a row too close to the mate's distance to call is resolved on the reference arithmetic).  The
four calls are timed in alternation, `repeats` windows of `iters` calls each after a warm-up of the same calls; median / min /
max per call.  Under `rocprofv3 --kernel-trace --stats -- python tools/rank_bench.py --shape big --repeats 1 --iters 3` the
per-kernel split (rank_prep_kernel / within_census_kernel / rank_resolve_kernel) comes from the profiler."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
from deep_insight_face import oneshot  # noqa: E402

D, K = 512, 64


def make(G, B, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    nid = max(1, G // 4)
    centres = torch.randn(nid, D, device='cuda', generator=gen)
    gal = centres[torch.arange(G, device='cuda') % nid] + 0.05 * torch.randn(G, D, device='cuda', generator=gen)
    pick = torch.randint(0, nid, (B,), device='cuda', generator=gen)
    probes = centres[pick] + 0.05 * torch.randn(B, D, device='cuda', generator=gen)
    genuine = pick + nid * torch.randint(0, 4, (B,), device='cuda', generator=gen)      # one of the identity's four rows
    random = torch.randint(0, G, (B,), device='cuda', generator=gen)
    return probes.contiguous(), gal.contiguous(), genuine.contiguous(), random.contiguous()


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def stats(v):
    v = sorted(v)
    return {'median_ms': v[len(v) // 2], 'min_ms': v[0], 'max_ms': v[-1]}


def run_shape(B, G, repeats, iters):
    probes, gal_rows, genuine, random = make(G, B, seed=G + B)
    gal = oneshot.Gallery(gal_rows)
    del gal_rows
    gal.set_option('filter', 0)
    rank = torch.empty(B, dtype=torch.int64, device='cuda')
    mdist = torch.empty(B, dtype=torch.float32, device='cuda')
    count = torch.empty(B, dtype=torch.int64, device='cuda')
    idx = torch.empty((B, K), dtype=torch.int64, device='cuda')
    dist = torch.empty((B, K), dtype=torch.float32, device='cuda')
    mi = torch.empty(B, dtype=torch.int64, device='cuda')
    md = torch.empty(B, dtype=torch.float32, device='cuda')
    calls = {
        'match_filter0': lambda: gal.match_into(probes, 1, mi, md),
        'within_sparse': lambda: gal.within_into(probes, 0.2, 1, count, idx, dist),
        'rank_genuine': lambda: gal.rank_into(probes, genuine, 1, rank, mdist),
        'rank_random': lambda: gal.rank_into(probes, random, 1, rank, mdist),
    }
    ranks = {}
    for name, fn in calls.items():                                   # warm-up: every shape the timed windows use
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if name.startswith('rank_'):
            ranks[name] = {'mean': float(rank.double().mean()), 'min': int(rank.min()), 'max': int(rank.max()),
                           'mean_mate_dist': float(mdist.double().mean())}
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():                               # alternated: drifts of clock and neighbours hit all four
            times[name].append(window(fn, iters))
    gal.close()
    out = {'probes': B, 'rows': G, 'd': D, 'metric': 1, 'within_tolerance': 0.2, 'within_max_hits': K,
           'iters_per_window': iters, 'windows': repeats, 'rank_of_mate': ranks}
    for name in calls:
        out[name] = stats(times[name])
    for name in ('within_sparse', 'rank_genuine', 'rank_random'):
        out[name]['ratio_to_match_filter0'] = out[name]['median_ms'] / out['match_filter0']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rank_bench.json'))
    ap.add_argument('--shape', default='all', choices=('all', 'big', 'small'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=0, help='calls per window (default: 20 at 1 M rows, 500 at 100 k)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'rank_bench needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'shapes': []}
    if a.shape in ('all', 'big'):
        res['shapes'].append(run_shape(512, 1_000_000, a.repeats, a.iters or 20))
    if a.shape in ('all', 'small'):
        res['shapes'].append(run_shape(1, 100_000, a.repeats, a.iters or 500))
    for s in res['shapes']:
        print(json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
