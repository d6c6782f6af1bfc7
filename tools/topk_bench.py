"""Times the top-k list (Gallery.topk at k = 1, 10, 128) next to the top-1 match on the f32 filter (Gallery.match, "filter" = 0 --
the same f32 MFMA main loop over the same rows) and the rank of a genuine mate (Gallery.rank), with HIP events, and writes
profiles/topk_bench.json.

    python tools/topk_bench.py [--out profiles/topk_bench.json] [--shape all|big|small] [--repeats 5] [--iters N]

tools/rank_bench.py's protocol: shapes 512 probes x 1 M rows x 512-d and 1 probe x 100 k rows x 512-d, metric 1; gallery of
identities of four near-duplicate rows (centre + 0.05 noise), probes drawn the same way; the calls timed in alternation,
`repeats` windows of `iters` calls each after a warm-up of the same calls; median / min / max per call.  The gallery option
"topk_seed" is left at its default unless --seed is given.  Under
`rocprofv3 --kernel-trace --stats -- python tools/topk_bench.py --shape big --repeats 1 --iters 3` the per-kernel split
(topk_tilemin_kernel / topk_select_kernel) comes from the profiler."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
from deep_insight_face import oneshot  # noqa: E402

D = 512
KS = (1, 10, 128)


def make(G, B, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    nid = max(1, G // 4)
    centres = torch.randn(nid, D, device='cuda', generator=gen)
    gal = centres[torch.arange(G, device='cuda') % nid] + 0.05 * torch.randn(G, D, device='cuda', generator=gen)
    pick = torch.randint(0, nid, (B,), device='cuda', generator=gen)
    probes = centres[pick] + 0.05 * torch.randn(B, D, device='cuda', generator=gen)
    genuine = pick + nid * torch.randint(0, 4, (B,), device='cuda', generator=gen)      # one of the identity's four rows
    return probes.contiguous(), gal.contiguous(), genuine.contiguous()


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


def run_shape(B, G, repeats, iters, seed_option):
    probes, gal_rows, genuine = make(G, B, seed=G + B)
    gal = oneshot.Gallery(gal_rows)
    del gal_rows
    gal.set_option('filter', 0)
    if seed_option:
        gal.set_option('topk_seed', seed_option)
    rank = torch.empty(B, dtype=torch.int64, device='cuda')
    mdist = torch.empty(B, dtype=torch.float32, device='cuda')
    mi = torch.empty(B, dtype=torch.int64, device='cuda')
    md = torch.empty(B, dtype=torch.float32, device='cuda')
    lists = {k: (torch.empty((B, k), dtype=torch.int64, device='cuda'), torch.empty((B, k), dtype=torch.float32, device='cuda'))
             for k in KS}
    calls = {
        'match_filter0': lambda: gal.match_into(probes, 1, mi, md),
        'rank_genuine': lambda: gal.rank_into(probes, genuine, 1, rank, mdist),
    }
    for k in KS:
        calls['topk_%d' % k] = (lambda k=k: gal.topk_into(probes, k, 1, lists[k][0], lists[k][1]))
    for name, fn in calls.items():                                   # warm-up: every shape the timed windows use
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    agree = {k: bool((lists[k][0][:, 0] == mi).all()) for k in KS}    # the head of every list is the arg-min
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():                               # alternated: drifts of clock and neighbours hit all calls
            times[name].append(window(fn, iters))
    gal.close()
    out = {'probes': B, 'rows': G, 'd': D, 'metric': 1, 'topk_seed': seed_option, 'iters_per_window': iters, 'windows': repeats,
           'head_is_argmin': agree}
    for name in calls:
        out[name] = stats(times[name])
        if name != 'match_filter0':
            out[name]['ratio_to_match_filter0'] = out[name]['median_ms'] / out['match_filter0']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'topk_bench.json'))
    ap.add_argument('--shape', default='all', choices=('all', 'big', 'small'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=0, help='calls per window (default: 10 at 1 M rows, 200 at 100 k)')
    ap.add_argument('--seed', type=int, default=0, help='gallery option "topk_seed" (0: the default, k tiles)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'topk_bench needs a HIP device'
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
