"""Times the tagged top-k list (Gallery.topk with row_tags and probe_masks, k = 10) with every row, an eighth and 1/128 of the
rows eligible, next to the untagged Gallery.topk -- untouched by the tagged entry points, so it stands for the library before
them -- and the untagged and tagged Gallery.topk_ids, with HIP events, and writes profiles/topk_tagged_bench.json.

    python tools/topk_tagged_bench.py [--out profiles/topk_tagged_bench.json] [--shape all|big|small] [--repeats 5] [--iters N]

tools/topk_bench.py's protocol: shapes 512 probes x 1 M rows x 512-d and 1 probe x 100 k rows x 512-d, metric 1; gallery of
identities of four near-duplicate rows (centre + 0.05 noise), probes drawn the same way; the calls timed in alternation,
`repeats` windows of `iters` calls each after a warm-up of the same calls; median / min / max per call.  Row tags: bit 0 on every
row, bit 1 on a random eighth, bit 2 on a random 1/128; every probe of a call carries the same mask (1, 2 or 4).  Beside the
times, the stat "topk_tagged_tiles" per probe of each tagged call (of 7813 and 782 tiles) and whether the all-eligible list
equals the untagged one bit for bit.  Under `rocprofv3 --kernel-trace --stats -- python tools/topk_tagged_bench.py --shape big
--repeats 1 --iters 3` the per-kernel split comes from the profiler."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deep_insight_face import oneshot  # noqa: E402
from topk_bench import D, make, stats, window  # noqa: E402

K = 10
SHARES = (('all', 1, 1.0), ('eighth', 2, 1 / 8), ('one_in_128', 4, 1 / 128))   # name, mask, share of the rows eligible


def run_shape(B, G, repeats, iters):
    probes, gal_rows, _ = make(G, B, seed=G + B)
    gal = oneshot.Gallery(gal_rows)
    del gal_rows
    gen = torch.Generator(device='cuda').manual_seed(7 + G)
    u = torch.rand((G, 2), device='cuda', generator=gen)
    tags = (1 + 2 * (u[:, 0] < 1 / 8).to(torch.int64) + 4 * (u[:, 1] < 1 / 128).to(torch.int64)).contiguous()
    labels = (torch.arange(G, device='cuda') % max(1, G // 4)).contiguous()
    masks = {name: torch.full((B,), m, dtype=torch.int64, device='cuda') for name, m, _ in SHARES}
    idx = {n: torch.empty((B, K), dtype=torch.int64, device='cuda') for n in ('plain', 'ids', 'ids_all') + tuple(masks)}
    dist = {n: torch.empty((B, K), dtype=torch.float32, device='cuda') for n in idx}
    calls = {'topk_untagged': lambda: gal.topk_into(probes, K, 1, idx['plain'], dist['plain'])}
    for name in masks:
        calls['topk_tagged_' + name] = (lambda n=name: gal.topk_into(probes, K, 1, idx[n], dist[n], tags, masks[n]))
    calls['topk_ids_untagged'] = lambda: gal.topk_ids_into(probes, K, 1, labels, None, idx['ids'], dist['ids'])
    calls['topk_ids_tagged_all'] = lambda: gal.topk_ids_into(probes, K, 1, labels, None, idx['ids_all'], dist['ids_all'], None,
                                                             tags, masks['all'])
    tiles = {}
    for name, fn in calls.items():                                   # warm-up: every shape the timed windows use
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if 'tagged_' in name:
            tiles[name] = gal.stat('topk_tagged_tiles') / B
    same = bool((idx['all'] == idx['plain']).all()) and bool((dist['all'].view(torch.int32) == dist['plain'].view(torch.int32)).all())
    same_ids = bool((idx['ids_all'] == idx['ids']).all())
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():                               # alternated: drifts of clock and neighbours hit all calls
            times[name].append(window(fn, iters))
    gal.close()
    out = {'probes': B, 'rows': G, 'd': D, 'metric': 1, 'k': K, 'tiles': (G + 127) // 128, 'iters_per_window': iters,
           'windows': repeats, 'eligible_share': {n: float(((tags & m) != 0).float().mean()) for n, m, _ in SHARES},
           'all_eligible_equals_untagged': same, 'ids_all_eligible_equals_untagged': same_ids, 'tagged_tiles_per_probe': tiles}
    for name in calls:
        out[name] = stats(times[name])
        base = 'topk_ids_untagged' if name.startswith('topk_ids') else 'topk_untagged'
        if name != base:
            out[name]['ratio_to_untagged'] = out[name]['median_ms'] / out[base]['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'topk_tagged_bench.json'))
    ap.add_argument('--shape', default='all', choices=('all', 'big', 'small'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=0, help='calls per window (default: 10 at 1 M rows, 200 at 100 k)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'topk_tagged_bench needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'shapes': []}
    if a.shape in ('all', 'big'):
        res['shapes'].append(run_shape(512, 1_000_000, a.repeats, a.iters or 10))
    if a.shape in ('all', 'small'):
        res['shapes'].append(run_shape(1, 100_000, a.repeats, a.iters or 200))
    for s in res['shapes']:
        print(json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
