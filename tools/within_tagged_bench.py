"""Times the tagged range search and rank (Gallery.within / Gallery.rank with row_tags and probe_masks) next to the untagged
calls, with HIP events, and writes profiles/within_tagged_bench.json.

    python tools/within_tagged_bench.py [--out profiles/within_tagged_bench.json] [--shape all|big|small] [--repeats 5] [--iters N]

Shapes: 512 probes x 1 M rows x 512-d and 1 probe x 100 k rows x 512-d, metric 1 (tools/within_bench.py's and
tools/rank_bench.py's).  Gallery: identities of four near-duplicate rows (centre + 0.05 noise), probes drawn the same way.
`within` at tolerance 0.2 (a probe's own identity: a handful of hits), max_hits 64; `rank` with every probe mated to a row of
its own identity.  Four forms of each: untagged; tagged with every row eligible (tags and masks -1: the untagged answer);
with 1/8 of the rows eligible; with 1/128 of them.  In the two selective forms the mate is made eligible, so the rank is a
number, not "behind every row".  The eight calls are timed in alternation in one process, `repeats` windows of `iters`
calls each after a warm-up of the same calls; median / min / max per call, and the (probe, tile) pairs evaluated row by row
per probe from stat('within_tagged_tiles')."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
from deep_insight_face import oneshot  # noqa: E402

D, K, TOL = 512, 64, 0.2


def make(G, B, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    nid = max(1, G // 4)
    centres = torch.randn(nid, D, device='cuda', generator=gen)
    gal = centres[torch.arange(G, device='cuda') % nid] + 0.05 * torch.randn(G, D, device='cuda', generator=gen)
    pick = torch.randint(0, nid, (B,), device='cuda', generator=gen)
    probes = centres[pick] + 0.05 * torch.randn(B, D, device='cuda', generator=gen)
    u = torch.rand(G, device='cuda', generator=gen)
    return probes.contiguous(), gal.contiguous(), pick, u


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
    probes, gal_rows, pick, u = make(G, B, seed=G + B)
    gal = oneshot.Gallery(gal_rows)
    del gal_rows
    mates = pick.to(torch.int64).contiguous()                          # the first row of the probe's identity
    ones = torch.full((B,), -1, dtype=torch.int64, device='cuda')
    forms = {'all': (torch.full((G,), -1, dtype=torch.int64, device='cuda'), ones)}
    for name, share, bit in (('eighth', 1 / 8, 2), ('1_128', 1 / 128, 4)):
        tags = torch.where(u < share, bit, 1).to(torch.int64)
        tags[mates] |= bit                                             # the mates are eligible
        forms[name] = (tags.contiguous(), torch.full((B,), bit, dtype=torch.int64, device='cuda'))
    count = torch.empty(B, dtype=torch.int64, device='cuda')
    idx = torch.empty((B, K), dtype=torch.int64, device='cuda')
    dist = torch.empty((B, K), dtype=torch.float32, device='cuda')
    rank = torch.empty(B, dtype=torch.int64, device='cuda')
    md = torch.empty(B, dtype=torch.float32, device='cuda')
    calls = {'within': lambda: gal.within_into(probes, TOL, 1, count, idx, dist),
             'rank': lambda: gal.rank_into(probes, mates, 1, rank, md)}
    for name, (t, m) in forms.items():
        calls['within_tagged_' + name] = lambda t=t, m=m: gal.within_into(probes, TOL, 1, count, idx, dist, t, m)
        calls['rank_tagged_' + name] = lambda t=t, m=m: gal.rank_into(probes, mates, 1, rank, md, t, m)
    info = {}
    for name, fn in calls.items():                                   # warm-up: every shape the timed windows use
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        info[name] = ({'hits_mean': float(count.double().mean()), 'hits_max': int(count.max())} if name.startswith('within')
                      else {'rank_mean': float(rank.double().mean()), 'rank_max': int(rank.max())})
        if 'tagged' in name:
            info[name]['tiles_per_probe'] = gal.stat('within_tagged_tiles') / B
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():                               # alternated: drifts of clock and neighbours hit all of them
            times[name].append(window(fn, iters))
    gal.close()
    out = {'probes': B, 'rows': G, 'tiles': (G + 127) // 128, 'd': D, 'metric': 1, 'max_hits': K, 'tolerance': TOL,
           'iters_per_window': iters, 'windows': repeats}
    for name in calls:
        out[name] = dict(stats(times[name]), **info[name])
        base = out['within' if name.startswith('within') else 'rank']
        if 'tagged' in name:
            out[name]['ratio_to_untagged'] = out[name]['median_ms'] / base['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'within_tagged_bench.json'))
    ap.add_argument('--shape', default='all', choices=('all', 'big', 'small'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=0, help='calls per window (default: 10 at 1 M rows, 300 at 100 k)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'within_tagged_bench needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'shapes': []}
    if a.shape in ('all', 'big'):
        res['shapes'].append(run_shape(512, 1_000_000, a.repeats, a.iters or 10))
    if a.shape in ('all', 'small'):
        res['shapes'].append(run_shape(1, 100_000, a.repeats, a.iters or 300))
    for s in res['shapes']:
        print(json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
