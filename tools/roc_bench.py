"""Times the all-pairs verification counts (Gallery.roc) at 100 and 400 thresholds next to the top-1 match on the f32 filter
(Gallery.match, "filter" = 0 -- the same f32 MFMA main loop over the same rows) and one sparse range search
(Gallery.within, max_hits = 0: the one-threshold census), with HIP events, and writes profiles/roc_bench.json.

    python tools/roc_bench.py [--out profiles/roc_bench.json] [--repeats 5] [--iters 10] [--rows 1000000]

Shape: 512 probes x 1 M rows x 512-d, metric 1.  Gallery: identities of four near-duplicate rows (centre + 0.05 noise),
probes drawn the same way, labelled by identity.  Thresholds: 0 .. 1 by 0.01 (T = 100) and 0 .. 1 by 0.0025 (T = 400), as
float32 on the device through roc_into (the allocation-free form: no conversion, no sort in the timed calls).  The four
calls are timed in alternation, `repeats` windows of `iters` calls each after a warm-up of the same calls; median / min / max
per call.  "roc_resolved" is the number of pairs too close to a threshold to call, evaluated one by one; its share of the
B x G pairs is recorded.  Under `rocprofv3 --kernel-trace --stats -- python tools/roc_bench.py --repeats 1 --iters 3` the
per-kernel split (roc_census_kernel / roc_resolve_kernel) comes from the profiler."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
from deep_insight_face import oneshot  # noqa: E402

D = 512


def make(G, B, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    nid = max(1, G // 4)
    centres = torch.randn(nid, D, device='cuda', generator=gen)
    row_labels = torch.arange(G, device='cuda') % nid
    gal = centres[row_labels] + 0.05 * torch.randn(G, D, device='cuda', generator=gen)
    probe_labels = torch.randint(0, nid, (B,), device='cuda', generator=gen)
    probes = centres[probe_labels] + 0.05 * torch.randn(B, D, device='cuda', generator=gen)
    return probes.contiguous(), gal.contiguous(), probe_labels.contiguous(), row_labels.contiguous()


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


def run(B, G, repeats, iters):
    probes, gal_rows, pl, rl = make(G, B, seed=G + B)
    gal = oneshot.Gallery(gal_rows)
    del gal_rows
    gal.set_option('filter', 0)
    thr = {T: torch.from_numpy(oneshot.up32(np.arange(T) / T)).cuda() for T in (100, 400)}
    acc = {T: torch.empty((T, 2), dtype=torch.int64, device='cuda') for T in thr}
    totals = torch.empty(4, dtype=torch.int64, device='cuda')
    count = torch.empty(B, dtype=torch.int64, device='cuda')
    none_i = torch.empty((B, 0), dtype=torch.int64, device='cuda')
    none_d = torch.empty((B, 0), dtype=torch.float32, device='cuda')
    mi = torch.empty(B, dtype=torch.int64, device='cuda')
    md = torch.empty(B, dtype=torch.float32, device='cuda')
    calls = {
        'match_filter0': lambda: gal.match_into(probes, 1, mi, md),
        'within_sparse': lambda: gal.within_into(probes, 0.2, 1, count, none_i, none_d),
        'roc_100': lambda: gal.roc_into(probes, pl, rl, None, thr[100], 1, acc[100], totals),
        'roc_400': lambda: gal.roc_into(probes, pl, rl, None, thr[400], 1, acc[400], totals),
    }
    found = {}
    for name, fn in calls.items():                                   # warm-up: every shape the timed windows use
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if name.startswith('roc_'):
            T = int(name.split('_')[1])
            resolved = gal.stat('roc_resolved')
            a, t = acc[T].cpu().numpy(), totals.cpu().numpy()
            found[name] = {'borderline_pairs': resolved, 'borderline_share': resolved / float(B * G),
                           'totals': t.tolist(), 'genuine_accepted_at_0.2': int(a[int(round(0.2 * T)), 0]),
                           'impostors_accepted_at_0.5': int(a[T // 2, 1])}
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():                               # alternated: drifts of clock and neighbours hit all four
            times[name].append(window(fn, iters))
    gal.close()
    out = {'probes': B, 'rows': G, 'd': D, 'metric': 1, 'within_tolerance': 0.2, 'within_max_hits': 0,
           'iters_per_window': iters, 'windows': repeats, 'counts': found}
    for name in calls:
        out[name] = stats(times[name])
    for name in ('roc_100', 'roc_400'):
        out[name]['ratio_to_match_filter0'] = out[name]['median_ms'] / out['match_filter0']['median_ms']
        out[name]['ratio_to_within_sparse'] = out[name]['median_ms'] / out['within_sparse']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'roc_bench.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--probes', type=int, default=512)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'roc_bench needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'shapes': [run(a.probes, a.rows, a.repeats, a.iters)]}
    for s in res['shapes']:
        print(json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
