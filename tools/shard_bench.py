"""Times the sharded gallery's queries in-process on one GPU -- for topk (k = 10 and 128), topk_ids, within and rank: ONE
shard's local query next to the device merge of all shards' results, and dif_match_rank_at next to dif_match_rank on the same
shard -- with HIP events, and writes profiles/shard_bench.json.

    python tools/shard_bench.py [--out profiles/shard_bench.json] [--repeats 5] [--commit ID]

Shape: R = 8 Gallery handles of 125 000 rows x 512-d (a 1 M-row gallery row-sharded over the GPUs of a node), 512 probes,
metric 1.  Gallery: identities of four near-duplicate rows (centre + 0.05 noise; an identity's rows are 250 000 apart, so they
lie in four different shards), probes drawn the same way from the identities whose first row is in shard 0; that row is the
rank's mate.  Every shard is queried once (untimed) to fill the stacked [R, ...] inputs of the merges; the timed calls are
shard 0's local query and the merge, in alternation, `repeats` windows each after a warm-up of the same calls; median / min /
max per call.  What a real node adds to these two -- the all-gathers -- is not measured here: one GPU has nobody to gather
from.  The two ratios the JSON records: merge / one shard's local query, and rank_at / rank."""
import argparse
import json
import os
import socket
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
from deep_insight_face import oneshot, parallel  # noqa: E402

D, R, ROWS, B, MAX_HITS, TOL = 512, 8, 125_000, 512, 64, 0.2


def make(seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    G = R * ROWS
    nid = G // 4
    centres = torch.randn(nid, D, device='cuda', generator=gen)
    rows = torch.arange(G, device='cuda')
    gal = centres[rows % nid] + 0.05 * torch.randn(G, D, device='cuda', generator=gen)
    pick = torch.randint(0, ROWS, (B,), device='cuda', generator=gen)           # identities whose first row is in shard 0
    probes = centres[pick] + 0.05 * torch.randn(B, D, device='cuda', generator=gen)
    return probes.contiguous(), gal.contiguous(), (rows % nid).contiguous(), pick.contiguous()


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


def commit_id():
    try:
        return subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL,
                                       text=True).strip()
    except Exception:
        return 'unknown'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shard_bench.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--commit', default=None, help='what the JSON names as the code measured (default: git rev-parse HEAD)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'shard_bench needs a HIP device'
    probes, gal, labels, mates = make(seed=R * ROWS + B)
    shards = [oneshot.Gallery(gal[r * ROWS:(r + 1) * ROWS], index_base=r * ROWS) for r in range(R)]
    lab = [labels[r * ROWS:(r + 1) * ROWS].contiguous() for r in range(R)]
    del gal
    g0 = shards[0]

    def i64(*shape):
        return torch.empty(shape, dtype=torch.int64, device='cuda')

    def f32(*shape):
        return torch.empty(shape, dtype=torch.float32, device='cuda')

    calls, iters = {}, {}
    for k in (10, 128):                                              # topk and topk_ids: every shard once, then shard 0 and the merge
        si, sd, sl = i64(R, B, k), f32(R, B, k), i64(R, B, k)
        for r, g in enumerate(shards):
            g.topk_into(probes, k, 1, si[r], sd[r])
        calls['topk_k%d_local' % k] = lambda k=k, i=i64(B, k), d=f32(B, k): g0.topk_into(probes, k, 1, i, d)
        calls['topk_k%d_merge' % k] = lambda si=si, sd=sd: parallel.merge_topk(si, sd)
        if k == 10:
            ti, td = si.clone(), sd.clone()
            for r, g in enumerate(shards):
                g.topk_ids_into(probes, k, 1, lab[r], None, ti[r], td[r], sl[r])
            calls['topk_ids_k10_local'] = lambda i=i64(B, k), d=f32(B, k), l=i64(B, k): g0.topk_ids_into(probes, 10, 1, lab[0],
                                                                                                        None, i, d, l)
            calls['topk_ids_k10_merge'] = lambda ti=ti, td=td, sl=sl: parallel.merge_topk_ids(ti, td, sl)
    wc, wi, wd = i64(R, B), i64(R, B, MAX_HITS), f32(R, B, MAX_HITS)
    for r, g in enumerate(shards):
        g.within_into(probes, TOL, 1, wc[r], wi[r], wd[r])
    calls['within_local'] = lambda c=i64(B), i=i64(B, MAX_HITS), d=f32(B, MAX_HITS): g0.within_into(probes, TOL, 1, c, i, d)
    calls['within_merge'] = lambda: parallel.merge_within(wc, wi, wd)
    rc, ro, rm = i64(R, B), i64(R, B), f32(R, B)
    for r, g in enumerate(shards):
        g.mate_dist_into(probes, mates, 1, rm[r], ro[r])
    _, dm = parallel.merge_rank(torch.zeros_like(ro), ro, rm)
    for r, g in enumerate(shards):
        g.rank_at_into(probes, mates, dm, 1, rc[r])
    rank, mdist, cnt = i64(B), f32(B), i64(B)
    calls['rank_local'] = lambda: g0.rank_into(probes, mates, 1, rank, mdist)              # dif_match_rank: the mate is shard 0's
    calls['rank_at_local'] = lambda: g0.rank_at_into(probes, mates, dm, 1, cnt)            # dif_match_rank_at, the same mates
    calls['mate_dist_local'] = lambda m=f32(B), o=i64(B): g0.mate_dist_into(probes, mates, 1, m, o)
    calls['rank_merge'] = lambda: parallel.merge_rank(rc, ro, rm)
    for name in calls:
        iters[name] = 500 if name.endswith('_merge') or name.startswith('mate_dist') else 50

    for name, fn in calls.items():                                   # warm-up: every call the timed windows make
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    total_rank, _ = parallel.merge_rank(rc, ro, rm)
    assert bool((ro.sum(0) == 1).all()) and int(total_rank.min()) >= 0
    times = {name: [] for name in calls}
    for _ in range(a.repeats):
        for name, fn in calls.items():                               # alternated: drifts of clock and neighbours hit every call
            times[name].append(window(fn, iters[name]))
    for g in shards:
        g.close()

    res = {'device': torch.cuda.get_device_name(0), 'box': socket.gethostname(), 'commit': a.commit or commit_id(),
           'shards': R, 'rows_per_shard': ROWS, 'd': D, 'probes': B, 'metric': 1, 'within_tolerance': TOL,
           'within_max_hits': MAX_HITS, 'windows': a.repeats, 'iters_per_window': iters,
           'rank_of_mate': {'mean': float(total_rank.double().mean()), 'max': int(total_rank.max())}}
    for name in calls:
        res[name] = stats(times[name])
    for q in ('topk_k10', 'topk_k128', 'topk_ids_k10', 'within', 'rank'):
        res[q + '_merge']['ratio_to_local'] = res[q + '_merge']['median_ms'] / res[q + '_local']['median_ms']
    res['rank_at_local']['ratio_to_rank_local'] = res['rank_at_local']['median_ms'] / res['rank_local']['median_ms']
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
