"""Un-enrolment cost: dif_gallery_remove of k rows drawn uniformly from G x 512 enrolled rows, against dif_gallery_update of k rows
in place (the yardstick: enrolment's O(k) path) and against the price of the one host read a removal makes (a tiny device write, an
8-byte read-back, a stream synchronise).  HIP events around single calls issued back to back in one process; every removal is
followed by an update that appends k rows, so the size stays G.  Default options: the filter's copy is row-major at 2^17 rows and
in fragment order at 2^20.  Development aid; writes profiles/remove_bench.json.
    python tools/remove_bench.py [reps]
The shape it checks (exit status 1 otherwise): at k = 8 a removal at 2^20 rows takes at most 1.5 x one at 2^17 rows -- a removal that
scanned the gallery would take about 8 x."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
from deep_insight_face import oneshot, _native as N  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
D = 512
hip = ctypes.CDLL('libamdhip64.so')
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
D2H = 2


def summary(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {'median_us': round(float(np.median(us)), 2), 'p10_us': round(float(us[len(us) // 10]), 2),
            'p90_us': round(float(us[(len(us) * 9) // 10]), 2), 'min_us': round(float(us[0]), 2), 'reps': len(us)}


def timed(calls):
    """calls: [(name, thunk)] issued back to back, an event between every two -> {name: [us per repetition]}"""
    names = [n for n, _ in calls[0]]
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(len(c) + 1)] for c in calls]
    for c, ev in zip(calls, evs):
        ev[0].record()
        for i, (_, thunk) in enumerate(c):
            thunk()
            ev[i + 1].record()
    torch.cuda.synchronize()
    return {n: [ev[i].elapsed_time(ev[i + 1]) * 1e3 for ev in evs] for i, n in enumerate(names)}


def bench(G, gen):
    rows = torch.nn.functional.normalize(torch.randn((G, D), device='cuda', generator=gen), dim=1)
    g = oneshot.Gallery(rows)
    st = N.stream_ptr()
    word = torch.zeros((2,), dtype=torch.int64, device='cuda')
    host = ctypes.c_int64(0)
    moved = torch.empty((2, 1024), dtype=torch.int64, device='cuda')
    m = ctypes.c_int64(0)
    out = {'rows': G, 'frag_copy': g.stat('frag_copy')}

    def read_back():
        hip.hipMemsetAsync(word.data_ptr(), 0, 8, st)
        hip.hipMemcpyAsync(ctypes.byref(host), word.data_ptr(), 8, D2H, st)
        hip.hipStreamSynchronize(st)

    def remove(r):
        N.check(N.lib.dif_gallery_remove(g._h, N.ptr(r), r.shape[0], N.ptr(moved[0]), N.ptr(moved[1]), ctypes.byref(m), st))

    def update(src, k, first):
        N.check(N.lib.dif_gallery_update(g._h, N.ptr(src), k, first, st))

    for k in (1, 8, 1024):
        draws = [torch.sort(torch.randperm(G, device='cuda', generator=gen)[:k])[0].contiguous() for _ in range(REPS + 20)]
        firsts = torch.randint(0, G - k, (REPS + 20,), generator=gen, device='cuda').tolist()
        new = rows[:k]
        calls = [[('remove', lambda r=r: remove(r)), ('append', lambda: update(new, k, G - k)),
                  ('update_in_place', lambda f=f: update(new, k, f)), ('read_back', read_back)]
                 for r, f in zip(draws, firsts)]
        t = timed(calls)
        out['k%d' % k] = {n: summary(v[20:]) for n, v in t.items()}             # (the first 20 repetitions warm up)
        assert len(g) == G
    # a removal that names a special row rebuilds the special-row lists from 8 bytes per gallery row: reported apart
    nan_row = rows[:1].clone()
    nan_row[0, 3] = float('nan')
    spots = torch.randint(0, G - 1, (REPS // 4 + 5,), generator=gen, device='cuda')
    calls = []
    for s in spots.tolist():
        r = torch.tensor([s], dtype=torch.int64, device='cuda')
        calls.append([('plant', lambda s=s: update(nan_row, 1, s)), ('remove_special', lambda r=r: remove(r)),
                      ('append', lambda: update(rows[:1], 1, G - 1))])
    out['k1_special_row'] = {n: summary(v[5:]) for n, v in timed(calls).items() if n == 'remove_special'}
    g.close()
    return out


def main():
    torch.cuda.set_device(0)
    gen = torch.Generator(device='cuda').manual_seed(4)
    res = {'device': torch.cuda.get_device_name(0), 'd': D, 'galleries': [bench(G, gen) for G in (1 << 17, 1 << 20)]}
    small, large = (x['k8']['remove']['median_us'] for x in res['galleries'])
    res['k8_remove_ratio_2p20_over_2p17'] = round(large / small, 3)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'remove_bench.json'), 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res, indent=1))
    if large > 1.5 * small:
        print('FAIL: remove(8) at 2^20 rows takes %.2f x its time at 2^17 rows' % (large / small))
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
