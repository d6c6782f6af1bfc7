"""Times dif_face_quality with HIP events and writes profiles/quality_bench.json.

    python tools/quality_bench.py [--out profiles/quality_bench.json] [--repeats 5] [--iters 20]

tools/tracks_bench.py's protocol: one process, `repeats` windows of `iters` calls each after a warm-up of the same calls;
median / min / max per call.  Timed on buffers allocated once, landmarks and boxes given:
  quality         dif_face_quality alone, M = 512 crops of 112 x 112 (19.3 MB read), then M = 512 of 256 x 256 and M = 8 of 112
  wrapper         detector.quality.face_quality on the same tensors (its two allocations included)
and as a yardstick from the same run a device-to-device copy of the crops' bytes (read + write).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
from deep_insight_face import _native as N  # noqa: E402
from deep_insight_face.detector.quality import face_quality  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters          # us per call


def timed(fn, repeats, iters):
    window(fn, iters)
    t = sorted(window(fn, iters) for _ in range(repeats))
    return {'median_us': t[len(t) // 2], 'min_us': t[0], 'max_us': t[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'quality_bench.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    dev = N.require_device()
    rng = np.random.default_rng(0)
    res = {'device': torch.cuda.get_device_name(dev), 'repeats': a.repeats, 'iters': a.iters, 'shapes': []}
    for m, s in ((512, 112), (512, 256), (8, 112)):
        crops = torch.from_numpy(rng.integers(0, 256, (m, s, s, 3), dtype=np.uint8)).to(dev)
        lm = torch.from_numpy(rng.uniform(0, 640, (m, 5, 2)).astype(np.float32)).to(dev)
        bx = torch.from_numpy(rng.uniform(0, 480, (m, 4)).astype(np.float32)).to(dev)
        stats = torch.empty((m, 6), dtype=torch.int64, device=dev)
        cols = torch.empty((m, 10), dtype=torch.float32, device=dev)
        dst = torch.empty_like(crops)
        st = N.stream_ptr()

        def quality():
            N.check(N.lib.dif_face_quality(N.ptr(crops), m, s, N.ptr(lm), N.ptr(bx), 480.0, 640.0, 0, 255, N.ptr(stats), N.ptr(cols), st))

        row = {'m': m, 'size': s, 'bytes_read': m * s * s * 3,
               'quality': timed(quality, a.repeats, a.iters),
               'wrapper': timed(lambda: face_quality(crops, lm, bx, (480, 640)), a.repeats, a.iters),
               'copy': timed(lambda: dst.copy_(crops), a.repeats, a.iters)}
        row['quality_gb_per_s'] = row['bytes_read'] / row['quality']['median_us'] / 1e3
        row['copy_gb_per_s_read_plus_write'] = 2 * row['bytes_read'] / row['copy']['median_us'] / 1e3
        res['shapes'].append(row)
        print(json.dumps(row))
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
