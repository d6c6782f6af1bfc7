"""Times FrameFaces.redact (dif_frames_redact) with HIP events and writes profiles/redact_bench.json.

    python tools/redact_bench.py [--out profiles/redact_bench.json] [--repeats 5] [--iters 10]

tools/tracks_bench.py's protocol: one process, the calls timed in alternation, `repeats` windows of `iters` calls each after a
warm-up of the same calls; median / min / max per call.  Shapes: 256 frames of 480 x 640, 4 and 16 generated faces per frame
of 40 to 120 pixels (seeded; square boxes placed anywhere in the frame, so some overlap), the defaults of the call (8 cells,
min_cell 4, margin 0, box), in place.  Timed per shape:
  fill / pixelate / smooth     FrameFaces.redact(frames, mode=..., out=frames) on every face (its workspace allocation included)
  pixelate_ellipse             the same with shape='ellipse'
('fill' launches pass 2 alone; the other modes both passes.)  As yardsticks from the same run, on the same frames:
  clone                        frames.clone(): the HBM copy a whole-frame pass would cost
  to_host                      frames.cpu(): the read-back a host redaction would start with (pageable memory, synchronous)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
from deep_insight_face.detector.faces import FrameFaces  # noqa: E402

FRAMES, H, W = 256, 480, 640


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def wall_window(fn, iters):
    """Milliseconds per call by the host clock: for a call that synchronises (the read-back)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def stats(v):
    v = sorted(v)
    return {'median_ms': v[len(v) // 2], 'min_ms': v[0], 'max_ms': v[-1]}


def faces(per_frame, dev):
    rng = np.random.default_rng(4000 + per_frame)
    m = FRAMES * per_frame
    side = rng.uniform(40, 120, m)
    x, y = rng.uniform(0, W - side), rng.uniform(0, H - side)
    boxes = np.stack([x, y, x + side, y + side], 1).astype(np.float32)
    off = np.arange(FRAMES + 1, dtype=np.int64) * per_frame
    frame = np.repeat(np.arange(FRAMES), per_frame)
    ff = FrameFaces(torch.from_numpy(off).to(dev), torch.from_numpy(frame).to(dev), torch.from_numpy(boxes).to(dev),
                    torch.ones((m,), device=dev), None, torch.zeros((m, 1, 1, 3), dtype=torch.uint8, device=dev))
    return ff, float((side * side).sum())


def run_shape(per_frame, repeats, iters):
    dev = torch.device('cuda', 0)
    ff, box_pixels = faces(per_frame, dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    source = torch.randint(0, 256, (FRAMES, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    frames = source.clone()
    calls = {
        'fill': lambda: ff.redact(frames, None, 'fill', out=frames),
        'pixelate': lambda: ff.redact(frames, None, 'pixelate', out=frames),
        'smooth': lambda: ff.redact(frames, None, 'smooth', out=frames),
        'pixelate_ellipse': lambda: ff.redact(frames, None, 'pixelate', shape='ellipse', out=frames),
        'clone': lambda: source.clone(),
    }
    for fn in calls.values():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    source.cpu()
    times = {name: [] for name in list(calls) + ['to_host']}
    for _ in range(repeats):
        for name, fn in calls.items():
            times[name].append(window(fn, iters))
        times['to_host'].append(wall_window(lambda: frames.cpu(), 2))
    covered = int((ff.redact(source, None, 'fill', fill=(1, 2, 3)) != source).any(dim=3).sum())
    out = {'frames': FRAMES, 'h': H, 'w': W, 'faces_per_frame': per_frame, 'faces': FRAMES * per_frame, 'cells': 8, 'min_cell': 4,
           'frame_bytes': FRAMES * H * W * 3, 'box_pixels': box_pixels, 'pixels_changed_by_fill': covered, 'in_place': True,
           'iters_per_window': iters, 'windows': repeats}
    for name in times:
        out[name] = stats(times[name])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'redact_bench.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'redact_bench needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'shapes': []}
    for per_frame in (4, 16):
        res['shapes'].append(run_shape(per_frame, a.repeats, a.iters))
        print(json.dumps(res['shapes'][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
