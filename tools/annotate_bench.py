"""Times FrameFaces.annotate (dif_frames_annotate, dif_annotate_compose) with HIP events and writes profiles/annotate_bench.json.

    python tools/annotate_bench.py [--out profiles/annotate_bench.json] [--repeats 9] [--iters 100]

tools/redact_bench.py's protocol: one process, the calls timed in alternation, `repeats` windows of `iters` calls each after a
warm-up of the same calls; median / min / max per call (the defaults, 9 windows of 100 calls, are what the committed file was
written with: a window of 10 of these calls is half a millisecond).  Shape: 256 frames of 480 x 640 with four generated faces each of 40 to
120 pixels (tools/redact_bench.py's seeded boxes, five landmarks inside each), a label of 12 characters, scale 2, thickness 2,
mark 1, in place -- 1 024 faces, one block per face --; and 16 frames of 1080 x 1920 with four faces each of 300 to 600 pixels,
scale 4, thickness 4, mark 3 -- 64 faces, four blocks per face.  Timed per shape:
  annotate           FrameFaces.annotate(frames, text=text, colors=colors, out=frames): the drawing alone
  compose            compose_text(names, idx, known, values, length=12): the labels alone
  compose_annotate   FrameFaces.annotate(frames, names=..., known=..., values=..., colors=..., out=frames): both
As yardsticks from the same run, on the same frames and boxes:
  redact_fill        FrameFaces.redact(frames, mode='fill', out=frames): one opaque write of every box
  clone              frames.clone(): the HBM copy a whole-frame pass would cost
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from deep_insight_face.detector import annotate  # noqa: E402
from deep_insight_face.detector.faces import FrameFaces  # noqa: E402
from redact_bench import stats, window  # noqa: E402

PER_FRAME, LENGTH = 4, 12
SHAPES = ((256, 480, 640, 40, 120, 2, 2, 1), (16, 1080, 1920, 300, 600, 4, 4, 3))      # frames, h, w, box sides, thickness, scale, mark


def faces(frames, h, w, lo, hi, dev):
    """tools/redact_bench.py's generator (the same boxes at its shape): seeded squares anywhere in the frame."""
    rng = np.random.default_rng(4000 + PER_FRAME)
    m = frames * PER_FRAME
    side = rng.uniform(lo, hi, m)
    x, y = rng.uniform(0, w - side), rng.uniform(0, h - side)
    boxes = np.stack([x, y, x + side, y + side], 1).astype(np.float32)
    off = np.arange(frames + 1, dtype=np.int64) * PER_FRAME
    frame = np.repeat(np.arange(frames), PER_FRAME)
    ff = FrameFaces(torch.from_numpy(off).to(dev), torch.from_numpy(frame).to(dev), torch.from_numpy(boxes).to(dev),
                    torch.ones((m,), device=dev), None, torch.zeros((m, 1, 1, 3), dtype=torch.uint8, device=dev))
    return ff, float((side * side).sum())


def run(shape, repeats, iters):
    FRAMES, H, W, lo, hi, thickness, scale, mark = shape
    dev = torch.device('cuda', 0)
    ff, box_pixels = faces(FRAMES, H, W, lo, hi, dev)
    m = FRAMES * PER_FRAME
    draw = dict(thickness=thickness, scale=scale, mark=mark)
    rng = np.random.default_rng(4100)
    b = ff.boxes.cpu().numpy()
    lm = np.stack([b[:, :1] + (b[:, 2:3] - b[:, :1]) * rng.uniform(0.2, 0.8, (m, 5)),
                   b[:, 1:2] + (b[:, 3:4] - b[:, 1:2]) * rng.uniform(0.2, 0.8, (m, 5))], 2).astype(np.float32)
    table = annotate.NameTable(['name%04d' % k for k in range(1000)], length=8, device=dev)      # 8 + ' ' + '0.x' = 12 characters at 1 decimal
    ff = ff._replace(landmarks=torch.from_numpy(lm).to(dev), idx=torch.from_numpy(rng.integers(0, 1000, m)).to(dev),
                     dist=torch.from_numpy(rng.uniform(0.1, 0.9, m).astype(np.float32)).to(dev))
    known = ff.dist <= 2.0
    colors = annotate.palette(torch.from_numpy(rng.integers(0, 64, m)).to(dev))
    text = annotate.compose_text(table, ff.idx, known, ff.dist, 1, '?', LENGTH)
    assert int((text != 0).sum(1).min()) == LENGTH
    gen = torch.Generator(device=dev).manual_seed(7)
    source = torch.randint(0, 256, (FRAMES, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    frames = source.clone()
    calls = {
        'annotate': lambda: ff.annotate(frames, text=text, colors=colors, out=frames, **draw),
        'compose': lambda: annotate.compose_text(table, ff.idx, known, ff.dist, 1, '?', LENGTH),
        'compose_annotate': lambda: ff.annotate(frames, names=table, known=known, values=ff.dist, colors=colors, decimals=1, length=LENGTH,
                                                out=frames, **draw),
        'redact_fill': lambda: ff.redact(frames, None, 'fill', out=frames),
        'clone': lambda: source.clone(),
    }
    for fn in calls.values():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            times[name].append(window(fn, iters))
    painted = int((ff.annotate(source, text=text, colors=colors, **draw) != source).any(dim=3).sum())
    filled = int((ff.redact(source, None, 'fill', fill=(1, 2, 3)) != source).any(dim=3).sum())
    out = {'frames': FRAMES, 'h': H, 'w': W, 'faces_per_frame': PER_FRAME, 'faces': m, 'text_length': LENGTH, 'scale': scale, 'thickness': thickness, 'mark': mark,
           'frame_bytes': FRAMES * H * W * 3, 'box_pixels': box_pixels, 'pixels_changed_by_annotate': painted, 'pixels_changed_by_fill': filled,
           'in_place': True, 'iters_per_window': iters, 'windows': repeats}
    for name in times:
        out[name] = stats(times[name])
    out['annotate_over_redact_fill'] = out['annotate']['median_ms'] / out['redact_fill']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'annotate_bench.json'))
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--iters', type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'annotate_bench needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'shapes': []}
    for shape in SHAPES:
        res['shapes'].append(run(shape, a.repeats, a.iters))
        print(json.dumps(res['shapes'][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
