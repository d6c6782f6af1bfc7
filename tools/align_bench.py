"""Cost of five-point alignment next to the box crop it replaces, at the frames_mtcnn workload's shape (256 frames of
480 x 640 -> 112 x 112 crops, ResNet-50V2, MTCNN with synthetic weights that give every frame a detection).

    timeout -k 10 600 python tools/align_bench.py [--frames 256] [--repeats 50] [--pipeline-repeats 5] [--out FILE]

HIP events around batches of launches on one stream, after a warm-up; the two crop kernels and the two pipelines are
timed alternately in the same process so that they see the same machine.  One JSON line on stdout (and in --out).
Landmarks / boxes for the kernel timings describe the same faces: a similarity of scale ~1.5 .. 3 somewhere on the frame,
the box being the landmarks' bounding box grown to a face's proportions."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'deep-insight-face_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def _time(fn, repeats, rounds=5):
    """Median over `rounds` of the mean time of `repeats` back-to-back calls, ms."""
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / repeats)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--pipeline-repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from deep_insight_face import _native as N
    from deep_insight_face.detector import mtcnn as dm
    from deep_insight_face.detector.align import ARCFACE_TEMPLATE_112 as T, align_faces
    from deep_insight_face.detector.run import crop_faces
    from deep_insight_face.networks.triplet import DifEmbedder
    dev = N.require_device()
    n, h, w, size = args.frames, 480, 640, 112
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    rng = np.random.default_rng(2)
    lm = np.empty((n, 5, 2), np.float32)
    boxes = np.empty((n, 4), np.float32)
    scales = []
    for i in range(n):
        s, deg = rng.uniform(1.5, 3.0), rng.uniform(-20, 20)
        scales.append(s)
        c, si = s * np.cos(np.radians(deg)), s * np.sin(np.radians(deg))
        p = (T - T.mean(0)) @ np.array([[c, si], [-si, c]]) + [rng.uniform(200, 440), rng.uniform(170, 310)]
        lm[i] = p
        cx, cy, half = p[:, 0].mean(), p[:, 1].mean(), 56 * s - 4         # the template's 112-pixel window, less crop_faces' margin
        boxes[i] = [cx - half, cy - half, cx + half, cy + half]
    lm_d, boxes_d = torch.from_numpy(lm).to(dev), torch.from_numpy(boxes).to(dev)
    src_px = float(np.mean([(112 * s) ** 2 for s in scales]))           # frame pixels under one crop's 112 x 112 window
    res = {'shape': '%d frames of %dx%d -> %dx%d' % (n, h, w, size, size), 'device': torch.cuda.get_device_name(dev)}
    kern = {'dif_align_crop': lambda: align_faces(frames, lm_d, size), 'dif_crop_resize': lambda: crop_faces(frames, boxes_d, 8, size)}
    for fn in kern.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for name in ('dif_align_crop', 'dif_crop_resize', 'dif_align_crop', 'dif_crop_resize'):       # alternately, twice
        med, lo, hi = _time(kern[name], args.repeats)
        res.setdefault(name + '_ms', []).append(round(med, 4))
        res.setdefault(name + '_spread_ms', []).append([round(lo, 4), round(hi, 4)])
    out_bytes = n * size * size * 3
    res['floor'] = {'output_bytes': out_bytes, 'source_footprint_bytes': int(n * src_px * 3),
                    'note': 'bytes written + mean source square touched per crop x 3 channels; over HBM bandwidth = the least time'}
    det = dm.MtcnnDetector((h, w), max_batch=64).init_synthetic(2025, logit_scale=1e-3)
    emb = DifEmbedder('resnet', 'v2', 512, (size, size, 3), max_batch=n).init_synthetic(3)
    emb.set_input_transform(scale=1 / 255.)
    pipes = {'pipeline_align_off_ms': dm.MtcnnFramePipeline(det, emb, None, margin=8),
             'pipeline_align_on_ms': dm.MtcnnFramePipeline(det, emb, None, margin=8, align=True)}
    for pipe in pipes.values():
        for _ in range(2):
            pipe(frames)
    torch.cuda.synchronize()
    for name in list(pipes) * 2:
        med, lo, hi = _time(lambda: pipes[name](frames), args.pipeline_repeats, rounds=3)
        res.setdefault(name, []).append(round(med, 3))
        res.setdefault(name.replace('_ms', '_spread_ms'), []).append([round(lo, 3), round(hi, 3)])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
