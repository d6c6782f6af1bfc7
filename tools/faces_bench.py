"""Cost of `MtcnnFramePipeline.faces` -- every face of every frame -- next to the only equivalent there was before it:
detect -> dif_crop_resize_multi over ALL n * k slots, empty ones included -> embed all of them -> match.  The frames_mtcnn
workload's shape: 256 frames of 480 x 640, MTCNN with the benchmark's synthetic weights, ResNet-50V2 512-d at max_batch 256,
a gallery of 100 000 rows.

    timeout -k 10 900 python tools/faces_bench.py [--frames 256] [--repeats 3] [--rounds 5] [--logit-scales 1e-3,1.0]
                                                  [--out profiles/faces_bench.json]

HIP events around `repeats` back-to-back calls on one stream, after a warm-up; the median over `rounds` such windows, the
two paths timed alternately in the same process.  `--logit-scales`: MtcnnDetector.init_synthetic's knob -- 1e-3 is the
benchmark's detector (every slot that survives the suppressions passes), larger values leave more slots empty.  One JSON line
on stdout (and in --out)."""
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


def _window(fn, repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--logit-scales', default='1e-3,1.0')
    ap.add_argument('--gallery', type=int, default=100_000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from deep_insight_face import _native as N, oneshot
    from deep_insight_face.detector import mtcnn as dm
    from deep_insight_face.networks.triplet import DifEmbedder
    dev = N.require_device()
    n, h, w, size = args.frames, 480, 640, 112
    g = torch.Generator().manual_seed(1234)
    frames = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    emb = DifEmbedder('resnet', 'v2', 512, (size, size, 3), max_batch=256).init_synthetic(3)
    emb.set_input_transform(scale=1 / 255.)
    gal = oneshot.Gallery(np.random.default_rng(0).standard_normal((args.gallery, 512)).astype(np.float32))
    res = {'shape': '%d frames of %dx%d, embedder max_batch %d, gallery %d x 512' % (n, h, w, emb.max_batch, args.gallery),
           'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats, 'rounds': args.rounds, 'cases': []}
    for ls in (float(v) for v in args.logit_scales.split(',')):
        det = dm.MtcnnDetector((h, w), max_batch=64).init_synthetic(2025, logit_scale=ls)
        pipe = dm.MtcnnFramePipeline(det, emb, gal, margin=8)
        k = det.cap[2]

        def all_slots():
            mb = det.max_batch
            parts = [det.detect(frames[lo:lo + mb]) for lo in range(0, n, mb)]
            b, s = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            crops = torch.empty((n * k, size, size, 3), dtype=torch.uint8, device=dev)
            N.check(N.lib.dif_crop_resize_multi(N.ptr(frames), n, h, w, N.ptr(b), N.ptr(s), k, 8.0, N.ptr(crops), size, N.stream_ptr()))
            e = emb.embed(crops)
            return (s, e) + tuple(gal.match(e, 1))

        paths = {'faces_ms': lambda: pipe.faces(frames), 'all_slots_ms': all_slots}
        for fn in paths.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ff = pipe.faces(frames)
        s, e, idx, _ = all_slots()
        keep = (s >= 0).reshape(-1)
        case = {'logit_scale': ls, 'M': int(ff.frame.shape[0]), 'n_x_k': n * k, 'frames_with_a_face': int((ff.offsets[1:] > ff.offsets[:-1]).sum()),
                'most_faces_in_a_frame': int((ff.offsets[1:] - ff.offsets[:-1]).max()),
                'same_matches_as_all_slots': bool(torch.equal(ff.idx, idx[keep]))}
        times = {name: [] for name in paths}
        for _ in range(args.rounds):                           # alternately
            for name, fn in paths.items():
                times[name].append(_window(fn, args.repeats))
        for name, v in times.items():
            case[name] = round(float(np.median(v)), 3)
            case[name.replace('_ms', '_spread_ms')] = [round(min(v), 3), round(max(v), 3)]
        case['faces_over_all_slots'] = round(case['faces_ms'] / case['all_slots_ms'], 4)
        res['cases'].append(case)
        det.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
