"""Times one detector evaluation (deep_insight_face.evaluation.detection) at a WIDER-FACE-val-like size with HIP events
and writes profiles/deteval_bench.json.

    python tools/deteval_bench.py [--out profiles/deteval_bench.json] [--repeats 5] [--iters 10] [--no-host]

Size: 3 226 frames, about 39 k truths (a long-tailed count per frame, one frame in eight without a face, 5 % ignored), 300
detections per frame (967 800 in all: 70 % jittered off a truth of the frame, the rest strays; scores in steps of 2^-16, so
ties happen), 10 IoU thresholds 0.5 .. 0.95.  Seeded; the inputs are on the device before the clock starts.  tools/
tracks_bench.py's protocol: one process, the calls timed in alternation, `repeats` windows of `iters` calls each after a warm-
up of the same calls; median / min / max per call.  Timed:
  evaluate     evaluate_detections: one dif_det_match and one dif_det_curve, allocations included
  match        DetectionEvaluator.add alone (dif_det_match: best truth, the rank, claim, classify)
  curve        DetectionEvaluator.result alone on what one add left (dif_det_curve: the rank, the scans, AP)
  chunks       the same frames through one evaluator in 13 batches of up to 256 frames, then result
and once, on the host clock, the NumPy restatement tests/detection_ref.py on the same inputs: the sequential loop the rule is
told in, a yardstick of the host-side evaluation the reference's lineage runs, not a tuned implementation.  Every output of
the device is compared with it bit for bit (ap: to n_truth * 2^-52) before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import detection_ref as R  # noqa: E402
from deep_insight_face.evaluation import detection as D  # noqa: E402

FRAMES, PER_FRAME, MEAN_TRUTHS = 3226, 300, 12.2


def inputs(seed=3226):
    rng = np.random.default_rng(seed)
    counts = np.minimum(rng.geometric(1.0 / (MEAN_TRUTHS / 0.875), FRAMES), 900) * (rng.random(FRAMES) >= 0.125)
    go = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t = int(go[-1])
    xy = rng.random((t, 2)) * np.array([960.0, 700.0])
    gt = np.concatenate([xy, xy + 8.0 + rng.random((t, 2)) * 56.0], axis=1)
    ignore = (rng.random(t) < 0.05).astype(np.uint8)
    m = FRAMES * PER_FRAME
    do = np.arange(FRAMES + 1, dtype=np.int64) * PER_FRAME
    frame = np.repeat(np.arange(FRAMES), PER_FRAME)
    stray = (rng.random(m) >= 0.7) | (counts[frame] == 0)
    pick = go[frame] + (rng.random(m) * counts[frame]).astype(np.int64)
    base = gt[np.minimum(pick, max(t - 1, 0))]
    side = (base[:, 2] - base[:, 0] + base[:, 3] - base[:, 1])[:, None] / 2
    boxes = base + rng.normal(0.0, 1.0, (m, 4)) * side * 0.12 * rng.random((m, 1))
    p = rng.random((m, 2)) * np.array([960.0, 700.0])
    boxes[stray] = np.concatenate([p, p + 8.0 + rng.random((m, 2)) * 56.0], axis=1)[stray]
    scores = np.round(rng.random(m) * 65536) / 65536
    return dict(name='wider_val_like', det_boxes=boxes.astype(np.float32), det_scores=scores.astype(np.float32), det_offsets=do,
                gt_boxes=gt.astype(np.float32), gt_offsets=go, gt_ignore=ignore)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'deteval_bench.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--no-host', action='store_true', help='skip the NumPy restatement (and the comparison with it)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'deteval_bench needs a HIP device'
    dev = torch.device('cuda', 0)
    case = inputs()
    keys = ('det_boxes', 'det_scores', 'det_offsets', 'gt_boxes', 'gt_offsets')
    on_dev = [torch.from_numpy(case[k]).to(dev) for k in keys]
    ignore = torch.from_numpy(case['gt_ignore']).to(dev)
    spans = [(f, min(f + 256, FRAMES)) for f in range(0, FRAMES, 256)]
    parts = []
    for f0, f1 in spans:
        b = R.batch(case, f0, f1)
        parts.append(([torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in keys], torch.from_numpy(b['gt_ignore']).to(dev)))
    held = D.DetectionEvaluator(R.COCO)
    held.add(*on_dev, gt_ignore=ignore)

    def chunks():
        ev = D.DetectionEvaluator(R.COCO)
        for args, ign in parts:
            ev.add(*args, gt_ignore=ign)
        return ev.result()

    calls = {
        'evaluate': lambda: D.evaluate_detections(*on_dev, iou_thresholds=R.COCO, gt_ignore=ignore),
        'match': lambda: D.DetectionEvaluator(R.COCO).add(*on_dev, gt_ignore=ignore),
        'curve': held.result,
        'chunks': chunks,
    }
    res = calls['evaluate']()
    by_chunks = chunks()
    fields = ('assigned', 'iou', 'outcome', 'n_truth', 'order', 'tp_cum', 'fp_cum', 'recall', 'precision', 'ap')
    assert all(torch.equal(getattr(res, k), getattr(by_chunks, k)) for k in fields), 'chunks differ from one call'
    out = {'device': torch.cuda.get_device_name(0), 'frames': FRAMES, 'detections': int(case['det_offsets'][-1]),
           'truths': int(case['gt_offsets'][-1]), 'truths_not_ignored': int(res.n_truth.item()), 'thresholds': len(R.COCO),
           'largest_frame_truths': int(np.diff(case['gt_offsets']).max()), 'ap': res.ap.cpu().tolist(),
           'iters_per_window': a.iters, 'windows': a.repeats}
    if not a.no_host:
        t0 = time.perf_counter()
        want = R.evaluate(case, R.COCO)
        out['host_restatement_s'] = time.perf_counter() - t0
        for k in fields[:-1]:
            got = getattr(res, k).cpu().numpy()
            assert got.tobytes() == np.asarray(want[k]).astype(got.dtype).reshape(got.shape).tobytes(), k
        gap = np.abs(res.ap.cpu().numpy() - want['ap']).max()
        assert gap <= want['n_truth'] * 2.0 ** -52, gap
        out['equal_to_host_restatement'] = True
        out['ap_gap_to_host'] = float(gap)
    for fn in calls.values():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(a.repeats):
        for name, fn in calls.items():
            times[name].append(window(fn, a.iters))
    for name in calls:
        out[name] = stats(times[name])
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
