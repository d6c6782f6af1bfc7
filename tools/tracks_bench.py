"""Times FrameFaces.tracks (dif_tracks_link) and its passes with HIP events and writes profiles/tracks_bench.json.

    python tools/tracks_bench.py [--out profiles/tracks_bench.json] [--repeats 5] [--iters 20]

tools/topk_bench.py's protocol: one process, the calls timed in alternation, `repeats` windows of `iters` calls each after a
warm-up of the same calls; median / min / max per call.  Shapes: 256 frames, d = 512, 4 and 16 faces per frame at the most,
max_gap 1 and 4, metric 1, sequences and boxes of tests/tracks_ref.py's generator.  Timed per shape:
  tracks          FrameFaces.tracks with max_faces_per_frame given (no host read; its allocations included)
  link            dif_tracks_link alone on buffers allocated once: all three passes
  cand / walk     its candidate pass and its one-block walk alone (DIF_TRACKS_PASS_CAND / _WALK on the same buffers)
and as yardsticks from the same run, both existing code:
  cluster         FrameFaces.cluster(tolerance) on the same M faces
  pairwise        one dif_pairwise of M pairs (evaluation.utility.distance of the rows against themselves rolled by one)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tracks_ref  # noqa: E402
from deep_insight_face import _native as N  # noqa: E402
from deep_insight_face.detector.faces import FrameFaces  # noqa: E402
from deep_insight_face.evaluation import utility  # noqa: E402

FRAMES, D, TOL, MIN_IOU = 256, 512, 0.2, 0.3


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


def run_shape(per_frame, max_gap, repeats, iters):
    dev = torch.device('cuda', 0)
    off, boxes, emb, _ = tracks_ref.sequence(1000 + per_frame, FRAMES, per_frame, D, canvas=(160 * per_frame, 480), miss=0.1,
                                             false_rate=0.1 * per_frame, per_frame=per_frame)
    m = int(off[-1])
    frame = np.repeat(np.arange(FRAMES), np.diff(off))
    ff = FrameFaces(torch.from_numpy(off).to(dev), torch.from_numpy(frame).to(dev), torch.from_numpy(boxes).to(dev),
                    torch.ones((m,), device=dev), None, torch.zeros((m, 1, 1, 3), dtype=torch.uint8, device=dev),
                    emb=torch.from_numpy(emb).to(dev))
    i64 = dict(dtype=torch.int64, device=dev)
    prev, labels, age, cnt = torch.empty((m,), **i64), torch.empty((m,), **i64), torch.empty((m,), **i64), torch.empty((2,), **i64)
    dist = torch.empty((m,), dtype=torch.float32, device=dev)
    state = torch.empty((N.lib.dif_tracks_state_size(max_gap, per_frame, D),), dtype=torch.uint8, device=dev)
    work = torch.empty((N.lib.dif_tracks_workspace_size(m, max_gap, per_frame, 0),), dtype=torch.uint8, device=dev)

    def link(passes):
        N.check(N.lib.dif_tracks_link(N.ptr(ff.offsets), N.ptr(ff.boxes), N.ptr(ff.emb), FRAMES, m, D, TOL, MIN_IOU, max_gap, 1, per_frame,
                                      0, None, 0, 0, N.ptr(prev), N.ptr(dist), N.ptr(labels), N.ptr(age), N.ptr(cnt), N.ptr(cnt[1:]),
                                      N.ptr(state), per_frame, N.ptr(work), work.shape[0], passes, N.stream_ptr()))

    rolled = ff.emb.roll(1, 0).contiguous()
    calls = {
        'tracks': lambda: ff.tracks(TOL, MIN_IOU, max_gap, 1, max_faces_per_frame=per_frame),
        'link': lambda: link(0),
        'cand': lambda: link(1),
        'walk': lambda: link(2),
        'cluster': lambda: ff.cluster(TOL, 1),
        'pairwise': lambda: utility.distance(ff.emb, rolled, 1),
    }
    for fn in calls.values():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    t = ff.tracks(TOL, MIN_IOU, max_gap, 1, max_faces_per_frame=per_frame)
    link(0)
    assert torch.equal(t.labels, labels) and torch.equal(t.prev, prev)
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            times[name].append(window(fn, iters))
    out = {'frames': FRAMES, 'faces_per_frame': per_frame, 'faces': m, 'd': D, 'metric': 1, 'max_gap': max_gap, 'tolerance': TOL,
           'min_iou': MIN_IOU, 'tracks_started': int(cnt[0]), 'links': m - int(cnt[0]), 'clipped': int(cnt[1]),
           'clusters': int(ff.cluster(TOL, 1).unique().numel()), 'iters_per_window': iters, 'windows': repeats}
    for name in calls:
        out[name] = stats(times[name])
    out['walk_share_of_link'] = out['walk']['median_ms'] / out['link']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tracks_bench.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'tracks_bench needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'shapes': []}
    for per_frame in (4, 16):
        for max_gap in (1, 4):
            res['shapes'].append(run_shape(per_frame, max_gap, a.repeats, a.iters))
            print(json.dumps(res['shapes'][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
