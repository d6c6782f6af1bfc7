"""The layer-tap sweep of tests/test_layer_taps_gpu.py as a tool: every case, every launch, and per kernel form the worst
figures and where they occurred.

    python tools/layer_taps.py [substring of case ids ...] [--out profiles/layer_taps.json]

Per kernel label (op_table()'s `family<tile, operand form>`):
  hard   worst |y - ref| / B over every element of every image of every layer the form ran (B: the a-priori bound)
  tight  worst (max |y - ref| / A~) / max(max |y32 - ref| / A~, 2 u): the kernel against the float32 yardstick (gate: 8);
         for the GDC tail, l2norm_kernel and lrn_kernel the same in units of B.  The L2 / average pools are listed as
         maxpool_kernel[l2] / maxpool_kernel[avg] (hard only; 'max' mode is bit-exact and has no row).
  split<t>_hard, split<t>_max, split<t>_rms  (split-bf16 labels, t = 3 / 2 terms) against the split reference S, the float64 sum
         of the tier's kept products: worst |y - S| / B (gate 1), worst max-error and worst rms-error ratio of the kernel to the
         float32 yardstick in the kernel's order of products (gates 8 and layer_ref.RMS_MARGIN).
Needs the MI355X.  DESIGN 4l holds the table this writes.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'deep-insight-face_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_layer_taps_gpu as T  # noqa: E402
from test_nonsquare_gpu import Zoo  # noqa: E402


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, 'profiles', 'layer_taps.json')
    if '--out' in args:
        out = args[args.index('--out') + 1]
        del args[args.index('--out'):args.index('--out') + 2]
    cases = [c for c in T.CASES + T.SPLIT_CASES if not args or any(a in c['id'] for a in args)]
    zoo, env = Zoo(), T.Env()
    failures, per_case = [], []
    try:
        for c in cases:
            t0 = time.time()
            fails, seen, checked = (T.run_split_case if 'engaged' in c else T.run_case)(zoo, c, env)
            per_case.append({'case': c['id'], 'launches': checked, 'failures': len(fails), 'seconds': round(time.time() - t0, 2)})
            failures += ['%s: %s' % (c['id'], f) for f in fails]
            print('%-48s %3d launches %2d failures %.1f s' % (c['id'], checked, len(fails), time.time() - t0), flush=True)
    finally:
        zoo.close()
    forms = {k: {key: {'ratio': float('%.4g' % v[0]), 'layer': v[1]} for key, v in rec.items()} for k, rec in sorted(T.RECORD.items())}
    doc = {'what': 'worst per-layer figures of the layer-tap sweep per kernel form: hard = |y - ref| / B (gate 1), '
                   'tight = kernel error / float32 yardstick error, both relative to A~ (gate 8); split-bf16 labels, per tier t: '
                   'split<t>_hard = |y - S| / B against the float64 sum S of the kept products (gate 1), split<t>_max and split<t>_rms = '
                   'kernel / yardstick of max and rms (y - S) / A~ (gates 8 and %g)' % T.layer_sweep.L.RMS_MARGIN,
           'cases': per_case, 'forms': forms, 'failures': failures}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump(doc, fh, indent=1)
        fh.write('\n')
    print('%-72s %10s %10s' % ('kernel form', 'hard', 'tight'))
    for k, rec in forms.items():
        print('%-72s %10.4g %10s' % (k, rec.get('hard', {}).get('ratio', float('nan')),
                                     '%.3g' % rec['tight']['ratio'] if 'tight' in rec else '-'))
    print('%-58s %5s %10s %8s %8s' % ('split-bf16 label', 'terms', '|y - S|/B', 'max', 'rms'))
    for k, rec in forms.items():
        for t in (3, 2):
            if 'split%d_rms' % t in rec:
                print('%-58s %5d %10.4g %8.3g %8.3g' % ((k, t) + tuple(rec['split%d_%s' % (t, key)]['ratio'] for key in ('hard', 'max', 'rms'))))
    print('%d cases, %d failures -> %s' % (len(cases), len(failures), out))
    return 1 if failures else 0


if __name__ == '__main__':
    sys.exit(main())
