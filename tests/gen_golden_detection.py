"""Generates tests/golden/detection.npz by RUNNING the reference's own detector/utility.py on seeded inputs
(tests/detection_inputs.py).  Run once where a checkout of the reference exists:

    python tests/gen_golden_detection.py <root of the reference checkout>

The module is loaded by file path; what it imports at its top for drawing and image reading (cv2, skimage, and PIL or scipy
where they are missing) is replaced by empty stand-in modules, which compute_overlap and compute_ap never touch.  The fixture
holds data only -- the digest of the inputs, compute_overlap on their float64 casts, compute_ap on a handful of curves -- and
no text of the reference."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import detection_inputs as I   # noqa: E402


def load_reference_utility(root):
    path = os.path.join(root, 'deep_insight_face', 'detector', 'utility.py')
    for name in ('cv2', 'skimage', 'skimage.io', 'PIL', 'PIL.Image', 'scipy', 'scipy.special'):
        try:
            importlib.import_module(name)
        except ImportError:
            mod = types.ModuleType(name)
            mod.io = mod.Image = mod.special = mod.expit = None     # the names the module imports from them
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location('reference_detector_utility', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference_utility(sys.argv[1])
    a, b = I.overlap_boxes()
    rec = {'digest': np.array(I.digest()), 'overlap': ref.compute_overlap(a.astype(np.float64), b.astype(np.float64))}
    assert rec['overlap'].dtype == np.float64 and rec['overlap'].shape == (len(a), len(b)) and np.isfinite(rec['overlap']).all()
    curves = I.ap_curves()
    rec['ap'] = np.array([ref.compute_ap(r, p) for r, p in curves], dtype=np.float64)
    out = os.path.join(HERE, 'golden', 'detection.npz')
    np.savez_compressed(out, **rec)
    print('wrote %s (%d bytes): overlap %s, %d curves, ap %s' % (out, os.path.getsize(out), rec['overlap'].shape, len(curves), rec['ap']))


if __name__ == '__main__':
    main()
