"""CPU emulation of the Winograd kernels' arithmetic (F(2x2,3x3), f32) inside the NumPy oracle.

    python tools/winograd_error.py [n_crops] [arch] [max_map] [max_odd_map]

oracle/nets.py's conv2d is swapped, for this process only, for one that sends the layers conv_winograd.hpp admits by
shape (3x3 / stride 1 / pad 1, even maps of at most max_map x max_map, Cin % 32 == 0, Cout % 64 == 0) through the kernels'
order of operations.  max_map = 16 (default) is option "wino" = 1 (conv_wino_kernel); 112 is level 2 (conv_winow_kernel
on the wider maps; the layers with a sub-sampled first output are emulated too: the GPU runs them from 128 images per
launch up).  max_odd_map = 16 (default 0: none) adds the maps of at most that size with an odd side, zero-padded to even
sides and cropped -- what the kernel's out-of-range loads and masked stores do (IResNet's 7 x 7 stage).  The order of operations: U = G g G^T in float64 rounded once, V = B^T d B and Y = A^T M A in float32, the 16 GEMMs in float32.  It
reports the embedding difference against the direct f32 oracle, and both against a float64 oracle run.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import nets  # noqa: E402

_spec = importlib.util.spec_from_file_location(
    'dif_weights', os.path.join(ROOT, 'deep-insight-face_amd', 'deep_insight_face', 'networks', 'weights.py'))
weights = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(weights)

G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
direct_conv2d = nets.conv2d
taken = []
max_map = 16
max_odd_map = 0


def bt(a, axis):
    """B^T along one axis of length 4: (x0 - x2, x1 + x2, x2 - x1, x1 - x3)."""
    x0, x1, x2, x3 = (np.take(a, i, axis=axis) for i in range(4))
    return np.stack([x0 - x2, x1 + x2, x2 - x1, x1 - x3], axis=axis)


def wino_conv2d(x, w, bias=None, stride=1, pad=(0, 0, 0, 0)):
    kh, kw, cin, cout = w.shape
    n, h, wd, _ = x.shape
    if not (kh == 3 and kw == 3 and stride == 1 and tuple(pad) == (1, 1, 1, 1)
            and cin % 32 == 0 and cout % 64 == 0 and x.dtype == np.float32):
        return direct_conv2d(x, w, bias, stride, pad)
    if h % 2 or wd % 2:
        if h > max_odd_map or wd > max_odd_map:
            return direct_conv2d(x, w, bias, stride, pad)
        taken.append((h, wd, cin, cout))
        y = wino_even(np.pad(x, ((0, 0), (0, h % 2), (0, wd % 2), (0, 0))), w)[:, :h, :wd]
    elif h > max_map or wd > max_map:
        return direct_conv2d(x, w, bias, stride, pad)
    else:
        taken.append((h, wd, cin, cout))
        y = wino_even(x, w)
    if bias is not None:
        y = y + bias
    return y


def wino_even(x, w):
    cin, cout = w.shape[2:]
    n, h, wd, _ = x.shape
    u = np.einsum('ik,klco,jl->ijco', G, w.astype(np.float64), G).astype(np.float32)      # [4][4][Cin][Cout]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    th, tw = h // 2, wd // 2
    d = np.empty((n, th, tw, 4, 4, cin), np.float32)
    for r in range(4):
        for c in range(4):
            d[:, :, :, r, c, :] = xp[:, r:r + 2 * th:2, c:c + 2 * tw:2, :]
    v = bt(bt(d, 3), 4)                                                                     # rows, then columns
    m = np.einsum('ntsijc,ijco->ntsijo', v, u, dtype=np.float32, optimize=True)
    s0 = m[:, :, :, 0] + m[:, :, :, 1] + m[:, :, :, 2]
    s1 = m[:, :, :, 1] - m[:, :, :, 2] - m[:, :, :, 3]
    y = np.empty((n, th, 2, tw, 2, cout), np.float32)
    for a, s in enumerate((s0, s1)):
        y[:, :, a, :, 0] = s[:, :, :, 0] + s[:, :, :, 1] + s[:, :, :, 2]
        y[:, :, a, :, 1] = s[:, :, :, 1] - s[:, :, :, 2] - s[:, :, :, 3]
    return y.reshape(n, h, wd, cout)


def main():
    global max_map, max_odd_map
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    arch = sys.argv[2] if len(sys.argv) > 2 else 'iresnet100'
    max_map = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    max_odd_map = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    p = {k: np.asarray(v, np.float32) for k, v in weights.synth_params(nets.iresnet_spec(arch), 2024).items()}
    x = np.random.default_rng(1234).integers(0, 256, (n, 112, 112, 3)).astype(np.float32) / np.float32(255)
    direct = nets.embed(x, p, arch, 512, 'v2')
    nets.conv2d = wino_conv2d
    try:
        wino = nets.embed(x, p, arch, 512, 'v2')
    finally:
        nets.conv2d = direct_conv2d
    exact = nets.embed(x.astype(np.float64), nets.cast_params(p, np.float64), arch, 512, 'v2')

    def gap(a, b):
        a, b = a.astype(np.float64), b.astype(np.float64)
        return (1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))).max()

    print('%s, %d crops (seed 1234), He-normal weights (seed 2024); even maps up to %d x %d, odd up to %d x %d; Winograd layers: %d of shape %s'
          % (arch, n, max_map, max_map, max_odd_map, max_odd_map, len(taken), sorted(set(taken))))
    print('winograd f32 vs direct f32: max |diff| %.3e   cosine gap %.3e' % (np.abs(wino - direct).max(), gap(wino, direct)))
    print('direct f32   vs float64   : max |diff| %.3e   cosine gap %.3e' % (np.abs(direct - exact).max(), gap(direct, exact)))
    print('winograd f32 vs float64   : max |diff| %.3e   cosine gap %.3e' % (np.abs(wino - exact).max(), gap(wino, exact)))


if __name__ == '__main__':
    main()
