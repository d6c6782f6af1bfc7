"""The K-step of the four-wave Winograd shapes (conv_winograd.hpp: WinoW::B_HALVES): every B register set is re-filled in
two halves, each right behind the eight MFMAs that read it, so the loads of one set are in flight while its other half is
still being read, and the waits in front of the MFMAs count loads in an order the eight-wave shapes do not have.

What can go wrong is a wait that lets an MFMA read a register a load has not filled yet, or a load that overwrites one an
MFMA has not read: either shows as a forward that differs from the one before it, or from the same forward on the
eight-wave shapes, which keep whole sets and sum the same products in the same order (`dbg` 16777216: the narrow maps on
<64, 2, 1, false>; 65536: the wide maps on <64, 2, 2, true>).  So three forwards at level 2 must be equal to each other bit
for bit, and each equal to one forward under both bits.  The odd and y_sub forms have no 64-tile twin: they run the
four-wave loop in all four forwards and rest on the run-to-run equality here and on the digests of
test_winograd_bits_gpu.py / test_winograd_epilogue_gpu.py.

Cases, single lane (one launch sees the whole batch), 129 images (partial last blocks on every map):
  yolov3 on 32 x 64   conv_3 is 32 -> 64 channels: a K loop of two steps, the shortest wino_applies admits -- one pass of
                      the loop body, whose halves cross into the peeled last step -- with a shortcut
  iresnet50           K of 4 .. 32 steps, narrow, wide, odd and y_sub forms
  resnet50v2          K of 8 steps, ReLU epilogues, the 7 x 7 stage on the odd form
Each case asserts the set of Winograd kernels that ran in both configurations.
"""
import pytest
import torch

from test_nonsquare_gpu import Zoo

pytestmark = pytest.mark.gpu

TWIN_BITS = 16777216 | 65536        # conv_winograd.hpp: launch_conv_wino, launch_conv_winow
HALF, FULL = '32 tiles x 64', '64 tiles x 64'
NARROW, WIDE = 'conv_wino_kernel<F(2x2,3x3),%s>', 'conv_winow_kernel<F(2x2,3x3),%s>'
ODD, YSUB = 'conv_winox_kernel<F(2x2,3x3),%s,odd>' % HALF, 'conv_winox_kernel<F(2x2,3x3),%s,ysub>' % HALF
K2_LAYER, K2_MACS = 'conv_3', 9 * 32 * 64 * 16 * 32       # yolov3 on 32 x 64: Cin = 32 is two K-steps

CASES = {
    # name: (arch, head, emd, input, images, the forms without a twin that must run)
    'yolov3_129': ('yolov3', 'v3', 1, (32, 64), 129, []),
    'iresnet50_129': ('iresnet50', 'v2', 512, (112, 112), 129, [ODD, YSUB]),
    'resnet50v2_129': ('resnet', 'v2', 512, (112, 112), 129, [ODD]),
}


@pytest.fixture(scope='module')
def zoo(cuda):
    z = Zoo()
    yield z
    z.close()


def wino_kernels(model):
    return {name: k for name, k, _ in model.op_table() if k.startswith(('conv_wino_kernel', 'conv_winow_kernel', 'conv_winox_kernel'))}


def outputs(y):
    return list(y) if isinstance(y, (list, tuple)) else [y]


def equal(a, b):
    a, b = outputs(a), outputs(b)
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize('name', list(CASES))
def test_kstep_run_to_run_and_against_the_eight_wave_shapes(zoo, monkeypatch, name):
    arch, head, emd, hw, n, untwinned = CASES[name]
    m = zoo.net(arch, head, emd, hw, n, streams=1, monkeypatch=monkeypatch)
    dev = torch.from_numpy(zoo.pool(hw, n)).cuda()
    try:
        m.set_option('wino', 2)
        runs = [[t.clone() for t in outputs(m.embed(dev))] for _ in range(3)]
        k_new = wino_kernels(m)
        m.set_option('dbg', TWIN_BITS)
        twin = [t.clone() for t in outputs(m.embed(dev))]
        k_twin = wino_kernels(m)
    finally:
        m.set_option('dbg', 0)
        m.set_option('wino', 2)
    print('%s: %d Winograd layers: %s' % (name, len(k_new), ', '.join(sorted(set(k_new.values())))))
    assert sorted(set(k_new.values())) == sorted([NARROW % HALF, WIDE % HALF] + untwinned), k_new
    assert sorted(set(k_twin.values())) == sorted([NARROW % FULL, WIDE % FULL] + untwinned), k_twin
    assert list(k_new) == list(k_twin)
    if arch == 'yolov3':
        macs = {nm: mac for nm, _, mac in m.op_table()}
        assert k_new.get(K2_LAYER) == WIDE % HALF and macs[K2_LAYER] == K2_MACS, (k_new.get(K2_LAYER), macs.get(K2_LAYER))
    assert equal(runs[0], runs[1]) and equal(runs[0], runs[2])
    for r in runs:
        assert equal(r, twin)
