"""Winograd F(2x2,3x3) on the narrow maps at level 2: the half-block shape (conv_winograd.hpp: conv_winow_kernel<32, 4>,
reported as `conv_wino_kernel<F(2x2,3x3),32 tiles x 64>`) against conv_wino_kernel's 64-tile block.

Option "wino" = 2 runs the maps of at most 16 x 16 in blocks of 32 tiles x 64 channels, two per CU; level 1, and level 2
under `dbg` bit 16777216 (the A/B switch), keep conv_wino_kernel.  Every accumulator sums the same products in the same
order in both shapes, so the three must agree bit for bit wherever no wide-map layer runs.  All cases use the single-lane
executor (DIF_STREAMS=1 while the net is finalized), so one launch sees the whole batch.

Cases (the smallest at which the tiling can go wrong): IResNet-50 at 65 images (3185 tiles = 99 blocks of 32 + 17: blocks
span images, the last is partial) and at 64 (wino::MIN_TILES exactly, 98 whole blocks), ResNet-50V2 at 65 (ReLU epilogue,
K = 8 steps), VGG16 at 65 (no shortcut, 512 channels, K = 32 steps), and ResNet-50V2 on a 64 x 96 input, whose narrow map is
8 x 12, at the smallest odd batch that admits it.  That batch is 131 (3136 tiles / 24 per image), which is above the wide
rule's 128 images: there level 2 also runs the 16 x 24 layers on conv_winow_kernel, which level 1 leaves direct, so level 2
and level 1 form other products and are held to the gate between levels (cosine gap below 1e-6) instead of bit equality;
level 2 against level 2 under the A/B bit -- the pair that differs in the narrow maps' block shape alone -- stays bit for bit.
"""
import pytest
import torch

import nonsquare_gates as gates
from test_nonsquare_gpu import Zoo, ran, wino_batch

pytestmark = pytest.mark.gpu

AB_BIT = 16777216                   # conv_winograd.hpp: launch_conv_wino
FULL = 'conv_wino_kernel<F(2x2,3x3),64 tiles x 64>'
HALF = 'conv_wino_kernel<F(2x2,3x3),32 tiles x 64>'


@pytest.fixture(scope='module')
def zoo(cuda):
    z = Zoo()
    yield z
    z.close()


def narrow_kernels(model):
    return [(name, kern) for name, kern, _ in model.op_table() if kern.startswith('conv_wino_kernel')]


CASES = [
    # arch, head, input, batch, at least this many narrow-map layers
    ('iresnet50', 'v2', (112, 112), 65, 20),
    ('iresnet50', 'v2', (112, 112), 64, 20),
    ('resnet', 'v2', (112, 112), 65, 3),
    ('vgg16', 'v2', (112, 112), 65, 3),
    ('resnet', 'v3', (64, 96), wino_batch((8, 12)), 3),
]


@pytest.mark.parametrize('arch,head,hw,n,at_least', CASES)
def test_half_block_equals_full_block(zoo, monkeypatch, arch, head, hw, n, at_least):
    m = zoo.net(arch, head, 512, hw, n, streams=1, monkeypatch=monkeypatch)
    dev = torch.from_numpy(zoo.pool(hw, n)).cuda()
    try:
        m.set_option('wino', 2)
        half = m.embed(dev)
        k_half, wide = narrow_kernels(m), ran(m, 'conv_winow_kernel')
        again = m.embed(dev)
        m.set_option('dbg', AB_BIT)
        ab = m.embed(dev)
        k_ab, wide_ab = narrow_kernels(m), ran(m, 'conv_winow_kernel')
        m.set_option('dbg', 0)
        m.set_option('wino', 1)
        one = m.embed(dev)
        k_one = narrow_kernels(m)
    finally:
        m.set_option('dbg', 0)
        m.set_option('wino', 2)
    print('%s %s n=%d: %d narrow-map layers, %d wide' % (arch, hw, n, len(k_half), len(wide)))
    assert len(k_half) >= at_least, k_half
    assert all(kern == HALF for _, kern in k_half), k_half
    assert [name for name, _ in k_ab] == [name for name, _ in k_half] == [name for name, _ in k_one]
    assert all(kern == FULL for _, kern in k_ab) and all(kern == FULL for _, kern in k_one), (k_ab, k_one)
    assert wide_ab == wide                                  # the A/B bit moves the narrow maps only
    assert bool(wide) == (n >= 128), wide
    assert torch.equal(half, again)
    assert torch.equal(half, ab)
    if not wide:
        assert torch.equal(half, one)
    else:
        gap = gates.cosine_gap(half.cpu().numpy(), one.cpu().numpy()).max()
        print('    level 2 / level 1 (wide layers differ): cosine gap %.2e' % gap)
        assert gap < 1e-6
    rows = [0, n // 2, n - 1]
    want = zoo.want(arch, head, 512, hw, rows, n)[0]
    gap = gates.cosine_gap(half.cpu().numpy()[rows], want).max()
    print('    against the oracle, rows %s: cosine gap %.2e' % (rows, gap))
    assert gap < 1e-5
