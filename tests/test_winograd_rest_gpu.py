"""Winograd F(2x2,3x3) on the layers the even-map rule left direct (conv_winograd.hpp: WinoX, wino_applies class 3,
reported as `conv_winox_kernel<F(2x2,3x3),32 tiles x 64,odd>` / `...,ysub>`), option "wino" = 2.

odd:  maps of at most 16 x 16 with an odd side (IResNet's 7 x 7 stage), tiled as the map zero-padded to even sides: the input
      points beyond the map load as zero and the output pixels beyond it are masked.
ysub: even maps whose first output keeps the even pixels only (the last 3x3 of IResNet's stages 1 to 3).
Both need level 2 and at least 128 images per launch; odd maps also at least 128 x 16 tiles.  `dbg` bit 33554432 (conv_run)
sends the class back to the direct kernels: the A/B switch.

Gates are the suite's own: cosine gap below 1e-6 between option settings of one net (a slipped index or an unmasked
eighth row is an O(1) error), below 1e-5 against the oracle, the map gate of nonsquare_gates for 'v3' maps, and bit
equality run to run and wherever the class is empty.  Whole small nets, single-lane executor unless the case says otherwise.
"""
import pytest
import torch

import nonsquare_gates as gates
from test_nonsquare_gpu import Zoo, ran

pytestmark = pytest.mark.gpu

AB_BIT = 33554432                   # conv.hip: conv_run
REST = 'conv_winox_kernel'
ODD = REST + '<F(2x2,3x3),32 tiles x 64,odd>'
YSUB = REST + '<F(2x2,3x3),32 tiles x 64,ysub>'
R50_ODD = ['layer4_1_conv1', 'layer4_1_conv2', 'layer4_2_conv1', 'layer4_2_conv2']          # 7 x 7, 512 -> 512
R50_YSUB = ['layer1_2_conv2', 'layer2_3_conv2', 'layer3_13_conv2']                          # 56 x 56, 28 x 28, 14 x 14


@pytest.fixture(scope='module')
def zoo(cuda):
    z = Zoo()
    yield z
    z.close()


def rest_kernels(model):
    return {name: kern for name, kern, _ in model.op_table() if kern.startswith(REST)}


def run_settings(m, dev, levels=(1, 0)):
    """Embeddings and kernel lists at level 2 (twice), at level 2 under the A/B bit and at `levels`; the net is left at
    level 2 without the bit.  tab[key] = (class-3 layers: kernel, conv_wino_kernel layers, conv_winow_kernel layers)."""
    out, tab = {}, {}

    def take(key):
        out[key] = m.embed(dev)
        tab[key] = (rest_kernels(m), ran(m, 'conv_wino_kernel'), ran(m, 'conv_winow_kernel'))
    try:
        m.set_option('wino', 2)
        take(2)
        out['again'] = m.embed(dev)
        m.set_option('dbg', AB_BIT)
        take('ab')
        m.set_option('dbg', 0)
        for lvl in levels:
            m.set_option('wino', lvl)
            take(lvl)
    finally:
        m.set_option('dbg', 0)
        m.set_option('wino', 2)
    return out, tab


def gap(a, b):
    return float(gates.cosine_gap(a.cpu().numpy(), b.cpu().numpy()).max())


def check_settings(label, out, tab, want_rest):
    """The assertions every case shares.  want_rest: {layer: kernel} the class must list at level 2 ({}: none)."""
    assert tab[2][0] == want_rest, tab[2][0]
    assert torch.equal(out[2], out['again'])
    assert tab['ab'][0] == {}, tab['ab'][0]                    # the bit empties the class ...
    assert tab['ab'][1:] == tab[2][1:]                         # ... and moves nothing else
    for lvl in (1, 0):
        if lvl in tab:
            assert tab[lvl][0] == {}, (lvl, tab[lvl][0])
    if not want_rest:
        assert torch.equal(out[2], out['ab'])
    g_ab = gap(out[2], out['ab'])
    g_0 = gap(out[2], out[0]) if 0 in out else float('nan')
    print('%s: %d odd + %d ysub layers; cosine gap level 2 / A-B bit %.2e, level 2 / level 0 %.2e'
          % (label, sum(k == ODD for k in want_rest.values()), sum(k == YSUB for k in want_rest.values()), g_ab, g_0))
    assert g_ab < 1e-6
    if 0 in out:
        assert g_0 < 1e-6


def r50_rest():
    return dict([(n, YSUB) for n in R50_YSUB] + [(n, ODD) for n in R50_ODD])


def test_iresnet50_129(zoo, monkeypatch):
    """129 images on one lane: 2 064 tiles on the 7 x 7 maps are 64 whole blocks and one half-filled, and a 32-tile block spans
    two images; the three y_sub layers run 56 x 56, 28 x 28 and 14 x 14."""
    n, hw = 129, (112, 112)
    m = zoo.net('iresnet50', 'v2', 512, hw, n, streams=1, monkeypatch=monkeypatch)
    dev = torch.from_numpy(zoo.pool(hw, n)).cuda()
    out, tab = run_settings(m, dev)
    want = r50_rest()
    assert list(tab[2][0]) == sorted(want, key=[name for name, _, _ in m.op_table()].index)
    check_settings('iresnet50 n=129', out, tab, want)
    rows = [0, 64, 128]
    g = gates.cosine_gap(out[2].cpu().numpy()[rows], zoo.want('iresnet50', 'v2', 512, hw, rows, n)[0]).max()
    print('    against the oracle, rows %s: cosine gap %.2e' % (rows, g))
    assert g < 1e-5


@pytest.mark.parametrize('n', [128, 127])
def test_iresnet50_threshold(zoo, monkeypatch, n):
    """128 images: the threshold exactly (2 048 tiles on 7 x 7, whole blocks).  127: the class is empty and the result is the
    run under the A/B bit, bit for bit."""
    hw = (112, 112)
    m = zoo.net('iresnet50', 'v2', 512, hw, 129, streams=1, monkeypatch=monkeypatch)
    dev = torch.from_numpy(zoo.pool(hw, 129)[:n]).cuda()
    out, tab = run_settings(m, dev, levels=(0,))
    check_settings('iresnet50 n=%d' % n, out, tab, r50_rest() if n == 128 else {})
    if n == 127:
        assert torch.equal(out[2], out['ab'])


def test_iresnet50_two_lanes_of_128(zoo, monkeypatch):
    """256 images with the default lanes: both lanes of 128 take the class; against one lane of 256."""
    n, hw = 256, (112, 112)
    two = zoo.net('iresnet50', 'v2', 512, hw, n)
    one = zoo.net('iresnet50', 'v2', 512, hw, n, streams=1, monkeypatch=monkeypatch)
    dev = torch.from_numpy(zoo.pool(hw, n)).cuda()
    a = two.embed(dev)
    assert rest_kernels(two) == r50_rest()
    b = one.embed(dev)
    assert rest_kernels(one) == r50_rest()
    g = gap(a, b)
    print('iresnet50 n=256, two lanes / one lane: cosine gap %.2e' % g)
    assert g < 1e-6
    assert torch.equal(a, two.embed(dev))


# ResNet-50V2 'v3' (ReLU epilogues, no y_sub): input, its conv4 map (3x3 / stride 1 layers conv4_block1..5_2_conv) and its
# conv5 map, which falls below 2 048 tiles at 129 images and stays direct
V3_CASES = [((112, 144), (7, 9), (4, 5)),        # both sides odd and unequal: 4 x 5 tiles
            ((128, 112), (8, 7), (4, 4)),        # W odd only
            ((112, 128), (7, 8), (4, 4))]        # H odd only


@pytest.mark.parametrize('hw,conv4,conv5', V3_CASES)
def test_resnet50v2_odd_maps(zoo, monkeypatch, hw, conv4, conv5):
    n = 129
    assert tuple(-(-s // 16) for s in hw) == conv4 and tuple(-(-s // 32) for s in hw) == conv5
    m = zoo.net('resnet', 'v3', 512, hw, n, streams=1, monkeypatch=monkeypatch)
    dev = torch.from_numpy(zoo.pool(hw, n)).cuda()
    out, tab = run_settings(m, dev)
    macs = {name: mac for name, _, mac in m.op_table()}
    want = {}
    for b in range(1, 6):                                      # (block 6's 3x3 is the stride 2 one)
        name = 'conv4_block%d_2_conv' % b
        assert macs[name] == 9 * 256 * 256 * conv4[0] * conv4[1], (name, macs[name])     # the map, from op_table()
        want[name] = ODD
    for b in range(1, 4):
        name = 'conv5_block%d_2_conv' % b
        assert macs[name] == 9 * 512 * 512 * conv5[0] * conv5[1], (name, macs[name])
    check_settings('resnet50v2 %s n=129 (conv4 %s)' % (hw, conv4), out, tab, want)
    assert not any(k == YSUB for k in tab[2][0].values())
    rows = [0, 64, 128]
    got = out[2].cpu().numpy()[rows]
    want_rows = zoo.want('resnet', 'v3', 512, hw, rows, n)[0]
    assert got.shape[1:3] == conv5
    assert gates.cosine_gap(got, want_rows).max() < 1e-5
    worst = gates.check_map(got, want_rows)                    # (against_oracle asks for a non-square last map: 4 x 4 here)
    print('    against the oracle, rows %s: max |got - oracle| / max |oracle| = %.2e' % (rows, worst))
