"""Winograd F(2x2,3x3) on the wide maps (conv_winograd.hpp: conv_winow_kernel), option "wino" = 2, the default.

Level 2 is level 1 (conv_wino_kernel on the 14 x 14 stage) plus the 3x3 / stride 1 layers on even maps above 16 x 16 up to
112 x 112 -- IResNet's 28 x 28, 56 x 56 and 112 x 112 stages -- from 128 images per launch up.  Level 0 is the direct f32
fma chain.  All f32; the levels differ in the products formed.  Gates: cosine gap to level 0 below 1e-6 (the project's
gate between settings), spot rows within 1e-5 of the oracle, bit-identical run to run, and max |level 2 - level 0| at most
3x max |level 1 - level 0| on the same crops (the CPU emulation, tools/winograd_error.py, gives 1.5 - 1.9x; the margin
covers the spread of a maximum over 512 x 512 values).  Measured on MI355X: profiles/r07_wide_levels.txt."""
import numpy as np
import pytest
import torch

from oracle import nets

pytestmark = pytest.mark.gpu
WINO = 'conv_wino_kernel'
WIDE = 'conv_winow_kernel'

# IResNet-100's 3x3 / stride 1 layers on the wide maps, without the two whose first output is written at even pixels
# only (layer1_2_conv2, layer2_12_conv2; they stay direct): 112 x 112, 56 x 56 (64 in), 28 x 28 (128 in)
R100_WIDE = (['layer1_0_conv1'] + ['layer1_%d_conv%d' % (b, c) for b in (1, 2) for c in (1, 2)][:-1] + ['layer2_0_conv1']
             + ['layer2_%d_conv%d' % (b, c) for b in range(1, 13) for c in (1, 2)][:-1] + ['layer3_0_conv1'])


def crops_u8(n, hw=112, seed=1234):
    return np.random.default_rng(seed).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)


def cosine_gap(a, b):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def layers(model, prefix):
    return [name for name, kern, _ in model.op_table() if kern.startswith(prefix)]


def run_levels(model, u8, levels=(2, 1, 0)):
    """Embeddings and (conv_wino_kernel layers, conv_winow_kernel layers) per level; the net is left at level 2."""
    dev = torch.from_numpy(u8).cuda()
    out, tab = {}, {}
    try:
        for lvl in levels:
            model.set_option('wino', lvl)
            a = model.embed(dev)
            if lvl == 2:
                assert torch.equal(a, model.embed(dev))
            out[lvl] = a.cpu().numpy()
            tab[lvl] = (layers(model, WINO), layers(model, WIDE))
    finally:
        model.set_option('wino', 2)
    return out, tab


@pytest.fixture(scope='module')
def r100(cuda):
    from deep_insight_face.networks.triplet import DifEmbedder
    model = DifEmbedder('iresnet100', 'v2', 512, (112, 112, 3), max_batch=512).init_synthetic(2024)
    model.set_input_transform(scale=1 / 255.)
    yield model, model.get_weights()
    model.close()


@pytest.mark.parametrize('batch', [256, 512])
def test_iresnet100_levels(r100, batch):
    model, p = r100
    u8 = crops_u8(batch, seed=900 + batch)
    out, tab = run_levels(model, u8)
    assert tab[2][1] == R100_WIDE, tab[2][1]
    assert len(tab[2][0]) == 58 and tab[1][0] == tab[2][0]
    assert not tab[1][1] and tab[0] == ([], [])
    d2, d1 = np.abs(out[2] - out[0]).max(), np.abs(out[1] - out[0]).max()
    print('batch %d: max |level 2 - level 0| %.3e, max |level 1 - level 0| %.3e, cosine gap level 2 / level 0 %.3e'
          % (batch, d2, d1, cosine_gap(out[2], out[0]).max()))
    assert cosine_gap(out[2], out[0]).max() < 1e-6
    assert d2 <= 3 * d1, (d2, d1)
    rows = [0, batch // 2, batch - 1]
    want = nets.embed(u8[rows].astype(np.float32) / np.float32(255), p, 'iresnet100', 512, 'v2')
    assert cosine_gap(out[2][rows], want).max() < 1e-5


def test_wide_maps_in_64_tile_blocks_equal_32_tile_blocks(r100):
    """`dbg` bit 65536 runs the wide maps in the 64-tile block shape: the same layers, the same bits."""
    model, _ = r100
    dev = torch.from_numpy(crops_u8(256, seed=77)).cuda()
    try:
        model.set_option('wino', 2)
        half = model.embed(dev)
        tab_half = [(name, kern) for name, kern, _ in model.op_table() if kern.startswith(WIDE)]
        model.set_option('dbg', 65536)
        full = model.embed(dev)
        tab_full = [(name, kern) for name, kern, _ in model.op_table() if kern.startswith(WIDE)]
    finally:
        model.set_option('dbg', 0)
        model.set_option('wino', 2)
    assert [name for name, _ in tab_half] == R100_WIDE and [name for name, _ in tab_full] == R100_WIDE
    assert all(kern == WIDE + '<F(2x2,3x3),32 tiles x 64>' for _, kern in tab_half), tab_half
    assert all(kern == WIDE + '<F(2x2,3x3),64 tiles x 64>' for _, kern in tab_full), tab_full
    assert torch.equal(half, full)


@pytest.mark.parametrize('arch,batch,wide', [
    ('iresnet50', 258, True),     # lanes of 129: just above the threshold; 129 x 196 tiles, blocks span images, last one partial
    ('iresnet50', 254, False),    # lanes of 127: just below it, the wide layers stay direct
    ('iresnet50', 331, True),     # lanes of 166 and 165: 28 x 28 tiles per lane not a multiple of 32
    ('resnet', 258, True),        # ResNet-50V2: ReLU epilogues, 28 x 28 layers
    ('vgg16', 258, True),         # VGG16: ReLU, no shortcut, 112 x 112 .. 28 x 28 layers
])
def test_geometry_cases(cuda, arch, batch, wide):
    from deep_insight_face.networks.triplet import DifEmbedder
    model = DifEmbedder(arch, 'v2', 512, (112, 112, 3), max_batch=batch).init_synthetic(7)
    model.set_input_transform(scale=1 / 255.)
    try:
        out, tab = run_levels(model, crops_u8(batch, seed=5 + batch))
        if not wide:
            assert not tab[2][1]
        elif arch == 'iresnet50':
            assert tab[2][1]
        assert tab[0] == ([], []) and not tab[1][1] and tab[1][0] == tab[2][0]
        d2, d1 = np.abs(out[2] - out[0]).max(), np.abs(out[1] - out[0]).max()
        print('%s %d: %d wide layers, max |level 2 - level 0| %.3e, max |level 1 - level 0| %.3e, cosine gap %.3e'
              % (arch, batch, len(tab[2][1]), d2, d1, cosine_gap(out[2], out[0]).max()))
        assert cosine_gap(out[2], out[0]).max() < 1e-6      # an indexing slip is an O(1) error
        if tab[1][0]:                                       # the 3x rule needs level 1 to differ from level 0
            assert d2 <= 3 * d1, (d2, d1)
        if not tab[2][1]:
            assert np.array_equal(out[2], out[1])
    finally:
        model.close()


def test_batch_96_per_launch_stays_on_conv_tn_kernel(cuda):
    """IResNet-50 at 192 with default options is two lanes of 96 images: below the wide rule's 128 images per launch."""
    from deep_insight_face.networks.triplet import DifEmbedder
    model = DifEmbedder('iresnet50', 'v2', 512, (112, 112, 3), max_batch=192).init_synthetic(15)
    model.set_input_transform(scale=1 / 255.)
    try:
        model.embed(torch.from_numpy(crops_u8(192, seed=48)).cuda())
        assert not layers(model, WIDE)
        assert layers(model, 'conv_tn_kernel')
        assert layers(model, WINO)                          # 96 images of 14 x 14 are above level 1's threshold
    finally:
        model.close()


@pytest.mark.parametrize('batch', [1, 8, 12])
def test_small_batches_stay_direct(r100, batch):
    model, _ = r100
    model.predict_on_batch(crops_u8(batch, seed=batch))
    assert not layers(model, WINO) and not layers(model, WIDE)


def test_level_out_of_range_is_refused(r100):
    model, _ = r100
    with pytest.raises(ValueError):
        model.set_option('wino', 3)


def test_gallery_match_same_rows(r100):
    """The 1M-row gallery match returns the same rows from level 2's and level 0's embeddings."""
    from deep_insight_face import oneshot
    model, _ = r100
    out, tab = run_levels(model, crops_u8(256, seed=31), levels=(2, 0))
    assert tab[2][1]
    on, off = out[2], out[0]
    rng = np.random.default_rng(3)
    gal = rng.standard_normal((1 << 20, 512)).astype(np.float32)
    gal /= np.linalg.norm(gal, axis=1, keepdims=True)
    plant = rng.choice(gal.shape[0], 128, replace=False)
    gal[plant] = on[:128] + 0.02 * rng.standard_normal((128, 512)).astype(np.float32)
    gal[plant] /= np.linalg.norm(gal[plant], axis=1, keepdims=True)
    idx_on, _ = oneshot.match(on, gal, 1)
    idx_off, _ = oneshot.match(off, gal, 1)
    assert np.array_equal(idx_on, idx_off)
    assert np.array_equal(idx_on[:128], plant)
