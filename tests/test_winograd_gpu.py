"""Winograd F(2x2,3x3) (conv_winograd.hpp: conv_wino_kernel) on the large-batch 3x3 / stride 1 layers of small even maps.

Option "wino" (include/dif.h) 1 is the default; 0 restores the direct f32 fma chain.  The two differ in the products the
kernel forms, not in precision (all f32): embeddings agree within 5e-6 absolute and a cosine gap below 1e-6, spot rows stay
within 1e-5 of the oracle, and the kernel's own results are bit-identical run to run.  Which layers take it depends only on
the layer shape and the batch of the launch (at least 64 images of 14 x 14)."""
import numpy as np
import pytest
import torch

from oracle import nets

pytestmark = pytest.mark.gpu
WINO = 'conv_wino_kernel'


def crops_u8(n, hw=112, seed=1234):
    return np.random.default_rng(seed).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)


def cosine_gap(a, b):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def wino_layers(model):
    return [name for name, kern, _ in model.op_table() if kern.startswith(WINO)]


@pytest.fixture(scope='module')
def r100(cuda):
    from deep_insight_face.networks.triplet import DifEmbedder
    model = DifEmbedder('iresnet100', 'v2', 512, (112, 112, 3), max_batch=512).init_synthetic(2024)
    model.set_input_transform(scale=1 / 255.)
    yield model, model.get_weights()
    model.close()


def _on_off(model, u8):
    dev = torch.from_numpy(u8).cuda()
    model.set_option('wino', 1)
    on = model.embed(dev)
    again = model.embed(dev)
    layers = wino_layers(model)
    model.set_option('wino', 0)
    off = model.embed(dev)
    layers_off = wino_layers(model)
    model.set_option('wino', 1)
    assert torch.equal(on, again)
    return on.cpu().numpy(), off.cpu().numpy(), layers, layers_off


@pytest.mark.parametrize('batch', [256, 512])
def test_iresnet100_wino_vs_direct(r100, batch):
    model, p = r100
    u8 = crops_u8(batch, seed=900 + batch)
    on, off, layers, layers_off = _on_off(model, u8)
    # the 14 x 14 stage: layer3_1 .. layer3_29 conv1 / conv2 except layer3_29_conv2 (sub-sampled output), layer4_0_conv1
    assert len(layers) == 58, layers
    assert not layers_off
    assert np.abs(on - off).max() <= 5e-6
    assert cosine_gap(on, off).max() < 1e-6
    rows = [0, batch // 2, batch - 1]
    want = nets.embed(u8[rows].astype(np.float32) / np.float32(255), p, 'iresnet100', 512, 'v2')
    assert cosine_gap(on[rows], want).max() < 1e-5


@pytest.mark.parametrize('batch', [1, 8, 12])
def test_small_batches_stay_direct(r100, batch):
    model, _ = r100
    model.predict_on_batch(crops_u8(batch, seed=batch))
    assert not wino_layers(model)


def test_iresnet50_odd_batch(cuda):
    """129 images: blocks of 64 Winograd tiles span images, the last block is partial."""
    from deep_insight_face.networks.triplet import DifEmbedder
    model = DifEmbedder('iresnet50', 'v2', 512, (112, 112, 3), max_batch=129).init_synthetic(7)
    model.set_input_transform(scale=1 / 255.)
    try:
        u8 = crops_u8(129, seed=5)
        on, off, layers, layers_off = _on_off(model, u8)
        assert layers and not layers_off
        assert np.abs(on - off).max() <= 5e-6
        assert cosine_gap(on, off).max() < 1e-6
    finally:
        model.close()


def test_gallery_match_same_rows(r100):
    """The 1M-row gallery match returns the same rows from both sets of embeddings."""
    from deep_insight_face import oneshot
    model, _ = r100
    u8 = crops_u8(256, seed=31)
    on, off, _, _ = _on_off(model, u8)
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
