"""Every network that admits a non-square input, built with H != W and compared with the oracle.

`dif_net_create` takes in_h and in_w separately and the convolution dispatch is full of arithmetic that tells the two
apart (W + 2 / H + 1 halo strides, W / 8 tile columns, the 16 x 16 stem tiles, the Winograd (H / 2) x (W / 2) tiling);
every other network test is square, where a swapped pair computes the right answer.  Inputs are seeded random uint8
(no symmetry between the axes), weights `init_synthetic`.  Each case reads `op_table()` and asserts the family it is
named for did run on a backbone layer whose map is H != W: in the 'v3' nets every backbone map is non-square; the GDC
nets end on a square 3 x 3 map, and ResNet50V2's conv5 stack, which runs on it, is left out of that assertion.

Gates (nonsquare_gates.py; the square tests' own): against the oracle atol = 2e-4 * max |want|, rtol = 2e-3, embeddings
also cosine gap < 1e-5; between option settings of one net the gate of the square parity test of that family pair.
tests/test_oracle_nets.py::test_gates_reject_one_transposed_layer shows the oracle gates reject ONE transposed layer
(max error 0.11 - 0.40 of max |want|, three orders above the gate).

The GDC head ('v2') is built on a square map only (the reference's DepthwiseConv2D(int(nn.shape[1])) is a square
kernel): it is run on a non-square INPUT whose last map is 3 x 3, and H' != W' is refused at dif_net_create
(test_refused_shapes).  gdc_tail_* / dwfull_kernel read the map as H' * W' taps: no KH != KW form exists.

Measured on the MI355X, max |got - oracle| / max |oracle| (the gate is 2e-4), beside the float32-vs-float64 oracle on the
same input, 6e-7 on VGG16 48 x 80:
  default dispatch, n = 1 / 3 / 12 (conv_mt_kernel, conv_sk_kernel, conv_skp_kernel, stems, pools, dwconv, upsample)  6e-7 .. 2e-6
  large-batch families on 48 x 80 / 80 x 48 / 64 x 96 / 96 x 64 inputs (conv_t2 / conv_tn / conv_bdp / conv_pipe / patch forms)  8e-7 .. 2e-6
  Winograd level 2 at 129 / 131 images (conv_winow_kernel + conv_wino_kernel)                                             1.2e-6 .. 1.9e-6
  split-bf16: three terms 1.4e-6 .. 2.0e-6, two terms 9.3e-6 .. 1.8e-5
  two lanes, 65 images: 2.3e-6 (ResNet50V2), 3.1e-6 (YOLOv3); two lanes against one 2.5e-6 .. 3.3e-6, cosine gap 3e-12
Between option settings of one net (test_large_batch_families_vs_oracle), max |on - off| / max(max |map|, 1) on the 2 x 3 /
1 x 2 x C maps: t2, patch2d, bd 0 (bit-identical); patch 0 .. 1.1e-6; stem 6.5e-7 .. 1.5e-6 (gate 2e-5); tn 1.8e-6 .. 2.9e-6;
bdp 2.4e-6 .. 2.7e-6.  bdp and tn are the two pairs that re-split a tile's K range (stream-K partial sums in another
order), and their differences are of the size of the rounding the yardstick shows: 4 .. 5 times the float32-vs-float64
oracle difference (6e-7) after 13 .. 50 layers, the same size as GPU-vs-oracle itself (1e-6 .. 2e-6) and as two lanes against
one (2.5e-6 .. 3.3e-6); a slipped index gives 0.1 .. 0.4.  Both sides of every pair are within the oracle gate.  The square
tests state the bdp / t2 / tn gates as absolute differences between unit-norm GDC embeddings (largest element about 0.15:
2e-6 there is about 1.3e-5 of the largest element), so those pairs are held to them on GDC nets
(test_large_batch_families_agree), not to a figure relative to a ReLU map's maximum, which no square test sets.
"""
import contextlib

import numpy as np
import pytest
import torch

import nonsquare_gates as gates
from oracle import detector as odet
from oracle import nets

pytestmark = pytest.mark.gpu

DEFAULTS = {'pipe': 1, 'bdp': 1, 'stem': 1, 'patch': 1, 'patch2d': 1, 'bd': 1, 't2': 1, 'tn': 1, 'sk2': 1, 'mt': 1,
            'wino': 2, 'dbg': 0}
HEAD_OPS = ('head_', 'v1_', 'sv2_', 'embeddings', 'norm_embedding')
POOL = 40                                    # images per seeded pool; a case takes the first n


@contextlib.contextmanager
def options(model, **kw):
    try:
        for k, v in kw.items():
            model.set_option(k, v)
        yield model
    finally:
        for k in kw:
            model.set_option(k, DEFAULTS[k])


def ran(model, family):
    """Backbone layers whose last launch was a kernel of this family: `family` is any part of the kernel's name
    ('conv_tn_kernel', 'patch8x8', '+Bdirect').  The caller knows which of its net's layers run on a non-square map."""
    return [name for name, kern, _ in model.op_table() if family in kern and not name.startswith(HEAD_OPS)]


def families(model):
    return sorted({kern.split('<')[0] for _, kern, _ in model.op_table()})


def as_list(t):
    return [u.cpu().numpy() for u in t] if isinstance(t, list) else [t.cpu().numpy()]


class Zoo:
    """Nets, inputs and oracle rows shared by the module: one net per (arch, head, shape, max_batch, compute, lanes),
    one oracle row per (arch, head, shape, image)."""

    def __init__(self):
        self.nets, self.weights, self.pools, self.rows = {}, {}, {}, {}

    def net(self, arch, head, emd, hw, max_batch, compute='f32', streams=None, monkeypatch=None):
        from deep_insight_face.networks.triplet import DifEmbedder
        key = (arch, head, emd, hw, max_batch, compute, streams)
        if key not in self.nets:
            if streams is not None:
                monkeypatch.setenv('DIF_STREAMS', str(streams))
            m = DifEmbedder(arch, head, emd, hw + (3,), max_batch=max_batch, compute=compute).init_synthetic(2024)
            m.set_input_transform(scale=1 / 255.)
            m._finalize()                                         # the lane count is read from the environment here
            if streams is not None:
                monkeypatch.delenv('DIF_STREAMS')
            self.nets[key] = m
            self.weights.setdefault((arch, head, emd, hw), m.get_weights())
        return self.nets[key]

    def pool(self, hw, n=POOL):
        key = (hw, n)
        if key not in self.pools:
            self.pools[key] = gates.frames_u8(n, hw, seed=hw[0] * 1000 + hw[1] + n)
        return self.pools[key]

    def want(self, arch, head, emd, hw, rows, n_pool=POOL, dtype=np.float32):
        """Oracle outputs of the pool's images `rows`: a list of arrays (one per network output), [len(rows), ...]."""
        p = self.weights[(arch, head, emd, hw)]
        if dtype != np.float32:
            p = nets.cast_params(p, dtype)
        missing = [r for r in rows if (arch, head, emd, hw, n_pool, dtype, r) not in self.rows]
        if missing:
            x = gates.scaled(self.pool(hw, n_pool)[missing]).astype(dtype)
            y = odet.yolov3_forward(x, p) if arch == 'yolov3' else [nets.embed(x, p, arch, emd, head)]
            for i, r in enumerate(missing):
                self.rows[(arch, head, emd, hw, n_pool, dtype, r)] = [t[i] for t in y]
        got = [self.rows[(arch, head, emd, hw, n_pool, dtype, r)] for r in rows]
        return [np.stack([g[o] for g in got]) for o in range(len(got[0]))]

    def close(self):
        for m in self.nets.values():
            m.close()


@pytest.fixture(scope='module')
def zoo(cuda):
    z = Zoo()
    yield z
    z.close()


def out_hw(arch, hw):
    """The maps a 'v3' net returns: (H', W') per output."""
    if arch == 'yolov3':
        return [(hw[0] // s, hw[1] // s) for s in (32, 16, 8)]
    return [tuple(s // 32 if arch == 'vgg16' else -(-s // 32) for s in hw)]


def against_oracle(zoo, label, arch, head, emd, hw, got, rows, n_pool=POOL, f64_rows=()):
    """got: list of arrays (one per output) for the pool's images `rows`.  Prints the worst error, and beside it the
    float32-vs-float64 oracle difference on `f64_rows` (rounding's own size on this input)."""
    want = zoo.want(arch, head, emd, hw, rows, n_pool)
    check = gates.check_map if head == 'v3' else gates.check_embedding
    if head == 'v3':
        assert [g.shape[1:3] for g in got] == out_hw(arch, hw) and all(g.shape[1] != g.shape[2] for g in got)
    worst = max(check(g, w) for g, w in zip(got, want))
    line = '%s: max |got - oracle| / max |oracle| = %.2e' % (label, worst)
    if f64_rows:
        w32 = zoo.want(arch, head, emd, hw, list(f64_rows), n_pool)
        w64 = zoo.want(arch, head, emd, hw, list(f64_rows), n_pool, np.float64)
        line += ', oracle f32 vs f64 %.2e' % max(gates.worst(a, b) for a, b in zip(w32, w64))
    print(line)
    return worst


# ------------------------------------------------------------------------------------------- 1. default dispatch
SMALL = [('vgg16', 'v3', 512, (48, 80)), ('vgg16', 'v3', 512, (80, 48)), ('resnet', 'v3', 512, (64, 96)),
         ('resnet', 'v3', 512, (96, 64)), ('resnet', 'v3', 512, (72, 104)), ('mobilenet', 'v3', 512, (64, 96)),
         ('mobilenet', 'v3', 512, (75, 41)), ('yolov3', 'v3', 1, (64, 160)), ('yolov3', 'v3', 1, (160, 64))]
OWN_KERNELS = {'vgg16': ('maxpool_kernel',), 'resnet': ('maxpool_kernel', 'stem_mfma_kernel'), 'mobilenet': ('dwconv_kernel',),
               'yolov3': ('upsample2_kernel', 'stem3x3_kernel')}


def small_batch_family(arch, n):
    """What the library's own choice is at these sizes (read from op_table on the MI355X): one image -> conv_mt_kernel;
    3 -> split-K on VGG16 and the detector, ResNet50V2's short pointwise layers still conv_mt_kernel / conv_igemm_kernel;
    12 -> split-K with and without the halo patch.  MobileNetV2's K loops are too short for split-K at any batch
    (sk2_plan: at least 8 K-steps): its 1x1 layers stay on conv_mt_kernel, the 16- / 24- / 32-channel ones on the
    128 x 32 tile of conv_igemm_kernel."""
    if arch == 'mobilenet':
        return ['conv_mt_kernel', 'conv_igemm_kernel<128x32', 'dwconv_kernel']
    if n == 1:
        return ['conv_mt_kernel']
    if arch == 'resnet' and n == 3:
        return ['conv_mt_kernel', 'conv_igemm_kernel<64x64,pointwise']
    if arch == 'vgg16':
        return ['conv_sk_kernel', 'conv_skp_kernel'] if n == 3 else ['conv_skp_kernel']
    return ['conv_sk_kernel', 'conv_skp_kernel'] if n == 12 else ['conv_sk_kernel']


@pytest.mark.parametrize('n', [1, 3, 12])
@pytest.mark.parametrize('arch,head,emd,hw', SMALL)
def test_default_dispatch_vs_oracle(zoo, arch, head, emd, hw, n):
    """The kernels the library picks by itself at the reference's call shapes: one image (conv_mt_kernel, 16 x 16 tiles),
    3 and 12 (conv_sk_kernel / conv_skp_kernel + reduce), every element of every output map against the oracle.  Covers
    the input conversion, the stems' ragged 16 x 16 tiles (72 x 104: 36 x 52 out), maxpool / depthwise / upsample and the
    detector's concat views on H != W maps; 72 x 104 and 75 x 41 leave odd maps (9 x 13 .. 3 x 4; 38 x 21 .. 3 x 2)."""
    m = zoo.net(arch, head, emd, hw, 12)
    got = as_list(m.embed(torch.from_numpy(zoo.pool(hw)[:n]).cuda()))
    fam = families(m)
    for k in small_batch_family(arch, n):
        assert ran(m, k), (k, fam)
    for k in OWN_KERNELS[arch] + ('input_convert_kernel',):
        assert k in fam, (k, fam)
    against_oracle(zoo, '%s %s n=%d default' % (arch, hw, n), arch, head, emd, hw, got, list(range(n)), f64_rows=(0,) if n == 1 else ())


# ------------------------------------------------------------------------------------------- 2. stream-K and the large-batch families
def _pair(m, x, on, off, family, label, square=()):
    """Embed with option set `on` (the family must run on a layer whose map is non-square -- `square` names the
    beginnings of the layers that are not -- and twice bit-identically) and `off` (it must run nowhere).  Returns the two
    results as lists of arrays."""
    with options(m, sk2=0, mt=0, **on):
        a = as_list(m.embed(x))
        layers = [name for name in ran(m, family) if not name.startswith(tuple(square))] if square else ran(m, family)
        a2 = as_list(m.embed(x))
    with options(m, sk2=0, mt=0, **off):
        b = as_list(m.embed(x))
        layers_off = ran(m, family)
    assert layers, (label, family, sorted({k for _, k, _ in m.op_table()}))
    assert not layers_off, (label, layers_off)
    assert all(np.array_equal(u, v) for u, v in zip(a, a2)), label
    print('%s: %s on %s' % (label, family, layers))
    return a, b


# name: (options on, options off, what the family's kernel names hold, the square parity test's gate for the pair) --
# tests/test_embed_gpu.py: test_pipelined_kernel_equals_plain_kernel 2e-6, test_deferred_epilogue_kernel_equals_plain_kernel
# 2e-6, test_two_subtile_kernel_equals_plain_kernel 2e-6, test_wide_tile_kernel_equals_deferred_epilogue_kernel 5e-6,
# test_stem_kernels_equal_general_kernel 2e-5.  'patch' / 'patch2d' / 'bd' have no square twin: the same products, and the
# stream-K split of a tile's K range may move with the kernel's resident blocks -- conv_tn_kernel's case and gate, 5e-6.
AB = {
    'pipe':    (dict(stem=0, pipe=1), dict(stem=0, pipe=0), 'conv_pipe_kernel', 2e-6),   # (stem = 0: the 3-channel layer, gather form)
    'bdp':     (dict(bdp=2), dict(bdp=0), 'conv_bdp_kernel', 2e-6),
    't2':      (dict(t2=1), dict(t2=0), 'conv_t2_kernel', 2e-6),
    't2@gather': (dict(patch=0, t2=1), dict(patch=0, t2=0), 'conv_t2_kernel', 2e-6),     # ResNet's 16 x 24 maps once the linear patch is off
    'tn':      (dict(tn=1, dbg=512), dict(tn=0), 'conv_tn_kernel', 5e-6),
    'patch2d': (dict(patch2d=1), dict(patch2d=0), 'patch8x8', 5e-6),
    'patch':   (dict(patch=1), dict(patch=0), 'patch1', 5e-6),                           # patch128 / patch168: the linear halo patch
    'bd':      (dict(bd=1), dict(bd=0), '+Bdirect', 5e-6),
    'stem':    (dict(stem=1), dict(stem=0), 'stem_mfma_kernel', 2e-5),
}
MAP_GATED = ('pipe', 'stem')          # the pairs whose square test holds MAPS (YOLOv3's) to tol * max(max |map|, 1)
VGG_AB = ('pipe', 'bdp', 't2', 'tn', 'patch2d', 'patch', 'bd', 'stem')
VGG_NO_BDP = tuple(k for k in VGG_AB if k != 'bdp')    # 80 x 48: conv_tn_kernel / conv_t2_kernel take every layer 'bdp' = 2 would
RES_AB = ('bdp', 't2@gather', 'tn', 'patch', 'bd', 'stem')      # (no 8x8-tile layer by default: every map fits the linear patch)


@pytest.mark.parametrize('arch,hw,n,pairs', [('vgg16', (48, 80), 37, VGG_AB), ('vgg16', (80, 48), 37, VGG_NO_BDP),
                                             ('vgg16', (48, 80), 5, VGG_AB[1:]),      # (conv_pipe_kernel needs 1536 tiles: not at 5 images)
                                             ('resnet', (64, 96), 37, RES_AB), ('resnet', (96, 64), 9, RES_AB)])
def test_large_batch_families_vs_oracle(zoo, arch, hw, n, pairs):
    """'sk2' = 0, 'mt' = 0: the persistent stream-K grid and the large-batch families on odd batches (ragged last tiles, tiles
    spanning two images), every map H != W.  VGG16 48 x 80: 8-aligned maps 48 x 80 and 24 x 40 (conv_t2_kernel, the 8x8-tile
    patch of conv_bdp_kernel / conv_igemm_kernel), 12 x 20 .. 3 x 5 on the linear halo patch (conv_tn_kernel, conv_igemm_kernel);
    ResNet50V2 64 x 96: 16 x 24 (conv_tn_kernel patch256), 8 x 12, 4 x 6 (patch168 / patch128, conv_bdp_kernel), the stem's
    32 x 48 output.  Each family's output AND its fall-back's are held to the oracle on the first and last image, every element
    of the map.  Against each other the two are held to the square test's gate where that test states it for maps ('pipe',
    'stem'); the other pairs' gates are stated on the GDC embedding: test_large_batch_families_agree.  The general epilogue
    ('dbg' 1024) against the lean one bit for bit (test_lean_epilogue_equals_general_epilogue)."""
    m = zoo.net(arch, 'v3', 512, hw, 37)
    x = torch.from_numpy(zoo.pool(hw)[:n]).cuda()
    for name in pairs:
        on, off, family, tol = AB[name]
        label = '%s %s n=%d %s' % (arch, hw, n, name)
        a, b = _pair(m, x, on, off, family, label)
        for side, t in (('on', a), ('off', b)):
            against_oracle(zoo, '%s %s' % (label, side), arch, 'v3', 512, hw, [u[[0, n - 1]] for u in t], [0, n - 1])
        rel = max(float(np.abs(u - v).max()) / max(float(np.abs(v).max()), 1.0) for u, v in zip(a, b))
        print('%s: max |on - off| / max(max |off|, 1) = %.2e' % (label, rel))
        if name in MAP_GATED:
            assert rel <= tol, (label, rel)
    with options(m, sk2=0, mt=0, bdp=0):
        lean = as_list(m.embed(x))
        assert ran(m, 'conv_igemm_kernel<64x64,patch') and not ran(m, 'conv_bdp_kernel')
        with options(m, dbg=1024):
            general = as_list(m.embed(x))
    assert all(np.array_equal(u, v) for u, v in zip(lean, general))


GDC_VGG = ('pipe', 'bdp', 't2', 'tn', 'patch2d', 'patch', 'bd', 'stem')
GDC_RES = ('bdp', 'tn', 'patch', 'bd', 'stem')      # (24 x 20 .. 6 x 5: no 8-aligned map)


@pytest.mark.parametrize('arch,hw,n,pairs', [('vgg16', (96, 112), 37, GDC_VGG), ('vgg16', (112, 96), 5, GDC_VGG[1:]),
                                             ('resnet', (96, 80), 37, GDC_RES), ('resnet', (80, 96), 9, GDC_RES)])
def test_large_batch_families_agree(zoo, arch, hw, n, pairs):
    """The same pairs against each other at the square tests' gates verbatim: an absolute difference between unit-norm
    512-d GDC embeddings.  The library builds that head on a square last map only, so the inputs are 96 x 112 / 112 x 96
    (VGG16: 96 x 112 and 48 x 56 8-aligned, 24 x 28, 12 x 14, 6 x 7 -- every convolution on an H != W map) and 96 x 80 / 80 x 96
    (ResNet50V2: 48 x 40 stem output, 24 x 20, 12 x 10, 6 x 5; its conv5 stack runs on the square 3 x 3 map and does not count
    towards a family having run).  First and last image against the oracle."""
    m = zoo.net(arch, 'v2', 512, hw, 37)
    x = torch.from_numpy(zoo.pool(hw)[:n]).cuda()
    square = ('conv5_',) if arch == 'resnet' else ()
    for name in pairs:
        on, off, family, tol = AB[name]
        label = '%s %s n=%d %s' % (arch, hw, n, name)
        (a,), (b,) = _pair(m, x, on, off, family, label, square)
        worst = float(np.abs(a - b).max())
        print('%s: max |on - off| = %.2e (gate %.0e)' % (label, worst, tol))
        assert worst <= tol, (label, worst)
        against_oracle(zoo, label + ' on', arch, 'v2', 512, hw, [a[[0, n - 1]]], [0, n - 1])


# ------------------------------------------------------------------------------------------- 3. Winograd
MIN_TILES, WIDE_MIN_IMAGES = 64 * 49, 128          # conv_winograd.hpp: wino::MIN_TILES, wino::WIDE_MIN_IMAGES


def wino_batch(narrow_map):
    """The smallest odd batch at which wino_applies admits both the wide maps (128 images) and this narrow (<= 16 x 16) one."""
    n = max(WIDE_MIN_IMAGES, -(-MIN_TILES // ((narrow_map[0] // 2) * (narrow_map[1] // 2))))
    return n + 1 - n % 2


WINO_CASES = [
    # arch, input, the narrow map, conv_winow_kernel layers (maps with a side above 16), conv_wino_kernel layers
    ('vgg16', (32, 64), (8, 16), ['block1_conv2', 'block2_conv1', 'block2_conv2'], ['block3_conv1', 'block3_conv2', 'block3_conv3']),
    ('vgg16', (64, 32), (16, 8), ['block1_conv2', 'block2_conv1', 'block2_conv2'], ['block3_conv1', 'block3_conv2', 'block3_conv3']),
    ('resnet', (64, 96), (8, 12), ['conv2_block1_2_conv', 'conv2_block2_2_conv'], ['conv3_block%d_2_conv' % b for b in (1, 2, 3)]),
]


@pytest.mark.parametrize('arch,hw,narrow,wide_layers,narrow_layers', WINO_CASES)
def test_winograd_levels(zoo, monkeypatch, arch, hw, narrow, wide_layers, narrow_layers):
    """F(2x2,3x3) on even H != W maps, one lane: conv_winow_kernel on 32 x 64 and 16 x 32 (16 x 24), conv_wino_kernel on
    8 x 16 (8 x 12), whose tw = W / 2, tpi = (H / 2) * tw tiling is where the two sides part.  Levels 2, 1, 0 as
    test_winograd_wide_gpu.run_levels: cosine gap to level 0 below 1e-6, level 2 bit-identical run to run, spot rows
    against the oracle (cosine gap below 1e-5, and the map gate)."""
    n = wino_batch(narrow)
    m = zoo.net(arch, 'v3', 512, hw, n, streams=1, monkeypatch=monkeypatch)
    u8 = zoo.pool(hw, n)
    dev = torch.from_numpy(u8).cuda()
    out, tab = {}, {}
    try:
        for lvl in (2, 1, 0):
            m.set_option('wino', lvl)
            a = m.embed(dev)
            if lvl == 2:
                assert torch.equal(a, m.embed(dev))
            out[lvl] = a.cpu().numpy()
            tab[lvl] = (ran(m, 'conv_wino_kernel'), ran(m, 'conv_winow_kernel'))
    finally:
        m.set_option('wino', 2)
    assert tab[2] == (narrow_layers, wide_layers), tab[2]
    assert tab[1] == (narrow_layers, []) and tab[0] == ([], [])
    gap = gates.cosine_gap(out[2], out[0]).max()
    print('%s %s n=%d: cosine gap level 2 / level 0 %.2e, level 1 / level 0 %.2e, max |level 2 - level 0| / max %.2e'
          % (arch, hw, n, gap, gates.cosine_gap(out[1], out[0]).max(), gates.worst(out[2], out[0])))
    assert gap < 1e-6 and gates.cosine_gap(out[1], out[0]).max() < 1e-6
    rows = [0, n // 2, n - 1]
    want = zoo.want(arch, 'v3', 512, hw, rows, n)[0]
    assert gates.cosine_gap(out[2][rows], want).max() < 1e-5
    against_oracle(zoo, '%s %s n=%d wino 2' % (arch, hw, n), arch, 'v3', 512, hw, [out[2][rows]], rows, n)


# ------------------------------------------------------------------------------------------- 4. split-bf16
@pytest.mark.parametrize('compute', ['bf16x3', 'bf16x2'])
@pytest.mark.parametrize('arch,hw,n,forms', [('vgg16', (48, 80), 16, ('patch128+Bdirect', 'patch8x8+Bdirect')),
                                             ('resnet', (96, 64), 37, ('patch128+Bdirect',))])
def test_split_bf16_vs_f32_and_oracle(zoo, arch, hw, n, forms, compute):
    """bf3p_applies' two forms on H != W maps, at test_embed_bf16x3_mode_vs_oracle's gates: VGG16 48 x 80 takes the two 8x8
    sub-tiles on 48 x 80 / 24 x 40 and the linear patch from 12 x 20 down; every 3x3 / stride 1 map of ResNet50V2 96 x 64
    (24 x 16 .. 3 x 2) fits the linear patch, which conv_bf3p_form asks first, so that net has no sub-tile layer."""
    f32 = zoo.net(arch, 'v3', 512, hw, 37)
    b3 = zoo.net(arch, 'v3', 512, hw, 37, compute=compute)
    u8 = zoo.pool(hw)[:n]
    got, ref = b3.predict_on_batch(u8), f32.predict_on_batch(u8)
    for form in forms:
        assert ran(b3, 'conv_igemm_kernel[split-bf16]') and any(form in k for _, k, _ in b3.op_table() if 'split-bf16' in k), families(b3)
    assert np.all(np.isfinite(got))
    gap = gates.cosine_gap(got, ref).max()
    print('%s %s n=%d %s: cosine gap to f32 %.2e' % (arch, hw, n, compute, gap))
    assert gap < 1e-6
    rows = [0, 1, n // 2, n - 1]
    want = zoo.want(arch, 'v3', 512, hw, rows)[0]
    assert gates.cosine_gap(got[rows], want).max() < 1e-5
    against_oracle(zoo, '%s %s n=%d %s' % (arch, hw, n, compute), arch, 'v3', 512, hw, [got[rows]], rows)
    assert np.array_equal(b3.predict_on_batch(u8), got)           # deterministic
    assert not np.array_equal(got, ref)                            # ... and really another arithmetic


# ------------------------------------------------------------------------------------------- 5. heads
@pytest.mark.parametrize('arch,head,emd,hw,n,op,kernel', [
    ('resnet', 'v2', 512, (96, 80), 1, 'head_tail', 'gdc_tail_a_kernel+gdc_tail_b_kernel'),
    ('resnet', 'v2', 512, (96, 80), 2, 'head_tail', 'gdc_tail_a_kernel+gdc_tail_b_kernel'),
    ('resnet', 'v2', 512, (96, 80), 9, 'head_tail', 'gdc_tail_kernel<KSPLIT=2>'),
    ('resnet', 'v2', 100, (96, 80), 3, 'head_dw', 'dwfull_kernel'),               # emd % 8 != 0: the unfused tail
    ('vgg16', 'v2', 512, (96, 112), 3, 'head_tail', 'gdc_tail_kernel<KSPLIT=2>'),
    ('mobilenet', 'v2', 512, (96, 80), 2, 'head_tail', 'gdc_tail_a_kernel+gdc_tail_b_kernel'),
    ('vgg16', 'sv2', 128, (96, 160), 1, 'norm_embedding', 'conv_'),               # 3 x 5 -> ceil pools 2 x 3, 1 x 2 -> a 1 x 2 dense kernel
    ('vgg16', 'sv2', 128, (96, 160), 3, 'norm_embedding', 'conv_'),
    ('resnet', 'sv2', 128, (72, 104), 3, 'norm_embedding', 'conv_'),              # 3 x 4 -> 2 x 2 -> 1 x 1: the tap outside the map on one axis only
    ('resnet', 'v1', 128, (128, 256), 1, 'embeddings', 'conv_'),                  # 4 x 8 -> floor pools 2 x 4, 1 x 2 -> a 1 x 2 dense kernel
    ('resnet', 'v1', 128, (128, 256), 3, 'embeddings', 'conv_'),
])
def test_heads_vs_oracle(zoo, arch, head, emd, hw, n, op, kernel):
    """The embedding heads on H != W inputs: the GDC tail (a 3 x 3 last map under a non-square input: every backbone map but
    the last is non-square), the siamese head's 'same' pools and the v1 head's floor pools down to a dense kernel with
    KH != KW.  Embeddings: cosine gap and every element."""
    m = zoo.net(arch, head, emd, hw, 12)
    got = m.predict_on_batch(zoo.pool(hw)[:n])
    table = {name: kern for name, kern, _ in m.op_table()}
    assert table[op] == kernel if op == 'head_tail' else table[op].startswith(kernel), (op, table[op])
    against_oracle(zoo, '%s %s emd %d %s n=%d' % (arch, head, emd, hw, n), arch, head, emd, hw, [got], list(range(n)),
                   f64_rows=(0,) if n == 1 else ())


# ------------------------------------------------------------------------------------------- 6. input forms
def test_input_forms_agree(zoo):
    """test_embed_gpu.test_input_forms_agree / test_flipped_concat / test_bgr_mean_transform on a 64 x 96 input, on the whole
    2 x 3 x 2048 map: NCHW float and uint8 (the plane stride is H * W, the row stride W), the fused 1 / 255, the fused
    mirror (w -> W - 1 - w) and BGR + mean, with batches above max_batch."""
    from deep_insight_face.networks.triplet import DifEmbedder
    hw = (64, 96)
    m = DifEmbedder('resnet', 'v3', 512, hw + (3,), max_batch=4).init_synthetic(2024)
    try:
        u8 = gates.frames_u8(6, hw, seed=61)
        x = gates.scaled(u8)
        base = m.predict_on_batch(x)
        assert base.shape == (6, 2, 3, 2048)
        gates.check_map(base, nets.embed(x, m.get_weights(), 'resnet', 512, 'v3'))
        assert np.array_equal(base, m.predict_on_batch(np.ascontiguousarray(x.transpose(0, 3, 1, 2))))
        t = m.predict_on_batch(torch.from_numpy(x).cuda())
        assert torch.is_tensor(t) and np.array_equal(t.cpu().numpy(), base)
        m.set_input_transform(scale=1 / 255.)
        fused = m.predict_on_batch(u8)
        u8_nchw = np.ascontiguousarray(u8.transpose(0, 3, 1, 2))
        assert gates.cosine_gap(fused, base).max() < 1e-6
        assert np.array_equal(fused, m.predict_on_batch(u8_nchw))
        mirrored = m.predict_on_batch(u8[:, :, ::-1, :].copy())
        assert not np.array_equal(mirrored, fused)
        m.set_input_transform(scale=1 / 255., hflip=True)
        assert np.array_equal(m.predict_on_batch(u8), mirrored)
        assert np.array_equal(m.predict_on_batch(u8_nchw), mirrored)
        m.set_input_transform(hflip=True)
        flipped_f32 = m.predict_on_batch(x)
        assert np.array_equal(flipped_f32, m.predict_on_batch(np.ascontiguousarray(x.transpose(0, 3, 1, 2))))
        m.set_input_transform()
        assert np.array_equal(m.predict_on_batch(x[:, :, ::-1, :].copy()), flipped_f32)
        one = m.predict_on_batch(x[2:3])
        assert gates.cosine_gap(one, base[2:3]).max() < 1e-6
        assert np.array_equal(m.predict_on_batch(x), base)
        mean = np.array([103.939, 116.779, 123.68], dtype=np.float32)
        m.set_input_transform(scale=1.0, bias=tuple(-mean), bgr=True)
        got = m.predict_on_batch(x[:2])
        want = nets.embed(x[:2, ..., ::-1] - mean, m.get_weights(), 'resnet', 512, 'v3')
        assert gates.cosine_gap(got, want).max() < 1e-5
        gates.check_map(got, want)
        with pytest.raises(ValueError):
            m.predict_on_batch(np.zeros((2, 96, 64, 3), dtype=np.float32))          # the transposed shape is another network
    finally:
        m.close()
    # ... and a row does not depend on its batch beyond float32 rounding: the square test's atol = 2e-6, on the quantity it is
    # stated on (the GDC embedding; 96 x 80 input)
    g = zoo.net('resnet', 'v2', 512, (96, 80), 12)
    u = zoo.pool((96, 80))[:6]
    six, one = g.predict_on_batch(u), g.predict_on_batch(u[2:3])
    assert gates.cosine_gap(one, six[2:3]).max() < 1e-6
    np.testing.assert_allclose(one[0], six[2], atol=2e-6)


# ------------------------------------------------------------------------------------------- 7. two lanes
@pytest.mark.parametrize('arch,emd,hw', [('resnet', 512, (64, 96)), ('yolov3', 1, (64, 160))])
def test_two_lanes_equal_one_lane(zoo, monkeypatch, arch, emd, hw):
    """65 images: one above the 64 from which a forward of these sizes is split (Net::lane_min_images), lanes of 33 and 32,
    each writing its images' part of every output map; against the same batch on one lane at the gates of
    test_two_lane_forward_matches_single_lane / test_yolov3_two_lanes_equal_one_lane, both lanes' end rows against the oracle."""
    n = 65
    two = zoo.net(arch, 'v3', emd, hw, n, streams=2, monkeypatch=monkeypatch)
    one = zoo.net(arch, 'v3', emd, hw, n, streams=1, monkeypatch=monkeypatch)
    u8 = zoo.pool(hw, n)
    a, b = as_list(two.embed(torch.from_numpy(u8).cuda())), as_list(one.embed(torch.from_numpy(u8).cuda()))
    assert [t.shape[1:3] for t in a] == out_hw(arch, hw)
    for u, v in zip(a, b):
        print('%s %s two lanes vs one: cosine gap %.2e, max diff / max %.2e' % (arch, hw, gates.cosine_gap(u, v).max(), gates.worst(u, v)))
        assert gates.cosine_gap(u, v).max() < 1e-6
        np.testing.assert_allclose(u, v, rtol=1e-4, atol=1e-5 * np.abs(v).max())
    assert all(np.array_equal(u, v) for u, v in zip(as_list(two.embed(torch.from_numpy(u8).cuda())), a))
    assert not all(np.array_equal(u, v) for u, v in zip(a, b))     # the halves ran as batches of 33 and 32: other split sums
    rows = [0, 32, 33, 64]
    against_oracle(zoo, '%s %s n=65 two lanes' % (arch, hw), arch, 'v3', emd, hw, [t[rows] for t in a], rows, n)


# ------------------------------------------------------------------------------------------- 8. dif_yolo_decode
def _decode_maps(grids, num_classes, seed):
    rng = np.random.default_rng(seed)
    outs = []
    for gh, gw in grids:
        f = rng.standard_normal((1, gh, gw, 3 * (5 + num_classes))).astype(np.float32)
        f[..., 4::(5 + num_classes)] -= 3.0
        for _ in range(3):                                       # a few confident cells, off the diagonal
            y, x, a = int(rng.integers(0, gh)), int(rng.integers(0, gw)), int(rng.integers(0, 3))
            f[0, y, x, a * (5 + num_classes) + 4:(a + 1) * (5 + num_classes)] = rng.uniform(2.0, 5.0, 1 + num_classes)
        outs.append(f)
    return outs


@pytest.mark.parametrize('input_shape', [(64, 160), (160, 64)])
@pytest.mark.parametrize('num_classes,image_shape', [(1, (480, 640)), (2, (300, 900))])
def test_decode_nonsquare_vs_oracle(cuda, input_shape, num_classes, image_shape):
    """dif_yolo_decode with input_h != input_w (grids 2 x 5, 4 x 10, 8 x 20 and their mirrors): cell (y, x) of a gh x gw grid,
    box_xy / (gw, gh), box_wh / (input_w, input_h) and the letterbox correction per axis, at test_decode_and_nms_vs_oracle's
    tolerances; then the score filter and suppression on those boxes."""
    from deep_insight_face.detector import yolov3
    grids = [(input_shape[0] // s, input_shape[1] // s) for s in (32, 16, 8)]
    outs = _decode_maps(grids, num_classes, seed=num_classes + input_shape[0])
    boxes, scores = yolov3.boxes_and_scores_all(outs, odet.ANCHORS, num_classes, image_shape)
    want_b, want_s = [], []
    for l, mask in enumerate(([6, 7, 8], [3, 4, 5], [0, 1, 2])):
        b, s = odet.boxes_and_scores(outs[l], odet.ANCHORS[mask], num_classes, input_shape, image_shape)
        want_b.append(b)
        want_s.append(s)
    want_b, want_s = np.concatenate(want_b), np.concatenate(want_s)
    assert boxes.shape == (1, 3 * sum(gh * gw for gh, gw in grids), 4)
    np.testing.assert_allclose(boxes[0], want_b, rtol=2e-5, atol=2e-3)
    np.testing.assert_allclose(scores[0], want_s, rtol=2e-5, atol=1e-6)
    # (the oracle's get_yolo_output takes the input shape from the coarse grid x 32, per axis, as the library does)
    gb, gs, gc = yolov3.get_yolo_output(outs, odet.ANCHORS, num_classes, image_shape, 20, 0.3, 0.5)
    ob, os_, oc = odet.get_yolo_output(outs, odet.ANCHORS, num_classes, image_shape, 20, 0.3, 0.5)
    assert len(gs) == len(os_) and len(gs) > 0
    assert np.array_equal(gc, oc)
    np.testing.assert_allclose(gs, os_, rtol=2e-5)
    np.testing.assert_allclose(gb, ob, rtol=2e-5, atol=2e-3)
