"""Layer taps: every launch of a net against a float64 reference of THAT layer, fed the input the kernel read.

The whole-net tests see a convolution kernel through thirty layers and an L2 normalisation; a defect in one tile, one
border column, one K-step or one shortcut element of one layer passes their gates.  Here every case taps every launch
(`DifEmbedder.tap`), computes the layer on the device in float64 (tests/layer_ref.py: a sum over taps, no library
convolution) and holds every element of every image to the a-priori rounding bound, and the layer's worst relative error to
8 x that of a float32 run of the same reference (tests/layer_sweep.py states the gates; tests/test_layer_ref.py shows on
the CPU that they pass float32 arithmetic and reject five planted one-place defects).

The split-bf16 tiers are held, besides, to the float64 sum of the products they keep (the split reference: hard, max and rms
gates of tests/layer_sweep.py), the tier read from the model as it stands; SPLIT_CASES sweep only the launches that ran a
split-bf16 kernel, on IResNet-50, YOLOv3, a sub-sampled first output, the two-term tile under three terms, a model switched
3 -> 2 -> 3, and two liveness runs hand a tier the OTHER tier's reference.

Cases: the smallest shapes the existing tests use to reach each kernel form (tests/test_nonsquare_gpu.py,
tests/test_winograd_kstep_gpu.py), every net on ONE lane (the tap is single-lane by construction), odd batches so the
last blocks are partial.  Each case asserts by kernel label that its forms ran; the last test holds the union of labels
to the list observed on the MI355X.  tools/layer_taps.py runs the same cases and records the ratios
(profiles/layer_taps.json).
"""
import os

import pytest
import torch

import layer_sweep
from test_nonsquare_gpu import AB, RES_AB, VGG_AB, OWN_KERNELS, Zoo, options, small_batch_family, wino_batch

pytestmark = pytest.mark.gpu

TWIN_BITS = 16777216 | 65536        # conv_winograd.hpp: the eight-wave twins of the half-block shapes
SEEN, RECORD = set(), {}


class Env:
    """monkeypatch's setenv / delenv for a caller outside pytest (tools/layer_taps.py)."""

    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k):
        os.environ.pop(k, None)


def case(group, arch, head, emd, hw, n, opts=None, expect=(), absent=(), compute='f32', max_batch=None, name='', **more):
    """more: 'kinds' / 'names' (only these launches are swept), 'exact' ({launch name: the label it must have run}),
    'every' (every launch of the net must have been checked), 'pools' ({mode: count} of the pool launches checked)."""
    return dict({'id': '%s-%s-%dx%d-n%d%s' % (group, arch, hw[0], hw[1], n, ('-' + name) if name else ''), 'net': (arch, head, emd, hw),
                 'n': n, 'opts': dict(opts or {}), 'expect': tuple(expect), 'absent': tuple(absent), 'compute': compute,
                 'max_batch': max_batch or n}, **more)


TAIL_KINDS = ('gdctail', 'dwfull', 'l2norm', 'conv')
TAIL_NAMES = ('head_', 'norm_', 'embeddings')
K8, K2, AB_TAIL = 'gdc_tail_kernel<KSPLIT=8>', 'gdc_tail_kernel<KSPLIT=2>', 'gdc_tail_a_kernel+gdc_tail_b_kernel'
# the backbones that leave a last map of HW pixels
MAP_OF = {1: ('mobilenet', (32, 32)), '1v': ('vgg16', (32, 32)), 4: ('resnet', (64, 64)), 9: ('resnet', (96, 96)),
          49: ('mobilenet', (224, 224))}


def tail_form(emd, n):
    """What gdc_tail_run must dispatch (elementwise.hip), or None for the unfused tail (net.hip: build_heads)."""
    if emd % 8 or emd > 1024:
        return None
    if n >= 3:
        return K2
    return AB_TAIL if emd % 32 == 0 else K8


def tail_case(hw_key, emd, n, max_batch):
    arch, hw = MAP_OF[hw_key]
    form = tail_form(emd, n)
    exact = {'head_tail': form} if form else {'head_dw': 'dwfull_kernel', 'norm_embedding': 'l2norm_kernel'}
    return case('tail', arch, 'v2', emd, hw, n, expect=() if form else ('conv_',), max_batch=max_batch, name='emd%d-mb%d' % (emd, max_batch),
                kinds=TAIL_KINDS, names=TAIL_NAMES, exact=exact)


def build_cases():
    cases = []
    # 1. default dispatch at the reference's call shapes
    for arch, head, emd, hw in [('vgg16', 'v3', 512, (48, 80)), ('resnet', 'v3', 512, (64, 96)), ('resnet', 'v3', 512, (72, 104)),
                                ('mobilenet', 'v3', 512, (75, 41)), ('yolov3', 'v3', 1, (64, 160)), ('mtcnn_pnet', 'v3', 1, (37, 53))]:
        for n in (1, 3, 12):
            exp = ('conv_', 'maxpool_kernel') if arch == 'mtcnn_pnet' else tuple(small_batch_family(arch, n)) + OWN_KERNELS[arch]
            cases.append(case('default', arch, head, emd, hw, n, expect=exp + ('input_convert_kernel',), max_batch=12))
    # 2. the large-batch families, each option set of test_nonsquare_gpu.AB, and both epilogues
    for arch, hw, n, pairs, known in [('vgg16', (48, 80), 37, VGG_AB, True), ('vgg16', (48, 80), 5, VGG_AB[1:], True),
                                      ('resnet', (64, 96), 37, RES_AB, True), ('resnet', (64, 96), 9, RES_AB, False)]:
        for pair in pairs:
            on, off, fam, _ = AB[pair]
            cases.append(case('large', arch, 'v3', 512, hw, n, dict(sk2=0, mt=0, **on), (fam,) if known else (), name=pair + '-on', max_batch=37))
            cases.append(case('large', arch, 'v3', 512, hw, n, dict(sk2=0, mt=0, **off), (), (fam,) if known else (), name=pair + '-off', max_batch=37))
        cases.append(case('large', arch, 'v3', 512, hw, n, dict(sk2=0, mt=0, bdp=0), ('conv_igemm_kernel<64x64,patch',) if known else (),
                          ('conv_bdp_kernel',), name='lean-epilogue', max_batch=37))
        cases.append(case('large', arch, 'v3', 512, hw, n, dict(sk2=0, mt=0, bdp=0, dbg=1024), name='general-epilogue', max_batch=37))
    # 3. Winograd: levels 2, 1, 0 and the eight-wave twins
    for arch, head, emd, hw, n in [('iresnet50', 'v2', 512, (112, 112), 129), ('vgg16', 'v3', 512, (32, 64), wino_batch((8, 16))),
                                   ('vgg16', 'v3', 512, (64, 32), wino_batch((16, 8))), ('resnet', 'v3', 512, (64, 96), wino_batch((8, 12))),
                                   ('yolov3', 'v3', 1, (32, 64), 129)]:
        narrow = ('conv_wino_kernel',)
        rest = ('conv_winox_kernel<F(2x2,3x3),32 tiles x 64,odd>', 'conv_winox_kernel<F(2x2,3x3),32 tiles x 64,ysub>') if arch == 'iresnet50' else ()
        cases.append(case('wino', arch, head, emd, hw, n, dict(wino=2), narrow + ('conv_winow_kernel',) + rest, name='level2'))
        cases.append(case('wino', arch, head, emd, hw, n, dict(wino=1), narrow, ('conv_winow_kernel', 'conv_winox_kernel'), name='level1'))
        cases.append(case('wino', arch, head, emd, hw, n, dict(wino=0), (), layer_sweep.WINO, name='level0'))
        cases.append(case('wino', arch, head, emd, hw, n, dict(wino=2, dbg=TWIN_BITS), tuple('%s<F(2x2,3x3),64 tiles x 64>' % k for k in narrow + ('conv_winow_kernel',)) + rest,
                          name='twins'))
    # 4. split-bf16, both tiers, both patch forms
    for compute in ('bf16x3', 'bf16x2'):
        cases.append(case('bf16', 'vgg16', 'v3', 512, (48, 80), 16, None, ('split-bf16', 'patch128+Bdirect', 'patch8x8+Bdirect'), compute=compute,
                          max_batch=37, name=compute))
        cases.append(case('bf16', 'resnet', 'v3', 512, (96, 64), 37, None, ('split-bf16', 'patch128+Bdirect'), compute=compute, max_batch=37, name=compute))
    # 5. NN4.small2, every launch: lrn_kernel, the L2 / average pools, the concat views and their zero fills
    for n in (1, 3, 7):
        cases.append(case('nn4', 'nn4', 'v2', 128, (96, 96), n, expect=('lrn_kernel', 'l2norm_kernel', 'maxpool_kernel', 'memset', 'conv_'), max_batch=7,
                          every=True, pools={'l2': 3, 'avg': 1, 'max': 6}))
    # 6. the GDC tail in every form.  Every emd at HW 9; every HW at emd 512 and 136; each form at each of its batch sizes; max_batch
    # above n (8) in half of the one- and two-image cases.
    for emd, rows in [(8, [(1, 1), (2, 8), (3, 8)]), (40, [(1, 8), (2, 2), (5, 8)]), (136, [(1, 1), (2, 8), (8, 8)]),
                      (1000, [(1, 8), (2, 2), (3, 8), (5, 8)]), (32, [(1, 1), (2, 8), (3, 8)]), (512, [(1, 8), (2, 2), (5, 8), (8, 8)]),
                      (1024, [(1, 1), (2, 8), (3, 8)]), (100, [(1, 1), (3, 8)]), (1032, [(1, 8), (3, 3)])]:
        cases += [tail_case(9, emd, n, mb) for n, mb in rows]
    for key, emd, rows in [(1, 512, [(1, 8), (3, 8)]), ('1v', 136, [(2, 8), (5, 8)]), (4, 512, [(2, 2), (8, 8)]), (4, 136, [(1, 8), (3, 8)]),
                           (49, 512, [(1, 1), (3, 3)]), (49, 136, [(2, 8), (5, 8)])]:
        cases += [tail_case(key, emd, n, mb) for n, mb in rows]
    # IResNet-50 at 112 x 112 (a 7 x 7 last map): its own head is one dense layer over the map, not the GDC tail (net.hip), so of
    # the tail kinds it runs l2norm_kernel at D = 512; the fused tail at HW 49 is MobileNetV2's at 224 x 224 above
    cases.append(case('tail', 'iresnet50', 'v2', 512, (112, 112), 3, max_batch=129, kinds=TAIL_KINDS, names=TAIL_NAMES,
                      exact={'norm_embedding': 'l2norm_kernel'}))
    # 7. the v1 and sv2 heads, every launch: 2 x 2 pools, the whole-map valid convolution, the dense layer behind a BN
    cases.append(case('heads', 'resnet', 'v1', 128, (112, 112), 5, expect=('maxpool_kernel', 'conv_'), every=True))
    cases.append(case('heads', 'vgg16', 'sv2', 128, (96, 96), 2, expect=('maxpool_kernel', 'conv_'), every=True))
    return cases


CASES = build_cases()


def run_case(zoo, c, env, verbose=False):
    """-> (failures, kernel labels seen, launches checked); the net is built on one lane and its options restored."""
    arch, head, emd, hw = c['net']
    m = zoo.net(arch, head, emd, hw, c['max_batch'], compute=c['compute'], streams=1, monkeypatch=env)
    x = torch.from_numpy(zoo.pool(hw, max(c['n'], 40))[:c['n']]).cuda()
    with options(m, **c['opts']):
        fails, seen, checked = layer_sweep.sweep(m, x, c['id'], RECORD, verbose, kinds=c.get('kinds'), names=c.get('names'))
    descs, table = m.op_describe(), {name: kern for name, kern, _ in m.op_table()}
    for name, kern in c.get('exact', {}).items():
        if table.get(name) != kern:
            fails.append('%s: %s ran %r, this shape and batch dictate %r' % (c['id'], name, table.get(name), kern))
    if 'kinds' in c:
        want = sum(d['kind'] in c['kinds'] and d['name'].startswith(c['names']) for d in descs)
        if checked != want or checked < len(c['exact']):
            fails.append('%s: %d launches checked, %d match kinds / names' % (c['id'], checked, want))
        return fails, seen, checked
    if c.get('every') and checked != len(descs):
        fails.append('%s: %d launches checked of %d' % (c['id'], checked, len(descs)))
    for mode, count in c.get('pools', {}).items():
        got = sum(d['kind'] == 'maxpool' and d['pool'] == mode for d in descs)
        if got != count:
            fails.append('%s: %d pools of mode %s in the launch list, %d expected' % (c['id'], got, mode, count))
    for k in c['expect']:
        if not any(k in s for s in seen):
            fails.append('%s: no launch ran %s (ran: %s)' % (c['id'], k, sorted(seen)))
    for k in c['absent']:
        if any(k in s for s in seen):
            fails.append('%s: a launch ran %s, which this option set switches off' % (c['id'], k))
    n_conv = sum(d['kind'] == 'conv' for d in m.op_describe())
    if checked < n_conv + 1:
        fails.append('%s: %d launches checked, the net has %d convolutions' % (c['id'], checked, n_conv))
    return fails, seen, checked


@pytest.fixture(scope='module')
def zoo(cuda):
    z = Zoo()
    yield z
    z.close()


@pytest.mark.parametrize('c', CASES, ids=[c['id'] for c in CASES])
def test_every_launch_against_its_float64_layer(zoo, monkeypatch, c):
    fails, seen, checked = run_case(zoo, c, monkeypatch)
    SEEN.update(seen)
    print('%s: %d launches checked, %d kernel labels' % (c['id'], checked, len(seen)))
    assert not fails, '%d failures\n' % len(fails) + '\n'.join(fails)


def test_nn4_lrn_inputs_are_large_enough_to_see_a_short_window(zoo, monkeypatch):
    """A window one channel short moves an LRN output by 0.75e-4 v^2 relative (v: the missing value): against the bound's
    28 u = 1.7e-6 that shows for |v| above 0.15.  The synthetic weights give the maps tapped at lrn_1 and lrn_2 a median
    nonzero |x| of 0.64 and 0.92 (the float32 oracle on these inputs): no rescaling of bn1 / bn3 is needed, and this holds it."""
    m = zoo.net('nn4', 'v2', 128, (96, 96), 7, streams=1, monkeypatch=monkeypatch)
    x = torch.from_numpy(zoo.pool((96, 96), 40)[:7]).cuda()
    names = [d['name'] for d in m.op_describe()]
    for layer in ('lrn_1', 'lrn_2'):
        t = m.tap(x, names.index(layer))['x']
        med = float(t[t != 0].abs().median())
        print('%s: median nonzero |x| %.3f, %.0f %% nonzero, max %.2f' % (layer, med, 100 * float((t != 0).float().mean()), float(t.abs().max())))
        assert med >= 0.5


def _fresh(arch, emd, hw, max_batch, env, zero_dense=False):
    from deep_insight_face.networks.triplet import DifEmbedder
    env.setenv('DIF_STREAMS', '1')
    m = DifEmbedder(arch, 'v2', emd, hw + (3,), max_batch=max_batch).init_synthetic(2024)
    if zero_dense:
        p = m.get_weights()
        p['head_dense/kernel'] = 0 * p['head_dense/kernel']
        m.set_weights(p)
    m.set_input_transform(scale=1 / 255.)
    m._finalize()
    env.delenv('DIF_STREAMS')
    return m


@pytest.mark.parametrize('emd,n,label', [(40, 2, K8), (512, 2, AB_TAIL), (512, 3, K2), (100, 3, 'l2norm_kernel')])
def test_zero_dense_kernel_gives_exact_zero_rows(zoo, monkeypatch, emd, n, label):
    """head_dense/kernel all zero: every o is 0, sum o^2 = 0, and max(sum, eps) makes the row 0 * 1e6 = 0.0 exactly -- in each
    of the three fused forms and in l2norm_kernel -- with nothing non-finite.  Ordinary arithmetic: no fault is provoked."""
    m = _fresh('vgg16', emd, (32, 32), 3, monkeypatch, zero_dense=True)
    try:
        y = m.embed(torch.from_numpy(zoo.pool((32, 32), 40)[:n]).cuda())
        table = {name: kern for name, kern, _ in m.op_table()}
        assert table['head_tail' if emd % 8 == 0 else 'norm_embedding'] == label, table
        assert y.shape == (n, emd) and bool(torch.isfinite(y).all()) and bool((y == 0).all())
    finally:
        m.close()


def test_two_image_tail_twice_is_bit_identical(zoo, monkeypatch):
    """gdc_tail_a_kernel + gdc_tail_b_kernel draw a ticket per block; the last taker clears it.  Two consecutive calls at two
    images give the same bits (a ticket left above zero would let an earlier block normalise half-written rows), and rows of
    unit norm."""
    m = zoo.net('resnet', 'v2', 512, (96, 96), 2, streams=1, monkeypatch=monkeypatch)
    x = torch.from_numpy(zoo.pool((96, 96), 40)[:2]).cuda()
    a = m.embed(x).clone()
    b = m.embed(x).clone()
    assert dict((name, kern) for name, kern, _ in m.op_table())['head_tail'] == AB_TAIL
    assert torch.equal(a, b) and bool(((a.double() ** 2).sum(1) - 1).abs().max() < 1e-6)


def test_sweep_is_live_on_the_device(zoo, monkeypatch):
    """The comparison on the device has teeth: a reference handed ONE bias value off by 2^-10 -- the layer's outputs are of
    order 1, and the kernels run on the true weights -- fails that layer, at that channel, and no other layer; the same sweep
    with the true parameters passes (the cases above).  What a one-place defect in the KERNEL does to the gates: tests/test_layer_ref.py."""
    m = zoo.net('vgg16', 'v3', 512, (48, 80), 12, streams=1, monkeypatch=monkeypatch)
    x = torch.from_numpy(zoo.pool((48, 80), 40)[:3]).cuda()
    p = {k: v.copy() for k, v in m.get_weights().items()}
    p['block3_conv2/bias'][17] += 2.0 ** -10
    fails, _, _ = layer_sweep.sweep(m, x, 'live', None, params=p)
    print('\n'.join(fails))
    assert fails and all(f.startswith('block3_conv2 ') and 'channel 17' in f for f in fails), fails


def test_tail_sweep_is_live_on_the_device(zoo, monkeypatch):
    """The tail's gates have teeth on the device too: a reference handed the 1x1 kernel with ONE weight zeroed -- the largest
    product of output 7 of image 0, what a kernel that dropped that product would have computed -- fails head_tail and
    nothing else; the hard bound alone would pass it (tests/test_layer_ref.py), the tight gate is what fails."""
    m = zoo.net('resnet', 'v2', 40, (96, 96), 8, streams=1, monkeypatch=monkeypatch)
    x = torch.from_numpy(zoo.pool((96, 96), 40)[:3]).cuda()
    descs = m.op_describe()
    i = [d['name'] for d in descs].index('head_tail')
    p = {k: v.copy() for k, v in m.get_weights().items()}
    a, _ = layer_sweep.L._depthwise_full(descs[i], p, m.tap(x, i)['x'], torch.float64)
    k = int((a[0].cpu() * torch.from_numpy(p['head_pw/kernel'][0, 0, :, 7]).double()).abs().argmax())
    p['head_pw/kernel'][0, 0, k, 7] = 0
    fails, _, checked = layer_sweep.sweep(m, x, 'live', None, params=p, kinds=TAIL_KINDS, names=TAIL_NAMES)
    print('\n'.join(fails))
    assert checked == 2 and fails and all(f.startswith('head_tail ') for f in fails) and any('tight gate' in f for f in fails), fails


# ------------------------------------------------------------------------------------------------- split-bf16, term by term
SPLIT = 'split-bf16'
WIDE_LIN, WIDE_8X8 = '[split-bf16]<128x128,patch128+Bdirect>', '[split-bf16]<128x128,patch8x8+Bdirect>'
NARROW_LIN, NARROW_8X8 = '[split-bf16]<128x64,patch128+Bdirect>', '[split-bf16]<128x64,patch8x8+Bdirect>'
# IResNet-50: every 3x3 / stride 1 layer behind the stem -- conv1 and conv2 of every block but the stride-2 conv2 that opens a stage
IRES_BLOCKS = ((1, 3), (2, 4), (3, 14), (4, 3))
IRES_SPLIT = ['layer%d_%d_conv%d' % (s, b, k) for s, nb in IRES_BLOCKS for b in range(nb) for k in (1, 2) if (b, k) != (0, 2)]
IRES_F32 = ['conv1'] + ['layer%d_0_conv2' % s for s, _ in IRES_BLOCKS]


def ires_label(name, side):
    """The form conv_bf3p_form gives a layer of IResNet-50 on a `side` x `side` input: the linear patch where the 128-pixel
    tile's halo patch fits its 232 entries on the m x m map the layer reads (m <= 28), else two 8x8 sub-tiles; 64 columns at 64
    filters, else 128."""
    stage, block, k = (int(t) for t in name.replace('layer', '').replace('conv', '').split('_'))
    m = side >> (stage - 1 if (block, k) == (0, 1) else stage)
    lin = 127 + 2 * (126 // m + 1) + (m + 2) * (126 // (m * m) + 1) + 2 * (m + 2) + 4 <= 232
    return '[split-bf16]<128x%d,%s+Bdirect>' % (64 if stage == 1 else 128, 'patch128' if lin else 'patch8x8')


# YOLOv3 64 x 160: the 3x3 / stride 1 layers of at least 64 filters on maps 32 x 80 .. 4 x 10 (leaky ReLU; the backbone's with a
# shortcut, the heads' without); the 2 x 5 maps are too small -- a 128-pixel tile would wrap rows and images 288 patch entries'
# worth, 232 fit -- and stay on the f32 kernels
YOLO_SPLIT = ['conv_%d' % i for i in (3, 6, 8, 11, 13, 15, 17, 19, 21, 23, 25, 28, 30, 32, 34, 36, 38, 40, 42, 61, 63, 65, 69, 71, 73)]
YOLO_F32 = ['conv_%d' % i for i in (45, 47, 49, 51, 53, 55, 57)]
YOLO_LABEL = dict({'conv_3': NARROW_8X8, 'conv_6': WIDE_8X8, 'conv_8': WIDE_8X8}, **{n: WIDE_LIN for n in YOLO_SPLIT[3:]})
VGG_SPLIT = ['block1_conv2', 'block2_conv1', 'block2_conv2', 'block3_conv1', 'block3_conv2', 'block3_conv3', 'block4_conv1', 'block4_conv2', 'block4_conv3']
RES_SPLIT = ['conv2_block1_2_conv', 'conv2_block2_2_conv', 'conv3_block1_2_conv', 'conv3_block2_2_conv', 'conv3_block3_2_conv']


def split_case(arch, head, emd, hw, n, compute, engaged, f32=(), label_of=None, opts=None, max_batch=None, name='', **want):
    """engaged: the launches that must have run a split-bf16 kernel -- these and no others are swept; f32: launches that must NOT
    have; label_of: {launch: text its label holds}; want: 'res', 'y2', 'prelu', 'leaky', 'y_sub' -> the engaged launches whose
    describe line has it (a list of names, compared exactly)."""
    return {'id': 'bf16-%s-%dx%d-n%d-%s%s' % (arch, hw[0], hw[1], n, compute, ('-' + name) if name else ''), 'net': (arch, head, emd, hw), 'n': n,
            'compute': compute, 'engaged': list(engaged), 'f32': list(f32), 'label_of': dict(label_of or {}), 'opts': dict(opts or {}),
            'max_batch': max_batch or n, 'want': want}


def build_split_cases():
    cases = []
    for compute in ('bf16x3', 'bf16x2'):
        # IResNet-50 112 x 112: 56 x 56 (8x8 form; 64 and 128 columns), 28 / 14 / 7 (linear; at 7 x 7 a tile spans three images);
        # conv2 of a block: BN, shortcut, and the next block's BN as the second output; conv1: BN + PReLU; the last conv2 of a
        # stage stores the even pixels of its first output (the stride-2 shortcut's input)
        conv2 = [n for n in IRES_SPLIT if n.endswith('conv2')]
        cases.append(split_case('iresnet50', 'v2', 512, (112, 112), 3, compute, IRES_SPLIT, IRES_F32, {n: ires_label(n, 112) for n in IRES_SPLIT},
                                res=conv2, y2=conv2, prelu=[n for n in IRES_SPLIT if n.endswith('conv1')],
                                y_sub=['layer1_2_conv2', 'layer2_3_conv2', 'layer3_13_conv2']))
        cases.append(split_case('yolov3', 'v3', 1, (64, 160), 3, compute, YOLO_SPLIT, YOLO_F32, YOLO_LABEL, res=YOLO_SPLIT[:19], leaky=YOLO_SPLIT))
        # the smallest net with a sub-sampled first output in this mode: IResNet-50 at 32 x 32 (maps 16 .. 2) -- the last conv2 of
        # stages 1 and 2 (16 x 16 x 64: 64 columns; 8 x 8 x 128), epilogue variant 2; stage 3's 4 x 4 map stays on the f32 kernels
        small = [n for n in IRES_SPLIT if n < 'layer3_0_conv2' or n == 'layer3_0_conv1']
        cases.append(split_case('iresnet50', 'v2', 512, (32, 32), 3, compute, small, [n for n in IRES_SPLIT if n not in small] + IRES_F32,
                                {n: ires_label(n, 32) for n in small}, name='ysub', y_sub=['layer1_2_conv2', 'layer2_3_conv2']))
    # three terms on the two-term tile (dbg 128: Tile<4, 1, 1, 4> takes the linear 128-column layers): six products
    cases.append(split_case('resnet', 'v3', 512, (96, 64), 37, 'bf16x3', RES_SPLIT, opts={'dbg': 128}, name='bf2-tile'))
    return cases


SPLIT_CASES = build_split_cases()


def run_split_case(zoo, c, env, verbose=False):
    """-> (failures, labels seen, launches checked): the sweep of the launches that ran a split-bf16 kernel, and what the case
    states about them."""
    arch, head, emd, hw = c['net']
    m = zoo.net(arch, head, emd, hw, c['max_batch'], compute=c['compute'], streams=1, monkeypatch=env)
    x = torch.from_numpy(zoo.pool(hw, max(c['n'], 40))[:c['n']]).cuda()
    det = []
    with options(m, **c['opts']):
        fails, seen, checked = layer_sweep.sweep(m, x, c['id'], RECORD, verbose, labels=(SPLIT,), details=det)
        table = {name: kern for name, kern, _ in m.op_table()}
    ran = [name for name, _, _ in det]
    if checked < 1 or ran != c['engaged'] or not all(SPLIT in kern for _, kern, _ in det):
        fails.append('%s: the split-bf16 launches checked are %s, the case states %s' % (c['id'], ran, c['engaged']))
    fails += ['%s: %s ran %s, a split-bf16 kernel' % (c['id'], n, table[n]) for n in c['f32'] if SPLIT in table.get(n, SPLIT)]
    fails += ['%s: %s ran %s, the case states %s' % (c['id'], n, table.get(n), t) for n, t in c['label_of'].items() if t not in table.get(n, '')]
    has = {'res': lambda d: d['res'] is not None, 'y2': lambda d: d['y2'] is not None, 'prelu': lambda d: d['act'] == 'prelu' and d['alpha'],
           'leaky': lambda d: d['act'] == 'prelu' and not d['alpha'] and d['const_alpha'] > 0, 'y_sub': lambda d: d['y_sub'] == 1}
    for key, names in c['want'].items():
        got = [name for name, _, d in det if has[key](d)]
        if got != list(names) or not got:
            fails.append('%s: the checked launches with %s are %s, the case states %s' % (c['id'], key, got, list(names)))
    return fails, seen, checked


@pytest.mark.parametrize('c', SPLIT_CASES, ids=[c['id'] for c in SPLIT_CASES])
def test_split_bf16_launches_against_their_kept_terms(zoo, monkeypatch, c):
    fails, seen, checked = run_split_case(zoo, c, monkeypatch)
    SEEN.update(seen)
    print('%s: %d split-bf16 launches checked' % (c['id'], checked))
    assert checked >= 1
    assert not fails, '%d failures\n' % len(fails) + '\n'.join(fails)


def _vgg_split(zoo, monkeypatch, compute):
    m = zoo.net('vgg16', 'v3', 512, (48, 80), 3, compute=compute, streams=1, monkeypatch=monkeypatch)
    return m, torch.from_numpy(zoo.pool((48, 80), 40)[:3]).cuda()


def test_bf_terms_switched_on_one_model(zoo, monkeypatch):
    """dif_net_set_option("bf_terms") on ONE built model, 3 -> 2 -> 3: each setting passes the gates of ITS tier (the sweep
    reads the tier in force from the model), the two three-term outputs are bit-identical, and the two-term one is another."""
    m, x = _vgg_split(zoo, monkeypatch, 'bf16x3')
    outs = []
    try:
        for terms in (3, 2, 3):
            m.set_option('bf_terms', terms)
            assert m.bf_terms == terms
            det = []
            fails, _, checked = layer_sweep.sweep(m, x, 'terms %d' % terms, None, labels=(SPLIT,), details=det)
            assert [name for name, _, _ in det] == VGG_SPLIT and checked == len(VGG_SPLIT)
            assert not fails, '%d terms: %d failures\n' % (terms, len(fails)) + '\n'.join(fails)
            outs.append(m.embed(x).clone())
    finally:
        m.set_option('bf_terms', 3)
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('compute,ref_terms', [('bf16x2', 3), ('bf16x3', 2)])
def test_split_sweep_tells_the_tiers_apart_on_the_device(zoo, monkeypatch, compute, ref_terms):
    """No defect is planted in any kernel: a model running one tier is swept -- every launch of the net -- against the OTHER
    tier's split reference.  Every split-bf16 launch fails the rms gate; every failure is a gate against the split reference
    (rms, and max where the gap of 2^-17 |x| |w| a product passes 8 x the yardstick's worst element) of a split-bf16 launch:
    the a-priori bounds, against the true layer and against S, still hold, and no other launch fails.  The same sweeps against
    their own tier pass (the cases above)."""
    m, x = _vgg_split(zoo, monkeypatch, compute)
    det = []
    fails, _, checked = layer_sweep.sweep(m, x, 'live', None, ref_terms=ref_terms, details=det)
    print('\n'.join(fails))
    split = [name for name, kern, _ in det if SPLIT in kern]
    assert split == VGG_SPLIT and checked == len(m.op_describe())
    for name in split:
        assert any(f.startswith(name + ' ') and 'rms gate' in f for f in fails), name
    assert all(f.split(' ')[0] in split and 'against the split reference' in f and ('rms gate' in f or 'max gate' in f) for f in fails), fails


# every family the cases are there for (the issue's list); a label matches by containing the text
FAMILIES = ['conv_mt_kernel<16x16,pointwise,4 waves>', 'conv_mt_kernel<16x16,gather,8 waves>', 'conv_mt_kernel<16x16,pointwise,preact,16 waves>',
            'conv_sk_kernel', 'conv_skp_kernel', '+reduce', 'conv_igemm_kernel<128x32', 'conv_igemm_kernel<64x64,gather>', 'stem3x3_kernel',
            'stem_mfma_kernel', 'conv_pipe_kernel', 'conv_bdp_kernel', 'conv_t2_kernel', 'conv_tn_kernel', 'patch8x8', 'patch128>', 'patch168>',
            'patch128+Bdirect', 'patch168+Bdirect', 'conv_wino_kernel<F(2x2,3x3),32 tiles x 64>', 'conv_wino_kernel<F(2x2,3x3),64 tiles x 64>',
            'conv_winow_kernel<F(2x2,3x3),32 tiles x 64>', 'conv_winow_kernel<F(2x2,3x3),64 tiles x 64>',
            'conv_winox_kernel<F(2x2,3x3),32 tiles x 64,odd>', 'conv_winox_kernel<F(2x2,3x3),32 tiles x 64,ysub>',
            'conv_igemm_kernel[split-bf16]', 'input_convert_kernel', 'maxpool_kernel', 'dwconv_kernel', 'upsample2_kernel', 'copy_to_view_kernel',
            K8, K2, AB_TAIL, 'dwfull_kernel', 'l2norm_kernel', 'lrn_kernel', 'memset']
# what the cases ran on the MI355X (split-K factors left out: layer_sweep.family); conv_tn_kernel's third patch size, patch256,
# is reached by ResNet50V2 64 x 96
OBSERVED = ['conv_bdp_kernel<64x64,patch168+Bdirect>', 'conv_bdp_kernel<64x64,patch8x8+Bdirect>',
            'conv_igemm_kernel<128x32,gather>', 'conv_igemm_kernel<128x32,pointwise>', 'conv_igemm_kernel<64x64,gather>',
            'conv_igemm_kernel<64x64,patch128+Bdirect>', 'conv_igemm_kernel<64x64,patch128>',
            'conv_igemm_kernel<64x64,patch168+Bdirect>', 'conv_igemm_kernel<64x64,patch168>',
            'conv_igemm_kernel<64x64,patch8x8+Bdirect>', 'conv_igemm_kernel<64x64,patch8x8>',
            'conv_igemm_kernel<64x64,pointwise,preact>', 'conv_igemm_kernel<64x64,pointwise>',
            'conv_igemm_kernel[split-bf16]<128x128,patch128+Bdirect>',
            'conv_igemm_kernel[split-bf16]<128x128,patch8x8+Bdirect>',
            'conv_igemm_kernel[split-bf16]<128x64,patch128+Bdirect>', 'conv_igemm_kernel[split-bf16]<128x64,patch8x8+Bdirect>',
            'conv_mt_kernel<16x16,gather,16 waves>', 'conv_mt_kernel<16x16,gather,4 waves>',
            'conv_mt_kernel<16x16,gather,8 waves>', 'conv_mt_kernel<16x16,pointwise,16 waves>',
            'conv_mt_kernel<16x16,pointwise,4 waves>', 'conv_mt_kernel<16x16,pointwise,8 waves>',
            'conv_mt_kernel<16x16,pointwise,preact,16 waves>', 'conv_mt_kernel<16x16,pointwise,preact,4 waves>',
            'conv_mt_kernel<16x16,pointwise,preact,8 waves>', 'conv_pipe_kernel<64x64,gather>',
            'conv_pipe_kernel<64x64,pointwise,preact>', 'conv_pipe_kernel<64x64,pointwise>',
            'conv_sk_kernel<64x64,gather>+reduce', 'conv_sk_kernel<64x64,pointwise,preact>+reduce',
            'conv_sk_kernel<64x64,pointwise>+reduce', 'conv_skp_kernel<64x64,patch128+Bdirect>+reduce',
            'conv_skp_kernel<64x64,patch168+Bdirect>+reduce', 'conv_t2_kernel<128x64,2x(patch8x8)+Bdirect>',
            'conv_tn_kernel<64x128,patch128+Bdirect>', 'conv_tn_kernel<64x128,patch168+Bdirect>',
            'conv_tn_kernel<64x128,patch256+Bdirect>', 'conv_wino_kernel<F(2x2,3x3),32 tiles x 64>',
            'conv_wino_kernel<F(2x2,3x3),64 tiles x 64>', 'conv_winow_kernel<F(2x2,3x3),32 tiles x 64>',
            'conv_winow_kernel<F(2x2,3x3),64 tiles x 64>', 'conv_winox_kernel<F(2x2,3x3),32 tiles x 64,odd>',
            'conv_winox_kernel<F(2x2,3x3),32 tiles x 64,ysub>', 'copy_to_view_kernel', 'dwconv_kernel', 'input_convert_kernel',
            'l2norm_kernel', 'maxpool_kernel', 'stem3x3_kernel', 'stem_mfma_kernel', 'upsample2_kernel',
            'dwfull_kernel', K8, K2, AB_TAIL, 'lrn_kernel', 'memset']


def test_union_of_kernel_labels():
    """Runs after the cases above (file order): what they saw, together, holds every family the issue names and every label
    of the recorded run.  A change of dispatch that drops a form from these cases shows here."""
    assert SEEN, 'the cases of this module did not run before this test'
    seen = sorted({layer_sweep.family(s) for s in SEEN})
    print('kernel labels seen over all cases (%d):\n  %s' % (len(seen), '\n  '.join(seen)))
    missing = [k for k in FAMILIES if not any(k in s for s in seen)]
    assert not missing, missing
    assert not sorted(set(OBSERVED) - set(seen)), sorted(set(OBSERVED) - set(seen))
