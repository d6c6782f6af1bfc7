"""Layer taps: every launch of a net against a float64 reference of THAT layer, fed the input the kernel read.

The whole-net tests see a convolution kernel through thirty layers and an L2 normalisation; a defect in one tile, one
border column, one K-step or one shortcut element of one layer passes their gates.  Here every case taps every launch
(`DifEmbedder.tap`), computes the layer on the device in float64 (tests/layer_ref.py: a sum over taps, no library
convolution) and holds every element of every image to the a-priori rounding bound, and the layer's worst relative error to
8 x that of a float32 run of the same reference (tests/layer_sweep.py states the gates; tests/test_layer_ref.py shows on
the CPU that they pass float32 arithmetic and reject five planted one-place defects).

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


def case(group, arch, head, emd, hw, n, opts=None, expect=(), absent=(), compute='f32', max_batch=None, name=''):
    return {'id': '%s-%s-%dx%d-n%d%s' % (group, arch, hw[0], hw[1], n, ('-' + name) if name else ''), 'net': (arch, head, emd, hw),
            'n': n, 'opts': dict(opts or {}), 'expect': tuple(expect), 'absent': tuple(absent), 'compute': compute,
            'max_batch': max_batch or n}


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
    return cases


CASES = build_cases()


def run_case(zoo, c, env, verbose=False):
    """-> (failures, kernel labels seen, launches checked); the net is built on one lane and its options restored."""
    arch, head, emd, hw = c['net']
    m = zoo.net(arch, head, emd, hw, c['max_batch'], compute=c['compute'], streams=1, monkeypatch=env)
    x = torch.from_numpy(zoo.pool(hw, max(c['n'], 40))[:c['n']]).cuda()
    with options(m, **c['opts']):
        fails, seen, checked = layer_sweep.sweep(m, x, c['id'], RECORD, verbose)
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


# every family the cases are there for (the issue's list); a label matches by containing the text
FAMILIES = ['conv_mt_kernel<16x16,pointwise,4 waves>', 'conv_mt_kernel<16x16,gather,8 waves>', 'conv_mt_kernel<16x16,pointwise,preact,16 waves>',
            'conv_sk_kernel', 'conv_skp_kernel', '+reduce', 'conv_igemm_kernel<128x32', 'conv_igemm_kernel<64x64,gather>', 'stem3x3_kernel',
            'stem_mfma_kernel', 'conv_pipe_kernel', 'conv_bdp_kernel', 'conv_t2_kernel', 'conv_tn_kernel', 'patch8x8', 'patch128>', 'patch168>',
            'patch128+Bdirect', 'patch168+Bdirect', 'conv_wino_kernel<F(2x2,3x3),32 tiles x 64>', 'conv_wino_kernel<F(2x2,3x3),64 tiles x 64>',
            'conv_winow_kernel<F(2x2,3x3),32 tiles x 64>', 'conv_winow_kernel<F(2x2,3x3),64 tiles x 64>',
            'conv_winox_kernel<F(2x2,3x3),32 tiles x 64,odd>', 'conv_winox_kernel<F(2x2,3x3),32 tiles x 64,ysub>',
            'conv_igemm_kernel[split-bf16]', 'input_convert_kernel', 'maxpool_kernel', 'dwconv_kernel', 'upsample2_kernel', 'copy_to_view_kernel']
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
            'l2norm_kernel', 'maxpool_kernel', 'stem3x3_kernel', 'stem_mfma_kernel', 'upsample2_kernel']


def test_union_of_kernel_labels():
    """Runs after the cases above (file order): what they saw, together, holds every family the issue names and every label
    of the recorded run.  A change of dispatch that drops a form from these cases shows here."""
    assert SEEN, 'the cases of this module did not run before this test'
    seen = sorted({layer_sweep.family(s) for s in SEEN})
    print('kernel labels seen over all cases (%d):\n  %s' % (len(seen), '\n  '.join(seen)))
    missing = [k for k in FAMILIES if not any(k in s for s in seen)]
    assert not missing, missing
    assert not sorted(set(OBSERVED) - set(seen)), sorted(set(OBSERVED) - set(seen))
