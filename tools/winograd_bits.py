#!/usr/bin/env python3
"""SHA-256 digests of whole-net outputs (raw float32 bytes) on the cases that reach every conv_wino_kernel instantiation.

    python tools/winograd_bits.py --commit $(git rev-parse HEAD) [--lib libdif_parent.so] [--out tests/golden/winograd_bits.json]
    python tools/winograd_bits.py --cases epilogue --commit ...     (EPILOGUE_CASES -> tests/golden/winograd_epilogue_bits.json)

A change that only re-schedules the Winograd K loop must leave every bit of the outputs where it was.  The suite holds the
kernels to the oracle and to each other, but nothing in it holds one commit to the one before: this file does.  The golden
file is written by running this tool on the GPU with the build of the commit the bits are to be kept from (--lib names
a library in deep-insight-face_amd/lib, as DIF_LIB does; --commit is recorded).  tests/test_winograd_bits_gpu.py imports
CASES, run_case and digest from here and compares.

Single-lane executor (DIF_STREAMS=1 while the nets are finalized), synthetic weights of seed 2024, the seeded uint8 pools
of tests/nonsquare_gates.py (Zoo.pool's seeds), the fused 1 / 255 input transform.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (arch, head, emd, input, images, options, the Winograd kernels that must run -- what the case is there for)
HALF, FULL = '32 tiles x 64', '64 tiles x 64'
CASES = {
    # narrow, wide, odd and y_sub forms; 129 images leave partial last blocks on every map; K of 4 .. 32 steps
    'iresnet50_129': ('iresnet50', 'v2', 512, (112, 112), 129, {'wino': 2},
                      ['conv_wino_kernel<F(2x2,3x3),%s>' % HALF, 'conv_winow_kernel<F(2x2,3x3),%s>' % HALF,
                       'conv_winox_kernel<F(2x2,3x3),%s,odd>' % HALF, 'conv_winox_kernel<F(2x2,3x3),%s,ysub>' % HALF]),
    # the wide maps in the full-size block, two per CU: <64, 2, 2, true>
    'iresnet50_129_wide64': ('iresnet50', 'v2', 512, (112, 112), 129, {'wino': 2, 'dbg': 65536},
                             ['conv_wino_kernel<F(2x2,3x3),%s>' % HALF, 'conv_winow_kernel<F(2x2,3x3),%s>' % FULL,
                              'conv_winox_kernel<F(2x2,3x3),%s,odd>' % HALF, 'conv_winox_kernel<F(2x2,3x3),%s,ysub>' % HALF]),
    # level 1: <64, 2, 1, false> on the 14 x 14 stage, K of 16 steps
    'iresnet50_65_level1': ('iresnet50', 'v2', 512, (112, 112), 65, {'wino': 1}, ['conv_wino_kernel<F(2x2,3x3),%s>' % FULL]),
    # 512 channels: K of 32 steps, no shortcut
    'vgg16_65': ('vgg16', 'v2', 512, (112, 112), 65, {'wino': 2}, ['conv_wino_kernel<F(2x2,3x3),%s>' % HALF]),
    # ReLU epilogues, K of 8 steps on 14 x 14, the 7 x 7 stage on the odd form
    'resnet50v2_129': ('resnet', 'v2', 512, (112, 112), 129, {'wino': 2},
                       ['conv_wino_kernel<F(2x2,3x3),%s>' % HALF, 'conv_winow_kernel<F(2x2,3x3),%s>' % HALF,
                        'conv_winox_kernel<F(2x2,3x3),%s,odd>' % HALF]),
    # Darknet-53 on 32 x 64: conv_3 is 32 -> 64 channels on the 16 x 32 map, K of 2 steps (the shortest the rule admits)
    'yolov3_129': ('yolov3', 'v3', 1, (32, 64), 129, {'wino': 2},
                   ['conv_wino_kernel<F(2x2,3x3),%s>' % HALF, 'conv_winow_kernel<F(2x2,3x3),%s>' % HALF]),
}
K2_LAYER = ('yolov3_129', 'conv_3', 9 * 32 * 64 * 16 * 32)      # (case, layer, its multiply-adds per image: op_table())
DEFAULTS = {'wino': 2, 'dbg': 0}

# A second list, for a change to the half block's epilogue (round 12: one pass through LDS for both column fragments, the
# shortcut tiles requested under the last K-step); tests/test_winograd_epilogue_gpu.py.  Here the last field names the
# layers the case is there for: {layer: (kernel, multiply-adds per image)}, checked against op_table().
ODD, YSUB = 'conv_winox_kernel<F(2x2,3x3),%s,odd>' % HALF, 'conv_winox_kernel<F(2x2,3x3),%s,ysub>' % HALF
EPILOGUE_CASES = {
    # ResNet-50V2 maps out ('v3') at 128 images, the fewest the odd-map rule admits: conv4 on 7 x 9 (4 x 5 tiles: the last tile
    # row and column half off the map) and on 8 x 7 -- masked output pixels in both column fragments of one pass
    'resnet50v2_128_7x9': ('resnet', 'v3', 512, (112, 144), 128, {'wino': 2},
                           {'conv4_block%d_2_conv' % b: (ODD, 9 * 256 * 256 * 7 * 9) for b in range(1, 6)}),
    'resnet50v2_128_8x7': ('resnet', 'v3', 512, (128, 112), 128, {'wino': 2},
                           {'conv4_block%d_2_conv' % b: (ODD, 9 * 256 * 256 * 8 * 7) for b in range(1, 6)}),
    # the y_sub layer with Cout = 64 (one column block): IResNet-50's layer1_2_conv2 on 56 x 56; 129 images are 3 160 whole
    # blocks and a half-filled one, whose dense first store comes from the one-pass layout
    'iresnet50_129_ysub64': ('iresnet50', 'v2', 512, (112, 112), 129, {'wino': 2},
                             {'layer1_2_conv2': (YSUB, 9 * 64 * 64 * 56 * 56)}),
    # K of 2 steps with a shortcut (Darknet-53's conv_3 adds its block's input after the leaky ReLU): the shortcut requests
    # go out one loop pass after the prologue
    'yolov3_129_k2_shortcut': ('yolov3', 'v3', 1, (32, 64), 129, {'wino': 2},
                               {'conv_3': ('conv_winow_kernel<F(2x2,3x3),%s>' % HALF, K2_LAYER[2])}),
}


def check_layers(model, kern, want):
    """The layers an EPILOGUE_CASES entry names ran the kernel it names, on the shape it names."""
    macs = {nm: mac for nm, _, mac in model.op_table()}
    for layer, (kernel, mac) in want.items():
        assert kern.get(layer) == kernel and macs[layer] == mac, (layer, kern.get(layer), macs.get(layer))


def digest(out):
    """SHA-256 over the raw bytes of the output tensor (of every output in order, for a net with several)."""
    h = hashlib.sha256()
    for t in out if isinstance(out, (list, tuple)) else [out]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def pool(hw, n):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import nonsquare_gates as gates
    return gates.frames_u8(n, hw, seed=hw[0] * 1000 + hw[1] + n)


def run_case(model, dev_u8, opts):
    """The digest under `opts` and the Winograd kernels that ran: (hex digest, {layer: kernel}).  Options go back to DEFAULTS."""
    try:
        for k, v in opts.items():
            model.set_option(k, v)
        dig = digest(model.embed(dev_u8))
        kern = {name: k for name, k, _ in model.op_table() if k.startswith(('conv_wino_kernel', 'conv_winow_kernel', 'conv_winox_kernel'))}
    finally:
        for k in opts:
            model.set_option(k, DEFAULTS[k])
    return dig, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', help='library file name under deep-insight-face_amd/lib (DIF_LIB)')
    ap.add_argument('--commit', required=True, help='the commit the library was built from')
    ap.add_argument('--cases', choices=['kloop', 'epilogue'], default='kloop', help='CASES or EPILOGUE_CASES')
    ap.add_argument('--out', help='default: tests/golden/winograd_bits.json, or winograd_epilogue_bits.json for --cases epilogue')
    args = ap.parse_args()
    epi = args.cases == 'epilogue'
    out = args.out or os.path.join(ROOT, 'tests', 'golden', 'winograd_epilogue_bits.json' if epi else 'winograd_bits.json')
    if args.lib:
        os.environ['DIF_LIB'] = args.lib
    os.environ['DIF_STREAMS'] = '1'
    sys.path.insert(0, os.path.join(ROOT, 'deep-insight-face_amd'))
    import torch
    from deep_insight_face.networks.triplet import DifEmbedder
    nets, res = {}, {'commit': args.commit, 'cases': {}}
    for name, (arch, head, emd, hw, n, opts, want) in (EPILOGUE_CASES if epi else CASES).items():
        key = (arch, head, emd, hw, n)
        if key not in nets:
            m = DifEmbedder(arch, head, emd, hw + (3,), max_batch=n).init_synthetic(2024)
            m.set_input_transform(scale=1 / 255.)
            m._finalize()
            nets[key] = m
        dig, kern = run_case(nets[key], torch.from_numpy(pool(hw, n)).cuda(), opts)
        ran = sorted(set(kern.values()))
        if epi:
            check_layers(nets[key], kern, want)
        else:
            assert ran == sorted(want), (name, ran)
        res['cases'][name] = dig
        print('%-22s %s  %d Winograd layers: %s' % (name, dig[:16], len(kern), ', '.join(ran)), flush=True)
        if name == K2_LAYER[0]:
            macs = {nm: mac for nm, _, mac in nets[key].op_table()}
            assert K2_LAYER[1] in kern and macs[K2_LAYER[1]] == K2_LAYER[2], (kern, macs.get(K2_LAYER[1]))
    for m in nets.values():
        m.close()
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
