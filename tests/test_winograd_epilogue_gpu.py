"""The half block's one-pass epilogue, held to the bits of the commit before it: SHA-256 of whole-net outputs against
tests/golden/winograd_epilogue_bits.json.

Round 12 changed which wave owns which Winograd component in the four-wave shapes (a column of the 4 x 4 grid, not a row),
lets every wave form the first stage of A^T M A on its own accumulators, sends both 32-channel fragments through LDS in one
pass and requests the shortcut tiles inside the last K-step (conv_winograd.hpp).  Every output is still the same adds in the
same order, so no bit may move: the golden digests were written by tools/winograd_bits.py --cases epilogue with the build of
the parent commit, which the file names.  There is no tolerance.

Cases (tools/winograd_bits.py: EPILOGUE_CASES), single lane -- what tests/golden/winograd_bits.json does not pin, or
pins without saying so, and the new code could get wrong:
  resnet50v2_128_7x9      ResNet-50V2 'v3' on 112 x 144 at 128 images, the fewest the odd-map rule admits: conv4 on 7 x 9,
  resnet50v2_128_8x7      and on 128 x 112: 8 x 7.  Output pixels beyond the map are masked in both fragments of one pass
                          (test_winograd_rest_gpu.py holds these maps to a gate, not to bits)
  iresnet50_129_ysub64    the y_sub layer with Cout = 64 (layer1_2_conv2, 56 x 56): a partial last block and the dense first
                          store out of the one-pass layout
  yolov3_129_k2_shortcut  Darknet-53 on 32 x 64: conv_3 is a K loop of 2 steps that carries a shortcut, so the shortcut
                          requests go out one loop pass after the prologue
Each case asserts from op_table() that the layers it is there for ran the kernel it means, on the shape it means.
"""
import importlib.util
import json
import os

import pytest
import torch

from test_nonsquare_gpu import Zoo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('winograd_bits', os.path.join(ROOT, 'tools', 'winograd_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope='module')
def zoo(cuda):
    z = Zoo()
    yield z
    z.close()


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'winograd_epilogue_bits.json')) as fh:
        return json.load(fh)


def test_golden_lists_every_case(golden):
    assert sorted(golden['cases']) == sorted(bits.EPILOGUE_CASES)
    assert len(golden['commit']) == 40


def test_cases_sit_on_the_rules_edge():
    """128 images are the fewest the odd-map rule admits on both maps (128 images, and 2 048 tiles of the padded grid)."""
    for name in ('resnet50v2_128_7x9', 'resnet50v2_128_8x7'):
        _, _, _, hw, n, _, _ = bits.EPILOGUE_CASES[name]
        h, w = -(-hw[0] // 16), -(-hw[1] // 16)
        assert (h & 1) or (w & 1)
        assert n == 128 and n * ((h + 1) // 2) * ((w + 1) // 2) >= 128 * 16


@pytest.mark.parametrize('name', list(bits.EPILOGUE_CASES))
def test_bits_unchanged(zoo, monkeypatch, golden, name):
    arch, head, emd, hw, n, opts, want = bits.EPILOGUE_CASES[name]
    m = zoo.net(arch, head, emd, hw, n, streams=1, monkeypatch=monkeypatch)
    dig, kern = bits.run_case(m, torch.from_numpy(zoo.pool(hw, n)).cuda(), opts)
    bits.check_layers(m, kern, want)
    print('%s: %s (golden %s, commit %s)' % (name, dig, golden['cases'][name], golden['commit'][:7]))
    assert dig == golden['cases'][name]
