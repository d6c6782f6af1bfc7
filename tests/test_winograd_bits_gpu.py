"""The Winograd kernels' bits, held across commits: SHA-256 of whole-net outputs against tests/golden/winograd_bits.json.

The other Winograd tests hold every block shape to the oracle (cosine gap 1e-5), to each other bit for bit and run to run;
none of them would notice a build whose every shape moved together by one rounding.  A change to how conv_wino_kernel's K
loop is scheduled (conv_winograd.hpp, round 11) changes no product and no order of summation, so it must change no bit:
the golden digests were written by tools/winograd_bits.py with the build of the commit the file names, the parent of the
change.  A digest that differs is a failure -- there is no tolerance.  (A later change that means to alter the arithmetic
regenerates the file with the tool and says so.)

Cases (tools/winograd_bits.py: CASES), the smallest that reach every instantiation, single lane:
  iresnet50_129         level 2: narrow, wide, odd and y_sub forms, partial last blocks, K of 4 .. 32 steps
  iresnet50_129_wide64  the same under `dbg` 65536: the wide maps on <64, 2, 2, true>
  iresnet50_65_level1   level 1: <64, 2, 1, false>, K of 16 steps
  vgg16_65              K of 32 steps, no shortcut
  resnet50v2_129        ReLU epilogue, K of 8 steps, the 7 x 7 stage
  yolov3_129            Darknet-53 on 32 x 64: conv_3 (32 -> 64 channels, 16 x 32 map) is a K loop of 2 steps, the shortest
                        wino_applies admits; leaky ReLU with the shortcut after it
Each case also asserts the set of Winograd kernels that ran, so a case cannot quietly stop reaching its instantiation.
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
    with open(os.path.join(golden_dir, 'winograd_bits.json')) as fh:
        return json.load(fh)


def test_golden_lists_every_case(golden):
    assert sorted(golden['cases']) == sorted(bits.CASES)
    assert len(golden['commit']) == 40


@pytest.mark.parametrize('name', list(bits.CASES))
def test_bits_unchanged(zoo, monkeypatch, golden, name):
    arch, head, emd, hw, n, opts, want = bits.CASES[name]
    m = zoo.net(arch, head, emd, hw, n, streams=1, monkeypatch=monkeypatch)
    dig, kern = bits.run_case(m, torch.from_numpy(zoo.pool(hw, n)).cuda(), opts)
    assert sorted(set(kern.values())) == sorted(want), kern
    if name == bits.K2_LAYER[0]:
        macs = {nm: mac for nm, _, mac in m.op_table()}
        assert bits.K2_LAYER[1] in kern and macs[bits.K2_LAYER[1]] == bits.K2_LAYER[2]
    print('%s: %s (golden %s, commit %s)' % (name, dig, golden['cases'][name], golden['commit'][:7]))
    assert dig == golden['cases'][name]
