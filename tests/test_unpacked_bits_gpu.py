"""-m gpu: the kernels built without packed fp32 arithmetic (csrc/Makefile: UNPACKED) write the bytes they wrote before.

tools/make_golden_unpacked_bits.py launches every adopted instance once at its smallest shape that takes every code path --
dp_bwd16s<POOLDY> of both storage types: N = 1 at 32 x 64, N = 3 at 40 x 72 (ragged last strip, several bands), each with a
full-size and with a pooled dy -- and was run once on the library of the commit BEFORE the change
(tests/golden/unpacked_parent_bits.json).  Here the same launches run on the library of the tree: dx and the reduced
weight-gradient row have the same SHA-256 (a packed fma is two fmas: no element's arithmetic changed), the producer's
BN-backward sums -- fp64 atomics in launch order, not reproducible run to run on either library -- agree within the
max-norm bar tests/test_dp_descriptor_gpu.py holds the same sums to against fp64 (5e-5).

The families that stay packed (dp_bwd64, dp_fwd64s, dp_fwd16s, dp_bwd_kernel, stem_mma: slower or unchanged without packing,
profiles/unpacked_fp32.json) are built exactly as before and have no case here.
"""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_SUMS = 5e-5          # tests/test_dp_descriptor_gpu.py: 'in bstats' of the bwd16s cases


def _tool():
    spec = importlib.util.spec_from_file_location('make_golden_unpacked_bits',
                                                  os.path.join(ROOT, 'tools', 'make_golden_unpacked_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(TOOL.GOLDEN) as _f:
    PARENT = json.load(_f)['cases']


def test_every_case_has_a_recorded_parent():
    assert sorted(PARENT) == sorted(TOOL.CASES)


@pytest.mark.parametrize('name', sorted(TOOL.CASES))
def test_same_bits_as_the_parent(name):
    got, want = TOOL.run_case(name), PARENT[name]
    sums = torch.tensor([float.fromhex(v) for v in got['bstats']], dtype=torch.float64)
    ref = torch.tensor([float.fromhex(v) for v in want['bstats']], dtype=torch.float64)
    err = float((sums - ref).abs().max() / ref.abs().max())
    print(f'[{name}] dx {got["dx"][:12]} wgrad {got["wgrad"][:12]} BN-backward sums vs parent {err:.3g}')
    assert got['dx'] == want['dx'], 'dx differs from the parent build'
    assert got['wgrad'] == want['wgrad'], 'reduced weight-gradient row differs from the parent build'
    assert bool(ref.abs().max() > 0) and err < TOL_SUMS, err
