"""csrc/optim.hip under the rule of tests/test_isa_guard.py (no GPU needed): no loop that waits out each of its loads."""
import os
import subprocess

import pytest

import test_isa_guard as G


@pytest.mark.skipif(not os.path.exists(G.HIPCC), reason='hipcc not found')
def test_optim_kernels_have_no_loop_that_waits_out_every_load(tmp_path):
    out = str(tmp_path / 'optim.s')
    subprocess.run([G.HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-w', '-S', '--cuda-device-only', '-o', out,
                    os.path.join(G.CSRC, 'optim.hip')], check=True, capture_output=True, timeout=600)
    found = [f for f in G._scanner().scan(out) if f[1] >= 10]
    assert not found, found
    text = open(out).read()
    for kernel in ('grad_norm_kernel', 'sgd_grouped_kernel', 'adam_grouped_kernel'):
        assert kernel in text
