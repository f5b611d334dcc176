"""-m gpu: the pooled 16 -> 16 forward without its full-size output (a null YunetDP.z: dp_fwd16s_kernel<16,true>'s body
without the z path) writes the same winners, window positions and BatchNorm sums, byte for byte, as with one -- at the
kernel's entry and through one whole training step of the engine."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import yunet_amd._lib as L

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 32 x 64: the streaming kernel's minimum map, one band set, strips cut at the right edge only by the halo;
# 34 x 70: a ragged right edge and 17 row pairs (an odd number per band whatever the band height);
# 64 x 160: six 28-column strips per row, several tasks per wave on a small grid
MAPS = [(32, 64), (34, 70), (64, 160)]


def unit_inputs(h, w, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    n, c = 2, 16
    x = (torch.randn(n, h, w, c, generator=g) * 1.5 + 0.3).to(dtype)
    ws = [torch.randn(c, c, generator=g) * 0.25, torch.randn(c, generator=g) * 0.1,
          torch.randn(c, 9, generator=g) * 0.3, torch.randn(c, generator=g) * 0.1]
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[1], gamma[13], gamma[5] = -gamma[1], -0.7, 0.0         # falling BN: the minimum wins; constant: position 0
    xs = x.double().reshape(-1, c)
    in_stats = torch.cat([xs.sum(0), (xs * xs).sum(0)])          # the producer's BatchNorm sums (BN + ReLU input transform)
    return n, c, x, ws, gamma, torch.randn(c, generator=g) * 0.3, in_stats


def run_unit(k, n, c, h, w, x, ws, gamma, beta, in_stats, with_z):
    """yunet_dp_fwd on the pooled unit -> (z | guard, pooled, idx, stats): with_z = False passes a null z and puts a
    sentinel-filled buffer where z was allocated in the other run"""
    in_bn = k.BN(in_stats.clone(), torch.ones(c, device=DEV), torch.zeros(c, device=DEV), n * h * w)
    out_bn = k.BN(torch.zeros(2 * c, dtype=torch.float64, device=DEV), gamma, beta, n * h * w)
    z = torch.full((n, h, w, c), -777.0, device=DEV, dtype=x.dtype)
    pooled = torch.full((n, h // 2, w // 2, c), 555.0, device=DEV, dtype=x.dtype)
    idx = torch.full((n, h // 2, w // 2, c), 99, device=DEV, dtype=torch.uint8)
    d = k._dp_desc(x, *ws, z, in_bn, out_bn)
    d.pool_out, d.pool_idx = pooled.data_ptr(), idx.data_ptr()
    if not with_z:
        d.z = None
    fn = getattr(L.load(), 'yunet_dp_fwd' + ('_bf16' if x.dtype == torch.bfloat16 else ''))
    L.check(fn(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'yunet_dp_fwd')
    torch.cuda.synchronize()
    return z, pooled, idx, out_bn.stats


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('h,w', MAPS)
def test_kernel_same_bytes_without_z(h, w, dtype):
    import yunet_amd.kernels as k
    n, c, x, ws, gamma, beta, in_stats = unit_inputs(h, w, dtype, 7 * h + w)
    dev = [t.to(DEV) for t in (x, *ws, gamma, beta, in_stats)]
    args = (k, n, c, h, w, dev[0], dev[1:5], dev[5], dev[6], dev[7])
    z, pooled, idx, stats = run_unit(*args, with_z=True)
    assert not bool((z == -777.0).all()) and not bool((pooled == 555.0).any()) and not bool((idx == 99).any())
    zptr = z.data_ptr()
    ref = (pooled.cpu(), idx.cpu(), stats.cpu())
    del z
    guard, pooled2, idx2, stats2 = run_unit(*args, with_z=False)
    print(f'[pool z {h}x{w} {dtype}] guard at the former z: {guard.data_ptr() == zptr}')
    assert bool((guard == -777.0).all()), 'the run with a null z wrote where z would have been'
    assert torch.equal(pooled2.cpu().view(torch.uint8), ref[0].view(torch.uint8))
    assert torch.equal(idx2.cpu(), ref[1])
    assert torch.equal(stats2.cpu().view(torch.int64), ref[2].view(torch.int64))
    # the sums are those of the full-size output the first run stored (fp32 storage: the very values summed)
    if dtype == torch.float32:
        z, _, _, _ = run_unit(*args, with_z=True)
        zz = z.double().reshape(-1, c).cpu()
        want = torch.cat([zz.sum(0), (zz * zz).sum(0)])
        assert float((stats2.cpu() - want).abs().max() / want.abs().max()) < 1e-5


def test_null_z_rejected_on_the_device():
    """the same host-side refusals as tests/test_pool_z_elision_plan.py, with device pointers: nothing is launched, and
    the buffers stay as they were"""
    import yunet_amd.kernels as k
    n, h, w = 2, 32, 64
    for cin, cout, pool in ((16, 16, False), (64, 64, True), (16, 64, False)):
        x = torch.randn(n, h, w, cin, device=DEV)
        ws = [torch.randn(cout, cin, device=DEV), torch.zeros(cout, device=DEV), torch.randn(cout, 9, device=DEV),
              torch.zeros(cout, device=DEV)]
        out_bn = k.BN(torch.zeros(2 * cout, dtype=torch.float64, device=DEV), torch.ones(cout, device=DEV),
                      torch.zeros(cout, device=DEV), n * h * w)
        z = torch.zeros(n, h, w, cout, device=DEV)
        pooled = torch.full((n, h // 2, w // 2, cout), 555.0, device=DEV)
        idx = torch.full((n, h // 2, w // 2, cout), 99, device=DEV, dtype=torch.uint8)
        d = k._dp_desc(x, *ws, z, None, out_bn)
        if pool:
            d.pool_out, d.pool_idx = pooled.data_ptr(), idx.data_ptr()
        d.z = None
        rc = L.load().yunet_dp_fwd(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == L.EINVAL, (cin, cout, pool, rc)
        assert bool((pooled == 555.0).all()) and bool((idx == 99).all()) and float(out_bn.stats.abs().sum()) == 0.0


@pytest.fixture(scope='module')
def steps(tmp_path_factory):
    """{switch: {mode: results}}: one child process per value of YUNET_KEEP_POOL_Z (the switch is read when a plan is
    built, the C options once per process), each running the three modes"""
    out = {}
    for keep in ('0', '1'):
        path = tmp_path_factory.mktemp('pool_z') / f'keep{keep}.pt'
        env = dict(os.environ, YUNET_KEEP_POOL_Z=keep)
        subprocess.check_call([sys.executable, os.path.join(ROOT, 'tests', 'pool_z_elision_child.py'), str(path)], env=env,
                              cwd=ROOT, timeout=300)
        out[keep] = torch.load(path, weights_only=False)
    return out


@pytest.mark.parametrize('mode', ['fp32', 'deterministic', 'bf16'])
def test_training_step_same_bytes(steps, mode):
    """YuNet_n, N = 4, 128 x 128 (the stem's map is 64 x 64: dp_fwd16s<16,true> and dp_bwd16s): one training step with the
    elision and one with YUNET_KEEP_POOL_Z=1 -- the five losses, the flat gradient, the parameters and the momentum after
    the SGD step and the BatchNorm running statistics, byte for byte.  (deterministic: the tile kernels read z, so the
    plan keeps it under either value of the switch.)"""
    a, b = steps['0'][mode], steps['1'][mode]
    assert b['elided'] == 0 and a['elided'] == (0 if mode == 'deterministic' else 1)
    assert a['log'] == b['log'] and all(v == v and v > 0 for v in a['log'])
    for key in ('losses', 'grad', 'params', 'momentum', 'running_mean', 'running_var', 'num_batches_tracked'):
        ta, tb = a[key], b[key]
        assert ta.dtype == tb.dtype and ta.shape == tb.shape and ta.numel() > 0
        assert torch.equal(ta.contiguous().view(torch.uint8), tb.contiguous().view(torch.uint8)), (mode, key)
    assert float(a['grad'].abs().sum()) > 0 and bool(torch.isfinite(a['grad']).all())


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_plan_on_the_device(precision, monkeypatch):
    """the plan of a bound engine: the unit's forward op carries a null z and the plan holds one buffer of that size
    fewer than under the switch; forward_eval on the same plan allocates it and fills it"""
    import yunet_amd.engine as E
    import yunet_oracle as O
    monkeypatch.delenv('YUNET_KEEP_POOL_Z', raising=False)
    eng = E.YuNetEngine(O.yunet_arch('n'), DEV)
    eng.set_precision(precision)
    plan = eng.get_plan(4, 128, 128, 64)
    monkeypatch.setenv('YUNET_KEEP_POOL_Z', '1')
    kept = E.Plan(eng, 4, 128, 128, 64)
    numel = 4 * 64 * 64 * 16

    def count(p):
        return sum(1 for _, z in p.tensors.values() if z.buf is not None and z.buf.numel() == numel)
    f = [op for op in plan.c_fwd_a if op.opcode == L.OP_DP_FWD and op.dp.pool_out and op.dp.cin == 16]
    fk = [op for op in kept.c_fwd_a if op.opcode == L.OP_DP_FWD and op.dp.pool_out and op.dp.cin == 16]
    assert len(f) == len(fk) == 1 and f[0].dp.z is None and fk[0].dp.z
    assert count(kept) - count(plan) == 1
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(4, 3, 128, 128, generator=g) * 255).to(DEV)
    eng.forward_eval(img)
    torch.cuda.synchronize()
    assert eng.plan is plan
    z = plan.tensors['backbone.model0.conv2'][1].buf
    assert z is not None and z.numel() == numel and bool(torch.isfinite(z.float()).all())
    z.fill_(-777.0)                                     # (a fresh engine's parameters are zeros: so is a written z)
    eng.forward_eval(img)
    torch.cuda.synchronize()
    assert not bool((z == -777.0).any()), 'the eval forward does not write the full-size output'
