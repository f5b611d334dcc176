"""CPU: tests/frozen_ref.py is the composition it claims to be, its inputs tell a frozen BatchNorm from a training-mode
one, and torch's own fp32 autograd of the same composition stays inside every bar that
tests/test_frozen_bn_kernels_gpu.py holds the kernels to (the errors are printed: pytest -s)."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16_ref as R
import frozen_ref as FR
from test_dp_descriptor_gpu import BWD, NOT_WALKS, note
from test_kernels_gpu import nchw, nhwc, rel_err

F64, F32 = torch.float64, torch.float32
MIXED = ['tile-16x64-ragged', 'big16-ragged', 'bwd64-8w-ragged', 'bwd64-4w', 'bwd64-packed-5x10', 'bwd16s-ragged',
         'head-unpacked']
CASES = [(cid, 'ff') for cid in NOT_WALKS] + [(cid, rg) for cid in MIXED for rg in ('ft', 'tf') if cid != 'head-unpacked']
STEM = [(2, 32, 32), (3, 64, 96), (1, 20, 36), (5, 66, 150)]


@functools.lru_cache(maxsize=None)
def case(cid, regime):
    return FR.unit_case_of(BWD[cid], regime)


def bn_eval(p):
    bn = nn.BatchNorm2d(p.m.numel()).double()
    with torch.no_grad():
        bn.running_mean.copy_(p.m)
        bn.running_var.copy_(p.v)
        bn.weight.copy_(p.gamma.double())
        bn.bias.copy_(p.beta.double())
    return bn.eval()


def close(a, b, tol=1e-12):
    assert rel_err(a, b) < tol, rel_err(a, b)


# ------------------------------------------------------------------------------------------------ the composition
@pytest.mark.parametrize('cid', ['tile-16x64-ragged', 'bwd64-pooled', 'head-unpacked'])
def test_unit_composition_is_batchnorm_eval(cid):
    """[frozen BN + ReLU ->] conv1x1 -> dw3x3 [-> frozen BN + ReLU] with nn.BatchNorm2d(...).eval() inside autograd: the
    same gradients to 1e-12, the input layer's d(beta) | d(gamma) are the consumer sums, dy is the masked gradient"""
    u = case(cid, 'ff')
    cin, cout = u.cin, u.cout
    bn_in, bn_out = bn_eval(u.inp), (bn_eval(u.out) if u.out_mode == 'frozen' else None)
    x = u.x32.double()
    W = [t.double().clone().requires_grad_(True) for t in u.unit]
    y_in = bn_in(x)
    y_in.retain_grad()
    z = F.conv2d(F.conv2d(F.relu(y_in), W[0], W[1]), W[2], W[3], padding=1, groups=cout)
    if bn_out is not None:
        zb = bn_out(z)
        zb.retain_grad()
        (F.relu(zb) * u.r).sum().backward()
        dy = nhwc(zb.grad)
        if u.idx is not None:
            dy = torch.gather(R.windows(dy), -1, u.idx.long().unsqueeze(-1)).squeeze(-1)
        assert torch.equal(dy, u.dy)
    else:
        (z * u.r * u.scale.double().view(1, -1, 1, 1)).sum().backward()
    close(nhwc(z.detach()), u.z)
    close(nhwc(y_in.grad), u.ref['dx'])
    close(W[0].grad.reshape(cout, cin), u.ref['dw1'])
    close(W[1].grad, u.ref['db1'])
    close(W[2].grad.reshape(cout, 9), u.ref['dw2'])
    close(W[3].grad, u.ref['db2'])
    close(torch.cat([bn_in.bias.grad, bn_in.weight.grad]), u.ref['in_sums'])
    FR.check_dead(u, u.ref)


@pytest.mark.parametrize('cid', ['tile-16x64-ragged', 'head-unpacked', 'bwd64-pooled'])
def test_bf16_contract_reference_is_the_composition(cid):
    """bf16_ref.bwd_ref (the reference of the bf16-storage rows) given the frozen blocks as sums and zero backward sums,
    without its roundings: the autograd composition to 1e-12"""
    u = case(cid, 'ff')
    cin, cout = u.cin, u.cout
    W = [u.unit[0].view(cout, cin), u.unit[1], u.unit[2].view(cout, 9), u.unit[3]]
    ob = R.BNRef(u.out.stats, u.out.gamma, u.out.beta, u.count, bstats=u.out.bst) if u.out_mode == 'frozen' else None
    br = R.bwd_ref(nhwc(u.x32).double(), *W, z=u.z, dy=u.dy, in_bn=R.BNRef(u.inp.stats, u.inp.gamma, u.inp.beta, u.count),
                   out_bn=ob, dy_scale=None if ob is not None else u.scale, pool_idx=u.idx)
    for name in ('dx', 'dw1', 'db1', 'dw2', 'db2'):
        close(br[name], u.ref[name], 1e-11)
    close(br['in_bst'], u.ref['in_sums'], 1e-11)


def test_stem_pool_upadd_compositions_are_batchnorm_eval():
    s = FR.stem_case(1, 20, 36)
    bn = bn_eval(s.bn)
    wt, b = s.wt.double().requires_grad_(True), s.b.double().requires_grad_(True)
    (F.relu(bn(F.conv2d(s.img.double(), wt, b, stride=2, padding=1))) * s.r).sum().backward()
    close(wt.grad, s.dw)
    close(b.grad, s.db)
    assert float(s.db[FR.DEAD]) == 0.0 and float(s.dw[FR.DEAD].abs().max()) == 0.0 and float(s.db.abs().min()) == 0.0
    e = FR.ew_case(16)
    bna, bnb = bn_eval(e.a), bn_eval(e.b)
    za, zb = nchw(e.za).double().requires_grad_(True), nchw(e.zb).double().requires_grad_(True)
    ya = bna(za)
    ya.retain_grad()
    ((F.max_pool2d(F.relu(ya), 2) * nchw(e.r_p)).sum() + (F.relu(ya) * nchw(e.r_e)).sum()).backward()
    close(nhwc(ya.grad), e.pool_extra[0])
    close(torch.cat([bna.bias.grad, bna.weight.grad]), e.pool_extra[1])
    bna, bnb = bn_eval(e.a), bn_eval(e.b)
    ya, yb = bna(za), bnb(zb)
    ya.retain_grad(), yb.retain_grad()
    ((F.relu(ya) + F.interpolate(F.relu(yb), scale_factor=2., mode='nearest')) * nchw(e.r_e)).sum().backward()
    close(nhwc(ya.grad), e.upadd[0])
    close(nhwc(yb.grad), e.upadd[2])
    close(torch.cat([bna.bias.grad, bna.weight.grad]), e.upadd[1])
    close(torch.cat([bnb.bias.grad, bnb.weight.grad]), e.upadd[3])


# ------------------------------------------------------------------------------------------------ the inputs
def check_layer(p, t, count):
    """the fixed channels of a frozen layer over the NCHW tensor t"""
    y, xhat = FR.fbn(t.double(), p.m, p.v, p.gamma, p.beta)
    assert float(p.gamma[FR.NEG]) < 0 and float(p.gamma[FR.ZERO]) == 0 and float(p.beta[FR.ZERO]) > 0
    assert float(y[:, FR.DEAD].max()) < 0 and float(y[:, FR.ALIVE].min()) > 0
    far = float(p.m[FR.FAR].abs() / p.v[FR.FAR].sqrt())
    assert 20 < far < 125, far          # 50 exp(-N(0, 0.5^2) / 2 ...): within a factor of 2.5
    assert torch.equal(p.m, p.m.float().double()) and torch.equal(p.v, p.v.float().double())
    assert torch.equal(p.stats, torch.cat([p.m * count, (p.v + p.m * p.m) * count]))
    batch = t.double().mean(dim=(0, 2, 3))
    assert float(((p.m - batch).abs() / t.double().std(dim=(0, 2, 3))).max()) > 0.3, 'statistics too near the batch'
    return far


@pytest.mark.parametrize('cid,regime', CASES)
def test_unit_case_inputs_and_fp32_autograd(cid, regime):
    """Per case of the GPU file: the fixed channels are what they are called; the margin moved at most one element in
    1000; db2 behind a frozen layer is far from the training-mode db2 (~ 0) of the same inputs -- more than 100 bars, so
    a kernel that still subtracts batch sums cannot pass; and torch's fp32 autograd of the composition is inside every
    bar (bf16 rows whose contract rounds GEMM operands have no fp32 counterpart: inputs only)."""
    u = case(cid, regime)
    tol = BWD[cid].get('tol', 5e-5)
    print(f'[{cid} {regime}] elements moved off the threshold: {u.moved} of {u.x32.numel()}')
    assert u.moved * 1000 <= u.x32.numel()
    if u.in_mode == 'frozen':
        check_layer(u.inp, u.x32, u.count)
    if u.out_mode == 'frozen':
        check_layer(u.out, nchw(u.z.double()), u.count)
        assert not bool(u.out.bst.any())
        dy = nchw(R.expand_pooled(u.dy, u.idx)) if u.idx is not None else nchw(u.dy)
        assert not bool(dy[:, FR.DEAD].any()) and bool((dy[:, FR.ALIVE] != 0).any())
        # the same inputs behind a training-mode BatchNorm: sum(dz) = 0 per channel
        if not u.bf16:
            train = FR.unit_grads(u, out_mode='train').g['db2']
            margin = rel_err(train, u.ref['db2']) / tol
            print(f'[{cid} {regime}] frozen db2 max {float(u.ref["db2"].abs().max()):.4g}, training-mode db2 max '
                  f'{float(train.abs().max()):.3g}: {margin:.3g} bars apart')
            assert margin > 100
        assert float(u.ref['db2'].abs().max()) > 0 and float(u.ref['db2'][FR.DEAD]) == 0.0 == float(u.ref['db2'][FR.ZERO])
    FR.check_dead(u, u.ref)
    # the premise of the per-channel bars (frozen_ref.SEED_BUMP): no channel far below the tensor's maximum
    cdx, cdw1 = FR.conditioning(u.ref['dx'], 3), FR.conditioning(u.ref['dw1'], 0)
    print(f'[{cid} {regime}] max / weakest channel max: dx {cdx:.1f}, dw1 {cdw1:.1f}')
    assert cdx <= 16 and cdw1 <= 120
    if u.bf16 and u.cin == 64 and u.cout == 64:
        return
    if u.bf16:      # fp32 arithmetic on the widened stored tensors: the contract of these rows
        got = _fp32_bf16_row(u)
    else:
        f = FR.unit_grads(u, F32, dy_mask=u.mask)
        got = dict(f.g, bst=f.g.get('in_sums'))
    FR.check_unit(u, got, tol, note, f'fp32 cpu {regime}', FR.DB2_CH_BAR.get((cid, regime)))


def _fp32_bf16_row(u):
    """torch fp32 autograd on a bf16 row's stored tensors: dz from the given dy, as bf16_ref.bwd_ref"""
    cout = u.cout
    x = nchw(nhwc(u.x32)).float()
    W = [t.float().clone().requires_grad_(True) for t in u.unit]
    y_in, xhat = FR.fbn(x, u.inp.m, u.inp.v, u.inp.gamma, u.inp.beta)
    b_in = y_in.detach().requires_grad_(True)
    z = F.conv2d(F.conv2d(F.relu(b_in), W[0], W[1]), W[2], W[3], padding=1, groups=cout)
    if u.out_mode == 'frozen':
        k1 = (u.out.gamma.double() / torch.sqrt(u.out.v + FR.EPS)).float()
        dz = nchw(u.dy).float() * k1.view(1, -1, 1, 1)
    else:
        dz = nchw(u.dy).float() * u.scale.view(1, -1, 1, 1)
    (z * dz).sum().backward()
    return dict(dx=nhwc(b_in.grad), dw1=W[0].grad, db1=W[1].grad, dw2=W[2].grad, db2=W[3].grad,
                bst=FR.sums(b_in.grad.double(), xhat.double()))


@pytest.mark.parametrize('n,h,w', STEM)
def test_stem_case_fp32_autograd(n, h, w):
    """the stem cases: fixed channels, and the errors of torch's fp32 autograd that set the GPU file's db bar"""
    s = FR.stem_case(n, h, w)
    check_layer(s.bn, nchw(s.z), s.count)
    dwm, dbm = float(s.dw.abs().max()), float(s.db.abs().max())
    print(f'[stem {n}x{h}x{w}] fp32 cpu autograd: dw {s.err32[0] / dwm:.3g} of max |dw|, db {s.err32[1] / dbm:.3g} of max |db| '
          f'-> db bar {max(10 * s.err32[1] / dbm, 1e-5):.3g}')
    assert s.err32[0] / dwm < 1e-4
    assert float(s.db[FR.DEAD]) == 0.0 and float(s.db[FR.ZERO]) == 0.0 and float(s.db[FR.ALIVE]) != 0.0


@pytest.mark.parametrize('c', [16, 32, 64])
def test_ew_case(c):
    """the element-wise cases: fixed channels, no near-tie between a live window's two largest activations (fp32 and
    fp64 then agree on the winner), the four-way ties of the constant channel go to position 0, dead channels carry 0"""
    e = FR.ew_case(c)
    for p, z in ((e.a, e.za), (e.b, e.zb)):
        check_layer(p, nchw(z), z.numel() // c)
        assert p.moved * 1000 <= z.numel()
    print(f'[ew {c}] smallest gap between a window\'s maximum and its runner-up: {e.gap:.3g}')
    assert e.gap > 1e-5
    dx = e.pool[0]
    assert torch.equal(dx[:, 0::2, 0::2, FR.ZERO], e.r_p[..., FR.ZERO])
    assert float(dx[..., FR.ZERO].abs().sum()) == float(e.r_p[..., FR.ZERO].abs().sum())
    for d in (e.pool[0], e.pool_extra[0], e.upadd[0], e.upadd[2]):
        assert not bool(d[..., FR.DEAD].any())
    for sm in (e.pool[1], e.pool_extra[1], e.upadd[1], e.upadd[3]):
        assert float(sm[FR.DEAD]) == 0.0 == float(sm[c + FR.DEAD])
