"""The optimizer-surface kernels (csrc/optim.hip) through kernels.py against torch on the CPU.

Yardstick (everywhere a result is not required to be bit-identical): torch's own fp32 result against the fp64 run of the
same torch code on the same inputs.  The device may deviate from the fp64 run by at most 4 x what torch fp32 deviates
(the 4 x covers another reduction order / FMA contraction, not another formula), with a floor of one fp32 ulp of the
largest value compared.  Both deviations are printed before the assertion (pytest -s).

Measured on an MI355X (deviation from fp64: device / torch fp32 / bound):
  L2 norm, n = 3 tiles + 5:   2.082e-06 / 5.547e-06 / 2.219e-05      (the device sums in fp64 and rounds once)
  L2 norm, n = 257 tiles + 3: 5.273e-05 / 1.055e-02 / 4.220e-02
  L1 norm, n = 3 tiles + 5:   4.474e-04 / 1.803e-02 / 7.210e-02
  grouped SGD plain, step 5:  5.606e-07 / 5.606e-07 / 2.243e-06      (dampening: 3.866e-07 / 5.240e-07 / 2.096e-06)
  Adam, wd 0, step 5:         4.707e-07 / 4.707e-07 / 1.883e-06      (clipped, step 1: 1.197e-07 / 1.192e-07 / 4.766e-07)
  AdamW, wd > 0, step 5:      7.730e-07 / 7.730e-07 / 3.092e-06      (clipped: 5.595e-07 / 5.595e-07 / 2.238e-06)

Wherever the statement is "unchanged" (coefficient 1, one group without clipping) the check is bitwise.
"""
import functools

import pytest
import torch

import yunet_amd._lib as L
import yunet_amd.kernels as K
from optim_checks import check

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TILE, BLOCK, MAXB = L.NORM_TILE, L.NORM_BLOCK, L.NORM_MAX_BLOCKS


# ---- gradient norm ---------------------------------------------------------------------------------------------------

def torch_norm(g, max_norm, norm_type, grad_scale, dtype):
    """clip_grad_norm_'s arithmetic in `dtype`: (norm, clamp(max_norm / (norm + 1e-6), max=1))."""
    x = g.cpu().to(dtype) * torch.tensor(grad_scale, dtype=dtype)
    norm = torch.linalg.vector_norm(x, norm_type)
    return norm, torch.clamp(max_norm / (norm + 1e-6), max=1.0)


def grad_of(n, seed, offset=0):
    """n seeded values in device memory, `offset` floats past a 16-byte boundary."""
    gen = torch.Generator().manual_seed(seed)
    buf = torch.zeros(n + offset, device=DEV)
    buf[offset:].copy_(torch.randn(n, generator=gen))
    return buf[offset:]


SIZES = [1, 3, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5,
         (MAXB + 1) * TILE + 3]          # the last: more tiles than blocks, a block folds two


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'plus-one-float'])
@pytest.mark.parametrize('n', SIZES)
def test_norm_sizes(n, offset):
    g = grad_of(n, 100 + n, offset)
    assert g.data_ptr() % 16 == (4 * offset) % 16
    max_norm = 0.5
    out = K.grad_norm(g, max_norm, 2).cpu()
    n32, c32 = torch_norm(g, max_norm, 2, 1.0, torch.float32)
    n64, c64 = torch_norm(g, max_norm, 2, 1.0, torch.float64)
    check(f'norm n={n}', out[0], n32, n64)
    check(f'coef n={n}', out[1], c32, c64)
    # the same elements behind another alignment: the same bits
    other = grad_of(n, 100 + n, 1 - offset)
    assert torch.equal(other, g)
    assert torch.equal(K.grad_norm(other, max_norm, 2).cpu(), out)


@pytest.mark.parametrize('norm_type', [2, 1, float('inf')], ids=['l2', 'l1', 'inf'])
@pytest.mark.parametrize('grad_scale', [1.0, 1.0 / 512.0], ids=['unscaled', 'loss-scale-512'])
def test_norm_types_and_scale(norm_type, grad_scale):
    n = 3 * TILE + 5
    g = grad_of(n, 7) * (1.0 / grad_scale)
    max_norm = 2.0
    out = K.grad_norm(g, max_norm, norm_type, grad_scale).cpu()
    n32, c32 = torch_norm(g, max_norm, norm_type, grad_scale, torch.float32)
    n64, c64 = torch_norm(g, max_norm, norm_type, grad_scale, torch.float64)
    assert float(c64) < 1.0
    check(f'norm p={norm_type} scale={grad_scale}', out[0], n32, n64)
    check(f'coef p={norm_type} scale={grad_scale}', out[1], c32, c64)


def test_norm_rejects_other_types():
    g = grad_of(16, 1)
    for bad in (3, 0, 0.5, 'fro'):
        with pytest.raises(ValueError, match='norm_type'):
            K.grad_norm(g, 1.0, bad)


def test_norm_replay_without_reset_and_determinism():
    n = 3 * TILE + 5
    a, b = grad_of(n, 11), grad_of(n, 12) * 3.0
    scratch = K.grad_norm_scratch(DEV)
    out_a, out_b = torch.empty(2, device=DEV), torch.empty(2, device=DEV)
    K.grad_norm(a, 1.0, 2, scratch=scratch, out=out_a)      # two launches back to back, one scratch, nothing in between
    K.grad_norm(b, 1.0, 2, scratch=scratch, out=out_b)
    again = K.grad_norm(a, 1.0, 2, scratch=scratch).cpu()
    fresh_a, fresh_b = K.grad_norm(a, 1.0, 2).cpu(), K.grad_norm(b, 1.0, 2).cpu()
    assert torch.equal(out_a.cpu(), fresh_a) and torch.equal(out_b.cpu(), fresh_b) and torch.equal(again, fresh_a)
    assert not torch.equal(fresh_a, fresh_b)
    assert int(scratch.view(torch.int32)[0]) == 0            # the ticket counter is back at zero
    for g, out in ((a, fresh_a), (b, fresh_b)):
        n32, _ = torch_norm(g, 1.0, 2, 1.0, torch.float32)
        n64, _ = torch_norm(g, 1.0, 2, 1.0, torch.float64)
        check('replayed norm', out[0], n32, n64)


# ---- grouped updates -------------------------------------------------------------------------------------------------

SEG = [1, 16, 9 * 16 + 3, 255, 257] * 3                      # boundaries inside a float4 and inside a block
GROUP_OF_SEG = [i % 3 for i in range(len(SEG))]
N = sum(SEG)
STEPS = 5
ZERO_LANE = 5                                                # inside segment 1 (group 1): its gradient is 0 in every step


@functools.lru_cache(None)
def inputs():
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(N, generator=gen)
    grads = [torch.randn(N, generator=gen) for _ in range(STEPS)]
    for g in grads:
        g[ZERO_LANE] = 0.0
    gid = torch.cat([torch.full((n,), k, dtype=torch.uint8) for n, k in zip(SEG, GROUP_OF_SEG)])
    return p0, grads, gid


def torch_run(make_opt, group_hp, dtype, clip=None):
    """Five steps of a torch optimizer over one tensor per segment, grouped by hand; flat parameters after each step."""
    p0, grads, _ = inputs()
    segs = [s.clone().to(dtype).requires_grad_(True) for s in p0.split(SEG)]
    groups = [dict(hp, params=[s for s, k in zip(segs, GROUP_OF_SEG) if k == gi]) for gi, hp in enumerate(group_hp)]
    opt = make_opt(groups)
    out = []
    for g in grads:
        for s, gs in zip(segs, g.to(dtype).split(SEG)):
            s.grad = gs.clone()
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(segs, **clip)
        opt.step()
        out.append(torch.cat([s.detach() for s in segs]).clone())
    return out


def table_of(rows):
    return torch.tensor(rows, dtype=torch.float64, device=DEV)


SGD_HP = [dict(lr=0.1, weight_decay=5e-4, momentum=0.9), dict(lr=0.05, weight_decay=0.0, momentum=0.8),
          dict(lr=0.2, weight_decay=1e-3, momentum=0.9)]
SGD_VARIANTS = dict(plain=dict(), nesterov=dict(nesterov=True), dampening=dict(dampening=0.3), momentum0=dict(momentum=0.0))


@functools.lru_cache(None)
def sgd_reference(variant, clipped):
    extra = SGD_VARIANTS[variant]
    hp = [dict(h, **extra) for h in SGD_HP]
    clip = dict(max_norm=1.0, norm_type=2) if clipped else None
    return tuple(torch_run(lambda g: torch.optim.SGD(g, lr=0.1), hp, dt, clip) for dt in (torch.float32, torch.float64))


@pytest.mark.parametrize('clipped', [False, True], ids=['noclip', 'clip'])
@pytest.mark.parametrize('variant', list(SGD_VARIANTS))
def test_sgd_grouped(variant, clipped):
    extra = SGD_VARIANTS[variant]
    p0, grads, gid = inputs()
    t32, t64 = sgd_reference(variant, clipped)
    p, buf, gid = p0.to(DEV), torch.zeros(N, device=DEV), gid.to(DEV)
    table = table_of([[h['lr'], h['weight_decay'], extra.get('momentum', h['momentum']), 0.0] for h in SGD_HP])
    scratch, out = K.grad_norm_scratch(DEV), torch.empty(2, device=DEV)
    for k, g in enumerate(grads):
        g = g.to(DEV)
        coef = K.grad_norm(g, 1.0, 2, scratch=scratch, out=out)[1:2] if clipped else None
        K.sgd_step_grouped(p, g, buf, gid, table, clip_coef=coef, first=(k == 0),
                           dampening=extra.get('dampening', 0.0), nesterov=extra.get('nesterov', False))
        check(f'sgd {variant} clip={clipped} step {k + 1}', p, t32[k], t64[k])
    if variant == 'momentum0':
        assert not buf.any()                                  # momentum 0 leaves the buffer alone


ADAM_HP = [dict(lr=1e-2, betas=(0.9, 0.999)), dict(lr=5e-3, betas=(0.8, 0.99)), dict(lr=2e-2, betas=(0.9, 0.999))]
ADAM_WD = {'wd0': [0.0, 0.0, 0.0], 'wd': [1e-2, 0.0, 5e-2]}     # group 1 (the zero-gradient lane) never decays


@functools.lru_cache(None)
def adam_reference(kind, wd, clipped):
    hp = [dict(h, weight_decay=w) for h, w in zip(ADAM_HP, ADAM_WD[wd])]
    cls = torch.optim.AdamW if kind == 'AdamW' else torch.optim.Adam
    clip = dict(max_norm=1.0, norm_type=2) if clipped else None
    return tuple(torch_run(lambda g: cls(g, lr=1e-3), hp, dt, clip) for dt in (torch.float32, torch.float64))


@pytest.mark.parametrize('clipped', [False, True], ids=['noclip', 'clip'])
@pytest.mark.parametrize('wd', list(ADAM_WD))
@pytest.mark.parametrize('kind', ['Adam', 'AdamW'])
def test_adam_grouped(kind, wd, clipped):
    p0, grads, gid = inputs()
    t32, t64 = adam_reference(kind, wd, clipped)
    p, m, v, gid = p0.to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV), gid.to(DEV)
    table = table_of([[h['lr'], w, h['betas'][0], h['betas'][1]] for h, w in zip(ADAM_HP, ADAM_WD[wd])])
    scratch, out = K.grad_norm_scratch(DEV), torch.empty(2, device=DEV)
    for k, g in enumerate(grads):
        g = g.to(DEV)
        coef = K.grad_norm(g, 1.0, 2, scratch=scratch, out=out)[1:2] if clipped else None
        K.adam_step_grouped(p, g, m, v, gid, table, k + 1, decoupled=(kind == 'AdamW'), clip_coef=coef)
        check(f'{kind} {wd} clip={clipped} step {k + 1}', p, t32[k], t64[k])
    # the lane whose gradient is 0 in every step: 0 / (0 + eps) = 0, the parameter never moved
    assert float(p[ZERO_LANE]) == float(p0[ZERO_LANE]) and float(m[ZERO_LANE]) == 0.0 and float(v[ZERO_LANE]) == 0.0


# ---- "unchanged" is bitwise ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('variant', list(SGD_VARIANTS))
def test_one_group_without_clipping_is_sgd_step_ex(variant):
    extra = SGD_VARIANTS[variant]
    p0, grads, _ = inputs()
    mom = extra.get('momentum', 0.9)
    kw = dict(dampening=extra.get('dampening', 0.0), nesterov=extra.get('nesterov', False))
    pa, ba = p0.to(DEV), torch.zeros(N, device=DEV)
    pb, bb = p0.to(DEV), torch.zeros(N, device=DEV)
    lr_dev = torch.tensor([0.01], device=DEV)
    gid = torch.zeros(N, dtype=torch.uint8, device=DEV)
    table = table_of([[0.01, 5e-4, mom, 0.0]])
    for k, g in enumerate(grads):
        g = g.to(DEV)
        K.sgd_step(pa, g, ba, lr_dev, mom, 5e-4, 1.0 / 512.0, first=(k == 0), **kw)
        K.sgd_step_grouped(pb, g, bb, gid, table, grad_scale=1.0 / 512.0, first=(k == 0), **kw)
        assert torch.equal(pa, pb) and torch.equal(ba, bb), (variant, k)


def test_norm_below_max_norm_leaves_the_update_unchanged():
    p0, grads, gid = inputs()
    g = (grads[0] * 1e-3).to(DEV)                             # norm ~ 0.045 < max_norm
    out = K.grad_norm(g, 1.0, 2)
    assert float(out[1]) == 1.0 and 0.0 < float(out[0]) < 1.0
    table = table_of([[h['lr'], h['weight_decay'], h['momentum'], 0.0] for h in SGD_HP])
    res = []
    for coef in (None, out[1:2]):
        p, buf = p0.to(DEV), torch.zeros(N, device=DEV)
        K.sgd_step_grouped(p, g, buf, gid.to(DEV), table, clip_coef=coef, first=True)
        res.append((p, buf))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    res = []
    atable = table_of([[h['lr'], w, h['betas'][0], h['betas'][1]] for h, w in zip(ADAM_HP, ADAM_WD['wd'])])
    for coef in (None, out[1:2]):
        p, m, v = p0.to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        K.adam_step_grouped(p, g, m, v, gid.to(DEV), atable, 1, decoupled=True, clip_coef=coef)
        res.append(p)
    assert torch.equal(res[0], res[1])
