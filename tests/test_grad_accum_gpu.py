"""-m gpu: gradient accumulation in the fused engine: the yunet_grad_accum kernel bit for bit, the
accumulated gradient against the oracle, its composition under both deterministic modes, micro-batches of different
geometry, the fresh-backward rule, frozen parameters, and the two cumulative optimizer hooks through the runner.

Shapes are the smallest the engine takes with more than one pyramid cell per level (64 x 64, and 64 x 96 so that a wrong
per-layer count shows), N = 2.  Yardstick and bars of the oracle comparison: tests/test_finetune_gpu.py
(finetune_ref.step_fp32 / grads_fp64, every BatchNorm flag true).  The batch seeds were picked on the CPU so that
finetune_ref.near_tie is empty for each (asserted again here).
"""
import os

import numpy as np
import pytest
import torch

import finetune_ref as FR
import yunet_amd.runner as R
import yunet_oracle as O
from test_finetune_gpu import buffers, bytes_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_TRAIN = lambda name: True          # noqa: E731  (finetune_ref's flag per BatchNorm layer)


def model(kind, deterministic=False, accumulate=None, **backbone):
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    cfg.model.backbone.update(backbone)
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(FR.warm_state(kind, 1), strict=True)
    m.to(DEV).train()
    m.set_deterministic(deterministic)
    if accumulate is not None:
        m.set_grad_accumulation(accumulate)
    m._ensure_engine(torch.device(DEV, torch.cuda.current_device()))
    return m


def batch(h, w, seed, n=2):
    import yunet_amd.synthetic as S
    return S.make_batch(n, h, w, seed)


def micro_step(m, b, factor):
    """forward_train + (total / factor).backward(); returns the four losses as floats"""
    import yunet_amd.synthetic as S
    losses = m.forward_train(**S.to_device(b, DEV))
    (sum(losses.values()) / factor).backward()
    return {k: float(v) for k, v in losses.items()}


def flat_grad(m):
    torch.cuda.synchronize()
    return m.engine.params.grad.detach().clone()


def launches(m):
    return dict(m.engine.accum_launches)


# =================================================================================================== 1. the kernel
def special_values(n, seed):
    """n fp32 values: normal noise with NaN, +-Inf, +-0 and denormals spread over it (the two operands get different
    seeds, so most specials meet an ordinary number; the pairs that matter are placed by the caller)"""
    rng = np.random.RandomState(seed)
    v = rng.standard_normal(n).astype(np.float32)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -3e-42, 2.0 ** -126, -2.0 ** -149], dtype=np.float32)
    if n:
        idx = rng.permutation(n)[:min(n, 4 * len(specials))]
        v[idx] = specials[np.arange(len(idx)) % len(specials)]
    return v


PAD = 4          # floats in front of the data: element PAD of a fresh allocation is 16-byte aligned


def padded(values, off, fill):
    """device buffer [PAD + off | values | 1]: (buffer, view of the data); the data starts `off` floats past a 16-byte
    boundary, one float of padding on each side of it holds `fill`"""
    n = len(values)
    buf = torch.full((PAD + off + n + 1,), fill, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + off:PAD + off + n]
    view.copy_(torch.from_numpy(values))
    return buf, view


def host_bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('off_acc,off_grad', [(0, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize('n', [0, 1, 3, 4, 1027, 75856])
def test_kernel_bit_for_bit(n, off_acc, off_grad):
    import yunet_amd.kernels as K
    a, b = special_values(n, 3), special_values(n, 4)
    if n >= 1027:          # the pairs the contract names, inside the vector body and in head / tail elements
        for i in (0, 1, 2, 513, n - 3, n - 2, n - 1):
            a[i] = b[i] = -0.0                                  # -0 + -0 = -0
        a[7], b[7] = 0.0, -0.0                                  # +0 + -0 = +0
        a[9], b[9] = np.float32(1e-40), np.float32(2e-40)       # denormals are not flushed
        a[11], b[11] = np.float32(3.0), np.float32(np.nan)
    # Inf meets no Inf of the other sign: IEEE 754 leaves sign and payload of the NaN that produces to the implementation
    b[np.isinf(a) & np.isinf(b)] = 1.0
    acc_buf, acc = padded(np.zeros(n, np.float32), off_acc, 7.0)
    g_buf, g = padded(a, off_grad, 9.0)
    K.grad_accum(acc, g, 'save')
    torch.cuda.synchronize()
    assert np.array_equal(host_bits(acc), a.view(np.uint32)) and np.array_equal(host_bits(g), a.view(np.uint32))
    g.copy_(torch.from_numpy(b))
    K.grad_accum(acc, g, 'add')
    torch.cuda.synchronize()
    with np.errstate(all='ignore'):
        want = (a + b).astype(np.float32)
    got = host_bits(g)
    same = got == want.view(np.uint32)
    assert same.all(), (n, np.flatnonzero(~same)[:8], got[~same][:8], want.view(np.uint32)[~same][:8])
    assert np.array_equal(host_bits(acc), a.view(np.uint32))            # ADD leaves the saved total alone
    for buf, off, fill in ((acc_buf, off_acc, 7.0), (g_buf, off_grad, 9.0)):
        rest = torch.cat([buf[:PAD + off], buf[PAD + off + n:]]).cpu()
        assert rest.numel() == PAD + off + 1 and bool((rest == fill).all()), 'padding was written'


def test_kernel_inf_minus_inf_is_nan():
    import yunet_amd.kernels as K
    acc = torch.tensor([np.inf, -np.inf, np.inf, 1.0] * 2, device=DEV)
    g = torch.tensor([-np.inf, np.inf, np.inf, np.nan] * 2, device=DEV)
    saved = torch.empty_like(acc)
    K.grad_accum(saved, acc, 'save')
    K.grad_accum(saved, g, 'add')
    out = g.cpu()
    assert bool(torch.isnan(out[[0, 1, 3]]).all()) and float(out[2]) == np.inf


# ================================================================================= 2. gradients against the oracle
@pytest.mark.parametrize('kind,h,w,seeds', [('n', 64, 64, (43, 47, 48)), ('s', 64, 96, (50, 51, 52))])
def test_accumulated_gradient_vs_oracle(kind, h, w, seeds):
    """k = 3 micro-batches, each (loss / 3).backward() with no zero_grad in between: the total is the sum of the oracle's
    per-micro-batch gradients / 3.  Measured on an MI355X, worst gradient error / bound: 0.003 (YuNet_n), 0.002 (YuNet_s)."""
    k = len(seeds)
    m = model(kind, accumulate=True)
    arch = O.yunet_arch(kind)
    sd = {key: v.clone() for key, v in FR.warm_state(kind, 1).items()}
    start = {key: v.clone() for key, v in sd.items()}
    g32 = g64 = None
    for i, seed in enumerate(seeds):
        b = batch(h, w, seed)
        lv, gi32, aux, after = FR.step_fp32(b, sd, arch, ALL_TRAIN)
        assert FR.near_tie(aux, b) == [], 'pick another seed: the oracle assignment sits on a tie'
        got = micro_step(m, b, k)
        torch.cuda.synchronize()
        plan = m.engine.plan
        assert torch.equal(plan.gt_inds.cpu(), aux['gt_inds'].int()), f'assignment of micro-batch {i}'
        for name in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps'):
            print(f'[{kind} micro {i}] {name} {got[name]:.7g} oracle {lv[name]:.7g}')
            assert abs(got[name] - lv[name]) <= 1e-4 * abs(lv[name]) + 1e-6, (i, name, got[name], lv[name])
        gi64 = FR.grads_fp64(b, sd, arch, ALL_TRAIN, plan.dflat.cpu())
        g32 = {key: v / k for key, v in gi32.items()} if g32 is None else {key: g32[key] + v / k for key, v in gi32.items()}
        g64 = {key: v / k for key, v in gi64.items()} if g64 is None else {key: g64[key] + v / k for key, v in gi64.items()}
        sd = {key: v.clone() for key, v in after.items()}              # the oracle's steps chained: BatchNorm buffers move on
    assert launches(m) == dict(save=k - 1, add=k - 1)
    scale = max(float(v.abs().max()) for v in g64.values())
    named = dict(m.named_parameters())
    worst = (0.0, None)
    for key in g32:
        err_hip = float((named[key].grad.cpu().double() - g64[key]).abs().max())
        err_ref = float((g32[key].double() - g64[key]).abs().max())
        tol = 10 * max(err_ref, 1e-5 * scale) + 1e-2 * float(g64[key].abs().max())
        worst = max(worst, (err_hip / tol, key))
        assert err_hip <= tol, (key, err_hip, err_ref, float(g64[key].abs().max()), scale)
    print(f'[{kind}] worst accumulated-gradient error / bound {worst[0]:.3f} ({worst[1]})')
    now = m.state_dict()
    for key, v in sd.items():
        if key.endswith('num_batches_tracked'):
            assert int(now[key]) == int(v) == int(start[key]) + k, key
        elif key.endswith(('running_mean', 'running_var')):
            assert torch.allclose(now[key].cpu(), v, rtol=1e-3, atol=1e-4), key


# ======================================================================= 3. bit-exact composition, deterministic modes
def three_steps(level, accumulate, seeds=(43, 47, 48)):
    m = model('n', deterministic=level, accumulate=accumulate)
    grads = []
    for seed in seeds:
        micro_step(m, batch(64, 64, seed), len(seeds))
        grads.append(flat_grad(m))
    return m, grads


@pytest.mark.parametrize('level', ['fast', True])
def test_accumulation_composes_bit_exactly_in_deterministic_modes(level):
    _, (g1, g2, g3) = three_steps(level, False)
    want = bytes_of((g1 + g2) + g3)
    assert not torch.equal(bytes_of(g3), want)
    m, on = three_steps(level, True)
    assert torch.equal(bytes_of(on[0]), bytes_of(g1)) and torch.equal(bytes_of(on[1]), bytes_of(g1 + g2))
    assert torch.equal(bytes_of(on[2]), want) and launches(m) == dict(save=2, add=2)
    _, again = three_steps(level, True)
    assert torch.equal(bytes_of(again[2]), want)


# ================================================================================================ 4. mixed geometry
MIXED = ((64, 64, 43), (64, 96, 61))


def two_geometries(level, accumulate):
    m = model('n', deterministic=level, accumulate=accumulate)
    grads = []
    for h, w, seed in MIXED:
        micro_step(m, batch(h, w, seed), 2)
        grads.append(flat_grad(m))
    assert len(m.engine.plans) == 2
    return m, grads


@pytest.mark.parametrize('level', [False, 'fast'])
def test_micro_batches_of_different_geometry(level):
    arch, sd = O.yunet_arch('n'), FR.warm_state('n', 1)
    for h, w, seed in MIXED:
        b = batch(h, w, seed)
        assert FR.near_tie(FR.step_fp32(b, sd, arch, ALL_TRAIN)[2], b) == [], 'pick another seed'
    _, (g1, g2) = two_geometries(level, False)
    m, (t1, t2) = two_geometries(level, True)
    assert launches(m) == dict(save=1, add=1)
    want = g1 + g2
    if level == 'fast':
        assert torch.equal(bytes_of(t1), bytes_of(g1)) and torch.equal(bytes_of(t2), bytes_of(want))
    else:
        # the allowance tests/test_bench_gpu.py makes for the float atomics of the default mode
        scale = float(want.abs().max())
        err = float((t2.double() - want.double()).abs().max())
        print(f'[mixed geometry] |total - (g1 + g2)| {err:.3e}, gradient scale {scale:.3e}')
        assert err <= 1e-5 * scale + 1e-9


# ============================================================================ 5. fresh-backward rule, the off switch
def test_zero_grad_before_every_backward_costs_nothing():
    from yunet_amd.optim import FusedSGD
    _, off = three_steps('fast', False)
    m = model('n', deterministic='fast', accumulate=True)
    opt = FusedSGD(m, lr=0.0)
    for seed, want in zip((43, 47, 48), off):
        opt.zero_grad()
        micro_step(m, batch(64, 64, seed), 3)
        assert torch.equal(bytes_of(flat_grad(m)), bytes_of(want))
    assert launches(m) == dict(save=0, add=0) and m.engine._acc is None


def test_switch_off_allocates_and_launches_nothing():
    m, grads = three_steps('fast', False)
    assert m.engine.grad_accumulation is False and m.engine._acc is None and launches(m) == dict(save=0, add=0)
    assert not torch.equal(grads[1], grads[0] + grads[1])           # .grad was overwritten, as it always was
    # ... and the default engine of a model nobody told anything is the same
    m2 = model('n')
    micro_step(m2, batch(64, 64, 43), 1)
    micro_step(m2, batch(64, 64, 47), 1)
    assert m2.engine._acc is None and launches(m2) == dict(save=0, add=0)


def test_in_place_zero_and_set_to_none_give_the_second_gradient_alone():
    _, off = three_steps('fast', False, seeds=(43, 47))
    # p.grad.zero_() on every parameter: the total is read from the gradient itself, 0 + g = g (a -0 becomes +0: values)
    m = model('n', deterministic='fast', accumulate=True)
    micro_step(m, batch(64, 64, 43), 2)
    for p in m.parameters():
        p.grad.zero_()
    micro_step(m, batch(64, 64, 47), 2)
    assert torch.equal(flat_grad(m), off[1]) and launches(m) == dict(save=1, add=1)
    # zero_grad(set_to_none=True) of a torch optimizer: .grad is None, nothing to add to, nothing launched
    m = model('n', deterministic='fast', accumulate=True)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    micro_step(m, batch(64, 64, 43), 2)
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in m.parameters())
    micro_step(m, batch(64, 64, 47), 2)
    assert torch.equal(bytes_of(flat_grad(m)), bytes_of(off[1])) and launches(m) == dict(save=0, add=0)
    fp = m.engine.params
    assert all(p.grad is not None and p.grad.data_ptr() == fp.view(n, of=fp.grad).data_ptr() for n, p in m.named_parameters())
    # ... and without either, the two add up
    micro_step(m, batch(64, 64, 43), 2)
    assert torch.equal(bytes_of(flat_grad(m)), bytes_of(off[1] + off[0])) and launches(m) == dict(save=1, add=1)


# =============================================================================================== 6. frozen parameters
def test_frozen_stages_stay_zero_under_accumulation():
    m = model('s', accumulate=True, frozen_stages=2)
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    frozen_bn = [n for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) and not mod.training]
    assert frozen and frozen_bn
    before = buffers(m)
    micro_step(m, batch(64, 64, 70), 2)
    g1 = flat_grad(m)
    micro_step(m, batch(64, 64, 72), 2)
    total = flat_grad(m)
    assert launches(m) == dict(save=1, add=1)
    fp = m.engine.params
    named = dict(m.named_parameters())
    for n in frozen:
        assert named[n].grad is None, n
        assert not bool(fp.view(n, of=total).any()), f'{n}: frozen range of the flat gradient is not zero'
    trainable = [n for n in named if n not in frozen]
    assert all(named[n].grad is not None for n in trainable)
    assert any(bool((fp.view(n, of=total) != fp.view(n, of=g1)).any()) for n in trainable)
    now = m.state_dict()
    for key, was in before.items():
        if key.rsplit('.', 1)[0] in frozen_bn:
            assert torch.equal(bytes_of(now[key]), was), f'{key}: a frozen BatchNorm layer changed'


# ============================================================================================ 7. runner end to end
ITERS, K_ITERS = 5, 2
SGD = dict(lr=0.01, momentum=0.9, weight_decay=5e-4)


class Recorder(R.Hook):
    """the flat parameters the run starts from, and after the optimizer hook those every iteration leaves"""

    def __init__(self):
        self.start, self.params = None, []

    def before_run(self, runner):
        self.start = bytes_of(runner.model.engine.params.data)

    def after_train_iter(self, runner):
        self.params.append(bytes_of(runner.model.engine.params.data))


def source(iters=ITERS):
    return R.SyntheticWiderFace((64, 64), 2, iters_per_epoch=iters)


def run_hook(optimizer_config, m, extra_hooks=(), log=True, iters=ITERS):
    from yunet_amd.optim import FusedSGD
    opt = FusedSGD(m, **SGD)
    lines = []
    r = R.EpochBasedRunner(m, opt, None, lines.append, max_epochs=1)
    r.register_training_hooks(dict(policy='fixed'), optimizer_config, None,
                              dict(interval=1, hooks=[dict(type='TextLoggerHook')]) if log else None)
    rec = Recorder()
    r.register_hook(rec, 'LOW')
    for h in extra_hooks:
        r.register_hook(h, 'NORMAL')
    r.run([source(iters)], device=DEV)
    torch.cuda.synchronize()
    return r, opt, rec


def hand_loop():
    """The same five iterations out of what the engine did before: overwriting backwards, the window's sum formed in
    torch and copied into params.grad, the optimizer's step.  -> (model, optimizer, the windows' totals)"""
    from yunet_amd.optim import FusedSGD
    m = model('n', deterministic='fast')
    opt = FusedSGD(m, **SGD)
    src = source()
    totals, total = [], None
    for it in range(ITERS):
        factor = K_ITERS if it < ITERS // K_ITERS * K_ITERS else ITERS % K_ITERS
        out = m.train_step(src.batch(it, DEV), opt)
        (out['loss'] / factor).backward()
        g = m.engine.params.grad.detach().clone()
        total = g if total is None else total + g
        if (it + 1) % K_ITERS == 0 or it + 1 == ITERS:
            m.engine.params.grad.copy_(total)
            opt.step()
            totals.append(total)
            total = None
    torch.cuda.synchronize()
    assert m.engine._acc is None
    return m, opt, totals


@pytest.fixture(scope='module')
def by_hand():
    return hand_loop()


def test_runner_with_the_cumulative_hook_equals_the_hand_loop(by_hand):
    ref_m, ref_opt, _ = by_hand
    m = model('n', deterministic='fast')
    r, opt, rec = run_hook(dict(type='GradientCumulativeOptimizerHook', cumulative_iters=K_ITERS), m)
    assert m.engine.grad_accumulation is True and opt._steps == ref_opt._steps == 3
    assert launches(m) == dict(save=2, add=2)                 # iterations 1 and 3; 0, 2 and 4 follow a zero_grad
    assert torch.equal(rec.params[0], rec.start)
    assert torch.equal(rec.params[2], rec.params[1]) and not torch.equal(rec.params[1], rec.params[0])
    assert torch.equal(bytes_of(m.engine.params.data), bytes_of(ref_m.engine.params.data))
    assert torch.equal(bytes_of(opt._buf), bytes_of(ref_opt._buf))
    got, want = buffers(m), buffers(ref_m)
    assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in want)
    assert all('grad_norm' not in rec_ for rec_ in r.log_buffer) and len(r.log_buffer) == ITERS


def test_runner_with_the_cumulative_hook_and_grad_clip(by_hand):
    ref_m, _, totals = by_hand
    norms = [float(t.double().norm()) for t in totals]
    max_norm = 0.5 * min(norms)
    m = model('n', deterministic='fast')
    r, opt, rec = run_hook(dict(type='GradientCumulativeOptimizerHook', cumulative_iters=K_ITERS,
                                grad_clip=dict(max_norm=max_norm, norm_type=2)), m)
    assert opt._steps == 3
    coef = float(opt._norm_out[1])
    print(f'[clip] max_norm {max_norm:.4g}, window norms {norms}, last coefficient {coef:.4f}')
    assert coef < 1.0
    logged = {rec_['iter']: rec_.get('grad_norm') for rec_ in r.log_buffer}
    assert sorted(logged) == [1, 2, 3, 4, 5]
    assert [it for it, v in logged.items() if v is not None] == [2, 4, 5]       # the iterations that update
    assert logged[2] == pytest.approx(norms[0], rel=1e-5) and logged[2] > max_norm      # the first window is the hand loop's
    assert not torch.equal(bytes_of(m.engine.params.data), bytes_of(ref_m.engine.params.data))


def test_train_detector_builds_the_hook_under_cfg_deterministic():
    """cfg.deterministic with the plain cumulative hook is allowed: train_detector runs it"""
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    cfg.merge_from_dict({'deterministic': 'fast', 'optimizer_config': dict(type='GradientCumulativeOptimizerHook',
                                                                           cumulative_iters=2)})
    cfg['log_config'] = None
    cfg['checkpoint_config'] = None
    cfg['custom_hooks'] = None
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(FR.warm_state('n', 1), strict=True)
    R.train_detector(m, R.SyntheticWiderFace((64, 64), 2, iters_per_epoch=4), cfg, max_iters=4, device=DEV,
                     log=lambda *a: None)
    torch.cuda.synchronize()
    assert m.engine.grad_accumulation and m.engine.deterministic == 'fast' and launches(m) == dict(save=2, add=2)


# ================================================================================================== 8. the fp16 hook
def run_fp16(loss_scale, iters, extra_hooks=()):
    m = model('n')
    hook = R.GradientCumulativeFp16OptimizerHook(cumulative_iters=2, loss_scale=loss_scale)
    r, opt, rec = run_hook(hook, m, extra_hooks, log=False, iters=iters)
    assert m.engine.precision == 'bf16' and m.engine.plan.act_dtype == torch.bfloat16
    return m, hook, opt, rec


def test_fp16_hook_static_scale_is_removed_exactly():
    """bf16 storage, k = 2, one window: loss scale 512 -- a power of two, applied in the head's dy_scale and removed inside
    the update kernel -- gives the update of scale 1, to the bar tests/test_bf16_gpu.py uses for kernels fed identical
    inputs (1e-6 of the tensor's largest element: fp32 rounding and the order of the default mode's float atomics)."""
    m1, _, o1, rec1 = run_fp16(1.0, 2)
    m512, h512, o512, _ = run_fp16(512.0, 2)
    assert o1._steps == o512._steps == 1 and o512.grad_scale == 1.0 / 512.0 and h512.scale == 512.0
    assert launches(m512) == dict(save=1, add=1)
    for what, a, b in (('parameters', m1.engine.params.data, m512.engine.params.data), ('momentum', o1._buf, o512._buf)):
        err, top = float((a.double() - b.double()).abs().max()), float(a.abs().max())
        print(f'[fp16 scale 512 vs 1] {what}: max difference {err:.3e}, largest element {top:.3e}')
        assert err <= 1e-6 * (top + 1e-30), what
    assert not torch.equal(bytes_of(m1.engine.params.data), rec1.start)


class InjectInf(R.Hook):
    """an Inf in the flat gradient in front of iteration `at` (between the window's two backwards)"""

    def __init__(self, at):
        self.at = at

    def before_train_iter(self, runner):
        if runner.iter == self.at:
            runner.model.engine.params.grad[5] = float('inf')


def test_fp16_hook_skips_a_window_with_a_non_finite_total():
    m, hook, opt, rec = run_fp16('dynamic', 4, extra_hooks=[InjectInf(1)])
    start = rec.start
    # window 1 (iterations 0, 1): Inf + g = Inf at the boundary -> no update, the dynamic scale halves
    assert torch.equal(rec.params[0], start) and torch.equal(rec.params[1], start)
    assert hook.scale == 2.0 ** 15 and opt._steps == 1
    # window 2 starts fresh (iteration 2 launches nothing: the skipped boundary zeroed as well) and updates
    assert launches(m) == dict(save=2, add=2)
    assert torch.equal(rec.params[2], start) and not torch.equal(rec.params[3], start)
    assert bool(torch.isfinite(m.engine.params.data).all()) and bool(torch.isfinite(m.engine.params.grad).all())
    assert opt.grad_scale == 1.0 / 2.0 ** 15
