"""-m gpu: paramwise_cfg, grad_clip, AdamW and clipping under loss scaling through the runner, three iterations of
YuNet_n at the smallest geometry the runner tests use (8 images of 160 x 160).

After every step the flat parameters are compared with torch.optim.* on the CPU, fed the gradients the device step
consumed, with groups built by hand here and torch.nn.utils.clip_grad_norm_.  Bound as in test_optim_kernels_gpu.py:
the device may deviate from the fp64 torch run by at most 4 x what the fp32 torch run deviates (floor: one fp32 ulp of the
largest parameter); both figures are printed before the assertion.
"""
import pytest
import torch

import yunet_oracle as O
import yunet_amd.runner as R
from optim_checks import check

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ITERS = 3
BASE_LR, BASE_WD = 0.01, 5e-4


class Recorder(R.Hook):
    """Runs after the optimizer hook: the gradient this step consumed and the parameters it left."""

    def __init__(self):
        self.grads, self.params = [], []

    def after_train_iter(self, runner):
        eng = runner.model.engine
        self.grads.append(eng.params.grad.detach().cpu().clone())
        self.params.append(eng.params.data.detach().cpu().clone())


def _model():
    import yunet_amd
    cfg = yunet_amd.Config.fromfile('configs/yunet_n.py')
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(O.init_state(O.yunet_arch('n'), seed=5), strict=True)
    return m.to(DEV).train()


def run_case(optimizer, optimizer_config, fp16=None):
    from yunet_amd.optim import build_optimizer
    m = _model()
    start = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    opt = build_optimizer(m, optimizer)
    lines = []
    r = R.EpochBasedRunner(m, opt, None, lines.append, max_epochs=1)
    oc = R.Fp16OptimizerHook(**optimizer_config, **fp16) if fp16 else optimizer_config
    r.register_training_hooks(dict(policy='fixed'), oc, None, dict(interval=1, hooks=[dict(type='TextLoggerHook')]))
    rec = Recorder()
    r.register_hook(rec, 'NORMAL')
    r.run([R.SyntheticWiderFace((160, 160), 8, iters_per_epoch=ITERS)], device=DEV)
    torch.cuda.synchronize()
    base = m.engine.params.data.data_ptr()
    where = {n: ((p.data_ptr() - base) // 4, p.numel()) for n, p in m.named_parameters()}
    return m, opt, r, rec, start, where, lines


def hand_groups(m, rule):
    """{(lr, wd): [names]} from a rule written out here: rule(name, module) -> (lr, wd)."""
    groups = {}
    for name, _ in m.named_parameters():
        mod = m.get_submodule(name.rsplit('.', 1)[0])
        groups.setdefault(rule(name, mod), []).append(name)
    return groups


def torch_reference(make_opt, groups, start, where, grads, dtype, clip=None, grad_scale=1.0):
    """The same steps in torch on the CPU: per-parameter tensors, hand-built groups, the recorded gradients."""
    ps = {n: t.clone().to(dtype).requires_grad_(True) for n, t in start.items()}
    opt = make_opt([dict(params=[ps[n] for n in names], lr=lr, weight_decay=wd) for (lr, wd), names in groups.items()])
    out, norms = [], []
    for g in grads:
        for n, p in ps.items():
            off, cnt = where[n]
            p.grad = (g[off:off + cnt].to(dtype) * grad_scale).view(p.shape).clone()
        if clip is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(list(ps.values()), **clip).clone())
        opt.step()
        out.append({n: p.detach().clone() for n, p in ps.items()})
    return out, norms


def compare(what, rec, where, make_opt, groups, start, clip=None, grad_scale=1.0):
    r32, n32 = torch_reference(make_opt, groups, start, where, rec.grads, torch.float32, clip, grad_scale)
    r64, n64 = torch_reference(make_opt, groups, start, where, rec.grads, torch.float64, clip, grad_scale)
    assert len(rec.params) == ITERS
    names = list(where)
    for k in range(ITERS):
        dev = torch.cat([rec.params[k][where[n][0]:where[n][0] + where[n][1]] for n in names])
        t32 = torch.cat([r32[k][n].reshape(-1) for n in names])
        t64 = torch.cat([r64[k][n].reshape(-1) for n in names])
        check(f'{what} step {k + 1}', dev, t32, t64)
    return n32, n64


def sgd(groups):
    return torch.optim.SGD(groups, lr=BASE_LR, momentum=0.9)


def is_dw(mod):
    return isinstance(mod, torch.nn.Conv2d) and mod.groups == mod.in_channels


def test_paramwise_cfg():
    pw = dict(norm_decay_mult=0., bias_decay_mult=0., dwconv_decay_mult=0.5)
    m, opt, r, rec, start, where, _ = run_case(
        dict(type='SGD', lr=BASE_LR, momentum=0.9, weight_decay=BASE_WD, paramwise_cfg=pw), dict(grad_clip=None))
    assert len(opt.param_groups) == 3

    def rule(name, mod):
        if isinstance(mod, torch.nn.BatchNorm2d):
            return BASE_LR, 0.0
        if is_dw(mod):
            return BASE_LR, BASE_WD * 0.5
        return BASE_LR, (0.0 if name.endswith('.bias') else BASE_WD)
    compare('paramwise', rec, where, sgd, hand_groups(m, rule), start)
    # the three groups partition the parameters
    assert sum(len(g['params']) for g in opt.param_groups) == len(list(m.parameters()))


def _first_norm():
    """The gradient norm of the first step (one forward / backward, no update)."""
    from yunet_amd.optim import FusedSGD
    import yunet_amd.synthetic as S
    m = _model()
    src = R.SyntheticWiderFace((160, 160), 8, iters_per_epoch=ITERS)
    out = m.train_step(src.batch(0, DEV), FusedSGD(m, lr=0.0))
    out['loss'].backward()
    torch.cuda.synchronize()
    return float(m.engine.params.grad.double().norm())


@pytest.fixture(scope='module')
def max_norm():
    return 0.5 * _first_norm()                           # below the first step's norm: clipping is active


def test_grad_clip(max_norm):
    clip = dict(max_norm=max_norm, norm_type=2)
    m, opt, r, rec, start, where, lines = run_case(
        dict(type='SGD', lr=BASE_LR, momentum=0.9, weight_decay=BASE_WD), dict(grad_clip=clip))
    groups = hand_groups(m, lambda name, mod: (BASE_LR, BASE_WD))
    n32, n64 = compare('grad_clip', rec, where, sgd, groups, start, clip=clip)
    assert float(n64[0]) > max_norm                       # the first step was clipped
    logged = [rec_['grad_norm'] for rec_ in r.log_buffer]
    assert len(logged) == ITERS and all('grad_norm' in ln for ln in lines if ln.startswith('Epoch'))
    for k in range(ITERS):
        check(f'logged grad_norm step {k + 1}', logged[k], n32[k], n64[k])


def test_adamw():
    m, opt, r, rec, start, where, _ = run_case(dict(type='AdamW', lr=1e-3, weight_decay=0.05), dict(grad_clip=None))
    groups = hand_groups(m, lambda name, mod: (1e-3, 0.05))
    compare('AdamW', rec, where, lambda g: torch.optim.AdamW(g, lr=1e-3), groups, start)
    assert opt._steps == ITERS and opt.state_dict()['exp_avg_sq'].abs().sum() > 0


def test_grad_clip_under_loss_scaling(max_norm):
    clip = dict(max_norm=max_norm, norm_type=2)
    m, opt, r, rec, start, where, _ = run_case(
        dict(type='SGD', lr=BASE_LR, momentum=0.9, weight_decay=BASE_WD), dict(grad_clip=clip), fp16=dict(loss_scale=512.))
    assert opt.grad_scale == 1.0 / 512.0                  # the scale is removed inside the kernels, not by a mul_ pass
    groups = hand_groups(m, lambda name, mod: (BASE_LR, BASE_WD))
    n32, n64 = compare('fp16 grad_clip', rec, where, sgd, groups, start, clip=clip, grad_scale=1.0 / 512.0)
    assert float(n64[0]) > max_norm
    for k in range(ITERS):                                # the norm is that of the UNSCALED gradient
        check(f'fp16 logged grad_norm step {k + 1}', r.log_buffer[k]['grad_norm'], n32[k], n64[k])
