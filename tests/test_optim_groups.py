"""build_optimizer without a GPU: parameter groups by the rules of mmcv 1.x DefaultOptimizerConstructor, the errors,
per-group learning rates under a schedule that is no multiple of the base schedule, and the state-dict round trip."""
import math

import pytest
import torch

import yunet_amd
import yunet_amd.runner as R
from yunet_amd.optim import FusedAdam, FusedSGD, build_optimizer, paramwise_options

LR, WD = 0.01, 5e-4
# one of each kind, by name: a BN weight, a depthwise bias, a pointwise bias, a head (pointwise) conv weight
BN_W = 'backbone.model1.conv1.bn.weight'
DW_B = 'backbone.model1.conv1.conv2.bias'
PW_B = 'backbone.model1.conv1.conv1.bias'
HEAD_W = 'bbox_head.multi_level_cls.0.conv1.weight'
STEM_B = 'backbone.model0.conv1.bias'


@pytest.fixture(scope='module', params=['n', 's'])
def model(request):
    cfg = yunet_amd.Config.fromfile(f'configs/yunet_{request.param}.py')
    return yunet_amd.build_detector(cfg.model)


def table(model, paramwise, wd=WD):
    return {n: (lr, w) for n, _, lr, w in paramwise_options(model, LR, wd, paramwise)}


def sgd(model, **paramwise):
    return build_optimizer(model, dict(type='SGD', lr=LR, momentum=0.9, weight_decay=WD, paramwise_cfg=paramwise))


def test_every_parameter_is_named_once_in_model_order(model):
    got = paramwise_options(model, LR, WD, dict(norm_decay_mult=0.))
    assert [n for n, *_ in got] == [n for n, _ in model.named_parameters()]
    assert all(a is b for (_, a, _, _), b in zip(got, model.parameters()))


@pytest.mark.parametrize('paramwise, want', [
    (dict(norm_decay_mult=0.), {BN_W: (LR, 0.0), DW_B: (LR, WD), PW_B: (LR, WD), HEAD_W: (LR, WD)}),
    (dict(bias_decay_mult=0.), {BN_W: (LR, WD), DW_B: (LR, WD), PW_B: (LR, 0.0), STEM_B: (LR, 0.0), HEAD_W: (LR, WD)}),
    # the chain: norm, else depthwise (weight AND bias), else bias
    (dict(bias_decay_mult=0., dwconv_decay_mult=0.5),
     {BN_W: (LR, WD), DW_B: (LR, WD * 0.5), PW_B: (LR, 0.0), HEAD_W: (LR, WD),
      'backbone.model1.conv1.conv2.weight': (LR, WD * 0.5), 'bbox_head.multi_level_kps.2.conv2.weight': (LR, WD * 0.5)}),
    (dict(norm_decay_mult=0., bias_decay_mult=0., dwconv_decay_mult=0.5),
     {BN_W: (LR, 0.0), 'backbone.model0.bn1.bias': (LR, 0.0), DW_B: (LR, WD * 0.5), PW_B: (LR, 0.0), HEAD_W: (LR, WD)}),
    # bias_lr_mult: biases outside norm layers, depthwise ones included
    (dict(bias_lr_mult=2.), {BN_W: (LR, WD), 'backbone.model1.conv1.bn.bias': (LR, WD), DW_B: (LR * 2, WD),
                             PW_B: (LR * 2, WD), HEAD_W: (LR, WD)}),
    # custom_keys: the longer key wins over a shorter one that matches too, and a matched parameter skips the other rules
    (dict(custom_keys={'backbone': dict(lr_mult=0.1), 'backbone.model1': dict(lr_mult=0., decay_mult=2.)},
          norm_decay_mult=0., bias_decay_mult=0.),
     {BN_W: (0.0, WD * 2), DW_B: (0.0, WD * 2), PW_B: (0.0, WD * 2), STEM_B: (LR * 0.1, WD),
      'backbone.model0.bn1.weight': (LR * 0.1, WD), HEAD_W: (LR, WD), 'bbox_head.multi_level_cls.0.conv1.bias': (LR, 0.0)}),
    (dict(bypass_duplicate=True), {BN_W: (LR, WD), DW_B: (LR, WD)}),
])
def test_rules(model, paramwise, want):
    got = table(model, paramwise)
    for name, pair in want.items():
        assert got[name] == pytest.approx(pair, rel=1e-12), name


def test_key_order_is_longest_first_then_alphabetical(model):
    # two keys of one length that both match: the alphabetically first one wins (sorted(sorted(keys), key=len, reverse=True))
    got = table(model, dict(custom_keys={'conv2': dict(lr_mult=3.), 'conv1': dict(lr_mult=5.)}))
    assert got[DW_B][0] == pytest.approx(LR * 5) and got['backbone.model0.conv2.bn.weight'][0] == pytest.approx(LR * 3)


def test_groups_are_the_distinct_pairs(model):
    opt = sgd(model, norm_decay_mult=0., bias_decay_mult=0., dwconv_decay_mult=0.5)
    assert isinstance(opt, FusedSGD)
    assert [(g['lr'], g['weight_decay']) for g in opt.param_groups] == [(LR, WD), (LR, 0.0), (LR, WD * 0.5)]
    n_params = len(list(model.parameters()))
    assert sum(len(g['params']) for g in opt.param_groups) == n_params
    for g in opt.param_groups:
        assert g['momentum'] == 0.9 and g['initial_lr'] == g['lr'] and len(g['param_names']) == len(g['params'])
    by_name = {n: gi for gi, g in enumerate(opt.param_groups) for n in g['param_names']}
    assert (by_name[HEAD_W], by_name[BN_W], by_name[PW_B], by_name[DW_B]) == (0, 1, 1, 2)
    # no paramwise_cfg: one group, every parameter, the default path
    one = build_optimizer(model, dict(type='SGD', lr=LR, momentum=0.9, weight_decay=WD))
    assert len(one.param_groups) == 1 and len(one.param_groups[0]['params']) == n_params and not one._grouped()


def test_errors(model):
    with pytest.raises(ValueError, match='base_wd'):
        build_optimizer(model, dict(type='SGD', lr=LR, paramwise_cfg=dict(norm_decay_mult=0.)))
    with pytest.raises(ValueError, match='base_wd'):
        build_optimizer(model, dict(type='SGD', lr=LR, paramwise_cfg=dict(custom_keys={'bn': dict(decay_mult=0.)})))
    with pytest.raises(NotImplementedError, match='dcn_offset_lr_mult'):
        sgd(model, dcn_offset_lr_mult=0.1)
    with pytest.raises(NotImplementedError, match='amsgrad'):
        build_optimizer(model, dict(type='AdamW', lr=1e-3, amsgrad=True))
    with pytest.raises(NotImplementedError, match='Lamb'):
        build_optimizer(model, dict(type='Lamb', lr=1e-3))
    with pytest.raises(ValueError, match='unknown'):
        sgd(model, nrom_decay_mult=0.)
    opt = sgd(model)
    for bad in (3, 0.5):
        with pytest.raises(ValueError, match='norm_type'):
            opt.set_grad_clip(dict(max_norm=1.0, norm_type=bad))
    opt.set_grad_clip(dict(max_norm=35, norm_type=2))
    assert opt.grad_clip == dict(max_norm=35.0, norm_type=2) and opt._grouped()
    # more than 255 groups: one per parameter with its own lr
    many = {n: dict(lr_mult=2.0 + i) for i, (n, _) in enumerate(model.named_parameters()) if i < 120}
    assert len(sgd(model, custom_keys=many).param_groups) == 121
    p = list(model.parameters())
    with pytest.raises(ValueError, match='255'):
        FusedSGD(model, lr=LR, groups=[dict(lr=LR * (i + 1), weight_decay=0.0, params=[p[i % len(p)]]) for i in range(256)])


def test_adam_and_adamw(model):
    a = build_optimizer(model, dict(type='Adam', lr=1e-3, betas=(0.8, 0.99), weight_decay=1e-4))
    w = build_optimizer(model, dict(type='AdamW', lr=1e-3, weight_decay=0.05, paramwise_cfg=dict(norm_decay_mult=0.)))
    assert isinstance(a, FusedAdam) and not a.decoupled and a.param_groups[0]['betas'] == (0.8, 0.99)
    assert w.decoupled and [g['weight_decay'] for g in w.param_groups] == [0.05, 0.0]
    assert w.param_groups[0]['eps'] == 1e-8
    # no weight_decay key: torch's defaults (AdamW 1e-2, Adam 0)
    assert build_optimizer(model, dict(type='AdamW', lr=1e-3)).param_groups[0]['weight_decay'] == 1e-2
    assert build_optimizer(model, dict(type='Adam', lr=1e-3)).param_groups[0]['weight_decay'] == 0.0


class _Runner:
    def __init__(self, opt):
        self.optimizer, self.epoch, self.iter, self.max_epochs, self.max_iters = opt, 0, 0, 10, 1000


def test_lr_hook_follows_each_groups_initial_lr(model):
    opt = sgd(model, bias_lr_mult=2., custom_keys={'bbox_head': dict(lr_mult=0.)})
    bases = [g['initial_lr'] for g in opt.param_groups]
    assert sorted(bases) == [0.0, LR, 2 * LR]
    cfg = dict(policy='CosineAnnealing', min_lr=1e-3, by_epoch=False, warmup='linear', warmup_iters=100, warmup_ratio=0.1)
    hook = R.StepLrUpdaterHook(**cfg)
    run = _Runner(opt)
    hook.before_run(run)
    for it in (0, 50, 99, 100, 500, 999):
        run.iter = it
        hook.before_train_iter(run)
        for g, b in zip(opt.param_groups, bases):
            # mmcv, written out: annealing_cos(base, min_lr, it / max_iters), then the linear warm-up of that value
            want = 1e-3 + 0.5 * (b - 1e-3) * (math.cos(math.pi * it / 1000) + 1)
            if it < 100:
                want *= 1 - (1 - it / 100) * (1 - 0.1)
            assert g['lr'] == pytest.approx(want, rel=1e-12, abs=1e-18), (it, b)
    # not a multiple of the base schedule: with min_lr the 2x group is NOT at twice the 1x group
    lr = {g['initial_lr']: g['lr'] for g in opt.param_groups}
    assert lr[2 * LR] != pytest.approx(2 * lr[LR], rel=1e-3)


def test_state_dict_round_trip(model):
    n = sum(p.numel() for p in model.parameters())
    pw = dict(norm_decay_mult=0., bias_lr_mult=2.)
    a = build_optimizer(model, dict(type='AdamW', lr=1e-3, weight_decay=0.05, paramwise_cfg=pw))
    a._state = dict(exp_avg=torch.randn(n), exp_avg_sq=torch.rand(n))
    a._steps = 7
    a.param_groups[1]['lr'] = 3e-4
    sd = a.state_dict()
    b = build_optimizer(model, dict(type='AdamW', lr=1e-3, weight_decay=0.05, paramwise_cfg=pw))
    b.load_state_dict(sd)
    assert b._steps == 7 and torch.equal(b._state['exp_avg'], sd['exp_avg']) and torch.equal(b._state['exp_avg_sq'], sd['exp_avg_sq'])
    strip = lambda gs: [{k: v for k, v in g.items() if k != 'params'} for g in gs]      # noqa: E731
    assert strip(b.param_groups) == strip(a.param_groups) and b.param_groups[1]['lr'] == 3e-4
    s = sgd(model, norm_decay_mult=0.)
    s._buf, s._steps = torch.randn(n), 4
    s2 = sgd(model, norm_decay_mult=0.)
    s2.load_state_dict(s.state_dict())
    assert s2._steps == 4 and torch.equal(s2._buf, s._buf) and strip(s2.param_groups) == strip(s.param_groups)


def test_torch_format_adam_state_waits_for_the_layout(model):
    """torch.optim.AdamW's state dict (one group, parameters numbered in model.parameters() order) is kept per parameter
    until the engine's flat layout exists -- resume happens before the first forward."""
    ps = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    ref = torch.optim.AdamW(ps, lr=1e-3)
    for p in ps:
        p.grad = torch.ones_like(p)
    ref.step()
    ref.step()
    opt = build_optimizer(model, dict(type='AdamW', lr=1e-3))
    opt.load_state_dict(ref.state_dict())
    assert opt._steps == 2 and opt._pending is not None and len(opt._pending) == len(ps)
    p0, st0 = opt._pending[0]
    assert p0 is next(model.parameters()) and torch.equal(st0['exp_avg'], ref.state[ps[0]]['exp_avg'].reshape(-1))
