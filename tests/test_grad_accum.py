"""CPU: the gradient-accumulation hooks (runner.GradientCumulativeOptimizerHook and its fp16 variant) -- their schedule
against a literal restatement of mmcv's rule, the two warnings, the config surface -- and the C header's new entry.
No GPU: runner, model and optimizer are fakes that record the calls."""
import os
import re

import pytest
import torch
import torch.nn as nn

import yunet_amd.runner as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'yunet_hip.h')


# ------------------------------------------------------------------------------------------------------------- fakes
class FakeLoss:
    """runner.outputs['loss']: remembers what it was multiplied and divided by, and records the backward."""

    def __init__(self, log, mul=1.0, div=None):
        self.log, self.mul, self.div = log, mul, div

    def __truediv__(self, d):
        return FakeLoss(self.log, self.mul, d)

    def __mul__(self, m):
        return FakeLoss(self.log, self.mul * m, self.div)

    def backward(self):
        self.log.append(('backward', self.div, self.mul))


class FakeOptimizer:
    def __init__(self, log):
        self.log = log
        self.param_groups = [dict(lr=0.1)]
        self.clip_seen = 'unset'

    def set_grad_clip(self, grad_clip):
        self.clip_seen = grad_clip

    def step(self):
        self.log.append(('step',))

    def zero_grad(self):
        self.log.append(('zero_grad',))


class FakeModel(nn.Module):
    def __init__(self, bn=True):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 1)
        if bn:
            self.bn = nn.BatchNorm2d(4)
        self.accum = None

    def set_grad_accumulation(self, flag=True):
        self.accum = flag


class Wrapped(nn.Module):                 # what a data-parallel wrapper looks like to the hook
    def __init__(self, module):
        super().__init__()
        self.module = module


class FakeRunner:
    def __init__(self, model, start, max_iters):
        self.log, self.messages = [], []
        self.model, self.optimizer = model, FakeOptimizer(self.log)
        self.iter, self.max_iters = start, max_iters
        self.outputs = None

    def logger(self, msg):
        self.messages.append(msg)


def mmcv_rule(start, max_iters, k):
    """mmcv/runner/hooks/optimizer.py, GradientCumulativeOptimizerHook, restated: _init at the first iteration, then per
    iteration the loss factor and whether the optimizer steps; the factor's threshold relative to the starting iteration
    (the hook's documented deviation; identical for start = 0)."""
    residual_iters = max_iters - start
    divisible_iters = residual_iters // k * k
    remainder_iters = residual_iters - divisible_iters
    out = []
    for it in range(start, max_iters):
        loss_factor = k if it < start + divisible_iters else remainder_iters
        every_n_iters = (it + 1) % k == 0
        is_last_iter = it + 1 == max_iters
        out.append((loss_factor, every_n_iters or is_last_iter))
    return out


def drive(hook, start, max_iters, model=None):
    model = model if model is not None else FakeModel()
    model.train()
    runner = FakeRunner(model, start, max_iters)
    hook.before_run(runner)
    per_iter = []
    for it in range(start, max_iters):
        runner.iter = it
        runner.outputs = dict(loss=FakeLoss(runner.log), log_vars={})
        n0 = len(runner.log)
        hook.after_train_iter(runner)
        per_iter.append(runner.log[n0:])
    return runner, per_iter


# ---------------------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize('k', [1, 2, 3, 4])
@pytest.mark.parametrize('start,max_iters', [(0, 8), (0, 5), (4, 8), (3, 8), (2, 5), (12, 17)])
def test_schedule_is_mmcvs(start, max_iters, k):
    runner, per_iter = drive(R.GradientCumulativeOptimizerHook(cumulative_iters=k), start, max_iters)
    want = mmcv_rule(start, max_iters, k)
    assert len(per_iter) == len(want) == max_iters - start
    for it, (calls, (factor, boundary)) in enumerate(zip(per_iter, want), start):
        # no zero_grad in front of the backward; step and zero_grad, in that order, at a boundary only
        assert calls[0] == ('backward', factor, 1.0), (it, calls)
        assert calls[1:] == ([('step',), ('zero_grad',)] if boundary else []), (it, calls)
        assert factor >= 1
    # the last iteration of a run always flushes, and every backward lies in front of an update
    assert per_iter[-1][-2:] == [('step',), ('zero_grad',)]
    # a window that is not cut short by the run's end or a resume holds k backwards
    if start % k == 0 and (max_iters - start) % k == 0:
        assert sum(c == ('step',) for calls in per_iter for c in calls) == (max_iters - start) // k
    assert runner.model.accum is True and runner.optimizer.clip_seen is None


def test_remainder_window_divides_by_its_own_length():
    """max_iters 5, k 2 (the GPU runner test's geometry): factors 2 2 2 2 1, updates after iterations 1, 3 and 4."""
    _, per_iter = drive(R.GradientCumulativeOptimizerHook(cumulative_iters=2), 0, 5)
    assert [c[0][1] for c in per_iter] == [2, 2, 2, 2, 1]
    assert [len(c) == 3 for c in per_iter] == [False, True, False, True, True]


def test_fp16_hook_scales_the_loss_and_keeps_the_schedule():
    hook = R.GradientCumulativeFp16OptimizerHook(cumulative_iters=3, loss_scale=512.)
    assert hook.scale == 512. and not hook.dynamic and hook.cumulative_iters == 3
    runner = FakeRunner(FakeModel(), 0, 8)
    seen = []
    hook._unscale_and_step = lambda r: seen.append(r.iter)        # (the device part: tests/test_grad_accum_gpu.py)
    for it in range(8):
        runner.iter = it
        runner.outputs = dict(loss=FakeLoss(runner.log))
        hook.after_train_iter(runner)
    want = mmcv_rule(0, 8, 3)
    backs = [c for c in runner.log if c[0] == 'backward']
    assert backs == [('backward', f, 512.) for f, _ in want]
    assert seen == [it for it, (_, b) in enumerate(want) if b] == [2, 5, 7]
    assert runner.log.count(('zero_grad',)) == 3 and ('step',) not in runner.log
    dyn = R.GradientCumulativeFp16OptimizerHook(cumulative_iters=2, loss_scale='dynamic')
    assert dyn.dynamic and dyn.scale == 2. ** 16


def test_before_run_unwraps_the_model_and_hands_the_clip_to_a_fused_optimizer():
    inner = FakeModel()
    runner = FakeRunner(Wrapped(inner), 0, 4)
    clip = dict(max_norm=3.0, norm_type=2)
    R.GradientCumulativeOptimizerHook(cumulative_iters=2, grad_clip=clip).before_run(runner)
    assert inner.accum is True and runner.optimizer.clip_seen == clip


# ---------------------------------------------------------------------------------------------------------- warnings
def test_warnings():
    resumed = 'Resume iter number is not divisible by cumulative_iters'
    bn = 'BatchNorm'
    # divisible start, BatchNorm in train mode, k > 1: the BatchNorm warning alone
    runner, _ = drive(R.GradientCumulativeOptimizerHook(cumulative_iters=2), 4, 8)
    assert len(runner.messages) == 1 and bn in runner.messages[0]
    # resumed off a boundary: both
    runner, _ = drive(R.GradientCumulativeOptimizerHook(cumulative_iters=2), 3, 8)
    assert len(runner.messages) == 2 and resumed in runner.messages[0] and bn in runner.messages[1]
    # k = 1: nothing accumulates, nothing to warn about
    runner, _ = drive(R.GradientCumulativeOptimizerHook(cumulative_iters=1), 3, 8)
    assert runner.messages == []
    # no BatchNorm layer
    runner, _ = drive(R.GradientCumulativeOptimizerHook(cumulative_iters=2), 0, 4, model=FakeModel(bn=False))
    assert runner.messages == []


def test_batchnorm_warning_is_silent_with_every_layer_in_eval():
    class Frozen(FakeModel):
        def train(self, mode=True):              # norm_eval: train() keeps the statistics frozen
            super().train(mode)
            self.bn.eval()
            return self
    runner, _ = drive(R.GradientCumulativeOptimizerHook(cumulative_iters=4), 0, 8, model=Frozen())
    assert runner.messages == []
    runner, _ = drive(R.GradientCumulativeOptimizerHook(cumulative_iters=4), 2, 8, model=Frozen())
    assert len(runner.messages) == 1 and 'Resume' in runner.messages[0]
    # a logger object (mmcv's runner.logger) takes the warning through .warning
    class Log:
        def __init__(self):
            self.w = []

        def warning(self, msg):
            self.w.append(msg)
    r = FakeRunner(FakeModel().train(), 0, 4)
    r.logger = Log()
    r.outputs = dict(loss=FakeLoss(r.log))
    R.GradientCumulativeOptimizerHook(cumulative_iters=2).after_train_iter(r)
    assert len(r.logger.w) == 1 and 'BatchNorm' in r.logger.w[0]


# ---------------------------------------------------------------------------------------------------- config surface
def registered(optimizer_config):
    runner = R.EpochBasedRunner(FakeModel(), FakeOptimizer([]), max_epochs=1)
    runner.register_training_hooks(None, optimizer_config)
    assert len(runner.hooks) == 1
    return runner.hooks[0]


def cfg_of(**kw):
    import yunet_amd
    return yunet_amd.Config(yunet_amd.registry.ConfigDict.wrap(kw))


def test_config_surface():
    # optimizer_config.type reaches the hooks through the runner's lookup (a KeyError before they existed)
    h = registered(dict(type='GradientCumulativeOptimizerHook', cumulative_iters=4))
    assert type(h) is R.GradientCumulativeOptimizerHook and h.cumulative_iters == 4 and h.grad_clip is None
    h = registered(dict(type='GradientCumulativeOptimizerHook', cumulative_iters=2, grad_clip=dict(max_norm=35, norm_type=2)))
    assert h.grad_clip == dict(max_norm=35, norm_type=2)
    h = registered(dict(type='GradientCumulativeFp16OptimizerHook', cumulative_iters=2, loss_scale=128.))
    assert type(h) is R.GradientCumulativeFp16OptimizerHook and h.scale == 128. and h.cumulative_iters == 2
    assert isinstance(h, R.Fp16OptimizerHook) and h.priority == R.PRIORITY['ABOVE_NORMAL']
    # train_detector's choice (optimizer_hook_config): cfg.fp16 with a cumulative type -> the cumulative fp16 hook
    for t in R.CUMULATIVE_HOOKS:
        oc = R.optimizer_hook_config(cfg_of(fp16=dict(loss_scale='dynamic'),
                                            optimizer_config=dict(type=t, cumulative_iters=3, grad_clip=dict(max_norm=1.0))))
        h = registered(oc)
        assert type(h) is R.GradientCumulativeFp16OptimizerHook and h.dynamic and h.cumulative_iters == 3
        assert h.grad_clip == dict(max_norm=1.0)
    # ... without cfg.fp16 the dict goes through unchanged
    oc = R.optimizer_hook_config(cfg_of(optimizer_config=dict(type='GradientCumulativeOptimizerHook', cumulative_iters=3)))
    assert isinstance(oc, dict) and type(registered(oc)) is R.GradientCumulativeOptimizerHook
    # every other combination builds what it built before
    assert type(registered(R.optimizer_hook_config(cfg_of(optimizer_config=dict(grad_clip=None))))) is R.OptimizerHook
    assert type(registered(R.optimizer_hook_config(cfg_of()))) is R.OptimizerHook
    h = registered(R.optimizer_hook_config(cfg_of(fp16=dict(loss_scale=512.), optimizer_config=dict(grad_clip=None))))
    assert type(h) is R.Fp16OptimizerHook and h.scale == 512.
    h = registered(R.optimizer_hook_config(cfg_of(fp16=dict(loss_scale=512.), optimizer_config=dict(type='OptimizerHook'))))
    assert type(h) is R.Fp16OptimizerHook
    assert type(registered(dict(type='Fp16OptimizerHook', loss_scale=64.))) is R.Fp16OptimizerHook


def test_unknown_options_are_not_swallowed():
    with pytest.raises((TypeError, NotImplementedError)):
        registered(dict(type='GradientCumulativeOptimizerHook', cumulative_iters=2, cumulative_steps=4))
    with pytest.raises((TypeError, NotImplementedError)):
        registered(dict(type='GradientCumulativeFp16OptimizerHook', cumulative_iters=2, bogus=1))
    with pytest.raises((TypeError, NotImplementedError)):
        R.optimizer_hook_config(cfg_of(fp16=dict(loss_scale=512.),
                                       optimizer_config=dict(type='GradientCumulativeOptimizerHook', accumulate=2)))
    for bad in (0, -1, 2.0, '2', True):
        with pytest.raises((TypeError, NotImplementedError)):
            R.GradientCumulativeOptimizerHook(cumulative_iters=bad)


def test_deterministic_with_the_fp16_cumulative_hook_is_refused():
    """cfg.deterministic is allowed with the plain cumulative hook (the GPU test runs it); the fp16 one is refused like
    cfg.fp16 itself, before anything touches a device."""
    for extra in (dict(fp16=dict(loss_scale=512.), optimizer_config=dict(type='GradientCumulativeOptimizerHook')),
                  dict(optimizer_config=dict(type='GradientCumulativeFp16OptimizerHook', cumulative_iters=2))):
        for level in (True, 'fast'):
            with pytest.raises(NotImplementedError, match='deterministic'):
                R.train_detector(FakeModel(), None, cfg_of(deterministic=level, **extra))


# ------------------------------------------------------------------------------------------------------------ header
def test_header_declares_the_entry_and_keeps_the_abi_number():
    import yunet_amd._lib as L
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+yunet_grad_accum\s*\(([^)]*)\)\s*;', txt)
    assert m, 'yunet_grad_accum is not declared'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 5 and args[2].startswith('int64_t') and args[4].startswith('void*')
    assert re.search(r'YUNET_ACCUM_SAVE\s*=\s*0\s*,\s*YUNET_ACCUM_ADD\s*=\s*1', txt)
    assert (L.ACCUM_SAVE, L.ACCUM_ADD) == (0, 1) and len(L._SIGNATURES['yunet_grad_accum'][1]) == 5
    assert re.search(r'#define\s+YUNET_ABI_VERSION\s+12\b', txt)
    lib = L.load()
    assert lib.yunet_abi_version() == 12 and hasattr(lib, 'yunet_grad_accum')
    # n = 0 is a clean no-op (nothing is launched: no device needed), a bad mode or a negative n is refused
    assert lib.yunet_grad_accum(None, None, 0, L.ACCUM_ADD, None) == 0
    assert lib.yunet_grad_accum(None, None, 0, 2, None) == L.EINVAL
    assert lib.yunet_grad_accum(None, None, -1, L.ACCUM_SAVE, None) == L.EINVAL


def test_zero_grad_of_a_fused_optimizer_stays_a_no_op_without_an_engine():
    from yunet_amd.optim import FusedSGD
    m = FakeModel()
    m.engine = None
    assert FusedSGD(m, lr=0.1).zero_grad() is None

    class Eng:
        zeroed = 0

        def mark_grad_zeroed(self):
            self.zeroed += 1
    m.engine = Eng()
    opt = FusedSGD(m, lr=0.1)
    opt.zero_grad()
    opt.zero_grad(set_to_none=True)
    assert m.engine.zeroed == 2
