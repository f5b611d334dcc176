#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/custom_hooks_reference.{npz,json} by running the UNMODIFIED
reference hooks (mmdet/core/hook/ema.py, yunet_sample_size_statistics_hook.py, checkloss_hook.py) on the CPU:

    python tools/make_golden_custom_hooks.py          # needs the reference tree (oracle/ref_stub.py)

oracle/ref_stub.py's mmcv stub lacks what these files import; this tool adds it at run time, without touching
oracle/: mmcv.runner.hooks.{HOOKS, Hook} (a registry and mmcv's Hook stage dispatch) and
mmcv.parallel.is_module_wrapper.

EMA: a small conv + BatchNorm module driven by a fake runner over 2 epochs of 3 iterations; before each
after_train_iter every state_dict entry is overwritten from a seeded sequence (standing in for the optimizer and the
BN statistics update).  Per configuration (Exp / Linear, interval 1 / 2, skip_buffers both ways) the fixture holds the
EMA buffers after every iteration, the full state_dict after every epoch end (swapped), and the key order.
Statistics: fixed GT batches (empty images, repeated sizes, fractional and negative extents) through
before_train_iter, then dump_json.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ref_stub  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
EPOCHS, ITERS = 2, 3
CONFIGS = [  # name, hook type, kwargs
    ('exp_i1', 'ExpMomentumEMAHook', dict(momentum=0.25, interval=1, total_iter=5)),
    ('exp_i2', 'ExpMomentumEMAHook', dict(momentum=0.25, interval=2, total_iter=5)),
    ('exp_i1_skip', 'ExpMomentumEMAHook', dict(momentum=0.25, interval=1, total_iter=5, skip_buffers=True)),
    ('lin_i1', 'LinearMomentumEMAHook', dict(momentum=0.5, interval=1, warm_up=4)),
    ('lin_i2', 'LinearMomentumEMAHook', dict(momentum=0.5, interval=2, warm_up=4)),
    ('lin_i2_skip', 'LinearMomentumEMAHook', dict(momentum=0.5, interval=2, warm_up=4, skip_buffers=True)),
]


def tiny_module():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv2d(2, 3, 1), nn.BatchNorm2d(3), nn.Conv2d(3, 2, 1))


def state_sequence(model, n, seed=7):
    """n seeded states: fp32 entries ~ N(0, 1), num_batches_tracked = iteration + 1."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for it in range(n):
        st = {}
        for k, v in model.state_dict().items():
            st[k] = (torch.full_like(v, it + 1) if not v.dtype.is_floating_point
                     else torch.randn(v.shape, generator=g, dtype=v.dtype))
        out.append(st)
    return out


def install_hook_stubs():
    ref_stub._install_mmcv_stub()
    import mmcv
    hooks = types.ModuleType('mmcv.runner.hooks')
    hooks.HOOKS = ref_stub._Registry('hook')

    class Hook:
        def before_run(self, runner): pass                    # noqa: E704
        def after_run(self, runner): pass                     # noqa: E704
        def before_epoch(self, runner): pass                  # noqa: E704
        def after_epoch(self, runner): pass                   # noqa: E704
        def before_iter(self, runner): pass                   # noqa: E704
        def after_iter(self, runner): pass                    # noqa: E704
        def before_train_epoch(self, runner): self.before_epoch(runner)      # noqa: E704
        def after_train_epoch(self, runner): self.after_epoch(runner)        # noqa: E704
        def before_train_iter(self, runner): self.before_iter(runner)        # noqa: E704
        def after_train_iter(self, runner): self.after_iter(runner)          # noqa: E704

        def every_n_iters(self, runner, n):
            return (runner.iter + 1) % n == 0 if n > 0 else False

    hooks.Hook = Hook
    mmcv.runner.hooks = hooks
    sys.modules['mmcv.runner.hooks'] = hooks
    parallel = types.ModuleType('mmcv.parallel')
    parallel.is_module_wrapper = lambda m: False
    mmcv.parallel = parallel
    sys.modules['mmcv.parallel'] = parallel


def load_ref(name):
    path = os.path.join(ref_stub.REF_ROOT, 'mmdet', 'core', 'hook', name + '.py')
    spec = importlib.util.spec_from_file_location('ref_hook_' + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class FakeRunner:
    def __init__(self, model, work_dir=None):
        self.model, self.work_dir = model, work_dir
        self.iter = self.epoch = 0
        self.data_batch = self.outputs = None
        self.logged = []

    class _Logger:
        def __init__(self, sink):
            self.sink = sink

        def info(self, msg):
            self.sink.append(msg)

    @property
    def logger(self):
        return FakeRunner._Logger(self.logged)


def flat(sd, keys):
    return np.concatenate([sd[k].detach().double().reshape(-1).numpy() for k in keys])


def run_ema(ema, name, cls, kw, arrays, meta):
    model = tiny_module()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    seq = state_sequence(model, EPOCHS * ITERS)
    runner = FakeRunner(model)
    hook = getattr(ema, cls)(**kw)
    hook.before_run(runner)
    keys = list(model.state_dict().keys())
    ema_keys = [k for k in keys if k.startswith('ema_')]
    traj, ends = [], []
    for _ in range(EPOCHS):
        hook.before_train_epoch(runner)
        for _ in range(ITERS):
            with torch.no_grad():
                for k, v in seq[runner.iter].items():
                    model.state_dict()[k].copy_(v)
            hook.after_train_iter(runner)
            traj.append(flat(model.state_dict(), ema_keys))
            runner.iter += 1
        hook.after_train_epoch(runner)
        ends.append(flat(model.state_dict(), keys))
        runner.epoch += 1
    arrays[f'{name}/traj'] = np.stack(traj)
    arrays[f'{name}/epoch_end'] = np.stack(ends)
    arrays[f'{name}/momenta'] = np.array([hook.get_momentum(type('R', (), {'iter': i})) for i in range(EPOCHS * ITERS)])
    meta['ema'][name] = dict(type=cls, kwargs=kw, keys=keys, ema_keys=ema_keys)
    if name == CONFIGS[0][0]:
        arrays['init'] = flat(init, list(init))
        arrays['sequence'] = np.stack([flat(s, list(init)) for s in seq])
        meta['module_keys'] = list(init)
        meta['module_shapes'] = [list(v.shape) for v in init.values()]


class DC:
    """mmcv DataContainer as the collate delivers it: .data[0] is the per-image list."""

    def __init__(self, lst):
        self.data = [lst]


def stat_batches():
    f = np.float32
    return [
        [np.array([[0, 0, 10, 12], [5, 5, 15, 17], [1.5, 2.25, 11.75, 14.0]], f),
         np.zeros((0, 4), f),
         np.array([[3, 4, 33.9, 20.1], [0, 0, 10, 12]], f)],
        [np.array([[100, 50, 140.5, 99.999], [0, 0, 0.5, 0.25]], f),
         np.array([[7, 7, 17, 19], [2.0, 3.0, 1.5, 3.75], [8, 9, 38.9, 29.1]], f),
         np.zeros((0, 4), f)],
        [np.zeros((0, 4), f),
         np.array([[0, 0, 10, 12], [10, 20, 70, 80], [5, 5, 15, 17], [40, 30, 79.99, 63.5], [20, 20, 17.5, 25]], f)],
    ]


def run_stats(st, arrays, meta):
    batches = stat_batches()
    with tempfile.TemporaryDirectory() as d:
        runner = FakeRunner(None, work_dir=d)
        hook = st.YuNetSampleSizeStatisticsHook('stats.json', save_interval=1)
        hook.before_run(runner)
        for it, b in enumerate(batches):
            runner.iter = it
            runner.data_batch = {'gt_bboxes': DC([torch.from_numpy(x) for x in b])}
            hook.before_train_iter(runner)
        hook.dump_json()
        with open(os.path.join(d, 'stats.json')) as f:
            js = json.load(f)
    js.pop('datetime:')
    meta['stats'] = dict(json=js, iterations=list(range(len(batches))))
    for i, b in enumerate(batches):
        arrays[f'stats/batch{i}/n'] = np.array([len(x) for x in b], np.int32)
        arrays[f'stats/batch{i}/boxes'] = np.concatenate(b).astype(np.float32)


def run_checkloss(ck, meta):
    out = []
    for vals in ([1.0, float('nan'), 2.0, 3.0, float('inf'), float('-inf'), 5.0, float('nan')],):
        hook = ck.CheckInvalidLossHook(interval=2)
        runner = FakeRunner(None)
        for it, v in enumerate(vals):
            runner.iter = it
            runner.outputs = {'loss': torch.tensor(v)}
            try:
                hook.after_train_iter(runner)
                out.append([it, v, 'ok'])
            except AssertionError:
                out.append([it, v, 'assert'])
    meta['checkloss'] = dict(interval=2, results=[[i, repr(v), r] for i, v, r in out])


def main():
    if not ref_stub.available():
        sys.exit('the reference tree is not available')
    install_hook_stubs()
    ema, st, ck = load_ref('ema'), load_ref('yunet_sample_size_statistics_hook'), load_ref('checkloss_hook')
    arrays, meta = {}, dict(ema={}, epochs=EPOCHS, iters=ITERS)
    for name, cls, kw in CONFIGS:
        run_ema(ema, name, cls, kw, arrays, meta)
    run_stats(st, arrays, meta)
    run_checkloss(ck, meta)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, 'custom_hooks_reference.npz'), **arrays)
    with open(os.path.join(OUT, 'custom_hooks_reference.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print('wrote', sorted(arrays)[:4], '...', os.path.getsize(os.path.join(OUT, 'custom_hooks_reference.npz')), 'bytes')


if __name__ == '__main__':
    main()
