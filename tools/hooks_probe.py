#!/usr/bin/env python
"""Cost of the custom hooks on the flagship step (YuNet_n, 320 x 320, batch 256), written to
profiles/custom_hooks.json:

  - one fused EMA update (yunet_ema_update over the flat parameters, running_mean and running_var): event timing
    of every launch, median of --launches;
  - the same update as the reference's per-tensor loop (mul_ then add_ per floating-point state_dict entry), event
    timing around the whole loop, median of --loops;
  - ms per iteration of the runner (resident synthetic batches) with no custom hook, with ExpMomentumEMAHook
    (priority 49) and with YuNetSampleSizeStatisticsHook: wall time between synchronised marks over --iters
    iterations after --warmup.

    python tools/hooks_probe.py [--out profiles/custom_hooks.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import yunet_amd  # noqa: E402
import yunet_amd.kernels as K  # noqa: E402
from yunet_amd.hooks import ExpMomentumEMAHook  # noqa: E402
from yunet_amd.optim import build_optimizer  # noqa: E402
from yunet_amd.runner import EpochBasedRunner, Hook, SyntheticWiderFace  # noqa: E402

S, BS = 320, 256


def make_model(cfg):
    m = yunet_amd.build_detector(cfg.model).to('cuda').train()
    return m, build_optimizer(m, cfg.optimizer)


class Timer(Hook):
    """Synchronised wall-clock marks: at the start of iteration `warmup` and after the run."""

    def __init__(self, warmup):
        self.warmup, self.t0, self.t1, self.n0 = warmup, None, None, None

    def before_train_iter(self, runner):
        if runner.iter == self.warmup:
            torch.cuda.synchronize()
            self.t0, self.n0 = time.perf_counter(), runner.iter

    def after_run(self, runner):
        torch.cuda.synchronize()
        self.t1 = time.perf_counter()
        self.ms = (self.t1 - self.t0) * 1e3 / (runner.iter - self.n0)


def runner_ms(cfg, custom, iters, warmup, work_dir):
    m, opt = make_model(cfg)
    r = EpochBasedRunner(m, opt, work_dir=work_dir, logger=lambda *a: None, max_epochs=1)
    r.register_training_hooks(None, dict(), None, None, None, custom)
    t = Timer(warmup)
    r.register_hook(t, 'LOWEST')
    r.run([SyntheticWiderFace(img_scale=(S, S), samples_per_gpu=BS, iters_per_epoch=iters, resident=4)], device='cuda')
    return t.ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'custom_hooks.json'))
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--loops', type=int, default=50)
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))

    # ---- the update alone, on a bound model with its EMA mirror
    m, opt = make_model(cfg)
    import yunet_amd.synthetic as SY
    b = SY.to_device(SY.make_batch(BS, S, S, 1), 'cuda')
    out = m.train_step(b, opt)
    opt.zero_grad()
    out['loss'].backward()
    opt.step()

    class R:
        model = m
    ExpMomentumEMAHook(momentum=1e-4).before_run(R)
    pairs, _ = m.engine.params.ema_pairs()
    seg = [p[0].numel() for p in pairs]
    torch.cuda.synchronize()
    for _ in range(20):
        K.ema_update(pairs, 1e-4)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
    for e0, e1 in ev:
        e0.record()
        K.ema_update(pairs, 1e-4)
        e1.record()
    torch.cuda.synchronize()
    fused = [e0.elapsed_time(e1) for e0, e1 in ev]

    sd = m.state_dict()
    bufs = dict(m.named_buffers())
    loop = [(sd[k], bufs['ema_' + k.replace('.', '_')]) for k in sd if not k.startswith('ema_')
            and sd[k].dtype.is_floating_point]

    def eager(mom=1e-4):
        for p, e in loop:
            e.mul_(1 - mom).add_(p, alpha=mom)
    for _ in range(5):
        eager()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.loops)]
    host = []
    for e0, e1 in ev:
        t = time.perf_counter()
        e0.record()
        eager()
        e1.record()
        host.append((time.perf_counter() - t) * 1e3)
    torch.cuda.synchronize()
    per_tensor = [e0.elapsed_time(e1) for e0, e1 in ev]
    n_loop = len(loop)
    del m, opt, pairs, loop, sd, bufs
    torch.cuda.empty_cache()

    # ---- the runner with and without the hooks
    with tempfile.TemporaryDirectory() as d:
        none = runner_ms(cfg, [], a.iters, a.warmup, d)
        ema = runner_ms(cfg, [dict(type='ExpMomentumEMAHook', momentum=1e-4, priority=49)], a.iters, a.warmup, d)
        stats = runner_ms(cfg, [dict(type='YuNetSampleSizeStatisticsHook', out_file='sizes.json', save_interval=50)],
                          a.iters, a.warmup, d)
    res = dict(
        workload=f'YuNet_n {S}x{S} batch {BS}, fp32, resident synthetic batches',
        device=torch.cuda.get_device_name(0),
        ema_segments_floats=seg,
        ema_tensors_in_reference_loop=n_loop,
        fused_ema_update_ms=dict(median=statistics.median(fused), min=min(fused), launches=len(fused)),
        reference_per_tensor_loop_ms=dict(median=statistics.median(per_tensor), min=min(per_tensor),
                                          host_issue_median=statistics.median(host), loops=len(per_tensor)),
        runner_ms_per_iter=dict(no_custom_hook=none, exp_momentum_ema_hook=ema, sample_size_statistics_hook=stats,
                                iters_timed=a.iters - a.warmup),
    )
    res['fused_share_of_step'] = res['fused_ema_update_ms']['median'] / none
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
