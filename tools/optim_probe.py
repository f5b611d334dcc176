#!/usr/bin/env python
"""Times the clip-plus-update path over the flat buffers of YuNet_n and YuNet_s on the GPU of this box.

  (A) the former form: torch.nn.utils.clip_grad_norm_ over the per-parameter views of the flat gradient, then
      yunet_sgd_step_ex;
  (B) the fused form: yunet_grad_norm, then yunet_sgd_step_grouped reading the coefficient from device memory;
  and the grouped update (three groups, as paramwise_cfg makes them) against the ungrouped one, both without clipping.

The variants alternate in one process on one box; a sample is the wall time of `--iters` back-to-back iterations
(launch cost included: that is what a training iteration pays) divided by their number, after a synchronize.  Medians and
the spread over `--rounds` samples per variant go to profiles/optim_surface.json together with the box.

  python tools/optim_probe.py [--iters 200] [--rounds 15] [--out profiles/optim_surface.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import yunet_amd  # noqa: E402
import yunet_amd.kernels as K  # noqa: E402
from yunet_amd.optim import build_param_groups  # noqa: E402

DEV = 'cuda'


def flat_model(variant):
    """Flat parameter / gradient buffers of the model's size, the per-parameter views torch would clip, the group map."""
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{variant}.py'))
    model = yunet_amd.build_detector(cfg.model)
    named = list(model.named_parameters())
    n = sum(p.numel() for _, p in named)
    gen = torch.Generator().manual_seed(1)
    flat = (torch.randn(n, generator=gen) * 0.1).to(DEV)
    grad = torch.randn(n, generator=gen).to(DEV)
    groups = build_param_groups(model, 0.01, 5e-4, dict(norm_decay_mult=0., bias_decay_mult=0., dwconv_decay_mult=0.5))
    group_of = {id(p): gi for gi, g in enumerate(groups) for p in g['params']}
    views, gid, off = [], torch.zeros(n, dtype=torch.uint8), 0
    for _, p in named:
        v = flat[off:off + p.numel()].view(p.shape)
        v.grad = grad[off:off + p.numel()].view(p.shape)
        views.append(v)
        gid[off:off + p.numel()] = group_of[id(p)]
        off += p.numel()
    table = torch.tensor([[g['lr'], g['weight_decay'], 0.9, 0.0] for g in groups], dtype=torch.float64, device=DEV)
    return dict(n=n, views=views, flat=flat, grad=grad, gid=gid.to(DEV), table=table, groups=len(groups))


def variants(m):
    buf = torch.zeros_like(m['flat'])
    lr_dev = torch.tensor([0.0], device=DEV)                   # lr 0: the buffers keep their values over the run
    one_gid = torch.zeros_like(m['gid'])
    one_table = torch.tensor([[0.0, 5e-4, 0.9, 0.0]], dtype=torch.float64, device=DEV)
    table0 = m['table'].clone()
    table0[:, 0] = 0.0
    scratch, out = K.grad_norm_scratch(DEV), torch.empty(2, device=DEV)
    max_norm = 1e9                                             # coefficient 1: the gradient keeps its values too

    def a_torch_clip_then_sgd():
        torch.nn.utils.clip_grad_norm_(m['views'], max_norm, 2)
        K.sgd_step(m['flat'], m['grad'], buf, lr_dev, 0.9, 5e-4)

    def b_norm_kernel_then_grouped():
        K.grad_norm(m['grad'], max_norm, 2, scratch=scratch, out=out)
        K.sgd_step_grouped(m['flat'], m['grad'], buf, one_gid, one_table, clip_coef=out[1:2])

    def ungrouped_update():
        K.sgd_step(m['flat'], m['grad'], buf, lr_dev, 0.9, 5e-4)

    def grouped_update():
        K.sgd_step_grouped(m['flat'], m['grad'], buf, m['gid'], table0)

    return dict(A_torch_clip_then_sgd=a_torch_clip_then_sgd, B_norm_kernel_then_grouped=b_norm_kernel_then_grouped,
                ungrouped_update=ungrouped_update, grouped_update=grouped_update)


def sample(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_surface.json'))
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    res = dict(box=dict(device=props.name, arch=getattr(props, 'gcnArchName', ''),
                        compute_units=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip),
               unit='microseconds per iteration (wall, launches included; median / min / max over the rounds)',
               iters=a.iters, rounds=a.rounds, models={})
    for variant in ('n', 's'):
        m = flat_model(variant)
        fns = variants(m)
        for fn in fns.values():                                # warm-up: first launches, allocator, clocks
            sample(fn, a.iters)
        times = {k: [] for k in fns}
        for _ in range(a.rounds):                              # alternate the variants inside every round
            for k, fn in fns.items():
                times[k].append(sample(fn, a.iters))
        row = {k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
               for k, v in times.items()}
        row['B_over_A'] = round(row['B_norm_kernel_then_grouped']['median'] / row['A_torch_clip_then_sgd']['median'], 4)
        row['grouped_over_ungrouped'] = round(row['grouped_update']['median'] / row['ungrouped_update']['median'], 4)
        res['models'][f'yunet_{variant}'] = dict(elements=m['n'], parameters=len(m['views']), groups=m['groups'], **row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
