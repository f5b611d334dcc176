#!/usr/bin/env python
"""What gradient accumulation costs next to the default step (needs a GPU; reads nothing outside the repository).

    tools/grad_accum_probe.py --out profiles/grad_accum.json [--kind n --size 320 --batch 256 --steps 20 --warmup 4 --k 4]

One model, one process, ready batches.  Two loops over the same forward / backward / FusedSGD kernels:

    off    accumulation off: zero_grad, backward, step -- every iteration updates (OptimizerHook)
    k      accumulation on:  (loss / k).backward() every iteration; step + zero_grad every k-th
           (GradientCumulativeOptimizerHook)

Blocks run  off | k | k | off; each is `--warmup` untimed + `--steps` timed iterations between two device events (steps and
warm-up are multiples of k, so a block starts and ends on an update).  Reported per mode: ms per iteration (both blocks and
their mean), ms per update, and the launches of yunet_grad_accum inside the timed blocks.  No time is fixed in advance; the
expectation that IS checked (exit status 1 otherwise) is the launch count: with k > 1 the first backward of a window follows
a zero_grad and launches nothing, the other k - 1 launch SAVE and ADD -- "two short launches on three of four iterations"
at k = 4 -- and the off blocks launch none and allocate no buffer.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import torch  # noqa: E402

import yunet_amd  # noqa: E402
import yunet_amd.synthetic as S  # noqa: E402
from yunet_amd.optim import FusedSGD  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--kind', default='n')
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--k', type=int, default=4)
    a = ap.parse_args(argv)
    if a.k < 2 or a.steps % a.k or a.warmup % a.k:
        ap.error('--k >= 2, and --steps / --warmup multiples of it')
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{a.kind}.py'))
    m = yunet_amd.build_detector(cfg.model)
    ck = torch.load(os.path.join(ROOT, 'tests', 'golden', f'yunet_{a.kind}_synth_trained.pth'), map_location='cpu',
                    weights_only=False)
    m.load_state_dict(ck['state_dict'], strict=True)
    m.to(dev).train()
    opt = FusedSGD(m, lr=1e-5, momentum=0.9, weight_decay=5e-4)
    batches = [S.to_device(S.make_batch(a.batch, a.size, a.size, 1234 + i), dev) for i in range(a.k)]

    def iteration(i, k):
        out = m.train_step(batches[i % len(batches)], opt)
        if k == 1:
            opt.zero_grad()
            out['loss'].backward()
            opt.step()
            return
        (out['loss'] / k).backward()
        if (i + 1) % k == 0:
            opt.step()
            opt.zero_grad()

    def block(k):
        m.set_grad_accumulation(k > 1)
        opt.zero_grad()
        for i in range(a.warmup):
            iteration(i, k)
        before = dict(m.engine.accum_launches)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.steps):
            iteration(i, k)
        e1.record()
        torch.cuda.synchronize()
        after = dict(m.engine.accum_launches)
        return e0.elapsed_time(e1) / a.steps, {mode: after[mode] - before[mode] for mode in after}

    iteration(0, 1)                                   # binds the engine, builds the plan
    order = [1, a.k, a.k, 1]
    acc_after_first_off = None
    runs = []
    for idx, k in enumerate(order):
        runs.append(block(k))
        if idx == 0:
            acc_after_first_off = m.engine._acc is not None
    name = {1: 'off', a.k: f'k{a.k}'}
    modes = {}
    for k in (1, a.k):
        mine = [r for r, kk in zip(runs, order) if kk == k]
        ms = sum(t for t, _ in mine) / len(mine)
        modes[name[k]] = dict(ms_per_iteration=round(ms, 4), blocks=[round(t, 4) for t, _ in mine],
                              ms_per_update=round(ms * k, 4), updates_per_block=a.steps // k,
                              grad_accum_launches_per_block=[n for _, n in mine])
    want = dict(save=a.steps // a.k * (a.k - 1), add=a.steps // a.k * (a.k - 1))
    ok = (all(n == want for n in modes[name[a.k]]['grad_accum_launches_per_block'])
          and all(n == dict(save=0, add=0) for n in modes['off']['grad_accum_launches_per_block'])
          and acc_after_first_off is False)
    res = dict(model=f'yunet_{a.kind}', size=a.size, batch=a.batch, steps=a.steps, warmup=a.warmup, k=a.k,
               device=torch.cuda.get_device_name(0), order=[name[k] for k in order], modes=modes,
               ratio_per_iteration=round(modes[name[a.k]]['ms_per_iteration'] / modes['off']['ms_per_iteration'], 4),
               flat_gradient_bytes=4 * m.engine.layout.numel,
               expectation=dict(what=f'SAVE and ADD on {a.k - 1} of {a.k} iterations, none with the switch off, no buffer '
                                     'before the switch is first used',
                                launches_per_block_expected=want, buffer_allocated_by_off_block=acc_after_first_off, met=ok))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
