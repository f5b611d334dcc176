#!/usr/bin/env python
"""What the deterministic mode costs, and what it removes (needs a GPU; reads nothing outside the repository).

    tools/deterministic_probe.py --out profiles/deterministic.json [--kind n --size 320 --batch 256 --steps 20 --runs 20]
    tools/deterministic_probe.py --fast --out profiles/deterministic_fast.json

* step time of the default and the deterministic mode for one model in one process, alternating A B B A (A = default), each
  block `--warmup` untimed + `--steps` timed steps (forward, backward, SGD) between two events: the four times, the two means
  and their ratio.  No threshold: the ratio is the result.
* `--runs` consecutive evaluations of one step (forward + backward, no update) from the same state and batch in each mode:
  how many distinct byte patterns the flat gradient took.  Default mode: the spread this mode removes (a measurement, the
  count varies from run to run); deterministic mode: 1.
* `--fast`: the third mode, deterministic='fast' (the order-fixed forms of the default mode's kernels), in the same process:
  blocks A B C C B A (A = default, B = True, C = 'fast'), the three means, the ratios of 'fast' to the default mode and to
  True, and per mode the gradient's byte patterns over `--runs` evaluations with their hash.
"""
import argparse
import hashlib
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
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--fast', action='store_true', help="also measure deterministic='fast' (blocks A B C C B A)")
    a = ap.parse_args(argv)
    import yunet_oracle as O
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{a.kind}.py'))
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(O.init_state(O.yunet_arch(a.kind), seed=1), strict=True)
    m.to(dev).train()
    opt = FusedSGD(m, lr=1e-5, momentum=0.9, weight_decay=5e-4)
    batch = S.to_device(S.make_batch(a.batch, a.size, a.size, 1234), dev)

    def step(update=True):
        out = m.train_step(batch, opt)
        opt.zero_grad()
        out['loss'].backward()
        if update:
            opt.step()

    def timed(det):
        m.set_deterministic(det)
        for _ in range(a.warmup):
            step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    if a.fast:
        return three_modes(a, m, step, timed)
    order = [False, True, True, False]
    times = [timed(d) for d in order]
    dflt, det = (times[0] + times[3]) / 2, (times[1] + times[2]) / 2

    def patterns(det):
        m.set_deterministic(det)
        seen = set()
        for _ in range(a.runs):
            step(update=False)
            torch.cuda.synchronize()
            seen.add(hashlib.sha256(m.engine.params.grad.cpu().numpy().tobytes()).hexdigest())
        return len(seen)

    res = dict(model=f'yunet_{a.kind}', size=a.size, batch=a.batch, steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0),
               order=['deterministic' if d else 'default' for d in order], ms_per_step=[round(t, 4) for t in times],
               default_ms=round(dflt, 4), deterministic_ms=round(det, 4), ratio=round(det / dflt, 4),
               runs=a.runs, distinct_gradient_byte_patterns=dict(default=patterns(False), deterministic=patterns(True)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


def three_modes(a, m, step, timed):
    names = {False: 'default', True: 'deterministic', 'fast': 'fast'}
    order = [False, True, 'fast', 'fast', True, False]
    times = [timed(d) for d in order]
    mean = {names[d]: (times[i] + times[5 - i]) / 2 for i, d in enumerate(order[:3])}

    def patterns(det):
        m.set_deterministic(det)
        seen = []
        for _ in range(a.runs):
            step(update=False)
            torch.cuda.synchronize()
            h = hashlib.sha256(m.engine.params.grad.cpu().numpy().tobytes()).hexdigest()
            if h not in seen:
                seen.append(h)
        return dict(distinct=len(seen), sha256=seen[:4])

    res = dict(model=f'yunet_{a.kind}', size=a.size, batch=a.batch, steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), order=[names[d] for d in order], ms_per_step=[round(t, 4) for t in times],
               default_ms=round(mean['default'], 4), deterministic_ms=round(mean['deterministic'], 4), fast_ms=round(mean['fast'], 4),
               ratio_deterministic_to_default=round(mean['deterministic'] / mean['default'], 4),
               ratio_fast_to_default=round(mean['fast'] / mean['default'], 4),
               ratio_fast_to_deterministic=round(mean['fast'] / mean['deterministic'], 4),
               runs=a.runs, gradient_byte_patterns={names[d]: patterns(d) for d in (False, True, 'fast')})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
