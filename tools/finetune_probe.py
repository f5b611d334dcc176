#!/usr/bin/env python
"""What a fine-tuning step costs next to the default step (needs a GPU; reads nothing outside the repository).

    tools/finetune_probe.py --out profiles/finetune.json [--kind n --size 320 --batch 256 --steps 20 --warmup 3]

Five modes of one model in one process, set through the modules' own flags as a user would:

    default          everything trains
    all_bn_frozen    every BatchNorm in eval() under model.train(); every parameter trains
    frozen_stages_2  YuNetBackbone.frozen_stages = 2: model0 .. model2 in eval(), their parameters without gradient
    backbone_frozen  frozen_stages = last stage: neck and head train
    head_only        backbone and neck frozen: the head trains

Blocks run A B C D E E D C B A; each is `--warmup` untimed + `--steps` timed steps (forward, backward, FusedSGD) between two
events.  Per mode: the two block times, their mean, the ratio to the default mode and the number of kernel ops in the
backward list.  No threshold: the figures are the result.  Weights: tests/golden/yunet_<kind>_synth_trained.pth (running
statistics a frozen layer can use).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import yunet_amd  # noqa: E402
import yunet_amd._lib as L  # noqa: E402
import yunet_amd.synthetic as S  # noqa: E402
from yunet_amd.optim import FusedSGD  # noqa: E402

MODES = ('default', 'all_bn_frozen', 'frozen_stages_2', 'backbone_frozen', 'head_only')


def set_mode(m, mode):
    """Back to the default flags, then the mode's."""
    for p in m.parameters():
        p.requires_grad = True
    m.backbone.frozen_stages = {'frozen_stages_2': 2, 'backbone_frozen': m.backbone.layer_num - 1,
                                'head_only': m.backbone.layer_num - 1}.get(mode, -1)
    m.train()
    if mode == 'all_bn_frozen':
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.eval()
    if mode == 'head_only':
        m.neck.eval()
        for p in m.neck.parameters():
            p.requires_grad = False


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--kind', default='n')
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{a.kind}.py'))
    m = yunet_amd.build_detector(cfg.model)
    ck = torch.load(os.path.join(ROOT, 'tests', 'golden', f'yunet_{a.kind}_synth_trained.pth'), map_location='cpu',
                    weights_only=False)
    m.load_state_dict(ck['state_dict'], strict=True)
    m.to(dev).train()
    opt = FusedSGD(m, lr=1e-5, momentum=0.9, weight_decay=5e-4)
    batch = S.to_device(S.make_batch(a.batch, a.size, a.size, 1234), dev)
    bwd_ops = {}

    def step():
        out = m.train_step(batch, opt)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()

    def timed(mode):
        set_mode(m, mode)
        for _ in range(a.warmup):
            step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        kernels = (L.OP_DP_BWD, L.OP_STEM_BWD, L.OP_POOL_BWD, L.OP_UPADD_BWD)
        bwd_ops[mode] = sum(op.opcode in kernels for op in m.engine.plan.bwd)
        return e0.elapsed_time(e1) / a.steps

    order = list(MODES) + list(reversed(MODES))
    times = [timed(mode) for mode in order]
    n = len(MODES)
    mean = {mode: (times[i] + times[2 * n - 1 - i]) / 2 for i, mode in enumerate(MODES)}
    res = dict(model=f'yunet_{a.kind}', size=a.size, batch=a.batch, steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), order=order, ms_per_step=[round(t, 4) for t in times],
               modes={mode: dict(ms=round(mean[mode], 4), blocks=[round(times[i], 4), round(times[2 * n - 1 - i], 4)],
                                 ratio_to_default=round(mean[mode] / mean['default'], 4), backward_kernel_ops=bwd_ops[mode])
                      for i, mode in enumerate(MODES)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
