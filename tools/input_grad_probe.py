#!/usr/bin/env python
"""What the gradient with respect to the image costs (needs a GPU; reads nothing outside the repository).

    tools/input_grad_probe.py --out profiles/input_grad.json [--kind n --size 320 --batch 256 --steps 20 --warmup 3]

One model in one process:

    kernel      the backward-data launch alone (OP_STEM_BWD_DX of the step's own plan, replayed on the tensors the last
                step left): 3 untimed + 20 back-to-back launches between two events
    yardstick   the stem weight-gradient launch of the same plan (OP_STEM_BWD), timed the same way: it reads the same dy
                and the image
    step        the whole training step (forward, backward, FusedSGD) with the image detached | asking for a gradient,
                in blocks off / on / on / off of `--warmup` untimed + `--steps` timed steps

and the achieved GB/s of both launches on their algorithmic bytes (per z pixel: dy 64 B + z 64 B as stored in fp32 + 48 B
of image gradient | 64 B + 48 B of image).  No threshold: the figures are the result.  Weights:
tests/golden/yunet_<kind>_synth_trained.pth.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import torch  # noqa: E402

import yunet_amd  # noqa: E402
import yunet_amd._lib as L  # noqa: E402
import yunet_amd.synthetic as S  # noqa: E402
from yunet_amd.engine import Plan  # noqa: E402
from yunet_amd.optim import FusedSGD  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--kind', default='n')
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20)
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
    leaf = dict(batch)
    leaf['img'] = batch['img'].clone().requires_grad_(True)

    def step(on):
        b = leaf if on else batch
        leaf['img'].grad = None
        out = m.train_step(b, opt)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()

    def block(on):
        for _ in range(a.warmup):
            step(on)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step(on)
        e1.record()
        torch.cuda.synchronize()
        assert m.engine.plan.input_grad == on and (leaf['img'].grad is not None) == on
        return e0.elapsed_time(e1) / a.steps

    order = [False, True, True, False]
    times = [block(on) for on in order]
    off, on = (times[0] + times[3]) / 2, (times[1] + times[2]) / 2

    # the two launches alone, on the tensors the last input_grad step left in its plan
    step(True)
    torch.cuda.synchronize()
    plan = m.engine.plan
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    scratch = torch.empty(a.batch, 3, a.size, a.size, device=dev, dtype=torch.float32)

    def launch_ms(opcode, p0):
        idx = [i for i, op in enumerate(plan.bwd) if op.opcode == opcode]
        assert len(idx) == 1
        op = Plan._clone_op(plan.c_bwd[idx[0]])
        op.p[0] = p0
        arr = (L.YunetOp * 1)(op)
        for _ in range(3):
            L.check(lib.yunet_exec(arr, 1, stream), 'yunet_exec')
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            L.check(lib.yunet_exec(arr, 1, stream), 'yunet_exec')
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.launches

    t_dx = launch_ms(L.OP_STEM_BWD_DX, scratch.data_ptr())
    t_wg = launch_ms(L.OP_STEM_BWD, batch['img'].data_ptr())
    zpix = a.batch * (a.size // 2) * (a.size // 2)
    act = 2 if plan.act_dtype == torch.bfloat16 else 4
    bytes_dx, bytes_wg = zpix * (64 + 16 * act + 48), zpix * (64 + 48)
    res = dict(model=f'yunet_{a.kind}', size=a.size, batch=a.batch, steps=a.steps, warmup=a.warmup, launches=a.launches,
               device=torch.cuda.get_device_name(0),
               kernel=dict(name='stem_bwd_dx_kernel', ms=round(t_dx, 4), algorithmic_bytes=bytes_dx,
                           gb_per_s=round(bytes_dx / t_dx / 1e6, 1)),
               yardstick=dict(name='stem_mma_kernel<true> (OP_STEM_BWD)', ms=round(t_wg, 4), algorithmic_bytes=bytes_wg,
                              gb_per_s=round(bytes_wg / t_wg / 1e6, 1)),
               kernel_over_yardstick=round(t_dx / t_wg, 3),
               step=dict(order=['off', 'on', 'on', 'off'], ms_per_step=[round(t, 4) for t in times], off_ms=round(off, 4),
                         on_ms=round(on, 4), added_ms=round(on - off, 4), ratio=round(on / off, 4)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
