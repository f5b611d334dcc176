#!/usr/bin/env python
"""What a validation step costs, next to the steps it is built from (needs a GPU).

    tools/val_loss_probe.py --out profiles/val_workflow.json [--batch 256 --size 320 --blocks 6 --steps 30 --launches 200]

YuNet_n at the bench geometry (N = 256, 320 x 320) on one device, one process.  Every candidate runs warm passes first; then
the candidates alternate in blocks of `--steps` between two device events, `--blocks` times round, so that a drift of the
box falls on all of them alike (the spread of a candidate's block means is recorded beside its mean).

* step_ms: forward_val (eval conv stack + assignment + value-only loss), forward_eval (the conv stack alone) on the same
  batch, and the forward half of a training step (engine.forward: batch-statistics conv stack + assignment + loss with
  gradient + running-statistics update).
* loss_launch_us: yunet_loss_terms alone on the plan's buffers, with and without dflat, back to back.
* train_step_ms: the plain training step (forward, backward, SGD) before and after a validation epoch of `--steps` steps.
No threshold: nobody had measured these; the file records them.  That the training step is untouched is shown by the
byte-identical op lists (tests/test_val_workflow.py) and profiles/val_loss_codegen.txt, not by a time.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--blocks', type=int, default=6)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warm', type=int, default=10)
    ap.add_argument('--launches', type=int, default=200)
    a = ap.parse_args(argv)
    import torch

    import yunet_amd
    import yunet_amd._lib as L
    import yunet_amd.kernels as K
    import yunet_amd.synthetic as S
    from yunet_amd.optim import FusedSGD
    if not torch.cuda.is_available():
        raise SystemExit('val_loss_probe needs a GPU: no time is reported without one')
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    m = yunet_amd.build_detector(cfg.model)
    ck = torch.load(os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth'), map_location='cpu', weights_only=False)
    m.load_state_dict(ck['state_dict'], strict=True)
    m.to(dev).train()
    opt = FusedSGD(m, lr=1e-5, momentum=0.9, weight_decay=5e-4)
    batches = [S.to_device(S.make_batch(a.batch, a.size, a.size, 1234 + i, structured=True), dev) for i in range(2)]
    img = batches[0]['img'].float().contiguous()
    gb, gk = batches[0]['gt_bboxes'], batches[0]['gt_keypointss']

    def train_step(i=0):
        out = m.train_step(batches[i % 2], opt)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()

    train_step()
    eng = m.engine
    plan = eng.plan

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def alternate(cands, n, rounds):
        for fn in cands.values():
            timed(fn, a.warm)
        rows = {k: [] for k in cands}
        for _ in range(rounds):
            for k, fn in cands.items():
                rows[k].append(timed(fn, n))
        return {k: dict(mean=statistics.mean(v), min=min(v), max=max(v), blocks=v) for k, v in rows.items()}

    res = dict(model='yunet_n', batch=a.batch, size=a.size, device=torch.cuda.get_device_name(0), blocks=a.blocks,
               steps_per_block=a.steps, warm=a.warm, plans=None)
    # ---- the plain training step before any validation step ran on this plan
    res['train_step_ms'] = dict(before=alternate({'train': train_step}, a.steps, a.blocks)['train'])
    # ---- validation step | eval forward | forward half of a training step, alternated
    m.eval()
    res['step_ms'] = alternate({
        'forward_val': lambda i: eng.forward_val(img, gb, gk),
        'forward_eval': lambda i: eng.forward_eval(img),
        'train_forward_half': lambda i: eng.forward(img, gb, gk),
    }, a.steps, a.blocks)
    # ---- the loss launch alone, with and without dflat, on the buffers the last forward left
    lib = L.load()
    arch = eng.arch
    kc = K.make_loss_cfg(arch['loss_bbox'], arch['loss_cls_weight'], arch['loss_bbox_weight'], arch['loss_obj_weight'],
                         arch['loss_kps_weight'], float(arch.get('loss_bbox_eps', 1e-6)),
                         float(arch.get('loss_bbox_smooth_point', 0.1)), arch['kps_beta'], arch.get('loss_bbox_mode'))
    part = torch.empty_like(plan.loss_partials)
    dflat = torch.empty_like(plan.dflat)

    def loss_launch(with_grad):
        def fn(i):
            L.check(lib.yunet_loss_terms(K._p(plan.flat), K._p(plan.gt_inds), K._p(plan.max_overlaps), K._p(plan.gt_boxes),
                                         K._p(plan.gt_kps), C.byref(plan.levels), C.byref(kc), None, K._p(plan.norm), plan.n,
                                         plan.P, plan.gmax, K._p(dflat) if with_grad else None, K._p(part), plan.loss_blocks,
                                         K._stream()), 'yunet_loss_terms')
        return fn

    us = alternate({'with_dflat': loss_launch(True), 'value_only': loss_launch(False)}, a.launches, a.blocks)
    res['loss_launch_us'] = {k: {kk: ([x * 1e3 for x in vv] if isinstance(vv, list) else vv * 1e3) for kk, vv in v.items()}
                             for k, v in us.items()}
    # ---- a validation epoch, then the plain training step again
    with torch.no_grad():
        for i in range(a.steps):
            m.val_step(batches[i % 2], opt)
    m.train()
    train_step()
    res['train_step_ms']['after'] = alternate({'train': train_step}, a.steps, a.blocks)['train']
    res['plans'] = len(eng.plans)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: ({kk: round(vv['mean'], 4) for kk, vv in v.items()} if isinstance(v, dict) else v)
                      for k, v in res.items()}))


if __name__ == '__main__':
    main()
