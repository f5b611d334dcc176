#!/usr/bin/env python
"""Cost of ignore regions for YuNet_n 320 x 320, batch 256.

    python tools/ignore_probe.py [--iters 50] [--blocks 2] [--steps 30] [--parent DIR] [--out profiles/ignore.json]

Launches (device events over --iters launches, blocks alternating after a warm-up block):
    aug_ignore          yunet_aug_ignore on the decide's table of one batch of WIDER-sized sources, 8 ignore boxes an image
    ignore_mark         yunet_ignore_mark over that batch's padded ignore boxes (16 rows) at P = 2100
    loss / loss_flagged yunet_loss_terms_ex with flags 0 and YUNET_LOSS_IGNORE on one assignment, a third of whose
                        background priors are marked for the flagged launch
Step (forward_train + backward of the fused engine on one synthetic batch, --steps steps per block, A B B A):
    step_off / step_on  ignore_iof_thr = -1 against 0.5 with the batch's ignore boxes bound
Default step against the parent commit (only with --parent DIR, a built checkout of the parent): bench.py --gpus 1 in
fresh child processes, this tree and the parent in A B B A order; `default_vs_parent_pct` is the difference of the means.

Prints / writes one JSON object with every block's figure and the means.  Nothing here promises a time."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def alternate(fns, iters, blocks):
    for f in fns.values():
        timed(f, max(2, iters // 5))               # warm-up
    out = {k: [] for k in fns}
    for _ in range(blocks):
        for k, f in fns.items():
            out[k].append(timed(f, iters))
    return out


def launches(a, res):
    import numpy as np
    import torch
    import yunet_amd
    import yunet_amd._lib as L
    import yunet_amd.kernels as K
    import yunet_amd.synthetic as synthetic
    from yunet_amd.pipelines import DevicePipeline, SourceBatch, _ptr, _stream
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    lst = [dict(p) for p in cfg.train_pipeline]
    for p in lst:
        if p['type'] == 'Resize':
            p['img_scale'] = (a.size, a.size)
    rng = np.random.default_rng(0)
    gen = torch.Generator().manual_seed(0)
    hw = ((768, 1024), (1024, 683), (500, 375), (683, 1024))
    imgs, boxes, kps, ign = [], [], [], []
    for i in range(a.batch):
        h, w = hw[i % len(hw)]
        imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        b, _, k = synthetic.make_gt(1, h, w, gen, 64)
        boxes.append(b[0])
        kps.append(k[0])
        x1, y1 = rng.uniform(0, w - 40, 8), rng.uniform(0, h - 40, 8)
        ign.append(np.stack([x1, y1, x1 + rng.uniform(8, 120, 8), y1 + rng.uniform(8, 120, 8)], 1).astype(np.float32))
    dev = torch.device('cuda', 0)
    src = SourceBatch.from_lists(imgs, boxes, kps, dev, gt_bboxes_ignore=ign)
    pipe = DevicePipeline(lst, seed=0, ignore_rows=16)
    batch = pipe(src, 0)
    assert pipe.check() == []
    ib, ic = batch['gt_bboxes_ignore'].padded, batch['gt_bboxes_ignore'].counts
    lib = L.load()
    sizes, strides = [(a.size // s, a.size // s) for s in (8, 16, 32)], [8, 16, 32]
    lv = K.make_levels(sizes, strides)
    P = sum(h * w for h, w in sizes)
    ob, oc = torch.empty_like(ib), torch.empty_like(ic)
    # one assignment to time the loss on: crafted predictions around the batch's GT
    gb, gk, cnt = batch['gt_bboxes'].padded, batch['gt_keypointss'].padded, batch['gt_bboxes'].counts
    flat = (torch.randn(a.batch, P, 16, generator=torch.Generator().manual_seed(1)) * 0.5).to(dev)
    gi, ovl, st, _ = K.assign(flat, gb, gk, cnt, sizes, strides)
    norm = K.loss_norm(st)
    gi_marked = gi.clone()
    K.ignore_mark(gi_marked, ib, ic, sizes, strides, 0.5)
    third = (torch.rand(gi.shape, device=dev) < 1.0 / 3.0) & (gi == 0)
    gi_marked[third] = -1
    kc = K.make_loss_cfg()
    blocks_n = lib.yunet_loss_blocks(a.batch, P)
    part, dflat = torch.empty(blocks_n, 4, device=dev), torch.empty_like(flat)
    work = gi.clone()

    def aug_ignore():
        L.check(lib.yunet_aug_ignore(_ptr(pipe.params), _ptr(src.ign_boxes), _ptr(src.ign_off), a.size, a.batch, 16, _ptr(ob),
                                     _ptr(oc), _stream()), 'yunet_aug_ignore')

    def mark(thr=1.0):
        # timed at thr = 1: the same walk over every background prior and box, but nothing is marked, so every launch of a
        # block does the work of the first (a marked prior is skipped by the next launch)
        L.check(lib.yunet_ignore_mark(_ptr(ib), _ptr(ic), C.byref(lv), a.batch, P, 16, thr, _ptr(work), None, _stream()),
                'yunet_ignore_mark')

    def loss(flags, g):
        def run():
            L.check(lib.yunet_loss_terms_ex(_ptr(flat), _ptr(g), _ptr(ovl), _ptr(gb), _ptr(gk), C.byref(lv), C.byref(kc), None,
                                            flags, _ptr(norm), a.batch, P, gb.shape[1], _ptr(dflat), _ptr(part), blocks_n,
                                            _stream()), 'yunet_loss_terms_ex')
        return run
    out = alternate({'aug_ignore': aug_ignore, 'ignore_mark': mark, 'loss': loss(0, gi),
                     'loss_flagged': loss(L.LOSS_IGNORE, gi_marked)}, a.iters, a.blocks)
    res['launch_ms_blocks'] = out
    res['launch_ms'] = {k: round(sum(v) / len(v), 4) for k, v in out.items()}
    res['ignore_boxes_kept_per_image'] = round(float(ic.float().mean()), 2)
    assert int((work == -1).sum()) == 0
    mark(0.5)
    res['priors_marked_by_boxes'] = int((work == -1).sum())
    res['priors_marked_for_flagged_loss'] = int((gi_marked == -1).sum())
    return ib, ic


def steps(a, res, ib, ic):
    import torch
    import yunet_amd
    import yunet_amd.synthetic as S
    dev = torch.device('cuda', 0)
    b = S.to_device(S.make_batch(a.batch, a.size, a.size, 0), dev)
    models = {}
    for name, thr in (('step_off', -1), ('step_on', 0.5)):
        cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
        cfg.model.train_cfg.assigner['ignore_iof_thr'] = thr
        m = yunet_amd.build_detector(cfg.model)
        m.init_weights()
        models[name] = m.to(dev).train()
    from yunet_amd.pipelines import DeviceGT
    dg = DeviceGT(list(ib))
    dg.padded, dg.counts = ib, ic

    def step(name):
        def run():
            losses = models[name].forward_train(**b, gt_bboxes_ignore=dg)
            sum(losses.values()).backward()
        return run
    order = ['step_off', 'step_on', 'step_on', 'step_off']
    for n in set(order):
        timed(step(n), 5)
    out = {'step_off': [], 'step_on': []}
    for _ in range(a.blocks):
        for n in order:
            out[n].append(timed(step(n), a.steps))
    res['step_ms_blocks'] = out
    res['step_ms'] = {k: round(sum(v) / len(v), 4) for k, v in out.items()}
    res['step_on_vs_off_pct'] = round(100.0 * (res['step_ms']['step_on'] / res['step_ms']['step_off'] - 1.0), 2)
    res['marked_in_step'] = int((models['step_on'].engine.plan.gt_inds < 0).sum())


def bench_of(root, a):
    out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup', '10'], cwd=root,
                         capture_output=True, text=True, timeout=600, check=True).stdout
    row = json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1])
    return float(row.get('images_per_sec') or row.get('value') or row['throughput'])


def against_parent(a, res):
    rates = {'here': [], 'parent': []}
    for which in ('here', 'parent', 'parent', 'here'):
        rates[which].append(round(bench_of(ROOT if which == 'here' else a.parent, a), 1))
    res['bench_images_per_sec'] = rates
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    res['default_vs_parent_pct'] = round(100.0 * (mean['here'] / mean['parent'] - 1.0), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--blocks', type=int, default=2)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--bench-steps', type=int, default=60)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'what': __doc__.split('\n')[0], 'batch': a.batch, 'size': a.size, 'iters': a.iters, 'blocks': a.blocks,
           'steps': a.steps}
    if a.parent:               # first: fresh child processes, before this process holds the device
        against_parent(a, res)
    ib, ic = launches(a, res)
    steps(a, res, ib, ic)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
