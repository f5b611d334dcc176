#!/usr/bin/env python
"""What wider padded GT rows cost (needs a GPU; reads nothing outside the repository).

    tools/gt_capacity_probe.py --out profiles/gt_capacity.json [--kind n --size 320 --batch 256 --steps 20]

RetinaFaceSource(gt_capacity=...) pads every crop's GT to one width for the whole run: 64 rows by default, up to 4096.  This
probe pads THE SAME ground truth (a synthetic batch whose images carry at most 64 faces) to 64, 512, 2048 and 4096 rows
and measures, in one process:

* the whole training step (forward, backward, SGD) per width, alternated 64 / wide / wide / 64 for each wide width, every
  block `--warmup` untimed + `--steps` timed steps between two events.  The yardstick of a width is the mean of the two
  64-row blocks of its own alternation; `ratio` is wide / that.
* per width, `--steps` back-to-back calls between two events of: the decide launch (DevicePipeline._decide on 256 decoded
  synthetic sources), yunet_assign_cfg (its three launches together: compact, top-k, resolve) and the loss launch
  (yunet_loss_terms + finalize), each with its host-side issue -- and which assign path ran: the pair-list launches for
  Gmax < P, the one-workgroup-per-image launches otherwise.
* the same step and launches for one crowded batch (eight images with 65 .. 1968 faces among the 256) at 2048 and 4096 rows.

No threshold: the numbers are the result (DESIGN.md records what was decided from them).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import yunet_amd  # noqa: E402
import yunet_amd.kernels as K  # noqa: E402
import yunet_amd.synthetic as S  # noqa: E402
from yunet_amd.optim import FusedSGD  # noqa: E402

WIDTHS = (64, 512, 2048, 4096)
CROWD = (1968, 1024, 709, 512, 300, 178, 128, 65)


def padded_batch(batch, rows, dev):
    """The batch with its GT padded to `rows` rows, on the device (img shared)."""
    out = dict(batch)
    out['gt_labels'] = [torch.zeros(int(t.shape[0]), dtype=torch.int64, device=dev) for t in batch['gt_bboxes']]
    for key, tail in (('gt_bboxes', (4,)), ('gt_keypointss', (5, 3))):
        lst = S.GTList([t.to(dev) for t in batch[key]])
        pad, cnt = S._pad(list(batch[key]), tail, rows)
        lst.padded, lst.counts = pad.to(dev), cnt.to(dev)
        out[key] = lst
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--kind', default='n')
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args(argv)
    import crafted as C
    import pipeline_oracle as P
    import yunet_oracle as O
    from yunet_amd.pipelines import DevicePipeline, SourceBatch
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{a.kind}.py'))
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(O.init_state(O.yunet_arch(a.kind), seed=1), strict=True)
    m.to(dev).train()
    opt = FusedSGD(m, lr=1e-5, momentum=0.9, weight_decay=5e-4)
    h = w = a.size
    sizes = C.featmap_sizes(h, w)
    n_priors = sum(x * y for x, y in sizes)
    host = S.make_batch(a.batch, h, w, 1234)
    host['img'] = host['img'].to(dev)
    assert max(int(b.shape[0]) for b in host['gt_bboxes']) <= 64
    crowd = dict(host)
    cb, _, ck = C.crowded_gt(list(CROWD), h, w, 77)
    crowd['gt_bboxes'] = list(cb) + list(host['gt_bboxes'][len(CROWD):])
    crowd['gt_keypointss'] = list(ck) + list(host['gt_keypointss'][len(CROWD):])

    def between_events(fn, reps, warm):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def step_ms(batch):
        def step():
            out = m.train_step(batch, opt)
            opt.zero_grad()
            out['loss'].backward()
            opt.step()
        return between_events(step, a.steps, a.warmup)

    def launches(batch, flat):
        gb, gk, cnt = batch['gt_bboxes'].padded, batch['gt_keypointss'].padded, batch['gt_bboxes'].counts
        gi, ovl, st, _ = K.assign(flat, gb, gk, cnt, sizes, [8, 16, 32])
        lcfg = K.make_loss_cfg('EIoULoss')
        return dict(
            assign_ms=round(between_events(lambda: K.assign(flat, gb, gk, cnt, sizes, [8, 16, 32]), a.steps, a.warmup), 4),
            loss_ms=round(between_events(lambda: K.loss(flat, gi, ovl, gb, gk, st, sizes, [8, 16, 32], lcfg), a.steps, a.warmup), 4),
            assign_path='pair-list' if gb.shape[1] < n_priors else 'per-image')

    # the decide launch: 256 decoded sources with at most 64 faces each, the reference pipeline at the probe's size
    rng = np.random.default_rng(3)
    srcs = [P.synth_image(rng, 240, 320, int(rng.integers(1, 65))) for _ in range(a.batch)]
    sb = SourceBatch.from_lists([s[0] for s in srcs], [s[1] for s in srcs], [s[2] for s in srcs], dev)
    pipeline = [dict(p) for p in cfg.train_pipeline]
    pipeline[3]['img_scale'] = (a.size, a.size)

    def decide_ms(rows):
        pipe = DevicePipeline(pipeline, seed=0, gmax=rows)
        return round(between_events(lambda: pipe._decide(sb, 0, dev), a.steps, a.warmup), 4)

    res = dict(model=f'yunet_{a.kind}', size=a.size, batch=a.batch, priors=n_priors, steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), widths={}, crowded={})
    batches = {rows: padded_batch(host, rows, dev) for rows in WIDTHS}
    flat = C.crafted_preds(host['gt_bboxes'], host['gt_keypointss'], h, w, 5).to(dev).contiguous()
    for rows in WIDTHS[1:]:
        order = [64, rows, rows, 64]
        t = [step_ms(batches[r]) for r in order]
        base, wide = (t[0] + t[3]) / 2, (t[1] + t[2]) / 2
        res['widths'][str(rows)] = dict(order=order, ms_per_step=[round(x, 4) for x in t], rows64_ms=round(base, 4),
                                        step_ms=round(wide, 4), ratio=round(wide / base, 4), decide_ms=decide_ms(rows),
                                        **launches(batches[rows], flat))
    res['widths']['64'] = dict(step_ms=round(float(np.mean([v['rows64_ms'] for v in res['widths'].values()])), 4),
                               decide_ms=decide_ms(64), **launches(batches[64], flat))
    cflat = C.crafted_preds(crowd['gt_bboxes'], crowd['gt_keypointss'], h, w, 6).to(dev).contiguous()
    for rows in (2048, 4096):
        b = padded_batch(crowd, rows, dev)
        res['crowded'][str(rows)] = dict(counts=list(CROWD), step_ms=round(step_ms(b), 4), **launches(b, cflat))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
