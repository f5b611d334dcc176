#!/usr/bin/env python
"""Pixel-pass time of the device train pipeline with PhotoMetricDistortion absent (NONE), after RandomFlip (POST) and
before RandomSquareCrop (PRE): one 256-image batch of WIDER-sized decoded sources (SyntheticSourceImages' default
sizes) to 320 x 320, the same batch and iterations for the three lists.

    python tools/photometric_probe.py [--iters 20] [--out probe.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o probe -- python tools/photometric_probe.py     # per-kernel times

Prints one JSON object: per list the mean event time of a whole DevicePipeline call (aug_decide + [photometric table]
+ pixel pass) over --iters calls after 3 warm-up calls."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import yunet_amd
    import yunet_amd.synthetic as synthetic
    from yunet_amd.pipelines import DevicePipeline, SourceBatch
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    base = [dict(p) for p in cfg.train_pipeline]
    for p in base:
        if p['type'] == 'Resize':
            p['img_scale'] = (a.size, a.size)
    lists = {'none': base,
             'post': base[:5] + [dict(type='PhotoMetricDistortion')] + base[5:],
             'pre': base[:2] + [dict(type='PhotoMetricDistortion')] + base[2:]}
    rng = np.random.default_rng(0)
    gen = torch.Generator().manual_seed(0)
    hw = ((768, 1024), (1024, 683), (500, 375), (683, 1024))
    imgs, boxes, kps = [], [], []
    for i in range(a.batch):
        h, w = hw[i % len(hw)]
        imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        b, _, k = synthetic.make_gt(1, h, w, gen, 64)
        boxes.append(b[0])
        kps.append(k[0])
    dev = torch.device('cuda', 0)
    src = SourceBatch.from_lists(imgs, boxes, kps, dev)
    res = {'what': __doc__.split('\n')[0], 'batch': a.batch, 'size': a.size, 'iters': a.iters, 'pipeline_ms': {}}
    for name, lst in lists.items():
        pipe = DevicePipeline(lst, seed=0)
        for it in range(3):
            pipe(src, it)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(a.iters):
            pipe(src, 3 + it)
        e1.record()
        torch.cuda.synchronize()
        assert pipe.check() == []
        res['pipeline_ms'][name] = round(e0.elapsed_time(e1) / a.iters, 4)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
