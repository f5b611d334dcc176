#!/usr/bin/env python
"""Cost of CutOut in the device train pipeline (YuNet_n 320 x 320, batch 256, resident sources).

The pixel pass alone against the pixel pass plus the yunet_aug_cutout launch, and the tools/train.py rate without and
with the transform.

    python tools/cutout_probe.py [--iters 50] [--blocks 3] [--train-iters 100] [--out profiles/cutout.json]

The transform: CutOut(n_holes=(0, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.2)]) in front of Normalize.

Launches.  One batch of WIDER-sized decoded sources (SyntheticSourceImages' default sizes) goes through DevicePipeline
once, so that the decide's table and the pixel pass's descriptor exist; then yunet_aug_pixels alone (`pixels`) and
yunet_aug_pixels + yunet_aug_cutout (`pixels_cutout`) are timed with device events over --iters launches, in
alternating blocks (--blocks of each) after a warm-up block of both.

Training.  tools/train.py on configs/yunet_n.py with resident SyntheticSourceImages, --train-iters iterations per run,
without (`none`) and with (`cutout`) the transform, alternating, --blocks runs of each in this one process; the rate is
the batch over the runner's time per iteration with the first logging interval (start-up) left out.

Prints / writes one JSON object with every block's figure and the means."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CUTOUT = dict(type='CutOut', n_holes=(0, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.2)])


def launches(a, res):
    import numpy as np
    import torch
    import yunet_amd
    import yunet_amd._lib as L
    import yunet_amd.synthetic as synthetic
    from yunet_amd.pipelines import DevicePipeline, SourceBatch
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    lst = [dict(p) for p in cfg.train_pipeline]
    for p in lst:
        if p['type'] == 'Resize':
            p['img_scale'] = (a.size, a.size)
    lst.insert([p['type'] for p in lst].index('Normalize'), dict(CUTOUT))
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
    pipe = DevicePipeline(lst, seed=0)
    img = pipe(src, 0)['img']
    assert pipe.check() == []
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = C.c_void_p(img.data_ptr())

    def block(with_cutout, it0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(a.iters):
            L.check(lib.yunet_aug_pixels(C.byref(pipe._pixels), C.byref(pipe.cfg), a.batch, ptr, stream), 'pixels')
            if with_cutout:
                pipe._cutout(img, None, it0 + it, dev)
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / a.iters, 4)
    block(False, 0), block(True, 0)           # warm-up
    out = {'pixels': [], 'pixels_cutout': []}
    for b in range(a.blocks):
        out['pixels'].append(block(False, 0))
        out['pixels_cutout'].append(block(True, 1000 * b))
    table = pipe.cutout_holes.cpu().numpy()
    res['launch_ms_blocks'] = out
    res['launch_ms'] = {k: round(sum(v) / len(v), 4) for k, v in out.items()}
    res['launch_ms']['cutout_added'] = round(res['launch_ms']['pixels_cutout'] - res['launch_ms']['pixels'], 4)
    res['holes_in_last_batch'] = int(table[:, 0].sum())
    res['hole_pixels_in_last_batch'] = int(sum((r[4 + 4 * j] - r[2 + 4 * j]) * (r[5 + 4 * j] - r[3 + 4 * j])
                                               for r in table for j in range(r[0])))


def training(a, res):
    import torch
    import yunet_amd
    spec = importlib.util.spec_from_file_location('yunet_train_tool', os.path.join(ROOT, 'tools', 'train.py'))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    base = open(os.path.join(ROOT, 'configs', 'yunet_n.py')).read()
    edits = {'none': '', 'cutout': f"\ntrain_pipeline.insert([p['type'] for p in train_pipeline].index('Normalize'), {CUTOUT!r})\n"}
    fixture = os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth')
    out = {'none': [], 'cutout': []}
    with tempfile.TemporaryDirectory() as tmp:
        for b in range(a.blocks):
            for name in ('none', 'cutout'):
                config = os.path.join(tmp, f'yunet_n_{name}.py')
                with open(config, 'w') as f:
                    f.write(base + edits[name])
                interval = max(1, a.train_iters // 4)
                hist = T.main([config, '--work-dir', os.path.join(tmp, f'w_{name}_{b}'), '--max-iters', str(a.train_iters),
                               '--no-validate', '--seed', '0', '--cfg-options', f'log_config.interval={interval}',
                               f'load_from={fixture}', 'data.train.type=SyntheticSourceImages',
                               f'data.samples_per_gpu={a.batch}'])
                torch.cuda.synchronize()
                assert (T.main.last_source.pipe.cutout is not None) == (name == 'cutout')
                rows = [r for r in hist if 'time' in r]
                steady = rows[1:] if len(rows) > 1 else rows
                t = sum(r['time'] for r in steady) / len(steady)
                bs = yunet_amd.Config.fromfile(config).data.samples_per_gpu
                out[name].append({'ms_per_iter': round(1000 * t, 3), 'images_per_sec': round(bs / t, 1),
                                  'final_loss': round(float(rows[-1]['loss']), 4)})
                T.main.last_source = None
                torch.cuda.empty_cache()
    res['train_blocks'] = out
    res['train_images_per_sec'] = {k: round(sum(r['images_per_sec'] for r in v) / len(v), 1) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--train-iters', type=int, default=100)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'what': __doc__.split('\n')[0], 'transform': repr(CUTOUT), 'batch': a.batch, 'size': a.size, 'iters': a.iters,
           'blocks': a.blocks, 'train_iters': a.train_iters}
    launches(a, res)
    if a.train_iters > 0:
        training(a, res)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
