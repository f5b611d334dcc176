#!/usr/bin/env python
"""Cost of MixUp in the device train pipeline (YuNet_n 320 x 320, batch 256, resident sources).

The two launches alone with their algorithmic bytes, the tools/train.py rate without and with the step, and -- given a
built checkout of the parent commit -- bench.py on the default list in both trees.

    python tools/mixup_probe.py [--iters 50] [--blocks 3] [--train-iters 100] [--parent DIR] [--out profiles/mixup.json]

The step: MixUp(img_scale=(size, size), use_kps=True) with the reference's defaults, in front of Normalize.

Launches.  One batch of WIDER-sized decoded sources (SyntheticSourceImages' default sizes) goes through DevicePipeline
once, so that the batch tensor and the padded GT exist; then yunet_aug_pixels alone (`pixels`, the figure every other
launch of the pipeline is reported next to), yunet_aug_mixup_decide alone and yunet_aug_mixup_pixels alone are timed
with device events over --iters launches, in alternating blocks (--blocks of each) after a warm-up block.  Algorithmic
bytes: the decide reads and writes the padded GT once (19 floats a row) and writes 18 doubles per image; the pixel
launch reads and writes every value of the batch tensor once (2 x N x 3 x E x E floats; the partner's uint8 taps, up to
16 source pixels per output pixel and mostly cache hits, are not counted).

Training.  tools/train.py on configs/yunet_n.py with resident SyntheticSourceImages, --train-iters iterations per run,
without (`none`) and with (`mixup`) the step, alternating, --blocks runs of each in this one process; the rate is the
batch over the runner's time per iteration with the first logging interval (start-up) left out.

Default list.  --parent DIR names a built checkout of the parent commit: `bench.py --gpus 1 --steps 40 --warmup 10` runs
as a child process in this tree (A) and in that one (B) in the order A B B A; its op lists are the same in both, so the
difference is expected inside the session spread.

Prints / writes one JSON object with every block's figure and the means."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIXUP = dict(type='MixUp', use_kps=True)          # img_scale follows --size


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
    plain = [dict(p) for p in lst]
    lst.insert([p['type'] for p in lst].index('Normalize'), dict(MIXUP, img_scale=(a.size, a.size)))
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
    pipe, base = DevicePipeline(lst, seed=0), DevicePipeline(plain, seed=0)
    base(src, 0)                    # `pixels` below is this list's pixel pass
    # the batch tensor and the GT the step is given, at the step's own capacity (MixUp doubles the padded rows, and the
    # entries take the row count from the configuration): the list with the step switched off
    pipe.update_skip_type_keys(('MixUp',))
    before = pipe(src, 0)
    pipe.update_skip_type_keys(())
    after = pipe(src, 0)
    assert pipe.check() == []
    img, gb, gk, cnt = before['img'], before['gt_bboxes'].padded, before['gt_keypointss'].padded, before['gt_bboxes'].counts
    lib, c = L.load(), pipe.mixup_cfg
    assert gb.shape[1] == gk.shape[1] == c.gmax and gb.is_contiguous() and gk.is_contiguous()
    view, _ = src.store_view()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, edge = a.batch, a.size
    table = torch.empty(n, L.MIXUP_WORDS, device=dev, dtype=torch.float64)
    ob, ok, oc, out = torch.empty_like(gb), torch.empty_like(gk), torch.empty_like(cnt), img.clone()
    scratch = torch.empty_like(img)

    def p(t):
        return C.c_void_p(t.data_ptr())

    def one(which, it):
        if which == 'pixels':
            L.check(lib.yunet_aug_pixels(C.byref(base._pixels), C.byref(base.cfg), n, p(scratch), stream), 'pixels')
        elif which == 'mixup_decide':
            L.check(lib.yunet_aug_mixup_decide(C.byref(c), it, n, edge, None, view.m, p(view.hw), p(view.goff), p(view.gcnt),
                                               p(view.boxes), p(view.kps), p(gb), p(gk), p(cnt), p(ob), p(ok), p(oc), p(table),
                                               stream), 'mixup_decide')
        else:           # in place: every launch blends the buffer again, the work per launch is the same
            L.check(lib.yunet_aug_mixup_pixels(p(table), c.img_scale, c.pad_val, n, edge, None, view.m, p(src.src), p(view.off),
                                               p(view.hw), p(out), stream), 'mixup_pixels')

    def block(which, it0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(a.iters):
            one(which, it0 + it)
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / a.iters, 4)
    names = ('pixels', 'mixup_decide', 'mixup_pixels')
    for w in names:
        block(w, 0)                 # warm-up
    blocks = {w: [] for w in names}
    for b in range(a.blocks):
        for w in names:
            blocks[w].append(block(w, 1000 * b))
    gmax = int(gb.shape[1])
    nbytes = {'mixup_decide': 2 * n * gmax * 19 * 4 + n * 4 * 2 + n * L.MIXUP_WORDS * 8,
              'mixup_pixels': 2 * n * 3 * edge * edge * 4 + n * L.MIXUP_WORDS * 8}
    res['launch_ms_blocks'] = blocks
    res['launch_ms'] = {k: round(sum(v) / len(v), 4) for k, v in blocks.items()}
    res['launch_ms']['mixup_added'] = round(res['launch_ms']['mixup_decide'] + res['launch_ms']['mixup_pixels'], 4)
    res['algorithmic_bytes'] = nbytes
    res['algorithmic_gb_per_s'] = {k: round(v / (res['launch_ms'][k] * 1e-3) / 1e9, 1) for k, v in nbytes.items()}
    res['gt_rows_per_image'] = gmax
    res['rows_in_last_batch'] = {'before': int(cnt.sum()), 'after': int(after['gt_bboxes'].counts.sum())}


def training(a, res):
    import torch
    import yunet_amd
    spec = importlib.util.spec_from_file_location('yunet_train_tool', os.path.join(ROOT, 'tools', 'train.py'))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    base = open(os.path.join(ROOT, 'configs', 'yunet_n.py')).read()
    step = dict(MIXUP, img_scale=(a.size, a.size))
    edits = {'none': '', 'mixup': f"\ntrain_pipeline.insert([p['type'] for p in train_pipeline].index('Normalize'), {step!r})\n"}
    fixture = os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth')
    out = {'none': [], 'mixup': []}
    with tempfile.TemporaryDirectory() as tmp:
        for b in range(a.blocks):
            for name in ('none', 'mixup'):
                config = os.path.join(tmp, f'yunet_n_{name}.py')
                with open(config, 'w') as f:
                    f.write(base + edits[name])
                interval = max(1, a.train_iters // 4)
                hist = T.main([config, '--work-dir', os.path.join(tmp, f'w_{name}_{b}'), '--max-iters', str(a.train_iters),
                               '--no-validate', '--seed', '0', '--cfg-options', f'log_config.interval={interval}',
                               f'load_from={fixture}', 'data.train.type=SyntheticSourceImages',
                               f'data.samples_per_gpu={a.batch}'])
                torch.cuda.synchronize()
                assert (T.main.last_source.pipe.mixup is not None) == (name == 'mixup')
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


def default_list(a, res):
    """bench.py in this tree (A) and in the parent's (B), A B B A, each run a child process of its own."""
    runs = []
    for name, tree in (('this', ROOT), ('parent', a.parent), ('parent', a.parent), ('this', ROOT)):
        line = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '40', '--warmup', '10'],
                              cwd=tree, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
        r = json.loads(line)
        runs.append({'tree': name, **{k: r[k] for k in ('value', 'unit', 'ms_per_step', 'final_loss') if k in r}})
    res['default_list_abba'] = runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--train-iters', type=int, default=100)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'what': __doc__.split('\n')[0], 'transform': repr(dict(MIXUP, img_scale=(a.size, a.size))), 'batch': a.batch,
           'size': a.size, 'iters': a.iters,
           'blocks': a.blocks, 'train_iters': a.train_iters}
    if a.parent:
        a.parent = os.path.abspath(a.parent)        # the children run with the tree as their working directory
    if a.parent:        # first: the child processes run while this one holds no device memory
        default_list(a, res)
    launches(a, res)
    if a.train_iters > 0:
        training(a, res)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
