#!/usr/bin/env python
"""End-to-end images/s of tools/train.py: the reference's command line, 200 iterations of
configs/yunet_n.py (YuNet_n 320 x 320, 256 images per GPU) from three data sources, next to the step bench.py times:

  ready     SyntheticWiderFace      finished fp32 batches resident in HBM (what bench.py feeds: the step alone + the runner's
                                    hooks, LR schedule, logging)
  resident  SyntheticSourceImages   decoded uint8 sources resident in HBM, the reference's train pipeline (RandomSquareCrop ->
                                    Resize -> RandomFlip -> Normalize -> collate) on the GPU every iteration
  host_fed  SyntheticSourceImages   the same sources in PINNED HOST memory, each batch uploaded on a copy stream into one of
            (host_fed=True)         two device buffers while the previous step runs
  host_window SyntheticSourceImages   the same pinned sources as a host SourceStore: per batch only each image's crop-window
            (host_fed='window')     rectangle travels (2D copies on a copy stream, planned two iterations ahead)
  host_window_kernel                the same windows read by the GPU itself from the pinned store (yunet_fetch_windows on
            (+ host_fetch=kernel)   the copy stream, plan from device memory, no host wait)

    python tools/train_e2e.py [--iters 200] [--out profiles/r06_train_e2e.json] [--photometric pre|post]
                              [--multiscale LO,HI | --size S] [--samples-per-gpu N]

--photometric inserts the reference's PhotoMetricDistortion (default arguments) into the config's train_pipeline, before
RandomSquareCrop (pre) or after RandomFlip (post); the modes other than `ready` then run it in the pixel pass.

--multiscale LO,HI rewrites the config's Resize entry to Resize(img_scale=(LO, HI), multiscale_mode='square_range',
keep_ratio=False) (multi-scale training: the batch geometry changes from step to step); --size S to the fixed
img_scale=(S, S); --samples-per-gpu N sets data.samples_per_gpu.  `ready` feeds finished batches and ignores the pipeline.

Prints / writes one JSON object: per mode images/s over the last three logging intervals (150 iterations), the runner's
time per iteration, and the source's own events (upload ms / GB/s, pipeline ms).  Weights: the trained fixture
(tests/golden/yunet_n_synth_trained.pth) so that SimOTA works as in bench.py."""
import argparse
import importlib.util
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_train_tool():
    spec = importlib.util.spec_from_file_location('yunet_train_tool', os.path.join(ROOT, 'tools', 'train.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--config', default=os.path.join(ROOT, 'configs', 'yunet_n.py'))
    ap.add_argument('--out', default=None)
    ap.add_argument('--modes', default=None,
                    help='comma-separated subset of ready,resident,host_fed,host_window,host_window_kernel')
    ap.add_argument('--photometric', choices=('pre', 'post'), default=None)
    ap.add_argument('--multiscale', default=None, metavar='LO,HI')
    ap.add_argument('--size', type=int, default=None)
    ap.add_argument('--mosaic', type=int, default=None, metavar='S',
                    help="Mosaic(img_scale=(S, S), use_kps=True) in front of RandomSquareCrop (resident mode only)")
    ap.add_argument('--samples-per-gpu', type=int, default=None)
    a = ap.parse_args()
    if a.multiscale and a.size:
        ap.error('--multiscale and --size both rewrite the Resize entry')
    import torch
    T = load_train_tool()
    config = a.config
    edits = []
    if a.multiscale or a.size:
        lo, hi = [int(v) for v in a.multiscale.split(',')] if a.multiscale else (a.size, a.size)
        resize = (f"dict(type='Resize', img_scale=({lo}, {hi}), multiscale_mode='square_range', keep_ratio=False)"
                  if a.multiscale else f"dict(type='Resize', img_scale=({lo}, {hi}), keep_ratio=False)")
        edits.append(f"train_pipeline[[p['type'] for p in train_pipeline].index('Resize')] = {resize}")
    if a.photometric:
        at = {'pre': 2, 'post': 5}[a.photometric]
        edits.append(f"train_pipeline.insert({at}, dict(type='PhotoMetricDistortion'))")
    if a.mosaic:
        edits.append(f"train_pipeline.insert(2, dict(type='Mosaic', img_scale=({a.mosaic}, {a.mosaic}), use_kps=True))")
    if a.samples_per_gpu:
        edits.append(f"data['samples_per_gpu'] = {a.samples_per_gpu}")
    if edits:
        tmp = tempfile.NamedTemporaryFile('w', suffix='.py', delete=False)
        tmp.write(open(a.config).read() + '\n' + '\n'.join(edits) + '\n')
        tmp.close()
        config = tmp.name
    fixture = os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth')
    modes = [('ready', ['data.train.type=SyntheticWiderFace', 'data.train.resident=2']),
             ('resident', ['data.train.type=SyntheticSourceImages', 'data.train.timing=True']),
             ('host_fed', ['data.train.type=SyntheticSourceImages', 'data.train.timing=True', 'data.train.host_fed=True']),
             ('host_window', ['data.train.type=SyntheticSourceImages', 'data.train.timing=True',
                              'data.train.host_fed=window']),
             ('host_window_kernel', ['data.train.type=SyntheticSourceImages', 'data.train.timing=True',
                                     'data.train.host_fed=window', 'data.train.host_fetch=kernel'])]
    if a.modes:
        modes = [m for m in modes if m[0] in a.modes.split(',')]
    res = {'what': __doc__.split('\n')[0], 'config': os.path.basename(a.config), 'iters': a.iters,
           'photometric': a.photometric, 'multiscale': a.multiscale, 'size': a.size, 'mosaic': a.mosaic, 'modes': {}}
    for name, opts in modes:
        with tempfile.TemporaryDirectory() as wd:
            argv = [config, '--work-dir', wd, '--max-iters', str(a.iters), '--no-validate', '--seed', '0',
                    '--cfg-options', 'log_config.interval=50', f'load_from={fixture}'] + opts
            hist = T.main(argv)
            torch.cuda.synchronize()
        rows = [r for r in hist if 'time' in r]
        bs = None
        import yunet_amd
        bs = yunet_amd.Config.fromfile(config).data.samples_per_gpu
        steady = rows[1:] if len(rows) > 1 else rows          # the first interval holds start-up (plan build, first launches)
        t = sum(r['time'] for r in steady) / len(steady)
        m = {'ms_per_iter': round(1000 * t, 3), 'images_per_sec': round(bs / t, 1), 'batch': bs,
             'intervals_ms_per_iter': [round(1000 * r['time'], 3) for r in rows],
             'final_loss': round(float(rows[-1]['loss']), 4)}
        src = getattr(T.main, 'last_source', None)
        if src is not None and hasattr(src, 'report'):
            m['source_events'] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in src.report().items()}
        res['modes'][name] = m
        print(name, json.dumps(m), flush=True)
        del src
        T.main.last_source = None
        torch.cuda.empty_cache()
    if config != a.config:
        os.unlink(config)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
