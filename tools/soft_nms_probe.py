#!/usr/bin/env python
"""What Soft-NMS costs next to greedy NMS in kernels.detect (needs a GPU).

    tools/soft_nms_probe.py --out profiles/soft_nms.json [--size 640 --crowd 2400 --blocks 7 --launches 200]

One image per launch (one workgroup), two inputs at P = 8400 (640 x 640):
  * head     the head outputs of YuNet_n with the trained fixture weights on a structured synthetic image;
  * crowded  synthetic head outputs with about 2000 priors above score_thr (`--crowd` draws, runs of eight neighbouring
             priors that may coincide), boxes four strides wide so that neighbours overlap -- a crowded WIDER-Face image.
Candidates: greedy NMS (iou 0.45, the default test_cfg) and Soft-NMS naive / linear / gaussian (mmcv's defaults:
iou_threshold 0.3, sigma 0.5, min_score 1e-3).  All candidates run warm launches first; then they alternate in blocks of
`--launches` launches between two device events, `--blocks` times round; a candidate's time is the MEDIAN of its block
means (min and max beside it).  The numpy restatement's host time (tests/soft_nms_ref.py, on the decoded candidates,
best of three) stands beside them for context; it is not a baseline anybody ships.
No threshold: nobody had measured this kernel; the file records what it costs.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

STRIDES = [8, 16, 32]
SCORE_THR = 0.02
SOFT = dict(iou_thr=0.3, sigma=0.5, min_score=1e-3)


def crowded_flat(sizes, crowd, seed):
    """[1, P, 16] head outputs: `crowd` priors of the stride-8 level, in contiguous runs, with scores well above the
    threshold and boxes about four strides wide (so that each overlaps its neighbours); everything else far below it."""
    import torch
    g = torch.Generator().manual_seed(seed)
    P = sum(h * w for h, w in sizes)
    flat = torch.randn(1, P, 16, generator=g) * 0.3
    flat[..., 0] -= 6.0
    flat[..., 5] -= 6.0
    n0 = sizes[0][0] * sizes[0][1]
    start = torch.randint(0, n0 - 8, (crowd // 8,), generator=g)
    idx = torch.unique((start[:, None] + torch.arange(8)[None]).reshape(-1))
    k = idx.numel()
    flat[0, idx, 0] = 0.5 + torch.randn(k, generator=g)
    flat[0, idx, 5] = 0.5 + torch.randn(k, generator=g)
    flat[0, idx, 3:5] = 1.4 + 0.3 * torch.randn(k, 2, generator=g)
    return flat.contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--crowd', type=int, default=2400)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--warm', type=int, default=20)
    a = ap.parse_args(argv)
    import torch

    import soft_nms_ref as R
    import yunet_amd
    import yunet_amd.kernels as K
    import yunet_amd.synthetic as S
    import yunet_oracle as O
    if not torch.cuda.is_available():
        raise SystemExit('soft_nms_probe needs a GPU: no time is reported without one')
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    m = yunet_amd.build_detector(cfg.model)
    ck = torch.load(os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth'), map_location='cpu', weights_only=False)
    m.load_state_dict(ck['state_dict'], strict=True)
    m.to(dev).eval()
    img = S.make_batch(1, a.size, a.size, 31, structured=True)['img'].to(dev).float().contiguous()
    eng = m._ensure_engine(dev)
    head = eng.forward_eval(img).clone()                # (the eval plan of this geometry exists from here on)
    sizes = [tuple(s) for s in eng.plan.sizes]
    inputs = {'head': head, 'crowded': crowded_flat(sizes, a.crowd, 7).to(dev)}

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n            # microseconds per call

    res = dict(device=torch.cuda.get_device_name(0), size=a.size, P=int(inputs['head'].shape[1]), score_thr=SCORE_THR,
               blocks=a.blocks, launches_per_block=a.launches, warm=a.warm, soft=SOFT, unit='us per kernels.detect call',
               inputs={})
    for name, flat in inputs.items():
        cands = {'greedy': lambda f=flat: K.detect(f, sizes, STRIDES, SCORE_THR, 0.45)}
        for method in ('naive', 'linear', 'gaussian'):
            cands['soft_' + method] = lambda f=flat, mt=method: K.detect(f, sizes, STRIDES, SCORE_THR, soft=dict(SOFT, method=mt))
        for fn in cands.values():
            timed(fn, a.warm)
        rows = {k: [] for k in cands}
        for _ in range(a.blocks):
            for k, fn in cands.items():
                rows[k].append(timed(fn, a.launches))
        entry = dict(candidates=int((flat[0, :, 0].sigmoid() * flat[0, :, 5].sigmoid() >= SCORE_THR).sum()), detect_us={},
                     survivors={}, numpy_restatement_ms={})
        for k, fn in cands.items():
            entry['detect_us'][k] = dict(median=statistics.median(rows[k]), min=min(rows[k]), max=max(rows[k]))
            entry['survivors'][k] = int(fn()[2][0])
        # the restatement on the host, for context: decoded candidates -> live-set form in fp32
        f = flat.cpu()
        pri = O.grid_priors(sizes, STRIDES)
        boxes = O.bbox_decode(pri, f[0, :, 1:5]).numpy()
        scores = (f[0, :, 0].sigmoid() * f[0, :, 5].sigmoid()).numpy()
        for method in ('naive', 'linear', 'gaussian'):
            best = float('inf')
            for _ in range(3):
                t0 = time.perf_counter()
                keep, _ = R.soft_nms_live(boxes, scores, method=method, score_thr=SCORE_THR, **SOFT)
                best = min(best, time.perf_counter() - t0)
            entry['numpy_restatement_ms'][method] = best * 1e3
            entry['survivors']['numpy_' + method] = int(len(keep))
        res['inputs'][name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({n: dict(candidates=e['candidates'], survivors=e['survivors'],
                              detect_us={k: round(v['median'], 1) for k, v in e['detect_us'].items()},
                              numpy_ms={k: round(v, 1) for k, v in e['numpy_restatement_ms'].items()})
                      for n, e in res['inputs'].items()}))


if __name__ == '__main__':
    main()
