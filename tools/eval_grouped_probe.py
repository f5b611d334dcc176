#!/usr/bin/env python
"""Origin-size evaluation throughput: one image per batch against batches grouped by padded canvas.

    python tools/eval_grouped_probe.py [--images N] [--batch 16] [--rounds 3] [--out profiles/eval_grouped.json]

A synthetic set with WIDER-Face val's size list (tests/golden/wider_val_sizes.npy, noise pixels), YuNet_n with the
trained fixture, through grouped_eval.run_test with cache='device', after one warm pass of each mode (decode and first
plan builds outside the window), three modes alternated a b c per round in one process:
  a  samples_per_gpu=--batch without group_by: more batch geometries than engine.MAX_PLANS, so one image per batch
     (test_pipeline.run_test as it stood before group_by existed: that file is unchanged);
  b  samples_per_gpu=1;
  c  samples_per_gpu=--batch, group_by='canvas', the default pixel cap.
Per mode: images/s per round with median and spread, batches, geometries, plan builds and evictions per pass, and
torch.cuda.max_memory_allocated; c's detections are compared with b's (np.array_equal per image).
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class SizedNoise:
    """A test-mode dataset stand-in: images of the listed (h, w), windows of one block of uint8 noise."""

    def __init__(self, hw, seed=0):
        import numpy as np
        self.np = np
        self.data_infos = [dict(filename=f'{i}.jpg', height=int(h), width=int(w)) for i, (h, w) in enumerate(hw)]
        self.block = np.random.default_rng(seed).integers(0, 256, (max(h for h, _ in hw) + 256, max(w for _, w in hw), 3),
                                                          dtype=np.uint8)

    def __len__(self):
        return len(self.data_infos)

    def load_image(self, i):
        d = self.data_infos[i]
        top = (i * 37) % 256
        return self.np.ascontiguousarray(self.block[top:top + d['height'], :d['width']])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=None, help='the first N sizes of the list (default: all)')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import yunet_amd
    from yunet_amd import grouped_eval as GE
    from yunet_amd import test_pipeline as TP
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    model = yunet_amd.build_detector(cfg.model)
    sd = torch.load(os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth'), map_location='cpu',
                    weights_only=False)['state_dict']
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    hw = [(int(h), int(w)) for h, w in np.load(os.path.join(ROOT, 'tests', 'golden', 'wider_val_sizes.npy'))]
    if a.images:
        hw = hw[:a.images]
    ds = SizedNoise(hw)
    idx = list(range(len(ds)))
    pipe = TP.DeviceTestPipeline([dict(type='MultiScaleFlipAug', scale_factor=1.0, flip=False, transforms=[
        dict(type='Resize', keep_ratio=True), dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img'])])])
    source = TP.TestSource(ds, cache='device', device=dev)
    eng = model._ensure_engine(dev)
    count = dict(builds=0, evictions=0)
    get_plan = eng.get_plan

    def counting(n, h, w, max_gt):
        had, known = len(eng.plans), any(k[:3] == (n, h, w) for k in eng.plans)
        plan = get_plan(n, h, w, max_gt)
        if not known:
            count['builds'] += 1
            count['evictions'] += had + 1 - len(eng.plans)
        return plan
    eng.get_plan = counting
    modes = dict(a=dict(samples_per_gpu=a.batch), b=dict(samples_per_gpu=1),
                 c=dict(samples_per_gpu=a.batch, group_by='canvas'))
    said, stats, dets = [], {}, {}

    def one(name):
        count.update(builds=0, evictions=0)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        with torch.no_grad():
            out = GE.run_test(model, ds, dev, idx, pipe, source, log=said.append, **modes[name])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        dets[name] = out
        return dict(seconds=round(dt, 3), images_per_s=round(len(idx) / dt, 1), plan_builds=count['builds'],
                    plan_evictions=count['evictions'], max_memory_allocated=int(torch.cuda.max_memory_allocated(dev)))

    for name in modes:                      # the warm pass: decode into the store, first plan builds
        w = one(name)
        print(f'warm {name}: {w}', file=sys.stderr, flush=True)
        stats[name] = dict(warm_pass=w, rounds=[])
    for r in range(a.rounds):
        for name in modes:
            stats[name]['rounds'].append(one(name))
            print(f'round {r} {name}: {stats[name]["rounds"][-1]}', file=sys.stderr, flush=True)
    info = {i: ds.data_infos[i] for i in idx}
    sizes = {i: (info[i]['height'], info[i]['width']) for i in idx}
    for name, kw in modes.items():
        batches = GE.plan_batches(pipe, sizes, idx, log=None, **kw)
        rates = sorted(x['images_per_s'] for x in stats[name]['rounds'])
        stats[name].update(options=kw, batches=len(batches),
                           geometries=len({(len(b),) + pipe.canvas([sizes[i] for i in b]) for b in batches}),
                           images_per_s_median=rates[len(rates) // 2], images_per_s_min=rates[0], images_per_s_max=rates[-1])
    equal = sum(1 for x, y in zip(dets['b'], dets['c']) if x[0].shape == y[0].shape and np.array_equal(x[0], y[0]))
    res = dict(what='origin-size evaluation of a WIDER-val-sized synthetic set: a = samples_per_gpu=B without group_by (the '
                    'one-image fallback), b = samples_per_gpu=1, c = group_by=canvas at B with the default pixel cap',
               tool='tools/eval_grouped_probe.py ' + ' '.join(sys.argv[1:]), device=torch.cuda.get_device_name(0),
               images=len(idx), batch=a.batch, rounds=a.rounds, order='a b c per round, after one warm pass each',
               max_plans=__import__('yunet_amd.engine', fromlist=['MAX_PLANS']).MAX_PLANS, fallback_lines=len(said),
               detections=int(sum(x[0].shape[0] for x in dets['b'])), images_c_equal_to_b=equal, modes=stats,
               timing='wall clock (perf_counter) between device synchronisations around run_test, decoded sources '
                      "resident (cache='device'); a runs on this tree, not on a checkout of the parent commit")
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
