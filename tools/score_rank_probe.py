#!/usr/bin/env python
"""The mAP protocol with the ranking on the device (eval_map_single_class(device='cuda', rank='device')) against the
two paths tools/score_probe.py times (host; device='cuda' with the ranking on the host), on that tool's synthetic set
with WIDER val's shape and at its two prediction densities.  Whole calls, wall clock between device synchronisations,
the three paths alternating A B C C B A after a warm-up; the kernels of the device ranking alone with device events.

The synthetic scores are float64 draws cast to float32, so at the heavy density thousands of them tie.  There the host
path's unstable argsort and the device's stable order may legitimately differ; the probe records whether they do, the
number of tied rows, and compares the device result with the host's arithmetic on the STABLE order (tp / fp of the
device scorer visited in np.argsort(kind='stable') order, stable global argsort, numpy cumulative sums and area).
Writes one JSON file (default profiles/score_rank_device.json).

    python tools/score_rank_probe.py [--out FILE] [--images 3226] [--rounds 1] [--light 10] [--heavy 300]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)


def stable_host_ranking(E, K, torch, dets, anns, iou_thr, dev):
    """eval_map_single_class(device=...) with kind='stable' in both of its argsort calls."""
    d = [np.asarray(x[0], dtype=np.float32).reshape(-1, 5) for x in dets]
    gtl = [np.asarray(a['bboxes'], dtype=np.float32).reshape(-1, 4) for a in anns]
    ignl = [np.asarray(a['bboxes_ignore'], dtype=np.float32).reshape(-1, 4) for a in anns]
    off = lambda n: np.concatenate([[0], np.cumsum(np.asarray(n, dtype=np.int64))]).astype(np.int64)
    alld = np.concatenate(d)
    order = np.concatenate([np.argsort(-x[:, -1], kind='stable') for x in d]).astype(np.int32)
    t = E._upload(dev, [off([x.shape[0] for x in d]), off([g.shape[0] + k.shape[0] for g, k in zip(gtl, ignl)]), alld,
                        np.concatenate([np.vstack([g, k]) for g, k in zip(gtl, ignl)]),
                        np.asarray([g.shape[0] for g in gtl], dtype=np.int32), order])
    tp, fp = K.score_map_tpfp(t[2], t[0], t[3], t[1], t[4], t[5], float(np.float32(iou_thr)))
    both = torch.stack([tp, fp]).cpu().numpy()
    rank = np.argsort(-alld[:, -1], kind='stable')
    ctp, cfp = np.cumsum(both[0][rank]), np.cumsum(both[1][rank])
    eps = np.finfo(np.float32).eps
    recalls = ctp / np.maximum(np.array([sum(g.shape[0] for g in gtl)]), eps)
    precisions = ctp / np.maximum(ctp + cfp, eps)
    return float(E.average_precision_area(recalls, precisions)), recalls, precisions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_rank_device.json'))
    ap.add_argument('--images', type=int, default=3226)
    ap.add_argument('--rounds', type=int, default=1)
    ap.add_argument('--light', type=float, default=10)
    ap.add_argument('--heavy', type=float, default=300)
    a = ap.parse_args()
    import torch
    import score_probe as SP
    import yunet_amd.evaluation as E
    from yunet_amd import kernels as K
    if not torch.cuda.is_available():
        raise RuntimeError('score_rank_probe measures the device scorer: it needs a GPU')
    dev = torch.device('cuda', 0)
    sync = lambda: torch.cuda.synchronize(dev)
    out = dict(command='python tools/score_rank_probe.py ' + ' '.join(sys.argv[1:]), device=torch.cuda.get_device_name(0),
               images=a.images, timing='wall clock between device synchronisations, host / device / rank alternating '
               'A B C C B A after a warm-up; the device figures include packing, upload, kernels, read-back and the host '
               'AP step', densities=[])
    for label, rows in (('light', a.light), ('heavy', a.heavy)):
        events, pred = SP.synth_set(a.images, rows)
        dets, anns = SP.map_inputs(events, pred)
        paths = dict(host=lambda: E.eval_map_single_class(dets, anns, 0.5),
                     device=lambda: E.eval_map_single_class(dets, anns, 0.5, device=dev),
                     rank=lambda: E.eval_map_single_class(dets, anns, 0.5, device=dev, rank='device'))
        got = {k: f() for k, f in paths.items()}                       # the warm-up
        scores = np.concatenate([d[0][:, 4] for d in dets])
        rec = dict(density=label, rows_per_image=rows, predictions=int(scores.shape[0]),
                   tied_rows=int(scores.shape[0] - np.unique(scores).shape[0]),
                   map_value={k: v[0] for k, v in got.items()},
                   equal_map_host_device=bool(got['host'][0] == got['device'][0]),
                   equal_map_host_rank=bool(got['host'][0] == got['rank'][0]
                                            and np.array_equal(got['host'][1]['precision'], got['rank'][1]['precision'])))
        smap, srec, sprec = stable_host_ranking(E, K, torch, dets, anns, 0.5, dev)
        rec['map_value']['stable_host_ranking'] = smap
        rec['equal_map_stable_rank'] = bool(smap == got['rank'][0] and np.array_equal(srec, got['rank'][1]['recall'])
                                            and np.array_equal(sprec, got['rank'][1]['precision']))
        t = {k: [] for k in paths}
        for _ in range(a.rounds):
            for which in ('host', 'device', 'rank', 'rank', 'device', 'host'):
                sync()
                t0 = time.perf_counter()
                paths[which]()
                sync()
                t[which].append(time.perf_counter() - t0)
        rec['map'] = {k: dict(median_s=float(np.median(v)), min_s=float(np.min(v)), max_s=float(np.max(v)), calls=len(v))
                      for k, v in t.items()}
        rec['map']['host_over_rank'] = rec['map']['host']['median_s'] / rec['map']['rank']['median_s']
        rec['map']['device_over_rank'] = rec['map']['device']['median_s'] / rec['map']['rank']['median_s']
        # the kernels alone: per-image ranking, tp / fp, global ranking, curve -- on an uploaded set
        d = [np.asarray(x[0], dtype=np.float32).reshape(-1, 5) for x in dets]
        gtl, ignl = [x['bboxes'] for x in anns], [x['bboxes_ignore'] for x in anns]
        off = lambda n: np.concatenate([[0], np.cumsum(np.asarray(n, dtype=np.int64))]).astype(np.int64)
        up = E._upload(dev, [off([x.shape[0] for x in d]), off([g.shape[0] + k.shape[0] for g, k in zip(gtl, ignl)]),
                             np.concatenate(d), np.concatenate([np.vstack([g, k]) for g, k in zip(gtl, ignl)]),
                             np.asarray([g.shape[0] for g in gtl], dtype=np.int32)])

        def kernels():
            order = K.score_rank_images(up[2], up[0])
            tp, fp = K.score_map_tpfp(up[2], up[0], up[3], up[1], up[4], order, 0.5)
            return K.score_map_curve(tp, fp, K.score_rank_global(up[2]))

        kernels()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 10
        sync()
        ev0.record()
        for _ in range(reps):
            kernels()
        ev1.record()
        sync()
        rec['map']['rank_kernels_only_s'] = ev0.elapsed_time(ev1) / reps / 1e3
        out['densities'].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
