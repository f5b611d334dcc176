#!/usr/bin/env python
"""Host scorer against device scorer (evaluation.py device=None / device='cuda') on a synthetic set with WIDER val's
shape: 3 226 images in 61 events, a heavy-tailed number of faces per image that reaches 709, and two prediction
densities (about 10 rows per image, and a few hundred).  For each density and protocol (WIDER easy / medium / hard AP;
the single-class mAP EvalHook reports) it times the whole call on both paths -- wall clock between device
synchronisations, so the device figure holds packing, the upload, the kernels, the read-back and the host AP step --
alternating A B B A after a warm-up, checks that both paths return the same integers and APs, and times the kernels
alone with device events.  Writes one JSON file (default profiles/score_device.json).

    python tools/score_probe.py [--out FILE] [--images 3226] [--rounds 1] [--light 10] [--heavy 300]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle')):
    if p not in sys.path:
        sys.path.insert(0, p)


def synth_set(n_images, rows_per_image, seed=0, n_events=61, max_faces=709):
    """(events, pred) in the layouts of wider_fixture.synth_events.  Faces per image: a log-normal draw (median 4,
    like WIDER's crowd scenes a long tail) clipped to max_faces, with one image at exactly max_faces; predictions: a
    jittered copy of most faces, then stray boxes up to about rows_per_image, in descending score."""
    rng = np.random.default_rng(seed)
    faces = np.minimum(np.floor(np.exp(rng.normal(np.log(4.0), 1.35, n_images))).astype(np.int64), max_faces)
    faces[rng.uniform(size=n_images) < 0.01] = 0
    faces[int(rng.integers(0, n_images))] = max_faces
    events, pred = [], {}
    for e in range(n_events):
        events.append(dict(name=f'{e}--Event_{e}', images=[]))
        pred[events[-1]['name']] = {}
    for i in range(n_images):
        ev = events[i % n_events]
        g = int(faces[i])
        xy = rng.uniform(0, 1000, (g, 2))
        wh = np.exp(rng.uniform(np.log(6), np.log(200), (g, 1))) * np.array([[1.0, 1.25]])
        boxes = np.round(np.concatenate([xy, wh], 1))
        size = boxes[:, 2]
        keep = {k: (np.nonzero(size >= t)[0] + 1).astype(np.int64) for k, t in (('easy', 50), ('medium', 20), ('hard', 8))}
        name = f'{i % n_events}_Event_{i}'
        ev['images'].append(dict(name=name, boxes=boxes.astype(np.float64), keep=keep))
        n = max(0, int(rng.poisson(rows_per_image)))
        near = min(n, int(0.8 * g))
        rows = np.zeros((n, 5))
        if near:
            pick = rng.choice(g, near, replace=False)
            rows[:near, :4] = boxes[pick] + rng.normal(0, 0.1, (near, 4)) * boxes[pick][:, [2, 3, 2, 3]]
            rows[:near, 4] = rng.uniform(0.3, 0.99, near)
        rows[near:, :2] = rng.uniform(0, 1000, (n - near, 2))
        rows[near:, 2:4] = rng.uniform(8, 120, (n - near, 2))
        rows[near:, 4] = rng.uniform(0.02, 0.7, n - near)
        pred[ev['name']][name] = rows[np.argsort(-rows[:, 4], kind='stable')]
    return events, pred


def map_inputs(events, pred):
    """The same set as EvalHook sees it: float32 xyxy detections per image; the faces outside 'hard' are ignored boxes."""
    dets, anns = [], []
    for ev in events:
        for im in ev['images']:
            d = pred[ev['name']][im['name']].astype(np.float32)
            d[:, 2:4] += d[:, :2]
            b = im['boxes'].astype(np.float32)
            b[:, 2:4] += b[:, :2]
            hard = np.zeros(len(b), dtype=bool)
            hard[im['keep']['hard'] - 1] = True
            dets.append([d])
            anns.append(dict(bboxes=b[hard], bboxes_ignore=b[~hard]))
    return dets, anns


def abba(host, device, rounds, sync):
    """Seconds per call of host() and device(), alternating A B B A `rounds` times (the caller has run both once: the
    equality check is the warm-up)."""
    t = {'host': [], 'device': []}
    for _ in range(rounds):
        for which in ('host', 'device', 'device', 'host'):
            sync()
            t0 = time.perf_counter()
            (host if which == 'host' else device)()
            sync()
            t[which].append(time.perf_counter() - t0)
    return {k: dict(median_s=float(np.median(v)), min_s=float(np.min(v)), max_s=float(np.max(v)), calls=len(v))
            for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_device.json'))
    ap.add_argument('--images', type=int, default=3226)
    ap.add_argument('--rounds', type=int, default=1)
    ap.add_argument('--light', type=float, default=10)
    ap.add_argument('--heavy', type=float, default=300)
    a = ap.parse_args()
    import torch
    import yunet_amd.evaluation as E
    from yunet_amd import kernels as K
    if not torch.cuda.is_available():
        raise RuntimeError('score_probe measures the device scorer: it needs a GPU')
    dev = torch.device('cuda', 0)
    sync = lambda: torch.cuda.synchronize(dev)
    out = dict(command='python tools/score_probe.py ' + ' '.join(sys.argv[1:]), device=torch.cuda.get_device_name(0),
               images=a.images, timing='wall clock between device synchronisations, A B B A after a warm-up; the device '
               'figure includes packing, upload, kernels, read-back and the host AP step', densities=[])
    for label, rows in (('light', a.light), ('heavy', a.heavy)):
        events, pred = synth_set(a.images, rows)
        n_pred = sum(len(v) for p in pred.values() for v in p.values())
        n_gt = sum(len(im['boxes']) for ev in events for im in ev['images'])
        rec = dict(density=label, rows_per_image=rows, predictions=n_pred, ground_truths=n_gt,
                   max_faces_per_image=max(len(im['boxes']) for ev in events for im in ev['images']))
        # ---- WIDER
        with np.errstate(all='ignore'):
            ch, fh = E.wider_pr_counts(copy.deepcopy(pred), events)
            cd, fd = E.wider_pr_counts(copy.deepcopy(pred), events, device=dev)
            aps_h, aps_d = E.wider_aps_from_counts(ch, fh), E.wider_aps_from_counts(cd, fd)
        rec['equal_counts'] = bool(np.array_equal(ch, cd) and np.array_equal(fh, fd))
        rec['equal_aps'] = bool(aps_h == aps_d)
        rec['aps'] = aps_d
        copies = [copy.deepcopy(pred) for _ in range(4 * a.rounds)]       # each call normalises its input in place
        t = abba(lambda: E.wider_evaluation(copies.pop(), events), lambda: E.wider_evaluation(copies.pop(), events, device=dev),
                 a.rounds, sync)
        rec['wider'] = dict(t, host_over_device=t['host']['median_s'] / t['device']['median_s'])
        packed = E.pack_wider(pred, events)
        d = E._upload(dev, [packed[0], packed[1], packed[2], packed[3], E._thresholds(), packed[4]])
        K.score_wider(d[0], d[1], d[2], d[3], d[5], d[4], 0.5)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 10
        sync()
        ev0.record()
        for _ in range(reps):
            K.score_wider(d[0], d[1], d[2], d[3], d[5], d[4], 0.5)
        ev1.record()
        sync()
        rec['wider']['kernels_only_s'] = ev0.elapsed_time(ev1) / reps / 1e3
        # ---- mAP
        dets, anns = map_inputs(events, pred)
        mh, rh = E.eval_map_single_class(dets, anns, 0.5)
        md, rd = E.eval_map_single_class(dets, anns, 0.5, device=dev)
        rec['equal_map'] = bool(mh == md and np.array_equal(rh['precision'], rd['precision']))
        rec['map_value'] = md
        t = abba(lambda: E.eval_map_single_class(dets, anns, 0.5), lambda: E.eval_map_single_class(dets, anns, 0.5, device=dev),
                 a.rounds, sync)
        rec['map'] = dict(t, host_over_device=t['host']['median_s'] / t['device']['median_s'])
        out['densities'].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
