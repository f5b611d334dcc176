#!/usr/bin/env python
"""Evaluation throughput per image: the per-image path (prepare_test_image + simple_test with the per-image tail) against
the batched device test pipeline (DeviceTestPipeline + simple_test with the batched tail) from a resident store.

    python tools/test_pipeline_probe.py [--images 256] [--batches 1,8,32,64] [--mode 640] [--min-s 0.5] [--out probe.json]

YuNet_n with the trained fixture, --images synthetic WIDER-sized uint8 sources (decoded already: PIL decode is host
time outside both paths and is not measured here), one view at (mode, mode).  Order A B B A in one process:
  a  per image: wall time of prepare_test_image -> eval forward -> get_bboxes_flat -> .cpu() per image (what
     YuNet.simple_test did before its tail was batched), images/s over at least --min-s seconds after a warm-up pass,
     and a second pass with a device synchronisation between the phases for the prepare / forward+detect / host-tail split;
  b  the new path at each batch size from a SourceStore(placement='device'), images/s the same way;
  c  yunet_test_pixels alone at the largest batch: event time and GB/s of source bytes read + canvas bytes written.
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--batches', default='1,8,32,64')
    ap.add_argument('--mode', type=int, default=640)
    ap.add_argument('--min-s', type=float, default=0.5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import yunet_amd
    from yunet_amd import evaluation as E
    from yunet_amd import test_pipeline as TP
    from yunet_amd.source_store import SourceStore
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    model = yunet_amd.build_detector(cfg.model)
    sd = torch.load(os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth'), map_location='cpu',
                    weights_only=False)['state_dict']
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    rng = np.random.default_rng(0)
    hw = ((768, 1024), (1024, 683), (500, 375), (683, 1024))
    sizes = [hw[i % len(hw)] for i in range(a.images)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    store = SourceStore(sizes, placement='device', device=dev)
    for i, im in enumerate(imgs):
        store.put(i, im, np.zeros((0, 4), np.float32), np.zeros((0, 15), np.float32))
    scale = (a.mode, a.mode)
    pipe = TP.DeviceTestPipeline(None, scale=scale)
    sync = torch.cuda.synchronize

    def per_image(i, split=None):
        t0 = time.perf_counter()
        x, meta = E.prepare_test_image(imgs[i], scale, dev)
        if split is not None:
            sync()
            t1 = time.perf_counter()
        eng = model._ensure_engine(dev)
        flat = eng.forward_eval(x.float().contiguous())
        if split is not None:
            sync()
            t2 = time.perf_counter()
        res, _ = model.bbox_head.get_bboxes_flat(flat, eng.plan.sizes, [meta], rescale=True)
        out = [[d.cpu().numpy()] for d, _ in res]
        if split is not None:
            t3 = time.perf_counter()
            split[0] += t1 - t0
            split[1] += t2 - t1
            split[2] += t3 - t2
        return out

    def run_a():
        with torch.no_grad():
            for i in range(min(16, a.images)):
                per_image(i)
            sync()
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < a.min_s or n < a.images:
                per_image(n % a.images)
                n += 1
            sync()
            dt = time.perf_counter() - t0
            split = [0.0, 0.0, 0.0]
            for i in range(a.images):
                per_image(i, split)
        return dict(images=n, seconds=round(dt, 4), images_per_s=round(n / dt, 1), ms_per_image=round(1e3 * dt / n, 4),
                    split_ms_with_syncs=dict(prepare=round(1e3 * split[0] / a.images, 4),
                                             forward_detect=round(1e3 * split[1] / a.images, 4),
                                             host_tail=round(1e3 * split[2] / a.images, 4)))

    def run_b(B):
        batches = TP.batches_of(range(a.images), B)

        def one(b):
            img, metas = pipe((store.data, store.offsets[b], store.hw[b]), 0)
            return model(return_loss=False, rescale=True, img=[img], img_metas=[metas])
        with torch.no_grad():
            for b in batches[:max(2, 16 // B)] + batches[-1:]:
                one(b)
            sync()
            n, k, t0 = 0, 0, time.perf_counter()
            while time.perf_counter() - t0 < a.min_s or k < len(batches):
                b = batches[k % len(batches)]
                one(b)
                n += len(b)
                k += 1
            sync()
            dt = time.perf_counter() - t0
        return dict(images=n, seconds=round(dt, 4), images_per_s=round(n / dt, 1), ms_per_image=round(1e3 * dt / n, 4))

    def run_c(B):
        b = list(range(min(B, a.images)))
        img, metas = pipe((store.data, store.offsets[b], store.hw[b]), 0)
        table = np.array([[m['img_shape'][0], m['img_shape'][1], 0, 0] for m in metas], dtype=np.int32)
        d_off = torch.from_numpy(store.offsets[b]).to(dev)
        d_hw = torch.from_numpy(store.hw[b]).to(dev)
        d_tab = torch.from_numpy(table).to(dev)
        for _ in range(3):
            TP.launch_pixels(store.data, d_off, d_hw, d_tab, img)
        sync()
        iters = 50
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            TP.launch_pixels(store.data, d_off, d_hw, d_tab, img)
        e1.record()
        sync()
        ms = e0.elapsed_time(e1) / iters
        nbytes = int(store.image_bytes[b].sum()) + img.numel() * 4
        return dict(batch=len(b), canvas=list(img.shape[2:]), ms=round(ms, 4), bytes_read_plus_written=nbytes,
                    gb_per_s=round(nbytes / ms / 1e6, 1))

    bs = [int(v) for v in a.batches.split(',')]
    res = {'what': ' '.join(__doc__.split('\n\n')[0].split()), 'images': a.images, 'mode': a.mode, 'sizes': [list(s) for s in hw],
           'device': torch.cuda.get_device_name(0), 'order': 'A B B A'}
    res['a_per_image'] = [run_a()]
    res['b_batched'] = {str(B): [run_b(B)] for B in bs}
    for B in bs:
        res['b_batched'][str(B)].append(run_b(B))
    res['a_per_image'].append(run_a())
    res['c_pixel_kernel'] = run_c(max(bs))
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
