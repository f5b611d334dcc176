#!/usr/bin/env python
"""Rate of yunet_fetch_windows alone (no training step running): the GPU reading each image's crop window from the
pinned host store, next to a linear pinned-host -> device copy_ of the same byte count, both timed with device events.

The sources and windows are train_e2e's host_window_kernel mode: configs/yunet_n.py's pipeline, bs 256 from
SyntheticSourceImages' default pool (64 decoded images of 768 x 1024 / 1024 x 683 / 500 x 375 / 683 x 1024), the
windows the real plan picks at iterations 0 .. --plans - 1.

    python tools/window_fetch_probe.py [--plans 8] [--reps 5] [--out profiles/window_fetch_probe.json]

Prints / writes one JSON object: window bytes per batch, fetch ms and GB/s (mean / min / max over plans x reps), the
linear copy's ms and GB/s, and the status word after all fetches (0: every plan row valid)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms, nbytes):
    gbs = [b / (t * 1e-3) / 1e9 for t, b in zip(ms, nbytes)]
    return {'ms_mean': round(sum(ms) / len(ms), 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4),
            'GBs_mean': round(sum(gbs) / len(gbs), 2), 'GBs_min': round(min(gbs), 2), 'GBs_max': round(max(gbs), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default=os.path.join(ROOT, 'configs', 'yunet_n.py'))
    ap.add_argument('--plans', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import yunet_amd
    import yunet_amd._lib as L
    import yunet_amd.runner as R
    if not torch.cuda.is_available():
        raise SystemExit('window_fetch_probe measures on the GPU: no device found')
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(a.config)
    bs = cfg.data.samples_per_gpu
    src = R.SyntheticSourceImages(cfg.train_pipeline, samples_per_gpu=bs, host_fed='window', host_fetch='kernel')
    src._build_window(dev)
    store, feed = src._feed.store, src._feed
    plans = []
    for it in range(a.plans):
        sb = store.batch(src._idx)
        _, rect, off = src.pipe.window_plan(sb, it, dev)
        plans.append((sb, rect, off))
    torch.cuda.synchronize()
    win = feed._bufs[0]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def fetch(sb, rect, off):
        L.check(L.load().yunet_fetch_windows(p(store.data), store.nbytes, p(sb.src_off), p(sb.src_hw), p(rect), p(off),
                                             sb.n, p(win), win.numel(), p(status), C.c_void_p(stream.cuda_stream)),
                'yunet_fetch_windows')

    for sb, rect, off in plans:                         # warm-up: code object load, first touch of the mappings
        fetch(sb, rect, off)
    torch.cuda.synchronize()
    ev = []
    for _ in range(a.reps):
        for sb, rect, off in plans:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fetch(sb, rect, off)
            e1.record(stream)
            ev.append((e0, e1, int(off[-1])))
    torch.cuda.synchronize()
    f_ms = [e0.elapsed_time(e1) for e0, e1, _ in ev]
    f_bytes = [b for _, _, b in ev]
    mean_bytes = sum(f_bytes) // len(f_bytes)
    # a linear copy of the same byte count from pinned memory
    host = torch.empty(mean_bytes, dtype=torch.uint8, pin_memory=True)     # the pool store is smaller than a batch
    dst = win[:mean_bytes]
    for _ in range(2):
        dst.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    lin = []
    for _ in range(a.reps * a.plans):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        dst.copy_(host, non_blocking=True)
        e1.record(stream)
        lin.append((e0, e1))
    torch.cuda.synchronize()
    l_ms = [e0.elapsed_time(e1) for e0, e1 in lin]
    res = {'what': __doc__.split('\n')[0], 'config': os.path.basename(a.config), 'batch': bs, 'plans': a.plans,
           'reps': a.reps, 'store_bytes': store.nbytes, 'batch_source_bytes': src._batch_bytes,
           'window_bytes_mean': mean_bytes, 'window_bytes_min': min(f_bytes), 'window_bytes_max': max(f_bytes),
           'fetch': _stats(f_ms, f_bytes), 'linear_copy': _stats(l_ms, [mean_bytes] * len(l_ms)),
           'status': int(status.item()), 'device': torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    if res['status']:
        raise SystemExit(f'yunet_fetch_windows flagged plan rows: status {res["status"]}')


if __name__ == '__main__':
    main()
