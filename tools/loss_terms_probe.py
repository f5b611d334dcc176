#!/usr/bin/env python
"""What the loss terms beyond the default selection cost, and that the default step costs what it did (needs a GPU; reads
nothing outside the repository but the parent checkout it is pointed at).

    tools/loss_terms_probe.py --out profiles/loss_terms.json [--parent DIR] [--batch 256 --size 320 --launches 200]

* kernel: one training step of YuNet_n at the bench geometry (N = 256, 320 x 320: P = 2100) fills the loss step's inputs
  (predictions, assignment, normaliser); then `--launches` back-to-back launches of yunet_loss_terms per selection between
  two device events, after a warm-up of 20: microseconds per launch for the default terms (= loss_kernel) and for each new
  term alone and all together (= loss_terms_kernel).  The new terms get no bar; their numbers are recorded.
* step (with --parent, a built checkout of the parent commit): `bench.py --gpus 1 --steps 40 --warmup 10` as a child process
  in the order parent / this / this / parent on one box.  The default mode passes if the two means differ by no more than the
  1.7 % session-to-session spread of DESIGN.md section 6 (exit status 1 otherwise).  A child that fails ends the probe.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

SPREAD = 0.017
VFL = dict(type='VarifocalLoss', alpha=0.75, gamma=2.0, iou_weighted=True)
BL1 = dict(type='BalancedL1Loss', alpha=0.5, gamma=1.5)
SELECTIONS = {
    'default': dict(),
    'vfl_cls': dict(loss_cls=VFL),
    'vfl_obj_gamma2': dict(loss_obj=VFL),
    'vfl_obj_gamma1.5': dict(loss_obj=dict(VFL, gamma=1.5)),
    'l1_kps': dict(loss_kps='L1Loss'),
    'mse_kps': dict(loss_kps='MSELoss'),
    'balanced_l1_kps': dict(loss_kps=BL1, kps_beta=1.0),
    'bounded_iou_box': dict(box='BoundedIoULoss', smooth_point=0.2, box_eps=1e-3),
    'all_new': dict(loss_cls=VFL, loss_obj=VFL, loss_kps=BL1, kps_beta=1.0, box='BoundedIoULoss', smooth_point=0.2, box_eps=1e-3),
}


def kernel_times(a):
    import ctypes as C

    import torch

    import yunet_amd
    import yunet_amd._lib as L
    import yunet_amd.kernels as K
    import yunet_amd.synthetic as S
    from yunet_amd.optim import FusedSGD
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    m = yunet_amd.build_detector(cfg.model)
    ck = torch.load(os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth'), map_location='cpu', weights_only=False)
    m.load_state_dict(ck['state_dict'], strict=True)
    m.to(dev).train()
    opt = FusedSGD(m, lr=1e-5, momentum=0.9, weight_decay=5e-4)
    out = m.train_step(S.to_device(S.make_batch(a.batch, a.size, a.size, 1234, structured=True), dev), opt)
    opt.zero_grad()
    out['loss'].backward()
    torch.cuda.synchronize()
    p = m.engine.plan
    n, P, gmax = p.flat.shape[0], p.flat.shape[1], p.gt_boxes.shape[1]
    lib = L.load()
    blocks = lib.yunet_loss_blocks(n, P)
    part = torch.empty(blocks, 4, device=dev)
    dflat = torch.empty_like(p.dflat)
    res = {}
    for name, sel in SELECTIONS.items():
        terms = K.make_loss_terms(sel.get('loss_cls'), sel.get('loss_obj'), sel.get('loss_kps'))
        c = K.make_loss_cfg(sel.get('box', 'EIoULoss'), box_eps=sel.get('box_eps', 1e-6), smooth_point=sel.get('smooth_point', 0.1),
                            kps_beta=sel.get('kps_beta', 1.0 / 9.0), terms=terms)

        def launch():
            L.check(lib.yunet_loss_terms(K._p(p.flat), K._p(p.gt_inds), K._p(p.max_overlaps), K._p(p.gt_boxes), K._p(p.gt_kps),
                                         C.byref(p.levels), C.byref(c), C.byref(terms), K._p(p.norm), n, P, gmax, K._p(dflat),
                                         K._p(part), blocks, K._stream()), 'yunet_loss_terms')
        for _ in range(20):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            launch()
        e1.record()
        torch.cuda.synchronize()
        res[name] = dict(us_per_launch=round(1000.0 * e0.elapsed_time(e1) / a.launches, 2),
                         kernel='loss_kernel' if name == 'default' else 'loss_terms_kernel',
                         finite=bool(torch.isfinite(dflat).all()))
    return dict(N=n, P=P, positives=int((p.gt_inds > 0).sum()), blocks=blocks, launches=a.launches,
                device=torch.cuda.get_device_name(0), selections=res)


def bench(tree):
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '40', '--warmup', '10'], cwd=tree,
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f'bench.py in {tree} ended with status {r.returncode}: {r.stderr[-400:]}')
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1]
    return json.loads(line)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--no-kernel', action='store_true')
    a = ap.parse_args(argv)
    res, ok = {}, True
    if a.parent:
        order = [('parent', a.parent), ('this', ROOT), ('this', ROOT), ('parent', a.parent)]
        runs = [(who, bench(tree)) for who, tree in order]
        mean = {w: sum(r['ms_per_step'] for ww, r in runs if ww == w) / 2 for w in ('parent', 'this')}
        diff = mean['this'] / mean['parent'] - 1.0
        ok = abs(diff) <= SPREAD
        res['default_step'] = dict(command='bench.py --gpus 1 --steps 40 --warmup 10', order=[w for w, _ in runs],
                                   ms_per_step=[r['ms_per_step'] for _, r in runs],
                                   images_per_sec=[r['value'] for _, r in runs],
                                   final_loss=[r.get('final_loss') for _, r in runs],
                                   mean_ms={k: round(v, 4) for k, v in mean.items()}, this_over_parent=round(1.0 + diff, 4),
                                   bar=f'|difference of the means| <= {SPREAD:.1%} (session-to-session spread, DESIGN.md section 6)',
                                   met=ok)
    if not a.no_kernel:
        res['loss_kernel'] = kernel_times(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
