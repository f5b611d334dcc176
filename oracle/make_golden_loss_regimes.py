#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- tests/golden/loss_regimes_reference.npz: the UNMODIFIED reference's box losses
(mmdet/models/losses/iou_loss.py: eiou / diou / giou / ciou / iou_loss in its three modes) and smooth_l1_loss
(smooth_l1_loss.py), run through oracle/ref_stub.py in float64 on the regime inputs of tests/loss_ref.py (ties,
touching and disjoint boxes, nested boxes, IoU up to 0.9999, smooth-L1 at d = 0 and on both sides of beta).  Stores
values and gradients with respect to the decoded box and the landmark predictions.  tests/test_loss_ref.py checks
the fp64 functions of tests/loss_ref.py, the yardstick of the loss-kernel tests, against this fixture.

    python oracle/make_golden_loss_regimes.py            # needs the reference tree
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(ROOT, 'tests')]
import ref_stub        # noqa: E402
import yunet_oracle as O   # noqa: E402
import loss_ref as R   # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'loss_regimes_reference.npz')


def main():
    if not ref_stub.available():
        raise SystemExit('needs the reference tree')
    ns = ref_stub.load_reference()
    iou = ns.mods['mmdet.models.losses.iou_loss']
    sl1 = ns.mods['mmdet.models.losses.smooth_l1_loss']
    case = R.make_case(2, 160, 160, 31, boxes=('generic', 'tie', 'touch', 'disjoint', 'nested'))
    cfg = R.make_cfg()
    r = R.ref_of(case, cfg)
    n_idx, p_idx, g_idx = r['pos']
    pri = O.grid_priors(case['sizes'], case['strides'], torch.float64)[p_idx]
    pred = O.bbox_decode(pri, case['flat'].double()[n_idx, p_idx, 1:5])
    tgt = case['gt_boxes'].double()[n_idx, g_idx]
    gk = case['gt_kps'].double()[n_idx, g_idx]
    kps_pred = case['flat'].double()[n_idx, p_idx, 6:]
    kps_tgt = O.kps_encode(pri, gk[:, :, :2].reshape(-1, 10))
    sp, eps, beta = cfg['smooth_point'], cfg['box_eps'], cfg['kps_beta']
    pack = dict(pred=pred.numpy(), target=tgt.numpy(), kps_pred=kps_pred.numpy(), kps_target=kps_tgt.numpy(),
                smooth_point=np.float64(sp), eps=np.float64(eps), beta=np.float64(beta))
    calls = {'EIoULoss': lambda p, t: iou.eiou_loss(p, t, reduction='none', smooth_point=sp, eps=eps),
             'DIoULoss': lambda p, t: iou.diou_loss(p, t, reduction='none', eps=eps),
             'GIoULoss': lambda p, t: iou.giou_loss(p, t, reduction='none', eps=eps),
             'CIoULoss': lambda p, t: iou.ciou_loss(p, t, reduction='none', eps=eps),
             'IoULoss_linear': lambda p, t: iou.iou_loss(p, t, reduction='none', mode='linear', eps=eps),
             'IoULoss_square': lambda p, t: iou.iou_loss(p, t, reduction='none', mode='square', eps=eps),
             'IoULoss_log': lambda p, t: iou.iou_loss(p, t, reduction='none', mode='log', eps=eps)}
    for key, fn in calls.items():
        p = pred.clone().requires_grad_(True)
        v = fn(p, tgt)
        g, = torch.autograd.grad(v.sum(), p)
        pack[f'{key}_value'] = v.detach().numpy()
        pack[f'{key}_grad'] = g.numpy()
    k = kps_pred.clone().requires_grad_(True)
    v = sl1.smooth_l1_loss(k, kps_tgt, reduction='none', beta=beta)
    g, = torch.autograd.grad(v.sum(), k)
    pack['smooth_l1_value'] = v.detach().numpy()
    pack['smooth_l1_grad'] = g.numpy()
    c = R.census(case, cfg, r)
    print('census', c)
    with open(OUT, 'wb') as f:
        np.savez(f, **pack)
    print('wrote', OUT)


if __name__ == '__main__':
    main()
