#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/loss_terms_cases.npz by running the UNMODIFIED reference loss
modules (mmdet/models/losses: varifocal_loss.py, smooth_l1_loss.py's L1Loss, mse_loss.py, balanced_l1_loss.py,
iou_loss.py's BoundedIoULoss) in float64, and the unmodified YuNet_Head.loss() in float32 (SimOTAAssigner builds float32
tensors of its own: sim_ota_assigner.py:175-182), under oracle/ref_stub.py.

    python tools/make_golden_loss_terms.py          # needs the reference tree

What the fixture holds (inputs and recorded results only):
  case_*            the inputs of tests/loss_terms_ref.make_case(*GOLDEN_CASE)
  <config>_losses / _dflat   for every entry of GOLDEN_CONFIGS: the four losses and d(sum of them)/d(flat), the reference's
                    modules composed the way YuNet_Head.loss composes them (yunet_head.py:506-527) on the case's assignment
  head_*            a 2-image 64 x 64 batch; per HEAD_CONFIGS entry the loss dict and d/d(flat) of the reference head's own
                    loss() and the assignment it made (gt_inds, max_overlaps)
  sa_*              small inputs and the reference modules' results for every reduction they accept, with and without
                    weight / avg_factor (the stand-alone modules of libfacedetection.train_amd/losses.py)"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import ref_stub                # noqa: E402
import yunet_oracle as O       # noqa: E402
import loss_terms_ref as LT    # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'loss_terms_cases.npz')
F64 = torch.float64


def build(builder, spec):
    return builder.build_loss(dict(spec))


def module_specs(cfg):
    """the reference modules' constructor arguments of a loss_terms_ref.make_cfg dict"""
    def cls(s, w):
        extra = {k: v for k, v in s.items() if k != 'type'}
        return dict(type=s['type'], use_sigmoid=True, reduction='sum', loss_weight=w, **extra)
    ks = dict(cfg['kps'])
    kind = ks.pop('type')
    kps = dict(type=kind, reduction='mean', loss_weight=cfg['w_kps'], **ks)
    if kind in ('SmoothL1Loss', 'BalancedL1Loss'):
        kps['beta'] = cfg['kps_beta']
    if cfg['box_loss'] == 'BoundedIoULoss':
        box = dict(type='BoundedIoULoss', beta=cfg['smooth_point'], eps=cfg['box_eps'], reduction='sum', loss_weight=cfg['w_box'])
    else:
        box = dict(type=cfg['box_loss'], eps=cfg['box_eps'], reduction='sum', loss_weight=cfg['w_box'])
        if cfg['box_loss'] == 'EIoULoss':
            box['smooth_point'] = cfg['smooth_point']
    return cls(cfg['cls'], cfg['w_cls']), box, cls(cfg['obj'], cfg['w_obj']), kps


def composed(builder, case, cfg):
    """YuNet_Head.loss's composition (yunet_head.py:506-527) of the reference's own modules on a given assignment."""
    l_cls, l_box, l_obj, l_kps = (build(builder, s) for s in module_specs(cfg))
    N, P, _ = case['flat'].shape
    x = case['flat'].to(F64).clone().requires_grad_(True)
    pri = O.grid_priors(case['sizes'], case['strides'], F64)
    gi = case['gt_inds'].long()
    pos = gi > 0
    n_idx, p_idx = pos.nonzero(as_tuple=True)
    g_idx = gi[pos] - 1
    gb = case['gt_boxes'].to(F64)[n_idx, g_idx]
    gk = case['gt_kps'].to(F64).reshape(N, -1, 5, 3)[n_idx, g_idx]
    nt = max(float(n_idx.numel()), 1.0)
    decoded = O.bbox_decode(pri[p_idx], x[n_idx, p_idx, 1:5])
    loss_bbox = l_box(decoded, gb) / nt
    loss_obj = l_obj(x[..., 5].reshape(-1, 1), pos.reshape(-1, 1).to(F64)) / nt
    loss_cls = l_cls(x[..., 0][pos].reshape(-1, 1), case['max_overlaps'].to(F64)[pos].reshape(-1, 1)) / nt
    kw = gk[:, :, 2].mean(dim=1, keepdim=True)
    enc = O.kps_encode(pri[p_idx], gk[:, :, :2].reshape(-1, 10))
    loss_kps = l_kps(x[n_idx, p_idx, 6:], enc, weight=kw.view(-1, 1), avg_factor=torch.sum(kw))
    losses = torch.stack([loss_cls, loss_bbox, loss_obj, loss_kps])
    g, = torch.autograd.grad(losses.sum(), x)
    return losses.detach().numpy(), g.numpy()


def head_case(seed=5):
    gen = torch.Generator().manual_seed(seed)
    sizes, strides = [(8, 8), (4, 4), (2, 2)], [8, 16, 32]
    flat = torch.randn(2, 84, 16, generator=gen, dtype=F64) * 0.4
    flat[..., 5] -= 1.0
    gt_boxes = [torch.tensor([[6.0, 8.0, 30.0, 34.0], [36.0, 30.0, 60.0, 58.0], [20.0, 40.0, 33.0, 55.0]], dtype=F64),
                torch.tensor([[10.0, 10.0, 50.0, 52.0], [40.0, 4.0, 56.0, 22.0]], dtype=F64)]
    gt_kps = []
    for b in gt_boxes:
        k = torch.rand(b.shape[0], 5, 3, generator=gen, dtype=F64)
        k[..., 0] = b[:, None, 0] + k[..., 0] * (b[:, None, 2] - b[:, None, 0])
        k[..., 1] = b[:, None, 1] + k[..., 1] * (b[:, None, 3] - b[:, None, 1])
        k[..., 2] = (k[..., 2] < 0.7).to(F64)
        gt_kps.append(k)
    return flat, gt_boxes, gt_kps, sizes, strides


def run_head(head_cfg, flat, gt_boxes, gt_kps, sizes):
    model, _ = ref_stub.build_detector('yunet_n.py', head=head_cfg)
    head = model.bbox_head
    rec = []
    assign = head.assigner.assign

    def recording(*a, **k):
        r = assign(*a, **k)
        rec.append((r.gt_inds.clone(), r.max_overlaps.clone()))
        return r
    head.assigner.assign = recording
    x = flat.float().requires_grad_(True)
    gt_boxes, gt_kps = [b.float() for b in gt_boxes], [k.float() for k in gt_kps]
    maps, off = ([], [], [], []), 0
    for h, w in sizes:
        m = x[:, off:off + h * w].reshape(2, h, w, 16).permute(0, 3, 1, 2)
        off += h * w
        for o, (a, b) in zip(maps, ((0, 1), (1, 5), (5, 6), (6, 16))):
            o.append(m[:, a:b])
    out = head.loss(*maps, gt_boxes, [torch.zeros(b.shape[0], dtype=torch.long) for b in gt_boxes], gt_kps,
                    [dict(img_shape=(64, 64, 3))] * 2)
    losses = torch.stack([out['loss_cls'], out['loss_bbox'], out['loss_obj'], out['loss_kps']])
    g, = torch.autograd.grad(losses.sum(), x)
    gt_inds = torch.stack([r[0] for r in rec]).int()
    ovl = torch.stack([r[1] for r in rec])
    return losses.detach().numpy(), g.numpy(), gt_inds.numpy(), ovl.numpy()


def standalone(builder, pack):
    gen = torch.Generator().manual_seed(3)
    n = 12
    lg, tg = torch.randn(n, 1, generator=gen, dtype=F64) * 2, torch.rand(n, 1, generator=gen, dtype=F64)
    tg[::3] = 0.0
    d_pred, d_tgt = torch.randn(n, 10, generator=gen, dtype=F64), torch.randn(n, 10, generator=gen, dtype=F64) * 0.5
    d_pred[0, :3] = d_tgt[0, :3]
    xy = torch.rand(n, 2, generator=gen, dtype=F64) * 40
    wh = torch.rand(n, 2, generator=gen, dtype=F64) * 30 + 4
    b_tgt = torch.cat([xy, xy + wh], 1)
    b_pred = b_tgt + torch.randn(n, 4, generator=gen, dtype=F64) * wh.repeat(1, 2) * 0.4
    b_pred = torch.cat([torch.minimum(b_pred[:, :2], b_pred[:, 2:] - 1), b_pred[:, 2:]], 1)
    w1 = torch.rand(n, 1, generator=gen, dtype=F64)
    pack.update(sa_logit=lg.numpy(), sa_score=tg.numpy(), sa_pred=d_pred.numpy(), sa_target=d_tgt.numpy(),
                sa_box_pred=b_pred.numpy(), sa_box_target=b_tgt.numpy(), sa_weight=w1.numpy())
    for name, spec, (p, t) in (
            ('vfl', dict(type='VarifocalLoss', alpha=0.6, gamma=1.5, iou_weighted=True, loss_weight=2.0), (lg, tg)),
            ('vfl_now', dict(type='VarifocalLoss', iou_weighted=False), (lg, tg)),
            ('l1', dict(type='L1Loss', loss_weight=0.5), (d_pred, d_tgt)),
            ('mse', dict(type='MSELoss', loss_weight=0.5), (d_pred, d_tgt)),
            ('bl1', dict(type='BalancedL1Loss', alpha=0.4, gamma=1.2, beta=0.5, loss_weight=3.0), (d_pred, d_tgt)),
            ('bounded', dict(type='BoundedIoULoss', beta=0.1, eps=1e-3, loss_weight=2.0), (b_pred, b_tgt))):
        mod = build(builder, spec)
        for red in ('none', 'mean', 'sum'):
            pack[f'sa_{name}_{red}'] = mod(p, t, reduction_override=red).detach().numpy()
            pack[f'sa_{name}_{red}_w'] = mod(p, t, weight=w1, reduction_override=red).detach().numpy()
        pack[f'sa_{name}_mean_w_avg'] = mod(p, t, weight=w1, avg_factor=7.5, reduction_override='mean').detach().numpy()
        q = p.clone().requires_grad_(True)
        g, = torch.autograd.grad(mod(q, t, weight=w1, reduction_override='sum'), q)
        pack[f'sa_{name}_grad'] = g.numpy()


def main():
    if not ref_stub.available():
        raise SystemExit('needs the reference tree')
    ns = ref_stub.load_reference()
    for m in ('varifocal_loss', 'balanced_l1_loss', 'mse_loss'):
        importlib.import_module('mmdet.models.losses.' + m)
    builder = ns.builder
    case = LT.make_case(*LT.GOLDEN_CASE)
    pack = {f'case_{k}': np.asarray(v) if not torch.is_tensor(v) else v.numpy()
            for k, v in case.items() if k != 'img_stats'}
    for name, kw in LT.GOLDEN_CONFIGS.items():
        cfg = LT.make_cfg(**kw)
        pack[f'{name}_losses'], pack[f'{name}_dflat'] = composed(builder, case, cfg)
        print(name, pack[f'{name}_losses'], LT.census(case, cfg))
    flat, gt_boxes, gt_kps, sizes, strides = head_case()
    pack.update(head_flat=flat.float().numpy(), head_sizes=np.asarray(sizes), head_strides=np.asarray(strides),
                head_gt_count=np.asarray([b.shape[0] for b in gt_boxes]))
    gmax = max(b.shape[0] for b in gt_boxes)
    gb, gk = np.zeros((2, gmax, 4), np.float32), np.zeros((2, gmax, 5, 3), np.float32)
    for i, (b, k) in enumerate(zip(gt_boxes, gt_kps)):
        gb[i, :b.shape[0]], gk[i, :b.shape[0]] = b.numpy(), k.numpy()
    pack.update(head_gt_boxes=gb, head_gt_kps=gk)
    for name, head in LT.HEAD_CONFIGS.items():
        (pack[f'head_{name}_losses'], pack[f'head_{name}_dflat'], pack[f'head_{name}_gt_inds'],
         pack[f'head_{name}_max_overlaps']) = run_head(head, flat, gt_boxes, gt_kps, sizes)
        print('head', name, pack[f'head_{name}_losses'], 'positives', int((pack[f'head_{name}_gt_inds'] > 0).sum()))
    standalone(builder, pack)
    with open(OUT, 'wb') as f:
        np.savez_compressed(f, **pack)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
