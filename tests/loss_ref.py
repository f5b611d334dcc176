"""fp64 reference of the fused loss step, its branch census, a per-element checker and regime constructors.

The kernels under test are loss_kernel / loss_norm_kernel / loss_finalize_kernel of
libfacedetection.train_amd/csrc/loss_step.hip.  `loss_ref` takes the loss kernel's own inputs -- the assignment
(gt_inds, max_overlaps) comes in as data, so assignment ties cannot mix into loss checks -- and composes the oracle's
restatements (O.bbox_decode, O.kps_encode, O.box_loss_fn, O.smooth_l1, binary_cross_entropy_with_logits) the way
O.loss_step composes them.  Its gradient is torch autograd: it shares no arithmetic with the kernel's forward-mode dual
numbers.  In float32 it reproduces O.loss_step on the oracle's own assignment (tests/test_loss_ref.py); in float64 it
is the yardstick, pinned to the reference's own loss functions by tests/golden/loss_regimes_reference.npz.

`check` grades a kernel result element by element against the fp64 value with a bar that follows each element's
own conditioning (see ELEMENT_A / ELEMENT_B), and the four losses with the sum of their terms' bars plus the
reduction's own rounding."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import yunet_oracle as O

U32 = 2.0 ** -24                                   # unit roundoff of fp32
F32_EPS = float(torch.finfo(torch.float32).eps)    # the kps normaliser's eps (yunet_head.py, loss_step.hip)
# per-element bar: ELEMENT_A * max(|f32 - f64|, spread) + ELEMENT_B * U32 * |f64| + TINY.
#  - |f32 - f64| is what one fp32 evaluation order (the restatement under autograd) actually lost; spread is what a
#    1-ulp move of the fp32 inputs does to the exact result (the element's conditioning).  The kernel evaluates in
#    another order, so it may lose a few times either: factor 16.
#  - the longest fp32 chain behind one element (decode, EIoU's inter / union, the dual-number quotient rule, the
#    weight and the normaliser) is ~40 roundings; ELEMENT_B = 64 covers it where both terms above happen to be small.
#  - TINY only lets fp32 flush what fp64 keeps below the fp32 range (sigmoid(-100) ~ 4e-44).
# Fixed here, not tuned per case.
ELEMENT_A = 16.0
ELEMENT_B = 64.0
TINY = 1e-30
LOSS_THREADS = 256
MAX_LOSS_BLOCKS = 2048
BOX_LOSSES = [('EIoULoss', None), ('DIoULoss', None), ('GIoULoss', None), ('CIoULoss', None),
              ('IoULoss', 'linear'), ('IoULoss', 'square'), ('IoULoss', 'log')]


def _f32(v):
    return float(np.float32(v))


def make_cfg(box_loss='EIoULoss', box_mode=None, box_eps=1e-6, w_cls=1.0, w_box=5.0, w_obj=1.0, w_kps=0.1,
             smooth_point=0.1, kps_beta=1.0 / 9.0):
    """The loss parameters of kernels.make_loss_cfg, rounded to the fp32 values the kernel receives: the reference
    computes the same operation with the same constants."""
    if box_loss == 'IoULoss' and box_mode is None:
        box_mode = 'log'
    c = dict(box_loss=box_loss, box_mode=box_mode)
    for k, v in dict(box_eps=box_eps, w_cls=w_cls, w_box=w_box, w_obj=w_obj, w_kps=w_kps, smooth_point=smooth_point,
                     kps_beta=kps_beta).items():
        c[k] = _f32(v)
    return c


def kernel_cfg(cfg, defer=False):
    """-> the YunetLossCfg of a make_cfg dict."""
    import yunet_amd.kernels as k
    c = k.make_loss_cfg(cfg['box_loss'], w_cls=cfg['w_cls'], w_box=cfg['w_box'], w_obj=cfg['w_obj'],
                        w_kps=cfg['w_kps'], box_eps=cfg['box_eps'], smooth_point=cfg['smooth_point'],
                        kps_beta=cfg['kps_beta'], box_mode=cfg['box_mode'])
    c.defer_num_total = 1 if defer else 0
    return c


def arch_of(cfg):
    return dict(loss_bbox=cfg['box_loss'], loss_bbox_eps=cfg['box_eps'], loss_bbox_mode=cfg['box_mode'],
                loss_bbox_smooth_point=cfg['smooth_point'])


# ------------------------------------------------------------------------------------------- branch restatements
def _edges(pred, target):
    lt = torch.max(pred[:, :2], target[:, :2])
    rb = torch.min(pred[:, 2:], target[:, 2:])
    return rb - lt                                  # overlap width / height before clamp(min=0)


def ious_eps(pred, target, eps):
    """overlap / (ap + ag - overlap + eps): the IoU of diou_loss / ciou_loss and, rearranged, 1 - x of eiou_loss."""
    wh = _edges(pred, target).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    ap = (pred[:, 2] - pred[:, 0]) * (pred[:, 3] - pred[:, 1])
    ag = (target[:, 2] - target[:, 0]) * (target[:, 3] - target[:, 1])
    return overlap / (ap + ag - overlap + eps)


def eiou_x(pred, target, eps):
    """x of eiou_loss, in O.eiou_loss's evaluation order (so its branch decision is the same one, in both dtypes)."""
    px1, py1, px2, py2 = pred.unbind(-1)
    tx1, ty1, tx2, ty2 = target.unbind(-1)
    ex1, ey1 = torch.min(px1, tx1), torch.min(py1, ty1)
    ix1, iy1 = torch.max(px1, tx1), torch.max(py1, ty1)
    ix2, iy2 = torch.min(px2, tx2), torch.min(py2, ty2)
    xmin, ymin = torch.min(ix1, ix2), torch.min(iy1, iy2)
    xmax, ymax = torch.max(ix1, ix2), torch.max(iy1, iy2)
    inter = (ix2 - ex1) * (iy2 - ey1) + (xmin - ex1) * (ymin - ey1) \
        - (ix1 - ex1) * (ymax - ey1) - (xmax - ex1) * (iy1 - ey1)
    union = (px2 - px1) * (py2 - py1) + (tx2 - tx1) * (ty2 - ty1) - inter + eps
    return 1 - inter / union


def eiou_forced(quad, smooth_point, eps):
    """eiou_loss with its branch given per row (ambiguous rows: the value of the other branch)."""
    def fn(pred, target):
        x = eiou_x(pred, target, eps)
        return torch.where(quad, 0.5 * (x ** 2) / smooth_point, x - 0.5 * smooth_point)
    return fn


def ciou_forced(gate, eps, alpha_grad=False):
    """ciou_loss with the alpha gate (ious > 0.5) given per row; alpha_grad lets alpha carry a gradient (a defect)."""
    def fn(pred, target):
        ious = ious_eps(pred, target, eps)
        e1 = torch.min(pred[:, :2], target[:, :2])
        e2 = torch.max(pred[:, 2:], target[:, 2:])
        ewh = (e2 - e1).clamp(min=0)
        c2 = ewh[:, 0] ** 2 + ewh[:, 1] ** 2 + eps
        w1, h1 = pred[:, 2] - pred[:, 0], pred[:, 3] - pred[:, 1] + eps
        w2, h2 = target[:, 2] - target[:, 0], target[:, 3] - target[:, 1] + eps
        left = ((target[:, 0] + target[:, 2]) - (pred[:, 0] + pred[:, 2])) ** 2 / 4
        right = ((target[:, 1] + target[:, 3]) - (pred[:, 1] + pred[:, 3])) ** 2 / 4
        v = (4 / math.pi ** 2) * torch.pow(torch.atan(w2 / h2) - torch.atan(w1 / h1), 2)
        if alpha_grad:
            alpha = gate.to(v.dtype) * v / (1 - ious + v)
        else:
            with torch.no_grad():
                alpha = gate.to(v.dtype) * v / (1 - ious + v)
        cious = ious - ((left + right) / c2 + alpha * v)
        return 1 - cious.clamp(min=-1.0, max=1.0)
    return fn


def sl1_forced(quad, beta):
    def fn(pred, target):
        d = (pred - target).abs()
        return torch.where(quad, 0.5 * d * d / beta, d - 0.5 * beta)
    return fn


# ------------------------------------------------------------------------------------------------ the reference
def loss_ref(flat, gt_inds, max_overlaps, gt_boxes, gt_kps, sizes, strides, cfg, num_total=None, kps_den=None,
             dtype=torch.float64, branches=None, hooks=None):
    """The four losses, dflat [N,P,16] and the per-prior terms of the fused loss step, in `dtype`.

    flat [N,P,16]; gt_inds [N,P] (1-based, 0 = negative); max_overlaps [N,P]; gt_boxes [N,Gmax,4]; gt_kps
    [N,Gmax,5,3] (or [N,Gmax,15]).  num_total: the (world-mean) positive count, None = this batch's; kps_den: the
    landmark normaliser, None = sum of the positives' mean visibility + fp32 eps.  branches: per-positive
    {'eiou_quad', 'ciou_gate', 'sl1_quad'} decisions to use instead of the computed ones (the other branch of an
    ambiguous element).  hooks: {'box_fn', 'kps_weight', 'kps_eps', 'priors'} replacements, for the checker's own
    rejection tests only.
    -> dict(losses [4] (cls, bbox, obj, kps), dflat, terms {cls, box, obj, kps: [N,P] before weight and normaliser},
            pos (n, p, g index tensors), sig_box [M,9], sig_kps [M,10], branches)."""
    hooks = hooks or {}
    N, P, _ = flat.shape
    Gmax = gt_boxes.shape[1]
    x = flat.detach().to(dtype).clone().requires_grad_(True)
    priors = hooks.get('priors')
    priors = (O.grid_priors(sizes, strides, dtype) if priors is None else priors).to(dtype)
    gi = gt_inds.long()
    pos = gi > 0
    n_idx, p_idx = pos.nonzero(as_tuple=True)           # row-major: O.loss_step's per-image ascending positives
    g_idx = gi[pos] - 1
    gb = gt_boxes.detach().to(dtype)[n_idx, g_idx]
    gk = gt_kps.detach().to(dtype).reshape(N, Gmax, 5, 3)[n_idx, g_idx]
    ovl = max_overlaps.detach().to(dtype)[pos]
    M = int(n_idx.numel())
    cls, box, obj, kps = x[..., 0], x[..., 1:5], x[..., 5], x[..., 6:]
    pri = priors[p_idx]
    decoded = O.bbox_decode(pri, box[n_idx, p_idx])
    # discrete decisions, in this dtype (the census; ambiguity between dtypes)
    with torch.no_grad():
        eps = cfg['box_eps']
        d = decoded.detach()
        x_e = eiou_x(d, gb, eps)
        iou_g = ious_eps(d, gb, eps)
        iou_a = O.aligned_iou(d, gb)[0]
        enc = O.kps_encode(pri, gk[:, :, :2].reshape(-1, 10))
        dk = kps.detach()[n_idx, p_idx] - enc
        own = {'eiou_quad': x_e < cfg['smooth_point'], 'ciou_gate': iou_g > 0.5,
               'sl1_quad': dk.abs() < cfg['kps_beta']}
        # edge ties | overlap width, height against 0 | EIoU quad | CIoU alpha gate | IoU clamped at eps
        sig_box = torch.cat([torch.sign(d - gb), torch.sign(_edges(d, gb)),
                             torch.stack([own['eiou_quad'], own['ciou_gate'], ~(iou_a >= eps)], 1).to(dtype)],
                            1).to(torch.int8)
        sig_kps = (torch.sign(dk) * torch.where(own['sl1_quad'], 1.0, 2.0)).to(torch.int8)
    br = dict(own)
    if branches:
        br.update(branches)
    kind = cfg['box_loss']
    box_fn = hooks.get('box_fn')
    if box_fn is None:
        if kind == 'EIoULoss' and branches and 'eiou_quad' in branches:
            box_fn = eiou_forced(br['eiou_quad'], cfg['smooth_point'], eps)
        elif kind == 'CIoULoss' and branches and 'ciou_gate' in branches:
            box_fn = ciou_forced(br['ciou_gate'], eps)
        else:
            box_fn = O.box_loss_fn(arch_of(cfg))
    nt = float(M) if num_total is None else float(num_total)
    nt = max(nt, 1.0)
    box_t = box_fn(decoded, gb)
    obj_t = F.binary_cross_entropy_with_logits(obj.reshape(-1), pos.reshape(-1).to(dtype), reduction='none')
    cls_t = F.binary_cross_entropy_with_logits(cls[pos], ovl, reduction='none')
    kps_w = hooks['kps_weight'](gk) if 'kps_weight' in hooks else gk[:, :, 2].mean(dim=1, keepdim=True)
    if branches and 'sl1_quad' in branches:
        sl1 = sl1_forced(br['sl1_quad'], cfg['kps_beta'])(kps[n_idx, p_idx], enc)
    else:
        sl1 = O.smooth_l1(kps[n_idx, p_idx], enc, cfg['kps_beta'])
    kps_t = sl1 * kps_w
    den = kps_w.sum() + hooks.get('kps_eps', F32_EPS) if kps_den is None else torch.tensor(float(kps_den), dtype=dtype)
    l_box = cfg['w_box'] * box_t.sum() / nt
    l_obj = cfg['w_obj'] * obj_t.sum() / nt
    l_cls = cfg['w_cls'] * cls_t.sum() / nt
    l_kps = cfg['w_kps'] * kps_t.sum() / den
    losses = torch.stack([l_cls, l_box, l_obj, l_kps])
    dflat, = torch.autograd.grad(losses.sum(), x, allow_unused=True)
    terms = {}
    for name, t in (('cls', cls_t), ('box', box_t), ('kps', kps_t.sum(1))):
        z = torch.zeros(N, P, dtype=dtype)
        z[n_idx, p_idx] = t.detach()
        terms[name] = z
    terms['obj'] = obj_t.detach().reshape(N, P)
    return dict(losses=losses.detach(), dflat=dflat.detach(), terms=terms, pos=(n_idx, p_idx, g_idx),
                sig_box=sig_box, sig_kps=sig_kps, branches=own, den=float(den), num_total=nt,
                weights=(cfg['w_cls'], cfg['w_box'], cfg['w_obj'], cfg['w_kps']))


def ref_of(case, cfg, **kw):
    return loss_ref(case['flat'], case['gt_inds'], case['max_overlaps'], case['gt_boxes'], case['gt_kps'],
                    case['sizes'], case['strides'], cfg, **kw)


# ---------------------------------------------------------------------------------------------------- census
def census(case, cfg=None, ref=None):
    """Per positive prior, each branch the loss kernel takes, counted (fp64 decisions)."""
    cfg = cfg or make_cfg()
    r = ref if ref is not None else ref_of(case, cfg)
    sb, sk = r['sig_box'].long(), r['sig_kps'].long()
    n_idx, p_idx, g_idx = r['pos']
    c = dict(pos=int(sb.shape[0]))
    c['eiou_quad'] = int((sb[:, 6] == 1).sum()); c['eiou_lin'] = c['pos'] - c['eiou_quad']
    c['ciou_alpha_on'] = int((sb[:, 7] == 1).sum()); c['ciou_alpha_off'] = c['pos'] - c['ciou_alpha_on']
    c['iou_eps_clamp'] = int((sb[:, 8] == 1).sum())
    c['overlap_pos'] = int((sb[:, 4:6] > 0).sum())
    c['overlap_zero'] = int((sb[:, 4:6] == 0).sum())
    c['overlap_neg'] = int((sb[:, 4:6] < 0).sum())
    c['edge_tie'] = int((sb[:, :4] == 0).sum())
    c['sl1_quad'] = int((sk.abs() == 1).sum())
    c['sl1_lin'] = int((sk.abs() == 2).sum())
    c['sl1_zero'] = int((sk == 0).sum())
    N, Gmax = case['gt_boxes'].shape[:2]
    vis = case['gt_kps'].reshape(N, Gmax, 5, 3)[n_idx, g_idx][:, :, 2].double().mean(1)
    for v in range(6):
        c[f'vis_{v / 5:.1f}'] = int(((vis * 5).round() == v).sum())
    bases = np.cumsum([0] + [h * w for h, w in case['sizes']])
    for lvl in range(len(case['sizes'])):
        c[f'level_{lvl}'] = int(((p_idx >= int(bases[lvl])) & (p_idx < int(bases[lvl + 1]))).sum())
    if c['pos']:
        d = O.bbox_decode(O.grid_priors(case['sizes'], case['strides'], torch.float64)[p_idx],
                          case['flat'].double()[n_idx, p_idx, 1:5])
        gb = case['gt_boxes'].double()[n_idx, g_idx]
        c['iou_max'] = round(float(O.aligned_iou(d, gb)[0].max()), 5)
    return c


# ---------------------------------------------------------------------------------------------------- checker
def perturb(case, gen):
    """The fp32 inputs each moved by one ulp, up or down (landmark visibility flags and the assignment stay)."""
    out = dict(case)

    def mv(t):
        t = t.float()
        s = torch.randint(0, 2, t.shape, generator=gen) * 2 - 1
        up = torch.nextafter(t, torch.full_like(t, math.inf))
        dn = torch.nextafter(t, torch.full_like(t, -math.inf))
        return torch.where(s > 0, up, dn)
    out['flat'] = mv(case['flat'])
    out['max_overlaps'] = mv(case['max_overlaps'])
    out['gt_boxes'] = mv(case['gt_boxes'])
    N, G = case['gt_boxes'].shape[:2]
    k = case['gt_kps'].reshape(N, G, 5, 3).clone().float()
    k[..., :2] = mv(k[..., :2])
    out['gt_kps'] = k
    return out


def default_blocks(N, P):
    return int(min(max(-(-N * P // LOSS_THREADS), 1), MAX_LOSS_BLOCKS))


class Report:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return (f'ok={self.ok} worst_ratio={self.worst:.3g} worst_loss_ratio={self.worst_loss:.3g} '
                f'loss_bar_rel={self.loss_rel_bar:.2g} '
                f'bad={self.n_bad} ambiguous={self.n_amb} unresolved={self.n_unres} {self.detail}')


def _listed(cfg):
    """columns of sig_box whose flip between precisions is a listed (resolvable) branch for this box loss"""
    return {'EIoULoss': [6], 'CIoULoss': [7]}.get(cfg['box_loss'], [])


def _quad_flip(a, b):
    """|d| against beta decided differently (d != 0 on both sides): the listed smooth-L1 ambiguity"""
    return (a.abs() != b.abs()) & (a != 0) & (b != 0)


def check(got_losses, got_dflat, case, cfg, num_total=None, kps_den=None, blocks=None, draws=4, seed=0, ref=None):
    """Grade a loss-kernel result (losses [4], dflat [N,P,16], fp32) against the fp64 reference.
    -> Report(ok, worst, worst_loss, loss_rel_bar, n_bad, n_pos, n_amb, n_unres, detail): worst / worst_loss are the
    largest error / bar ratios of dflat and of the four losses; loss_rel_bar the largest loss bar relative to its
    (non-zero) loss; n_amb the elements resolved against both branches of EIoU / CIoU / smooth-L1, n_unres those
    whose tie or clamp decision differs between fp32 and fp64 and which are graded against the fp32 restatement too."""
    kw = dict(num_total=num_total, kps_den=kps_den)
    r64 = ref if ref is not None else ref_of(case, cfg, **kw)
    r32 = ref_of(case, cfg, dtype=torch.float32, **kw)
    N, P, _ = case['flat'].shape
    M = r64['sig_box'].shape[0]
    n_idx, p_idx, _ = r64['pos']
    listed = _listed(cfg)
    other = [c for c in range(9) if c not in listed and c not in (6, 7)]
    # -- spread: the fp64 result under 1-ulp moves of the fp32 inputs, draws that change a prior's discrete path
    # left out for that prior's channels
    gen = torch.Generator().manual_seed(seed)
    spread = torch.zeros(N, P, 16, dtype=torch.float64)
    spread_t = {k: torch.zeros(N, P, dtype=torch.float64) for k in r64['terms']}
    amb_box = torch.zeros(M, dtype=torch.bool)
    amb_kps = torch.zeros(M, 10, dtype=torch.bool)
    for _ in range(draws):
        rd = ref_of(perturb(case, gen), cfg, **kw)
        flip_box = (rd['sig_box'] != r64['sig_box'])
        flip_kps = rd['sig_kps'] != r64['sig_kps']
        if listed:
            amb_box |= flip_box[:, listed].any(1)
        amb_kps |= _quad_flip(rd['sig_kps'], r64['sig_kps'])
        keep = torch.ones(N, P, 16, dtype=torch.bool)
        keep[n_idx, p_idx, 1:5] = ~flip_box[:, listed + other].any(1, keepdim=True).expand(M, 4)
        keep[n_idx, p_idx, 6:] = ~flip_kps
        diff = (rd['dflat'] - r64['dflat']).abs()
        spread = torch.where(keep, torch.maximum(spread, diff), spread)
        keep_t = {'cls': torch.ones(N, P, dtype=torch.bool), 'obj': torch.ones(N, P, dtype=torch.bool)}
        keep_t['box'] = keep[..., 1].clone()
        keep_t['kps'] = keep[..., 6:].all(-1)
        for k in spread_t:
            dt = (rd['terms'][k] - r64['terms'][k]).abs()
            spread_t[k] = torch.where(keep_t[k], torch.maximum(spread_t[k], dt), spread_t[k])
    # -- the fp32 restatement's own decisions
    f32_box = r32['sig_box'] != r64['sig_box']
    if listed:
        amb_box |= f32_box[:, listed].any(1)
    amb_kps |= _quad_flip(r32['sig_kps'], r64['sig_kps'])
    unres_box = f32_box[:, other].any(1) & ~amb_box
    unres_kps = (r32['sig_kps'] != r64['sig_kps']) & ~amb_kps
    # -- per-element bars
    f64, f32v = r64['dflat'], r32['dflat'].double()
    # the four box partials of a prior come out of one dual-number chain: a partial that cancels to (nearly) 0 in fp64
    # keeps the rounding of the chain's larger partials, so each carries the prior's largest
    floor = torch.full_like(f64, TINY)
    floor[..., 1:5] += ELEMENT_B * U32 * f64[..., 1:5].abs().amax(-1, keepdim=True)
    bar = ELEMENT_A * torch.maximum((f32v - f64).abs(), spread) + ELEMENT_B * U32 * f64.abs() + floor
    got = got_dflat.double()
    err = (got - f64).abs()
    ratio = err / bar
    amb_mask = torch.zeros(N, P, 16, dtype=torch.bool)
    amb_mask[n_idx, p_idx, 1:5] = amb_box[:, None].expand(M, 4)
    amb_mask[n_idx, p_idx, 6:] = amb_kps
    unres_mask = torch.zeros(N, P, 16, dtype=torch.bool)
    unres_mask[n_idx, p_idx, 1:5] = unres_box[:, None].expand(M, 4)
    unres_mask[n_idx, p_idx, 6:] = unres_kps
    alt = None
    if bool(amb_mask.any()):
        flipped = {k: v.clone() for k, v in r64['branches'].items()}
        if cfg['box_loss'] == 'EIoULoss':
            flipped['eiou_quad'] = flipped['eiou_quad'] ^ amb_box
        if cfg['box_loss'] == 'CIoULoss':
            flipped['ciou_gate'] = flipped['ciou_gate'] ^ amb_box
        flipped['sl1_quad'] = flipped['sl1_quad'] ^ amb_kps
        alt = ref_of(case, cfg, branches=flipped, **kw)
        amb_bar = lambda v: ELEMENT_A * spread + ELEMENT_B * U32 * v.abs() + floor   # noqa: E731
        r_a = torch.minimum(err / amb_bar(f64), (got - alt['dflat']).abs() / amb_bar(alt['dflat']))
        ratio = torch.where(amb_mask, r_a, ratio)
    if bool(unres_mask.any()):
        ub = lambda v: ELEMENT_A * spread + ELEMENT_B * U32 * v.abs() + floor   # noqa: E731
        r_u = torch.minimum(err / ub(f64), (got - f32v).abs() / ub(f32v))
        ratio = torch.where(unres_mask, r_u, ratio)
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    bad = ratio > 1.0
    # -- losses: the terms' bars summed, plus the reduction: elements per thread, 6 shuffle levels, 4 waves and the
    # weight / normaliser in fp32, the fp64 sum over blocks rounded to fp32, the deferred 1/num_total; the fp32
    # normaliser of the landmark term carries the rounding of the per-image and tree sums behind it
    blocks = blocks or default_blocks(N, P)
    ept = -(-N * P // (blocks * LOSS_THREADS))
    red = (ept + 6 + 3 + 2 + 3) * U32
    den_err = (math.ceil(math.log2(max(N, 2))) + 10) * U32
    names = ('cls', 'box', 'obj', 'kps')
    unres_prior = torch.zeros(N, P, dtype=torch.bool)
    unres_prior[n_idx, p_idx] = unres_box | unres_kps.any(1)
    loss_ratio, loss_rel_bar = [], []
    for i, k in enumerate(names):
        t64, t32 = r64['terms'][k], r32['terms'][k].double()
        tb = ELEMENT_A * torch.maximum((t32 - t64).abs(), spread_t[k]) + ELEMENT_B * U32 * t64.abs() + TINY
        if alt is not None:
            tb = tb + (alt['terms'][k] - t64).abs()
        if k in ('box', 'kps'):
            # an unresolved prior may sit on either side of its discrete decision: its term on the fp32 side counts
            tb = tb + torch.where(unres_prior, (t32 - t64).abs(), torch.zeros_like(t64))
        scale = r64['weights'][i] / (r64['den'] if k == 'kps' else r64['num_total'])
        lb = scale * (float(tb.sum()) + red * float(t64.abs().sum())) + abs(float(r64['losses'][i])) * den_err + TINY
        q = abs(float(got_losses[i]) - float(r64['losses'][i])) / lb
        loss_ratio.append(q if math.isfinite(q) else math.inf)          # a NaN loss is a failure, whatever max() says
        if float(r64['losses'][i]) != 0.0:
            loss_rel_bar.append(lb / abs(float(r64['losses'][i])))
    worst_loss = max(loss_ratio)
    nb = int(bad.sum())
    detail = ''
    if nb:
        idx = torch.nonzero(bad)[:3].tolist()
        detail = 'first bad (n,p,c): ' + '; '.join(
            f'{tuple(i)} got {float(got[tuple(i)]):.9g} ref {float(f64[tuple(i)]):.9g} bar {float(bar[tuple(i)]):.3g}'
            for i in idx)
    if worst_loss > 1.0:
        detail += f' losses got {[float(v) for v in got_losses]} ref {r64["losses"].tolist()} ratios {loss_ratio}'
    return Report(ok=nb == 0 and worst_loss <= 1.0, worst=float(ratio.max()) if ratio.numel() else 0.0,
                  worst_loss=worst_loss, loss_rel_bar=max(loss_rel_bar, default=0.0), n_bad=nb, n_pos=M, n_amb=int(amb_box.sum()) + int(amb_kps.sum()),
                  n_unres=int(unres_box.sum()) + int(unres_kps.sum()), detail=detail, ref=r64)


# ------------------------------------------------------------------------------------------ regime constructors
def _prior_table(sizes, strides):
    pri = O.grid_priors(sizes, strides, torch.float64)
    lvl = torch.cat([torch.full((h * w,), i) for i, (h, w) in enumerate(sizes)])
    return pri, lvl


def make_case(N, h, w, seed, boxes=('generic',), vis='fractional', logits='mixed', frac=0.12, strides=(8, 16, 32),
              edges=True):
    """A loss-kernel input batch whose positives reach the branches named.

    boxes: the box regimes mixed over the positives -- 'generic' (IoU ~0.3 .. 0.9999, both EIoU branches, both sides
    of the CIoU gate), 'tie' (a predicted edge equal to its GT edge to the last bit), 'touch' (overlap width or height
    exactly 0), 'disjoint' (negative overlap: IoU 0, the IoU-loss eps clamp), 'nested' (one box inside the other).
    Exact regimes use dw = dh = 0 (exp(0) = 1), dyadic dx / dy and power-of-two strides, so the decoded box and the GT
    edge are exact in fp32 and fp64 alike.  vis: 'fractional' (0, 0.2, .. 1 mean visibility), 'binary',
    'invisible' (every positive's landmarks invisible: kps_den = eps).  logits: 'mixed' (ordinary, saturated +-30 /
    +-100, and cls targets within a few ulps of sigmoid(x)) or 'plain'.  edges: positives on the first and last prior
    of every level.  -> dict(flat, gt_inds, max_overlaps, gt_boxes, gt_kps, img_stats, sizes, strides)."""
    gen = torch.Generator().manual_seed(seed)
    sizes = [(h // s, w // s) for s in strides]
    pri, lvl = _prior_table(sizes, strides)
    P = pri.shape[0]
    bases = np.cumsum([0] + [a * b for a, b in sizes])

    def rnd(*shape):
        return torch.rand(*shape, generator=gen, dtype=torch.float64)

    pos_lists = []
    for n in range(N):
        k = max(1, int(frac * P))
        p = torch.randperm(P, generator=gen)[:k]
        if edges:
            p = torch.cat([p, torch.tensor([int(bases[i]) for i in range(len(sizes))] +
                                           [int(bases[i + 1]) - 1 for i in range(len(sizes))])])
        pos_lists.append(torch.unique(p))
    Gmax = max(int(p.numel()) for p in pos_lists)
    flat = (torch.randn(N, P, 16, generator=gen, dtype=torch.float64) * 0.5).float()
    flat[..., 5] = (torch.randn(N, P, generator=gen) * 2.0 - 3.0).float()
    gt_inds = torch.zeros(N, P, dtype=torch.int32)
    ovl = torch.full((N, P), -100000.0)
    gt_boxes = torch.zeros(N, Gmax, 4)
    gt_kps = torch.zeros(N, Gmax, 5, 3)
    img_stats = torch.zeros(N, 2)
    for n in range(N):
        p = pos_lists[n]
        m = int(p.numel())
        s = pri[p, 2]
        px, py = pri[p, 0], pri[p, 1]
        kind = torch.randint(0, len(boxes), (m,), generator=gen)
        # generic: a noisy prediction, the GT its edges moved by log-uniform fractions of the box size
        dxy = (rnd(m, 2) * 2.0 - 0.5)
        dwh = torch.log(1.0 + 7.0 * rnd(m, 2))
        pred = torch.cat([dxy, dwh], 1).float()
        exact = torch.zeros(m, dtype=torch.bool)
        for j, b in enumerate(boxes):
            if b != 'generic':
                exact |= kind == j
        # exact regimes: dyadic offsets, unit size (exp(0) = 1)
        dy8 = (torch.randint(-4, 13, (m, 2), generator=gen).double() / 8.0).float()
        pred[exact, :2] = dy8[exact]
        pred[exact, 2:] = 0.0
        flat[n, p, 1:5] = pred
        dec = O.bbox_decode(pri[p], pred.double())                        # exact for the exact regimes
        bw, bh = dec[:, 2] - dec[:, 0], dec[:, 3] - dec[:, 1]
        frac_mv = torch.exp(math.log(1e-6) + (math.log(0.4) - math.log(1e-6)) * rnd(m, 4))
        sgn = torch.where(rnd(m, 4) < 0.5, -1.0, 1.0)
        size4 = torch.stack([bw, bh, bw, bh], 1)
        gt = dec + sgn * frac_mv * size4
        gt = torch.stack([torch.minimum(gt[:, 0], gt[:, 2] - 0.5), torch.minimum(gt[:, 1], gt[:, 3] - 0.5),
                          gt[:, 2], gt[:, 3]], 1)
        q = (torch.randint(1, 5, (m, 4), generator=gen).double() * s[:, None] / 4.0)   # dyadic moves
        for j, b in enumerate(boxes):
            sel = kind == j
            if b == 'tie':
                # one to four edges equal to the prediction's, the others moved by a dyadic amount
                tie = rnd(m, 4) < 0.5
                tie[:, 0] |= ~tie.any(1)
                # never all four: an exact match makes CIoU's alpha 0 / 0 in fp32 (1 - iou rounds to 0, v = 0) in
                # the reference as in the kernel, while fp64 stays finite
                tie[:, 3] &= ~tie[:, :3].all(1)
                mv = torch.where(sgn > 0, q, -q * 0.25)          # outward by up to s, inward by up to s / 4
                e = torch.where(tie, dec, dec + torch.tensor([[-1.0, -1.0, 1.0, 1.0]]) * mv)
                gt[sel] = e[sel]
            elif b == 'touch':
                # GT to the right of (or below) the prediction, sharing the edge: overlap width (height) exactly 0
                e = dec.clone()
                horiz = rnd(m) < 0.5
                e[:, 0] = torch.where(horiz, dec[:, 2], dec[:, 0] - q[:, 0])
                e[:, 2] = torch.where(horiz, dec[:, 2] + s, dec[:, 2] + q[:, 2])
                e[:, 1] = torch.where(horiz, dec[:, 1] - q[:, 1], dec[:, 3])
                e[:, 3] = torch.where(horiz, dec[:, 3] + q[:, 3], dec[:, 3] + s)
                gt[sel] = e[sel]
            elif b == 'disjoint':
                e = dec.clone()
                e[:, 0] = dec[:, 2] + q[:, 0]
                e[:, 2] = e[:, 0] + s
                e[:, 1] = dec[:, 1] - q[:, 1]
                e[:, 3] = dec[:, 3] + q[:, 3]
                gt[sel] = e[sel]
            elif b == 'nested':
                inner = rnd(m) < 0.5
                e = torch.where(inner[:, None], dec + torch.tensor([[1.0, 1.0, -1.0, -1.0]]) * q / 8.0,
                                dec + torch.tensor([[-1.0, -1.0, 1.0, 1.0]]) * q)
                gt[sel] = e[sel]
        gt_boxes[n, :m] = gt.float()
        gt_inds[n, p] = torch.arange(1, m + 1, dtype=torch.int32)
        # landmarks: dyadic targets half the time (exact encodings), d = 0 | quad | linear per coordinate
        beta = _f32(1.0 / 9.0)
        dy_t = torch.randint(-16, 33, (m, 10), generator=gen).double() / 16.0
        rn_t = (rnd(m, 10) * 3.0 - 1.0).float().double()
        use_dy = rnd(m, 1) < 0.5
        enc = torch.where(use_dy, dy_t, rn_t)
        kxy = enc.reshape(m, 5, 2) * s[:, None, None] + torch.stack([px, py], 1)[:, None, :]
        gt_kps[n, :m, :, :2] = kxy.float()
        enc32 = O.kps_encode(pri[p].float(), gt_kps[n, :m, :, :2].reshape(m, 10))
        mode = torch.randint(0, 3, (m, 10), generator=gen)
        mag = torch.where(mode == 1, beta * (0.02 + 0.86 * rnd(m, 10)), beta * 1.15 + 2.5 * rnd(m, 10))
        dd = torch.where(mode == 0, 0.0, mag * torch.where(rnd(m, 10) < 0.5, -1.0, 1.0))
        flat[n, p, 6:] = (enc32.double() + dd).float()
        flat[n, p, 6:] = torch.where(mode == 0, enc32, flat[n, p, 6:])
        if vis == 'fractional':
            nv = torch.randint(0, 6, (m,), generator=gen)
        elif vis == 'binary':
            nv = torch.where(rnd(m) < 0.7, 5, 0)
        else:
            nv = torch.zeros(m, dtype=torch.long)
        order = torch.argsort(rnd(m, 5), 1)
        flags = (order < nv[:, None]).float()
        gt_kps[n, :m, :, 2] = flags
        # logits and soft targets
        t = (0.05 + 0.949 * rnd(m)).float()
        xc = (torch.randn(m, generator=gen, dtype=torch.float64) * 1.5 + 0.5).float()
        xo = (torch.randn(m, generator=gen, dtype=torch.float64) * 2.0 + 1.0).float()
        if logits == 'mixed':
            sat = torch.tensor([30.0, -30.0, 100.0, -100.0])
            r = rnd(m)
            which = torch.randint(0, 4, (m,), generator=gen)
            xc = torch.where(r < 0.1, sat[which], xc)
            xo = torch.where(r > 0.9, sat[which], xo)
            # cls target within a few ulps of sigmoid(x): the cancellation of a trained head
            canc = (r >= 0.1) & (r < 0.3)
            sg = torch.sigmoid(xc.double()).float()
            k = torch.randint(-3, 4, (m,), generator=gen)
            tc = sg.clone()
            for step in range(3):
                tc = torch.where(k > step, torch.nextafter(tc, torch.ones_like(tc)), tc)
                tc = torch.where(k < -step, torch.nextafter(tc, torch.zeros_like(tc)), tc)
            t = torch.where(canc & (sg > 0.01) & (sg < 0.99), tc, t)
            neg = ~torch.zeros(P, dtype=torch.bool).index_fill_(0, p, True)
            nneg = int(neg.sum())
            rn = rnd(nneg)
            on = flat[n, neg, 5]
            on = torch.where(rn < 0.05, torch.tensor(-100.0), torch.where(rn < 0.1, torch.tensor(30.0), on))
            flat[n, neg, 5] = on
        flat[n, p, 0] = xc
        flat[n, p, 5] = xo
        ovl[n, p] = t
        img_stats[n, 0] = float(m)
        img_stats[n, 1] = float(flags.double().mean(1).sum())
    return dict(flat=flat.contiguous(), gt_inds=gt_inds, max_overlaps=ovl, gt_boxes=gt_boxes,
                gt_kps=gt_kps.contiguous(), img_stats=img_stats, sizes=sizes, strides=list(strides))
