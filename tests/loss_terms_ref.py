"""fp64 / fp32 restatement of the loss terms beyond the default selection, and their per-element grading.

The kernel under test is loss_terms_kernel of libfacedetection.train_amd/csrc/loss_step.hip (entry yunet_loss_terms):
VarifocalLoss on loss_cls / loss_obj, L1Loss / MSELoss / BalancedL1Loss on loss_kps, BoundedIoULoss on loss_bbox, each
beside the default terms of tests/loss_ref.py.  `terms_ref` is loss_ref.loss_ref with the term functions chosen by the
configuration; its gradient is torch autograd.  In float64 it is the yardstick, pinned to the reference's own modules by
tests/golden/loss_terms_cases.npz (tools/make_golden_loss_terms.py).

`check` grades with the rule and the constants of loss_ref.check:
    bar = ELEMENT_A * max(|fp32 restatement - fp64|, spread under 1-ulp input moves) + ELEMENT_B * U32 * |fp64| + floor
per element of dflat, and the four losses with the sum of their terms' bars plus the reduction's rounding.  What it adds
is the bookkeeping of the new branch points.  Every discrete decision behind an element is a column of a *group*:
    cls_neg     varifocal's t <= 0 side (loss_cls; on loss_obj t comes from the assignment and cannot move)
    box_first   bounded-IoU: the centre terms' max(., 0) clamp | the width / height terms' side of the min
    box_smooth  bounded-IoU: component < beta
    eiou_quad, ciou_gate, box_other   the default box losses' decisions, as loss_ref has them
    kps_quad    smooth-L1 / balanced-L1: |d| < beta;   kps_sign  sign of d
A forcible group's decision that flips under a 1-ulp move of the inputs, or between fp32 and fp64, makes its elements
ambiguous: they are graded against the fp64 value of both sides, and the prior's term enters the loss's reference on the
side its gradient took.  Flips of the other groups (ties, signs) are graded against fp64 and the fp32 restatement.  No
element is left out."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import yunet_oracle as O
import loss_ref as LR
from loss_ref import ELEMENT_A, ELEMENT_B, TINY, U32, F32_EPS, _f32

CLS_DEFAULT = dict(type='CrossEntropyLoss')
KPS_DEFAULT = dict(type='SmoothL1Loss')


def _spec(spec, default):
    spec = dict(default if spec is None else (dict(type=spec) if isinstance(spec, str) else spec))
    if spec['type'] == 'VarifocalLoss':
        spec = dict(type='VarifocalLoss', alpha=_f32(spec.get('alpha', 0.75)), gamma=_f32(spec.get('gamma', 2.0)),
                    iou_weighted=bool(spec.get('iou_weighted', True)))
    elif spec['type'] == 'BalancedL1Loss':
        spec = dict(type='BalancedL1Loss', alpha=_f32(spec.get('alpha', 0.5)), gamma=_f32(spec.get('gamma', 1.5)))
    return spec


def make_cfg(loss_cls=None, loss_obj=None, loss_kps=None, box_loss='EIoULoss', box_mode=None, box_eps=None,
             smooth_point=None, kps_beta=1.0 / 9.0, **weights):
    """loss_ref.make_cfg plus the terms' specs (type name or dict(type=, alpha=, gamma=, iou_weighted=)), parameters
    rounded to the fp32 values the kernel receives.  BoundedIoULoss: smooth_point is its beta (0.2), box_eps its eps (1e-3)."""
    bounded = box_loss == 'BoundedIoULoss'
    c = LR.make_cfg('EIoULoss' if bounded else box_loss, box_mode,
                    box_eps=(1e-3 if bounded else 1e-6) if box_eps is None else box_eps,
                    smooth_point=(0.2 if bounded else 0.1) if smooth_point is None else smooth_point, kps_beta=kps_beta,
                    **weights)
    c['box_loss'] = box_loss
    c['cls'], c['obj'], c['kps'] = _spec(loss_cls, CLS_DEFAULT), _spec(loss_obj, CLS_DEFAULT), _spec(loss_kps, KPS_DEFAULT)
    return c


def kernel_cfg(cfg, defer=False):
    """-> (YunetLossCfg, YunetLossTerms) of a make_cfg dict."""
    import yunet_amd.kernels as k
    t = k.make_loss_terms(cfg['cls'], cfg['obj'], cfg['kps'])
    c = k.make_loss_cfg(cfg['box_loss'], w_cls=cfg['w_cls'], w_box=cfg['w_box'], w_obj=cfg['w_obj'], w_kps=cfg['w_kps'],
                        box_eps=cfg['box_eps'], smooth_point=cfg['smooth_point'], kps_beta=cfg['kps_beta'],
                        box_mode=cfg['box_mode'], terms=t)
    c.defer_num_total = 1 if defer else 0
    return c, t


# ------------------------------------------------------------------------------------------------ the term functions
def varifocal(x, t, alpha, gamma, iou_weighted, neg=None):
    """varifocal_loss (varifocal_loss.py:41-54), element-wise.  neg: the t <= 0 decision to use instead of the own one."""
    if neg is None:
        pos_m, neg_m = (t > 0.0).to(x.dtype), (t <= 0.0).to(x.dtype)
    else:
        neg_m = neg.to(x.dtype)
        pos_m = 1.0 - neg_m
    fw = (t * pos_m if iou_weighted else pos_m) + alpha * (x.sigmoid() - t).abs().pow(gamma) * neg_m
    return F.binary_cross_entropy_with_logits(x, t, reduction='none') * fw


def kps_elementwise(kind, d, beta, alpha=0.5, gamma=1.5, quad=None):
    """l1_loss / mse_loss / smooth_l1_loss / balanced_l1_loss of d = pred - target, element-wise."""
    diff = d.abs()
    if kind == 'L1Loss':
        return diff
    if kind == 'MSELoss':
        return d * d
    q = (diff < beta) if quad is None else quad
    if kind == 'SmoothL1Loss':
        return torch.where(q, 0.5 * diff * diff / beta, diff - 0.5 * beta)
    b = math.e ** (gamma / alpha) - 1
    return torch.where(q, alpha / b * (b * diff + 1) * torch.log(b * diff / beta + 1) - alpha * diff,
                       gamma * diff + gamma / b - alpha * beta)


def bounded_iou(pred, target, beta, eps, first=None, smooth=None):
    """bounded_iou_loss (iou_loss.py:55-97) -> ([M,4] element-wise loss, its decisions first [M,4], smooth [M,4]).
    first: centre terms ratio > 0 (not clamped) | size terms target / pred is the smaller ratio.  With `first` /
    `smooth` given, those sides are taken instead of the own ones."""
    pcx, pcy = (pred[:, 0] + pred[:, 2]) * 0.5, (pred[:, 1] + pred[:, 3]) * 0.5
    pw, ph = pred[:, 2] - pred[:, 0], pred[:, 3] - pred[:, 1]
    tcx, tcy = (target[:, 0] + target[:, 2]) * 0.5, (target[:, 1] + target[:, 3]) * 0.5
    tw, th = target[:, 2] - target[:, 0], target[:, 3] - target[:, 1]
    dx, dy = tcx - pcx, tcy - pcy
    rx = (tw - 2 * dx.abs()) / (tw + 2 * dx.abs() + eps)
    ry = (th - 2 * dy.abs()) / (th + 2 * dy.abs() + eps)
    aw, bw = tw / (pw + eps), pw / (tw + eps)
    ah, bh = th / (ph + eps), ph / (th + eps)
    own_first = torch.stack([rx > 0, ry > 0, aw < bw, ah < bh], 1).detach()
    if first is None:
        ldx, ldy = 1 - torch.max(rx, torch.zeros_like(rx)), 1 - torch.max(ry, torch.zeros_like(ry))
        ldw, ldh = 1 - torch.min(aw, bw), 1 - torch.min(ah, bh)
    else:
        z = torch.zeros_like(rx)
        ldx, ldy = 1 - torch.where(first[:, 0], rx, z), 1 - torch.where(first[:, 1], ry, z)
        ldw, ldh = 1 - torch.where(first[:, 2], aw, bw), 1 - torch.where(first[:, 3], ah, bh)
    comb = torch.stack([ldx, ldy, ldw, ldh], dim=-1)
    own_smooth = (comb < beta).detach()
    sm = own_smooth if smooth is None else smooth
    return torch.where(sm, 0.5 * comb * comb / beta, comb - 0.5 * beta), own_first, own_smooth


# ------------------------------------------------------------------------------------------------ the reference
def terms_ref(flat, gt_inds, max_overlaps, gt_boxes, gt_kps, sizes, strides, cfg, num_total=None, kps_den=None,
              dtype=torch.float64, forced=None):
    """loss_ref.loss_ref with the terms of `cfg` (make_cfg).  forced: {group name: bool [M,k]} decisions to take instead
    of the computed ones.  -> loss_ref's dict plus groups: [dict(name, val int8 [M,k], chans [k lists of dflat channels],
    forcible)]."""
    forced = forced or {}
    N, P, _ = flat.shape
    Gmax = gt_boxes.shape[1]
    x = flat.detach().to(dtype).clone().requires_grad_(True)
    priors = O.grid_priors(sizes, strides, dtype).to(dtype)
    gi = gt_inds.long()
    pos = gi > 0
    n_idx, p_idx = pos.nonzero(as_tuple=True)
    g_idx = gi[pos] - 1
    gb = gt_boxes.detach().to(dtype)[n_idx, g_idx]
    gk = gt_kps.detach().to(dtype).reshape(N, Gmax, 5, 3)[n_idx, g_idx]
    ovl = max_overlaps.detach().to(dtype)[pos]
    M = int(n_idx.numel())
    cls, box, obj, kps = x[..., 0], x[..., 1:5], x[..., 5], x[..., 6:]
    pri = priors[p_idx]
    decoded = O.bbox_decode(pri, box[n_idx, p_idx])
    enc = O.kps_encode(pri, gk[:, :, :2].reshape(-1, 10))
    groups = []

    def group(name, val, chans, forcible):
        groups.append(dict(name=name, val=val.detach().reshape(M, -1).to(torch.int8), chans=chans, forcible=forcible))

    # ---- cls
    cs = cfg['cls']
    if cs['type'] == 'VarifocalLoss':
        cls_t = varifocal(cls[pos], ovl, cs['alpha'], cs['gamma'], cs['iou_weighted'],
                          forced['cls_neg'].reshape(M) if 'cls_neg' in forced else None)
        group('cls_neg', ovl <= 0.0, [[0]], True)
    else:
        cls_t = F.binary_cross_entropy_with_logits(cls[pos], ovl, reduction='none')
    # ---- obj (its target is the assignment: no decision can move)
    os_ = cfg['obj']
    t_obj = pos.reshape(-1).to(dtype)
    if os_['type'] == 'VarifocalLoss':
        obj_t = varifocal(obj.reshape(-1), t_obj, os_['alpha'], os_['gamma'], os_['iou_weighted'])
    else:
        obj_t = F.binary_cross_entropy_with_logits(obj.reshape(-1), t_obj, reduction='none')
    # ---- box
    eps, kind = cfg['box_eps'], cfg['box_loss']
    if kind == 'BoundedIoULoss':
        b4, first, smooth = bounded_iou(decoded, gb, cfg['smooth_point'], eps, forced.get('box_first'), forced.get('box_smooth'))
        box_t = b4.sum(1)
        per_chan = [[1], [2], [3], [4]]
        group('box_first', first, per_chan, True)
        group('box_smooth', smooth, per_chan, True)
    else:
        with torch.no_grad():
            d = decoded.detach()
            quad, gate = LR.eiou_x(d, gb, eps) < cfg['smooth_point'], LR.ious_eps(d, gb, eps) > 0.5
            other = torch.cat([torch.sign(d - gb), torch.sign(LR._edges(d, gb)),
                               (~(O.aligned_iou(d, gb)[0] >= eps)).to(dtype)[:, None]], 1)
        allc = [1, 2, 3, 4]
        if kind == 'EIoULoss':
            box_fn = LR.eiou_forced(forced['eiou_quad'].reshape(M), cfg['smooth_point'], eps) if 'eiou_quad' in forced \
                else O.box_loss_fn(LR.arch_of(cfg))
            group('eiou_quad', quad, [allc], True)
        elif kind == 'CIoULoss':
            box_fn = LR.ciou_forced(forced['ciou_gate'].reshape(M), eps) if 'ciou_gate' in forced \
                else O.box_loss_fn(LR.arch_of(cfg))
            group('ciou_gate', gate, [allc], True)
        else:
            box_fn = O.box_loss_fn(LR.arch_of(cfg))
        group('box_other', other, [allc] * 7, False)
        box_t = box_fn(decoded, gb)
    # ---- kps
    ks = cfg['kps']
    dk = kps[n_idx, p_idx] - enc
    has_quad = ks['type'] in ('SmoothL1Loss', 'BalancedL1Loss')
    kl = kps_elementwise(ks['type'], dk, cfg['kps_beta'], ks.get('alpha', 0.5), ks.get('gamma', 1.5),
                         forced.get('kps_quad') if has_quad else None)
    kch = [[6 + j] for j in range(10)]
    if has_quad:
        group('kps_quad', dk.detach().abs() < cfg['kps_beta'], kch, True)
    group('kps_sign', torch.sign(dk.detach()), kch, False)
    kps_w = gk[:, :, 2].mean(dim=1, keepdim=True)
    kps_t = kl * kps_w
    den = kps_w.sum() + F32_EPS if kps_den is None else torch.tensor(float(kps_den), dtype=dtype)
    nt = max(float(M) if num_total is None else float(num_total), 1.0)
    losses = torch.stack([cfg['w_cls'] * cls_t.sum() / nt, cfg['w_box'] * box_t.sum() / nt,
                          cfg['w_obj'] * obj_t.sum() / nt, cfg['w_kps'] * kps_t.sum() / den])
    dflat, = torch.autograd.grad(losses.sum(), x, allow_unused=True)
    terms = {}
    for name, t in (('cls', cls_t), ('box', box_t), ('kps', kps_t.sum(1))):
        z = torch.zeros(N, P, dtype=dtype)
        z[n_idx, p_idx] = t.detach()
        terms[name] = z
    terms['obj'] = obj_t.detach().reshape(N, P)
    return dict(losses=losses.detach(), dflat=dflat.detach(), terms=terms, pos=(n_idx, p_idx, g_idx), groups=groups,
                den=float(den), num_total=nt, weights=(cfg['w_cls'], cfg['w_box'], cfg['w_obj'], cfg['w_kps']))


def ref_of(case, cfg, **kw):
    return terms_ref(case['flat'], case['gt_inds'], case['max_overlaps'], case['gt_boxes'], case['gt_kps'],
                     case['sizes'], case['strides'], cfg, **kw)


# ---------------------------------------------------------------------------------------------------- census
def census(case, cfg, ref=None):
    """Elements on each side of every decision of `cfg`'s terms (fp64 decisions), plus the inputs the new terms need:
    positives with max_overlaps == 0, saturated logits, landmark differences of exactly 0."""
    r = ref if ref is not None else ref_of(case, cfg)
    n_idx, p_idx, _ = r['pos']
    c = dict(pos=int(n_idx.numel()))
    for g in r['groups']:
        v = g['val'].long()
        if g['name'] == 'box_first':
            c['bounded_clamped'], c['bounded_unclamped'] = int((v[:, :2] == 0).sum()), int((v[:, :2] == 1).sum())
            c['bounded_min_target_over_pred'], c['bounded_min_pred_over_target'] = int((v[:, 2:] == 1).sum()), int((v[:, 2:] == 0).sum())
        elif g['name'] == 'box_smooth':
            c['bounded_quad'], c['bounded_lin'] = int((v == 1).sum()), int((v == 0).sum())
        elif g['name'] == 'cls_neg':
            c['vfl_cls_neg'], c['vfl_cls_pos'] = int((v == 1).sum()), int((v == 0).sum())
        elif g['name'] == 'kps_quad':
            c['kps_quad'], c['kps_lin'] = int((v == 1).sum()), int((v == 0).sum())
        elif g['name'] == 'kps_sign':
            c['kps_zero'] = int((v == 0).sum())
    gi = case['gt_inds'].long() > 0
    c['vfl_obj_neg'], c['vfl_obj_pos'] = int((~gi).sum()), int(gi.sum())
    c['ovl_zero'] = int((case['max_overlaps'][gi] == 0).sum())
    c['cls_logit_sat'] = int((case['flat'][..., 0][gi].abs() >= 30).sum())
    c['obj_logit_sat'] = int((case['flat'][..., 5].abs() >= 30).sum())
    return c


# ---------------------------------------------------------------------------------------------------- checker
def _chan_mask(N, P, pos, colmask, chans):
    """[M,k] flags of a group -> [N,P,16] flags of the dflat elements its columns decide."""
    n_idx, p_idx, _ = pos
    m = torch.zeros(N, P, 16, dtype=torch.bool)
    for j, ch in enumerate(chans):
        for c in ch:
            m[n_idx, p_idx, c] |= colmask[:, j]
    return m


def check(got_losses, got_dflat, case, cfg, num_total=None, kps_den=None, blocks=None, draws=4, seed=0, ref=None):
    """loss_ref.check for the terms of `cfg`: -> loss_ref.Report (n_amb / n_unres count dflat elements; n_dec = the
    number of decision columns of the case)."""
    kw = dict(num_total=num_total, kps_den=kps_den)
    r64 = ref if ref is not None else ref_of(case, cfg, **kw)
    r32 = ref_of(case, cfg, dtype=torch.float32, **kw)
    N, P, _ = case['flat'].shape
    pos = r64['pos']
    n_idx, p_idx, _ = pos
    M = int(n_idx.numel())
    G = r64['groups']
    gen = torch.Generator().manual_seed(seed)
    spread = torch.zeros(N, P, 16, dtype=torch.float64)
    spread_t = {k: torch.zeros(N, P, dtype=torch.float64) for k in r64['terms']}
    amb = [torch.zeros_like(g['val'], dtype=torch.bool) for g in G]       # forcible groups: columns to take both sides of
    oth = [torch.zeros_like(g['val'], dtype=torch.bool) for g in G]       # the other groups: fp32 decided differently
    term_of = lambda m: {'cls': m[..., 0], 'box': m[..., 1:5].any(-1), 'obj': m[..., 5], 'kps': m[..., 6:].any(-1)}  # noqa: E731
    for _ in range(draws):
        rd = ref_of(LR.perturb(case, gen), cfg, **kw)
        moved = torch.zeros(N, P, 16, dtype=torch.bool)
        for i, (g, gd) in enumerate(zip(G, rd['groups'])):
            flip = gd['val'] != g['val']
            if g['forcible']:
                amb[i] |= flip
            moved |= _chan_mask(N, P, pos, flip, g['chans'])
        spread = torch.where(~moved, torch.maximum(spread, (rd['dflat'] - r64['dflat']).abs()), spread)
        mt = term_of(moved)
        for k in spread_t:
            dt = (rd['terms'][k] - r64['terms'][k]).abs()
            spread_t[k] = torch.where(~mt[k], torch.maximum(spread_t[k], dt), spread_t[k])
    for i, (g, g32) in enumerate(zip(G, r32['groups'])):
        flip = g32['val'] != g['val']
        (amb if g['forcible'] else oth)[i] |= flip
    amb_mask = torch.zeros(N, P, 16, dtype=torch.bool)
    unres_mask = torch.zeros(N, P, 16, dtype=torch.bool)
    for i, g in enumerate(G):
        amb_mask |= _chan_mask(N, P, pos, amb[i], g['chans'])
        unres_mask |= _chan_mask(N, P, pos, oth[i], g['chans'])
    unres_mask &= ~amb_mask
    f64, f32v = r64['dflat'], r32['dflat'].double()
    floor = torch.full_like(f64, TINY)
    if cfg['box_loss'] != 'BoundedIoULoss':        # (bounded-IoU's four partials are four separate chains)
        floor[..., 1:5] += ELEMENT_B * U32 * f64[..., 1:5].abs().amax(-1, keepdim=True)
    bar = ELEMENT_A * torch.maximum((f32v - f64).abs(), spread) + ELEMENT_B * U32 * f64.abs() + floor
    got = got_dflat.double()
    err = (got - f64).abs()
    ratio = err / bar
    either = lambda v: ELEMENT_A * spread + ELEMENT_B * U32 * v.abs() + floor   # noqa: E731
    alt = None
    if bool(amb_mask.any()):
        forced = {g['name']: g['val'].bool() ^ amb[i] for i, g in enumerate(G) if g['forcible']}
        alt = ref_of(case, cfg, forced=forced, **kw)
        r_own, r_alt = err / either(f64), (got - alt['dflat']).abs() / either(alt['dflat'])
        ratio = torch.where(amb_mask, torch.minimum(r_own, r_alt), ratio)
        # which side the result took, per term and prior: its loss is graded against the sum over those sides
        took_alt, took_own = term_of(amb_mask & (r_alt < r_own)), term_of(amb_mask & ~(r_alt < r_own))
    if bool(unres_mask.any()):
        r_u = torch.minimum(err / either(f64), (got - f32v).abs() / either(f32v))
        ratio = torch.where(unres_mask, r_u, ratio)
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    bad = ratio > 1.0
    # ---- losses (loss_ref.check's bar)
    blocks = blocks or LR.default_blocks(N, P)
    ept = -(-N * P // (blocks * LR.LOSS_THREADS))
    red = (ept + 6 + 3 + 2 + 3) * U32
    den_err = (math.ceil(math.log2(max(N, 2))) + 10) * U32
    unres_t = term_of(unres_mask)
    loss_ratio, loss_rel_bar = [], []
    for i, k in enumerate(('cls', 'box', 'obj', 'kps')):
        t64, t32 = r64['terms'][k], r32['terms'][k].double()
        tb = ELEMENT_A * torch.maximum((t32 - t64).abs(), spread_t[k]) + ELEMENT_B * U32 * t64.abs() + TINY
        scale = r64['weights'][i] / (r64['den'] if k == 'kps' else r64['num_total'])
        want = float(r64['losses'][i])
        if alt is not None:
            # an ambiguous prior counts with the side its gradient took (loss_ref.check widens the bar by both sides'
            # difference instead; with max_overlaps == 0 positives that difference is the whole term); a prior whose
            # elements took different sides widens the bar as there
            delta = alt['terms'][k] - t64
            want += scale * float(delta[took_alt[k] & ~took_own[k]].sum())
            tb = tb + torch.where(took_alt[k] & took_own[k], delta.abs(), torch.zeros_like(t64))
        tb = tb + torch.where(unres_t[k], (t32 - t64).abs(), torch.zeros_like(t64))
        lb = scale * (float(tb.sum()) + red * float(t64.abs().sum())) + abs(float(r64['losses'][i])) * den_err + TINY
        q = abs(float(got_losses[i]) - want) / lb
        loss_ratio.append(q if math.isfinite(q) else math.inf)
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
    return LR.Report(ok=nb == 0 and worst_loss <= 1.0, worst=float(ratio.max()) if ratio.numel() else 0.0,
                     worst_loss=worst_loss, loss_rel_bar=max(loss_rel_bar, default=0.0), n_bad=nb, n_pos=M,
                     n_amb=int(amb_mask.sum()), n_unres=int(unres_mask.sum()), detail=detail, ref=r64,
                     n_dec=sum(int(g['val'].numel()) for g in G if g['forcible']),
                     amb_cols=sum(int(a.sum()) for a in amb))


# ------------------------------------------------------------------------------------------ the case constructor
def make_case(N, h, w, seed):
    """loss_ref.make_case (generic boxes, mixed logits: saturated +-30 / +-100, d == 0 landmarks, differences on both
    sides of 1/9, 0.3 and 1.0) moved onto the new branch points: every fourth positive has max_overlaps == 0 (varifocal's
    t <= 0 side on loss_cls), every fifth a GT centre beyond half the GT's size from the predicted centre in x, y or both
    (bounded-IoU's clamp), every fifth a GT 0.4 .. 2.5 times the predicted size (both sides of the min, components on
    both sides of beta = 0.2 and 0.05)."""
    case = LR.make_case(N, h, w, seed, boxes=('generic',), logits='mixed')
    gen = torch.Generator().manual_seed(seed + 7919)
    pri = O.grid_priors(case['sizes'], case['strides'], torch.float64)
    gi = case['gt_inds'].long()
    for n in range(N):
        p = (gi[n] > 0).nonzero().flatten()
        g = gi[n, p] - 1
        m = int(p.numel())
        dec = O.bbox_decode(pri[p], case['flat'][n, p, 1:5].double())
        bw, bh = dec[:, 2] - dec[:, 0], dec[:, 3] - dec[:, 1]
        k = torch.arange(m)
        u = torch.rand(m, 4, generator=gen, dtype=torch.float64)
        gt = case['gt_boxes'][n, g].double()
        far = (k % 5) == 1
        sx = torch.where(u[:, 0] < 0.5, -1.0, 1.0) * (0.55 + u[:, 1]) * (gt[:, 2] - gt[:, 0]) * (k % 3 != 0)
        sy = torch.where(u[:, 2] < 0.5, -1.0, 1.0) * (0.55 + u[:, 3]) * (gt[:, 3] - gt[:, 1]) * (k % 3 != 1)
        shifted = gt + torch.stack([sx, sy, sx, sy], 1)
        scale = (k % 5) == 3
        fw, fh = torch.exp((u[:, 0] * 2 - 1) * math.log(2.5)), torch.exp((u[:, 2] * 2 - 1) * math.log(2.5))
        cx, cy = (dec[:, 0] + dec[:, 2]) / 2 + (u[:, 1] - 0.5) * 0.2 * bw, (dec[:, 1] + dec[:, 3]) / 2 + (u[:, 3] - 0.5) * 0.2 * bh
        scaled = torch.stack([cx - bw * fw / 2, cy - bh * fh / 2, cx + bw * fw / 2, cy + bh * fh / 2], 1)
        gt = torch.where(far[:, None], shifted, torch.where(scale[:, None], scaled, gt))
        case['gt_boxes'][n, g] = gt.float()
        ovl = case['max_overlaps'][n, p]
        case['max_overlaps'][n, p] = torch.where((k % 4) == 2, torch.zeros_like(ovl), ovl)
    return case


# ------------------------------------------------------------------------------ the committed cases (tests/golden)
def _vfl(alpha, gamma, iw):
    return dict(type='VarifocalLoss', alpha=alpha, gamma=gamma, iou_weighted=iw)


# name -> make_cfg arguments: what tools/make_golden_loss_terms.py runs the reference's modules on, and the tests the
# restatement and the kernel
GOLDEN_CONFIGS = {f'vfl_a{a}_g{g}_iw{int(iw)}': dict(loss_cls=_vfl(a, g, iw), loss_obj=_vfl(a, g, iw))
                  for a in (0.75, 0.5) for g in (2.0, 1.5) for iw in (True, False)}
GOLDEN_CONFIGS.update({
    'l1': dict(loss_kps='L1Loss'),
    'mse': dict(loss_kps='MSELoss'),
    'bl1_b1.0': dict(loss_kps=dict(type='BalancedL1Loss', alpha=0.5, gamma=1.5), kps_beta=1.0),
    'bl1_b0.3': dict(loss_kps=dict(type='BalancedL1Loss', alpha=0.5, gamma=1.5), kps_beta=0.3),
    'bounded_b0.2': dict(box_loss='BoundedIoULoss', smooth_point=0.2, box_eps=1e-3),
    'bounded_b0.05': dict(box_loss='BoundedIoULoss', smooth_point=0.05, box_eps=1e-3),
    'mixed': dict(loss_cls=_vfl(0.75, 2.0, True), loss_obj=_vfl(0.75, 2.0, True),
                  loss_kps=dict(type='BalancedL1Loss', alpha=0.5, gamma=1.5), kps_beta=0.3,
                  box_loss='BoundedIoULoss', smooth_point=0.2, box_eps=1e-3),
})
GOLDEN_CASE = (3, 64, 96, 11)          # make_case arguments: P = 126
# the reference head's own loss() (2 images, 64 x 64): bbox_head settings per case
HEAD_CONFIGS = {
    'mixed': dict(loss_cls=dict(type='VarifocalLoss', use_sigmoid=True, alpha=0.75, gamma=2.0, iou_weighted=True,
                                reduction='sum', loss_weight=1.0),
                  loss_obj=dict(type='VarifocalLoss', use_sigmoid=True, alpha=0.75, gamma=2.0, iou_weighted=True,
                                reduction='sum', loss_weight=1.0),
                  loss_kps=dict(type='BalancedL1Loss', alpha=0.5, gamma=1.5, beta=0.3, reduction='mean', loss_weight=0.1),
                  loss_bbox=dict(type='BoundedIoULoss', beta=0.2, eps=1e-3, reduction='sum', loss_weight=5.0)),
    'vfl_obj_mse': dict(loss_obj=dict(type='VarifocalLoss', use_sigmoid=True, alpha=0.5, gamma=1.5, iou_weighted=False,
                                      reduction='sum', loss_weight=1.0),
                        loss_kps=dict(type='MSELoss', reduction='mean', loss_weight=0.1)),
    'l1': dict(loss_kps=dict(type='L1Loss', reduction='mean', loss_weight=0.1)),
}


def cfg_of_head(head):
    """make_cfg of a HEAD_CONFIGS entry (keys it leaves out: configs/yunet_n.py's -- CE, EIoU 5.0, CE, SmoothL1 1/9 0.1)."""
    def spec(d):
        return None if d is None else {k: v for k, v in d.items() if k in ('type', 'alpha', 'gamma', 'iou_weighted')}
    box, kps = head.get('loss_bbox'), head.get('loss_kps')
    kw = {}
    if box is not None:
        kw.update(box_loss=box['type'], smooth_point=box.get('beta'), box_eps=box.get('eps'), w_box=box['loss_weight'])
    if kps is not None:
        kw.update(kps_beta=kps.get('beta', 1.0), w_kps=kps['loss_weight'])
    return make_cfg(spec(head.get('loss_cls')), spec(head.get('loss_obj')), spec(kps), **kw)
