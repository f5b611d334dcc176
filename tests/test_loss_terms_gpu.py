"""-m gpu: loss_terms_kernel (yunet_loss_terms, csrc/loss_step.hip) per element against the fp64 restatement of
tests/loss_terms_ref.py -- every new term one at a time and all together -- the deferred normaliser, run-to-run bytes,
the all-zero selection against yunet_loss, and the terms inside the fused engine against the head's stand-alone loss()."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import loss_ref as R
import loss_terms_ref as LT
import yunet_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cases, _refs = {}, {}


def case_of(key):
    """The committed case (N = 3, 64 x 96, P = 126) and N = 5 at 96 x 96, built once."""
    if key not in _cases:
        _cases[key] = LT.make_case(*(LT.GOLDEN_CASE if key == 'golden' else (5, 96, 96, 23)))
    return _cases[key]


def ref_of(key, name, **kw):
    k = (key, name, tuple(sorted(kw.items())))
    if k not in _refs:
        _refs[k] = LT.ref_of(case_of(key), LT.make_cfg(**LT.GOLDEN_CONFIGS[name]), **kw)
    return _refs[k]


def run_terms(case, cfg, blocks=None, defer=False, num_total=None, terms='cfg', entry='yunet_loss_terms'):
    """yunet_loss_terms (or yunet_loss) + yunet_loss_finalize_ex through the C ABI -> (losses [5], dflat, dy_norm) on the host."""
    import yunet_amd._lib as L
    import yunet_amd.kernels as k
    d = {key: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for key, v in case.items()}
    N, P, _ = d['flat'].shape
    lib = L.load()
    norm = k.loss_norm(d['img_stats'])
    blocks = blocks or int(lib.yunet_loss_blocks(N, P))
    part = torch.empty(blocks, 4, device=DEV)
    dflat = torch.full_like(d['flat'], float('nan'))
    losses = torch.empty(5, device=DEV)
    lv = k.make_levels(d['sizes'], d['strides'])
    kc, kt = LT.kernel_cfg(cfg, defer)
    head = [k._p(d['flat']), k._p(d['gt_inds']), k._p(d['max_overlaps']), k._p(d['gt_boxes']), k._p(d['gt_kps']), C.byref(lv),
            C.byref(kc)]
    tail = [k._p(norm), N, P, d['gt_boxes'].shape[1], k._p(dflat), k._p(part), blocks, k._stream()]
    if entry == 'yunet_loss':
        L.check(lib.yunet_loss(*head, *tail), entry)
    else:
        tp = None if terms is None else C.byref(kt if terms == 'cfg' else terms)
        L.check(lib.yunet_loss_terms(*head, tp, *tail), entry)
    nt = dyn = None
    if defer:
        nt = torch.tensor([float(num_total)], device=DEV)
        dyn = torch.full((16,), float('nan'), device=DEV)
    L.check(lib.yunet_loss_finalize_ex(k._p(part), blocks, k._p(losses), None, k._p(nt), k._p(dyn), k._stream()),
            'yunet_loss_finalize_ex')
    torch.cuda.synchronize()
    return losses.cpu(), dflat.cpu(), None if dyn is None else dyn.cpu()


def grade(tag, key, name, losses, dflat, **kw):
    case, cfg = case_of(key), LT.make_cfg(**LT.GOLDEN_CONFIGS[name])
    ref_kw = {k: v for k, v in kw.items() if k in ('num_total', 'kps_den')}
    rep = LT.check(losses[:4], dflat, case, cfg, ref=ref_of(key, name, **ref_kw), **kw)
    print(f'\n[{tag}] {rep}')
    assert rep.ok, rep
    assert bool(torch.isfinite(dflat).all()) and bool(torch.isfinite(losses).all())
    # the escape routes stay small: decisions graded against both sides, elements graded against the fp32 restatement too
    if rep.n_dec:
        assert rep.amb_cols <= 0.02 * rep.n_dec, rep
    assert rep.n_unres <= 0.01 * 16 * rep.n_pos + 5, rep
    return rep


ONE_AT_A_TIME = ['vfl_a0.75_g2.0_iw1', 'vfl_a0.5_g1.5_iw0', 'vfl_a0.5_g2.0_iw0', 'vfl_a0.75_g1.5_iw1', 'l1', 'mse', 'bl1_b1.0',
                 'bl1_b0.3', 'bounded_b0.2', 'bounded_b0.05', 'mixed']


@pytest.mark.parametrize('name', ONE_AT_A_TIME)
@pytest.mark.parametrize('key', ['golden', '5x96'])
def test_terms_per_element(key, name):
    case = case_of(key)
    losses, dflat, _ = run_terms(case, LT.make_cfg(**LT.GOLDEN_CONFIGS[name]))
    grade(f'{key}/{name}', key, name, losses, dflat)
    tot = ((losses[0] + losses[1]) + losses[2]) + losses[3]
    assert float(losses[4]) == float(tot)
    neg = case['gt_inds'] == 0
    assert bool((dflat[neg][:, [0, 1, 2, 3, 4] + list(range(6, 16))] == 0).all())


def test_two_blocks_walk_the_grid_stride_loop_and_the_block_reduction():
    """N * P = 5 * 189 = 945 priors over 2 blocks of 256 threads: two trips of the loop for most threads."""
    case, cfg = case_of('5x96'), LT.make_cfg(**LT.GOLDEN_CONFIGS['mixed'])
    assert case['flat'].shape[1] == 189
    losses, dflat, _ = run_terms(case, cfg, blocks=2)
    grade('blocks=2', '5x96', 'mixed', losses, dflat, blocks=2)
    l_full, d_full, _ = run_terms(case, cfg)
    assert torch.equal(dflat, d_full)                         # the gradient does not depend on the grid


@pytest.mark.parametrize('name', ['vfl_a0.5_g1.5_iw0', 'bl1_b0.3', 'bounded_b0.05'])
@pytest.mark.parametrize('num_total', [0.0, 37.25])
def test_deferred_normaliser(name, num_total):
    """defer_num_total = 1: the kernel leaves cls / bbox / obj un-normalised (num_total = 1 in the reference), finalize
    applies 1 / max(num_total, 1) to the losses and hands it to the head backward as dy_norm."""
    case, cfg = case_of('golden'), LT.make_cfg(**LT.GOLDEN_CONFIGS[name])
    losses, dflat, dyn = run_terms(case, cfg, defer=True, num_total=num_total)
    inv = np.float32(1.0) / np.float32(max(num_total, 1.0))
    assert dyn.tolist() == [float(inv)] * 6 + [1.0] * 10
    # the un-normalised gradient against the reference at num_total = 1 ...
    ref1 = ref_of('golden', name, num_total=1.0)
    rep = LT.check(ref1['losses'], dflat, case, cfg, ref=ref1, num_total=1.0)
    print(f'\n[defer {name} {num_total}] {rep}')
    assert rep.ok, rep
    # ... and the finalized losses against the reference at the deferred num_total
    grade(f'defer {name} {num_total}', 'golden', name, losses, dflat * dyn, num_total=max(num_total, 1.0))
    # x (1 / num_total) once, in the same product order: the same bits as the undeferred launch when num_total is this batch's
    if num_total == 0.0:
        c2 = dict(case)
        c2['gt_inds'] = torch.zeros_like(case['gt_inds'])
        c2['img_stats'] = torch.zeros_like(case['img_stats'])
        l_d, d_d, dy = run_terms(c2, cfg, defer=True, num_total=0.0)
        l_u, d_u, _ = run_terms(c2, cfg)
        assert torch.equal(d_d * dy, d_u) and torch.equal(l_d, l_u)


def test_two_runs_give_the_same_bytes():
    case, cfg = case_of('5x96'), LT.make_cfg(**LT.GOLDEN_CONFIGS['mixed'])
    a, b = run_terms(case, cfg), run_terms(case, cfg)
    assert a[0].numpy().tobytes() == b[0].numpy().tobytes() and a[1].numpy().tobytes() == b[1].numpy().tobytes()


@pytest.mark.parametrize('box,mode', [('EIoULoss', None), ('IoULoss', 'square'), ('CIoULoss', None)])
def test_all_zero_selection_is_yunet_loss(box, mode):
    import yunet_amd._lib as L
    case = case_of('5x96')
    cfg = LT.make_cfg(box_loss=box, box_mode=mode)
    want = run_terms(case, cfg, entry='yunet_loss')
    for terms in (None, L.YunetLossTerms()):
        got = run_terms(case, cfg, terms=terms)
        assert got[0].numpy().tobytes() == want[0].numpy().tobytes()
        assert got[1].numpy().tobytes() == want[1].numpy().tobytes()
    # and yunet_loss is still graded by the default terms' own reference
    rep = R.check(want[0][:4], want[1], case, R.make_cfg(box, mode))
    assert rep.ok, rep


def test_entry_rejects_what_the_kernel_cannot_compute():
    import yunet_amd._lib as L
    case, cfg = case_of('golden'), LT.make_cfg(**LT.GOLDEN_CONFIGS['mixed'])
    for field, val in (('cls_gamma', 0.5), ('obj_alpha', -1.0), ('kps_loss', 9), ('cls_loss', 2), ('kps_alpha', 0.0)):
        _, t = LT.kernel_cfg(cfg)
        setattr(t, field, val)
        with pytest.raises(RuntimeError):
            run_terms(case, cfg, terms=t)


# ------------------------------------------------------------------------------------------------ the fused engine
def _build(sd, mode):
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    for k, v in LT.HEAD_CONFIGS['mixed'].items():
        cfg.model.bbox_head[k] = v
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).train()
    if mode == 'bf16':
        m.set_precision('bf16')
    if mode == 'det-fast':
        m.set_deterministic('fast')
    return m


@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'det-fast'])
def test_fused_engine_runs_the_terms(mode):
    """forward_train + backward of YuNet_n at 2 x 64 x 64 with VFL cls + VFL obj + BalancedL1 kps + BoundedIoU box: the op
    list's slots carry the selection.  Against the head's stand-alone loss() (_LossStep: yunet_loss_terms called directly)
    on the engine's own predictions, and in fp32 storage against the per-module training path on the same weights, at
    the tolerances tests/test_modules_autograd_gpu.py and tests/test_engine_gpu.py use between those paths (1e-4)."""
    import yunet_amd._lib as L
    import yunet_amd.synthetic as S
    sd = O.init_state(O.yunet_arch('n'), seed=3)
    bd = S.to_device(S.make_batch(2, 64, 64, 77), DEV)
    m = _build(sd, mode)
    losses_f = m.forward_train(**bd)
    sum(losses_f.values()).backward()
    torch.cuda.synchronize()
    plan = m.engine.plan
    op = [o for o in plan.fwd_b if o.opcode == L.OP_LOSS][0]
    assert list(op.i[4:8]) == [L.CLS_VARIFOCAL, L.CLS_VARIFOCAL, L.KPS_BALANCED_L1, 3] and op.loss.box_loss == L.BOX_BOUNDED
    gi_f, flat, dflat_f = plan.gt_inds.clone(), plan.flat.detach().clone(), plan.dflat.detach().clone()
    assert int((gi_f > 0).sum()) >= 2
    grads_f = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    # the stand-alone loss() on the same predictions
    fl = flat.float().requires_grad_(True)
    maps, off = ([], [], [], []), 0
    for fh, fw in plan.sizes:
        mm = fl[:, off:off + fh * fw].reshape(fl.shape[0], fh, fw, 16).permute(0, 3, 1, 2)
        off += fh * fw
        for o, (a, b) in zip(maps, ((0, 1), (1, 5), (5, 6), (6, 16))):
            o.append(mm[:, a:b])
    losses_s = m.bbox_head.loss(*maps, bd['gt_bboxes'], bd['gt_labels'], bd['gt_keypointss'], bd['img_metas'])
    sum(losses_s.values()).backward()
    torch.cuda.synchronize()
    assert torch.equal(m.bbox_head.last_gt_inds, gi_f)
    for k in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps'):
        assert float(losses_s[k].detach()) == pytest.approx(float(losses_f[k].detach()), rel=1e-4), k
        assert float(losses_f[k].detach()) > 0 and np.isfinite(float(losses_f[k].detach()))
    assert float((fl.grad - dflat_f).abs().max()) <= 1e-4 * float(dflat_f.abs().max())
    if mode == 'bf16':
        return
    # the per-module path (backbone -> neck -> head.forward -> head.loss) on the same weights: the flat parameter gradient
    mod = _build(sd, 'fp32')
    losses_m = mod.bbox_head.forward_train(mod.extract_feat(bd['img']), bd['img_metas'], bd['gt_bboxes'], bd['gt_labels'],
                                           bd['gt_keypointss'])
    sum(losses_m.values()).backward()
    torch.cuda.synchronize()
    assert torch.equal(mod.bbox_head.last_gt_inds, gi_f), 'the two paths assigned different priors'
    for k in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps'):
        assert float(losses_m[k].detach()) == pytest.approx(float(losses_f[k].detach()), rel=1e-4), k
    scale = max(float(v.abs().max()) for v in grads_f.values())
    for k, p in mod.named_parameters():
        assert float((p.grad - grads_f[k]).abs().max()) / scale <= 1e-4, k
