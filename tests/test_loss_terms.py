"""CPU: the loss terms beyond the default selection -- VarifocalLoss, L1Loss, MSELoss, BalancedL1Loss, BoundedIoULoss.

The fp64 restatement of tests/loss_terms_ref.py against the unmodified reference's modules and head (recorded in
tests/golden/loss_terms_cases.npz by tools/make_golden_loss_terms.py); the stand-alone modules against the same; the
committed case's coverage of every new branch; the checker on the restatement itself and on defects; and the surface from
the config to the op list's slots."""
import os

import numpy as np
import pytest
import torch

import loss_terms_ref as LT
import yunet_amd
import yunet_amd._lib as L
import yunet_amd.engine as E
import yunet_amd.kernels as K
import yunet_amd.losses as Lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'loss_terms_cases.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope='module')
def case(golden):
    c = {k[5:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith('case_')}
    c['sizes'] = [tuple(int(v) for v in s) for s in c['sizes']]
    c['strides'] = [int(s) for s in c['strides']]
    return c


_refs = {}


def ref64(case, name):
    if name not in _refs:
        _refs[name] = LT.ref_of(case, LT.make_cfg(**LT.GOLDEN_CONFIGS[name]))
    return _refs[name]


def close(a, b, rel):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= rel * float(b.abs().max())


def test_committed_case_is_the_constructor_s(case):
    made = LT.make_case(*LT.GOLDEN_CASE)
    for k in ('flat', 'gt_inds', 'max_overlaps', 'gt_boxes', 'gt_kps'):
        assert torch.equal(made[k], case[k]), k
    assert made['sizes'] == case['sizes'] and made['strides'] == case['strides']


@pytest.mark.parametrize('name', list(LT.GOLDEN_CONFIGS))
def test_restatement_matches_the_reference_modules(case, golden, name):
    """Same formula, same precision (fp64), only the order of operations differs: 1e-12 of each tensor's largest magnitude.
    Graded per term, so that a small term cannot hide behind a large one.  A term left at CrossEntropyLoss is not under
    test here and gets 1e-6: the reference's binary_cross_entropy casts its target with .float()
    (cross_entropy_loss.py:104-145), so torch evaluates that one term in mixed precision under an fp64 prediction."""
    r = ref64(case, name)
    cfg = LT.make_cfg(**LT.GOLDEN_CONFIGS[name])
    tol = [1e-6 if cfg[k]['type'] == 'CrossEntropyLoss' else 1e-12 for k in ('cls',)] + [1e-12] + \
        [1e-6 if cfg['obj']['type'] == 'CrossEntropyLoss' else 1e-12, 1e-12]
    for i, ch in enumerate(((0,), (1, 2, 3, 4), (5,), tuple(range(6, 16)))):
        assert abs(float(r['losses'][i]) - float(golden[f'{name}_losses'][i])) <= tol[i] * abs(float(r['losses'][i])), i
        assert close(r['dflat'][..., ch], golden[f'{name}_dflat'][..., ch], tol[i]), ch


@pytest.mark.parametrize('name', list(LT.HEAD_CONFIGS))
def test_reference_head_loss_matches_the_whole_step(golden, name):
    """YuNet_Head.loss() of the reference, run in fp32 (its assigner builds fp32 tensors), against the fp32 restatement on
    the assignment that run made.  Both are the same formula in fp32 in different orders: the longest chain behind an
    element is ~40 roundings and a loss sums up to ~170 terms, so 2^-24 * 256 ~ 2e-5 of the largest magnitude bounds it."""
    sizes = [tuple(int(v) for v in s) for s in golden['head_sizes']]
    cfg = LT.cfg_of_head(LT.HEAD_CONFIGS[name])
    r = LT.terms_ref(torch.from_numpy(golden['head_flat']), torch.from_numpy(golden[f'head_{name}_gt_inds']),
                     torch.from_numpy(golden[f'head_{name}_max_overlaps']), torch.from_numpy(golden['head_gt_boxes']),
                     torch.from_numpy(golden['head_gt_kps']), sizes, [int(s) for s in golden['head_strides']], cfg,
                     dtype=torch.float32)
    assert int(r['pos'][0].numel()) >= 4
    want_l, want_g = golden[f'head_{name}_losses'], golden[f'head_{name}_dflat']
    for i in range(4):
        assert abs(float(r['losses'][i]) - float(want_l[i])) <= 2e-5 * abs(float(want_l[i])), (i, r['losses'], want_l)
    for ch in ((0,), (1, 2, 3, 4), (5,), tuple(range(6, 16))):
        assert close(r['dflat'][..., ch], want_g[..., ch], 2e-5), ch


STANDALONE = [('vfl', lambda: Lo.VarifocalLoss(alpha=0.6, gamma=1.5, iou_weighted=True, loss_weight=2.0), 'logit', 'score'),
              ('vfl_now', lambda: Lo.VarifocalLoss(iou_weighted=False), 'logit', 'score'),
              ('l1', lambda: Lo.L1Loss(loss_weight=0.5), 'pred', 'target'),
              ('mse', lambda: Lo.MSELoss(loss_weight=0.5), 'pred', 'target'),
              ('bl1', lambda: Lo.BalancedL1Loss(alpha=0.4, gamma=1.2, beta=0.5, loss_weight=3.0), 'pred', 'target'),
              ('bounded', lambda: Lo.BoundedIoULoss(beta=0.1, eps=1e-3, loss_weight=2.0), 'box_pred', 'box_target')]


@pytest.mark.parametrize('name,make,pk,tk', STANDALONE, ids=[s[0] for s in STANDALONE])
def test_standalone_modules_match_the_reference_modules(golden, name, make, pk, tk):
    mod = make()
    p, t, w = (torch.from_numpy(golden['sa_' + k]) for k in (pk, tk, 'weight'))
    for red in ('none', 'mean', 'sum'):
        assert close(mod(p, t, reduction_override=red), golden[f'sa_{name}_{red}'], 1e-12), red
        assert close(mod(p, t, weight=w, reduction_override=red), golden[f'sa_{name}_{red}_w'], 1e-12), red
    assert close(mod(p, t, weight=w, avg_factor=7.5, reduction_override='mean'), golden[f'sa_{name}_mean_w_avg'], 1e-12)
    with pytest.raises(ValueError):
        mod(p, t, avg_factor=7.5, reduction_override='sum')
    q = p.clone().requires_grad_(True)
    g, = torch.autograd.grad(mod(q, t, weight=w, reduction_override='sum'), q)
    assert close(g, golden[f'sa_{name}_grad'], 1e-12)


def test_standalone_constructor_defaults_are_the_reference_s():
    v, b, bi = Lo.VarifocalLoss(), Lo.BalancedL1Loss(), Lo.BoundedIoULoss()
    assert (v.use_sigmoid, v.alpha, v.gamma, v.iou_weighted, v.reduction, v.loss_weight) == (True, 0.75, 2.0, True, 'mean', 1.0)
    assert (b.alpha, b.gamma, b.beta, b.reduction, b.loss_weight) == (0.5, 1.5, 1.0, 'mean', 1.0)
    assert (bi.beta, bi.eps, bi.reduction, bi.loss_weight) == (0.2, 1e-3, 'mean', 1.0)
    for m in (Lo.L1Loss(), Lo.MSELoss()):
        assert (m.reduction, m.loss_weight) == ('mean', 1.0)
    with pytest.raises(ValueError, match='gamma'):
        Lo.VarifocalLoss(gamma=0.5)
    with pytest.raises(ValueError, match='alpha'):
        Lo.VarifocalLoss(alpha=-0.1)
    z = torch.zeros(0, 10)
    assert float(Lo.L1Loss()(z, z)) == 0.0 and float(Lo.BalancedL1Loss()(z, z)) == 0.0


# ------------------------------------------------------------------------------------------------- coverage
MIN = 8


def test_census_of_the_committed_case(case):
    """Every new branch holds at least 8 elements in the fp64 reference, and the inputs the issue names are there."""
    c = LT.census(case, LT.make_cfg(**LT.GOLDEN_CONFIGS['mixed']))
    for k in ('vfl_cls_neg', 'vfl_cls_pos', 'vfl_obj_neg', 'vfl_obj_pos', 'ovl_zero', 'bounded_clamped', 'bounded_unclamped',
              'bounded_min_target_over_pred', 'bounded_min_pred_over_target', 'bounded_quad', 'bounded_lin', 'kps_quad',
              'kps_lin', 'kps_zero', 'obj_logit_sat'):
        assert c[k] >= MIN, (k, c)
    assert c['cls_logit_sat'] >= 1, c                      # a positive's cls logit at +-30 / +-100
    for name in ('bl1_b1.0', 'bl1_b0.3', 'bounded_b0.2', 'bounded_b0.05'):
        c = LT.census(case, LT.make_cfg(**LT.GOLDEN_CONFIGS[name]))
        for k in ('kps_quad', 'kps_lin') + (('bounded_quad', 'bounded_lin') if 'bounded' in name else ()):
            assert c[k] >= MIN, (name, k, c)
    # saturated logits on both sides of varifocal's t <= 0 decision, finite in the restatement
    gi = case['gt_inds'] > 0
    xo = case['flat'][..., 5]
    assert int((xo[~gi] >= 30).sum()) >= 1 and int((xo[~gi] <= -30).sum()) >= 1
    r = ref64(case, 'mixed')
    assert bool(torch.isfinite(r['dflat']).all()) and bool(torch.isfinite(r['losses']).all())


@pytest.mark.parametrize('name', ['vfl_a0.5_g1.5_iw0', 'l1', 'mse', 'bl1_b0.3', 'bounded_b0.05', 'mixed'])
def test_checker_accepts_the_fp32_restatement_and_few_elements_are_ambiguous(case, name):
    cfg = LT.make_cfg(**LT.GOLDEN_CONFIGS[name])
    r32 = LT.ref_of(case, cfg, dtype=torch.float32)
    rep = LT.check(r32['losses'], r32['dflat'], case, cfg, ref=ref64(case, name))
    assert rep.ok, rep
    if rep.n_dec:
        assert rep.amb_cols <= 0.02 * rep.n_dec, (rep.amb_cols, rep.n_dec)
    n_owned = case['flat'].shape[0] * case['flat'].shape[1] + 15 * rep.n_pos        # obj everywhere, 15 more per positive
    assert rep.n_amb + rep.n_unres <= 0.02 * n_owned, rep


def test_checker_rejects_defects(case):
    """What a kernel could get wrong in the new terms, each as the fp64 result with that defect."""
    name = 'mixed'
    cfg, r = LT.make_cfg(**LT.GOLDEN_CONFIGS[name]), ref64(case, name)
    n_idx, p_idx, _ = r['pos']
    flat = case['flat'].double()

    def graded(dflat, losses=None):
        return LT.check(r['losses'].float() if losses is None else losses, dflat.float(), case, cfg, ref=r)
    assert graded(r['dflat']).ok
    # 1. the focal weight of the t <= 0 side detached: d/dx loses bce * d(fw)/dx (objectness of the negatives)
    x = flat[..., 5]
    sg = torch.sigmoid(x)
    neg = (case['gt_inds'] == 0)
    detached = r['dflat'].clone()
    detached[..., 5] = torch.where(neg, cfg['w_obj'] * (cfg['obj']['alpha'] * sg ** 2) * sg / r['num_total'], detached[..., 5])
    assert not graded(detached).ok
    # 2. balanced-L1 with the plain-L1 slope on the linear side
    bad = r['dflat'].clone()
    kq = [g for g in r['groups'] if g['name'] == 'kps_quad'][0]['val'].bool()
    sub = bad[n_idx, p_idx, 6:]
    bad[n_idx, p_idx, 6:] = torch.where(kq, sub, sub / cfg['kps']['gamma'])
    assert not graded(bad).ok
    # 3. bounded-IoU without the clamp of the centre terms: a gradient where the reference has none
    bad = r['dflat'].clone()
    first = [g for g in r['groups'] if g['name'] == 'box_first'][0]['val'].bool()
    sub = bad[n_idx, p_idx, 1:3]
    bad[n_idx, p_idx, 1:3] = torch.where(first[:, :2], sub, torch.full_like(sub, 1e-3))
    assert not graded(bad).ok
    # 4. a loss off by one part in 1e4
    lo = r['losses'].float().clone()
    lo[0] *= 1.0001
    assert not graded(r['dflat'], lo).ok


# ------------------------------------------------------------------------------------------------- surface
def _model(**head):
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    for k, v in head.items():
        cfg.model.bbox_head[k] = v
    return yunet_amd.build_detector(cfg.model)


VFL = dict(type='VarifocalLoss', use_sigmoid=True, alpha=0.5, gamma=1.5, iou_weighted=False, reduction='sum', loss_weight=1.0)
MIXED = dict(loss_cls=VFL, loss_obj=dict(VFL, alpha=0.75, gamma=2.0, iou_weighted=True),
             loss_kps=dict(type='BalancedL1Loss', alpha=0.4, gamma=1.2, beta=0.3, reduction='mean', loss_weight=0.1),
             loss_bbox=dict(type='BoundedIoULoss', beta=0.05, eps=1e-3, reduction='sum', loss_weight=5.0))


def _loss_op(plan):
    ops = [op for op in plan.fwd_b if op.opcode == L.OP_LOSS]
    assert len(ops) == 1
    return ops[0]


def test_config_to_loss_cfg_to_op_slots():
    m = _model(**MIXED)
    c = m.bbox_head.loss_cfg()
    t = c.terms
    assert c.box_loss == L.BOX_BOUNDED and c.smooth_point == pytest.approx(0.05) and c.box_eps == pytest.approx(1e-3)
    assert c.kps_beta == pytest.approx(0.3)
    assert (t.cls_loss, t.obj_loss, t.kps_loss) == (L.CLS_VARIFOCAL, L.CLS_VARIFOCAL, L.KPS_BALANCED_L1)
    assert (t.cls_iou_weighted, t.obj_iou_weighted) == (0, 1)
    assert (t.cls_alpha, t.cls_gamma, t.obj_alpha, t.obj_gamma) == pytest.approx((0.5, 1.5, 0.75, 2.0))
    assert (t.kps_alpha, t.kps_gamma) == pytest.approx((0.4, 1.2))
    op = _loss_op(E.Plan(E.YuNetEngine(m.arch(), 'cpu'), 2, 64, 64, 64))
    assert list(op.i[4:8]) == [L.CLS_VARIFOCAL, L.CLS_VARIFOCAL, L.KPS_BALANCED_L1, 2]
    assert list(op.f[:6]) == pytest.approx([0.5, 1.5, 0.75, 2.0, 0.4, 1.2])
    assert op.loss.box_loss == L.BOX_BOUNDED and op.loss.smooth_point == pytest.approx(0.05)
    for kps, code in (('L1Loss', L.KPS_L1), ('MSELoss', L.KPS_MSE)):
        m = _model(loss_kps=dict(type=kps, reduction='mean', loss_weight=0.1))
        assert m.bbox_head.loss_cfg().terms.kps_loss == code
        op = _loss_op(E.Plan(E.YuNetEngine(m.arch(), 'cpu'), 2, 64, 64, 64))
        assert list(op.i[4:8]) == [0, 0, code, 0] and list(op.f) == [0.0] * 8


def test_default_config_leaves_the_new_slots_zero():
    import yunet_oracle as O
    m = _model()
    assert m.bbox_head.loss_cfg().terms is None
    for arch in (m.arch(), O.yunet_arch('n')):                    # the oracle's arch dict has none of the new keys
        op = _loss_op(E.Plan(E.YuNetEngine(arch, 'cpu'), 2, 64, 64, 64))
        assert list(op.i[4:9]) == [0] * 5 and list(op.f) == [0.0] * 8
        assert op.loss.box_loss == L.BOX_EIOU
    assert K.make_loss_terms().is_default() and K.make_loss_terms().op_slots() == ([0, 0, 0, 0], [0.0] * 6)


def test_rejections():
    with pytest.raises(NotImplementedError, match="reduction='sum'"):         # VarifocalLoss's own default is 'mean'
        _model(loss_cls=dict(type='VarifocalLoss', loss_weight=1.0)).bbox_head.loss_cfg()
    with pytest.raises(NotImplementedError, match="reduction='sum'"):
        _model(loss_obj=dict(type='VarifocalLoss')).arch()
    with pytest.raises(NotImplementedError, match="reduction='mean'"):
        _model(loss_kps=dict(type='L1Loss', reduction='sum')).bbox_head.loss_cfg()
    with pytest.raises(ValueError, match='gamma'):
        _model(loss_cls=dict(VFL, gamma=0.9))
    with pytest.raises(ValueError, match='alpha'):
        _model(loss_obj=dict(VFL, alpha=-1.0))
    with pytest.raises(NotImplementedError, match='Only sigmoid'):
        _model(loss_cls=dict(VFL, use_sigmoid=False))
    with pytest.raises(KeyError):                                             # not a loss the reference head can run
        _model(loss_cls=dict(type='FocalLoss', reduction='sum'))
    # a registered loss in a term that has no kernel for it: the message names what is implemented
    with pytest.raises(NotImplementedError, match='CrossEntropyLoss, VarifocalLoss'):
        _model(loss_cls=dict(type='L1Loss', reduction='sum')).bbox_head.loss_cfg()
    with pytest.raises(NotImplementedError, match='SmoothL1Loss, L1Loss, MSELoss, BalancedL1Loss'):
        _model(loss_kps=dict(type='VarifocalLoss', reduction='mean')).arch()
    with pytest.raises(NotImplementedError, match='BoundedIoULoss'):
        K.box_loss_code('SmoothL1Loss')
    with pytest.raises(ValueError, match='gamma'):
        K.make_loss_terms(loss_obj=dict(type='VarifocalLoss', gamma=0.5))
    with pytest.raises(NotImplementedError, match='use_sigmoid'):
        K.make_loss_terms(loss_cls=dict(type='VarifocalLoss', use_sigmoid=False))
    with pytest.raises(ValueError, match='beta'):
        K.make_loss_cfg('BoundedIoULoss', smooth_point=0.0)


def test_abi_additions_are_consistent(tmp_path):
    """The new struct's ctypes layout is the header's, the entry is in the signature table, the version stays 12 and
    YunetOp / YunetLossCfg keep their size (no field was added to a record inside an op)."""
    import ctypes as C
    import re
    import subprocess
    hdr = open(os.path.join(ROOT, 'include', 'yunet_hip.h')).read()
    assert 'yunet_loss_terms' in L._SIGNATURES and re.search(r'\bint yunet_loss_terms\(', hdr)
    assert len(L._SIGNATURES['yunet_loss_terms'][1]) == len(L._SIGNATURES['yunet_loss'][1]) + 1
    assert L._SIGNATURES['yunet_loss_terms'][1][7] is C.POINTER(L.YunetLossTerms)
    assert L.load().yunet_abi_version() == 12
    for name, val in (('YUNET_BOX_BOUNDED', L.BOX_BOUNDED), ('YUNET_CLS_VARIFOCAL', L.CLS_VARIFOCAL), ('YUNET_KPS_L1', L.KPS_L1),
                      ('YUNET_KPS_MSE', L.KPS_MSE), ('YUNET_KPS_BALANCED_L1', L.KPS_BALANCED_L1)):
        assert int(re.search(rf'\b{name} = (\d+)', hdr).group(1)) == val, name
    cc = 'gcc'
    src = tmp_path / 'layout.c'
    fields = [f[0] for f in L.YunetLossTerms._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yunet_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(YunetLossTerms), sizeof(YunetOp), sizeof(YunetLossCfg));\n' +
                   ''.join(f'  printf(" %zu", offsetof(YunetLossTerms, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(L.YunetLossTerms), C.sizeof(L.YunetOp), C.sizeof(L.YunetLossCfg)] + \
        [getattr(L.YunetLossTerms, f).offset for f in fields]
    assert got == want


def test_train_cli_takes_the_new_terms(tmp_path, monkeypatch):
    from test_train_cli import CFG, T
    seen = {}

    def fake_train(m, ds, cfg, **kw):
        seen['model'] = m
        return []
    monkeypatch.setattr(T.R, 'train_detector', fake_train)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda i: None)
    T.main([CFG, '--no-validate', '--work-dir', str(tmp_path), '--cfg-options', 'data.samples_per_gpu=4',
            'data.train.type=SyntheticWiderFace', 'data.train.img_scale=(160,160)', 'data.train.iters_per_epoch=2',
            'model.bbox_head.loss_cls.type=VarifocalLoss', 'model.bbox_head.loss_kps.type=BalancedL1Loss',
            'model.bbox_head.loss_bbox.type=BoundedIoULoss', 'model.bbox_head.loss_bbox.eps=0.001'])
    hd = seen['model'].bbox_head
    assert type(hd.loss_cls).__name__ == 'VarifocalLoss' and hd.loss_cls.reduction == 'sum'
    t = hd.loss_cfg().terms
    assert (t.cls_loss, t.obj_loss, t.kps_loss) == (L.CLS_VARIFOCAL, L.CLS_BCE, L.KPS_BALANCED_L1)
    assert seen['model'].arch()['loss_bbox'] == 'BoundedIoULoss'
