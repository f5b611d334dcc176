"""-m gpu: fine-tuning in the fused engine.  The kernels are the ones every other test pins; what can
fail here is wiring, so the shapes are small (64 x 64, one 64 x 96 so that a wrong per-layer count shows; N = 2 or 3) and
reach every op.  Weights are fresh, BatchNorm buffers those one train-mode step leaves behind (finetune_ref.warm_state).

Yardstick: oracle/yunet_oracle.py composed with a `training` flag per part (finetune_ref.py).  Gradients by the rule of
test_engine_gpu.py::test_forward_train_vs_oracle -- both fp32 implementations against an fp64 evaluation of the same
composition; the HIP error within 10 x the oracle's own plus 1 % of the tensor -- losses at its 1e-4, the assignment exact
with NO near-tie exemption: the seeds below were picked so that helpers.image_near_tie is false for every image (asserted).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import finetune_ref as FR
import yunet_amd._lib as L
import yunet_oracle as O
from optim_checks import check
from test_deterministic_gpu import CONTRACT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- set-ups
def all_bn(m):
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.eval()


def head_only(m):
    for part in (m.backbone, m.neck):
        part.eval()
        for p in part.parameters():
            p.requires_grad = False


def middle_unit(m):
    u = m.neck.lateral_convs[1]
    for p in list(u.conv1.parameters()) + list(u.conv2.parameters()):
        p.requires_grad = False


# name -> (kind, N, H, W, batch seed, backbone arguments, set-up after train())
CASES = {
    'all_bn_n': ('n', 2, 64, 64, 11, {}, all_bn),
    'all_bn_s': ('s', 3, 64, 96, 12, {}, all_bn),
    'norm_eval': ('n', 3, 64, 96, 13, dict(norm_eval=True), None),
    'stages0': ('n', 2, 64, 64, 14, dict(frozen_stages=0), None),
    'stages2': ('s', 3, 64, 64, 15, dict(frozen_stages=2), None),
    'stages_last': ('n', 2, 64, 64, 16, dict(frozen_stages=5), None),
    'head_only': ('n', 2, 64, 64, 27, {}, head_only),
    'middle_unit': ('s', 2, 64, 64, 27, {}, middle_unit),
}


def build(name, dev=DEV):
    import yunet_amd
    import yunet_amd.synthetic as S
    kind, n, h, w, seed, bb, setup = CASES[name]
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    cfg.model.backbone.update(bb)
    m = yunet_amd.build_detector(cfg.model)
    sd = FR.warm_state(kind, 1)
    m.load_state_dict(sd, strict=True)
    m.to(dev).train()
    if setup is not None:
        setup(m)
    return m, sd, O.yunet_arch(kind), S.make_batch(n, h, w, seed)


def flags_of(m):
    """(flag(BatchNorm name) -> training, frozen parameter names) as the model's modules say"""
    bn = {n: mod.training for n, mod in m.named_modules() if isinstance(mod, nn.BatchNorm2d)}
    return (lambda name: bn.get(name, True)), [n for n, p in m.named_parameters() if not p.requires_grad]      # (YuNet_s: no BN in the head)


def bytes_of(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()


def buffers(m):
    return {k: bytes_of(v) for k, v in m.state_dict().items() if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}


def run_case(name, deterministic=False):
    """One fused step of the case against the yardstick; returns what the callers look at further."""
    import yunet_amd.synthetic as S
    m, sd, arch, b = build(name)
    m.set_deterministic(deterministic)
    flag, frozen = flags_of(m)
    lv, g32, aux, after = FR.step_fp32(b, sd, arch, flag)
    assert FR.near_tie(aux, b) == [], 'pick another seed: the oracle assignment sits on a tie'
    m._ensure_engine(torch.device(DEV, torch.cuda.current_device()))
    before = buffers(m)
    losses = m.forward_train(**S.to_device(b, DEV))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    plan = m.engine.plan
    assert torch.equal(plan.gt_inds.cpu(), aux['gt_inds'].int()), 'assignment'
    ref_flat = aux['flat']
    err = float((plan.flat.cpu().double() - ref_flat.double()).abs().max() / ref_flat.double().abs().max())
    print(f'[{name}] flat rel err {err:.2e}')
    assert err < 5e-4
    for k in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps'):
        print(f'[{name}] {k} {float(losses[k]):.7g} oracle {lv[k]:.7g}')
        assert abs(float(losses[k]) - lv[k]) <= 1e-4 * abs(lv[k]) + 1e-6, (k, float(losses[k]), lv[k])
    # gradients: trainable ones by the 10 x + 1 % rule; frozen ranges exactly zero and .grad None
    g64 = FR.grads_fp64(b, sd, arch, flag, plan.dflat.cpu())
    scale = max(float(v.abs().max()) for k, v in g64.items() if k not in frozen)
    named = dict(m.named_parameters())
    fp = m.engine.params
    worst = (0.0, None)
    for k in g32:
        if k in frozen:
            assert named[k].grad is None, k
            assert not bool(fp.view(k, of=fp.grad).any()), f'{k}: frozen range of the flat gradient is not zero'
            continue
        got = named[k].grad.cpu().double()
        err_hip = float((got - g64[k]).abs().max())
        err_ref = float((g32[k].double() - g64[k]).abs().max())
        tol = 10 * max(err_ref, 1e-5 * scale) + 1e-2 * float(g64[k].abs().max())
        worst = max(worst, (err_hip / tol, k))
        assert err_hip <= tol, (k, err_hip, err_ref, float(g64[k].abs().max()), scale)
    print(f'[{name}] worst gradient error / bound {worst[0]:.3f} ({worst[1]})')
    # BatchNorm buffers: a frozen layer keeps its bytes, a training one moves as the oracle's
    now = m.state_dict()
    for k, was in before.items():
        bn_name = k.rsplit('.', 1)[0]
        if not flag(bn_name):
            assert torch.equal(bytes_of(now[k]), was), f'{k}: a frozen BatchNorm layer changed'
        elif k.endswith('num_batches_tracked'):
            assert int(now[k]) == int(after[k]) == int(sd[k]) + 1, k
        else:
            assert torch.allclose(now[k].cpu(), after[k], rtol=1e-3, atol=1e-4), k
            assert not torch.equal(bytes_of(now[k]), was), k
    return m, sd, frozen, flag


# ---------------------------------------------------------------------------------------------------------- 1, 2, 4, 5
@pytest.mark.parametrize('name', ['all_bn_n', 'all_bn_s'])
def test_all_batchnorm_frozen(name):
    m, sd, frozen, flag = run_case(name)
    assert frozen == [] and not any(flag(n) for n in m.engine.layout.bn_names)
    assert m.engine.plan.nbt_step is None and m.engine.plan.bn_table_run is None


@pytest.mark.parametrize('level', [True, 'fast'])
def test_all_batchnorm_frozen_in_a_deterministic_plan(level):
    """Frozen layers whose gamma / beta train, deterministic: the readers take the zero block while the backward fold stays
    and feeds the mode-1 launch (row 0) -- d(gamma), d(beta) and everything upstream against the same yardstick."""
    m, sd, frozen, flag = run_case('all_bn_n', deterministic=level)
    plan = m.engine.plan
    n_bn = len(m.engine.layout.bn_names)
    assert plan.det and frozen == [] and len(plan.frozen_bn) == n_bn
    assert [op.opcode for op in plan.fwd_a].count(L.OP_BN_FOLD) == 0 and [op.opcode for op in plan.bwd].count(L.OP_BN_FOLD) == n_bn


def test_norm_eval_freezes_the_backbone_statistics_only():
    m, sd, frozen, flag = run_case('norm_eval')
    names = m.engine.layout.bn_names
    assert frozen == [] and [n for n in names if not flag(n)] == [n for n in names if n.startswith('backbone.')]


def ran_backward_units(m):
    """unit names of every OP_DP_BWD / OP_STEM_BWD in the lists a backward of this plan executes"""
    eng, plan = m.engine, m.engine.plan
    lay = eng.layout
    ptr_of = {lay.unit_ptrs(eng.params.data, u)[0]: u for u in lay.units if u != 'stem'}
    lists = [plan.c_bwd] + ([plan.c_bwd_a_k, plan.c_tail_a, plan.c_bwd_b, plan.c_bwd_a] if plan.split_off is not None else [])
    out = []
    for lst in lists:
        names = []
        for op in lst:
            if op.opcode == L.OP_DP_BWD:
                names.append(ptr_of[op.dp.w_pw])
            elif op.opcode in (L.OP_STEM_BWD, L.OP_POOL_BWD, L.OP_UPADD_BWD):
                names.append({L.OP_STEM_BWD: 'stem', L.OP_POOL_BWD: 'pool', L.OP_UPADD_BWD: 'upadd'}[op.opcode])
        out.append(names)
    return out


def test_head_only_runs_no_backbone_or_neck_backward():
    m, sd, frozen, flag = run_case('head_only')
    assert all(k.startswith('bbox_head.') for k, p in m.named_parameters() if p.requires_grad)
    lists = ran_backward_units(m)
    assert lists[0] and all(u.startswith(('bbox_head.', 'head.')) for names in lists for u in names), lists


def test_frozen_unit_in_the_middle_passes_the_gradient_on():
    m, sd, frozen, flag = run_case('middle_unit')
    assert sorted(frozen) == sorted(f'neck.lateral_convs.1.{c}.{t}' for c in ('conv1', 'conv2') for t in ('weight', 'bias'))
    assert 'neck.lateral_convs.1' in ran_backward_units(m)[0] and all(flag(n) for n in m.engine.layout.bn_names)


# ------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('name', ['stages0', 'stages2', 'stages_last'])
def test_frozen_stages_gradients_and_one_sgd_step(name):
    from yunet_amd.optim import FusedSGD
    m, sd, frozen, flag = run_case(name)
    k = m.backbone.frozen_stages
    assert frozen and all(int(n.split('.')[1][5:]) <= k for n in frozen)
    assert 'stem' not in ran_backward_units(m)[0]
    lr, mom, wd = 0.05, 0.9, 5e-4
    opt = FusedSGD(m, lr=lr, momentum=mom, weight_decay=wd)
    eng = opt._bind()
    fp = eng.params
    gen = torch.Generator().manual_seed(5)
    opt._buf.copy_(torch.randn(fp.data.numel(), generator=gen) * 1e-3)          # a momentum state worth keeping
    opt._steps = 1
    p0, g0, b0 = fp.data.cpu().clone(), fp.grad.cpu().clone(), opt._buf.cpu().clone()
    opt.step()
    torch.cuda.synchronize()
    assert int((opt._map == L.OPT_FROZEN).sum()) == sum(fp.view(n).numel() for n in frozen)
    p1, b1 = fp.data.cpu(), opt._buf.cpu()
    mask = torch.zeros(p0.numel(), dtype=torch.bool)
    for n in frozen:
        off, shape = fp.layout.entries[n]
        mask[off:off + int(np.prod(shape))] = True
    assert torch.equal(bytes_of(p1[mask]), bytes_of(p0[mask])) and torch.equal(bytes_of(b1[mask]), bytes_of(b0[mask]))
    assert not bool(g0[mask].any())

    def formula(dtype):                                                         # torch/optim/sgd.py, not the first step
        p, g, b = p0[~mask].to(dtype), g0[~mask].to(dtype), b0[~mask].to(dtype)
        d = g + torch.tensor(wd, dtype=dtype) * p
        b = b * torch.tensor(mom, dtype=dtype) + d
        return p - torch.tensor(lr, dtype=dtype) * b, b
    (p32, b32), (p64, b64) = formula(torch.float32), formula(torch.float64)
    check(f'{name} parameters', p1[~mask], p32, p64)
    check(f'{name} momentum', b1[~mask], b32, b64)
    assert not torch.equal(p1[~mask], p0[~mask])


# ------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize('kind', ['n', 's'])
def test_fused_step_with_frozen_batchnorm_equals_the_per_module_path(kind):
    """every bn.eval() under model.train(): YuNet.forward_train (the engine) against backbone -> neck -> head.forward ->
    head.loss (one autograd node per unit, functional.py reads bn.training), at the 1e-4 bar of
    test_modules_autograd_gpu.py::test_per_module_training_path_equals_the_fused_engine"""
    import yunet_amd.synthetic as S
    name = 'all_bn_' + kind
    b = None
    out = []
    for path in ('fused', 'modules'):
        m, sd, arch, b = build(name)
        bd = S.to_device(b, DEV)
        before = buffers(m)
        if path == 'fused':
            losses = m.forward_train(**bd)
        else:
            losses = m.bbox_head.forward_train(m.extract_feat(bd['img']), bd['img_metas'], bd['gt_bboxes'], bd['gt_labels'],
                                               bd['gt_keypointss'])
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        gi = m.engine.plan.gt_inds.clone() if path == 'fused' else m.bbox_head.last_gt_inds.clone()
        for k, was in before.items():
            assert torch.equal(bytes_of(m.state_dict()[k]), was), (path, k)
        out.append((gi, {k: float(v) for k, v in losses.items()}, {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    (gi_f, l_f, g_f), (gi_m, l_m, g_m) = out
    assert torch.equal(gi_m, gi_f), 'the two paths assigned different priors'
    for k in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps'):
        assert l_m[k] == pytest.approx(l_f[k], rel=1e-4), k
    scale = max(float(v.abs().max()) for v in g_f.values())
    worst = max((float((g_m[k] - g_f[k]).abs().max()) / scale, k) for k in g_f)
    print(f'[per-module {kind}] worst gradient difference {worst[0]:.2e} ({worst[1]}) of the largest gradient')
    assert worst[0] <= 1e-4, worst


# ------------------------------------------------------------------------------------------------------------------- 7
SEG = [1, 16, 9 * 16 + 3, 255, 257] * 3                      # group boundaries inside a float4 and inside a block
N_EL = sum(SEG)


def group_maps():
    """(map without the frozen byte, the same map with 255 scattered: single elements, both sides of every group boundary,
    a whole segment, the first and the last element)"""
    gid = torch.cat([torch.full((n,), i % 3, dtype=torch.uint8) for i, n in enumerate(SEG)])
    frozen = torch.zeros(N_EL, dtype=torch.bool)
    frozen[[0, N_EL - 1]] = True
    frozen[torch.arange(5, N_EL, 37)] = True
    edge = 0
    for i, n in enumerate(SEG[:-1]):
        edge += n
        frozen[edge - 1 if i % 2 else edge] = True               # last element of one group | first of the next
    frozen[sum(SEG[:3]):sum(SEG[:4])] = True                      # a whole 255-element segment
    with_frozen = gid.clone()
    with_frozen[frozen] = L.OPT_FROZEN
    return gid.to(DEV), with_frozen.to(DEV), frozen


@pytest.mark.parametrize('which', ['sgd', 'sgd-first-nesterov', 'adam', 'adamw-clipped'])
def test_grouped_kernels_skip_the_frozen_byte(which):
    import yunet_amd.kernels as K
    gid, gid_f, frozen = group_maps()
    gen = torch.Generator().manual_seed(9)
    p0, g, s1, s2 = (torch.randn(N_EL, generator=gen).to(DEV) for _ in range(4))
    s2 = s2.abs()
    coef = torch.tensor([0.37], device=DEV) if 'clipped' in which else None
    if which.startswith('sgd'):
        table = torch.tensor([[0.1, 5e-4, 0.9, 0], [0.02, 0.0, 0.5, 0], [0.3, 1e-2, 0.9, 0]], dtype=torch.float64, device=DEV)
    else:
        table = torch.tensor([[1e-2, 1e-2, 0.9, 0.999], [3e-3, 0.0, 0.8, 0.99], [1e-1, 0.1, 0.9, 0.999]], dtype=torch.float64,
                             device=DEV)

    def launch(m):
        p, a, b = p0.clone(), s1.clone(), s2.clone()
        if which.startswith('sgd'):
            first = 'first' in which
            K.sgd_step_grouped(p, g, a, m, table, grad_scale=0.5, first=first, nesterov=first)
        else:
            K.adam_step_grouped(p, g, a, b, m, table, 3, decoupled='adamw' in which, grad_scale=0.5, clip_coef=coef)
        torch.cuda.synchronize()
        return p.cpu(), a.cpu(), b.cpu()
    got, ref = launch(gid_f), launch(gid)
    start = (p0.cpu(), s1.cpu(), s2.cpu())
    n_state = 2 if which.startswith('sgd') else 3
    for k in range(n_state):
        assert torch.equal(bytes_of(got[k][frozen]), bytes_of(start[k][frozen])), (which, k, 'a frozen element moved')
        assert torch.equal(bytes_of(got[k][~frozen]), bytes_of(ref[k][~frozen])), (which, k, 'another element differs')
        assert not torch.equal(ref[k][frozen], start[k][frozen])                    # (the unfrozen launch does move them)
    # every element frozen: nothing moves
    none = launch(torch.full((N_EL,), L.OPT_FROZEN, dtype=torch.uint8, device=DEV))
    assert all(torch.equal(bytes_of(none[k]), bytes_of(start[k])) for k in range(3))


# ------------------------------------------------------------------------------------------------------------------- 8
def child(tmp_path, tag, *args, lr=0.01):
    out = str(tmp_path / f'{tag}.npz')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'finetune_child.py'), *map(str, args), out, str(lr)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


def test_deterministic_fast_with_frozen_stages_is_bitwise_reproducible(tmp_path):
    """deterministic='fast', frozen_stages=2, three SGD steps of batch 2 at 64 x 64 from the trained YuNet_n fixture, in two
    fresh processes: the same bytes for the whole contract; the frozen stages' parameters, momentum and BN buffers are the
    fixture's."""
    import helpers as Hh
    a = child(tmp_path, 'a', 'n', 'conv_stack_n_160.npz', 2, 64, 3, 2)
    b = child(tmp_path, 'b', 'n', 'conv_stack_n_160.npz', 2, 64, 3, 2)
    assert np.isfinite(a['losses']).all() and float(np.abs(a['grad']).max()) > 0
    for k in CONTRACT:
        assert np.array_equal(a[k], b[k]), k
    g = Hh.load_golden('conv_stack_n_160.npz')
    start = int(g['w:backbone.model0.bn1.num_batches_tracked'])
    assert int(a['num_batches_tracked'][0]) == start and int(a['num_batches_tracked'][-1]) == start + 3
    n_frozen = int(a['frozen_elements'])
    assert n_frozen > 0 and not a['grad'][:n_frozen].any() and not a['momentum'][:n_frozen].any()
    assert np.array_equal(a['params'][:432], g['w:backbone.model0.conv1.weight'].reshape(-1))
    assert np.array_equal(a['running_var'][:16], g['w:backbone.model0.bn1.running_var'])


def test_deterministic_fast_with_all_batchnorm_frozen_is_bitwise_reproducible(tmp_path):
    """deterministic='fast', every BatchNorm in eval() and every parameter training (the backward folds of frozen layers
    feed d(gamma) / d(beta)): three SGD steps in two fresh processes give the same bytes; the BN buffers are the fixture's.
    lr 1e-4: without batch statistics the trained fixture diverges at 0.01 on these batches (NaN in the third step, in the
    oracle as well), and NaN compares unequal to itself."""
    import helpers as Hh
    a = child(tmp_path, 'a', 'n', 'conv_stack_n_160.npz', 2, 64, 3, 'bn', lr=1e-4)
    b = child(tmp_path, 'b', 'n', 'conv_stack_n_160.npz', 2, 64, 3, 'bn', lr=1e-4)
    assert np.isfinite(a['losses']).all() and int(a['frozen_elements']) == 0
    assert np.isfinite(a['grad']).all() and np.isfinite(a['params']).all() and float(np.abs(a['grad']).max()) > 0
    for k in CONTRACT:
        assert np.array_equal(a[k], b[k]), k
    g = Hh.load_golden('conv_stack_n_160.npz')
    assert (a['num_batches_tracked'] == int(g['w:backbone.model0.bn1.num_batches_tracked'])).all()
    assert np.array_equal(a['running_var'][:16], g['w:backbone.model0.bn1.running_var'])
    assert np.array_equal(a['running_mean'][:16], g['w:backbone.model0.bn1.running_mean'])
    off = 16 * 27 + 16                                            # gamma | beta of the stem's BatchNorm
    assert a['grad'][off:off + 32].any() and not np.array_equal(a['params'][off:off + 16], g['w:backbone.model0.bn1.weight'])


# ------------------------------------------------------------------------------------------------------------------- 9
def test_bf16_storage_with_frozen_batchnorm_runs_and_keeps_the_frozen_bytes():
    import yunet_amd.synthetic as S
    from yunet_amd.optim import FusedSGD
    m, sd, arch, b = build('stages0')
    m.set_precision('bf16')
    all_bn(m)
    before = buffers(m)
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    was = {n: bytes_of(p) for n, p in m.named_parameters()}
    opt = FusedSGD(m, lr=0.01, momentum=0.9, weight_decay=5e-4)
    out = m.train_step(S.to_device(b, DEV), opt)
    out['loss'].backward()
    opt.step()
    torch.cuda.synchronize()
    assert m.engine.plan.act_dtype == torch.bfloat16 and np.isfinite(float(out['log_vars']['loss']))
    for k, v in before.items():
        assert torch.equal(bytes_of(m.state_dict()[k]), v), k
    for n, p in m.named_parameters():
        assert torch.equal(bytes_of(p), was[n]) == (n in frozen), n
    fp = m.engine.params
    assert frozen and all(not bool(fp.view(n, of=fp.grad).any()) for n in frozen)
