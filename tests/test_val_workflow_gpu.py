"""-m gpu: the validation workflow.

  * kernel: the value-only instances of the loss kernel (kernels.loss(grad=False)) against the gradient-writing ones, byte
    for byte, normalised and with the deferred normaliser, default terms and Varifocal + BalancedL1 + BoundedIoU;
  * step: YuNet.forward_train under model.eval() against the oracle with every BatchNorm on its running statistics
    (finetune_ref.step_fp32 with flag False, pinned on the live reference by tests/test_val_workflow.py) at the bars of
    tests/test_finetune_gpu.py, and what it must leave alone;
  * a validation step between two training steps (and between two micro-batches) changes no byte of the second;
  * the deferred form in a single-process group, bf16 storage, and train_detector end to end.
Shapes are the small ones of tests/test_finetune_gpu.py: what can fail here is wiring and one compile-time switch."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import finetune_ref as FR
import loss_terms_ref as LT
import yunet_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('n', 2, 64, 64, 11), ('s', 3, 64, 96, 12), ('n', 3, 64, 96, 32)]
EVAL = lambda name: False          # noqa: E731
KEYS = ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps')


def bytes_of(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()


# ------------------------------------------------------------------------------------------------------------- kernel
@functools.lru_cache(None)
def loss_case(key):
    return LT.make_case(*((2, 64, 64, 41) if key == '2x64' else (5, 96, 96, 23)))


@pytest.mark.parametrize('defer', [False, True], ids=['normalised', 'deferred'])
@pytest.mark.parametrize('terms', ['default', 'mixed'])
@pytest.mark.parametrize('key', ['2x64', '5x96'])       # 168 priors in one block | 945 in four
def test_value_only_loss_kernel_equals_the_gradient_writing_one(key, terms, defer):
    import yunet_amd._lib as L
    import yunet_amd.kernels as K
    case = loss_case(key)
    cfg = LT.make_cfg(**({} if terms == 'default' else LT.GOLDEN_CONFIGS['mixed']))
    kc, kt = LT.kernel_cfg(cfg, defer)
    if terms != 'default':
        kc.terms = kt
    d = {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in case.items()}
    N, P, _ = d['flat'].shape
    blocks = int(L.load().yunet_loss_blocks(N, P))
    assert blocks == (1 if key == '2x64' else 4)
    args = (d['flat'], d['gt_inds'], d['max_overlaps'], d['gt_boxes'], d['gt_kps'], d['img_stats'], d['sizes'], d['strides'], kc)
    norm = K.loss_norm(d['img_stats'])
    part = {g: torch.full((blocks, 4), float('nan'), device=DEV) for g in (True, False)}
    peak = {}
    out = {}
    total = lambda: torch.cuda.memory_stats()['allocated_bytes.all.allocated']      # noqa: E731  cumulative: frees do not lower it
    for g in (True, False):
        torch.cuda.synchronize()
        base = total()
        out[g] = K.loss(*args, norm=norm, grad=g, partials=part[g])
        torch.cuda.synchronize()
        peak[g] = total() - base           # bytes the call asked the allocator for
    (la, da, _), (lb, db, _) = out[True], out[False]
    assert db is None and da is not None and bool(torch.isfinite(da).all())
    flat_bytes = d['flat'].numel() * 4
    assert peak[True] >= flat_bytes > peak[False], (peak, flat_bytes)      # no [N,P,16] buffer behind the value-only launch
    assert bool(torch.isfinite(part[True]).all()) and float(part[True].abs().sum()) > 0
    assert torch.equal(bytes_of(part[True]), bytes_of(part[False])), 'partial rows'
    assert torch.equal(bytes_of(la), bytes_of(lb)), 'losses'
    if defer:       # un-normalised cls / bbox / obj: not what the normalised launch gives (num_pos > 1 in both cases)
        kn, _ = LT.kernel_cfg(cfg, False)
        if terms != 'default':
            kn.terms = kt
        ln, _, _ = K.loss(*args[:-1], kn, norm=norm, grad=False)
        assert not torch.equal(ln[:3].cpu(), lb[:3].cpu()) and torch.equal(ln[3].cpu(), lb[3].cpu())


# --------------------------------------------------------------------------------------------------------------- step
def build(kind, n, h, w, seed, precision='fp32', deterministic=False):
    """as tests/test_finetune_gpu.build: fresh weights, the BatchNorm buffers one train-mode step leaves behind"""
    import yunet_amd
    import yunet_amd.synthetic as S
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    m = yunet_amd.build_detector(cfg.model)
    sd = FR.warm_state(kind, 1)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).train()
    m.set_precision(precision)
    m.set_deterministic(deterministic)
    return m, sd, O.yunet_arch(kind), S.make_batch(n, h, w, seed)


@functools.lru_cache(None)
def reference(kind, n, h, w, seed):
    import yunet_amd.synthetic as S
    lv, _, aux, after = FR.step_fp32(S.make_batch(n, h, w, seed), FR.warm_state(kind, 1), O.yunet_arch(kind), EVAL)
    return lv, aux


def state_bytes(m, opt=None):
    out = {'param/' + k: bytes_of(p) for k, p in m.named_parameters()}
    out.update({'grad/' + k: bytes_of(p.grad) for k, p in m.named_parameters() if p.grad is not None})
    out.update({'buffer/' + k: bytes_of(v) for k, v in m.named_buffers()})
    out['flat_grad'] = bytes_of(m.engine.params.grad)
    if opt is not None:
        out['momentum'] = bytes_of(opt._buf)
    return out


@pytest.mark.parametrize('kind,n,h,w,seed', CASES)
def test_validation_step_vs_oracle_and_what_it_leaves_alone(kind, n, h, w, seed):
    import yunet_amd.synthetic as S
    from yunet_amd.optim import FusedSGD
    m, sd, arch, b = build(kind, n, h, w, seed)
    lv, aux = reference(kind, n, h, w, seed)
    assert FR.near_tie(aux, b) == []
    bd = S.to_device(b, DEV)
    m.eval()
    losses = m.forward_train(**bd)              # grad mode ON: still no graph
    torch.cuda.synchronize()
    eng, plan = m.engine, m.engine.plan
    assert set(losses) == set(KEYS) and not any(v.requires_grad or v.grad_fn is not None for v in losses.values())
    with pytest.raises(RuntimeError, match='does not require grad'):
        sum(losses.values()).backward()
    assert torch.equal(plan.gt_inds.cpu(), aux['gt_inds'].int()), 'assignment'
    ref_flat = aux['flat']
    err = float((plan.flat.cpu().double() - ref_flat.double()).abs().max() / ref_flat.double().abs().max())
    print(f'[{kind} {n}x{h}x{w}] flat rel err {err:.2e}')
    assert err < 5e-4
    for k in KEYS:
        print(f'[{kind} {n}x{h}x{w}] {k} {float(losses[k]):.7g} oracle {lv[k]:.7g}')
        assert abs(float(losses[k]) - lv[k]) <= 1e-4 * abs(lv[k]) + 1e-6, (k, float(losses[k]), lv[k])
    flat_val = bytes_of(plan.flat)
    n_plans = len(eng.plans)
    assert torch.equal(bytes_of(eng.forward_eval(bd['img'].float().contiguous())), flat_val), 'the eval conv stack'
    assert len(eng.plans) == n_plans == 1 and eng.plan is plan
    # one training step on the same geometry: the same plan (the validation step read no module flag: nothing is frozen)
    m.train()
    opt = FusedSGD(m, lr=1e-3, momentum=0.9, weight_decay=5e-4)
    out = m.train_step(bd, opt)
    opt.zero_grad()
    out['loss'].backward()
    opt.step()
    torch.cuda.synchronize()
    assert len(eng.plans) == 1 and eng.plan is plan and plan.frozen_bn == frozenset()
    fresh, acc_launches = eng._grad_fresh, dict(eng.accum_launches)
    before = state_bytes(m, opt)
    assert int(before['momentum'].max()) > 0 and int(before['flat_grad'].max()) > 0
    # ... and a validation step after it: every parameter, .grad, momentum and BatchNorm buffer keeps its bytes
    m.eval()
    with torch.no_grad():
        res = m.val_step(bd, opt)
    torch.cuda.synchronize()
    now = state_bytes(m, opt)
    assert set(now) == set(before)
    for k, v in before.items():
        assert torch.equal(now[k], v), k
    assert len(eng.plans) == 1 and eng.plan is plan
    assert eng._grad_fresh == fresh and eng.accum_launches == acc_launches and m._log_pending is None
    assert list(res['log_vars']) == list(KEYS) + ['loss'] and res['num_samples'] == n and not res['loss'].requires_grad
    got = [float(v) for v in res['log_vars'].values()]
    assert got == res['log_tensor'].cpu().tolist() == plan.losses[:5].cpu().tolist()
    assert got[4] == float(np.float32(np.float32(np.float32(got[0]) + np.float32(got[1])) + np.float32(got[2])) + np.float32(got[3]))
    m.train()
    assert all(mod.training for mod in m.modules())


# ------------------------------------------------------------------------------------------------------- interleaving
def run_sequence(seq, accumulate):
    """seq of ('train' | 'val', batch) on one model under deterministic='fast' -> bytes after the last training step"""
    import yunet_amd.synthetic as S
    from yunet_amd.optim import FusedSGD
    m, _, _, _ = build('n', 2, 64, 64, 11, deterministic='fast')
    if accumulate:
        m.set_grad_accumulation(True)
    opt = FusedSGD(m, lr=1e-3, momentum=0.9, weight_decay=5e-4)
    opt.zero_grad()
    last = None
    for what, b in seq:
        bd = S.to_device(b, DEV)
        if what == 'val':
            m.eval()
            with torch.no_grad():
                m.val_step(bd, opt)
            m.train()
            continue
        out = m.train_step(bd, opt)
        if accumulate:
            (out['loss'] / 2).backward()
        else:
            opt.zero_grad()
            out['loss'].backward()
            opt.step()
        last = [float(v) for v in out['log_vars'].values()]
    torch.cuda.synchronize()
    grad = bytes_of(m.engine.params.grad)
    if accumulate:
        opt.step()
        torch.cuda.synchronize()
    return dict(losses=last, grad=grad, params=bytes_of(m.engine.params.data), momentum=bytes_of(opt._buf),
                buffers={k: bytes_of(v) for k, v in m.named_buffers()})


@pytest.mark.parametrize('accumulate', [False, True], ids=['steps', 'micro_batches'])
def test_a_validation_step_in_between_changes_nothing(accumulate):
    import yunet_amd.synthetic as S
    b0, bv, b1 = S.make_batch(2, 64, 64, 11), S.make_batch(2, 64, 64, 32), S.make_batch(2, 64, 64, 14)
    a = run_sequence([('train', b0), ('val', bv), ('train', b1)], accumulate)
    c = run_sequence([('train', b0), ('train', b1)], accumulate)
    assert a['losses'] == c['losses']
    for k in ('grad', 'params', 'momentum'):
        assert torch.equal(a[k], c[k]), k
    assert a['buffers'].keys() == c['buffers'].keys() and all(torch.equal(a['buffers'][k], c['buffers'][k]) for k in c['buffers'])
    assert int(a['grad'].max()) > 0


# ------------------------------------------------------------------------------------------------------ deferred form
def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _deferred_worker(rank, port, out):
    """a single-process group with always_bucket, as tests/test_ddp_gpu.py forces the multi-GPU paths at world size 1"""
    import torch.distributed as dist
    import yunet_amd.synthetic as S
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    res = {}
    for mode in ('plain', 'deferred'):
        m, _, _, b = build('n', 3, 64, 96, 32)
        m.eval()
        eng = m._ensure_engine(dev)
        eng.always_bucket = mode == 'deferred'
        losses = m.forward_train(**S.to_device(b, dev))
        torch.cuda.synchronize()
        res[mode] = dict(losses=[float(losses[k]) for k in KEYS], raw=eng.plan.losses[:5].cpu().tolist(),
                         gt_inds=eng.plan.gt_inds.cpu(), norm=eng.plan.norm.cpu().tolist(),
                         partials=float(eng.plan.loss_partials[:, :3].sum()))
    out.update(res)
    dist.barrier()
    dist.destroy_process_group()


def test_deferred_validation_step_equals_the_undeferred_one():
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_deferred_worker, args=(_free_port(), out), nprocs=1, join=True)
    a, b = out['plain'], out['deferred']
    assert a['raw'] == b['raw'] and a['losses'] == b['losses'] and torch.equal(a['gt_inds'], b['gt_inds'])
    assert a['norm'] == b['norm'] and a['norm'][0] > 1.0
    assert a['partials'] != b['partials'], 'the deferred loss launch leaves cls / bbox / obj un-normalised'
    lv, _ = reference('n', 3, 64, 96, 32)
    for k, v in zip(KEYS, b['losses']):
        assert abs(v - lv[k]) <= 1e-4 * abs(lv[k]) + 1e-6, (k, v, lv[k])


# ------------------------------------------------------------------------------------------------------- bf16 storage
def test_validation_step_with_bf16_storage():
    """the bar of tests/test_bf16_gpu.py::test_bf16_step_vs_fp32_step_and_oracle for a forward (5 % per loss), at that
    test's smaller shape (YuNet_s, 8 x 160 x 160: enough positives for a loss of a bf16 forward to be a stable number)"""
    import yunet_amd.synthetic as S
    kind, n, h, seed = 's', 8, 160, 77
    m, sd, arch, b = build(kind, n, h, h, seed, precision='bf16')
    lv, _, aux, _ = FR.step_fp32(b, sd, arch, EVAL)
    m.eval()
    m._ensure_engine(torch.device(DEV, torch.cuda.current_device()))
    before = {k: bytes_of(v) for k, v in m.state_dict().items()}
    with torch.no_grad():
        losses = m.forward_train(**S.to_device(b, DEV))
    torch.cuda.synchronize()
    plan = m.engine.plan
    assert plan.act_dtype == torch.bfloat16 and m.engine.precision == 'bf16'
    for k in KEYS:
        print(f'[bf16] {k} {float(losses[k]):.7g} oracle {lv[k]:.7g}')
        assert abs(float(losses[k]) - lv[k]) <= 5e-2 * abs(lv[k]) + 1e-6, (k, float(losses[k]), lv[k])
    now = {k: bytes_of(v) for k, v in m.state_dict().items()}
    assert now.keys() == before.keys() and all(torch.equal(now[k], before[k]) for k in before)
    assert not bool(m.engine.params.grad.any())


# --------------------------------------------------------------------------------------------------------- end to end
def _e2e_cfg(tmp_path):
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    pipe = [dict(t, img_scale=(64, 64)) if t['type'] == 'Resize' else dict(t) for t in cfg.data.train.pipeline]
    cfg.merge_from_dict({'runner.max_epochs': 2, 'work_dir': str(tmp_path), 'checkpoint_config': None,
                         'workflow': [('train', 1), ('val', 1)]})
    cfg['log_config'] = dict(interval=1, hooks=[dict(type='TextLoggerHook')])
    return cfg, pipe


def test_train_detector_runs_the_workflow_end_to_end(tmp_path):
    import yunet_amd
    import yunet_amd.runner as R
    cfg, pipe = _e2e_cfg(tmp_path)
    sources = lambda: [R.SyntheticSourceImages(pipe, samples_per_gpu=2, iters_per_epoch=2, pool=4, seed=s) for s in (0, 1000003)]  # noqa: E731
    snaps = []

    class Snapshot(R.Hook):
        def before_val_epoch(self, runner):
            assert runner.mode == 'val' and not runner.model.training and not torch.is_grad_enabled()
            snaps.append({k: v.detach().clone() for k, v in runner.model.state_dict().items()})

    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(FR.warm_state('n', 1), strict=True)
    real = R.EpochBasedRunner.register_training_hooks

    def with_snapshot(self, *a, **kw):
        real(self, *a, **kw)
        self.register_hook(Snapshot(), 'LOWEST')

    R.EpochBasedRunner.register_training_hooks = with_snapshot
    lines = []
    try:
        hist = R.train_detector(m, sources(), cfg, validate=False, device=DEV, log=lines.append)
    finally:
        R.EpochBasedRunner.register_training_hooks = real
    torch.cuda.synchronize()
    val = [e for e in hist if e.get('mode') == 'val']
    assert len(val) == 2 and [(e['epoch'], e['iter']) for e in val] == [(1, 2), (2, 4)]
    assert len([e for e in hist if e.get('mode') != 'val']) == 4
    assert len([ln for ln in lines if ln.startswith('Epoch(val) [')]) == 2
    assert not m.training and len(snaps) == 2          # the run ended on a validation epoch; the next train() puts it back
    assert not torch.equal(snaps[0]['backbone.model0.conv1.weight'], snaps[1]['backbone.model0.conv1.weight'])
    # the hand loop: the model as each validation epoch found it, eval(), val_step over the same pass indices
    keys = list(KEYS) + ['loss']
    for v, (snap, entry) in enumerate(zip(snaps, val)):
        twin = yunet_amd.build_detector(cfg.model)
        twin.load_state_dict(snap, strict=True)
        twin.to(DEV).eval()
        src = sources()[1]
        tot, cnt = np.zeros(5, dtype=np.float64), 0.0
        with torch.no_grad():
            for i in range(2):
                out = twin.val_step(src.batch(v * 2 + i, DEV), None)
                tot += np.array([float(out['log_vars'][k]) for k in keys], dtype=np.float64) * out['num_samples']
                cnt += out['num_samples']
        for k, want in zip(keys, tot / cnt):
            assert abs(entry[k] - want) <= 1e-12 * abs(want), (v, k, entry[k], want)
    assert any(abs(val[0][k] - val[1][k]) > 1e-6 for k in keys)
