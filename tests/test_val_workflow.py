"""CPU: the validation workflow -- ('val', n) epochs with an eval-mode loss step.

  * what a validation step computes, pinned on the LIVE reference (skipped where the reference tree is absent): the
    unmodified detector under .eval() + no_grad against the oracle composed with every BatchNorm on its running statistics
    (finetune_ref.step_fp32 with flag False) -- the yardstick tests/test_val_workflow_gpu.py holds the HIP step to;
  * the plan's validation op lists, built on 'cpu' as in tests/test_finetune.py, and the training lists next to them;
  * the runner's workflow loop, hook stages, pass index, epoch mean and logger output with a stub model and stub sources;
  * tools/train.py up to the hand-over: one source per workflow entry."""
import ctypes as C
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

import finetune_ref as FR
import ref_stub
import yunet_amd
import yunet_amd._lib as L
import yunet_amd.engine as E
import yunet_amd.runner as R
import yunet_amd.tb_events as T
import yunet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

# (kind, N, H, W, batch seed): the three cases of the issue; seeds 31 and 33 are not tie-free
CASES = [('n', 2, 64, 64, 11), ('s', 3, 64, 96, 12), ('n', 3, 64, 96, 32)]
EVAL = lambda name: False          # noqa: E731  every BatchNorm layer on its running statistics


# ------------------------------------------------------------------------------------------------ the yardstick itself
@pytest.mark.skipif(not ref_stub.available(), reason='reference tree not present')
@pytest.mark.parametrize('kind,n,h,w,seed', CASES)
def test_eval_mode_loss_step_matches_live_reference(kind, n, h, w, seed):
    import yunet_amd.synthetic as S
    model, _ = ref_stub.build_detector(f'yunet_{kind}.py')
    sd = FR.warm_state(kind, 1)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    arch = O.yunet_arch(kind)
    b = S.make_batch(n, h, w, seed)
    model.eval()
    with torch.no_grad():
        losses = model.forward_train(b['img'], b['img_metas'], list(b['gt_bboxes']), b['gt_labels'], list(b['gt_keypointss']))
    lv, _, aux, _ = FR.step_fp32(b, sd, arch, EVAL)
    assert FR.near_tie(aux, b) == []
    for k in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps'):
        assert abs(float(losses[k]) - lv[k]) <= 1e-6 * abs(lv[k]) + 1e-7, (k, float(losses[k]), lv[k])
    now = model.state_dict()
    for k, v in sd.items():
        if k.endswith(('running_mean', 'running_var', 'num_batches_tracked')):
            assert torch.equal(now[k], v), k
    # and the train-mode step is another computation: a step that normalises with batch statistics cannot pass
    lt, _, _, _ = FR.step_fp32(b, sd, arch, lambda name: True)
    assert abs(lt['loss_obj'] - lv['loss_obj']) > 1e-2 * abs(lv['loss_obj'])


# ----------------------------------------------------------------------------------------------------------- op lists
def raw(op):
    return C.string_at(C.byref(op), C.sizeof(L.YunetOp))


def raw_list(ops):
    return [raw(op) for op in ops]


def training_lists(plan):
    out = {k: raw_list(getattr(plan, k)) for k in ('fwd_a', 'fwd_b', 'bwd')}
    for k in ('c_fwd_a', 'c_fwd_b', 'c_bwd', 'c_fwd_b_loss', 'c_fwd_b_rest', 'c_fwd_eval'):
        out[k] = raw_list(getattr(plan, k))
    return out


def engine(det=False, frozen=False):
    eng = E.YuNetEngine(O.yunet_arch('n'), 'cpu')
    eng.set_deterministic(det)
    if frozen:
        bn = [n for n in eng.layout.bn_names if n.startswith('backbone.model0') or n.startswith('backbone.model1')]
        keys = [k for k in eng.layout.entries if k.startswith('backbone.model0')]
        eng.set_frozen(bn, keys)
    return eng


def structure(ops):
    """the records without their pointers: what two plans of different engines share"""
    return [(op.opcode, tuple(op.i), tuple(op.f)) for op in ops]


@pytest.mark.parametrize('det,frozen', [(False, False), (True, False), ('fast', False), (False, True)],
                         ids=['default', 'det', 'det-fast', 'frozen'])
def test_validation_op_lists(det, frozen):
    eng = engine(det, frozen)
    plan = eng.get_plan(2, 64, 96, 1)
    assert getattr(plan, 'c_val', None) is None, 'built lazily'
    before = training_lists(plan)
    c_val = plan.val_ops()
    assert plan.val_ops() is c_val and len(c_val) == len(plan.val)
    after = training_lists(plan)
    assert before == after, 'the training lists moved'
    # ... and they are the lists of a plan that never heard of validation
    twin = engine(det, frozen).get_plan(2, 64, 96, 1)
    for k in ('fwd_a', 'fwd_b', 'bwd'):
        assert structure(getattr(plan, k)) == structure(getattr(twin, k)), k
    assert getattr(twin, 'c_val', None) is None
    # the list: fwd_eval, then what _build_eval skips, then the loss without a gradient and finalize
    ne = len(plan.fwd_eval)
    assert raw_list(plan.val[:ne]) == raw_list(plan.fwd_eval) == raw_list(plan.c_fwd_eval)
    codes = [op.opcode for op in plan.val]
    assert codes[ne:] == [L.OP_ASSIGN, L.OP_LOSS_NORM, L.OP_LOSS, L.OP_LOSS_FINALIZE]
    assign, norm, loss, fin = plan.val[ne:]
    assert raw(assign) == raw(plan.fwd_a[plan.assign_idx]) and raw(norm) == raw(plan.fwd_a[plan.assign_idx + 1])
    assert loss.p[6] is None and plan.fwd_b[0].p[6] == plan.dflat.data_ptr()
    patched = E.Plan._clone_op(plan.fwd_b[0])
    patched.p[6] = None
    assert raw(loss) == raw(patched), 'the loss op differs from the training step\'s in more than dflat'
    assert loss.loss.defer_num_total == 0
    patched = E.Plan._clone_op(plan.fwd_b[1])
    patched.p[2] = None
    assert raw(fin) == raw(patched) and fin.p[3] is None and fin.p[4] is None
    assert raw_list(c_val) == raw_list(plan.val)
    # nothing of the training step's bookkeeping
    assert L.OP_BN_FOLD not in codes and L.OP_MEMSET not in codes and L.OP_SGD not in codes
    assert not any(c in codes for c in (L.OP_DP_BWD, L.OP_STEM_BWD, L.OP_REDUCE_BATCH))
    batch = [op for op in plan.val if op.opcode == L.OP_BN_BATCH]
    assert batch and all(op.i[1] == 2 for op in batch), 'only the mode-2 fill from the running statistics'
    assert all(op.dp.out_has_bn == 0 for op in plan.val if op.opcode == L.OP_DP_FWD)
    # the deferred pair
    assert raw_list(plan.val_a) == raw_list(plan.val[:ne + 2]) == raw_list(plan.c_val_a)
    (ld,), (fd,) = plan.val_loss_def, plan.val_rest_def
    assert ld.opcode == L.OP_LOSS and ld.p[6] is None and ld.loss.defer_num_total == 1
    assert fd.opcode == L.OP_LOSS_FINALIZE and fd.p[3] == plan.norm.data_ptr() and fd.p[4] is None and fd.p[2] is None
    assert len(plan.c_val_loss_def) == 1 and len(plan.c_val_rest_def) == 1


def test_validation_lists_follow_the_bound_gt_and_image():
    eng = engine()
    plan = eng.get_plan(2, 64, 64, 1)
    plan.val_ops()
    ai = plan.val_assign_idx
    own = tuple(t.data_ptr() for t in plan.own_gt)
    assert (plan.c_val[ai].p[1], plan.c_val[ai].p[2], plan.c_val[ai].p[4]) == own
    gb, gk, gc = torch.zeros(2, 64, 4), torch.zeros(2, 64, 5, 3), torch.zeros(2, dtype=torch.int32)
    img = torch.zeros(2, 3, 64, 64)
    before = training_lists(plan)
    plan.bind_gt(gb, gk, gc)
    plan._bind_val(img)
    for arr in (plan.c_val, plan.c_val_a):
        assert (arr[ai].p[1], arr[ai].p[2], arr[ai].p[4]) == (gb.data_ptr(), gk.data_ptr(), gc.data_ptr())
    for op in (plan.c_val[ai + 2], plan.c_val_loss_def[0]):
        assert (op.p[3], op.p[4]) == (gb.data_ptr(), gk.data_ptr()) and op.p[6] is None
    stem = [i for i, op in enumerate(plan.val) if op.opcode == L.OP_STEM_FWD]
    assert stem and all(plan.c_val[i].p[0] == img.data_ptr() == plan.c_val_a[i].p[0] for i in stem)
    # the image went into the validation lists alone
    plan.bind_gt(*plan.own_gt)
    now = training_lists(plan)
    assert now == before


# ------------------------------------------------------------------------------------------------------------- runner
class StubModel(torch.nn.Module):
    """log values are a function of the batch, so the test knows the mean a validation epoch must report"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([1.0]))
        self.seen = []           # (mode by model.training, batch tag, grad mode)

    def _out(self, data):
        v = data['v']
        lv = OrderedDict(loss_cls=v, loss_bbox=2 * v, loss_obj=v * v, loss_kps=0.25 * v, loss=v + 1.0)
        return lv

    def train_step(self, data, optimizer):
        self.seen.append(('train' if self.training else 'eval', data['tag'], torch.is_grad_enabled()))
        loss = (self.w * data['v']).sum()
        return dict(loss=loss, log_vars=self._out(data), num_samples=data['n'])

    def val_step(self, data, optimizer):
        self.seen.append(('train' if self.training else 'eval', data['tag'], torch.is_grad_enabled()))
        return dict(loss=torch.tensor(0.0), log_vars=self._out(data), num_samples=data['n'])


class StubSource:
    def __init__(self, name, iters=3, bs=4, last=None):
        self.name, self.iters_per_epoch, self.bs, self.last = name, iters, bs, last
        self.asked = []

    def batch(self, it, device=None):
        self.asked.append(it)
        n = self.last if (self.last is not None and it % self.iters_per_epoch == self.iters_per_epoch - 1) else self.bs
        return dict(tag=(self.name, it), v=0.1 + 0.37 * it + (5.0 if self.name == 'val' else 0.0), n=n)


class Recorder(R.Hook):
    def __init__(self):
        self.calls = []

    def _rec(self, stage, runner):
        self.calls.append((stage, runner.epoch, runner.iter, runner.mode, runner.model.training))


for _stage in R.Hook.stages:
    setattr(Recorder, _stage, (lambda s: lambda self, runner: self._rec(s, runner))(_stage))


def make_runner(tmp_path, max_epochs, lines=None, loggers=('TextLoggerHook',), max_iters=None, checkpoints=None):
    m = StubModel()
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    lines = [] if lines is None else lines
    r = R.EpochBasedRunner(m, opt, str(tmp_path), lines.append, max_epochs=max_epochs, max_iters=max_iters)
    r.register_training_hooks(None, dict(), checkpoints, dict(interval=1, hooks=[dict(type=t) for t in loggers]))
    rec = Recorder()
    r.register_hook(rec, 'LOWEST')
    return r, m, rec, lines


def epoch_stages(calls):
    return [(c[0], c[1], c[2]) for c in calls if c[0].endswith('_epoch')]


def test_hook_stages_exist_and_map_onto_the_generic_ones():
    seen = []

    class H(R.Hook):
        def before_epoch(self, runner): seen.append('be')        # noqa: E704
        def after_epoch(self, runner): seen.append('ae')         # noqa: E704
        def before_iter(self, runner): seen.append('bi')         # noqa: E704
        def after_iter(self, runner): seen.append('ai')          # noqa: E704

    h = H()
    for s in ('before_val_epoch', 'before_val_iter', 'after_val_iter', 'after_val_epoch'):
        assert s in R.Hook.stages
        getattr(h, s)(None)
    assert seen == ['be', 'bi', 'ai', 'ae']


def test_train_val_alternate_in_mmcv_order(tmp_path):
    r, m, rec, _ = make_runner(tmp_path, 2)
    tr, va = StubSource('train'), StubSource('val', iters=2)
    hist = r.run([tr, va], [('train', 1), ('val', 1)], device='cpu')
    assert epoch_stages(rec.calls) == [
        ('before_train_epoch', 0, 0), ('after_train_epoch', 0, 3), ('before_val_epoch', 1, 3), ('after_val_epoch', 1, 3),
        ('before_train_epoch', 1, 3), ('after_train_epoch', 1, 6), ('before_val_epoch', 2, 6), ('after_val_epoch', 2, 6)]
    assert rec.calls[0][0] == 'before_run' and rec.calls[-1][0] == 'after_run'
    # per iteration: before_*_iter, step, after_*_iter; epoch / iter do not move in validation
    val_calls = [c for c in rec.calls if c[3] == 'val' and c[0] != 'after_run']
    assert [c[0] for c in val_calls[:6]] == ['before_val_epoch', 'before_val_iter', 'after_val_iter', 'before_val_iter',
                                             'after_val_iter', 'after_val_epoch']
    assert {(c[1], c[2]) for c in val_calls[:6]} == {(1, 3)} and {(c[1], c[2]) for c in val_calls[6:]} == {(2, 6)}
    assert all(c[4] is False for c in val_calls)
    assert all(c[4] is True for c in rec.calls if c[3] == 'train' and c[0] not in ('before_run',))
    # the model: eval + no_grad in validation, train + grad in training; val_step, not train_step
    assert [s[0] for s in m.seen] == ['train'] * 3 + ['eval'] * 2 + ['train'] * 3 + ['eval'] * 2
    assert [s[2] for s in m.seen] == [True] * 3 + [False] * 2 + [True] * 3 + [False] * 2
    assert [s[1][0] for s in m.seen] == ['train'] * 3 + ['val'] * 2 + ['train'] * 3 + ['val'] * 2
    assert r.epoch == 2 and r.iter == 6 and tr.asked == list(range(6))
    assert va.asked == [0, 1, 2, 3], 'pass 0, then pass 1'
    assert [e['mode'] for e in hist if 'mode' in e] == ['val', 'val']


def test_two_train_epochs_per_validation_and_a_short_last_cycle(tmp_path):
    r, m, rec, _ = make_runner(tmp_path, 3)
    tr, va = StubSource('train', iters=2), StubSource('val', iters=2)
    r.run([tr, va], [('train', 2), ('val', 1)], device='cpu')
    assert [s[:2] for s in epoch_stages(rec.calls)] == [
        ('before_train_epoch', 0), ('after_train_epoch', 0), ('before_train_epoch', 1), ('after_train_epoch', 1),
        ('before_val_epoch', 2), ('after_val_epoch', 2),
        ('before_train_epoch', 2), ('after_train_epoch', 2),            # the 'train' entry stops at max_epochs
        ('before_val_epoch', 3), ('after_val_epoch', 3)]
    assert va.asked == [0, 1, 2, 3] and r.epoch == 3


def test_pass_index_rule():
    f = R.EpochBasedRunner.val_pass_index
    wf = [('train', 1), ('val', 1)]
    assert [f(wf, e, 1, 0) for e in (1, 2, 3, 7)] == [0, 1, 2, 6]
    wf = [('train', 2), ('val', 3)]
    assert [f(wf, 2, 1, j) for j in range(3)] == [0, 1, 2] and [f(wf, 4, 1, j) for j in range(3)] == [3, 4, 5]
    assert f(wf, 5, 1, 0) == 6, 'a last cycle cut short at max_epochs = 5 is still a cycle'
    wf = [('val', 1), ('train', 2), ('val', 1)]
    assert [f(wf, 0, 0, 0), f(wf, 2, 2, 0), f(wf, 2, 0, 0), f(wf, 4, 2, 0)] == [0, 1, 2, 3]


def test_resumed_run_continues_the_validation_sequence(tmp_path):
    r, m, rec, _ = make_runner(tmp_path, 2, checkpoints=dict(interval=1))
    tr, va = StubSource('train'), StubSource('val', iters=2)
    r.run([tr, va], [('train', 1), ('val', 1)], device='cpu')
    assert va.asked == [0, 1, 2, 3]
    r2, m2, rec2, _ = make_runner(tmp_path / 'b', 3)
    r2.resume(str(tmp_path / 'epoch_2.pth'))
    assert (r2.epoch, r2.iter) == (2, 6)
    tr2, va2 = StubSource('train'), StubSource('val', iters=2)
    r2.run([tr2, va2], [('train', 1), ('val', 1)], device='cpu')
    assert tr2.asked == [6, 7, 8] and va2.asked == [4, 5], 'the third validation epoch of the run is pass 2'


def test_epoch_mean_weights_by_num_samples_with_a_short_last_batch(tmp_path):
    r, m, rec, lines = make_runner(tmp_path, 1, loggers=('TextLoggerHook', 'TextLoggerHook'))
    tr, va = StubSource('train', iters=1), StubSource('val', iters=3, bs=4, last=1)
    hist = r.run([tr, va], [('train', 1), ('val', 1)], device='cpu')
    val = [e for e in hist if e.get('mode') == 'val']
    assert len(val) == 1, 'one entry, however many logger hooks'
    e = val[0]
    assert e['epoch'] == 1 and e['iter'] == 1 and list(e)[:3] == ['mode', 'epoch', 'iter']
    v = np.array([0.1 + 0.37 * i + 5.0 for i in range(3)], dtype=np.float64)
    n = np.array([4, 4, 1], dtype=np.float64)
    want = dict(loss_cls=v, loss_bbox=2 * v, loss_obj=v * v, loss_kps=0.25 * v, loss=v + 1.0)
    assert set(e) == {'mode', 'epoch', 'iter'} | set(want)
    for k, x in want.items():
        ref = np.sum(x * n) / np.sum(n)
        assert abs(e[k] - ref) <= 1e-12 * abs(ref), (k, e[k], ref)
        assert abs(e[k] - np.mean(x)) > 1e-3, 'an unweighted mean would differ'
    assert r.val_sums.dtype == torch.float64 and float(r.val_sums[-1]) == 9.0
    out = [ln for ln in lines if ln.startswith('Epoch(val)')]
    assert len(out) == 2 and out[0].startswith('Epoch(val) [1][3]\tloss_cls: ') and out[0] == out[1]


def test_val_tags_in_the_tensorboard_event_file(tmp_path):
    r, m, rec, _ = make_runner(tmp_path, 2, loggers=('TextLoggerHook', 'TensorboardLoggerHook'))
    hist = r.run([StubSource('train', iters=2), StubSource('val', iters=2)], [('train', 1), ('val', 1)], device='cpu')
    ev_dir = tmp_path / 'tf_logs'
    (name,) = os.listdir(ev_dir)
    ev = T.read_events(str(ev_dir / name))
    val = [e for e in hist if e.get('mode') == 'val']
    for k in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps', 'loss'):
        got = [(e[0], e[2]) for e in ev if e[1] == 'val/' + k]
        assert [s for s, _ in got] == [2, 4], (k, got)               # step = runner.iter: iterations completed
        assert [x for _, x in got] == pytest.approx([val[0][k], val[1][k]], rel=1e-6)
    assert len([e for e in ev if e[1] == 'train/loss']) == 4


@pytest.mark.parametrize('workflow', [[('train', 1), ('test', 1)], [('train', 0)], [('train', 1.0)], [('train',)], ['train'],
                                      [('train', True)], [('val', 1)], [], 'train', [('train', 1), ('val', -1)]])
def test_malformed_workflows_raise(tmp_path, workflow):
    r, m, rec, _ = make_runner(tmp_path, 1)
    sources = [StubSource('s') for _ in range(max(1, len(workflow)))]
    with pytest.raises(ValueError) as e:
        r.run(sources, workflow, device='cpu')
    bad = [w for w in (workflow if isinstance(workflow, list) else [workflow])
           if not (isinstance(w, tuple) and len(w) == 2 and w[0] in ('train', 'val') and type(w[1]) is int and w[1] > 0)]
    assert repr(bad[0] if bad and isinstance(workflow, list) else workflow) in str(e.value)
    assert m.seen == [] and rec.calls == []


def test_one_source_per_workflow_entry(tmp_path):
    r, m, rec, _ = make_runner(tmp_path, 1)
    with pytest.raises(ValueError, match='one source per entry'):
        r.run([StubSource('train')], [('train', 1), ('val', 1)], device='cpu')
    with pytest.raises(ValueError, match='one source per entry'):
        r.run([StubSource('train'), StubSource('val')], [('train', 1)], device='cpu')
    assert m.seen == []
    r.run(StubSource('train'), [('train', 1)], device='cpu')        # a bare source still serves a one-entry workflow
    assert len(m.seen) == 3


def test_a_max_iters_cut_runs_no_validation(tmp_path):
    r, m, rec, _ = make_runner(tmp_path, 3, max_iters=4)
    tr, va = StubSource('train'), StubSource('val')
    hist = r.run([tr, va], [('train', 1), ('val', 1)], device='cpu')
    assert r.iter == 4 and va.asked == [3 * 0 + i for i in range(3)], 'the validation epoch after the first full epoch only'
    assert [c[0] for c in rec.calls][-1] == 'after_run'
    assert [s[1][0] for s in m.seen] == ['train'] * 3 + ['val'] * 3 + ['train']
    assert len([e for e in hist if e.get('mode') == 'val']) == 1
    # ... and cut inside the first epoch: none at all
    r, m, rec, _ = make_runner(tmp_path / 'b', 3, max_iters=2)
    va = StubSource('val')
    r.run([StubSource('train'), va], [('train', 1), ('val', 1)], device='cpu')
    assert va.asked == [] and r.mode == 'train' and not any(c[0].startswith(('before_val', 'after_val')) for c in rec.calls)


def test_train_detector_accepts_a_list_of_sources(monkeypatch, tmp_path):
    seen = {}

    def fake_run(self, data_sources, workflow=None, device=None):
        seen.update(sources=data_sources, workflow=workflow)
        return []

    monkeypatch.setattr(R.EpochBasedRunner, 'run', fake_run)
    monkeypatch.setattr(R, 'build_optimizer', lambda model, cfg: torch.optim.SGD(model.parameters(), lr=0.1))
    cfg = yunet_amd.Config(dict(optimizer=dict(type='SGD', lr=0.1), optimizer_config=dict(), lr_config=None,
                                runner=dict(type='EpochBasedRunner', max_epochs=1), work_dir=str(tmp_path),
                                workflow=[('train', 1), ('val', 1)]))
    a, b = StubSource('train'), StubSource('val')
    R.train_detector(StubModel(), [a, b], cfg, device='cpu', log=lambda *x: None)
    assert seen['sources'] == [a, b] and [tuple(w) for w in seen['workflow']] == [('train', 1), ('val', 1)]
    cfg2 = yunet_amd.Config(dict(cfg, workflow=[('train', 1)]))
    R.train_detector(StubModel(), a, cfg2, device='cpu', log=lambda *x: None)
    assert seen['sources'] == [a]


# ---------------------------------------------------------------------------------------------------- tools/train.py
CFG = os.path.join(ROOT, 'configs', 'yunet_n.py')
SYNTH = ['data.samples_per_gpu=4', 'data.train.type=SyntheticWiderFace', 'data.train.img_scale=(160,160)',
         'data.train.iters_per_epoch=2']


VAL = """
data['val'] = dict(type='SyntheticWiderFace', img_scale=(160, 160), iters_per_epoch=3, test_mode=True, ann_file='val/labelv2.txt',
                   pipeline=[dict(type='LoadImageFromFile'),
                             dict(type='MultiScaleFlipAug', img_scale=(160, 160), flip=False, transforms=[])])
"""


def config_with_val(tmp_path):
    path = tmp_path / 'yunet_n.py'
    path.write_text(open(CFG).read() + VAL)
    return str(path)


def hand_over(tmp_path, monkeypatch, extra, config=CFG):
    import train as TT
    seen = {}

    def fake_train(model, ds, cfg, **kw):
        seen.update(model=model, ds=ds, cfg=cfg, kw=kw)
        return ['history']

    monkeypatch.setattr(TT.R, 'train_detector', fake_train)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda i: None)
    out = TT.main([config, '--work-dir', str(tmp_path / 'w'), '--seed', '5', '--no-validate', '--cfg-options'] + SYNTH + extra)
    assert out == ['history']
    return TT, seen


def test_tool_passes_one_source_for_the_shipped_workflow(tmp_path, monkeypatch):
    TT, seen = hand_over(tmp_path, monkeypatch, [])
    assert type(seen['ds']).__name__ == 'SyntheticWiderFace' and seen['ds'].bs == 4
    assert [tuple(w) for w in seen['cfg'].workflow] == [('train', 1)]


def test_tool_builds_the_second_source_from_data_val_with_the_train_pipeline(tmp_path, monkeypatch):
    built = []
    import train as TT
    real = TT.build_source

    def spy(cfg, rank, world, seed, dcfg=None):
        built.append((seed, None if dcfg is None else dict(dcfg)))
        return real(cfg, rank, world, seed, dcfg)

    monkeypatch.setattr(TT, 'build_source', spy)
    TT, seen = hand_over(tmp_path, monkeypatch, ["workflow=[('train',1),('val',1)]"], config_with_val(tmp_path))
    assert [tuple(w) for w in seen['cfg'].workflow] == [('train', 1), ('val', 1)]
    ds = seen['ds']
    assert isinstance(ds, list) and len(ds) == 2 and all(type(s).__name__ == 'SyntheticWiderFace' for s in ds)
    assert ds[0].iters_per_epoch == 2 and ds[1].iters_per_epoch == 3 and ds[1].bs == 4
    (s0, d0), (s1, d1) = built
    assert d0 is None and s1 - s0 == TT.VAL_SEED_OFFSET == 1000003
    cfg = seen['cfg']
    assert d1['pipeline'] == list(cfg.data.train.pipeline) and d1['pipeline'] != list(cfg.data.val.pipeline)
    assert 'test_mode' not in d1 and d1['ann_file'] == cfg.data.val.ann_file
    assert list(cfg.data.val.pipeline)[1]['type'] == 'MultiScaleFlipAug', 'data.val itself is left alone (the EvalHook reads it)'


def test_val_source_config_flattens_a_multi_image_mix_train_set(tmp_path):
    import train as TT
    with pytest.raises(ValueError, match='no data.val'):
        TT.val_source_config(yunet_amd.Config(dict(yunet_amd.Config.fromfile(CFG), workflow=[('train', 1), ('val', 1)])))
    cfg = yunet_amd.Config.fromfile(config_with_val(tmp_path))
    inner = dict(cfg.data.train)
    load, rest = list(inner['pipeline'][:2]), list(inner['pipeline'][2:])
    inner['pipeline'] = load
    cfg.data.train = dict(type='MultiImageMixDataset', dataset=inner, pipeline=rest)
    v = TT.val_source_config(cfg)
    assert v['pipeline'] == load + rest and 'test_mode' not in v and v['type'] == cfg.data.val.type
    assert cfg.data.val.test_mode is True
