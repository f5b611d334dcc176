"""CPU: fine-tuning in the fused engine -- the surface (YuNetBackbone frozen_stages / norm_eval, the
modules' own flags, the config path), the plan key per freeze signature, the op lists of frozen plans built on 'cpu', and
the optimizers' group map with the byte that means no update."""
import os

import pytest
import torch
import torch.nn as nn

import yunet_amd
import yunet_amd._lib as L
import yunet_amd.engine as E
import yunet_oracle as O
from yunet_amd.optim import FusedAdam, FusedSGD, build_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 64, 64, 64)


def model(kind='n', **backbone):
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    cfg.model.backbone.update(backbone)
    return yunet_amd.build_detector(cfg.model), cfg


def bns(m):
    return {n: x for n, x in m.named_modules() if isinstance(x, nn.BatchNorm2d)}


def stage_of(name):
    return int(name.split('.')[1][len('model'):]) if name.startswith('backbone.model') else None


def engine(kind='n', det=False):
    eng = E.YuNetEngine(O.yunet_arch(kind), 'cpu')
    eng.set_deterministic(det)
    return eng


def stage_signature(eng, k):
    """what frozen_stages = k means to the engine: BN layers and parameters of model0 .. model{k}"""
    bn = tuple(n for n in eng.layout.bn_names if stage_of(n) is not None and stage_of(n) <= k)
    keys = tuple(n for n in eng.layout.entries if stage_of(n) is not None and stage_of(n) <= k)
    return bn, keys


def opcodes(ops):
    return [op.opcode for op in ops]


def memsets(plan, ops):
    g0 = plan.eng.params.grad.data_ptr()
    return [((op.p[0] - g0) // 4, (op.i[0] + (op.i[1] << 32)) // 4) for op in ops if op.opcode == L.OP_MEMSET]


# ------------------------------------------------------------------------------------------------------------ surface
def test_constructor_defaults_freeze_nothing_and_reference_configs_load():
    m, cfg = model()
    bb = m.backbone
    assert (bb.frozen_stages, bb.norm_eval) == (-1, False)
    assert 'frozen_stages' not in cfg.model.backbone and 'norm_eval' not in cfg.model.backbone
    m.train()
    assert all(p.requires_grad for p in m.parameters()) and all(b.training for b in bns(m).values())
    m.load_state_dict(O.init_state(O.yunet_arch('n'), seed=1), strict=True)
    with pytest.raises(ValueError):
        model(frozen_stages=len(bb.stage_channels))


@pytest.mark.parametrize('k', [0, 2, 5])
def test_frozen_stages_sets_the_modules_own_flags(k):
    m, _ = model(frozen_stages=k)
    for mode in (True, False, True):
        m.train(mode)
        for name, p in m.named_parameters():
            s = stage_of(name)
            assert p.requires_grad == (s is None or s > k), name
        for name, mod in m.named_modules():
            s = stage_of(name)
            if s is not None and s <= k:
                assert not mod.training, name
            elif name:
                assert mod.training == mode, name


def test_norm_eval_puts_the_backbone_batchnorms_into_eval_on_train():
    m, _ = model(norm_eval=True)
    m.train()
    for name, b in bns(m).items():
        assert b.training == (not name.startswith('backbone.')), name
    assert all(p.requires_grad for p in m.parameters())
    assert m.backbone.model1.conv1.training and m.backbone.model1.training       # the units themselves train
    m.eval()
    assert not any(b.training for b in bns(m).values())


def test_config_path_reaches_both_arguments():
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    cfg.merge_from_dict({'model.backbone.frozen_stages': 2, 'model.backbone.norm_eval': True})
    m = yunet_amd.build_detector(cfg.model)
    assert (m.backbone.frozen_stages, m.backbone.norm_eval) == (2, True)
    m.train()
    assert not m.backbone.model2.conv2.bn.training and not m.backbone.model4.conv1.bn.training
    assert not m.backbone.model2.conv1.conv1.weight.requires_grad and m.backbone.model3.conv1.conv1.weight.requires_grad


def test_model_reads_the_signature_from_the_flags(monkeypatch):
    m, _ = model(frozen_stages=0)
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    eng = m.bind_engine('cpu')
    m.train()
    m._sync_frozen(eng)
    bn, keys = stage_signature(eng, 0)
    assert eng.frozen == (frozenset(bn), frozenset(keys))
    named = dict(m.named_parameters())
    assert all(named[k].grad is None for k in keys)
    assert all(p.grad is not None and p.grad.data_ptr() == eng.params.view(k, of=eng.params.grad).data_ptr()
               for k, p in named.items() if k not in keys)
    assert m._sentinel[0] == 'backbone.model1.conv1.conv1.weight'
    # thaw everything, freeze one BatchNorm by hand: the torch-native spelling
    for p in m.parameters():
        p.requires_grad = True
    m.backbone.frozen_stages = -1
    m.train()
    m.neck.lateral_convs[1].bn.eval()
    m._sync_frozen(eng)
    assert eng.frozen == (frozenset(['neck.lateral_convs.1.bn']), frozenset())
    assert all(p.grad is not None for p in m.parameters())
    m.train()
    m._sync_frozen(eng)
    assert eng.frozen == (frozenset(), frozenset()) and eng._frozen_key == ()


# ----------------------------------------------------------------------------------------------------------- plan key
def test_plan_key_per_signature_and_the_default_plan_comes_back(monkeypatch):
    eng = engine()
    built = []
    monkeypatch.setattr(E, 'Plan', lambda eng_, n, h, w, g: built.append(eng_.frozen) or object())
    p_def = eng.get_plan(*SHAPE[:3], 1)
    assert next(reversed(eng.plans)) == (2, 64, 64, 64, 'fp32')
    bn, keys = stage_signature(eng, 2)
    eng.set_frozen(bn, keys)
    p_fr = eng.get_plan(*SHAPE[:3], 1)
    assert next(reversed(eng.plans)) == (2, 64, 64, 64, 'fp32', ('frozen', tuple(sorted(bn)), tuple(sorted(keys))))
    eng.set_frozen(bn, ())
    p_bn = eng.get_plan(*SHAPE[:3], 1)
    eng.set_deterministic('fast')
    p_fast = eng.get_plan(*SHAPE[:3], 1)
    assert next(reversed(eng.plans))[4:6] == ('fp32', 'det-fast')
    eng.set_deterministic(False)
    eng.set_frozen()
    assert eng.get_plan(*SHAPE[:3], 1) is p_def and len(built) == 4
    assert len({id(p_def), id(p_fr), id(p_bn), id(p_fast)}) == 4
    eng.set_frozen(bn, keys)
    assert eng.get_plan(*SHAPE[:3], 1) is p_fr and len(built) == 4


def test_freeze_thaw_freeze_of_one_signature_returns_the_frozen_plan(monkeypatch):
    """A -> nothing -> A, at the engine and through the model's flags: the second A is the frozen plan again, not the default."""
    eng = engine()
    bn, keys = stage_signature(eng, 0)
    eng.set_frozen(bn, keys)
    p_a = eng.get_plan(*SHAPE[:3], 1)
    eng.set_frozen((), ())
    p_def = eng.get_plan(*SHAPE[:3], 1)
    eng.set_frozen(bn, keys)
    assert eng.frozen == (frozenset(bn), frozenset(keys)) and eng._frozen_key != ()
    assert eng.get_plan(*SHAPE[:3], 1) is p_a and p_a is not p_def
    assert p_a.frozen_bn == frozenset(bn) and p_def.frozen_bn == frozenset()
    # the same through YuNet._sync_frozen
    m, _ = model()
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    eng = m.bind_engine('cpu')
    m.train()
    plans = []
    for freeze in (True, False, True):
        for mod in bns(m).values():
            mod.train(not freeze)
        m.backbone.model0.conv1.weight.requires_grad = not freeze
        m._sync_frozen(eng)
        plans.append(eng.get_plan(*SHAPE[:3], 1))
        assert bool(eng.frozen[0]) == freeze and bool(eng.frozen[1]) == freeze
        assert (m.backbone.model0.conv1.weight.grad is None) == freeze
        assert [n for n, _ in m.frozen_parameters()] == (['backbone.model0.conv1.weight'] if freeze else [])
    assert plans[0] is plans[2] and plans[0] is not plans[1]
    assert plans[0].frozen_bn == frozenset(eng.layout.bn_names) and plans[1].frozen_bn == frozenset()
    assert plans[0].fwd_a[1].opcode == L.OP_BN_BATCH and plans[1].fwd_a[1].opcode == L.OP_STEM_FWD


def test_unknown_names_are_refused_when_the_plan_is_built():
    eng = engine()
    eng.set_frozen(('no.such.bn',), ())
    with pytest.raises(KeyError, match='no.such.bn'):
        E.Plan(eng, *SHAPE)
    eng.set_frozen((), ('backbone.model0.conv1.wait',))
    with pytest.raises(KeyError, match='conv1.wait'):
        E.Plan(eng, *SHAPE)


# ------------------------------------------------------------------------------------------------------------ op lists
@pytest.mark.parametrize('det', [False, True, 'fast'])
def test_all_bn_frozen_plan(det):
    """Every BatchNorm frozen, every parameter trainable: one mode-2 launch over all layers right after the memset, no
    producer accumulates, no mode-0 launch, no fold op at all in the forward, the readers' backward sums are the zero block
    while the consumers' are the layers' own -- and the backward has every op of the default plan."""
    eng = engine(det=det)
    dflt = E.Plan(eng, *SHAPE)
    names = tuple(eng.layout.bn_names)
    eng.set_frozen(names, ())
    pl = E.Plan(eng, *SHAPE)
    assert opcodes(pl.fwd_a[:2]) == [L.OP_MEMSET, L.OP_BN_BATCH]
    fill = pl.fwd_a[1]
    assert (fill.i[0], fill.i[1]) == (len(names), 2) and fill.p[0] == pl.bn_table_frozen.data_ptr()
    assert fill.p[1] == pl.stats.data_ptr() and fill.p[2] == eng.params.running_mean.data_ptr()
    assert pl.bn_table_frozen.tolist() == pl.bn_table_f.tolist()
    assert all(row[6] == (1 if det else E.BN_SLOTS) for row in pl.bn_table_frozen.tolist())        # det: row 0 alone
    assert [op for op in pl.fwd_a if op.opcode == L.OP_BN_FOLD] == []
    assert len([op for op in dflt.fwd_a if op.opcode == L.OP_BN_FOLD]) == (len(names) if det else 0)
    assert opcodes([op for op in pl.fwd_a[2:] if op.opcode != L.OP_BN_FOLD]) == \
        opcodes([op for op in dflt.fwd_a[1:] if op.opcode != L.OP_BN_FOLD])
    for op in pl.fwd_a:
        if op.opcode == L.OP_DP_FWD:
            assert op.dp.out_has_bn == 0
        if op.opcode == L.OP_STEM_FWD:
            assert op.p[4] == pl.stem_scratch.data_ptr() and op.i[4] == 0
    assert opcodes(pl.fwd_b) == [L.OP_LOSS, L.OP_LOSS_FINALIZE] and pl.bn_table_run is None and pl.nbt_step is None
    assert opcodes(dflt.fwd_b) == [L.OP_LOSS, L.OP_LOSS_FINALIZE, L.OP_BN_BATCH] and dflt.nbt_step == 1
    # backward: same ops (gamma / beta train, so deterministic plans keep the folds that feed the mode-1 launch)
    assert opcodes(pl.bwd) == opcodes(dflt.bwd) and pl.reduce_jobs and len(pl.reduce_jobs) == len(dflt.reduce_jobs)
    assert pl.bn_table_b.tolist() == dflt.bn_table_b.tolist() and memsets(pl, pl.bwd) == []
    zero = pl.zero_bstats.data_ptr()
    assert pl.zero_bstats.numel() == (1 if det else E.BN_SLOTS) * 2 * max(eng.params.bn_channels)
    own = {pl.bn[n]['bstats'].data_ptr(): n for n in names}
    readers = 0
    for op in pl.bwd:
        if op.opcode == L.OP_DP_BWD:
            if op.dp.out_has_bn:
                assert op.dp.out_bn.bstats == zero and op.dp.out_bn.stats in {pl.bn[n]['stats'].data_ptr() for n in names}
                readers += 1
            if op.dp.in_bn.stats:
                assert op.dp.in_bn.bstats in own
        elif op.opcode == L.OP_STEM_BWD:
            assert op.bn[0].bstats == zero
            readers += 1
        elif op.opcode in (L.OP_POOL_BWD, L.OP_UPADD_BWD):
            assert op.bn[0].bstats in own
    assert readers == len(names)
    assert pl.zero_bstats.abs().sum() == 0
    # eval keeps its positions: op 0 fills every layer, the stem sits where set_img expects it
    assert len(pl.fwd_eval) == len([op for op in pl.fwd_a if op.opcode not in (L.OP_ASSIGN, L.OP_LOSS_NORM, L.OP_BN_FOLD)])
    assert pl.fwd_eval[0].i[1] == 2 and pl.fwd_eval[0].i[0] == len(names)
    for which, idx in pl.img_ptr_ops:
        if which == 'fwd_a':
            assert pl.fwd_a[idx].opcode == L.OP_STEM_FWD and pl.fwd_eval[idx].opcode == L.OP_STEM_FWD


@pytest.mark.parametrize('det', [False, True, 'fast'])
@pytest.mark.parametrize('k', [0, 2, 5])
def test_frozen_stages_plan(k, det):
    """frozen_stages = k: the mode-2 / mode-0 / mode-1 tables split the layers, no fold op of a frozen layer in either
    direction, no backward op, reduce job or memset-free range of the frozen prefix."""
    eng = engine(det=det)
    dflt = E.Plan(eng, *SHAPE)
    bn, keys = stage_signature(eng, k)
    eng.set_frozen(bn, keys)
    pl = E.Plan(eng, *SHAPE)
    lay = eng.layout
    rows = {n: r for n, r in zip(lay.bn_names, pl.bn_table_f.tolist())}
    assert pl.bn_table_frozen.tolist() == [rows[n] for n in lay.bn_names if n in bn]
    assert pl.bn_table_run.tolist() == [rows[n] for n in lay.bn_names if n not in bn]
    half = pl.stats.numel() // 2
    assert pl.bn_table_b.tolist() == [[rows[n][0] + half] + rows[n][1:] for n in lay.bn_names if n not in bn]
    assert pl.fwd_a[1].opcode == L.OP_BN_BATCH and (pl.fwd_a[1].i[0], pl.fwd_a[1].i[1]) == (len(bn), 2)
    assert pl.fwd_b[2].opcode == L.OP_BN_BATCH and (pl.fwd_b[2].i[0], pl.fwd_b[2].i[1]) == (len(lay.bn_names) - len(bn), 0)
    assert pl.nbt_step.tolist() == [int(n not in bn) for n in lay.bn_names]
    blocks = {}
    for n in lay.bn_names:
        blocks[pl.bn[n]['stats'].data_ptr()] = blocks[pl.bn[n]['bstats'].data_ptr()] = n
    for lst in (pl.fwd_a, pl.bwd):
        folds = [blocks[op.p[0]] for op in lst if op.opcode == L.OP_BN_FOLD]
        assert sorted(folds) == (sorted(n for n in lay.bn_names if n not in bn) if det else [])      # one each, none frozen
    # the frozen prefix has no backward: the first 2k + 2 units of the chain (stem, model0.conv2, two per later stage)
    n_prefix = 2 * k + 2
    kept = [op for op in pl.bwd if op.opcode in (L.OP_DP_BWD, L.OP_STEM_BWD)]
    all_ = [op for op in dflt.bwd if op.opcode in (L.OP_DP_BWD, L.OP_STEM_BWD)]
    assert len(kept) == len(all_) - n_prefix and L.OP_STEM_BWD not in opcodes(pl.bwd)
    frozen_w = {lay.unit_ptrs(eng.params.data, u)[0] for u in lay.units if stage_of(u) is not None and stage_of(u) <= k}
    assert not any(op.dp.w_pw in frozen_w for op in kept)
    assert len(pl.reduce_jobs) == len(dflt.reduce_jobs) - n_prefix
    end = max(lay.entries[key][0] + lay.entries[key][1][0] for key in keys)       # (the last entry is a BN vector)
    g0 = eng.params.grad.data_ptr()
    assert all(j[1] - g0 >= 4 * end for j in pl.reduce_jobs)
    assert pl._frozen_ranges() == [(0, end)]
    assert memsets(pl, pl.bwd) == [(0, end)] and opcodes(pl.bwd[-3:]) == [L.OP_REDUCE_BATCH, L.OP_BN_BATCH, L.OP_MEMSET]
    assert [w for w, _ in pl.img_ptr_ops] == ['fwd_a']
    # pools of the prefix are gone too; the boundary unit still produces dx (eliding it is out of scope)
    pools = lambda p: len([op for op in p.bwd if op.opcode == L.OP_POOL_BWD])
    assert pools(pl) <= pools(dflt)
    # a unit with fused pooling whose backward is gone keeps its z: nothing was elided that a kept op reads
    for zt, fop in pl.elided_z:
        assert any(op.opcode == L.OP_DP_BWD and op.dp.pool_idx == fop.dp.pool_idx for op in pl.bwd)
    # the two-segment copy: memsets split at the bucket boundary, every frozen element covered once
    if pl.split_off is not None:
        a, b = memsets(pl, pl.bwd_a), memsets(pl, pl.bwd_b)
        assert all(off >= pl.split_off for off, _ in a) and all(off + n <= pl.split_off for off, n in b)
        assert sum(n for _, n in a + b) == end
        assert len(pl.c_bwd_a_k) + len(pl.c_tail_a) == len(pl.bwd_a)


def test_head_only_plan_has_no_backbone_or_neck_backward():
    eng = engine()
    lay = eng.layout
    keys = tuple(k for k in lay.entries if not k.startswith('bbox_head.'))
    bn = tuple(n for n in lay.bn_names if not n.startswith('bbox_head.'))
    eng.set_frozen(bn, keys)
    pl = E.Plan(eng, *SHAPE)
    ptr_of = {lay.unit_ptrs(eng.params.data, u)[0]: u for u in lay.units if u != 'stem'}
    units = [ptr_of[op.dp.w_pw] for op in pl.bwd if op.opcode == L.OP_DP_BWD]
    assert units and all(u.startswith(('bbox_head.', 'head.')) for u in units)
    assert set(opcodes(pl.bwd)) == {L.OP_DP_BWD, L.OP_REDUCE_BATCH, L.OP_BN_BATCH, L.OP_MEMSET}
    assert len(pl.reduce_jobs) == len(units)


def test_frozen_unit_in_the_middle_keeps_its_backward_without_a_job():
    """neck.lateral_convs.1: its four conv tensors frozen, its BatchNorm training and gamma / beta trainable -- dx must flow
    to the backbone, so the op stays; its partials go nowhere; the four tensors are one memset range."""
    eng = engine()
    lay = eng.layout
    u = 'neck.lateral_convs.1'
    keys = tuple(f'{u}.{c}.{t}' for c in ('conv1', 'conv2') for t in ('weight', 'bias'))
    dflt = E.Plan(eng, *SHAPE)
    eng.set_frozen((), keys)
    pl = E.Plan(eng, *SHAPE)
    assert opcodes(pl.fwd_a) == opcodes(dflt.fwd_a) and opcodes(pl.fwd_b) == opcodes(dflt.fwd_b)
    assert opcodes(pl.bwd) == opcodes(dflt.bwd) + [L.OP_MEMSET]
    g = eng.params.grad.data_ptr() + 4 * lay.units[u]['off']
    assert g in [j[1] for j in dflt.reduce_jobs] and g not in [j[1] for j in pl.reduce_jobs]
    assert len(pl.reduce_jobs) == len(dflt.reduce_jobs) - 1
    assert memsets(pl, pl.bwd) == [(lay.units[u]['off'], lay.unit_width(u))]
    assert pl.bn_table_b.tolist() == dflt.bn_table_b.tolist() and pl.nbt_step == 1
    # one tensor of a unit frozen: the job stays, the memset follows it
    eng.set_frozen((), (f'{u}.conv2.weight', f'{u}.bn.weight'))
    pl = E.Plan(eng, *SHAPE)
    assert len(pl.reduce_jobs) == len(dflt.reduce_jobs) and pl.bn_table_b.tolist() == dflt.bn_table_b.tolist()
    assert memsets(pl, pl.bwd) == [(lay.entries[f'{u}.conv2.weight'][0], 64 * 9), (lay.entries[f'{u}.bn.weight'][0], 64)]
    assert opcodes(pl.bwd[-4:]) == [L.OP_REDUCE_BATCH, L.OP_BN_BATCH, L.OP_MEMSET, L.OP_MEMSET]


def test_default_plan_is_untouched_by_an_empty_signature():
    eng = engine()
    a = E.Plan(eng, *SHAPE)
    eng.set_frozen((), ())
    b = E.Plan(eng, *SHAPE)
    assert a.bn_table_run is a.bn_table_f and a.zero_bstats is None and not hasattr(a, 'op_fill_frozen')
    for la, lb in ((a.fwd_a, b.fwd_a), (a.fwd_b, b.fwd_b), (a.bwd, b.bwd)):
        assert opcodes(la) == opcodes(lb)


# ---------------------------------------------------------------------------------------------------------- optimizers
class FakeEngine:
    def __init__(self, n):
        self.device = torch.device('cpu')
        self.params = type('P', (), {})()
        self.params.data = torch.zeros(n)


def bound_params(eng, sizes):
    out, off = [], 0
    for s in sizes:
        p = nn.Parameter(torch.zeros(1))
        p.data = eng.params.data[off:off + s]
        out.append(p)
        off += s
    return out


@pytest.mark.parametrize('cls', [FusedSGD, FusedAdam])
def test_optimizers_map_frozen_and_uncovered_elements_to_255(cls):
    assert L.OPT_FROZEN == 255 and L.OPT_MAX_GROUPS == 255
    eng = FakeEngine(40)
    p = bound_params(eng, [7, 5, 9, 11, 8])
    p[1].requires_grad = False
    p[3].requires_grad = False
    m = type('M', (), dict(parameters=lambda self: iter(p), engine=eng))()
    opt = cls(m, lr=0.1, groups=[dict(params=[p[0], p[1]]), dict(params=[p[2], p[3]], lr=0.2)])    # p[4]: in no group
    host = opt._host_map(eng)
    want = [0] * 7 + [255] * 5 + [1] * 9 + [255] * 11 + [255] * 8
    assert host.tolist() == want and host.dtype == torch.uint8
    # one group over everything, nothing frozen: the plain path as before; one frozen parameter: the grouped launch
    opt = cls(m, lr=0.1)
    for q in p:
        q.requires_grad = True
    assert opt._host_map(eng).tolist() == [0] * 40
    if cls is FusedSGD:
        assert not opt._grouped(eng)
        p[2].requires_grad = False
        assert opt._grouped(eng) and opt._host_map(eng).tolist() == [0] * 12 + [255] * 9 + [0] * 19
        p[2].requires_grad = True
        opt = cls(m, lr=0.1, groups=[dict(params=p[:4])])
        assert opt._grouped(eng) and opt._host_map(eng).tolist() == [0] * 32 + [255] * 8


def test_optimizer_takes_the_frozen_parameters_from_a_bound_yunet(monkeypatch):
    m, _ = model(frozen_stages=0)
    assert m.frozen_parameters() is None                      # not bound: an optimizer reads requires_grad itself
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    eng = m.bind_engine('cpu')
    m.train()
    m._sync_frozen(eng)
    opt = FusedSGD(m, lr=0.1)
    frozen = [p for p in m.parameters() if not p.requires_grad]
    assert opt._frozen_ids() == frozenset(id(p) for p in frozen) and opt._grouped(eng)
    host = opt._host_map(eng)
    assert int((host == L.OPT_FROZEN).sum()) == sum(p.numel() for p in frozen) and set(host.tolist()) == {0, L.OPT_FROZEN}
    end = sum(p.numel() for p in frozen)                      # stage 0 is the head of the flat buffer
    assert bool((host[:end] == L.OPT_FROZEN).all()) and bool(host[end:].eq(0).all())


def test_build_optimizer_accepts_a_model_with_frozen_stages():
    m, cfg = model(frozen_stages=2)
    opt = build_optimizer(m, dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=5e-4))
    assert isinstance(opt, FusedSGD)
    opt = build_optimizer(m, dict(type='AdamW', lr=1e-3, weight_decay=0.01, paramwise_cfg=dict(norm_decay_mult=0.0)))
    assert isinstance(opt, FusedAdam) and len(opt.param_groups) == 2
