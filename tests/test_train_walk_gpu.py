"""-m gpu: one training step (forward_train + backward through the module API) walked op by op against fp64, each op from
its own stored inputs, at the bars every kernel meets alone (tests/train_walk.py states them and where each comes from).

record_of() turns the live Plan into train_walk's Record.  It only reads: Plan.tensors, Plan.bn, fwd_op_of / pooled_into,
the op records of fwd_a / fwd_b and of the backward lists that ran (matched by pointer, as test_eval_forward_gpu's
check_layers does), the device tables of the reduction and BatchNorm ops, elided_z, flat, dflat, the dy_scale vectors and
the flat parameter and gradient views.  What an op record CLAIMS (a count, a table row, an accumulate flag) is never the
reference: the reference is the graph and the stored values, so a wrong claim shows as a wrong value.

Cases (train_walk.CASES): the trained fixtures tests/golden/yunet_{n,s}_synth_trained.pth on synthetic.make_batch batches
whose oracle assignment sits on no tie (finetune_ref.near_tie == [], asserted; the fp32 cases assert the assignment exact)
and whose tensors stay under the ambiguous-element cap, at train_walk.GEOMETRY -- the smallest batch-4 shape whose plans
launch exactly the benchmark's kernel instances (asserted on the CPU by tests/test_train_walk.py; no instance is left
uncovered, so none is delegated to a kernel-level test).  Per case -s prints one line per node with its worst error /
bound and, for a tensor's gradient, the count of ambiguous elements; the number of kernel ops the walked nodes stand for
equals the number in the plan's lists (the loss step's four ops, memsets, fork / join and folds counted apart).

On the first run every node of every case met its kernel's bar, bf16 included, except the one check profiles/train_walk.json
lists (see train_walk.py); the walk found no wiring defect in engine.py, dp_route.h or the op tables."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import finetune_ref as FR
import train_walk as TW
import yunet_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def cpu(t):
    return None if t is None else t.detach().cpu().clone()


# ------------------------------------------------------------------------------------------------ Plan -> Record
def ran_backward(eng, plan):
    """the backward op records a one-GPU backward() executed: the two segments with their own tails, or the single list"""
    if plan.split_off is not None and eng.overlap_reduce:
        return plan.bwd_a + plan.bwd_b
    return plan.bwd


def record_of(eng, plan, img, before, after):
    """before / after: the model's state_dict (CPU) around the step"""
    import yunet_amd._lib as L
    lay, fp = eng.layout, eng.params
    rec = TW.Record(eng.precision, img.cpu())
    bwd = ran_backward(eng, plan)
    tables = {t.data_ptr(): t for t in list(plan.keep) + [plan.reduce_table] + [getattr(plan, a, None) for a in (
        'bn_table_f', 'bn_table_run', 'bn_table_b', 'bn_table_ba', 'bn_table_bb', 'bn_table_frozen')]
        if torch.is_tensor(t)}
    pdata, pgrad = fp.data.detach().cpu(), fp.grad.detach().cpu()

    def pslice(buf, off, shape):
        return buf[off:off + int(torch.tensor(shape).prod())].view(*shape).clone()

    # ---- BatchNorm layers
    layer_of_goff = {}
    for name in lay.bn_names:
        b = plan.bn[name]
        g_off, b_off = lay.entries[name + '.weight'][0], lay.entries[name + '.bias'][0]
        layer_of_goff[g_off] = name
        c = b['c']
        lr = rec.layer(name, c=c, stats=cpu(b['stats']), bstats=cpu(b['bstats']), slots=plan.bn_slots,
                       gamma=pslice(pdata, g_off, (c,)), beta=pslice(pdata, b_off, (c,)), frozen=name in plan.frozen_bn,
                       rm0=before[name + '.running_mean'], rv0=before[name + '.running_var'],
                       nbt0=int(before[name + '.num_batches_tracked']), rm1=after[name + '.running_mean'],
                       rv1=after[name + '.running_var'], nbt1=int(after[name + '.num_batches_tracked']),
                       dgamma=pslice(pgrad, g_off, (c,)), dbeta=pslice(pgrad, b_off, (c,)))
        lr.counts = set()
    layer_of_stats = {plan.bn[n]['stats'].data_ptr(): n for n in lay.bn_names}
    layer_of_bstats = {plan.bn[n]['bstats'].data_ptr(): n for n in lay.bn_names}

    def saw(bn):
        """a count an op record carries, filed under the layer whose block the record names"""
        name = layer_of_stats.get(bn.stats)
        if name is not None:
            rec.bn[name].counts.add(int(bn.count))

    # ---- tensors, named by the op that wrote them
    name_of, by_ptr, by_grad = {}, {}, {}

    def declare(t, name):
        if id(t) in name_of:
            return name_of[id(t)]
        name_of[id(t)] = name
        rec.tensor(name, cpu(t.buf), (t.n, t.h, t.w, t.c), bn=t.bn, grad=cpu(t.grad))
        if t.buf is not None:
            by_ptr[t.buf.data_ptr()] = t
        if t.grad is not None:
            by_grad[t.grad.data_ptr()] = name
        return name
    objs = {}
    for unit, (x, z) in plan.tensors.items():
        declare(z, unit)
        if z.pooled_into is not None:
            declare(z.pooled_into[0], f'pool({unit})')
        objs[id(x)] = x
    declare(plan.tensors['backbone.model0.conv2'][0], 'stem')
    for x in objs.values():             # written by a pool or a merge: named below, found by pointer here
        if id(x) not in name_of and x.buf is not None:
            by_ptr[x.buf.data_ptr()] = x
    for op in plan.fwd_a:               # (a tap's pool backward names the merge output's gradient: declare both kinds first)
        if op.opcode == L.OP_POOL_FWD:
            declare(by_ptr[op.p[1]], f'pool({name_of[id(by_ptr[op.p[0]])]})')
        elif op.opcode == L.OP_UPADD_FWD:
            declare(by_ptr[op.p[2]], f'upadd({name_of[id(by_ptr[op.p[0]])]})')
    unit_of_w = {lay.unit_ptrs(fp.data, u)[0]: u for u in lay.units if u != 'stem'}
    part_of = {t.data_ptr(): t for t in plan.keep if torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2}
    gbase = fp.grad.data_ptr()

    # ---- the backward records, by what they point at
    b_dp = {op.dp.w_pw: op for op in bwd if op.opcode == L.OP_DP_BWD}
    b_stem = [op for op in bwd if op.opcode == L.OP_STEM_BWD]
    b_pool = {op.p[0]: op for op in bwd if op.opcode == L.OP_POOL_BWD}
    b_upadd = {(op.p[0], op.p[1]): op for op in bwd if op.opcode == L.OP_UPADD_BWD}
    jobs = {}                           # partials pointer -> (destination offset in the flat gradient, rows, accumulate)
    n_reduce = 0
    for op in bwd:
        if op.opcode == L.OP_REDUCE_BATCH:
            tab = tables[op.p[0]].cpu()
            for r in range(op.i[0]):
                jobs[int(tab[r, 0])] = ((int(tab[r, 1]) - gbase) // 4, int(tab[r, 2]) & 0xffffffff, int(tab[r, 3]) & 0xffffffff)
            n_reduce += 1

    def grads_of(unit, part_ptr, widths):
        """(the unit's gradients where the LAYOUT puts them, its partials) -- or (None, None) without a reduction job"""
        if part_ptr not in jobs:
            return None, None
        off, out = lay.units[unit]['off'], []
        for wd in widths:
            out.append(pgrad[off:off + wd].clone())
            off += wd
        return out, cpu(part_of[part_ptr])

    for op in list(plan.fwd_a) + list(plan.fwd_b):
        code = op.opcode
        if code == L.OP_STEM_FWD:
            off = lay.units['stem']['off']
            w = (pdata[off:off + 432].view(16, 27).clone(), pdata[off + 432:off + 448].clone())
            nd = rec.node('stem', 'stem', z='stem', w=w, out_bn='backbone.model0.bn1', bwd=bool(b_stem), g=None, partials=None,
                          rows=0)
            if b_stem:
                saw(b_stem[0].bn[0])
                nd.g, nd.partials = grads_of('stem', b_stem[0].p[3], [432, 16])
                nd.rows = int(b_stem[0].i[4])
        elif code == L.OP_DP_FWD:
            d = op.dp
            unit = unit_of_w[d.w_pw]
            u = lay.units[unit]
            ci, co = u['cin'], u['cout']
            off = u['off']
            w = [pdata[off:off + co * ci].view(co, ci).clone(), pdata[off + co * ci:off + co * ci + co].clone(),
                 pdata[off + co * ci + co:off + co * ci + 10 * co].view(co, 9).clone(),
                 pdata[off + co * ci + 10 * co:off + co * ci + 11 * co].clone()]
            xt = by_ptr[d.x]
            nd = rec.node('unit', unit, x=name_of[id(xt)], z=unit if u['bn'] else None, w=w, out_bn=unit + '.bn' if u['bn'] else None,
                          pool_out=None, pool_idx=None, flat_rows=None, dy=None, dy_scale=None, accumulate=0, zmode='stored',
                          bwd=False, g=None, partials=None, rows=0)
            if xt.bn is not None:
                saw(d.in_bn)
            if u['bn']:
                saw(d.out_bn)
                zt = plan.tensors[unit][1]
                if zt.pooled_into is not None:
                    nd.pool_out, nd.pool_idx = name_of[id(zt.pooled_into[0])], cpu(zt.pooled_into[1])
                    assert d.pool_out == zt.pooled_into[0].buf.data_ptr() and d.pool_idx == zt.pooled_into[1].data_ptr()
                if not d.z:
                    nd.zmode = 'elided'
                    assert zt.buf is None and any(t is zt for t, _ in plan.elided_z)
            else:
                base = (d.z - plan.flat.data_ptr()) // 64
                assert d.z_img_stride == plan.P * 16 and (d.z - plan.flat.data_ptr()) % 64 == 0
                nd.flat_rows = cpu(plan.flat[:, base:base + xt.h * xt.w]).reshape(xt.n, xt.h, xt.w, 16)
            bop = b_dp.get(d.w_pw)
            if bop is not None:
                bd = bop.dp
                nd.bwd, nd.accumulate, nd.rows = True, int(bd.accumulate_dx), int(bd.wgrad_blocks)
                if nd.zmode == 'stored' and not L.load().yunet_dp_bwd_reads_z(C.byref(bd)):
                    nd.zmode = 'recomputed'
                if xt.bn is not None:
                    saw(bd.in_bn)
                if bd.dy_scale:
                    base = (bd.dy - plan.dflat.data_ptr()) // 64
                    nd.dy = ('dflat', cpu(plan.dflat[:, base:base + xt.h * xt.w]).reshape(xt.n, xt.h, xt.w, 16))
                    vec = [v for v in (plan.dy_scale, plan.dy_scale_cls, plan.dy_scale_reg) if v.data_ptr() == bd.dy_scale]
                    nd.dy_scale = cpu(vec[0])
                else:
                    nd.dy = ('grad', by_grad[bd.dy])
                nd.g, nd.partials = grads_of(unit, bd.wgrad_partials, [co * ci, co, co * 9, co])
        elif code == L.OP_POOL_FWD:
            xt, ot = by_ptr[op.p[0]], by_ptr[op.p[1]]
            saw(op.bn[0])
            xn = name_of[id(xt)]
            bop = b_pool.get(op.p[0])
            nd = rec.node('pool', f'pool {xn}', x=xn, out=name_of[id(ot)], extra=None, bwd=bop is not None)
            if bop is not None:
                saw(bop.bn[0])
                nd.extra = by_grad[bop.p[3]] if bop.p[3] else None
        elif code == L.OP_UPADD_FWD:
            at, bt, ot = by_ptr[op.p[0]], by_ptr[op.p[1]], by_ptr[op.p[2]]
            saw(op.bn[0]), saw(op.bn[1])
            bop = b_upadd.get((op.p[0], op.p[1]))
            rec.node('upadd', f'upadd -> {name_of[id(ot)]}', a=name_of[id(at)], b=name_of[id(bt)], out=name_of[id(ot)],
                     skip_a=bop is not None and not bop.p[3], bwd=bop is not None)
            if bop is not None:
                saw(bop.bn[0]), saw(bop.bn[1])
        elif code == L.OP_BN_FOLD:
            rec.node('fold', f'fold {layer_of_stats[op.p[0]]}', layer=layer_of_stats[op.p[0]], backward=False)
        elif code == L.OP_BN_BATCH:
            tab = tables[op.p[0]].cpu()
            names = [layer_of_goff[int(tab[r, 4])] for r in range(op.i[0])]
            for r, nm in enumerate(names):
                rec.bn[nm].counts.add(int(tab[r, 2]))
            rec.node('bn_run' if op.i[1] == 0 else 'bn_fill', 'bn_run' if op.i[1] == 0 else 'bn_fill', layers=names)
            assert op.i[1] in (0, 2)
    if not any(nd.kind == 'bn_run' for nd in rec.nodes):
        rec.node('bn_run', 'bn_run (no op: every layer frozen)', layers=[])
        rec.nodes[-1].ops = 0
    layers_b = []
    for op in bwd:
        if op.opcode == L.OP_BN_FOLD:
            rec.node('fold', f'fold backward {layer_of_bstats[op.p[0]]}', layer=layer_of_bstats[op.p[0]], backward=True)
        elif op.opcode == L.OP_BN_BATCH:
            assert op.i[1] == 1
            tab = tables[op.p[0]].cpu()
            layers_b.append([layer_of_goff[int(tab[r, 4])] for r in range(op.i[0])])
    for k, names in enumerate(layers_b):
        rec.node('bn_grad', f'bn_grad {k}', layers=names)
    for k in range(n_reduce):
        rec.node('reduce_batch', f'reduce_batch {k}')
    for key in plan.frozen_params:
        off, shape = lay.entries[key]
        rec.frozen[key] = pslice(pgrad, off, shape)
    rec.flat, rec.dflat = cpu(plan.flat), cpu(plan.dflat)
    return rec


def kernel_ops(eng, plan):
    """(ops the walk must stand for, loss-step ops, memsets + fork / join, folds) of the lists a step runs"""
    import yunet_amd._lib as L
    ops = list(plan.fwd_a) + list(plan.fwd_b) + list(ran_backward(eng, plan))
    loss = sum(op.opcode in (L.OP_ASSIGN, L.OP_LOSS_NORM, L.OP_LOSS, L.OP_LOSS_FINALIZE) for op in ops)
    plumbing = sum(op.opcode in (L.OP_MEMSET, L.OP_FORK, L.OP_JOIN) for op in ops)
    folds = sum(op.opcode == L.OP_BN_FOLD for op in ops)
    return len(ops) - loss - plumbing - folds, loss, plumbing, folds


# ------------------------------------------------------------------------------------------------ one case
def trained(kind):
    return torch.load(os.path.join(GOLDEN, f'yunet_{kind}_synth_trained.pth'), map_location='cpu', weights_only=False)['state_dict']


_ORACLE = {}


def oracle_assignment(kind, seed, flag_key, flag, sd, batch):
    key = (kind, seed, flag_key)
    if key not in _ORACLE:
        _, _, aux, _ = FR.step_fp32(batch, sd, O.yunet_arch(kind), flag)
        _ORACLE[key] = (FR.near_tie(aux, batch), aux['gt_inds'].int())
    return _ORACLE[key]


def run_case(name, raise_on_fail=True):
    """-> (worst per node, the flat gradient's bytes on the CPU, the record)"""
    import yunet_amd
    import yunet_amd.synthetic as S
    c = TW.CASES[name]
    assert bool(os.environ.get('YUNET_KEEP_POOL_Z')) == c['keep_pool_z'], 'the switch is read when the plan is built'
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f"yunet_{c['kind']}.py"))
    if c['finetune']:
        cfg.model.backbone.update(dict(norm_eval=True, frozen_stages=2))
    m = yunet_amd.build_detector(cfg.model)
    sd = trained(c['kind'])
    m.load_state_dict(sd, strict=True)
    m.to(DEV).train()
    m.set_precision(c['precision'])
    m.set_deterministic(c['deterministic'])
    n, h, w = TW.GEOMETRY
    b = S.make_batch(n, h, w, c['seed'])
    eng = m._ensure_engine(torch.device(DEV, torch.cuda.current_device()))
    before = {k: cpu(v) for k, v in m.state_dict().items()}
    losses = m.forward_train(**S.to_device(b, DEV))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    plan = eng.plan
    after = {k: cpu(v) for k, v in m.state_dict().items()}
    assert (plan.n, plan.h, plan.w) == TW.GEOMETRY
    bn_training = {nm: mod.training for nm, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)}
    ties, gt_inds = oracle_assignment(c['kind'], c['seed'], c['finetune'], lambda nm: bn_training.get(nm, True), sd, b)
    assert ties == [], 'pick another seed: the oracle assignment sits on a tie'
    if c['precision'] == 'fp32':
        assert torch.equal(plan.gt_inds.cpu(), gt_inds), 'assignment'
    if c['finetune']:
        sig = TW.finetune_signature(eng.layout)
        assert eng.frozen == (frozenset(sig[0]), frozenset(sig[1])), 'the CPU geometry test builds another freeze signature'
        assert plan.frozen_bn and plan.frozen_params
    assert len(plan.elided_z) == (1 if name in ('n_fp32', 's_fp32', 'n_bf16', 'n_det_fast') else 0)
    rec = record_of(eng, plan, b['img'], before, after)
    worst = TW.walk(rec, tag=name, raise_on_fail=raise_on_fail)
    with open(os.path.join(ROOT, 'profiles', 'train_walk.json')) as f:
        listed = {(r['node'], r['check']) for r in json.load(f)['measurements']}
    extra = [r for r in rec.measured if (r['node'], r['check']) not in listed]
    assert not extra, ('a check outside profiles/train_walk.json fell back to a measured bound', extra)
    want, loss, plumbing, folds = kernel_ops(eng, plan)
    walked = sum(k for _, k in rec.walked)
    print(f'[train walk {name}] kernel ops walked {walked} of {want}; loss step {loss}, memset / fork / join {plumbing}, folds {folds}')
    assert walked == want, (walked, want, rec.walked)
    assert sum(nd.kind == 'fold' for nd in rec.nodes) == folds
    if c['finetune']:      # no op exists for the frozen prefix, and its readers see zeros
        assert not any(nd.bwd for nd in rec.nodes if nd.kind in ('stem', 'unit') and
                       nd.name in ('stem', 'backbone.model0.conv2', 'backbone.model1.conv1', 'backbone.model1.conv2',
                                   'backbone.model2.conv1', 'backbone.model2.conv2'))
        assert not bool(plan.zero_bstats.any())
    return worst, eng.params.grad.detach().cpu().contiguous().view(torch.uint8).clone(), rec


_GRAD = {}


@pytest.mark.parametrize('name', [k for k in TW.CASES if not TW.CASES[k]['keep_pool_z']])
def test_train_step_walk(name):
    worst, grad, rec = run_case(name)
    _GRAD[name] = grad
    assert max(worst.values()) <= 1.0
    if name == 'n_fp32':
        tampered(rec)


def tampered(rec):
    """The live record at this geometry with a wiring error applied after the fact (one partial row of 80 left out of a
    reduction, two layers' d(gamma) exchanged, a tap without the merge's share): the walk names the node and passes again
    once the record is restored.  (tests/test_train_walk.py does this for ten defects on the CPU.)"""
    def fails(node):
        with pytest.raises(TW.WalkError) as e:
            TW.walk(rec, quiet=True)
        assert node in e.value.nodes, (node, e.value.nodes)
    # the reduction leaves out the last of a unit's partial rows: the unit with the most rows (the smallest share) among
    # those whose last workgroup had a tile to work on
    nd = max((n for n in rec.nodes if n.kind == 'unit' and n.partials is not None and bool(n.partials[n.rows - 1].any())),
             key=lambda n: n.rows)
    keep = [g.clone() for g in nd.g]
    last = torch.split(nd.partials[nd.rows - 1], [g.numel() for g in nd.g])
    print(f'[tampered] last of {nd.rows} partial rows of {nd.name}: {float(last[0].abs().max() / nd.g[0].abs().max()):.2e} of max |dw1|')
    nd.g = [g - l for g, l in zip(nd.g, last)]
    fails(f'reduce {nd.name}')
    nd.g = keep
    # d(gamma) / d(beta) of one layer read from its neighbour's block
    a, b = rec.bn['neck.lateral_convs.0.bn'], rec.bn['neck.lateral_convs.1.bn']
    a.dgamma, b.dgamma = b.dgamma, a.dgamma
    fails('bn_grad 0')
    a.dgamma, b.dgamma = b.dgamma, a.dgamma
    # a pyramid tap without the merge's share of its gradient
    tap, out = rec.tensors['backbone.model4.conv2'], rec.tensors['upadd(backbone.model4.conv2)']
    bn = TW._Walk(rec)
    bn.count = {tap.bn: tap.n * tap.h * tap.w}
    ref = bn.bnref(tap.bn)
    y = ref.xhat(tap.buf.double()) * ref.gamma + ref.beta
    keep = tap.grad.clone()
    tap.grad = (tap.grad.double() - out.grad.double() * (y > 0)).float()
    fails('grad backbone.model4.conv2')
    tap.grad = keep
    TW.walk(rec, quiet=True)


def test_train_step_walk_keep_pool_z(tmp_path):
    """YUNET_KEEP_POOL_Z=1 in a fresh process (the switch is read when the plan is built): the same walk with every z stored,
    and the flat gradient's bytes are the default plan's"""
    out = tmp_path / 'walk.pt'
    env = dict(os.environ, YUNET_KEEP_POOL_Z='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'train_walk_child.py'), 'n_keep_pool_z', str(out)],
                       env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(out, weights_only=False)
    assert max(got['worst'].values()) <= 1.0
    if 'n_fp32' not in _GRAD:
        _GRAD['n_fp32'] = run_case('n_fp32')[1]
    assert torch.equal(got['grad'], _GRAD['n_fp32']), 'the flat gradient differs from the default plan'
