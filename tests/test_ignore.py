"""CPU: ignore regions -- the capacity rule and the source's constructor, the combinations that
raise, ignore_iof_thr parsing, the engine's plans with and without the option, the C header against the ctypes binding,
the fixture made by the unmodified reference (tools/make_golden_ignore.py) and the fp64 restatements of
tests/ignore_ref.py, pinned to the reference's own CrossEntropyLoss with a 0 / 1 weight."""
import importlib.util
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ignore_ref as G
import loss_ref as R
import ref_stub
import yunet_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(ROOT, 'configs', 'yunet_n.py')
ICOUNTS = [0, 2, 20]          # ignore boxes per image of the label file below


def write_labels(path, icounts=ICOUNTS, w=96, h=80, prefix='im'):
    """A labelv2 file: image i has two faces with landmarks and icounts[i] rows that carry the ignore flag."""
    lines = []
    for i, c in enumerate(icounts):
        lines.append(f'# {prefix}{i}.png {w} {h}')
        for g in range(2):
            x, y = 10 + 40 * g, 12 + 20 * g
            kp = ' '.join(f'{x + 3 + 2 * j} {y + 4 + j} 1' for j in range(5))
            lines.append(f'{x} {y} {x + 24} {y + 28} {kp}')
        for g in range(c):
            x, y = 2 + 9 * (g % 10), 3 + 30 * (g // 10)
            lines.append(f'{x} {y} {x + 7} {y + 9} 1')
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return str(path)


def ref_pipeline():
    import yunet_amd
    return yunet_amd.Config.fromfile(CFG).data.train.pipeline


def make_source(tmp_path, icounts=ICOUNTS, **kw):
    from yunet_amd.datasets import RetinaFaceDataset, RetinaFaceSource
    ds = RetinaFaceDataset(write_labels(tmp_path / 'l.txt', icounts), img_prefix=str(tmp_path), min_size=kw.pop('min_size', None))
    return RetinaFaceSource(ds, kw.pop('pipeline', None) or ref_pipeline(), samples_per_gpu=3, workers=0, **kw)


# ------------------------------------------------------------------------------------------------------ capacity
def test_capacity_rule_table():
    from yunet_amd.kernels import ignore_capacity_rows as rows_k
    from yunet_amd.pipelines import ignore_capacity_rows
    for cap, rows in [(0, 16), (1, 16), (16, 16), (17, 32), (33, 64), (1000, 1024), (1024, 1024), (5000, 1024)]:
        assert ignore_capacity_rows(cap) == rows == rows_k(cap)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError):
            ignore_capacity_rows(bad)


def test_source_capacity_none_dataset_int(tmp_path, caplog):
    from yunet_amd.datasets import ignore_counts
    with caplog.at_level(logging.WARNING):
        off = make_source(tmp_path)
        assert off.ignore_rows is None and off.pipe.ignore_rows is None
        ds_rows = make_source(tmp_path, ignore_capacity='dataset')
        assert ignore_counts(ds_rows.ds) == ICOUNTS
        assert ds_rows.ignore_rows == 32 == ds_rows.pipe.ignore_rows
        assert make_source(tmp_path, ignore_capacity=20).ignore_rows == 32
        assert make_source(tmp_path, ignore_capacity=2000, icounts=[0, 1]).ignore_rows == 1024
        assert make_source(tmp_path, ignore_capacity='dataset', icounts=[0, 1]).ignore_rows == 16       # the floor
    assert not caplog.records
    with caplog.at_level(logging.WARNING):
        assert make_source(tmp_path, ignore_capacity=3).ignore_rows == 16
    lines = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(lines) == 1 and '1 images' in lines[0] and 'largest 20' in lines[0] and '4 boxes' in lines[0], lines
    with pytest.raises(ValueError, match='ignore_capacity'):
        make_source(tmp_path, ignore_capacity='all')
    # min_size turns small faces into ignore rows: the count of the dataset rule follows
    small = make_source(tmp_path, ignore_capacity='dataset', min_size=8, icounts=[0, 30])
    assert ignore_counts(small.ds) == [0, 30] and small.ignore_rows == 32       # 7 px wide rows: below min_size and flagged


def test_train_config_surface(tmp_path):
    """data.train.ignore_capacity reaches the source through tools/train.py's build_source, a digit string included."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import yunet_amd
    spec = importlib.util.spec_from_file_location('train_tool', os.path.join(ROOT, 'tools', 'train.py'))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    cfg = yunet_amd.Config.fromfile(CFG)
    cfg.data.train.type = 'RetinaFaceDataset'
    cfg.data.train.ann_file, cfg.data.train.img_prefix = write_labels(tmp_path / 'l.txt'), str(tmp_path)
    cfg.data.samples_per_gpu = 1
    for given, rows in ((None, None), ('dataset', 32), ('40', 64), (5, 16)):
        if given is None:
            cfg.data.train.pop('ignore_capacity', None)
        else:
            cfg.data.train['ignore_capacity'] = given
        assert T.build_source(cfg, 0, 1, 0).ignore_rows == rows


@pytest.mark.parametrize('step', ['Mosaic', 'RandomAffine', 'MixUp'])
def test_mixing_steps_with_ignore_capacity_raise(step):
    from yunet_amd.pipelines import DevicePipeline
    base = [dict(p) for p in ref_pipeline()]
    names = [p['type'] for p in base]
    extra = dict(Mosaic=dict(type='Mosaic', img_scale=(640, 640), use_kps=True),
                 RandomAffine=dict(type='RandomAffine', use_kps=True),
                 MixUp=dict(type='MixUp', img_scale=(640, 640), use_kps=True))[step]
    at = names.index('RandomSquareCrop') if step == 'Mosaic' else names.index('Normalize')
    cfg = base[:at] + [extra] + base[at:]
    DevicePipeline(cfg, seed=0, gmax=64)                                   # the list itself is one this pipeline runs
    with pytest.raises(NotImplementedError, match=step):
        DevicePipeline(cfg, seed=0, gmax=64, ignore_rows=16)
    with pytest.raises(ValueError, match='power of two'):
        DevicePipeline(base, seed=0, gmax=64, ignore_rows=17)
    assert DevicePipeline(base, seed=0, gmax=64, ignore_rows=32).ignore_rows == 32


def test_ignore_iof_thr_parsing():
    from yunet_amd.sim_ota_assigner import SimOTAAssigner, parse_ignore_iof_thr
    assert SimOTAAssigner().ignore_iof_thr == -1.0
    for given, want in ((-1, -1.0), (-0.5, -1.0), (None, -1.0), (0, 0.0), (0.5, 0.5), (1, 1.0)):
        assert parse_ignore_iof_thr(given) == want
        assert SimOTAAssigner(ignore_iof_thr=given).ignore_iof_thr == want
    for bad in (1.5, float('nan')):
        with pytest.raises(ValueError):
            SimOTAAssigner(ignore_iof_thr=bad)
    for bad in ('0.5', True):
        with pytest.raises(TypeError):
            SimOTAAssigner(ignore_iof_thr=bad)
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(CFG)
    assert 'ignore_iof_thr' not in yunet_amd.build_detector(cfg.model).arch()             # off: the arch it always was
    cfg.model.train_cfg.assigner['ignore_iof_thr'] = 0.5
    assert yunet_amd.build_detector(cfg.model).arch()['ignore_iof_thr'] == 0.5


# --------------------------------------------------------------------------------------------------------- plans
def _plan_dump():
    spec = importlib.util.spec_from_file_location('plan_dump', os.path.join(ROOT, 'tools', 'dbg', 'plan_dump.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dump(pd, eng, plan):
    lines = []
    pd.dump_plan(eng, plan, lines.append)
    return lines


@pytest.mark.parametrize('kind,det', [('n', False), ('s', False), ('n', 'fast')])
def test_plans_without_the_option_are_the_parents_and_with_it_differ_in_two_ops(kind, det, monkeypatch):
    """The default plan's dump is pinned to the parent's by tests/golden/plan_dump_default.sha256 (tests/test_deterministic.py
    runs the whole table); here: an engine that KNOWS a threshold but gets no ignore boxes builds the same lists under the
    same key, and a plan with them has every op of the default plan plus one OP_IGNORE_MARK, and the flag on OP_LOSS."""
    import yunet_amd._lib as L
    import yunet_amd.engine as E
    monkeypatch.setenv('YUNET_KEEP_POOL_Z', '1')          # (the dump names every tensor: tools/dbg/plan_dump.py)
    pd = _plan_dump()
    shape = (2, 64, 64, 64)
    eng0 = E.YuNetEngine(O.yunet_arch(kind), 'cpu')
    eng1 = E.YuNetEngine(dict(O.yunet_arch(kind), ignore_iof_thr=0.5), 'cpu')
    for e in (eng0, eng1):
        e.set_deterministic(det)
    assert eng0.ignore_iof_thr == -1.0 and eng1.ignore_iof_thr == 0.5
    p0, p1 = eng0.get_plan(2, 64, 64, 1), eng1.get_plan(2, 64, 64, 1)
    assert list(eng0.plans) == list(eng1.plans) and 'ignore' not in list(eng1.plans)[0]
    assert _dump(pd, eng0, p0) == _dump(pd, eng1, p1)
    # the option: keyed by ('ignore', Imax)
    boxes, cnt = torch.zeros(2, 16, 4), torch.zeros(2, dtype=torch.int32)
    assert eng0._imax(boxes, cnt) == 0 and eng1._imax(None, None) == 0 and eng1._imax(boxes, cnt) == 16
    pi = eng1.get_plan(2, 64, 64, 1, 16)
    key = [k for k in eng1.plans if 'ignore' in k]
    assert len(key) == 1 and key[0][-2:] == ('ignore', 16) and key[0][:-2] == list(eng0.plans)[0]
    assert eng1.get_plan(2, 64, 64, 1, 32) is not pi and eng1.get_plan(2, 64, 64, 1, 16) is pi
    ops0 = [op.opcode for op in p1.fwd_a]
    opsi = [op.opcode for op in pi.fwd_a]
    assert opsi == ops0 + [L.OP_IGNORE_MARK] and opsi[-3:] == [L.OP_ASSIGN, L.OP_LOSS_NORM, L.OP_IGNORE_MARK]
    assert [op.opcode for op in pi.fwd_b] == [op.opcode for op in p1.fwd_b]
    assert [op.opcode for op in pi.bwd] == [op.opcode for op in p1.bwd]
    assert [op.opcode for op in pi.fwd_eval] == [op.opcode for op in p1.fwd_eval]          # eval: no mark op either
    assert p1.fwd_b[0].i[L.LOSS_FLAGS_SLOT] == 0 and pi.fwd_b[0].i[L.LOSS_FLAGS_SLOT] == L.LOSS_IGNORE
    assert pi.c_fwd_b_loss[0].i[L.LOSS_FLAGS_SLOT] == L.LOSS_IGNORE and pi.c_fwd_b_loss[0].loss.defer_num_total == 1
    m = pi.c_fwd_a[pi.mark_idx]
    assert (m.i[0], m.i[1], m.i[2]) == (2, pi.P, 16) and m.f[0] == 0.5
    assert m.p[0] == pi.ign_boxes.data_ptr() and m.p[1] == pi.ign_count.data_ptr() and m.p[2] == pi.gt_inds.data_ptr()
    assert m.p[3] is None
    # bound without a copy: the batch's tensors, then the plan's own again
    pi.bind_ignore(boxes, cnt, 0.25)
    m = pi.c_fwd_a[pi.mark_idx]
    assert m.p[0] == boxes.data_ptr() and m.p[1] == cnt.data_ptr() and m.f[0] == 0.25
    # the validation lists: mark between the normaliser and the value-only flagged loss
    pi.val_ops()
    ai = pi.val_assign_idx
    assert [op.opcode for op in pi.c_val[ai:]] == [L.OP_ASSIGN, L.OP_LOSS_NORM, L.OP_IGNORE_MARK, L.OP_LOSS, L.OP_LOSS_FINALIZE]
    assert pi.c_val[ai + 2].p[0] == boxes.data_ptr() and pi.c_val[ai + 2].f[0] == 0.25
    assert pi.c_val[ai + 3].p[6] is None and pi.c_val[ai + 3].i[L.LOSS_FLAGS_SLOT] == L.LOSS_IGNORE
    p1.val_ops()
    assert [op.opcode for op in p1.c_val[p1.val_assign_idx:]] == [L.OP_ASSIGN, L.OP_LOSS_NORM, L.OP_LOSS, L.OP_LOSS_FINALIZE]


@pytest.mark.skipif(not shutil.which('cc'), reason='no C compiler')
def test_constants_and_layouts_match_the_header(tmp_path):
    import ctypes as C
    import yunet_amd._lib as L
    src = tmp_path / 'h.c'
    src.write_text('#include <stdio.h>\n#include "yunet_hip.h"\n'
                   'int main(){printf("%d %d %d %d %zu %zu %zu\\n",YUNET_OP_IGNORE_MARK,YUNET_OP_STEM_BWD_DX,YUNET_LOSS_IGNORE,'
                   'YUNET_ABI_VERSION,sizeof(YunetOp),sizeof(YunetLossCfg),sizeof(YunetLossTerms));return 0;}')
    exe = tmp_path / 'h'
    subprocess.check_call(['cc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [L.OP_IGNORE_MARK, L.OP_STEM_BWD_DX, L.LOSS_IGNORE, 12, C.sizeof(L.YunetOp), C.sizeof(L.YunetLossCfg),
                   C.sizeof(L.YunetLossTerms)]
    assert L.OP_IGNORE_MARK == L.OP_STEM_BWD_DX + 1                    # appended at the end of the enum
    assert L.LOSS_FLAGS_SLOT == 8 and L.LOSS_FLAGS_SLOT not in (L.OP_LANE, L.OP_GROUP, 11)
    for name in ('yunet_ignore_mark', 'yunet_loss_terms_ex', 'yunet_aug_ignore'):
        assert name in L.EXPORTED
        assert f'int {name}(' in open(os.path.join(ROOT, 'include', 'yunet_hip.h')).read()
    lib = L.load()
    assert lib.yunet_abi_version() == 12
    # argument checks that need no device: a null box pointer, too many rows, a negative threshold
    lv = __import__('yunet_amd.kernels', fromlist=['x']).make_levels([(8, 8), (4, 4), (2, 2)], [8, 16, 32])
    one = C.c_void_p(16)
    assert lib.yunet_ignore_mark(None, one, C.byref(lv), 1, 84, 16, 0.5, one, None, None) == L.EINVAL
    assert lib.yunet_ignore_mark(one, one, C.byref(lv), 1, 84, 2048, 0.5, one, None, None) == L.EINVAL
    assert lib.yunet_ignore_mark(one, one, C.byref(lv), 1, 84, 16, -1.0, one, None, None) == L.EINVAL
    assert lib.yunet_ignore_mark(one, one, C.byref(lv), 1, 85, 16, 0.5, one, None, None) == L.EINVAL       # P of other levels
    assert lib.yunet_aug_ignore(one, one, None, 64, 1, 16, one, one, None) == L.EINVAL


# ------------------------------------------------------------------------------------------------------- fixture
@pytest.mark.parametrize('name', list(G.SETS))
def test_fixture_holds_the_hard_cases_and_the_restatement_gives_it(name):
    iteration, items, outs = G.load_set(name)
    assert len(items) == 4 and [len(it['ign']) for it in items][1] == 0
    seen = G.hard_cases(items, outs)
    assert all(seen.values()), seen
    for it, o in zip(items, outs):
        mine, mask = G.transform(it['ign'], it['left'], it['top'], it['cw'], it['S'], it['flip'])
        assert mine.dtype == o.dtype and np.array_equal(mine, o)
        assert o.shape[0] == int(mask.sum())
        assert (o >= 0).all() and (o <= it['S']).all()
    assert max(len(o) for o in outs) == 17 and G.ROWS == 16              # 17 kept rows into 16
    if name == 'r32_96':
        assert len({it['S'] for it in items}) >= 2 and all(it['S'] in (32, 64, 96) for it in items)
    ob, oc = G.padded(outs)
    assert oc.tolist() == [min(len(o), 16) for o in outs] and not ob[1].any()
    assert os.path.getsize(G.GOLD) < 64 * 1024


# -------------------------------------------------------------------------------------------------- restatements
def test_mark_rule_on_exact_thresholds_and_positives():
    sizes, strides = [(8, 8), (4, 4), (2, 2)], [8, 16, 32]
    gi = torch.zeros(1, 84, dtype=torch.int32)
    gi[0, 9] = 3                                                          # a positive under the box: stays
    # [8, 8, 12, 16] covers half of cell (1, 1) of stride 8 (prior 9) and 1/8 of cell (0, 0) of stride 16 (prior 64)
    boxes = torch.tensor([[[8.0, 8.0, 12.0, 16.0], [0.0, 0.0, 64.0, 64.0]]])
    cnt = torch.tensor([1], dtype=torch.int32)                            # the second row is beyond the count: not read
    out, iof = G.mark_ref(gi, boxes, cnt, sizes, strides, 0.5)
    assert float(iof[0, 9]) == 0.5 and float(iof[0, 64]) == 0.125 and int((iof > 0).sum()) == 3
    assert int((out == -1).sum()) == 0 and int(out[0, 9]) == 3            # iof exactly on thr does not mark
    out, _ = G.mark_ref(gi, boxes, cnt, sizes, strides, 0.0)              # any overlap marks; the positive stays
    assert sorted((out[0] == -1).nonzero().flatten().tolist()) == [64, 80] and int(out[0, 9]) == 3
    gi[0, 9] = 0
    assert (G.mark_ref(gi, boxes, cnt, sizes, strides, 0.25)[0][0] == -1).nonzero().flatten().tolist() == [9]
    out, _ = G.mark_ref(gi, boxes, torch.tensor([0], dtype=torch.int32), sizes, strides, 0.0)
    assert torch.equal(out, gi)


def test_masked_case_equals_the_masked_reference():
    case = R.make_case(2, 64, 64, 5, boxes=('generic', 'tie'))
    cfg = R.make_cfg('EIoULoss')
    marked, _ = G.mark_some(case, seed=1)
    assert 0.2 < float(marked.sum()) / float((case['gt_inds'] == 0).sum()) < 0.45
    a = G.masked_loss_ref(case, cfg, marked)
    b = R.ref_of(G.masked_case(case, marked), cfg)
    assert torch.equal(a['losses'], b['losses']) and torch.equal(a['dflat'], b['dflat'])
    assert float(a['losses'][2]) < float(a['ref']['losses'][2])
    assert torch.equal(a['losses'][[0, 1, 3]], a['ref']['losses'][[0, 1, 3]])
    r32 = R.ref_of(G.masked_case(case, marked), cfg, dtype=torch.float32)
    assert bool((r32['dflat'][marked] == 0).all()) and bool((r32['terms']['obj'][marked] == 0).all())


@pytest.mark.skipif(not ref_stub.available(), reason='reference tree not present')
def test_masked_loss_obj_is_the_references_cross_entropy_with_a_weight():
    """mmdet's CrossEntropyLoss(use_sigmoid=True, reduction='sum') called with weight = 0 on the marked priors and
    avg_factor-free, divided by num_total as yunet_head.py:509-510 does: the masked loss_obj and its gradient."""
    ns = ref_stub.load_reference()
    case = R.make_case(2, 64, 64, 6, boxes=('generic',))
    cfg = R.make_cfg('EIoULoss')
    marked, _ = G.mark_some(case, seed=2)
    mine = G.masked_loss_ref(case, cfg, marked)
    ce = ns.losses.ce.CrossEntropyLoss(use_sigmoid=True, reduction='sum', loss_weight=cfg['w_obj'])
    # the reference's own precision: its binary_cross_entropy casts label and weight to float32
    x = case['flat'][..., 5].reshape(-1, 1).clone().requires_grad_(True)
    target = (case['gt_inds'] > 0).float().reshape(-1, 1)
    weight = (~marked).float().reshape(-1, 1)
    loss = ce(x, target, weight=weight) / mine['ref']['num_total']
    g, = torch.autograd.grad(loss, x)
    g = g.reshape(marked.shape).double()
    # an fp32 sum of N * P terms against fp64: n * u * sum |term|, here relative to the (all-positive) sum
    n_terms = marked.numel()
    assert abs(float(loss.detach()) - float(mine['losses'][2])) <= (n_terms + 8) * R.U32 * float(mine['losses'][2])
    # sigmoid(x) - t in fp32, times weight / num_total: a few roundings of values below 1 / num_total
    assert float((g - mine['dflat'][..., 5]).abs().max()) <= 8 * R.U32 * cfg['w_obj'] / mine['ref']['num_total']
    assert bool((g[marked] == 0).all()) and bool((mine['dflat'][..., 5][marked] == 0).all())
    assert bool((g[~marked] != 0).any())
