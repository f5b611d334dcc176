"""CPU: the fast deterministic level (deterministic='fast') -- its surface from the command line down
to the plan key, the plan it builds (a deterministic plan whose descriptors carry YUNET_DET_FAST), and that the DET instances
of the wave-streaming and split-bf16 kernels hold no fp64 atomic of any scope."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import yunet_amd
import yunet_amd._lib as L
import yunet_amd.engine as E
import yunet_amd.runner as R
import yunet_oracle as O
from test_train_cli import CFG, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'libfacedetection.train_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
FAST = E.DET_ROWS | L.DET_FAST
UNIT = 'backbone.model0.conv2'          # the pooled 16 -> 16 unit


@pytest.fixture(autouse=True)
def reset_flag():
    yield
    R._DETERMINISTIC = False


def model(kind='n'):
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    return yunet_amd.build_detector(cfg.model), cfg


# ------------------------------------------------------------------------------------------------------------ surface
def test_levels_are_stored_as_given_and_other_strings_are_refused():
    m, _ = model()
    eng = E.YuNetEngine(m.arch(), 'cpu')
    for flag, want in ((False, False), (True, True), ('fast', 'fast'), (1, True), (0, False)):
        eng.set_deterministic(flag)
        m.set_deterministic(flag)
        assert eng.deterministic == want and type(eng.deterministic) is type(want)
        assert m._deterministic == want and type(m._deterministic) is type(want)
    for bad in ('slow', 'Fast', 'true', ''):
        with pytest.raises(ValueError):
            eng.set_deterministic(bad)
        with pytest.raises(ValueError):
            m.set_deterministic(bad)
        with pytest.raises(ValueError):
            R.set_random_seed(1, deterministic=bad)
        with pytest.raises(ValueError):
            R.wants_deterministic(yunet_amd.Config(dict(deterministic=bad)))
    assert L.DET_FAST == 1 << 30 and re.search(r'#define YUNET_DET_FAST \(1 << 30\)',
                                               open(os.path.join(ROOT, 'include', 'yunet_hip.h')).read())


def test_model_passes_fast_to_its_engine_and_the_three_plans_coexist(monkeypatch):
    m, _ = model()
    m.set_deterministic('fast')
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)       # (bind_engine's logging buffer; no GPU here)
    eng = m.bind_engine('cpu')
    assert eng.deterministic == 'fast'
    built = []
    monkeypatch.setattr(E, 'Plan', lambda eng_, n, h, w, g: built.append(eng_.deterministic) or object())
    p_fast = eng.get_plan(2, 64, 64, 1)
    assert next(reversed(eng.plans)) == (2, 64, 64, 64, 'fp32', 'det-fast')
    m.set_deterministic(True)
    assert eng.deterministic is True
    p_det = eng.get_plan(2, 64, 64, 1)
    m.set_deterministic(False)
    p_def = eng.get_plan(2, 64, 64, 1)
    assert built == ['fast', True, False] and len({id(p_fast), id(p_det), id(p_def)}) == 3
    assert set(eng.plans) == {(2, 64, 64, 64, 'fp32'), (2, 64, 64, 64, 'fp32', 'det'), (2, 64, 64, 64, 'fp32', 'det-fast')}
    m.set_deterministic('fast')
    assert eng.get_plan(2, 64, 64, 1) is p_fast and len(built) == 3


def test_bf16_with_fast_raises_in_both_orders_and_in_the_plan():
    m, _ = model()
    m.set_deterministic('fast')
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        m.set_precision('bf16')
    m.set_deterministic(False)
    m.set_precision('bf16')
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        m.set_deterministic('fast')
    eng = E.YuNetEngine(m.arch(), 'cpu')
    eng.set_deterministic('fast')
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        eng.set_precision('bf16')
    eng.set_deterministic(False)
    eng.set_precision('bf16')
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        eng.set_deterministic('fast')
    eng.deterministic = 'fast'                             # (set behind the setters' back: the plan builder checks too)
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        E.Plan(eng, 2, 64, 64, 64)


def test_cli_flag_sets_the_config_key(tmp_path, monkeypatch):
    seen = {}

    def fake_train(m, ds, cfg, **kw):
        seen.update(cfg=cfg, wants=R.wants_deterministic(cfg), flag=R._DETERMINISTIC)
        return []
    monkeypatch.setattr(T.R, 'train_detector', fake_train)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda i: None)
    common = [CFG, '--seed', '7', '--no-validate', '--cfg-options', 'data.samples_per_gpu=4',
              'data.train.type=SyntheticWiderFace', 'data.train.img_scale=(160,160)', 'data.train.iters_per_epoch=2']
    T.main(common + ['--work-dir', str(tmp_path / 'a'), '--deterministic-fast'])
    assert seen['cfg']['deterministic'] == 'fast' and seen['wants'] == 'fast' and seen['flag'] == 'fast'
    assert yunet_amd.Config.fromfile(str(tmp_path / 'a' / 'yunet_n.py')).deterministic == 'fast'
    R._DETERMINISTIC = False
    T.main(common + ['--work-dir', str(tmp_path / 'b'), '--deterministic'])
    assert seen['cfg']['deterministic'] is True and seen['wants'] is True and seen['flag'] is True


class Stop(Exception):
    pass


def test_train_detector_passes_the_level_on_to_the_model(monkeypatch):
    m, cfg = model()
    calls = []
    monkeypatch.setattr(type(m), 'to', lambda self, *a, **k: (_ for _ in ()).throw(Stop()))
    monkeypatch.setattr(type(m), 'set_deterministic', lambda self, flag=True: calls.append(flag))
    cfg['deterministic'] = 'fast'
    with pytest.raises(Stop):
        R.train_detector(m, None, cfg)
    del cfg['deterministic']
    R.set_random_seed(3, deterministic='fast')
    with pytest.raises(Stop):
        R.train_detector(m, None, cfg)
    cfg['deterministic'] = True                           # (the config's own spelling wins over the process-wide one)
    with pytest.raises(Stop):
        R.train_detector(m, None, cfg)
    assert calls == ['fast', 'fast', True]
    cfg['deterministic'] = 'fast'
    cfg['fp16'] = dict(loss_scale=512.)
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        R.train_detector(m, None, cfg)


# --------------------------------------------------------------------------------------------------------------- plan
def bn_words(plan):
    """(slots, det_rows) of every BatchNorm descriptor with a sum block, over the forward and backward lists"""
    out = []
    for lst in (plan.fwd_a, plan.fwd_b, plan.bwd):
        for op in lst:
            if op.opcode in (L.OP_DP_FWD, L.OP_DP_BWD):
                out += [(bn.slots, bn.det_rows) for bn in (op.dp.in_bn, op.dp.out_bn) if bn.stats]
    return out


def fold_ops(plan):
    return [[(op.i[0], op.i[1]) for op in lst if op.opcode == L.OP_BN_FOLD] for lst in (plan.fwd_a, plan.bwd)]


def test_fast_plan_is_a_deterministic_plan_with_the_flag_in_every_descriptor(monkeypatch):
    """N = 4 at 128 x 128 (the stem's map is 64 x 64: the pooled 16 -> 16 unit is on the streaming kernels): the same fold ops,
    row counts, memset and eval handling as the True plan, no lanes and no grouped launch; R | YUNET_DET_FAST in every
    BatchNorm descriptor where the True plan has R; the pooled unit's z elided where the True plan keeps it."""
    monkeypatch.delenv('YUNET_KEEP_POOL_Z', raising=False)
    eng = E.YuNetEngine(O.yunet_arch('n'), 'cpu')
    shape = (4, 128, 128, 64)
    dflt = E.Plan(eng, *shape)
    eng.set_deterministic(True)
    det = E.Plan(eng, *shape)
    eng.set_deterministic('fast')
    fast = E.Plan(eng, *shape)
    assert fast.det and det.det and not dflt.det and (dflt.det_rows, det.det_rows, fast.det_rows) == (0, E.DET_ROWS, FAST)
    n_bn = len(eng.layout.bn_names)
    assert fold_ops(fast) == fold_ops(det) and [len(f) for f in fold_ops(fast)] == [n_bn, n_bn]
    assert all(rows == E.DET_ROWS for f in fold_ops(fast) for rows, _ in f)
    assert fast.stats.numel() == det.stats.numel() == dflt.stats.numel() // E.BN_SLOTS * (1 + E.DET_ROWS)
    assert [op.opcode for op in fast.fwd_a] == [op.opcode for op in det.fwd_a]
    assert [op.opcode for op in fast.bwd] == [op.opcode for op in det.bwd]
    assert bn_words(fast) and set(bn_words(fast)) == {(1, FAST)} and set(bn_words(det)) == {(1, E.DET_ROWS)}
    assert len(bn_words(fast)) == len(bn_words(det))
    assert fast.bn_table_f.tolist() == det.bn_table_f.tolist()
    for op in fast.fwd_a:
        if op.opcode == L.OP_STEM_FWD:
            assert op.i[4] == E.DET_ROWS                       # (the stem entry takes the plain row count)
        if op.opcode == L.OP_DP_FWD:
            assert op.i[L.OP_GROUP] == 0
    assert not fast.lanes_ok
    assert any(op.opcode == L.OP_DP_FWD and op.i[L.OP_GROUP] >= 2 for op in dflt.fwd_a)
    assert not any(op.opcode == L.OP_BN_FOLD for op in fast.fwd_eval)
    stem = [op for op in fast.fwd_eval if op.opcode == L.OP_STEM_FWD]
    assert len(stem) == 1 and stem[0].i[4] == 0 and stem[0].p[4] == fast.eval_scratch.data_ptr()
    # pool-z elision follows the backward dispatch: dp_bwd16s at the fast level, the tile kernel at the True level
    assert [zt for zt, _ in fast.elided_z] == [fast.tensors[UNIT][1]] and det.elided_z == []
    assert fast.tensors[UNIT][1].buf is None and det.tensors[UNIT][1].buf is not None
    for plan, null in ((fast, True), (det, False)):
        f = [op for op in plan.fwd_a if op.opcode == L.OP_DP_FWD and op.dp.pool_out and op.dp.cin == 16]
        b = [op for op in plan.bwd if op.opcode == L.OP_DP_BWD and op.dp.pool_idx and op.dp.cin == 16]
        assert len(f) == len(b) == 1 and (f[0].dp.z is None) == (b[0].dp.z is None) == null


# -------------------------------------------------------------------------------------------------------- instructions
FILES = ['conv_fwd64.hip', 'conv_fwd16.hip', 'conv_bwd16.hip', 'conv_bwd64.hip']
KERNELS = ('dp_fwd64s_kernel', 'dp_fwd16s_kernel', 'dp_bwd16s_kernel', 'dp_bwd64_kernel')
ATOMIC_F64 = re.compile(r'\b(ds_add(_rtn)?_f64|(global|flat|buffer)_atomic_add_f64)\b')


def _assembly(tmp, name):
    out = os.path.join(tmp, name.replace('.hip', '.s'))
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-Wno-unused-value', '-w']
    subprocess.run([HIPCC] + flags + ['-S', '--cuda-device-only', '-o', out, os.path.join(CSRC, name)], check=True,
                   capture_output=True, timeout=600)
    return out


def _functions(path):
    """{mangled symbol: body text} of every function of an assembly file"""
    txt = open(path).read()
    out = {}
    for m in re.finditer(r'^\s*\.type\s+(\S+),@function\n', txt, re.M):
        end = re.compile(r'^\.Lfunc_end\d+:', re.M).search(txt, m.end())
        out[m.group(1)] = txt[m.end():end.start()]
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
def test_det_instances_hold_no_fp64_atomic(tmp_path):
    """Every kernel whose last template argument (DET) is true holds no fp64 atomic add, LDS or global; the DET = false
    instance with the same leading arguments holds at least one, so the search sees them."""
    with ThreadPoolExecutor(4) as ex:
        paths = list(ex.map(lambda n: _assembly(str(tmp_path), n), FILES))
    funcs = {}
    for p in paths:
        funcs.update(_functions(p))
    syms = sorted(funcs)
    cxxfilt = shutil.which('llvm-cxxfilt') or shutil.which('c++filt') or '/opt/rocm/llvm/bin/llvm-cxxfilt'
    names = subprocess.run([cxxfilt], input='\n'.join(syms), capture_output=True, text=True, check=True).stdout.split('\n')
    inst = {}          # (kernel, leading template arguments) -> {DET: number of fp64 atomics}
    for sym, name in zip(syms, names):
        m = re.search(r'(\w+)<([^>]*)>\(', name)
        if not m or m.group(1) not in KERNELS:
            continue
        args = [a.strip() for a in m.group(2).split(',')]
        assert args[-1] in ('true', 'false'), name
        inst.setdefault((m.group(1), tuple(args[:-1])), {})[args[-1] == 'true'] = len(ATOMIC_F64.findall(funcs[sym]))
    want = {'dp_fwd64s_kernel': 2, 'dp_fwd16s_kernel': 3, 'dp_bwd16s_kernel': 2, 'dp_bwd64_kernel': 6}
    for kernel, count in want.items():
        assert sum(k[0] == kernel for k in inst) == count, (kernel, sorted(inst))
    for key, forms in inst.items():
        assert set(forms) == {True, False}, key
        assert forms[True] == 0, (key, forms)
        assert forms[False] >= 1, (key, forms)
