"""CPU: the gradient with respect to the input image -- the additive C ABI, the plan key component
`input_grad`, the op lists with the option off (unchanged) and on (one OP_STEM_BWD_DX, a backward that reaches the stem
whatever is frozen), built on 'cpu' like the plans of tests/test_deterministic.py and tests/test_finetune.py."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest
import torch

import yunet_amd._lib as L
import yunet_amd.engine as E
import yunet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 64, 64, 64)


def plan_dump():
    spec = importlib.util.spec_from_file_location('plan_dump', os.path.join(ROOT, 'tools', 'dbg', 'plan_dump.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dump(mod, eng, plan):
    lines = []
    mod.dump_plan(eng, plan, lines.append)
    return lines


def opcodes(ops):
    return [op.opcode for op in ops]


def stage_of(name):
    return int(name.split('.')[1][len('model'):]) if name.startswith('backbone.model') else None


def stage_signature(eng, k):
    bn = tuple(n for n in eng.layout.bn_names if stage_of(n) is not None and stage_of(n) <= k)
    keys = tuple(n for n in eng.layout.entries if stage_of(n) is not None and stage_of(n) <= k)
    return bn, keys


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_additions(tmp_path):
    """ABI 12 stays; both entries are declared, bound and exported with ten arguments; the op code is a new one, the same
    number in the header and in the ctypes mirror; bad arguments are refused on the host before any launch."""
    hdr = open(os.path.join(ROOT, 'include', 'yunet_hip.h')).read()
    lib = L.load()
    assert lib.yunet_abi_version() == 12
    for name in ('yunet_stem_bwd_dx', 'yunet_stem_bwd_dx_bf16'):
        assert name in L.EXPORTED and hasattr(lib, name) and re.search(rf'\bint {name}\(', hdr), name
        assert len(L._SIGNATURES[name][1]) == 10
    others = [v for k, v in vars(L).items() if k.startswith('OP_') and k not in ('OP_STEM_BWD_DX', 'OP_LANE', 'OP_GROUP')]
    assert len(others) >= 23 and len(set(others)) == len(others) and L.OP_STEM_BWD_DX not in others
    src = tmp_path / 'o.c'
    src.write_text('#include <stdio.h>\n#include "yunet_hip.h"\n'
                   'int main(){printf("%d %d %d\\n",YUNET_OP_STEM_BWD_DX,YUNET_OP_BN_FOLD,YUNET_ABI_VERSION);return 0;}')
    exe = tmp_path / 'o'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [L.OP_STEM_BWD_DX, L.OP_BN_FOLD, 12]
    bn = L.YunetBN(8, 8, 8, 8, 1, 1e-5)
    p = C.c_void_p(16)
    for fn in (lib.yunet_stem_bwd_dx, lib.yunet_stem_bwd_dx_bf16):
        assert fn(None, p, C.byref(bn), p, p, 1, 32, 32, 16, None) == L.EINVAL
        assert fn(p, None, C.byref(bn), p, p, 1, 32, 32, 16, None) == L.EINVAL
        assert fn(p, p, None, p, p, 1, 32, 32, 16, None) == L.EINVAL
        assert fn(p, p, C.byref(bn), None, p, 1, 32, 32, 16, None) == L.EINVAL
        assert fn(p, p, C.byref(bn), p, None, 1, 32, 32, 16, None) == L.EINVAL
        assert fn(p, p, C.byref(bn), p, p, 1, 31, 32, 16, None) == L.EINVAL
        assert fn(p, p, C.byref(bn), p, p, 1, 32, 30 + 1, 16, None) == L.EINVAL
        assert fn(p, p, C.byref(bn), p, p, 1, 32, 32, 8, None) == L.EINVAL
        assert fn(p, p, C.byref(bn), p, p, 0, 32, 32, 16, None) == L.EINVAL
        assert fn(p, p, C.byref(L.YunetBN(8, None, 8, 8, 1, 1e-5)), p, p, 1, 32, 32, 16, None) == L.EINVAL


# ------------------------------------------------------------------------------------------------------------ option off
@pytest.mark.parametrize('kind', ['n', 's'])
def test_option_off_changes_no_op(kind, monkeypatch):
    """A plan built with the option off, in an engine that built an input_grad plan before, against the same plan of an
    engine without the attribute: every field of every op of every list, pointers as (buffer, offset)."""
    monkeypatch.setenv('YUNET_KEEP_POOL_Z', '1')          # (the dump names every tensor: tools/dbg/plan_dump.py)
    mod = plan_dump()
    old = E.YuNetEngine(O.yunet_arch(kind), 'cpu')
    del old.input_grad, old.input_grad_out                # the engine as it was before the option existed
    p_old = E.Plan(old, *SHAPE)
    assert not p_old.input_grad and p_old.dimg_ptr_ops == []
    new = E.YuNetEngine(O.yunet_arch(kind), 'cpu')
    new.set_input_grad(True)
    p_on = new.get_plan(*SHAPE)
    new.set_input_grad(False)
    p_off = new.get_plan(*SHAPE)
    assert p_off is not p_on and not p_off.input_grad and p_on.input_grad
    assert dump(mod, old, p_old) == dump(mod, new, p_off)
    assert not any(op.opcode == L.OP_STEM_BWD_DX for lst in (p_off.fwd_a, p_off.fwd_b, p_off.bwd, p_off.fwd_eval) for op in lst)
    # the forward lists of the option's own plan are those of the plain one too
    a, b = dump(mod, new, p_on), dump(mod, new, p_off)
    cut = lambda lines: lines[:next(i for i, l in enumerate(lines) if l.startswith('  c_bwd:'))]
    assert cut(a) == cut(b)


# ------------------------------------------------------------------------------------------------------------- option on
@pytest.mark.parametrize('det', [False, True, 'fast'])
@pytest.mark.parametrize('kind', ['n', 's'])
def test_option_on_appends_one_op_and_keys_the_plan(kind, det):
    eng = E.YuNetEngine(O.yunet_arch(kind), 'cpu')
    eng.set_deterministic(det)
    dflt = eng.get_plan(2, 64, 64, 1)
    eng.set_input_grad(True)
    pl = eng.get_plan(2, 64, 64, 1)
    eng.set_input_grad(False)
    assert eng.get_plan(2, 64, 64, 1) is dflt
    eng.set_input_grad(True)
    assert eng.get_plan(2, 64, 64, 1) is pl and pl is not dflt and len(eng.plans) == 2
    keys = list(eng.plans)
    assert keys[0] + ('input-grad',) == keys[1]
    dx = [i for i, op in enumerate(pl.bwd) if op.opcode == L.OP_STEM_BWD_DX]
    assert len(dx) == 1 and pl.dimg_ptr_ops == dx
    i = dx[0]
    # right behind the stem's weight gradient (and, deterministic plans, the fold in front of it), same dy, z and reader
    assert pl.bwd[i - 1].opcode == L.OP_STEM_BWD
    assert opcodes(pl.bwd[:i]) + opcodes(pl.bwd[i + 1:]) == opcodes(dflt.bwd)
    op, wg = pl.bwd[i], pl.bwd[i - 1]
    assert (op.p[1], op.p[2]) == (wg.p[1], wg.p[2]) and op.p[3] == wg.p[4] and not op.p[0]
    assert list(op.i[:4]) == [2, 64, 64, 16] and op.i[11] == L.F32
    assert bytes(op.bn[0]) == bytes(wg.bn[0])
    assert len(pl.reduce_jobs) == len(dflt.reduce_jobs)
    # set_dimg patches the one-list form and the two-segment copies
    t = torch.empty(2, 3, 64, 64)
    pl.set_dimg(t)
    assert pl.c_bwd[i].p[0] == t.data_ptr()
    if pl.split_off is not None:
        assert i >= pl.split_ops and pl.c_bwd_b[i - pl.split_ops].p[0] == t.data_ptr()
        assert pl.c_bwd_b[i - pl.split_ops].opcode == L.OP_STEM_BWD_DX
    with pytest.raises(AssertionError):
        dflt.set_dimg(t)


def test_bf16_plan_carries_the_storage_flag():
    eng = E.YuNetEngine(O.yunet_arch('n'), 'cpu')
    eng.set_precision('bf16')
    eng.set_input_grad(True)
    pl = eng.get_plan(2, 64, 64, 1)
    op = [op for op in pl.bwd if op.opcode == L.OP_STEM_BWD_DX]
    assert len(op) == 1 and op[0].i[11] == L.BF16 and (2, 64, 64, 64, 'bf16', 'input-grad') in eng.plans


# ---------------------------------------------------------------------------------------------------------- frozen prefix
@pytest.mark.parametrize('det', [False, True, 'fast'])
def test_frozen_prefix_reaches_the_stem(det):
    """frozen_stages = 2 with the image gradient: every backward op of the default plan but the stem's weight gradient is
    there, the frozen units have no reduce job, no fold op serves a frozen layer, and the list ends its kernels with the
    backward-data op reading the zero block."""
    eng = E.YuNetEngine(O.yunet_arch('n'), 'cpu')
    eng.set_deterministic(det)
    dflt = E.Plan(eng, *SHAPE)
    bn, keys = stage_signature(eng, 2)
    eng.set_frozen(bn, keys)
    frozen = E.Plan(eng, *SHAPE)
    eng.set_input_grad(True)
    pl = E.Plan(eng, *SHAPE)
    kern = (L.OP_DP_BWD, L.OP_POOL_BWD, L.OP_UPADD_BWD)
    assert opcodes([op for op in pl.bwd if op.opcode in kern]) == opcodes([op for op in dflt.bwd if op.opcode in kern])
    assert len([op for op in frozen.bwd if op.opcode == L.OP_DP_BWD]) == len([op for op in dflt.bwd if op.opcode == L.OP_DP_BWD]) - 5
    assert L.OP_STEM_BWD not in opcodes(pl.bwd) and opcodes(pl.bwd).count(L.OP_STEM_BWD_DX) == 1
    assert [w for w, _ in pl.img_ptr_ops] == ['fwd_a']
    # the reduce jobs, the d(gamma) / d(beta) table and the zeroed ranges are those of the frozen plan without the option
    g0 = eng.params.grad.data_ptr()
    assert [(j[1] - g0,) + j[2:] for j in pl.reduce_jobs] == [(j[1] - g0,) + j[2:] for j in frozen.reduce_jobs]
    assert len(pl.reduce_jobs) == len(dflt.reduce_jobs) - 6
    assert pl.bn_table_b.tolist() == frozen.bn_table_b.tolist() and pl._frozen_ranges() == frozen._frozen_ranges()
    blocks = {pl.bn[n]['bstats'].data_ptr(): n for n in eng.layout.bn_names}
    folds = [blocks[op.p[0]] for op in pl.bwd if op.opcode == L.OP_BN_FOLD]
    assert sorted(folds) == (sorted(n for n in eng.layout.bn_names if n not in bn) if det else [])
    # frozen readers take the zero block; the backward-data op is the stem's reader
    zero = pl.zero_bstats.data_ptr()
    dx = [op for op in pl.bwd if op.opcode == L.OP_STEM_BWD_DX][0]
    assert dx.bn[0].bstats == zero and dx.bn[0].stats == pl.bn['backbone.model0.bn1']['stats'].data_ptr()
    frozen_w = {eng.layout.unit_ptrs(eng.params.data, u)[0] for u in eng.layout.units
                if stage_of(u) is not None and stage_of(u) <= 2 and u != 'stem'}
    seen = [op for op in pl.bwd if op.opcode == L.OP_DP_BWD and op.dp.w_pw in frozen_w]
    assert len(seen) == 5 and all(op.dp.out_bn.bstats == zero and op.dp.dx for op in seen)
    job_rows = {j[0] for j in pl.reduce_jobs}
    assert not any(op.dp.wgrad_partials in job_rows for op in seen)


def test_everything_frozen_keeps_the_whole_backward():
    """Every BatchNorm and every parameter frozen: without the option the backward has no kernel at all, with it every
    dx-producing op and no reduction."""
    eng = E.YuNetEngine(O.yunet_arch('n'), 'cpu')
    dflt = E.Plan(eng, *SHAPE)
    eng.set_frozen(tuple(eng.layout.bn_names), tuple(eng.layout.entries))
    eng.set_input_grad(True)
    pl = E.Plan(eng, *SHAPE)
    kern = (L.OP_DP_BWD, L.OP_POOL_BWD, L.OP_UPADD_BWD)
    assert opcodes([op for op in pl.bwd if op.opcode in kern]) == opcodes([op for op in dflt.bwd if op.opcode in kern])
    assert pl.reduce_jobs == [] and L.OP_REDUCE_BATCH not in opcodes(pl.bwd) and L.OP_STEM_BWD not in opcodes(pl.bwd)
    assert opcodes(pl.bwd).count(L.OP_STEM_BWD_DX) == 1 and pl.bn_table_b is None
