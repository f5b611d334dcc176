"""CPU: the plumbing of the deterministic mode (command line -> config -> set_random_seed -> model -> engine -> plan key), its
refusal of bf16 storage, the C ABI additions, and that the option's presence leaves the default plan builder alone."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

import yunet_amd
import yunet_amd._lib as L
import yunet_amd.engine as E
import yunet_amd.runner as R
from test_train_cli import CFG, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def reset_flag():
    yield
    R._DETERMINISTIC = False


def model(kind='n'):
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    return yunet_amd.build_detector(cfg.model), cfg


def test_cli_sets_config_key_and_seed_flag(tmp_path, monkeypatch):
    seen = {}

    def fake_train(m, ds, cfg, **kw):
        seen.update(cfg=cfg, wants=R.wants_deterministic(cfg), flag=R._DETERMINISTIC, draw=float(torch.rand(1)))
        return []
    monkeypatch.setattr(T.R, 'train_detector', fake_train)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda i: None)
    common = [CFG, '--seed', '7', '--no-validate', '--cfg-options', 'data.samples_per_gpu=4',
              'data.train.type=SyntheticWiderFace', 'data.train.img_scale=(160,160)', 'data.train.iters_per_epoch=2']
    T.main(common + ['--work-dir', str(tmp_path / 'a'), '--deterministic'])
    assert seen['cfg']['deterministic'] is True and seen['wants'] and seen['flag']
    det_draw = seen['draw']
    dumped = yunet_amd.Config.fromfile(str(tmp_path / 'a' / 'yunet_n.py'))
    assert dumped.deterministic is True
    R._DETERMINISTIC = False
    T.main(common + ['--work-dir', str(tmp_path / 'b')])
    assert 'deterministic' not in seen['cfg'] and not seen['wants'] and not seen['flag']
    assert seen['draw'] == det_draw                      # the same torch seed either way
    import argparse
    helps = {}
    monkeypatch.setattr(argparse.ArgumentParser, 'add_argument',
                        (lambda orig: lambda self, *a, **k: helps.__setitem__(a[0], k.get('help', '')) or orig(self, *a, **k))(
                            argparse.ArgumentParser.add_argument))
    T.parse_args([CFG])
    assert 'reproducible' in helps['--deterministic'] and 'compatibility' not in helps['--deterministic']


def test_set_random_seed_seeds_and_selects_the_mode():
    import random
    import numpy as np
    R.set_random_seed(11, deterministic=True)
    a = (random.random(), float(np.random.rand()), float(torch.rand(1)))
    assert R._DETERMINISTIC and R.wants_deterministic(yunet_amd.Config(dict()))
    R.set_random_seed(11)                  # (as in the reference, False does not switch a mode off)
    assert (random.random(), float(np.random.rand()), float(torch.rand(1))) == a
    assert R._DETERMINISTIC
    R._DETERMINISTIC = False
    R.set_random_seed(11)
    assert not R._DETERMINISTIC and not R.wants_deterministic(yunet_amd.Config(dict()))
    assert R.wants_deterministic(yunet_amd.Config(dict(deterministic=True)))
    assert list(inspect.signature(R.set_random_seed).parameters) == ['seed', 'deterministic']


class Stop(Exception):
    pass


def test_train_detector_turns_the_mode_on_for_its_model(monkeypatch):
    m, cfg = model()
    calls = []
    monkeypatch.setattr(type(m), 'to', lambda self, *a, **k: (_ for _ in ()).throw(Stop()))
    monkeypatch.setattr(type(m), 'set_deterministic', lambda self, flag=True: calls.append(flag))
    with pytest.raises(Stop):
        R.train_detector(m, None, cfg)
    assert calls == []                                    # default: untouched
    cfg['deterministic'] = True
    with pytest.raises(Stop):
        R.train_detector(m, None, cfg)
    assert calls == [True]
    del cfg['deterministic']
    R.set_random_seed(3, deterministic=True)
    with pytest.raises(Stop):
        R.train_detector(m, None, cfg)
    assert calls == [True, True]
    cfg['fp16'] = dict(loss_scale=512.)
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        R.train_detector(m, None, cfg)


def test_model_passes_the_mode_to_its_engine_and_plans_are_keyed_by_it(monkeypatch):
    m, _ = model()
    m.set_deterministic(True)
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)       # (bind_engine's logging buffer; no GPU here)
    eng = m.bind_engine('cpu')
    assert eng.deterministic is True
    built = []
    monkeypatch.setattr(E, 'Plan', lambda eng_, n, h, w, g: built.append(eng_.deterministic) or object())
    p_det = eng.get_plan(2, 64, 64, 1)
    m.set_deterministic(False)
    assert eng.deterministic is False
    p_def = eng.get_plan(2, 64, 64, 1)
    assert built == [True, False] and p_det is not p_def and len(eng.plans) == 2        # both plans coexist
    assert (2, 64, 64, 64, 'fp32') in eng.plans and (2, 64, 64, 64, 'fp32', 'det') in eng.plans
    m.set_deterministic(True)
    assert eng.get_plan(2, 64, 64, 1) is p_det and built == [True, False]


def test_bf16_with_deterministic_raises():
    m, _ = model()
    m.set_deterministic(True)
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        m.set_precision('bf16')
    m.set_deterministic(False)
    m.set_precision('bf16')
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        m.set_deterministic(True)
    eng = E.YuNetEngine(m.arch(), 'cpu')
    eng.set_deterministic(True)
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        eng.set_precision('bf16')
    eng.set_deterministic(False)
    eng.set_precision('bf16')
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        eng.set_deterministic(True)
    eng.deterministic = True                               # (set behind the setters' back: the plan builder checks too)
    with pytest.raises(NotImplementedError, match='fp32 storage'):
        E.Plan(eng, 2, 64, 64, 64)


def test_default_op_lists_are_the_recorded_ones(tmp_path):
    """tools/dbg/plan_dump.py builds the default plans of 300 configurations without a GPU and writes every field of every
    op with pointers as (buffer, offset).  tests/golden/plan_dump_default.sha256 is the digest of that dump at the commit
    before the deterministic option existed (its `reserved_` word spelled `det_rows`, the name it has now): the option's
    presence changes no op, no stride, no row count and no allocation order of the default mode."""
    import hashlib
    import sys
    out = tmp_path / 'plans.txt'
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tools', 'dbg', 'plan_dump.py'), str(out)],
                          stdout=subprocess.DEVNULL, cwd=ROOT)
    h = hashlib.sha256()
    with open(out, 'rb') as f:
        for chunk in iter(lambda: f.read(1 << 22), b''):
            h.update(chunk)
    assert h.hexdigest() == open(os.path.join(ROOT, 'tests', 'golden', 'plan_dump_default.sha256')).read().strip()


def test_deterministic_plan_differs_where_it_should():
    """The same builder with the option on, on the CPU: fold ops after every producer of sums and in front of every unit's
    backward, [1 + DET_ROWS] rows and det_rows in every descriptor, the stem op carrying the row count, no grouped launch;
    eval() without folds and with the stem on its plain scratch block."""
    import yunet_oracle as O
    eng = E.YuNetEngine(O.yunet_arch('n'), 'cpu')
    dflt = E.Plan(eng, 2, 64, 64, 64)
    eng.set_deterministic(True)
    det = E.Plan(eng, 2, 64, 64, 64)
    assert not dflt.det and det.det and E.DET_ROWS >= L.load().yunet_conv_blocks()
    assert not any(op.opcode == L.OP_BN_FOLD for lst in (dflt.fwd_a, dflt.fwd_b, dflt.bwd) for op in lst)
    n_bn = len(eng.layout.bn_names)
    for lst in (det.fwd_a, det.bwd):
        folds = [op for op in lst if op.opcode == L.OP_BN_FOLD]
        assert len(folds) == n_bn and all(op.i[0] == E.DET_ROWS for op in folds)
    assert det.stats.numel() == dflt.stats.numel() // E.BN_SLOTS * (1 + E.DET_ROWS)
    for i, op in enumerate(det.fwd_a):
        if op.opcode == L.OP_STEM_FWD:
            assert op.i[4] == E.DET_ROWS and det.fwd_a[i + 1].opcode == L.OP_BN_FOLD
        if op.opcode == L.OP_DP_FWD:
            assert op.i[L.OP_GROUP] == 0
            for bn in (op.dp.in_bn, op.dp.out_bn):
                assert (bn.slots, bn.det_rows) == (1, E.DET_ROWS) or not bn.stats
            if op.dp.out_has_bn:
                nxt = det.fwd_a[i + 1]
                assert nxt.opcode == L.OP_BN_FOLD and nxt.p[0] == op.dp.out_bn.stats
    for i, op in enumerate(det.bwd):
        if op.opcode == L.OP_DP_BWD and op.dp.out_has_bn:
            assert det.bwd[i - 1].opcode == L.OP_BN_FOLD and det.bwd[i - 1].p[0] == op.dp.out_bn.bstats
    assert all(r[6] == 1 for r in det.bn_table_f.tolist()) and all(r[6] == E.BN_SLOTS for r in dflt.bn_table_f.tolist())
    assert not any(op.opcode == L.OP_BN_FOLD for op in det.fwd_eval)
    stem = [op for op in det.fwd_eval if op.opcode == L.OP_STEM_FWD]
    assert len(stem) == 1 and stem[0].i[4] == 0 and stem[0].p[4] == det.eval_scratch.data_ptr()
    assert any(op.opcode == L.OP_DP_FWD and op.i[L.OP_GROUP] >= 2 for op in dflt.fwd_a)       # (the default groups the share convs)


def test_abi_additions_are_consistent(tmp_path):
    """Header, ctypes mirror and library: YunetBN keeps its layout with det_rows in the former padding word, the two new
    entry points and the new opcode are declared, bound and exported, the ABI version is unchanged."""
    hdr = open(os.path.join(ROOT, 'include', 'yunet_hip.h')).read()
    src = tmp_path / 'o.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yunet_hip.h"\n'
                   'int main(){printf("%zu %zu %zu %d %d\\n",sizeof(YunetBN),offsetof(YunetBN,slots),offsetof(YunetBN,det_rows),'
                   'YUNET_OP_BN_FOLD,YUNET_ABI_VERSION);return 0;}')
    exe = tmp_path / 'o'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(L.YunetBN), L.YunetBN.slots.offset, L.YunetBN.det_rows.offset, L.OP_BN_FOLD, 12]
    assert C.sizeof(L.YunetBN) == 48 and L.YunetBN.det_rows.offset == 44
    lib = L.load()
    for name in ('yunet_bn_fold', 'yunet_stem_fwd_det'):
        assert name in L.EXPORTED and hasattr(lib, name) and re.search(rf'\bint {name}\(', hdr)
    assert len(L._SIGNATURES['yunet_stem_fwd_det'][1]) == 11 and len(L._SIGNATURES['yunet_bn_fold'][1]) == 4
    assert L.YunetBN(None, None, None, None, 1, 1e-5).det_rows == 0
    # bad arguments are refused on the host, before any launch
    assert lib.yunet_bn_fold(None, 4, 16, None) == L.EINVAL and lib.yunet_bn_fold(C.c_void_p(8), 0, 16, None) == L.EINVAL
    assert lib.yunet_stem_fwd_det(None, None, None, None, None, 1024, 1, 32, 32, 16, None) == L.EINVAL
