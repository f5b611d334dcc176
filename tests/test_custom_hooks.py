"""The reference's custom hooks (ExpMomentumEMAHook, LinearMomentumEMAHook, YuNetSampleSizeStatisticsHook,
CheckInvalidLossHook) on the CPU: config plumbing and hook order, the restatement (tests/hooks_ref.py) and the hooks'
host paths against the fixture made by the unmodified reference hooks (tools/make_golden_custom_hooks.py), the C
entry points' argument checks, checkpoints with ema_* entries, and a static assembly guard over the new kernels."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import hooks_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


def _fixture():
    z = np.load(os.path.join(GOLDEN, 'custom_hooks_reference.npz'))
    meta = json.load(open(os.path.join(GOLDEN, 'custom_hooks_reference.json')))
    return z, meta


def _tiny():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv2d(2, 3, 1), nn.BatchNorm2d(3), nn.Conv2d(3, 2, 1))


def _flat(sd, keys):
    return np.concatenate([sd[k].detach().double().reshape(-1).numpy() for k in keys])


def _unflat(vec, keys, shapes, like):
    out, o = {}, 0
    for k, s in zip(keys, shapes):
        n = int(np.prod(s))
        out[k] = torch.tensor(vec[o:o + n]).reshape(s).to(like[k].dtype)
        o += n
    return out


class FakeRunner:
    def __init__(self, model=None, work_dir=None):
        self.model, self.work_dir = model, work_dir
        self.iter = self.epoch = 0
        self.data_batch = self.outputs = None
        self.logged = []

    def logger(self, msg):
        self.logged.append(msg)


# --------------------------------------------------------------------------------------------- config plumbing
def _runner(custom, checkpoint=True):
    from yunet_amd.runner import EpochBasedRunner, EvalHook
    r = EpochBasedRunner(_tiny(), torch.optim.SGD(_tiny().parameters(), lr=0.1), logger=lambda *a: None, max_epochs=1)
    r.register_training_hooks(None, dict(), dict(interval=1) if checkpoint else None, dict(interval=1), None, custom)
    r.register_hook(EvalHook(dataset=None), 'LOW')
    return [type(h).__name__ for h in r.hooks]


def test_custom_hooks_build_from_config():
    names = _runner([dict(type='ExpMomentumEMAHook', momentum=1e-4, priority=49),
                     dict(type='LinearMomentumEMAHook', momentum=1e-4, warm_up=10),
                     dict(type='YuNetSampleSizeStatisticsHook', out_file='s.json'),
                     dict(type='CheckInvalidLossHook', interval=10)])
    for n in ('ExpMomentumEMAHook', 'LinearMomentumEMAHook', 'YuNetSampleSizeStatisticsHook', 'CheckInvalidLossHook'):
        assert n in names


@pytest.mark.parametrize('priority,before_ckpt', [(49, True), (50, False), ('NORMAL', False), ('ABOVE_NORMAL', True),
                                                  (70, False)])
def test_ema_hook_order_against_checkpoint_and_eval(priority, before_ckpt):
    """mmcv's rule: a lower priority value runs first; equal priorities keep registration order (the config's
    checkpoint hook is registered before the custom hooks, EvalHook after them)."""
    names = _runner([dict(type='ExpMomentumEMAHook', momentum=1e-4, priority=priority)])
    e, c, v = names.index('ExpMomentumEMAHook'), names.index('CheckpointHook'), names.index('EvalHook')
    assert (e < c) == before_ckpt
    assert e < v
    assert names.index('OptimizerHook') < e


def test_unknown_custom_hook_still_raises_keyerror():
    with pytest.raises(KeyError):
        _runner([dict(type='SyncRandomSizeHook')])


def test_momentum_must_lie_in_open_unit_interval():
    from yunet_amd.hooks import ExpMomentumEMAHook, LinearMomentumEMAHook
    for bad in (0, 1, -0.1, 1.5):
        with pytest.raises(AssertionError):
            ExpMomentumEMAHook(momentum=bad)
        with pytest.raises(AssertionError):
            LinearMomentumEMAHook(momentum=bad)


# --------------------------------------------------------------------------------------------- EMA vs the fixture
def _replay_config(z, meta, name, impl):
    """Drive the tiny module through the fixture's state sequence; impl 'ref' = tests/hooks_ref.py, 'hook' = the
    package's hook on a fake runner.  Returns (EMA trajectory, epoch-end states, key order)."""
    from yunet_amd import hooks as HK
    cfg = meta['ema'][name]
    kw = dict(cfg['kwargs'])
    model = _tiny()
    init = model.state_dict()
    keys0, shapes = meta['module_keys'], meta['module_shapes']
    assert np.array_equal(_flat(init, keys0), z['init'])
    seq = [_unflat(v, keys0, shapes, init) for v in z['sequence']]
    runner = FakeRunner(model)
    traj, ends = [], []
    if impl == 'hook':
        hook = getattr(HK, cfg['type'])(**kw)
        hook.before_run(runner)
    else:
        skip = kw.pop('skip_buffers', False)
        entries = dict(model.named_parameters()) if skip else model.state_dict()
        mf = H.momentum_fun(cfg['type'], **kw)
        replay = H.EMAReplay(entries, kw.get('interval', 1), mf)
        for k, v in replay.ema.items():
            model.register_buffer(H.ema_name(k), v)        # the replay's state is the model's ema_ buffers
    keys = list(model.state_dict())
    ema_keys = [k for k in keys if k.startswith('ema_')]
    for _ in range(meta['epochs']):
        if impl == 'hook':
            hook.before_train_epoch(runner)
        elif runner.epoch > 0:
            replay.swap(model.state_dict())
        for _ in range(meta['iters']):
            with torch.no_grad():
                for k, v in seq[runner.iter].items():
                    model.state_dict()[k].copy_(v)
            if impl == 'hook':
                hook.after_train_iter(runner)
            else:
                with torch.no_grad():
                    replay.step(runner.iter, model.state_dict())
            traj.append(_flat(model.state_dict(), ema_keys))
            runner.iter += 1
        if impl == 'hook':
            hook.after_train_epoch(runner)
        else:
            replay.swap(model.state_dict())
        ends.append(_flat(model.state_dict(), keys))
        runner.epoch += 1
    return np.stack(traj), np.stack(ends), keys


@pytest.mark.parametrize('impl', ['ref', 'hook'])
@pytest.mark.parametrize('name', ['exp_i1', 'exp_i2', 'exp_i1_skip', 'lin_i1', 'lin_i2', 'lin_i2_skip'])
def test_ema_reproduces_reference_fixture(name, impl):
    z, meta = _fixture()
    traj, ends, keys = _replay_config(z, meta, name, impl)
    assert keys == meta['ema'][name]['keys']
    assert np.array_equal(traj, z[f'{name}/traj'])
    assert np.array_equal(ends, z[f'{name}/epoch_end'])


def test_momentum_schedules_match_fixture():
    z, meta = _fixture()
    for name, cfg in meta['ema'].items():
        kw = {k: v for k, v in cfg['kwargs'].items() if k != 'skip_buffers'}
        mf = H.momentum_fun(cfg['type'], **kw)
        assert [mf(i) for i in range(len(z[f'{name}/momenta']))] == z[f'{name}/momenta'].tolist()


def test_ema_coefficients_are_fp32_of_the_double_values():
    import yunet_amd.kernels as K
    for m in (1e-4, 0.3, 2e-4 + (1 - 2e-4) * np.exp(-1 / 2000)):
        keep, mm = K.ema_coefficients(m)
        assert keep == float(np.float32(1.0 - m)) and mm == float(np.float32(m))


# --------------------------------------------------------------------------------------------- statistics
def _stat_batches(z, meta):
    out = []
    for i in meta['stats']['iterations']:
        n, boxes = z[f'stats/batch{i}/n'], torch.from_numpy(z[f'stats/batch{i}/boxes'])
        out.append((i, list(torch.split(boxes, n.tolist()))))
    return out


def test_size_statistics_restatement_reproduces_fixture():
    z, meta = _fixture()
    data, total, noimg = H.size_statistics(_stat_batches(z, meta))
    js = meta['stats']['json']
    assert list(data.items()) == list(js['data'].items())
    assert total == js['Total_sample'] and noimg == js['Noimg']


def test_statistics_hook_host_path_reproduces_fixture(tmp_path):
    from yunet_amd.hooks import YuNetSampleSizeStatisticsHook
    z, meta = _fixture()
    runner = FakeRunner(work_dir=str(tmp_path))
    hook = YuNetSampleSizeStatisticsHook('sizes.json', save_interval=2)
    hook.before_run(runner)
    for it, lists in _stat_batches(z, meta):
        runner.iter = it
        runner.data_batch = dict(gt_bboxes=lists)
        hook.before_train_iter(runner)
    runner.epoch = 0
    hook.before_epoch(runner)
    assert not os.path.exists(tmp_path / 'sizes.json')          # (epoch + 1) % save_interval != 0
    runner.epoch = 1
    hook.before_epoch(runner)
    js = json.load(open(tmp_path / 'sizes.json'))
    assert list(js) == ['datetime:', 'Batch_size', 'Total_sample', 'Noimg', 'Shapeless2', 'data']
    js.pop('datetime:')
    assert js == meta['stats']['json']
    assert list(js['data']) == list(meta['stats']['json']['data'])


# --------------------------------------------------------------------------------------------- loss check
class _Lazy:
    def __init__(self, v):
        self.v, self.resolved = v, False

    def __float__(self):
        self.resolved = True
        return self.v


def test_check_invalid_loss_hook_matches_fixture():
    from yunet_amd.hooks import CheckInvalidLossHook
    _, meta = _fixture()
    ck = meta['checkloss']
    hook = CheckInvalidLossHook(interval=ck['interval'])
    runner = FakeRunner()
    for it, v, result in ck['results']:
        v = float(v)
        lazy = _Lazy(v)
        runner.iter = it
        runner.outputs = dict(loss=torch.tensor(v), log_vars=dict(loss=lazy))
        if result == 'assert':
            with pytest.raises(AssertionError):
                hook.after_train_iter(runner)
            assert runner.logged[-1] == 'loss become infinite or NaN!'
        else:
            hook.after_train_iter(runner)
        assert lazy.resolved == ((it + 1) % ck['interval'] == 0)     # resolved only on checked iterations


# --------------------------------------------------------------------------------------------- C ABI
def test_library_exports_hook_entry_points():
    import yunet_amd._lib as L
    lib = L.load()
    assert hasattr(lib, 'yunet_ema_update') and hasattr(lib, 'yunet_box_size_hist')
    assert lib.yunet_abi_version() == 12


def test_ema_update_rejects_bad_arguments_without_launching():
    import ctypes as C
    import yunet_amd._lib as L
    lib = L.load()
    P, N = C.c_void_p, C.c_longlong
    good = (P * 1)(0x1000)

    def call(src, ema, n, k):
        return lib.yunet_ema_update(src, ema, n, k, C.c_float(0.5), C.c_float(0.5), None)
    assert call(None, good, (N * 1)(4), 1) == L.EINVAL
    assert call(good, None, (N * 1)(4), 1) == L.EINVAL
    assert call(good, good, None, 1) == L.EINVAL
    assert call(good, good, (N * 1)(-1), 1) == L.EINVAL                       # negative size
    assert call((P * 1)(None), good, (N * 1)(4), 1) == L.EINVAL              # null segment pointer
    assert call((P * 1)(0x1002), good, (N * 1)(4), 1) == L.EINVAL            # not 4-byte aligned
    four = (P * 4)(0x1000, 0x1000, 0x1000, 0x1000)
    assert call(four, four, (N * 4)(4, 4, 4, 4), 4) == L.EINVAL              # more segments than supported
    assert call(good, good, (N * 1)(4), 0) == L.EINVAL
    assert call((P * 1)(None), (P * 1)(None), (N * 1)(0), 1) == 0            # empty: nothing to launch


def test_box_size_hist_rejects_bad_arguments_without_launching():
    import ctypes as C
    import yunet_amd._lib as L
    lib = L.load()
    p = C.c_void_p(0x1000)

    def call(boxes=p, counts=p, N=2, G=4, it=0, W=8, H=8, bc=p, bf=p, tot=p, spill=p, cap=4):
        return lib.yunet_box_size_hist(boxes, counts, N, G, it, W, H, bc, bf, tot, spill, cap, None)
    for kw in (dict(boxes=None), dict(counts=None), dict(bc=None), dict(bf=None), dict(tot=None),
               dict(N=-1), dict(G=0), dict(N=1 << 16, G=1 << 15), dict(W=-1), dict(H=70000), dict(it=-1),
               dict(it=1 << 31), dict(cap=-1), dict(spill=None, cap=1)):
        assert call(**kw) == L.EINVAL, kw
    assert call(N=0) == 0                                                      # empty batch: nothing to launch


# --------------------------------------------------------------------------------------------- checkpoints
def _ema_checkpoint(model):
    sd = dict(model.state_dict())
    ema = {H.ema_name(k): v.clone() + 1 for k, v in sd.items()}
    return dict(ema, **sd)


def test_load_model_state_tolerates_ema_entries_only():
    from yunet_amd.runner import load_model_state
    src, dst = _tiny(), nn.Sequential(nn.Conv2d(2, 3, 1), nn.BatchNorm2d(3), nn.Conv2d(3, 2, 1))
    sd = _ema_checkpoint(src)
    with pytest.warns(UserWarning, match=r'9 unexpected and 0 missing ema_\*'):
        load_model_state(dst, sd, strict=True)
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v)
    # the other direction: a model with ema_ buffers, a checkpoint without them
    for k, v in src.state_dict().items():
        dst.register_buffer(H.ema_name(k), torch.zeros_like(v))
    with pytest.warns(UserWarning, match=r'0 unexpected and 9 missing ema_\*'):
        load_model_state(dst, src.state_dict(), strict=True)
    # anything else stays strict
    bad = dict(sd, extra_key=torch.zeros(1))
    with pytest.raises(RuntimeError):
        load_model_state(_tiny(), bad, strict=True)
    short = {k: v for k, v in sd.items() if k != '0.weight'}
    with pytest.raises(RuntimeError):
        load_model_state(_tiny(), short, strict=True)
    plain = nn.Sequential(nn.Conv2d(2, 3, 1), nn.BatchNorm2d(3), nn.Conv2d(3, 2, 1))
    with pytest.raises(RuntimeError):
        plain.load_state_dict(bad, strict=True)


def _yunet_n():
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    return yunet_amd.build_detector(cfg.model)


def test_runner_load_checkpoint_accepts_ema_checkpoint(tmp_path):
    from yunet_amd.runner import load_checkpoint
    m = _yunet_n()
    path = str(tmp_path / 'ema.pth')
    torch.save(dict(meta=dict(epoch=1, iter=3), state_dict=_ema_checkpoint(m)), path)
    m2 = _yunet_n()
    with pytest.warns(UserWarning, match='ema_'):
        meta = load_checkpoint(m2, path)
    assert meta['iter'] == 3
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v)


@pytest.mark.parametrize('tool,args,out', [('yunet2cpp.py', [], 'model.cpp'),
                                           ('yunet2onnx.py', ['--shape', '160', '160'], 'model.onnx')])
def test_export_tools_ignore_ema_entries(tmp_path, tool, args, out):
    m = _yunet_n()
    sd = dict(m.state_dict())
    plain, ema = str(tmp_path / 'plain.pth'), str(tmp_path / 'ema.pth')
    torch.save(dict(state_dict=sd), plain)
    torch.save(dict(state_dict=_ema_checkpoint(m)), ema)
    outs = []
    for ck in (plain, ema):
        d = tmp_path / os.path.basename(ck)[:-4]
        d.mkdir()
        cmd = [sys.executable, os.path.join(ROOT, 'tools', tool), os.path.join(ROOT, 'configs', 'yunet_n.py'), ck]
        r = subprocess.run(cmd + args + _out_flag(tool, str(d / out)), capture_output=True, text=True, timeout=600,
                           cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(open(d / out, 'rb').read())
    assert outs[0] == outs[1]


def _out_flag(tool, path):
    return ['--output-file', path]


# --------------------------------------------------------------------------------------------- assembly guard
ALLOWED_SCALAR = {'load', 'mov', 'movk', 'add', 'addc', 'sub', 'subb', 'mul', 'lshl', 'lshr', 'ashr', 'and', 'or',
                  'xor', 'andn2', 'orn2', 'not', 'cmp', 'cselect', 'cbranch', 'branch', 'waitcnt', 'endpgm', 'nop',
                  'bcnt1', 'ff1', 'min', 'max', 'abs', 'bfe', 'lshl1', 'lshl2', 'lshl3', 'lshl4', 'setpc', 'getpc',
                  'sext', 'cvt', 'and_saveexec', 'or_saveexec', 'andn2_saveexec', 'xor_saveexec', 'setprio', 'barrier',
                  'mul_hi', 'brev', 'flbit', 'bitset0', 'bitset1', 'cmpk', 'addk', 'mulk', 'sleep', 'sethalt', 'trap'}


def _hooks_asm(tmp):
    out = os.path.join(tmp, 'hooks.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-w', '-S', '--cuda-device-only',
                    '-o', out, os.path.join(ROOT, 'libfacedetection.train_amd', 'csrc', 'hooks.hip')],
                   check=True, capture_output=True, timeout=600)
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r'^(_Z\w+):.*?\n(.*?)^\s+s_endpgm', text, re.S | re.M):
        kernels[m.group(1)] = re.findall(r'^\s+([a-z][a-z0-9_]*)', m.group(2), re.M)
    return kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
def test_hook_kernels_assembly_guard(tmp_path):
    kernels = _hooks_asm(str(tmp_path))
    ema = [v for k, v in kernels.items() if 'ema_update_kernel' in k]
    hist = [v for k, v in kernels.items() if 'box_size_hist_kernel' in k]
    assert len(ema) == 1 and len(hist) == 1
    for ins in ema + hist:
        for op in ins:
            if op.startswith('s_'):
                fam = op[2:].split('_')[0]
                assert fam in ALLOWED_SCALAR or op[2:].rsplit('_', 1)[0] in ALLOWED_SCALAR, op
                if fam in ('load', 'buffer'):
                    assert op.startswith(('s_load_', 's_buffer_load_')), op
            assert not op.startswith(('scratch_', 'buffer_')), op                 # no spills, no buffer access
    ema, hist = ema[0], hist[0]
    assert 'global_store_dwordx4' in ema and 'global_load_dwordx4' in ema         # 16-byte body
    assert any(op.startswith(('v_fma_f32', 'v_pk_fma_f32', 'v_fmac_f32', 'v_fmamk_f32', 'v_fmaak_f32')) for op in ema)
    assert not any(op.startswith(('v_add_f32', 'v_pk_add_f32')) for op in ema)    # the add is fused, never separate
    assert 'global_atomic_umin_x2' in hist and 'global_atomic_add_x2' in hist     # 64-bit integer atomics only
    assert not any(op.startswith('global_atomic') and ('f32' in op or 'f64' in op) for op in hist)


def test_yunet_strict_load_skips_ema_entries_only():
    """What tools/test_widerface.py, tools/yunet2cpp.py and tools/yunet2onnx.py do: YuNet.load_state_dict(strict=True)
    on an EMA checkpoint loads the regular entries with a warning; any other mismatch still fails."""
    m = _yunet_n()
    sd = _ema_checkpoint(m)
    m2 = _yunet_n()
    with pytest.warns(UserWarning, match=r'YuNet.load_state_dict: \d+ unexpected and 0 missing ema_\*'):
        m2.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v)
    with pytest.raises(RuntimeError, match='extra_key'):
        _yunet_n().load_state_dict(dict(sd, extra_key=torch.zeros(1)), strict=True)
    with pytest.raises(RuntimeError, match='Missing key'):
        _yunet_n().load_state_dict({k: v for k, v in sd.items() if k != 'backbone.model0.conv1.weight'}, strict=True)
