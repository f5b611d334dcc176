"""-m gpu: the custom hooks on the device path -- yunet_ema_update against torch's own eager update bit for bit,
the EMA hooks in the full runner against an eager replay (tests/hooks_ref.py), checkpoints / eval / resume with
ema_* entries, and the box-size statistics hook against the restatement."""
import json
import os

import numpy as np
import pytest
import torch

import hooks_ref as H
import yunet_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


# --------------------------------------------------------------------------------------------- yunet_ema_update
MOMENTA = [1e-4, 0.5] + [H.momentum_fun('ExpMomentumEMAHook', 2e-4, total_iter=2000)(x) for x in (0, 777, 5000)]


def _special(n, g):
    e = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 8)
    vals = torch.tensor([0.0, -0.0, float('inf'), float('-inf'), float('nan'), 1e-45, -1e-45, 1e-38, 3e38, -3e38])
    k = min(n, vals.numel())
    idx = torch.randperm(n, generator=g)[:k]
    e[idx] = vals[:k]
    return e


@pytest.mark.parametrize('n', [1, 3, 255, 256, 257, 54608, 75856])
@pytest.mark.parametrize('offsets', [(0, 0), (1, 1), (1, 2), (3, 0)])
def test_ema_update_bit_identical_to_torch(n, offsets):
    import yunet_amd.kernels as K
    g = torch.Generator().manual_seed(n * 7 + offsets[0])
    so, eo = offsets
    src_base = _special(n + 4, g).to(DEV)
    ema_base = _special(n + 4, g).to(DEV)
    for m in MOMENTA:
        src, ema = src_base[so:so + n], ema_base[eo:eo + n].clone() if eo == 0 else ema_base.clone()[eo:eo + n]
        want = ema.clone()
        want.mul_(1 - m).add_(src, alpha=m)
        K.ema_update([(src, ema)], m)
        torch.cuda.synchronize()
        assert torch.equal(_bits(ema), _bits(want)), (n, offsets, m)


def test_ema_update_three_segments_one_call():
    import yunet_amd.kernels as K
    g = torch.Generator().manual_seed(3)
    pairs = [(torch.randn(n, generator=g).to(DEV)[1:], torch.randn(n, generator=g).to(DEV)[1:]) for n in (75857, 2001, 2001)]
    want = [e.clone().mul_(1 - 0.3).add_(s, alpha=0.3) for s, e in pairs]
    K.ema_update(pairs, 0.3)
    torch.cuda.synchronize()
    for (_, e), w in zip(pairs, want):
        assert torch.equal(_bits(e), _bits(w))


def test_ema_update_matches_cpu_fixture_within_2ulp():
    import yunet_amd.kernels as K
    z = np.load(os.path.join(GOLDEN, 'custom_hooks_reference.npz'))
    meta = json.load(open(os.path.join(GOLDEN, 'custom_hooks_reference.json')))
    sizes = [int(np.prod(s)) for s in meta['module_shapes']]
    isf = np.concatenate([np.full(s, 'num_batches_tracked' not in k) for k, s in zip(meta['module_keys'], sizes)])
    for name in ('exp_i1', 'lin_i1'):
        ema = torch.tensor(z['init'][isf], dtype=torch.float32, device=DEV)
        for it in range(z['sequence'].shape[0]):
            src = torch.tensor(z['sequence'][it][isf], dtype=torch.float32, device=DEV)
            K.ema_update([(src, ema)], float(z[f'{name}/momenta'][it]))
            keys = meta['ema'][name]['ema_keys']
            want = z[f'{name}/traj'][it][np.concatenate([np.full(s, not k.endswith('num_batches_tracked'))
                                                         for k, s in zip(keys, sizes)])].astype(np.float32)
            got = ema.cpu().numpy()
            ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            assert ulp.max() <= 2, (name, it, ulp.max())


# --------------------------------------------------------------------------------------------- full runner
class Recorder:
    """priority 45: after the optimizer (40), before the EMA hook (49): the live state after every step."""
    priority = 45

    def __init__(self):
        self.init, self.steps, self.epoch_ends = None, [], []

    def _state(self, runner):
        m = runner.model
        return {k: v.detach().clone() for k, v in m.state_dict().items() if not k.startswith('ema_')}

    def before_run(self, runner):
        self.init = self._state(runner)

    def after_train_iter(self, runner):
        self.steps.append(self._state(runner))

    def __getattr__(self, name):
        if name.startswith(('before_', 'after_')):
            return lambda runner: None
        raise AttributeError(name)


class EpochEnd(Recorder):
    """priority 80: the full state_dict after every epoch end (after the EMA swap and the checkpoint)."""

    def before_run(self, runner):
        pass

    def after_train_iter(self, runner):
        pass

    def after_train_epoch(self, runner):
        self.epoch_ends.append({k: v.detach().clone() for k, v in runner.model.state_dict().items()})


def _model(seed=5):
    import yunet_amd
    cfg = yunet_amd.Config.fromfile('configs/yunet_s.py')
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(O.init_state(O.yunet_arch('s'), seed=seed), strict=True)
    return m.to(DEV).train()


def _run(work_dir, hooks, epochs=3, iters=3, model=None, extra=(), checkpoint=True):
    from yunet_amd.optim import FusedSGD
    from yunet_amd.runner import EpochBasedRunner, SyntheticWiderFace
    m = model if model is not None else _model()
    opt = FusedSGD(m, lr=0.01, momentum=0.9, weight_decay=5e-4)
    r = EpochBasedRunner(m, opt, work_dir=str(work_dir), logger=lambda *a: None, max_epochs=epochs)
    r.register_training_hooks(None, dict(), dict(interval=1) if checkpoint else None, None, None, hooks)
    for h, p in extra:
        r.register_hook(h, p)
    src = SyntheticWiderFace(img_scale=(160, 160), samples_per_gpu=8, iters_per_epoch=iters)
    r.run([src], device=DEV)
    torch.cuda.synchronize()
    return r, m, opt


CASES = [dict(type='ExpMomentumEMAHook', momentum=0.3, interval=1, total_iter=4, priority=49),
         dict(type='LinearMomentumEMAHook', momentum=0.5, interval=2, warm_up=3, priority=49),
         dict(type='ExpMomentumEMAHook', momentum=0.3, interval=1, total_iter=4, skip_buffers=True, priority=49)]


@pytest.mark.parametrize('case', range(len(CASES)))
def test_runner_ema_equals_eager_replay(tmp_path, case):
    cfg = CASES[case]
    rec, ends = Recorder(), EpochEnd()
    r, m, _ = _run(tmp_path, [cfg], extra=[(rec, 45), (ends, 80)])
    assert m.engine.params.ema_data is not None
    skip = cfg.get('skip_buffers', False)
    keys = [k for k, _ in m.named_parameters()] if skip else list(rec.init)
    replay = H.EMAReplay({k: rec.init[k] for k in keys}, cfg['interval'], H.hook_momentum_fun(cfg))
    it = 0
    for e in range(3):
        live = None
        for _ in range(3):
            live = {k: v.clone() for k, v in rec.steps[it].items()}
            replay.step(it, live)
            it += 1
        replay.swap(live)                        # epoch end: what the checkpoint / eval see
        got = ends.epoch_ends[e]
        for k in rec.init:
            want_live = live[k]
            assert torch.equal(got[k], want_live), (e, k)
            if k in replay.ema:
                assert torch.equal(got[H.ema_name(k)], replay.ema[k]), (e, 'ema', k)
        replay.swap(live)                        # next epoch start
    # the model as the run leaves it: EMA swapped in
    final = m.state_dict()
    replay.swap(live)
    for k in keys:
        assert torch.equal(final[k], live[k]) and torch.equal(final[H.ema_name(k)], replay.ema[k]), k


@pytest.mark.parametrize('priority', [49, 50])
def test_epoch_checkpoint_keys_and_contents(tmp_path, priority):
    cfg = dict(CASES[0], priority=priority)
    rec = Recorder()
    r, m, _ = _run(tmp_path, [cfg], epochs=1, extra=[(rec, 45)])
    ck = torch.load(str(tmp_path / 'epoch_1.pth'), map_location='cpu', weights_only=False)['state_dict']
    base = list(rec.init)
    assert list(ck) == [H.ema_name(k) for k in base] + base
    replay = H.EMAReplay(rec.init, 1, H.hook_momentum_fun(cfg))
    live = None
    for it in range(3):
        live = {k: v.clone() for k, v in rec.steps[it].items()}
        replay.step(it, live)
    ema = replay.ema
    for k in base:
        reg, sav = (ema[k], live[k]) if priority == 49 else (live[k], ema[k])
        assert torch.equal(ck[k], reg.cpu()) and torch.equal(ck[H.ema_name(k)], sav.cpu()), k


def test_eval_after_swap_equals_fresh_model_with_ema_weights(tmp_path):
    import yunet_amd.synthetic as S
    from yunet_amd.runner import load_model_state
    r, m, _ = _run(tmp_path, [CASES[0]], epochs=1)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    img = S.make_batch(2, 160, 160, 77)['img'].to(DEV)
    metas = [dict(img_shape=(160, 160, 3), scale_factor=np.ones(4, np.float32))] * 2
    m.eval()
    a = m.simple_test(img, metas)
    fresh = _model(seed=11)
    with pytest.warns(UserWarning, match='ema_'):
        load_model_state(fresh, sd, strict=True)
    fresh.eval()
    b = fresh.simple_test(img, metas)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0])


def test_resume_through_hook_equals_uninterrupted(tmp_path):
    cfg = CASES[0]
    _, full, opt_full = _run(tmp_path / 'full', [cfg], epochs=3)
    _run(tmp_path / 'a', [cfg], epochs=2)
    ck = str(tmp_path / 'a' / 'epoch_2.pth')
    _, res, opt_res = _run(tmp_path / 'b', [dict(cfg, resume_from=ck)], epochs=3, model=_model(seed=99))
    a, b = full.state_dict(), res.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.allclose(a[k].double(), b[k].double(), rtol=1e-6, atol=1e-7), k
    sa, sb = opt_full.state_dict(), opt_res.state_dict()
    assert sa['steps'] == sb['steps']
    assert torch.allclose(sa['momentum_buffer'].double(), sb['momentum_buffer'].double(), rtol=1e-6, atol=1e-7)


def test_train_detector_loads_ema_checkpoint_without_hook(tmp_path):
    import yunet_amd
    from yunet_amd.runner import SyntheticWiderFace, train_detector
    _run(tmp_path / 'a', [CASES[0]], epochs=1)
    ck = str(tmp_path / 'a' / 'epoch_1.pth')
    for key in ('resume_from', 'load_from'):
        cfg = yunet_amd.Config.fromfile('configs/yunet_s.py')
        cfg['work_dir'] = str(tmp_path / key)
        cfg[key] = ck
        cfg['runner'] = dict(type='EpochBasedRunner', max_epochs=1 if key == 'load_from' else 2)
        cfg['log_config'] = None
        cfg['checkpoint_config'] = None
        with pytest.warns(UserWarning, match='ema_'):
            train_detector(_model(seed=3), SyntheticWiderFace(img_scale=(160, 160), samples_per_gpu=8,
                                                              iters_per_epoch=1), cfg, max_iters=None, log=lambda *a: None)


# --------------------------------------------------------------------------------------------- statistics hook
class BatchRecorder:
    def __init__(self):
        self.batches = []

    def before_train_iter(self, runner):
        gt = runner.data_batch['gt_bboxes']
        self.batches.append((runner.iter, H.padded_to_lists(gt.padded, gt.counts)))

    def __getattr__(self, name):
        if name.startswith(('before_', 'after_')):
            return lambda runner: None
        raise AttributeError(name)


def _check_stats(path, batches, batch_size):
    js = json.load(open(path))
    assert list(js) == ['datetime:', 'Batch_size', 'Total_sample', 'Noimg', 'Shapeless2', 'data']
    data, total, noimg = H.size_statistics(batches)
    assert js['Batch_size'] == batch_size and js['Total_sample'] == total and js['Noimg'] == noimg
    assert js['Shapeless2'] == 0
    assert list(js['data'].items()) == list(data.items())


@pytest.mark.parametrize('source', ['synthetic', 'device_pipeline'])
def test_statistics_hook_in_runner(tmp_path, source):
    from yunet_amd.optim import FusedSGD
    from yunet_amd.runner import EpochBasedRunner, SyntheticSourceImages, SyntheticWiderFace
    m = _model()
    opt = FusedSGD(m, lr=0.01, momentum=0.9, weight_decay=5e-4)
    r = EpochBasedRunner(m, opt, work_dir=str(tmp_path), logger=lambda *a: None, max_epochs=3)
    r.register_training_hooks(None, dict(), None, None, None,
                              [dict(type='YuNetSampleSizeStatisticsHook', out_file='sizes.json', save_interval=3)])
    rec = BatchRecorder()
    r.register_hook(rec, 10)
    if source == 'synthetic':
        src = SyntheticWiderFace(img_scale=(160, 160), samples_per_gpu=8, iters_per_epoch=2)
    else:
        pipe = [dict(type='LoadImageFromFile', to_float32=True),
                dict(type='LoadAnnotations', with_bbox=True, with_keypoints=True),
                dict(type='RandomSquareCrop', crop_choice=[0.5, 0.7, 0.9, 1.1, 1.3, 1.5]),
                dict(type='Resize', img_scale=(160, 160), keep_ratio=False),
                dict(type='RandomFlip', flip_ratio=0.5),
                dict(type='Normalize', mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False),
                dict(type='DefaultFormatBundle'),
                dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_bboxes_ignore', 'gt_keypointss'])]
        src = SyntheticSourceImages(pipe, samples_per_gpu=8, iters_per_epoch=2, pool=8)
    r.run([src], device=DEV)
    # dumped at the start of epoch index 2: the batches of epochs 0 and 1
    _check_stats(str(tmp_path / 'sizes.json'), [b for b in rec.batches if b[0] < 4], 8)


def test_statistics_hook_hand_built_batches_with_empty_images_and_spill(tmp_path):
    from yunet_amd.hooks import YuNetSampleSizeStatisticsHook
    from yunet_amd.synthetic import GTList
    z = np.load(os.path.join(GOLDEN, 'custom_hooks_reference.npz'))
    meta = json.load(open(os.path.join(GOLDEN, 'custom_hooks_reference.json')))

    class R:
        work_dir, iter, epoch = str(tmp_path), 0, 0

    hook = YuNetSampleSizeStatisticsHook('s.json', save_interval=1)
    hook.before_run(R)
    batches = []
    for i in range(len(meta['stats']['iterations'])):
        n, boxes = z[f'stats/batch{i}/n'], torch.from_numpy(z[f'stats/batch{i}/boxes'])
        lists = list(torch.split(boxes, n.tolist()))
        gt = GTList([b.to(DEV) for b in lists])
        gmax = 8
        gt.padded = torch.zeros(len(lists), gmax, 4)
        for j, b in enumerate(lists):
            gt.padded[j, :len(b)] = b
        gt.padded, gt.counts = gt.padded.to(DEV), torch.tensor(n, dtype=torch.int32, device=DEV)
        R.iter = i
        R.data_batch = dict(img=torch.zeros(len(lists), 3, 64, 64, device=DEV), gt_bboxes=gt)
        hook.before_train_iter(R)
        batches.append((i, lists))
    assert int(hook._dev['totals'][3]) & 1, 'the negative-width box takes the spill path'
    hook.before_epoch(R)
    _check_stats(str(tmp_path / 's.json'), batches, len(lists))
    js = json.load(open(str(tmp_path / 's.json')))
    js.pop('datetime:')
    assert js == meta['stats']['json']


def test_widerface_tool_same_output_from_ema_checkpoint(tmp_path):
    """tools/test_widerface.py (strict load) on an EMA checkpoint gives the same predictions and APs as on the same
    checkpoint with its ema_* entries removed."""
    import subprocess
    import sys
    from PIL import Image
    import detect_oracle as D
    import wider_fixture as WF
    events, _ = WF.synth_events(7, n_events=2, imgs_per_event=2)
    rng = np.random.default_rng(0)
    lines = []
    for ev in events:
        os.makedirs(tmp_path / 'images' / ev['name'], exist_ok=True)
        for im in ev['images']:
            h, w = int(rng.integers(200, 420)), int(rng.integers(260, 520))
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(
                tmp_path / 'images' / ev['name'] / (im['name'] + '.jpg'))
            lines.append(f"# {ev['name']}/{im['name']}.jpg {w} {h}")
            for b in im['boxes']:
                lines.append('%d %d %d %d' % (b[0], b[1], b[0] + b[2], b[1] + b[3]))
    os.makedirs(tmp_path / 'labelv2' / 'val', exist_ok=True)
    (tmp_path / 'labelv2' / 'val' / 'labelv2.txt').write_text('\n'.join(lines) + '\n')
    WF.write_mats(events, str(tmp_path / 'labelv2' / 'val' / 'gt'))
    _, sd = D.make_state('n', 5, size=160)
    ema = {H.ema_name(k): (v * 0.5 if v.dtype.is_floating_point else v) for k, v in sd.items()}
    torch.save(dict(state_dict=sd, meta={}), tmp_path / 'plain.pth')
    torch.save(dict(state_dict=dict(ema, **sd), meta={}), tmp_path / 'ema.pth')
    cfg = open('configs/yunet_n.py').read() + f"""
data = dict(samples_per_gpu=1, test=dict(type='RetinaFaceDataset',
            ann_file={str(tmp_path / 'labelv2' / 'val' / 'labelv2.txt')!r},
            img_prefix={str(tmp_path / 'images')!r}, pipeline=[]))
"""
    (tmp_path / 'cfg.py').write_text(cfg)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for name in ('plain', 'ema'):
        out = tmp_path / f'out_{name}'
        r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'test_widerface.py'), str(tmp_path / 'cfg.py'),
                            str(tmp_path / f'{name}.pth'), '--out', str(out), '--save-preds', '--mode', '320',
                            '--thr', '0.3'], capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-1500:]
        files = {}
        for dirpath, _, fnames in os.walk(out):
            for f in fnames:
                p = os.path.join(dirpath, f)
                files[os.path.relpath(p, out)] = open(p, 'rb').read()
        outs[name] = files
        if name == 'ema':
            assert 'ema_* entries skipped' in r.stderr
    assert outs['plain'].keys() == outs['ema'].keys() and 'aps' in outs['plain']
    assert outs['plain'] == outs['ema']
