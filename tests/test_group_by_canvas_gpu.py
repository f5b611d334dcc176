"""-m gpu: evaluation batched by padded canvas (grouped_eval.run_test(..., group_by='canvas')) against the per-image path
(samples_per_gpu=1).  A grouped batch's canvas is each image's own pad_shape, so every comparison is bit equality, in
dataset order.  The set: 11 tiny images of the painted-face generator on the canvases 64 x 96 (5 images), 96 x 64 (5)
and 64 x 64 (1), interleaved; B = 2 gives the five geometries (2 | 1, 64, 96), (2 | 1, 96, 64), (1, 64, 64)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from yunet_amd import grouped_eval as GE
from test_test_pipeline_gpu import DEV, ROOT, TRAINED, build_model, face_images, write_set

pytestmark = pytest.mark.gpu

SIZES = [(50, 90), (90, 50), (64, 96), (33, 40), (70, 60), (60, 70), (96, 64), (40, 90), (80, 33), (64, 65), (65, 64)]
CANVAS = [((h + 31) // 32 * 32, (w + 31) // 32 * 32) for h, w in SIZES]
SEED = 11
INNER = [dict(type='Resize', keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.0),
         dict(type='Normalize', mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False),
         dict(type='Pad', size_divisor=32, pad_val=0), dict(type='ImageToTensor', keys=['img']),
         dict(type='Collect', keys=['img'])]
ORIGIN = [dict(type='LoadImageFromFile'), dict(type='MultiScaleFlipAug', scale_factor=1.0, flip=False, transforms=INNER)]


def origin_pipe():
    from yunet_amd import test_pipeline as TP
    return TP.DeviceTestPipeline(ORIGIN)


class Landmarks:
    """Keeps the landmarks of every image a run detects: simple_test(with_landmarks=True) behind the model's forward."""

    def __init__(self, model):
        self.model, self.kps, self.calls = model, [], 0

    def __enter__(self):
        def forward(return_loss=False, rescale=True, img=None, img_metas=None):
            assert len(img) == 1
            self.calls += 1
            res, kps = self.model.simple_test(img[0], img_metas[0], rescale=rescale, with_landmarks=True)
            self.kps.append((([m['ori_filename'] for m in img_metas[0]]), kps))
            return res
        self.model.forward = forward
        return self

    def __exit__(self, *exc):
        del self.model.forward

    def by_name(self):
        return {name: k for names, kps in self.kps for name, k in zip(names, kps)}


def run(model, ds, samples_per_gpu, cache=None, indices=None, **kw):
    """run_test over the whole set -> (dets per image, landmarks per image, forwards, log lines), dataset order."""
    from yunet_amd import test_pipeline as TP
    said = []
    indices = list(range(len(ds))) if indices is None else indices
    with torch.no_grad(), Landmarks(model) as seen:
        out = GE.run_test(model, ds, DEV, indices, origin_pipe(), TP.source_for(ds, cache, DEV), samples_per_gpu,
                          log=said.append, **kw)
    kps = seen.by_name()
    return out, [kps[ds.data_infos[i]['filename']] for i in indices], seen.calls, said


def same(a, b):
    """Two runs' boxes+scores and landmarks, image by image."""
    assert len(a[0]) == len(b[0]) == len(a[1]) == len(b[1])
    for i, (x, y, kx, ky) in enumerate(zip(a[0], b[0], a[1], b[1])):
        assert len(x) == len(y) == 1 and x[0].dtype == y[0].dtype == np.float32 and x[0].shape == y[0].shape, i
        assert np.array_equal(x[0], y[0]) and np.array_equal(kx, ky), (i, SIZES[i])


@pytest.fixture(scope='module')
def fixture(tmp_path_factory):
    """The model, the set and the per-image result (samples_per_gpu=1), computed once and left unchanged."""
    imgs, b = face_images(len(SIZES), SEED, SIZES)
    assert [im.shape[:2] for im in imgs] == SIZES
    ds = write_set(tmp_path_factory.mktemp('canvas'), imgs)
    model = build_model()
    base = run(model, ds, 1)
    assert base[2] == len(SIZES) and not base[3]
    n = [r[0].shape[0] for r in base[0]]
    print('detections per image', n)
    assert sum(1 for v in n if v >= 1) >= 6, f'the fixture must give detections: {n}'
    assert all(k.shape[0] == v for k, v in zip(base[1], n))
    return types.SimpleNamespace(model=model, ds=ds, base=base, imgs=imgs, gt=b['gt_bboxes'])


# 1 ------------------------------------------------------------------------------------------------------------
def test_grouped_equals_the_per_image_path_in_dataset_order(fixture):
    got = run(fixture.model, fixture.ds, 2, group_by='canvas')
    assert not got[3], 'the grouped mode logs no fallback'
    same(got, fixture.base)
    # a list that is not the dataset's order comes back in its own order
    order = [7, 2, 10, 0, 3, 9, 1]
    part = run(fixture.model, fixture.ds, 2, indices=order, group_by='canvas')
    same(part, ([fixture.base[0][i] for i in order], [fixture.base[1][i] for i in order]))


# 2 ------------------------------------------------------------------------------------------------------------
def test_grouped_is_the_protocol_and_consecutive_batches_are_the_collate(fixture):
    from yunet_amd import test_pipeline as TP
    pipe = origin_pipe()
    consecutive = run(fixture.model, fixture.ds, 2)
    assert not consecutive[3] and consecutive[2] == 6, 'consecutive batches of 2 must fit the plan cache here'
    mixed = [i for b in TP.batches_of(range(len(SIZES)), 2) for i in b if pipe.canvas([SIZES[k] for k in b]) != CANVAS[i]]
    assert len(mixed) >= 4
    differ = [i for i in mixed if not (consecutive[0][i][0].shape == fixture.base[0][i][0].shape and
                                       np.array_equal(consecutive[0][i][0], fixture.base[0][i][0]))]
    print('images in a mixed batch', mixed, 'whose detections differ from the per-image ones', differ)
    assert differ, 'a zero border around a smaller image must change some detection'
    grouped = run(fixture.model, fixture.ds, 2, group_by='canvas')
    same(grouped, fixture.base)


# 3 ------------------------------------------------------------------------------------------------------------
def test_grouped_runs_fewer_forwards(fixture):
    from yunet_amd import test_pipeline as TP
    hw = {i: s for i, s in enumerate(SIZES)}
    planned = GE.plan_batches(origin_pipe(), hw, list(range(len(SIZES))), 2, group_by='canvas')
    assert len(planned) == 7 and len({(len(b),) + CANVAS[b[0]] for b in planned}) == 5
    calls = []
    forward = fixture.model.forward
    fixture.model.forward = lambda *a, **k: (calls.append(len(k['img_metas'][0])), forward(*a, **k))[1]
    try:
        with torch.no_grad():
            out = GE.run_test(fixture.model, fixture.ds, DEV, list(range(len(SIZES))), origin_pipe(),
                              TP.source_for(fixture.ds, None, DEV), 2, group_by='canvas')
    finally:
        del fixture.model.forward
    assert calls == [len(b) for b in planned] and len(calls) < len(SIZES)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(out, fixture.base[0]))


# 4 ------------------------------------------------------------------------------------------------------------
def test_grouped_with_more_geometries_than_plans(fixture, monkeypatch):
    import yunet_amd.engine as EN
    monkeypatch.setattr(EN, 'MAX_PLANS', 2)
    model = build_model()                       # an engine without plans: each of the 5 geometries is built here
    got = run(model, fixture.ds, 2, group_by='canvas')
    assert not got[3]
    same(got, fixture.base)
    shapes = sorted(key[:3] for key in model.engine.plans)
    print('plans held', shapes)
    assert 1 <= len(shapes) <= 2


# 5 ------------------------------------------------------------------------------------------------------------
def test_pixel_cap_sends_every_image_alone(fixture):
    got = run(fixture.model, fixture.ds, 2, group_by='canvas', max_batch_pixels=64 * 96)
    assert got[2] == len(SIZES)
    same(got, fixture.base)


# 6 ------------------------------------------------------------------------------------------------------------
def test_grouped_from_a_device_store_decodes_once(fixture):
    from yunet_amd import evaluation as E
    from yunet_amd import test_pipeline as TP
    ds = fixture.ds
    calls = []
    load = ds.load_image
    ds.load_image = lambda i: (calls.append(i), load(i))[1]
    try:
        how = dict(samples_per_gpu=2, pipeline=ORIGIN, cache='device', group_by='canvas')
        one = E.single_gpu_test(fixture.model, ds, DEV, None, **how)
        assert sorted(calls) == list(range(len(SIZES)))
        del calls[:]
        two = E.single_gpu_test(fixture.model, ds, DEV, None, **how)
        assert calls == [], 'the second evaluation decodes nothing'
    finally:
        del ds.load_image
        TP.release_sources(ds)
    for i in range(len(SIZES)):
        assert np.array_equal(one[i][0], fixture.base[0][i][0]) and np.array_equal(two[i][0], fixture.base[0][i][0]), i


# 7 ------------------------------------------------------------------------------------------------------------
def test_widerface_tool_grouped(tmp_path):
    from PIL import Image
    import wider_fixture as WF
    import detect_oracle as D
    events, _ = WF.synth_events(7, n_events=2, imgs_per_event=3)
    rng = np.random.default_rng(0)
    sizes = iter([(50, 90), (90, 50), (64, 96), (33, 40), (40, 70), (96, 64)])
    lines = []
    for ev in events:
        os.makedirs(tmp_path / 'images' / ev['name'], exist_ok=True)
        for im in ev['images']:
            h, w = next(sizes)
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(
                tmp_path / 'images' / ev['name'] / (im['name'] + '.jpg'))
            lines.append(f"# {ev['name']}/{im['name']}.jpg {w} {h}")
            for b in im['boxes']:
                lines.append('%d %d %d %d' % (b[0], b[1], b[0] + b[2], b[1] + b[3]))
    os.makedirs(tmp_path / 'labelv2' / 'val', exist_ok=True)
    (tmp_path / 'labelv2' / 'val' / 'labelv2.txt').write_text('\n'.join(lines) + '\n')
    WF.write_mats(events, str(tmp_path / 'labelv2' / 'val' / 'gt'))
    arch, sd = D.make_state('n', 5, size=160)
    torch.save(dict(state_dict=sd, meta={}), tmp_path / 'ck.pth')
    aps, outs, said = {}, {}, {}
    # per image | --group canvas on the command line | data.test.group_by in the config
    for name, spg, extra_cfg, extra in (('one', 1, '', []), ('flag', 2, '', ['--group', 'canvas', '--cache', 'device']),
                                        ('config', 2, ", group_by='canvas'", ['--max-batch-pixels', str(2 * 64 * 96)])):
        cfg = open(os.path.join(ROOT, 'configs', 'yunet_n.py')).read() + f"""
data = dict(samples_per_gpu=1, test=dict(type='RetinaFaceDataset', samples_per_gpu={spg}{extra_cfg},
            ann_file={str(tmp_path / 'labelv2' / 'val' / 'labelv2.txt')!r},
            img_prefix={str(tmp_path / 'images')!r}, pipeline=[]))
"""
        (tmp_path / f'cfg_{name}.py').write_text(cfg)
        outs[name] = tmp_path / f'out_{name}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'widerface_batched.py'), str(tmp_path / f'cfg_{name}.py'),
                            str(tmp_path / 'ck.pth'), '--out', str(outs[name]), '--save-preds', '--mode', '2', '--thr', '0.3']
                           + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-1500:]
        aps[name] = [ln for ln in r.stdout.splitlines() if ln.startswith('APS:')]
        said[name] = r.stdout
    print(aps)
    assert len(aps['one']) == 1 and aps['flag'] == aps['one'] and aps['config'] == aps['one']
    assert all('batch geometries' not in s for s in said.values())
    rows = 0
    for name in ('flag', 'config'):
        assert (outs[name] / 'aps').read_text() == (outs['one'] / 'aps').read_text()
        for e in events:
            files = sorted(os.listdir(outs['one'] / e['name']))
            assert len(files) == 3 and sorted(os.listdir(outs[name] / e['name'])) == files
            for fn in files:
                text = (outs['one'] / e['name'] / fn).read_text()
                assert (outs[name] / e['name'] / fn).read_text() == text, (name, fn)
                rows += int(text.splitlines()[1])
    assert rows > 0, 'the prediction files must hold detections'


# 8 ------------------------------------------------------------------------------------------------------------
def test_eval_hook_grouped(fixture, tmp_path):
    import yunet_amd
    import yunet_amd.runner as R
    boxes = []
    for (h, w), g in zip(SIZES, fixture.gt):
        g = g.numpy()
        boxes.append(g[(g[:, 2] <= w) & (g[:, 3] <= h)])
    assert sum(len(g) for g in boxes) >= 1
    ds = write_set(tmp_path, fixture.imgs, boxes=boxes)
    sd = torch.load(TRAINED, map_location='cpu', weights_only=False)['state_dict']

    def config(loader):
        cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
        cfg.merge_from_dict(dict(
            data=dict(samples_per_gpu=8, val_dataloader=loader,
                      val=dict(type='RetinaFaceDataset', ann_file=ds.ann_file, img_prefix=ds.img_prefix, pipeline=ORIGIN)),
            evaluation=dict(interval=1, metric='mAP'), runner=dict(type='EpochBasedRunner', max_epochs=1),
            checkpoint_config=None, work_dir=str(tmp_path / 'work'),
            log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')])))
        cfg.optimizer['lr'] = 1e-5
        return cfg

    with pytest.raises(ValueError, match='group_by'):           # a bad value raises when the hook is made
        R.train_detector(yunet_amd.build_detector(config(dict()).model), R.SyntheticWiderFace((160, 160), 8, iters_per_epoch=1),
                         config(dict(samples_per_gpu=2, group_by='rows')), validate=True, device='cuda', log=lambda s: None)
    cfg = config(dict(samples_per_gpu=2, group_by='canvas'))
    model = yunet_amd.build_detector(cfg.model)
    model.load_state_dict(sd, strict=True)
    said = []
    hist = R.train_detector(model, R.SyntheticWiderFace((160, 160), 8, iters_per_epoch=1), cfg, validate=True,
                            device='cuda', log=said.append)
    val = [h for h in hist if h.get('mode') == 'val']
    logged = [s for s in said if s.startswith('Epoch(val) [1][11]')]
    assert len(val) == 1 and len(logged) == 1 and not any('batch geometries' in s for s in said), said
    # the same model (nothing trains after the last firing) through a hook at samples_per_gpu=1
    lines = []
    stub = types.SimpleNamespace(model=model, device='cuda', rank=0, logger=lines.append, log_buffer=[], epoch=0, iter=1)
    one = R.EvalHook(ds, samples_per_gpu=1, pipeline=ORIGIN)
    assert one.group_by is None
    one._evaluate(stub)
    print(logged, lines)
    assert lines == logged and one.results[0]['mAP'] == val[0]['mAP'] and val[0]['mAP'] > 0.0
    assert model.training
