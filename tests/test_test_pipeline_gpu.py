"""-m gpu: the batched device test pipeline (csrc/test_pipeline.hip, yunet_amd.test_pipeline) against the per-image
path that exists without it -- imresize.resize_linear_u8 (pinned to oracle/cv2_resize_oracle.py by
tests/test_cv2_resize.py), evaluation.prepare_test_image, YuNet_Head.get_bboxes_flat.  Every comparison is bit
equality: the kernel does the integer arithmetic of the former and the fp32 division of the latter."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAINED = os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth')

# (h, w, nw, nh): keep-ratio geometries of the modes, the same-size and the exact-2x special cases, an up-scale, odd
# one-pixel sizes, and the shapes of tests/test_zz_resize_gpu.py
CASES = [(480, 640, 640, 480), (640, 480, 480, 640), (641, 333, 333, 641), (500, 500, 640, 640), (1385, 1024, 473, 640),
         (768, 1024, 1650, 1238), (64, 96, 48, 32), (640, 640, 320, 320), (31, 33, 33, 31), (17, 400, 640, 27),
         (45, 70, 64, 41), (333, 500, 213, 320), (7, 5, 5, 7), (300, 420, 320, 229), (1, 9, 320, 36), (9, 1, 36, 320),
         (200, 300, 150, 100), (201, 300, 150, 100)]


def pack(imgs):
    sizes = np.array([im.size for im in imgs], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(DEV)
    hw = np.array([im.shape[:2] for im in imgs], dtype=np.int32)
    return src, off, hw


def build_model(sd=None):
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    model = yunet_amd.build_detector(cfg.model)
    if sd is None:
        sd = torch.load(TRAINED, map_location='cpu', weights_only=False)['state_dict']
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval()


def face_images(n, seed, crops=None):
    """uint8 BGR HWC images with painted faces (the fixture the trained weights saw), optionally cropped."""
    import yunet_amd.synthetic as S
    b = S.make_batch(n, 320, 320, seed, structured=True)
    out = []
    for i in range(n):
        arr = np.ascontiguousarray(b['img'][i].permute(1, 2, 0).clamp(0, 255).byte().numpy())
        if crops is not None:
            h, w = crops[i % len(crops)]
            arr = np.ascontiguousarray(arr[:h, :w])
        out.append(arr)
    return out, b


def write_set(tmp_path, imgs, boxes=None, sub='img', ext='png'):
    """A labelv2 list + image files (lossless) -> test-mode RetinaFaceDataset."""
    from PIL import Image
    import yunet_amd
    os.makedirs(tmp_path / sub, exist_ok=True)
    lines = []
    for i, im in enumerate(imgs):
        Image.fromarray(im[:, :, ::-1].copy()).save(tmp_path / sub / f'{i}.{ext}')
        lines.append(f'# {i}.{ext} {im.shape[1]} {im.shape[0]}')
        for box in ([] if boxes is None else boxes[i]):
            lines.append('%.2f %.2f %.2f %.2f' % tuple(float(v) for v in box))
    (tmp_path / f'{sub}.txt').write_text('\n'.join(lines) + '\n')
    return yunet_amd.build_dataset(dict(type='RetinaFaceDataset', ann_file=str(tmp_path / f'{sub}.txt'),
                                        img_prefix=str(tmp_path / sub), test_mode=True))


# ------------------------------------------------------------------------------ 5. the kernel vs the existing resize
@pytest.mark.parametrize('flip', [0, 1])
def test_kernel_equals_resize_linear_u8_in_a_mixed_batch(flip):
    from yunet_amd import imresize as R
    from yunet_amd import test_pipeline as TP
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w, _, _ in CASES]
    src, off, hw = pack(imgs)
    table = np.array([[nh, nw, flip, 0] for _, _, nw, nh in CASES], dtype=np.int32)
    Hc = (max(c[3] for c in CASES) + 31) // 32 * 32
    Wc = (max(c[2] for c in CASES) + 31) // 32 * 32
    out = torch.full((len(CASES), 3, Hc, Wc), float('nan'), device=DEV)
    TP.launch_pixels(src, off, hw, table, out)
    torch.cuda.synchronize()
    got = out.cpu()
    for i, (h, w, nw, nh) in enumerate(CASES):
        want = R.resize_linear_u8(torch.from_numpy(imgs[i]), (nw, nh)).permute(2, 0, 1).float()
        if flip:
            want = torch.flip(want, dims=[2])
        assert torch.equal(got[i, :, :nh, :nw], want), (i, CASES[i], int((got[i, :, :nh, :nw] != want).sum()))
        rest = got[i].clone()
        rest[:, :nh, :nw] = 0.0
        assert torch.equal(rest, torch.zeros_like(rest)), (i, CASES[i])          # exactly 0.0 (not NaN) outside the corner


def test_kernel_entry_refuses_bad_sizes_without_a_launch():
    from yunet_amd import _lib as L
    from yunet_amd import test_pipeline as TP
    img = np.zeros((8, 8, 3), np.uint8)
    src, off, hw = pack([img])
    table = np.array([[8, 8, 0, 0]], dtype=np.int32)
    for shape in ((1, 3, 32, 30), (1, 3, 1, L.AUG_MAX_EDGE + 32)):
        with pytest.raises(L.YunetHipError, match='yunet_test_pixels'):
            TP.launch_pixels(src, off, hw, table, torch.empty(shape, device=DEV))
    # a table that names a corner larger than the canvas, or an empty one, stays inside the canvas / writes zeros
    out = torch.full((2, 3, 32, 32), float('nan'), device=DEV)
    src2, off2, hw2 = pack([img, img])
    TP.launch_pixels(src2, off2, hw2, np.array([[64, 64, 0, 0], [0, -3, 1, 0]], dtype=np.int32), out)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.equal(out[1], torch.zeros_like(out[1]))


# --------------------------------------------------------------------------- 6. the pipeline vs the per-image path
@pytest.mark.parametrize('mode', [(640, 640), (320, 320), None, (1100, 1650)])
@pytest.mark.parametrize('cache', [None, 'device'])
def test_pipeline_at_batch_one_equals_prepare_test_image(tmp_path, mode, cache):
    from yunet_amd import evaluation as E
    from yunet_amd import test_pipeline as TP
    rng = np.random.default_rng(5)
    sizes = [(200, 300), (419, 260), (320, 320), (640, 640), (333, 517), (64, 48), (700, 500)]
    if mode == (320, 320):
        sizes.append((640, 640))          # exactly 2 x down
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    ds = write_set(tmp_path, imgs)
    pipe = TP.DeviceTestPipeline(None, scale=mode)
    source = TP.TestSource(ds, cache=cache, device=DEV)
    for i in range(len(ds)):
        assert np.array_equal(ds.load_image(i), imgs[i])
        want, wm = E.prepare_test_image(ds.load_image(i), mode, DEV)
        got, gm = pipe(source.fetch([i]), 0, [ds.data_infos[i]['filename']])
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want), (i, sizes[i], mode)
        assert len(gm) == 1
        for k, v in wm.items():
            assert k in gm[0], k
            if isinstance(v, np.ndarray):
                assert gm[0][k].dtype == v.dtype and np.array_equal(gm[0][k], v), k
            else:
                assert gm[0][k] == v, k
        assert gm[0]['ori_filename'] == ds.data_infos[i]['filename']
    # a batch: each image's corner is its B = 1 tensor's, the rest of the canvas is 0
    img, metas = pipe(source.fetch(list(range(len(ds)))), 0)
    assert img.shape[2] % 32 == 0 and img.shape[3] % 32 == 0
    for i in range(len(ds)):
        one, _ = E.prepare_test_image(imgs[i], mode, DEV)
        ph, pw = one.shape[2:]
        assert torch.equal(img[i, :, :ph, :pw], one[0])
        assert float(img[i, :, ph:].abs().sum()) == 0.0 and float(img[i, :, :, pw:].abs().sum()) == 0.0


# -------------------------------------------------------------------------------------- 7. batched detections
def parent_simple_test(model, x, metas):
    """YuNet.simple_test as it stands without the batched tail: per image get_bboxes_flat's own torch ops."""
    eng = model._ensure_engine(x.device)
    flat = eng.forward_eval(x.float().contiguous())
    res, lmk = model.bbox_head.get_bboxes_flat(flat, eng.plan.sizes, metas, rescale=True)
    return [d.cpu().numpy() for d, _ in res], [k.cpu().numpy() for k in lmk]


def test_batched_detections_equal_the_per_image_tail(tmp_path):
    from yunet_amd import evaluation as E
    from yunet_amd import test_pipeline as TP
    crops = [(320, 320), (300, 320), (320, 272), (256, 256), (320, 320), (288, 200)]
    imgs, _ = face_images(6, 31, crops)
    ds = write_set(tmp_path, imgs)
    model = build_model()
    inner = [dict(type='Resize', keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.0),
             dict(type='Normalize', mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False),
             dict(type='Pad', size=(320, 320), pad_val=0), dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img'])]
    pipe = TP.DeviceTestPipeline([dict(type='LoadImageFromFile'),
                                  dict(type='MultiScaleFlipAug', img_scale=(320, 320), flip=False, transforms=inner)])
    prepared = [E.prepare_test_image(im, (320, 320), DEV) for im in imgs]
    assert all(tuple(x.shape) == (1, 3, 320, 320) for x, _ in prepared)
    stack = torch.cat([x for x, _ in prepared]).contiguous()
    want_d, want_k = parent_simple_test(model, stack, [m for _, m in prepared])
    img, metas = pipe(TP.TestSource(ds, cache='device', device=DEV).fetch(list(range(6))), 0)
    assert torch.equal(img, stack)
    got, got_k = model.simple_test(img, metas, rescale=True, with_landmarks=True)
    for i in range(6):
        print('image', i, 'detections', want_d[i].shape[0])
        assert want_d[i].shape[0] >= 1, f'image {i}: the fixture must give detections'
        assert got[i][0].dtype == np.float32 and got[i][0].shape == want_d[i].shape
        assert np.array_equal(got[i][0], want_d[i]) and np.array_equal(got_k[i], want_k[i]), i
    assert any(m['scale_factor'][0] != 1.0 for m in metas), 'the rescale must be a real division for some image'
    # rescale=False: the same rows without the division
    eng = model._ensure_engine(img.device)
    flat = eng.forward_eval(stack)
    res, lmk = model.bbox_head.get_bboxes_flat(flat, eng.plan.sizes, [m for _, m in prepared], rescale=False)
    want_raw, want_raw_k = [d.cpu().numpy() for d, _ in res], [k.cpu().numpy() for k in lmk]
    raw, raw_k = model.simple_test(img, metas, rescale=False, with_landmarks=True)
    for i in range(6):
        assert np.array_equal(raw[i][0], want_raw[i]) and np.array_equal(raw_k[i], want_raw_k[i]), i
    assert any(not np.array_equal(raw[i][0], got[i][0]) for i in range(6))


# ------------------------------------------------------------------------------------------------ 8. consumers
def test_single_gpu_test_batched_from_a_device_store(tmp_path):
    from yunet_amd import evaluation as E
    imgs, _ = face_images(10, 7, [(320, 320), (280, 320), (320, 250), (200, 200)])
    ds = write_set(tmp_path, imgs)
    calls = []
    load = ds.load_image
    ds.load_image = lambda i: (calls.append(i), load(i))[1]
    model = build_model()
    # the default arguments: the per-image path, value for value
    base = E.single_gpu_test(model, ds, DEV, (320, 320))
    assert sorted(calls) == list(range(10))
    for i in range(10):
        x, m = E.prepare_test_image(imgs[i], (320, 320), DEV)
        want, _ = parent_simple_test(model, x, [m])
        assert len(base[i]) == 1 and np.array_equal(base[i][0], want[0]), i
    del calls[:]
    said = []
    one = E.single_gpu_test(model, ds, DEV, (320, 320), samples_per_gpu=4, cache='device', log=said.append)
    assert len(one) == 10 and sorted(calls) == list(range(10)) and not said
    # equal geometry (every image padded to 320 x 320) -> the batch rows are the per-image results, in dataset order
    for i in range(10):
        assert one[i][0].shape[1] == 5
    stack = torch.cat([E.prepare_test_image(im, (320, 320), DEV)[0] for im in imgs[:4]])
    want, _ = parent_simple_test(model, stack, [E.prepare_test_image(im, (320, 320), 'cpu')[1] for im in imgs[:4]])
    for i in range(4):
        assert np.array_equal(one[i][0], want[i]), i
    del calls[:]
    two = E.single_gpu_test(model, ds, DEV, (320, 320), samples_per_gpu=4, cache='device')
    assert calls == [], 'the second run decodes nothing'
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(one, two))
    # the device store is sized to the images that are evaluated, not to the dataset; no decode thread outlives a run
    from yunet_amd import test_pipeline as TP
    src = TP.source_for(ds, 'device', DEV)
    assert len(src.store) == 10 and src._pool is None
    small = write_set(tmp_path, imgs, sub='small')
    part = E.single_gpu_test(model, small, DEV, (320, 320), max_images=5, samples_per_gpu=4, cache='device')
    held = TP.source_for(small, 'device', DEV)
    assert len(held.store) == 5 and all(np.array_equal(a[0], b[0]) for a, b in zip(one, part))
    TP.release_sources(small)
    assert held.store is None and not small._test_sources
    # max_images, a short last batch, and no cache (decode-ahead + one packed upload per batch): same values
    three = E.single_gpu_test(model, ds, DEV, (320, 320), max_images=7, samples_per_gpu=4)
    assert len(three) == 7 and all(np.array_equal(a[0], b[0]) for a, b in zip(one, three))
    assert model.training is False


def test_multi_view_list_goes_through_aug_test(tmp_path):
    from yunet_amd import evaluation as E
    from yunet_amd import test_pipeline as TP
    imgs, _ = face_images(2, 3)
    ds = write_set(tmp_path, imgs)
    model = build_model()
    lst = [dict(type='MultiScaleFlipAug', img_scale=[(320, 320), (160, 160)], flip=True,
                transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                            dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img'])])]
    res = E.single_gpu_test(model, ds, DEV, pipeline=lst)
    pipe = TP.DeviceTestPipeline(lst)
    src = TP.TestSource(ds, device=DEV)
    for i in range(2):
        views = [pipe(src.fetch([i]), v) for v in range(4)]
        assert torch.equal(views[1][0], torch.flip(views[0][0], dims=[3]))        # 320 x 320: the corner is the canvas
        want = model.aug_test([v[0] for v in views], [v[1] for v in views], rescale=True)
        assert np.array_equal(res[i][0], want[0][0]) and res[i][0].shape[0] >= 1


def test_widerface_tool_batched(tmp_path):
    from PIL import Image
    import wider_fixture as WF
    import detect_oracle as D
    events, _ = WF.synth_events(7, n_events=2, imgs_per_event=3)
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
    arch, sd = D.make_state('n', 5, size=160)
    torch.save(dict(state_dict=sd, meta={}), tmp_path / 'ck.pth')
    aps, files, out_dirs, errs = {}, {}, {}, {}
    # tools/test_widerface.py stays the per-image tool (data.test.samples_per_gpu is accepted there and changes nothing);
    # tools/widerface_batched.py reads it and runs the batched device pipeline
    for tool, spg in (('test_widerface.py', 1), ('test_widerface.py', 4), ('widerface_batched.py', 1),
                      ('widerface_batched.py', 4)):
        cfg = open(os.path.join(ROOT, 'configs', 'yunet_n.py')).read() + f"""
data = dict(samples_per_gpu=1, test=dict(type='RetinaFaceDataset', samples_per_gpu={spg},
            ann_file={str(tmp_path / 'labelv2' / 'val' / 'labelv2.txt')!r},
            img_prefix={str(tmp_path / 'images')!r}, pipeline=[]))
"""
        (tmp_path / f'cfg{spg}.py').write_text(cfg)
        out = tmp_path / f'out_{tool[:-3]}_{spg}'
        extra = ['--cache', 'device'] if (tool, spg) == ('widerface_batched.py', 4) else []
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', tool), str(tmp_path / f'cfg{spg}.py'),
                            str(tmp_path / 'ck.pth'), '--out', str(out), '--save-preds', '--mode', '320', '--thr', '0.3']
                           + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-1500:]
        aps[tool, spg] = [float(v) for v in open(out / 'aps').read().strip().split(',')]
        files[tool, spg] = sum(len(os.listdir(out / e['name'])) for e in events)
        out_dirs[tool, spg] = out
        errs[tool, spg] = r.stderr
    print('APs per image', aps['test_widerface.py', 1], 'batched', aps['widerface_batched.py', 4])
    assert all(v == 6 for v in files.values()), files
    assert 'reached the dataset unread' in errs['test_widerface.py', 4]         # the per-image tool says so, loudly
    assert 'reached the dataset unread' not in errs['widerface_batched.py', 4]
    for key, v in aps.items():
        assert len(v) == 3 and all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in v), (key, v)
    # one image per batch has the per-image path's geometry: the prediction files are the same text
    for e in events:
        for fn in sorted(os.listdir(out_dirs['test_widerface.py', 1] / e['name'])):
            assert (out_dirs['widerface_batched.py', 1] / e['name'] / fn).read_text() == \
                (out_dirs['test_widerface.py', 1] / e['name'] / fn).read_text(), fn


def test_eval_hook_batched(tmp_path):
    import yunet_amd
    import yunet_amd.runner as R
    import yunet_amd.synthetic as S
    sd = torch.load(TRAINED, map_location='cpu', weights_only=False)['state_dict']
    imgs, b = face_images(6, 31)
    ds = write_set(tmp_path, imgs, boxes=b['gt_bboxes'])
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    cfg.merge_from_dict(dict(
        data=dict(samples_per_gpu=8, val_dataloader=dict(samples_per_gpu=4),
                  val=dict(type='RetinaFaceDataset', ann_file=ds.ann_file, img_prefix=ds.img_prefix, cache='device',
                           pipeline=[dict(type='MultiScaleFlipAug', img_scale=(320, 320), flip=False, transforms=[])])),
        evaluation=dict(interval=1, metric='mAP'), runner=dict(type='EpochBasedRunner', max_epochs=2),
        checkpoint_config=None, work_dir=str(tmp_path / 'work'),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')])))
    cfg.optimizer['lr'] = 1e-5
    model = yunet_amd.build_detector(cfg.model)
    model.load_state_dict(sd, strict=True)
    src = R.SyntheticWiderFace((160, 160), 8, iters_per_epoch=2)
    lines_out = []
    hist = R.train_detector(model, src, cfg, validate=True, device='cuda', log=lines_out.append)
    val = [h for h in hist if h.get('mode') == 'val']
    assert [v['epoch'] for v in val] == [1, 2] and all(0.0 <= v['mAP'] <= 1.0 for v in val) and val[0]['mAP'] > 0.2, val
    assert any(l.startswith('Epoch(val) [1][6]') for l in lines_out)
    assert model.training
