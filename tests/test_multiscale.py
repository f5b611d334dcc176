"""CPU: multi-scale training, Resize(multiscale_mode='square_range') -- the numpy restatement (tests/multiscale_ref.py)
against the fixture made by the unmodified reference classes (tools/make_golden_multiscale.py) and against the live
reference where its tree is available; the config surface of Resize / DevicePipeline; YuNetTextLoggerHook; the
plan-cache guard; the new C entry points in the header and the ctypes table."""
import importlib.util
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import multiscale_ref as M
import pipeline_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_PIPELINE = [
    dict(type='LoadImageFromFile', to_float32=True),
    dict(type='LoadAnnotations', with_bbox=True, with_keypoints=True),
    dict(type='RandomSquareCrop', crop_choice=[0.5, 0.7, 0.9, 1.1, 1.3, 1.5]),
    dict(type='Resize', img_scale=(320, 640), multiscale_mode='square_range', keep_ratio=False),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_bboxes_ignore', 'gt_keypointss']),
]


def ms_pipeline(**resize):
    cfg = [dict(p) for p in REF_PIPELINE]
    cfg[3] = dict(type='Resize', **resize)
    return cfg


# ------------------------------------------------------------------ restatement vs fixture / live reference
@pytest.mark.parametrize('name', M.SETS)
def test_restatement_matches_reference_fixture(name):
    g, seed, it, lo, hi, srcs = M.load_case(name)
    assert len(srcs) >= 8
    sizes = []
    for i, (img, boxes, kps) in enumerate(srcs):
        r = M.augment_image(img, boxes, kps, seed, it, i, lo, hi, g['crop_choice'])
        cw, flip, draws, kept, S = [int(v) for v in g[f'meta_{i}']]
        assert (int(r['params'][2]), int(r['params'][3]), r['draws'], int(r['mask'].sum()), r['S']) == \
            (cw, flip, draws, kept, S), f'decision differs from the reference (image {i})'
        assert np.array_equal(r['boxes'], g[f'boxes_{i}']), f'boxes differ (image {i})'
        assert np.array_equal(r['kps'], g[f'kps_{i}']), f'keypoints differ (image {i})'
        dig, corner, center = M.image_digest(r['img'])
        assert np.array_equal(corner, g[f'img_corner_{i}']) and np.array_equal(center, g[f'img_center_{i}'])
        assert np.array_equal(dig, g[f'img_digest_{i}'])
        sizes.append(S)
    assert len(set(sizes)) >= 3 and min(sizes) < max(sizes), 'the fixture must mix sizes'
    assert set(sizes) <= set(M.out_sizes(lo, hi))


def _tool():
    spec = importlib.util.spec_from_file_location('make_golden_multiscale',
                                                  os.path.join(ROOT, 'tools', 'make_golden_multiscale.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('seed,iteration,lo,hi', [(41, 0, 160, 320), (42, 7, 320, 640), (43, 999, 300, 500),
                                                  (44, 3, 320, 320), (45, 1, 33, 100)])
def test_restatement_matches_live_reference(seed, iteration, lo, hi):
    """Random sources through the UNMODIFIED reference transforms (draws redirected to the counter-based generator) and
    through the restatement: S_n, window, flip, number of draws, boxes, keypoints and the whole image identical."""
    import ref_stub
    if not ref_stub.available():
        pytest.skip('reference tree not present')
    MG = _tool()
    T = MG.load_transforms()
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.integers(40, 500)), int(rng.integers(40, 600)), int(rng.choice([1, 2, 5, 17, 40, -1, -3])))
              for _ in range(8)]
    imgs, boxes, kps = zip(*[P.synth_image(rng, h, w, g) for h, w, g in shapes])
    ref = MG.run_reference(T, imgs, boxes, kps, seed, iteration, lo, hi)
    for i, r in enumerate(ref):
        o = M.augment_image(imgs[i], boxes[i], kps[i], seed, iteration, i, lo, hi, np.array(M.CROP_CHOICE, np.float64))
        assert (o['S'], int(o['params'][2]), bool(o['params'][3]), o['draws']) == \
            (r['S'], int(r['cw']), r['flip'], r['draws']), (i, shapes[i])
        assert np.array_equal(o['boxes'], r['boxes']) and np.array_equal(o['kps'], r['kps']), (i, shapes[i])
        assert np.array_equal(o['img'], r['img']), (i, shapes[i])


def test_extra_draw_sits_between_crop_and_flip():
    """The square_range stream is the fixed-size stream with one draw inserted before the flip's: same window, and the
    flip decided by the NEXT counter; an image without GT makes exactly that one draw."""
    rng = np.random.default_rng(5)
    img, boxes, kps = P.synth_image(rng, 200, 260, 6)
    for it in range(20):
        fixed = P.augment_image(img, boxes, kps, 9, it, 0, 320, M.CROP_CHOICE)
        ms = M.augment_image(img, boxes, kps, 9, it, 0, 160, 320, M.CROP_CHOICE)
        assert np.array_equal(fixed['params'][:3], ms['params'][:3])
        st = P.Stream(9, it, 0)
        st.ctr = ms['draws'] - 2
        assert ms['S'] == st.randint(160, 321) // 32 * 32
        assert bool(ms['params'][3]) == (st.uniform() < 0.5)
    empty = M.augment_image(img, boxes[:0], kps[:0], 9, 0, 0, 160, 320, M.CROP_CHOICE)
    assert empty['status'] == 1 and empty['draws'] == 1 and empty['S'] == P.Stream(9, 0, 0).randint(160, 321) // 32 * 32


def test_collate_canvas_pads_bottom_right_with_zero():
    res = [dict(S=64, img=np.full((3, 64, 64), 128.0, np.float32)), dict(S=32, img=np.full((3, 32, 32), 7.0, np.float32))]
    out = M.collate_canvas(res)
    assert out.shape == (2, 3, 64, 64) and (out[0] == 128.0).all()
    assert (out[1, :, :32, :32] == 7.0).all()
    out[1, :, :32, :32] = 0
    assert not out[1].any()


# ------------------------------------------------------------------ config surface
def test_square_range_builds_and_lists_its_sizes():
    from yunet_amd.pipelines import DevicePipeline
    pipe = DevicePipeline(REF_PIPELINE, seed=0)
    assert pipe.scale_range == (320, 640) and pipe.out_size is None
    assert pipe.out_sizes == [320, 352, 384, 416, 448, 480, 512, 544, 576, 608, 640] == M.out_sizes(320, 640)
    pipe = DevicePipeline(ms_pipeline(img_scale=(500, 300), multiscale_mode='square_range', keep_ratio=False))
    assert pipe.scale_range == (300, 500) and pipe.out_sizes == [288, 320, 352, 384, 416, 448, 480]
    pipe = DevicePipeline(ms_pipeline(img_scale=[(320, 320)], multiscale_mode='square_range', keep_ratio=False))
    assert pipe.scale_range == (320, 320) and pipe.out_sizes == [320]       # degenerate: still makes the draw
    assert 'square_range' in repr(pipe.steps[3])


def test_fixed_size_config_is_untouched():
    import yunet_amd
    from yunet_amd.pipelines import DevicePipeline
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_s.py'))
    pipe = DevicePipeline(cfg.train_pipeline, seed=1)
    assert pipe.out_size == 320 and pipe.out_sizes == [320] and pipe.scale_range is None
    pipe.check_plan_cache(max_plans=1)
    # mmdet's default multiscale_mode='range' with one square scale is the fixed size, no draw
    pipe = DevicePipeline(ms_pipeline(img_scale=(640, 640), multiscale_mode='range', keep_ratio=False))
    assert pipe.out_size == 640 and pipe.scale_range is None


@pytest.mark.parametrize('resize,exc,match', [
    (dict(img_scale=(31, 320), multiscale_mode='square_range', keep_ratio=False), ValueError, 'rounds down'),
    (dict(img_scale=(16, 20), multiscale_mode='square_range', keep_ratio=False), ValueError, 'rounds down'),
    (dict(img_scale=(320, 640), multiscale_mode='square_range', keep_ratio=True), NotImplementedError, 'keep_ratio=False'),
    (dict(img_scale=(320, 640), multiscale_mode='square_range'), NotImplementedError, 'keep_ratio=False'),
    (dict(img_scale=[(320, 320), (640, 640)], multiscale_mode='square_range', keep_ratio=False), ValueError,
     'one img_scale'),
    (dict(img_scale=[(320, 320), (640, 640)], multiscale_mode='range', keep_ratio=False), NotImplementedError, "'range'"),
    (dict(img_scale=[(320, 320), (640, 640)], multiscale_mode='value', keep_ratio=False), NotImplementedError, "'value'"),
    (dict(img_scale=(320, 640), multiscale_mode='range', keep_ratio=False), NotImplementedError, "'range'"),
    (dict(img_scale=(320, 320), ratio_range=(0.5, 1.5), keep_ratio=False), NotImplementedError, 'ratio_range'),
    (dict(img_scale=(320, 640), multiscale_mode='square_range', ratio_range=(0.5, 1.5), keep_ratio=False),
     NotImplementedError, 'ratio_range'),
    (dict(img_scale=(320, 640), multiscale_mode='square_range', keep_ratio=False, interpolation='nearest'),
     NotImplementedError, 'bilinear'),
])
def test_rejected_resize_variants(resize, exc, match):
    from yunet_amd.pipelines import DevicePipeline
    with pytest.raises(exc, match=match):
        DevicePipeline(ms_pipeline(**resize))


def test_plan_cache_guard(monkeypatch):
    """More sizes than the engine keeps plans: every data source that builds the pipeline refuses, naming the knob."""
    import yunet_amd.engine as E
    import yunet_amd.runner as R
    from yunet_amd.datasets import RetinaFaceSource
    from yunet_amd.pipelines import DevicePipeline
    assert len(M.out_sizes(320, 640)) == 11 <= 16            # the issue's range fits the default
    R.SyntheticSourceImages(REF_PIPELINE, samples_per_gpu=2)
    wide = ms_pipeline(img_scale=(64, 1024), multiscale_mode='square_range', keep_ratio=False)     # 31 sizes
    if E.MAX_PLANS < 31:
        with pytest.raises(ValueError, match='YUNET_MAX_PLANS'):
            R.SyntheticSourceImages(wide, samples_per_gpu=2)
    monkeypatch.setattr(E, 'MAX_PLANS', 3)
    with pytest.raises(ValueError, match='YUNET_MAX_PLANS >= 11'):
        R.SyntheticSourceImages(REF_PIPELINE, samples_per_gpu=2)
    with pytest.raises(ValueError, match='YUNET_MAX_PLANS'):
        RetinaFaceSource(dataset=None, pipeline=REF_PIPELINE)      # raised before the dataset is looked at
    with pytest.raises(ValueError, match='YUNET_MAX_PLANS'):
        DevicePipeline(REF_PIPELINE).check_plan_cache()
    monkeypatch.setattr(E, 'MAX_PLANS', 11)
    R.SyntheticSourceImages(REF_PIPELINE, samples_per_gpu=2)


# ------------------------------------------------------------------ YuNetTextLoggerHook
class _ToyModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([1.0, -2.0]))

    def train_step(self, data, optimizer):
        loss = (self.w * data['x']).sum() ** 2
        return dict(loss=loss, log_vars=OrderedDict(loss=loss.detach()), num_samples=1)


class _ToySource:
    iters_per_epoch = 4
    SIZES = [(320, 320), (192, 192), (640, 640), (288, 288)]

    def batch(self, it, device=None):
        s = self.SIZES[it % 4]
        metas = [dict(img_shape=s + (3,), pad_shape=s + (3,), batch_input_shape=(640, 640)),
                 dict(img_shape=(640, 640, 3), pad_shape=(640, 640, 3), batch_input_shape=(640, 640))]
        return dict(x=torch.tensor([1.0 + it, 0.5]), img_metas=metas)


def test_yunet_text_logger_hook_logs_image_scale(tmp_path):
    import yunet_amd.runner as R
    lines = []
    m = _ToyModel()
    opt = torch.optim.SGD(m.parameters(), lr=0.01)
    opt.param_groups[0]['initial_lr'] = 0.01
    r = R.EpochBasedRunner(m, opt, str(tmp_path), lines.append, dict(seed=1), max_epochs=2)
    r.register_training_hooks(dict(policy='step', step=[1]), dict(grad_clip=None), None,
                              dict(interval=1, hooks=[dict(type='YuNetTextLoggerHook')]))
    assert [type(h).__name__ for h in r.hooks][-1] == 'YuNetTextLoggerHook'
    assert issubclass(R.HOOKS['YuNetTextLoggerHook'], R.TextLoggerHook)
    hist = r.run([_ToySource()], device='cpu')
    assert len(lines) == 8 and lines[0].startswith('Epoch [1][1] lr:')
    got = [re.search(r'image_scale: \((\d+), (\d+)\)', ln).groups() for ln in lines]
    assert got == [(str(h), str(w)) for h, w in _ToySource.SIZES * 2]       # the FIRST image of each batch
    assert all('loss: ' in ln for ln in lines)
    assert all('image_scale' not in rec for rec in (hist or r.log_buffer))   # log_buffer keeps scalars only


# ------------------------------------------------------------------ ABI
def test_new_entry_points_are_declared_and_bound():
    import yunet_amd._lib as L
    txt = open(os.path.join(ROOT, 'include', 'yunet_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for name in ('yunet_aug_decide', 'yunet_aug_pixels'):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', txt)
        assert m, f'{name} is not declared in include/yunet_hip.h'
        assert name in L.EXPORTED
        assert len(m.group(1).split(',')) == len(L._SIGNATURES[name][1]), f'{name}: argument counts differ'
    lib = L.load()
    assert hasattr(lib, 'yunet_aug_decide') and hasattr(lib, 'yunet_aug_pixels')
    assert lib.yunet_abi_version() == 12
    assert int(re.search(r'#define\s+YUNET_AUG_MAX_EDGE\s+(\d+)', txt).group(1)) == L.AUG_MAX_EDGE


def _aug_cfg():
    import yunet_amd._lib as L
    cfg = L.YunetAugCfg()
    cfg.out_size, cfg.n_choice, cfg.gmax, cfg.max_attempts, cfg.max_retries = 320, 1, 64, 250, 64
    return cfg


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument checks come before any launch: no device needed."""
    import ctypes as C
    import yunet_amd._lib as L
    lib = L.load()
    cfg = _aug_cfg()
    for lo, hi in ((31, 320), (0, 0), (320, 319), (320, L.AUG_MAX_EDGE + 1)):
        assert lib.yunet_aug_decide(None, None, None, None, 0, C.byref(cfg), 1, lo, hi, 0, 1, None, None, None, None,
                                    None) == L.EINVAL
    for hw, pos in ((0, L.PHOTO_NONE), (L.AUG_MAX_EDGE + 1, L.PHOTO_NONE), (320, 7), (320, L.PHOTO_POST)):
        a = L.YunetAugPixels(position=pos, out_hw=hw)
        assert lib.yunet_aug_pixels(C.byref(a), C.byref(cfg), 1, None, None) == L.EINVAL


def test_pixel_pass_refusal_table_without_a_gpu():
    """yunet_aug_pixels: every refusal of include/yunet_hip.h, one cause at a time.  The pointers of a case are non-NULL
    wherever its cause is not a NULL pointer (they address host memory: a refusal comes before any launch and nothing
    reads them), so a case cannot pass on account of another check; the descriptor without a fault is not called."""
    import ctypes as C
    import yunet_amd._lib as L
    lib = L.load()
    cfg = _aug_cfg()
    mem = (C.c_char * 64)()
    ptr = C.addressof(mem)
    mcfg = L.YunetMosaicCfg(img_scale=32, gmax=8, center_lo=0.5, center_hi=1.5, prob=1.0, pad_val=114.0)
    bad_mcfg = L.YunetMosaicCfg.from_buffer_copy(mcfg)
    bad_mcfg.img_scale = 0
    ok = dict(src=ptr, src_off=ptr, src_hw=ptr, params=ptr)
    mosaic = dict(ok, geom=ptr, mosaic=C.pointer(mcfg))
    cases = {
        'geom with rect': dict(mosaic, rect=ptr),
        'geom with PRE': dict(mosaic, position=L.PHOTO_PRE, pparams=ptr),
        'geom without mosaic': dict(ok, geom=ptr),
        'mosaic without geom': dict(ok, mosaic=C.pointer(mcfg)),
        'geom with a bad mosaic configuration': dict(mosaic, mosaic=C.pointer(bad_mcfg)),
        'PRE without pparams': dict(ok, position=L.PHOTO_PRE),
        'POST without pparams': dict(ok, position=L.PHOTO_POST),
        'POST without pparams, mosaic': dict(mosaic, position=L.PHOTO_POST),
        'position 7': dict(ok, position=7, pparams=ptr),
        'out_hw -1': dict(ok, out_hw=-1),
        'out_hw above the largest edge': dict(ok, out_hw=L.AUG_MAX_EDGE + 1),
        'NULL src': dict(ok, src=None),
        'NULL src_off': dict(ok, src_off=None),
        'NULL src_hw': dict(ok, src_hw=None),
        'NULL params': dict(ok, params=None),
    }
    for what, fields in cases.items():
        a = L.YunetAugPixels(**fields)
        assert lib.yunet_aug_pixels(C.byref(a), C.byref(cfg), 1, ptr, None) == L.EINVAL, what
    a = L.YunetAugPixels(**ok)
    assert lib.yunet_aug_pixels(C.byref(a), C.byref(cfg), 0, ptr, None) == L.EINVAL, 'N < 1'
    assert lib.yunet_aug_pixels(C.byref(a), C.byref(cfg), 1, None, None) == L.EINVAL, 'NULL out_img'
    assert lib.yunet_aug_pixels(C.byref(a), None, 1, ptr, None) == L.EINVAL, 'NULL cfg'
    assert lib.yunet_aug_pixels(None, C.byref(cfg), 1, ptr, None) == L.EINVAL, 'NULL a'
    cfg.out_size = 0
    assert lib.yunet_aug_pixels(C.byref(a), C.byref(cfg), 1, ptr, None) == L.EINVAL, 'out_hw == 0 with out_size < 1'


def test_decide_refusals_without_a_gpu():
    """yunet_aug_decide: multiscale = 0 needs cfg->out_size >= 1 and ignores the scale arguments; a negative in_gmax and
    a bad configuration are refused in every form (one check, aug_cfg_ok)."""
    import ctypes as C
    import yunet_amd._lib as L
    lib = L.load()

    def call(cfg, in_gmax, ms, lo, hi, n=1):
        return lib.yunet_aug_decide(None, None, None, None, in_gmax, C.byref(cfg) if cfg else None, ms, lo, hi, 0, n,
                                    None, None, None, None, None)
    for in_gmax in (0, 8):
        cfg = _aug_cfg()
        cfg.out_size = 0
        assert call(cfg, in_gmax, 0, 320, 640) == L.EINVAL
        assert call(_aug_cfg(), in_gmax, 0, 320, 640, n=0) == L.EINVAL
        assert call(None, in_gmax, 1, 320, 640) == L.EINVAL
        for field, value in (('n_choice', 0), ('n_choice', 9), ('gmax', 0), ('max_attempts', 0), ('max_retries', 0)):
            for ms in (0, 1):
                cfg = _aug_cfg()
                setattr(cfg, field, value)
                assert call(cfg, in_gmax, ms, 320, 640) == L.EINVAL, (field, ms)
    assert call(_aug_cfg(), -1, 0, 0, 0) == L.EINVAL


def test_cfg_options_reach_the_resize_entry_and_the_logger_hook():
    """The issue's command line: --cfg-options data.train.pipeline.3.*=... log_config.hooks.0.type=YuNetTextLoggerHook on
    the shipped config (a number after a list-valued key indexes the list, as mmcv's Config.merge_from_dict does)."""
    import yunet_amd
    import yunet_amd.runner as R
    from yunet_amd.pipelines import DevicePipeline
    from yunet_amd.registry import DictAction
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    cfg.merge_from_dict({'data.train.pipeline.3.img_scale': DictAction.parse_value('(320,640)'),
                         'data.train.pipeline.3.multiscale_mode': DictAction.parse_value('square_range'),
                         'log_config.hooks.0.type': 'YuNetTextLoggerHook',
                         'data.train.type': 'SyntheticSourceImages'})
    assert len(cfg.data.train.pipeline) == 8 and cfg.data.train.pipeline[3]['type'] == 'Resize'
    pipe = DevicePipeline(cfg.data.train.pipeline)
    assert pipe.scale_range == (320, 640) and len(pipe.out_sizes) == 11
    assert [h['type'] for h in cfg.log_config.hooks] == ['YuNetTextLoggerHook', 'TensorboardLoggerHook']
    assert cfg.log_config.hooks[0]['type'] in R.HOOKS
    cfg.merge_from_dict({'fp16.loss_scale': 512.0, 'data.train.pipeline': [1, 2]})       # the existing grammar holds
    assert cfg.fp16.loss_scale == 512.0 and cfg.data.train.pipeline == [1, 2]
