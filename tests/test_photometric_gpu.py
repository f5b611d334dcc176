"""-m gpu: PhotoMetricDistortion in the device train pipeline (csrc/augment.hip aug_photometric_kernel and the PRE /
POST instances of aug_pixels_kernel) against the numpy restatement (tests/photometric_ref.py) and the fixtures made by
the unmodified reference class; the crop / flip / GT side unchanged by the transform; every source feed bit-identical
with the transform on; a few tools/train.py iterations through it."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import photometric_ref as R
import pipeline_oracle as P
from test_photometric import BASE, pipeline_case, pixels_case, sha_hex, with_photo
from test_source_store_gpu import _same, _write_labelv2

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS = {'pre': 2, 'post': 5}
WIDE = dict(brightness_delta=50, contrast_range=(0.3, 1.9), saturation_range=(0.1, 2.5), hue_delta=90)


def _p(t):
    return C.c_void_p(t.data_ptr())


def make_pipe(S, seed, position=None, crop_choice=None, photo=None, gmax=64):
    from yunet_amd.pipelines import DevicePipeline
    cfg = with_photo(POS[position], **(photo or {})) if position else [dict(p) for p in BASE]
    rsc = [i for i, c in enumerate(cfg) if c['type'] == 'RandomSquareCrop'][0]
    rs = [i for i, c in enumerate(cfg) if c['type'] == 'Resize'][0]
    if crop_choice is not None:
        cfg[rsc]['crop_choice'] = list(crop_choice)
    cfg[rs]['img_scale'] = (S, S)
    return DevicePipeline(cfg, seed=seed, gmax=gmax)


def run(srcs, pipe, iteration):
    from yunet_amd.pipelines import SourceBatch
    sb = SourceBatch.from_lists([s[0] for s in srcs], [s[1] for s in srcs], [s[2] for s in srcs], DEV)
    out = pipe(sb, iteration)
    torch.cuda.synchronize()
    return out


def photometric_table(photo, seed, iteration, N):
    import yunet_amd._lib as L
    from yunet_amd.pipelines import PhotoMetricDistortion
    pp = torch.full((N, L.PHOTO_WORDS), -7.0, device=DEV)
    cfg = PhotoMetricDistortion(**photo).c_cfg(L.PHOTO_POST)
    L.check(L.load().yunet_aug_photometric(C.byref(cfg), seed, iteration, N, _p(pp),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'yunet_aug_photometric')
    torch.cuda.synchronize()
    return pp.cpu().numpy()


@pytest.mark.parametrize('photo', [{}, WIDE])
def test_photometric_table_equals_restatement(photo):
    N = 4096
    for seed, it in ((0, 0), (7, 3), (12345, 99), (0xFFFFFFFF, 0xFFFFFFFE)):
        got = photometric_table(photo, seed, it, N)
        want = np.stack([R.draw_table(seed, it, i, **photo)[0] for i in range(N)])
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, f'(seed {seed}, it {it}) images {bad[:8]}: {got[bad[:1]]} vs {want[bad[:1]]}'
        assert {R.combo(t) for t in got} == set(range(64))


def test_photometric_rejects_bad_configurations():
    import yunet_amd._lib as L
    lib = L.load()
    pp = torch.zeros(4, L.PHOTO_WORDS, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for field, value in (('brightness_delta', -1.0), ('hue_delta', 361.0), ('contrast_lower', 2.0),
                         ('saturation_upper', 0.1), ('hue_delta', float('nan')), ('position', L.PHOTO_NONE)):
        from yunet_amd.pipelines import PhotoMetricDistortion
        cfg = PhotoMetricDistortion().c_cfg(L.PHOTO_PRE)
        setattr(cfg, field, value)
        assert lib.yunet_aug_photometric(C.byref(cfg), 0, 0, 4, _p(pp), stream) == L.EINVAL, field
    cfg = PhotoMetricDistortion().c_cfg(L.PHOTO_PRE)
    assert lib.yunet_aug_photometric(C.byref(cfg), 0, 0, 0, _p(pp), stream) == L.EINVAL
    torch.cuda.synchronize()
    assert not pp.any()


@pytest.mark.parametrize('p,position', [(0, 'pre'), (1, 'post')])
def test_hard_case_pixels_equal_the_reference_fixture(p, position):
    g, seed, it, S, srcs = pixels_case()
    pipe = make_pipe(S, seed, position, crop_choice=[1.0])
    out = run(srcs, pipe, it)
    assert pipe.check() == []
    params = pipe.params.cpu().numpy()
    assert np.array_equal(params[:, [2, 3, 5, 4]], g['meta'][p])
    img = out['img'].cpu().numpy()
    for i in range(4):
        assert np.array_equal(img[i], g[f'{position}_img_{i}']), f'image {i}'
    bad = [i for i in range(len(srcs)) if R.digest(img[i]) != sha_hex(g['sha'][p, i])]
    assert not bad, f'{position}: images differ from the reference fixture {bad}'


@pytest.mark.parametrize('position', ['pre', 'post'])
def test_pipeline_equals_the_reference_fixture(position):
    g, seed, it, S, srcs = pipeline_case()
    pipe = make_pipe(S, seed, position, crop_choice=g['crop_choice'])
    out = run(srcs, pipe, it)
    assert pipe.check() == []
    params = pipe.params.cpu().numpy()
    cnt = out['gt_bboxes'].counts.cpu().numpy()
    gb, gk = out['gt_bboxes'].padded.cpu().numpy(), out['gt_keypointss'].padded.cpu().numpy()
    img = out['img'].cpu().numpy()
    for i in range(len(srcs)):
        cw, flip, draws, kept = [int(v) for v in g[f'{position}_meta_{i}']]
        assert [int(v) for v in params[i, [2, 3, 5, 4]]] == [cw, flip, draws, kept] and int(cnt[i]) == kept
        assert np.array_equal(gb[i, :kept], g[f'{position}_boxes_{i}'])
        assert np.array_equal(gk[i, :kept], g[f'{position}_kps_{i}'])
        assert np.array_equal(img[i, :, :8, :8], g[f'{position}_corner_{i}'])
        assert R.digest(img[i]) == str(g[f'{position}_sha_{i}']), f'{position}: image {i}'


def _random_sources(n, seed):
    rng = np.random.default_rng(300 + seed)
    srcs = []
    for i in range(n):
        h, w = int(rng.integers(60, 700)), int(rng.integers(60, 700))
        g = int(rng.integers(1, 30)) if i % 5 else -int(rng.integers(1, 3))
        srcs.append(P.synth_image(rng, h, w, g))
    return srcs


@pytest.mark.parametrize('position', ['pre', 'post'])
@pytest.mark.parametrize('S,n,seed,it,photo', [(160, 24, 3, 0, {}), (320, 12, 4, 17, WIDE), (64, 40, 9, 5, {})])
def test_random_batches_equal_the_restatement(position, S, n, seed, it, photo):
    srcs = _random_sources(n, seed)
    pipe = make_pipe(S, seed, position, photo=photo)
    out = run(srcs, pipe, it)
    assert pipe.check() == []
    img = out['img'].cpu().numpy()
    pp = pipe.pparams.cpu().numpy()
    for i, (im, b, k) in enumerate(srcs):
        r = R.augment_image(im, b, k, seed, it, i, S, BASE[2]['crop_choice'], position, photo)
        assert np.array_equal(pp[i], r['table'])
        if not np.array_equal(img[i], r['img']):
            d = np.abs(img[i] - r['img'])
            raise AssertionError(f'{position} image {i}: {int((d > 0).sum())} values differ, max {d.max()}')


def test_gt_and_decisions_identical_absent_pre_post():
    srcs = _random_sources(32, 11)
    outs = {}
    for position in (None, 'pre', 'post'):
        pipe = make_pipe(160, 11, position)
        o = run(srcs, pipe, 6)
        outs[position] = (pipe.params.cpu(), o)
    p0, o0 = outs[None]
    for position in ('pre', 'post'):
        p1, o1 = outs[position]
        assert torch.equal(p0, p1)
        for key in ('gt_bboxes', 'gt_keypointss'):
            assert torch.equal(o0[key].padded, o1[key].padded) and torch.equal(o0[key].counts, o1[key].counts)
        assert not torch.equal(o0['img'], o1['img'])
    assert not torch.equal(outs['pre'][1]['img'], outs['post'][1]['img'])


def test_shipped_list_equals_a_direct_pixel_launch():
    """Regression guard: without the transform DevicePipeline launches the plain pass (position = NONE) as before."""
    import yunet_amd._lib as L
    from yunet_amd.pipelines import SourceBatch
    srcs = _random_sources(16, 2)
    pipe = make_pipe(160, 2)
    sb = SourceBatch.from_lists([s[0] for s in srcs], [s[1] for s in srcs], [s[2] for s in srcs], DEV)
    out = pipe(sb, 4)
    assert pipe.pparams is None
    img = torch.empty_like(out['img'])
    a = L.YunetAugPixels(src=sb.src.data_ptr(), src_off=sb.src_off.data_ptr(), src_hw=sb.src_hw.data_ptr(),
                         params=pipe.params.data_ptr(), position=L.PHOTO_NONE)
    L.check(L.load().yunet_aug_pixels(C.byref(a), C.byref(pipe.cfg), sb.n, _p(img),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'pixels')
    torch.cuda.synchronize()
    assert torch.equal(out['img'], img)


def _photo_pipeline(position, S=None):
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_s.py'))
    pipeline = [dict(p) for p in cfg.train_pipeline]
    pipeline.insert(POS[position], dict(type='PhotoMetricDistortion'))
    if S is not None:
        pipeline[[i for i, c in enumerate(pipeline) if c['type'] == 'Resize'][0]]['img_scale'] = (S, S)
    return pipeline


@pytest.mark.parametrize('position', ['pre', 'post'])
def test_synthetic_feeds_bit_identical_with_the_transform(position):
    import yunet_amd.runner as R_
    pipeline = _photo_pipeline(position)
    kw = dict(samples_per_gpu=12, pool=5, seed=3, src_hw=((300, 420), (512, 384), (200, 200)))
    feeds = {'resident': R_.SyntheticSourceImages(pipeline, **kw),
             'host_fed': R_.SyntheticSourceImages(pipeline, host_fed=True, **kw),
             'window_dma': R_.SyntheticSourceImages(pipeline, host_fed='window', host_fetch='dma', **kw),
             'window_kernel': R_.SyntheticSourceImages(pipeline, host_fed='window', host_fetch='kernel', **kw)}
    plain = R_.SyntheticSourceImages([p for p in pipeline if p['type'] != 'PhotoMetricDistortion'], **kw)
    for it in range(6):
        outs = {k: f.batch(it, DEV) for k, f in feeds.items()}
        ref = plain.batch(it, DEV)
        torch.cuda.synchronize()
        for k in ('host_fed', 'window_dma', 'window_kernel'):
            _same(outs['resident'], outs[k])
        assert not torch.equal(outs['resident']['img'], ref['img'])
        for key in ('gt_bboxes', 'gt_keypointss'):
            assert torch.equal(outs['resident'][key].padded, ref[key].padded)
        # each batch carries its own iteration's table (WindowFeed plans two iterations ahead)
        want = np.stack([R.draw_table(3, it, i)[0] for i in range(12)])
        for k in ('resident', 'window_kernel'):
            assert np.array_equal(feeds[k].pipe.pparams.cpu().numpy(), want), (k, it)
    feeds['window_kernel']._feed.check()


def test_retinaface_caches_bit_identical_with_the_transform(tmp_path):
    from yunet_amd.datasets import RetinaFaceDataset, RetinaFaceSource
    ann, prefix = _write_labelv2(tmp_path)
    pipeline = _photo_pipeline('post', S=64)
    srcs = {}
    for cache, fetch in ((None, None), ('device', None), ('host', None), ('host', 'kernel')):
        ds = RetinaFaceDataset(ann, img_prefix=prefix, pipeline=pipeline)
        srcs[(cache, fetch)] = RetinaFaceSource(ds, pipeline, samples_per_gpu=4, seed=2, workers=2, cache=cache,
                                                host_fetch=fetch)
    ipe = srcs[(None, None)].iters_per_epoch
    for it in range(ipe + 2):
        outs = {k: s.batch(it, DEV) for k, s in srcs.items()}
        torch.cuda.synchronize()
        for k in list(srcs)[1:]:
            _same(outs[(None, None)], outs[k])


def test_train_cli_runs_with_the_transform(tmp_path):
    spec = importlib.util.spec_from_file_location('yunet_train_tool_photo', os.path.join(ROOT, 'tools', 'train.py'))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    cfg = tmp_path / 'yunet_s_photo.py'
    cfg.write_text(open(os.path.join(ROOT, 'configs', 'yunet_s.py')).read() +
                   "\ntrain_pipeline.insert(5, dict(type='PhotoMetricDistortion'))\n")
    hist = T.main([str(cfg), '--work-dir', str(tmp_path / 'w'), '--seed', '3', '--no-validate', '--max-iters', '4',
                   '--cfg-options', 'data.samples_per_gpu=8', 'data.train.type=SyntheticSourceImages',
                   'data.train.pool=4', 'log_config.interval=1'])
    losses = [h['loss'] for h in hist if 'loss' in h]
    assert losses and all(np.isfinite(losses)), hist
