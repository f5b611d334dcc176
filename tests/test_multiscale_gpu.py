"""-m gpu: multi-scale training on the device -- yunet_aug_decide (multiscale = 1) / yunet_aug_pixels (out_hw > 0) and
DevicePipeline with Resize(multiscale_mode='square_range') against (a) the fixture made by the unmodified reference
transforms, (b) the numpy restatement tests/multiscale_ref.py (everything bit-exact, zero border included), (c) the
fixed-size form of the pixel entry (out_hw = 0) at out_size = S_n, and (d) the engine fed with the same tensors as a ready batch.
Every case is one bounded pass: no retries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import multiscale_ref as M
import pipeline_oracle as P
from test_multiscale import ms_pipeline

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHOTO = dict(type='PhotoMetricDistortion', brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
             hue_delta=18)


def make_pipe(lo, hi, seed, gmax=64, photo=None):
    from yunet_amd.pipelines import DevicePipeline
    cfg = ms_pipeline(img_scale=(lo, hi), multiscale_mode='square_range', keep_ratio=False)
    if photo == 'pre':
        cfg.insert(2, dict(PHOTO))
    elif photo == 'post':
        cfg.insert(5, dict(PHOTO))
    return DevicePipeline(cfg, seed=seed, gmax=gmax)


def source_batch(srcs):
    from yunet_amd.pipelines import SourceBatch
    return SourceBatch.from_lists([s[0] for s in srcs], [s[1] for s in srcs], [s[2] for s in srcs], DEV)


def random_sources(rng, n, lo=60, hi=500):
    srcs = []
    for i in range(n):
        h, w = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
        g = int(rng.integers(1, 40)) if i % 5 else -int(rng.integers(1, 3))
        srcs.append(P.synth_image(rng, h, w, g))
    return srcs


# ------------------------------------------------------------------ (a) the reference fixture
@pytest.mark.parametrize('name', M.SETS)
def test_device_pipeline_vs_reference_fixture(name):
    """The bar of tests/test_pipeline_gpu.py::test_device_pipeline_vs_reference_fixtures: decisions equal, boxes /
    keypoints bit-exact, image windows and digests array_equal."""
    g, seed, it, lo, hi, srcs = M.load_case(name)
    pipe = make_pipe(lo, hi, seed)
    out = pipe(source_batch(srcs), it)
    torch.cuda.synchronize()
    assert pipe.check() == []
    params = pipe.params.cpu().numpy()
    cnt = out['gt_bboxes'].counts.cpu().numpy()
    gb, gk = out['gt_bboxes'].padded.cpu().numpy(), out['gt_keypointss'].padded.cpu().numpy()
    img = out['img'].cpu().numpy()
    sizes = [int(g[f'meta_{i}'][4]) for i in range(len(srcs))]
    smax = max(sizes)
    assert img.shape == (len(srcs), 3, smax, smax) and pipe.sizes.tolist() == sizes
    for i in range(len(srcs)):
        cw, flip, draws, kept, S = [int(v) for v in g[f'meta_{i}']]
        assert (int(params[i, 2]), int(params[i, 3]), int(params[i, 5]), int(params[i, 4]), int(params[i, 7])) == \
            (cw, flip, draws, kept, S), f'decision differs from the reference (image {i})'
        assert int(cnt[i]) == kept
        assert np.array_equal(gb[i, :kept], g[f'boxes_{i}']), f'boxes differ (image {i})'
        assert np.array_equal(gk[i, :kept], g[f'kps_{i}']), f'keypoints differ (image {i})'
        assert not gb[i, kept:].any() and not gk[i, kept:].any()
        dig, corner, center = M.image_digest(img[i, :, :S, :S])
        assert np.array_equal(corner, g[f'img_corner_{i}']) and np.array_equal(center, g[f'img_center_{i}'])
        assert np.array_equal(dig, g[f'img_digest_{i}'])
        border = img[i].copy()
        border[:, :S, :S] = 0
        assert not border.any(), f'collate border is not zero (image {i})'
        m = out['img_metas'][i]
        assert m['img_shape'] == (S, S, 3) == m['pad_shape'] and m['batch_input_shape'] == (smax, smax)


# ------------------------------------------------------------------ (b) the restatement, whole batch
@pytest.mark.parametrize('lo,hi,n,seed,it', [(160, 320, 20, 3, 0), (320, 640, 8, 4, 17), (300, 500, 10, 5, 2),
                                             (96, 96, 4, 6, 1)])
def test_device_pipeline_vs_restatement(lo, hi, n, seed, it):
    """Seeded batches, an image without GT among them (status 1: it still draws its S_n, its corner is the crop's pad
    value, its border zero): params, GT and the whole canvas bit-identical to tests/multiscale_ref.py."""
    rng = np.random.default_rng(200 + seed)
    srcs = random_sources(rng, n)
    srcs[1] = (srcs[1][0], srcs[1][1][:0], srcs[1][2][:0])
    pipe = make_pipe(lo, hi, seed)
    out = pipe(source_batch(srcs), it)
    torch.cuda.synchronize()
    params = pipe.params.cpu().numpy()
    gb, gk = out['gt_bboxes'].padded.cpu().numpy(), out['gt_keypointss'].padded.cpu().numpy()
    cnt = out['gt_bboxes'].counts.cpu().numpy()
    res = [M.augment_image(im, b, k, seed, it, i, lo, hi, pipe.steps[2].crop_choice) for i, (im, b, k) in enumerate(srcs)]
    for i, r in enumerate(res):
        assert int(params[i, 7]) == r['S'] and int(params[i, 5]) == r['draws'] and int(params[i, 6]) == r['status'], i
        if r['status'] == 0:
            assert np.array_equal(params[i, :4], r['params']), f'window / flip differ (image {i})'
        k = r['boxes'].shape[0]
        assert int(cnt[i]) == k and int(params[i, 4]) == k
        assert np.array_equal(gb[i, :k], r['boxes']) and np.array_equal(gk[i, :k], r['kps'])
    assert res[1]['status'] == 1 and res[1]['draws'] == 1
    want = M.collate_canvas(res)
    got = out['img'].cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), 'canvas differs from the restatement'
    with pytest.raises(ValueError, match='no window'):
        pipe.check()


# ------------------------------------------------------------------ (c) canvas vs the fixed-size entry points
def _window_buffer(pipe, sb, it):
    """pipe.window_plan on the device, the compact window buffer assembled on the host from the sources."""
    params, rect, off = pipe.window_plan(sb, it, torch.device(DEV))
    torch.cuda.synchronize()
    rect_h, off_h = rect.cpu().numpy(), off.cpu().numpy()
    src, src_off, hw = sb.src.cpu().numpy(), sb.src_off.cpu().numpy(), sb.src_hw.cpu().numpy()
    win = np.zeros(max(1, int(off_h[-1])), np.uint8)
    for n in range(sb.n):
        r0, c0, rows, cols = [int(v) for v in rect_h[n]]
        if rows * cols == 0:
            continue
        h, w = int(hw[n, 0]), int(hw[n, 1])
        im = src[int(src_off[n]):int(src_off[n]) + h * w * 3].reshape(h, w, 3)
        win[int(off_h[n]):int(off_h[n]) + rows * cols * 3] = im[r0:r0 + rows, c0:c0 + cols].reshape(-1)
    return torch.from_numpy(win).to(DEV), rect, off


def pixel_pass(cfg, n, out, *, src, src_off, src_hw, params, rect=None, pparams=None, position=0, out_hw=0):
    """One direct yunet_aug_pixels call on the current stream."""
    import yunet_amd._lib as L
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    a = L.YunetAugPixels(src=p(src), src_off=p(src_off), src_hw=p(src_hw), rect=p(rect), params=p(params),
                         pparams=p(pparams), position=position, out_hw=out_hw)
    return L.load().yunet_aug_pixels(C.byref(a), C.byref(cfg), n, C.c_void_p(out.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize('photo', [None, 'pre', 'post'])
@pytest.mark.parametrize('window', [False, True])
def test_canvas_corner_equals_fixed_size_pass_and_border_is_zero(photo, window):
    """For every image the S_n x S_n corner of yunet_aug_pixels at out_hw = Smax (the CANVAS = true instance) is
    bit-identical to the same entry at out_hw = 0 (the CANVAS = false instance; plain / window / photo / window+photo)
    run at out_size = S_n on the SAME params, and every other canvas pixel is exactly 0.0 -- PhotoMetricDistortion in
    the post position included.  The canvas is pre-filled with NaN."""
    import yunet_amd._lib as L
    lo, hi, seed, it, n = 160, 320, 13, 4, 12
    rng = np.random.default_rng(77)
    srcs = random_sources(rng, n)
    srcs[2] = (srcs[2][0], srcs[2][1][:0], srcs[2][2][:0])          # status 1: all pad inside, zero outside
    sb = source_batch(srcs)
    pipe = make_pipe(lo, hi, seed, photo=photo)
    dev = torch.device(DEV)
    _, _, _, params = pipe._decide(sb, it, dev)
    pp = pipe._photometric(n, it, dev) if photo else None
    win, rect, off = _window_buffer(pipe, sb, it) if window else (None, None, None)
    sizes = params[:, 7].cpu().numpy()
    assert len(set(sizes.tolist())) >= 3 and set(sizes.tolist()) <= set(pipe.out_sizes)
    smax = int(sizes.max())
    canvas = torch.full((n, 3, smax, smax), float('nan'), device=DEV)
    pix, pix_off = (win, off) if window else (sb.src, sb.src_off)
    form = dict(src=pix, src_off=pix_off, src_hw=sb.src_hw, params=params, rect=rect, pparams=pp,
                position=pipe.photo_position)
    L.check(pixel_pass(pipe.cfg, n, canvas, out_hw=smax, **form), 'canvas')
    torch.cuda.synchronize()
    for S in sorted(set(sizes.tolist())):
        cfg = L.YunetAugCfg.from_buffer_copy(pipe.cfg)
        cfg.out_size = int(S)
        fixed = torch.full((n, 3, S, S), float('nan'), device=DEV)
        L.check(pixel_pass(cfg, n, fixed, out_hw=0, **form), 'fixed-size pass')
        torch.cuda.synchronize()
        for i in np.nonzero(sizes == S)[0].tolist():
            a, b = canvas[i, :, :S, :S], fixed[i]
            assert not torch.isnan(b).any()
            assert torch.equal(a, b), f'corner differs from the fixed-size pass (image {i}, S {S})'
            rest = canvas[i].clone()
            rest[:, :S, :S] = 0
            assert torch.equal(rest, torch.zeros_like(rest)), f'border is not exactly zero (image {i}, S {S})'
    if photo != 'post':             # the image without GT: the crop's pad value inside (post distorts it), zero outside
        inside = canvas[2, :, :int(sizes[2]), :int(sizes[2])]
        assert float(inside.min()) == 128.0 == float(inside.max())


def test_canvas_entry_cuts_a_mismatched_size_at_the_canvas():
    """params whose S_n exceeds the canvas (a caller's mistake) never write outside it; S_n = 0 (params of the fixed-size
    decide) gives an all-zero image.  A guard band after the canvas stays untouched."""
    import yunet_amd._lib as L
    rng = np.random.default_rng(3)
    srcs = random_sources(rng, 3)
    sb = source_batch(srcs)
    pipe = make_pipe(160, 320, 2)
    _, _, _, params = pipe._decide(sb, 0, torch.device(DEV))
    params[0, 7] = 512
    params[1, 7] = 0
    hw = 160
    buf = torch.full((3 * 3 * hw * hw + 4096,), -7.0, device=DEV)
    L.check(pixel_pass(pipe.cfg, 3, buf, src=sb.src, src_off=sb.src_off, src_hw=sb.src_hw, params=params, out_hw=hw),
            'canvas')
    torch.cuda.synchronize()
    assert float(buf[3 * 3 * hw * hw:].min()) == -7.0 == float(buf[3 * 3 * hw * hw:].max())
    img = buf[:3 * 3 * hw * hw].view(3, 3, hw, hw)
    assert not img[1].any() and float(img[0].min()) >= 0.0 and float(img[0].max()) <= 255.0


# ------------------------------------------------------------------ windowed == __call__, determinism
@pytest.mark.parametrize('fetch', ['dma', 'kernel'])
def test_window_fed_multiscale_equals_resident(fetch):
    """runner.SyntheticSourceImages: resident sources (__call__, sizes read back after the decide) against
    host_fed='window' (windowed, sizes riding the plan made iterations ahead): bit-identical batches and metas."""
    import yunet_amd.runner as R
    kw = dict(samples_per_gpu=10, pool=5, seed=3, src_hw=((300, 420), (512, 384), (200, 200)))
    pipeline = ms_pipeline(img_scale=(160, 320), multiscale_mode='square_range', keep_ratio=False)
    a = R.SyntheticSourceImages(pipeline, **kw)
    b = R.SyntheticSourceImages(pipeline, host_fed='window', host_fetch=fetch, **kw)
    shapes = set()
    for it in range(6):
        ba, bb = a.batch(it, 'cuda'), b.batch(it, 'cuda')
        torch.cuda.synchronize()
        assert ba['img'].shape == bb['img'].shape and torch.equal(ba['img'], bb['img']), it
        assert torch.equal(ba['gt_bboxes'].padded, bb['gt_bboxes'].padded)
        assert torch.equal(ba['gt_bboxes'].counts, bb['gt_bboxes'].counts)
        assert torch.equal(ba['gt_keypointss'].padded, bb['gt_keypointss'].padded)
        assert ba['img_metas'] == bb['img_metas']
        assert torch.equal(a.pipe.params, b.pipe.params)
        shapes.add(tuple(int(m['img_shape'][0]) for m in ba['img_metas']))
    assert len(shapes) >= 3, 'the iterations draw their own sizes'
    b._feed.check()


def test_multiscale_is_deterministic_and_fixed_size_is_unchanged():
    """The same (seed, iteration) twice: identical batch; another iteration: another one.  The fixed-size pipeline on the
    sources of pipeline_s320.npz still gives that fixture (decisions, GT, image windows and digests: the parent's)."""
    from test_pipeline_gpu import make_pipe as fixed_pipe
    from test_pipeline_oracle import load_case
    rng = np.random.default_rng(1)
    sb = source_batch(random_sources(rng, 16, 100, 400))
    pipe = make_pipe(160, 320, 5)
    a = pipe(sb, 3)
    pa, sa = pipe.params.clone(), pipe.sizes.copy()
    b = pipe(sb, 3)
    assert torch.equal(pa, pipe.params) and np.array_equal(sa, pipe.sizes)
    assert torch.equal(a['img'], b['img']) and torch.equal(a['gt_bboxes'].padded, b['gt_bboxes'].padded)
    assert torch.equal(a['gt_keypointss'].padded, b['gt_keypointss'].padded) and a['img_metas'] == b['img_metas']
    pipe(sb, 4)
    assert not torch.equal(pa[:, [0, 1, 2, 7]], pipe.params[:, [0, 1, 2, 7]])
    g, seed, it, S, srcs = load_case('pipeline_s320.npz')
    fp = fixed_pipe(S, seed)
    out = fp(source_batch(srcs), it)
    torch.cuda.synchronize()
    params, img = fp.params.cpu().numpy(), out['img'].cpu().numpy()
    gb, gk = out['gt_bboxes'].padded.cpu().numpy(), out['gt_keypointss'].padded.cpu().numpy()
    assert img.shape == (len(srcs), 3, S, S) and not params[:, 7].any()
    for i in range(len(srcs)):
        cw, flip, draws, kept = [int(v) for v in g[f'meta_{i}']]
        assert (int(params[i, 2]), int(params[i, 3]), int(params[i, 5]), int(params[i, 4])) == (cw, flip, draws, kept)
        assert np.array_equal(gb[i, :kept], g[f'boxes_{i}']) and np.array_equal(gk[i, :kept], g[f'kps_{i}'])
        dig, corner, center = M.image_digest(img[i])
        assert np.array_equal(corner, g[f'img_corner_{i}']) and np.array_equal(center, g[f'img_center_{i}'])
        assert np.array_equal(dig, g[f'img_digest_{i}'])


# ------------------------------------------------------------------ (d) end to end
def test_three_train_steps_over_changing_geometry():
    """yunet_n, bs 8, square_range (160, 320): three train steps whose batches have three different Smax (the
    iterations are picked with the CPU restatement).  Losses finite; one engine plan per Smax; and before each step the
    same weights on the same padded tensor and GT handed over as a ready batch (ragged lists, the copy path) give the
    same loss -- exactly, the bar of tests/test_engine_gpu.py::test_padded_gt_is_read_in_place for GT delivered padded
    on the device against GT copied into the plan."""
    import yunet_amd
    from yunet_amd.optim import FusedSGD
    lo, hi, seed, bs = 160, 320, 11, 8
    rng = np.random.default_rng(8)
    srcs = [P.synth_image(rng, int(rng.integers(120, 300)), int(rng.integers(120, 300)), int(rng.integers(1, 12)))
            for _ in range(bs)]
    picked, seen = [], set()
    for it in range(400):
        smax = max(M.augment_image(im, b, k, seed, it, i, lo, hi, M.CROP_CHOICE)['S'] for i, (im, b, k) in enumerate(srcs))
        if smax not in seen:
            seen.add(smax)
            picked.append((it, smax))
        if len(picked) == 3:
            break
    assert len(picked) == 3, 'the range (160, 320) gives at least three batch sizes within 400 iterations'
    sb = source_batch(srcs)
    pipe = make_pipe(lo, hi, seed)
    torch.manual_seed(0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    model = yunet_amd.build_detector(cfg.model).to(DEV).train()
    opt = FusedSGD(model, lr=1e-4, momentum=0.9, weight_decay=5e-4)
    for step, (it, smax) in enumerate(picked):
        batch = pipe(sb, it)
        assert batch['img'].shape == (bs, 3, smax, smax) and pipe.check() == []
        cnt = batch['gt_bboxes'].counts.tolist()
        ready = dict(img=batch['img'].clone(), img_metas=[dict(m) for m in batch['img_metas']],
                     gt_bboxes=[batch['gt_bboxes'].padded[i, :c].clone() for i, c in enumerate(cnt)],
                     gt_labels=[torch.zeros(c, dtype=torch.int64, device=DEV) for c in cnt],
                     gt_keypointss=[batch['gt_keypointss'].padded[i, :c].clone() for i, c in enumerate(cnt)])
        want = {k: float(v) for k, v in model.train_step(ready, opt)['log_vars'].items()}
        out = model.train_step(batch, opt)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()
        torch.cuda.synchronize()
        got = {k: float(v) for k, v in out['log_vars'].items()}
        print(f'step {step}: iteration {it}, Smax {smax}, loss {got["loss"]!r} (ready batch {want["loss"]!r})')
        assert all(np.isfinite(v) for v in got.values()) and 0 < got['loss'] < 1e4
        assert got == want, (got, want)
        assert len(model.engine.plans) == step + 1
    assert sorted(k[1] for k in model.engine.plans) == sorted(s for _, s in picked)
    assert all(k[1] == k[2] for k in model.engine.plans)
