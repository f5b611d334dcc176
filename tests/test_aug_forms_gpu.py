"""-m gpu: every instance behind the two entries of the device train pipeline is reached by a GPU test.

yunet_aug_pixels dispatches on (rect, position, out_hw, geom) to 16 instances of aug_pixels_kernel<WIN, PH, CANVAS, MOSAIC>,
yunet_aug_decide on (multiscale, in_gmax) to 4 of aug_decide_kernel<MS, PAD>.  Where each is pinned:

  pixels, no mosaic, out_hw = 0
    whole sources, NONE          test_pipeline_gpu (the reference fixtures), test_photometric_gpu direct launch
    whole sources, PRE / POST    test_photometric_gpu (fixtures and restatement)
    window buffer, NONE          test_source_store_gpu (windowed == resident)
    window buffer, PRE / POST    test_photometric_gpu::test_synthetic_feeds_bit_identical_with_the_transform
  pixels, no mosaic, out_hw > 0
    all six of {whole, window} x {NONE, PRE, POST}
                                 test_multiscale_gpu::test_canvas_corner_equals_fixed_size_pass_and_border_is_zero
  pixels, mosaic (whole store)
    NONE, out_hw = 0 / POST, out_hw = 0 / NONE, out_hw > 0
                                 test_mosaic_gpu::test_pipeline_equals_existing_pipeline_on_materialised_canvases
                                 [fixed / post_photo / square_range]
    POST, out_hw > 0             no list of test_mosaic_gpu combines the three: test_mosaic_canvas_post_* below
  decide
    ragged, fixed / ragged, multiscale       test_pipeline_gpu / test_multiscale_gpu
    padded, fixed / padded, multiscale       test_mosaic_gpu [fixed / square_range], through the pipeline only;
                                             test_padded_decide_equals_ragged_decide below compares them directly

Shapes: three sources between 24 x 40 and 48 x 64, one wider than tall and one taller than wide, so a crop window leaves
the image on either axis; outputs 32 and 64 (one and four workgroups' worth of pixels, and both sides of a canvas)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pipeline_oracle as P
from test_mosaic import mosaic_list
from test_mosaic_gpu import make_store

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HW = ((24, 64), (48, 40), (36, 48))
SEED = 5


def sources():
    rng = np.random.default_rng(41)
    return [P.synth_image(rng, h, w, g) for (h, w), g in zip(HW, (3, 5, 2))]


def _skipped(seed, iteration, n, prob):
    """The prob draw of yunet_aug_mosaic_decide for image n (the fourth draw of its sub-stream), on the host."""
    import yunet_amd._lib as L
    from yunet_amd.pipelines import _mix32
    k = _mix32((seed & 0xFFFFFFFF) ^ ((iteration * 0x27D4EB2F) & 0xFFFFFFFF))
    k = _mix32(_mix32(k ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)) ^ L.MOSAIC_SALT)
    return _mix32(k ^ ((3 * 0x85EBCA6B + 0xC2B2AE35) & 0xFFFFFFFF)) / 4294967296.0 > prob


def test_mosaic_canvas_post_corner_equals_the_fixed_size_form():
    """Mosaic, PhotoMetricDistortion after RandomFlip, multi-scale canvas: the S_n x S_n corner of image n is bit-identical
    to the mosaic POST form at out_hw = 0, out_size = S_n (pinned by test_mosaic_gpu [post_photo]) on the same params,
    geometry and photometric table, and the border is exactly 0.  One image is skipped by prob (it reads its own
    source), one has no surviving box (status 1: the crop's pad value, distorted, inside its corner).  S_n is written
    by hand, (32, 64, 32): the range (32, 64) draws 64 once in 33, and the pixel pass reads nothing else of the draw."""
    import yunet_amd._lib as L
    from yunet_amd.pipelines import DevicePipeline
    prob, n = 0.6, 3
    it = next(i for i in range(64) if [_skipped(SEED, i, k, prob) for k in range(n)] == [False, True, False])
    pipe = DevicePipeline(mosaic_list(dict(type='Mosaic', img_scale=(32, 32), use_kps=True, prob=prob),
                                      dict(img_scale=(32, 64), multiscale_mode='square_range', keep_ratio=False), 'post'),
                          seed=SEED, gmax=2)
    assert pipe.gmax == 8 and pipe.photo_position == L.PHOTO_POST
    sb = make_store(sources()).batch(list(range(n)))
    view, idx = sb.store_view()
    dev = torch.device(DEV)
    merged = pipe._mosaic_decide((view, idx), n, it, dev)
    assert pipe.geom[:, L.MOSAIC_APPLIED].tolist() == [1, 0, 1]
    merged[2][2] = 0                                    # image 2: no box survives
    _, _, cnt, params = pipe._decide(sb, it, dev, merged)
    pp = pipe._photometric(n, it, dev)
    sizes = [32, 64, 32]
    params[:, 7] = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    st = params[:, 6].tolist()
    assert st[2] == 1 and st[1] == 0 and cnt.tolist()[2] == 0
    form = dict(src=sb.src, src_off=view.off, src_hw=merged[3], params=params, pparams=pp, position=L.PHOTO_POST)

    def run(cfg, out, out_hw):
        p = lambda t: t.data_ptr()   # noqa: E731
        a = L.YunetAugPixels(geom=p(pipe.geom), mosaic=C.pointer(pipe.mosaic_cfg), out_hw=out_hw,
                             **{k: (p(v) if torch.is_tensor(v) else v) for k, v in form.items()})
        L.check(L.load().yunet_aug_pixels(C.byref(a), C.byref(cfg), n, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'yunet_aug_pixels')
        torch.cuda.synchronize()

    canvas = torch.full((n, 3, 64, 64), float('nan'), device=DEV)
    run(pipe.cfg, canvas, 64)
    for S in (32, 64):
        cfg = L.YunetAugCfg.from_buffer_copy(pipe.cfg)
        cfg.out_size = S
        fixed = torch.full((n, 3, S, S), float('nan'), device=DEV)
        run(cfg, fixed, 0)
        assert not torch.isnan(fixed).any()
        for i in (k for k in range(n) if sizes[k] == S):
            assert torch.equal(canvas[i, :, :S, :S], fixed[i]), f'corner differs from the fixed-size form (image {i})'
            rest = canvas[i].clone()
            rest[:, :S, :S] = 0
            assert torch.equal(rest, torch.zeros_like(rest)), f'border is not exactly zero (image {i})'
    inside = canvas[2, :, :32, :32]                     # one pad value through one table: constant per channel
    assert all(float(inside[c].min()) == float(inside[c].max()) for c in range(3))
    assert float(canvas[1].std()) > 0


@pytest.mark.parametrize('multiscale,out_size', [(0, 32), (0, 64), (1, 32)])
def test_padded_decide_equals_ragged_decide(multiscale, out_size):
    """The same GT as ragged lists (in_gmax = 0, prefix offsets) and as a padded table (in_gmax = 8, counts): params,
    boxes, keypoints and counts bit-identical, fixed size and multi-scale.  One image has no GT; the padding rows hold
    a box over the whole image that would be kept if a row at or beyond the count were read."""
    import yunet_amd._lib as L
    from yunet_amd.pipelines import SourceBatch
    lib = L.load()
    srcs = sources()
    srcs[1] = (srcs[1][0], srcs[1][1][:0], srcs[1][2][:0])
    sb = SourceBatch.from_lists([s[0] for s in srcs], [s[1] for s in srcs], [s[2] for s in srcs], DEV)
    n, in_gmax, gmax = len(srcs), 8, 4
    pb = torch.tensor([0.0, 0.0, 64.0, 64.0], device=DEV).repeat(n, in_gmax, 1)
    pk = torch.full((n, in_gmax, 5, 3), 7.0, device=DEV)
    counts = torch.tensor([len(s[1]) for s in srcs], dtype=torch.int32, device=DEV)
    off = sb.gt_off.tolist()
    for i, c in enumerate(counts.tolist()):
        pb[i, :c] = sb.boxes[off[i]:off[i] + c]
        pk[i, :c] = sb.kps[off[i]:off[i] + c]
    cfg = L.YunetAugCfg(out_size=out_size, n_choice=2, flip_ratio=0.5, pad_value=128.0, seed=SEED, max_attempts=250,
                        max_retries=64, gmax=gmax)
    cfg.crop_choice[0], cfg.crop_choice[1] = 0.7, 1.3
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = []
    for boxes, kps, gt_idx, g in ((sb.boxes, sb.kps, sb.gt_off, 0), (pb, pk, counts, in_gmax)):
        out = (torch.full((n, 8), -7, dtype=torch.int32, device=DEV), torch.full((n, gmax, 4), -7.0, device=DEV),
               torch.full((n, gmax, 5, 3), -7.0, device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV))
        L.check(lib.yunet_aug_decide(p(sb.src_hw), p(boxes), p(kps), p(gt_idx), g, C.byref(cfg), multiscale, 32, 64, 9, n,
                                     p(out[0]), p(out[1]), p(out[2]), p(out[3]), stream), 'yunet_aug_decide')
        got.append(out)
    torch.cuda.synchronize()
    for a, b in zip(*got):
        assert torch.equal(a, b)
    params = got[0][0]
    assert params[:, 6].tolist() == [0, 1, 0] and int(got[0][3].sum()) > 0
    assert all(s in (32, 64) for s in params[:, 7].tolist()) if multiscale else not params[:, 7].any()
