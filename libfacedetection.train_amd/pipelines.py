"""The reference's TRAIN input pipeline (configs/yunet_n.py:36-56) as a device stage.

    pipe = DevicePipeline(cfg.data.train.pipeline, seed=0, gmax=64)   # the reference's own list
    src = SourceBatch.from_lists(images_u8_hwc, gt_bboxes, gt_keypointss, device)
    batch = pipe(src, iteration)        # dict(img, img_metas, gt_bboxes, gt_labels, gt_keypointss)
    out = model.train_step(batch, optimizer)

`RandomSquareCrop -> Resize(keep_ratio=False) -> RandomFlip -> Normalize(0, 1) ->
DefaultFormatBundle -> Collect` run as two HIP kernels (csrc/augment.hip), three with an optional
`PhotoMetricDistortion` before RandomSquareCrop or after RandomFlip, two more launches with an optional
`RandomAffine` after RandomFlip and one more with an optional `CutOut` in front of Normalize; the classes below carry
the configuration under the reference's registry names (mmdet/datasets/pipelines/transforms.py,
formatting.py, loading.py) so the reference's config files build unchanged.  Decoding image files
(LoadImageFromFile) is outside this stage: sources arrive as uint8 HWC arrays.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .builder import PIPELINES
from .registry import build_from_cfg
from .synthetic import GTList


class _Carrier:
    """Configuration carrier: the arithmetic lives in the fused device stage."""

    def __init__(self, **kw):
        self.cfg = dict(kw)
        for k, v in kw.items():
            setattr(self, k, v)

    def __call__(self, results):
        raise NotImplementedError(
            f'{type(self).__name__} is executed inside DevicePipeline (HIP kernels); there is no '
            'per-sample CPU implementation in this framework')

    def __repr__(self):
        return f'{type(self).__name__}({self.cfg})'


@PIPELINES.register_module()
class LoadImageFromFile(_Carrier):
    def __init__(self, to_float32=False, color_type='color', file_client_args=None):
        super().__init__(to_float32=to_float32, color_type=color_type)


@PIPELINES.register_module()
class LoadAnnotations(_Carrier):
    def __init__(self, with_bbox=True, with_label=True, with_keypoints=False, with_mask=False,
                 with_seg=False, **kw):
        super().__init__(with_bbox=with_bbox, with_label=with_label, with_keypoints=with_keypoints)


@PIPELINES.register_module()
class RandomSquareCrop(_Carrier):
    """transforms.py:975-1169."""

    def __init__(self, crop_ratio_range=None, crop_choice=None, bbox_clip_border=True):
        if crop_choice is None or crop_ratio_range is not None:
            raise NotImplementedError('only RandomSquareCrop(crop_choice=[...]) (the shipped configs)')
        if not bbox_clip_border:
            raise NotImplementedError('bbox_clip_border=False')
        super().__init__(crop_choice=[float(c) for c in crop_choice])


@PIPELINES.register_module()
class Resize(_Carrier):
    """transforms.py:52-330, the keep_ratio=False cases of the train configs: one square scale, or the reference's own
    multiscale_mode='square_range' (transforms.py:128-149): per sample one edge from [min(img_scale), max(img_scale)],
    rounded down to a multiple of 32 (`scale_range` = (lo, hi); None for the fixed size)."""

    def __init__(self, img_scale=None, multiscale_mode='range', ratio_range=None, keep_ratio=True,
                 bbox_clip_border=True, backend='cv2', interpolation='bilinear', override=False):
        square = multiscale_mode == 'square_range' and ratio_range is None
        if isinstance(img_scale, list):
            if len(img_scale) != 1:
                if square:      # random_sample_square asserts len(img_scales) == 1
                    raise ValueError("Resize(multiscale_mode='square_range') takes one img_scale=(a, b), got "
                                     f'{len(img_scale)}')
                raise NotImplementedError(f'multi-scale Resize(multiscale_mode={multiscale_mode!r}) with '
                                          f"{len(img_scale)} scales; implemented: 'square_range' with one (a, b)")
            img_scale = img_scale[0]
        if ratio_range is not None:
            raise NotImplementedError(f'multi-scale Resize(ratio_range={ratio_range!r})')
        if square:
            if keep_ratio or img_scale is None or interpolation != 'bilinear' or not bbox_clip_border:
                raise NotImplementedError("only Resize(img_scale=(a, b), multiscale_mode='square_range', "
                                          'keep_ratio=False, bilinear)')
            lo, hi = int(min(img_scale)), int(max(img_scale))
            if lo < 32:
                raise ValueError(f"Resize(multiscale_mode='square_range'): the low end {lo} rounds down to an edge of 0 "
                                 '(edges are multiples of 32)')
            if hi > L.AUG_MAX_EDGE:
                raise ValueError(f"Resize(multiscale_mode='square_range'): the high end {hi} exceeds {L.AUG_MAX_EDGE}")
            super().__init__(img_scale=(int(img_scale[0]), int(img_scale[1])), multiscale_mode=multiscale_mode)
            self.scale_range = (lo, hi)
            return
        if keep_ratio or img_scale is None or img_scale[0] != img_scale[1] \
                or interpolation != 'bilinear' or not bbox_clip_border:
            raise NotImplementedError('only Resize(img_scale=(S, S), keep_ratio=False, bilinear)' + (
                f'; multiscale_mode={multiscale_mode!r} is not implemented for img_scale={tuple(img_scale)}'
                if img_scale is not None and img_scale[0] != img_scale[1] else ''))
        super().__init__(img_scale=(int(img_scale[0]), int(img_scale[1])))
        self.scale_range = None


@PIPELINES.register_module()
class RandomFlip(_Carrier):
    """transforms.py:378-546 (horizontal)."""

    def __init__(self, flip_ratio=None, direction='horizontal'):
        if direction != 'horizontal' or not isinstance(flip_ratio, float):
            raise NotImplementedError('only RandomFlip(flip_ratio=<float>, direction="horizontal")')
        super().__init__(flip_ratio=flip_ratio)


@PIPELINES.register_module()
class PhotoMetricDistortion(_Carrier):
    """transforms.py:1211-1312, the reference's constructor and defaults.  Runs inside the pixel pass at one of two
    positions of the list (DevicePipeline.PHOTO_POSITIONS); its draws come from a sub-stream of the pipeline's
    generator (include/yunet_hip.h YUNET_PHOTO_SALT)."""

    def __init__(self, brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18):
        vals = [brightness_delta, *contrast_range, *saturation_range, hue_delta]
        if len(vals) != 6 or not all(math.isfinite(float(v)) for v in vals):
            raise ValueError('PhotoMetricDistortion: finite brightness_delta / hue_delta and (lower, upper) ranges')
        if brightness_delta < 0 or hue_delta < 0:
            raise ValueError(f'PhotoMetricDistortion: negative delta (brightness_delta={brightness_delta}, '
                             f'hue_delta={hue_delta})')
        if hue_delta > 360:
            raise ValueError(f'PhotoMetricDistortion: hue_delta={hue_delta} exceeds the 360 degrees of a hue turn')
        for name, (lo, hi) in (('contrast_range', contrast_range), ('saturation_range', saturation_range)):
            if lo > hi:
                raise ValueError(f'PhotoMetricDistortion: {name}={tuple((lo, hi))} has lower > upper')
        super().__init__(brightness_delta=brightness_delta, contrast_range=tuple(contrast_range),
                         saturation_range=tuple(saturation_range), hue_delta=hue_delta)
        self.contrast_lower, self.contrast_upper = contrast_range
        self.saturation_lower, self.saturation_upper = saturation_range

    def c_cfg(self, position):
        c = L.YunetPhotoCfg()
        c.brightness_delta, c.hue_delta = float(self.brightness_delta), float(self.hue_delta)
        c.contrast_lower, c.contrast_upper = float(self.contrast_lower), float(self.contrast_upper)
        c.saturation_lower, c.saturation_upper = float(self.saturation_lower), float(self.saturation_upper)
        c.position = position
        return c


@PIPELINES.register_module()
class Mosaic(_Carrier):
    """transforms.py:2218-2519 with the reference's constructor, under MultiImageMixDataset
    (dataset_wrappers.py:338-444).  Runs as yunet_aug_mosaic_decide + the MOSAIC form of the pixel pass; its draws come
    from a sub-stream of the pipeline's generator (include/yunet_hip.h YUNET_MOSAIC_SALT).  Partner indices are drawn
    from [0, len(dataset)), as by the reference: its `random` is numpy's (transforms.py:10), whose randint excludes the
    upper end."""

    def __init__(self, img_scale=(640, 640), center_ratio_range=(0.5, 1.5), min_bbox_size=0, bbox_clip_border=True,
                 skip_filter=True, pad_val=114, prob=1.0, use_kps=False):
        if not use_kps:
            raise NotImplementedError('Mosaic(use_kps=False): the device pipeline always carries the five landmarks '
                                      '(LoadAnnotations(with_keypoints=True)); write use_kps=True')
        if len(img_scale) != 2 or int(img_scale[0]) != int(img_scale[1]):
            raise NotImplementedError(f'Mosaic(img_scale={tuple(img_scale)}): only the square canvas '
                                      '(img_scale=(S, S)) is built; the rectangular one is not')
        S = int(img_scale[0])
        if not 1 <= S <= L.AUG_MAX_EDGE // 2:
            raise ValueError(f'Mosaic(img_scale=({S}, {S})): S must lie in [1, {L.AUG_MAX_EDGE // 2}]')
        lo, hi = (float(v) for v in center_ratio_range)
        if not 0.0 <= lo <= hi <= 2.0:
            raise ValueError(f'Mosaic(center_ratio_range={tuple(center_ratio_range)}): the centre must lie on the '
                             'canvas, 0 <= lo <= hi <= 2')
        if not 0 <= prob <= 1.0:
            raise ValueError(f'Mosaic: the probability should be in range [0, 1], got {prob}')
        if isinstance(pad_val, (list, tuple)) or not math.isfinite(float(pad_val)) \
                or not math.isfinite(float(min_bbox_size)):
            raise ValueError('Mosaic: one finite pad_val and a finite min_bbox_size')
        super().__init__(img_scale=(S, S), center_ratio_range=(lo, hi), min_bbox_size=min_bbox_size,
                         bbox_clip_border=bool(bbox_clip_border), skip_filter=bool(skip_filter), pad_val=pad_val,
                         prob=float(prob), use_kps=True)

    def c_cfg(self, seed, gmax):
        c = L.YunetMosaicCfg()
        c.img_scale, c.gmax = self.img_scale[0], gmax
        c.center_lo, c.center_hi = self.center_ratio_range
        c.prob, c.min_bbox_size, c.pad_val = self.prob, float(self.min_bbox_size), float(self.pad_val)
        c.seed, c.bbox_clip_border, c.skip_filter = seed & 0xFFFFFFFF, int(self.bbox_clip_border), int(self.skip_filter)
        return c


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


@PIPELINES.register_module()
class CutOut(_Carrier):
    """transforms.py:2143-2214 with the reference's constructor; its assertions are ValueErrors here.  Runs as
    yunet_aug_cutout on the finished batch tensor, between RandomFlip (or a POST PhotoMetricDistortion) and Normalize;
    its draws come from a sub-stream of the pipeline's generator (include/yunet_hip.h YUNET_CUTOUT_SALT).  `n_holes` is
    an int or the closed interval (a, b); a candidate is one (w, h) pair or a list of pairs -- pixels for `cutout_shape`,
    fractions of the image's edge for `cutout_ratio`; `fill_in` is a scalar or three values in the image's channel
    order (BGR).  Limits of this build: at most _lib.CUTOUT_MAX_HOLES holes and _lib.CUTOUT_MAX_CANDIDATES candidates."""

    def __init__(self, n_holes, cutout_shape=None, cutout_ratio=None, fill_in=(0, 0, 0)):
        if (cutout_shape is None) == (cutout_ratio is None):
            raise ValueError('CutOut: either cutout_shape or cutout_ratio should be specified, not both and not neither')
        with_ratio = cutout_ratio is not None
        arg = 'cutout_ratio' if with_ratio else 'cutout_shape'
        if isinstance(n_holes, (tuple, list)):
            if len(n_holes) != 2 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in n_holes) \
                    or not 0 <= n_holes[0] < n_holes[1]:
                raise ValueError(f'CutOut: n_holes={n_holes!r} must be an int or (a, b) with 0 <= a < b')
            n_holes = (int(n_holes[0]), int(n_holes[1]))
        elif isinstance(n_holes, (int, np.integer)) and not isinstance(n_holes, bool) and n_holes >= 0:
            n_holes = (int(n_holes), int(n_holes))
        else:
            raise ValueError(f'CutOut: n_holes={n_holes!r} must be a non-negative int or (a, b) with 0 <= a < b')
        if n_holes[1] > L.CUTOUT_MAX_HOLES:
            raise ValueError(f'CutOut: n_holes up to {n_holes[1]} exceeds the {L.CUTOUT_MAX_HOLES} holes per image of '
                             'this build (YUNET_CUTOUT_MAX_HOLES)')
        cands = cutout_ratio if with_ratio else cutout_shape
        if not isinstance(cands, (list, tuple)) or len(cands) == 0:
            raise ValueError(f'CutOut: {arg}={cands!r} must be one (w, h) pair or a list of pairs')
        if all(_is_number(v) for v in cands):       # one pair (the reference tells it from a list by the tuple type)
            cands = [cands]
        pairs = []
        for c in cands:
            if not isinstance(c, (list, tuple)) or len(c) != 2 or not all(_is_number(v) for v in c):
                raise ValueError(f'CutOut: {arg} entry {c!r} is not a (w, h) pair of numbers')
            if not all(math.isfinite(float(v)) and float(v) >= 0 for v in c):
                raise ValueError(f'CutOut: {arg} entry {c!r} must be non-negative and finite')
            if not with_ratio and not all(float(v) == int(v) for v in c):
                raise ValueError(f'CutOut: cutout_shape entry {c!r} must be whole pixels')
            pairs.append((float(c[0]), float(c[1])) if with_ratio else (int(c[0]), int(c[1])))
        if len(pairs) > L.CUTOUT_MAX_CANDIDATES:
            raise ValueError(f'CutOut: {arg} has {len(pairs)} candidates, this build takes at most '
                             f'{L.CUTOUT_MAX_CANDIDATES} (YUNET_CUTOUT_MAX_CANDIDATES)')
        fill = [fill_in] * 3 if _is_number(fill_in) else fill_in
        if not isinstance(fill, (list, tuple)) or len(fill) != 3 \
                or not all(_is_number(v) and math.isfinite(float(v)) for v in fill):
            raise ValueError(f'CutOut: fill_in={fill_in!r} must be a finite scalar or three finite values (B, G, R)')
        super().__init__(n_holes=n_holes, fill_in=fill_in, **{arg: cutout_ratio if with_ratio else cutout_shape})
        self.with_ratio, self.candidates, self.fill = with_ratio, pairs, tuple(float(v) for v in fill)

    def c_cfg(self, seed):
        c = L.YunetCutoutCfg()
        (c.n_lo, c.n_hi), c.n_cand, c.with_ratio = self.n_holes, len(self.candidates), int(self.with_ratio)
        for i, (w, h) in enumerate(self.candidates):
            c.cand[i][0], c.cand[i][1] = float(w), float(h)
        for i, v in enumerate(self.fill):
            c.fill[i] = v
        c.seed = seed & 0xFFFFFFFF
        return c


@PIPELINES.register_module()
class RandomAffine(_Carrier):
    """transforms.py:2787-3001 with the reference's constructor and one keyword more, `use_kps`, as the reference added
    it to Mosaic: the five landmarks go through the same matrix as the boxes.  Its assertions are ValueErrors here.  Runs
    as yunet_aug_affine_decide + yunet_aug_affine_pixels on the finished batch tensor and GT, after RandomFlip (or a POST
    PhotoMetricDistortion) and in front of CutOut / Normalize; its draws come from a sub-stream of the pipeline's
    generator (include/yunet_hip.h YUNET_AFFINE_SALT).  `border_val` is a scalar or three values in the image's channel
    order (BGR).  `border` stays (0, 0): the output keeps the input's size.  |max_shear_degree| stays below
    _lib.AFFINE_MAX_SHEAR, so that the matrix never mirrors the image (no left / right landmark swap is built)."""

    def __init__(self, max_rotate_degree=10.0, max_translate_ratio=0.1, scaling_ratio_range=(0.5, 1.5),
                 max_shear_degree=2.0, border=(0, 0), border_val=(114, 114, 114), min_bbox_size=2, min_area_ratio=0.2,
                 max_aspect_ratio=20, bbox_clip_border=True, skip_filter=True, use_kps=False):
        if not isinstance(scaling_ratio_range, (list, tuple)) or len(scaling_ratio_range) != 2:
            raise ValueError(f'RandomAffine: scaling_ratio_range={scaling_ratio_range!r} must be (min, max)')
        for name, v in (('max_rotate_degree', max_rotate_degree), ('max_translate_ratio', max_translate_ratio),
                        ('scaling_ratio_range', scaling_ratio_range[0]), ('scaling_ratio_range', scaling_ratio_range[1]),
                        ('max_shear_degree', max_shear_degree), ('min_bbox_size', min_bbox_size),
                        ('min_area_ratio', min_area_ratio), ('max_aspect_ratio', max_aspect_ratio)):
            if not _is_number(v) or not math.isfinite(float(v)):
                raise ValueError(f'RandomAffine: {name}={v!r} must be a finite number')
        if not 0 <= max_translate_ratio <= 1:
            raise ValueError(f'RandomAffine: max_translate_ratio={max_translate_ratio} must lie in [0, 1]')
        if not 0 < scaling_ratio_range[0] <= scaling_ratio_range[1]:
            raise ValueError(f'RandomAffine: scaling_ratio_range={tuple(scaling_ratio_range)} must have 0 < min <= max')
        if not abs(max_shear_degree) < L.AFFINE_MAX_SHEAR:
            raise ValueError(f'RandomAffine: max_shear_degree={max_shear_degree} must stay below {L.AFFINE_MAX_SHEAR} '
                             'degrees (YUNET_AFFINE_MAX_SHEAR): beyond it a draw can mirror the image')
        fill = [border_val] * 3 if _is_number(border_val) else border_val
        if not isinstance(fill, (list, tuple)) or len(fill) != 3 \
                or not all(_is_number(v) and math.isfinite(float(v)) for v in fill):
            raise ValueError(f'RandomAffine: border_val={border_val!r} must be a finite scalar or three finite values '
                             '(B, G, R)')
        if not isinstance(border, (list, tuple)) or len(border) != 2 or not all(_is_number(v) for v in border):
            raise ValueError(f'RandomAffine: border={border!r} must be two numbers')
        if tuple(border) != (0, 0):
            raise NotImplementedError(f'RandomAffine(border={tuple(border)}): the output keeps the input\'s size, '
                                      'border=(0, 0); the crop after Mosaic does here what border does in YOLOX')
        if not use_kps:
            raise NotImplementedError('RandomAffine(use_kps=False): the device pipeline always carries the five landmarks '
                                      '(LoadAnnotations(with_keypoints=True)); write use_kps=True')
        super().__init__(max_rotate_degree=max_rotate_degree, max_translate_ratio=max_translate_ratio,
                         scaling_ratio_range=tuple(scaling_ratio_range), max_shear_degree=max_shear_degree, border=(0, 0),
                         border_val=border_val, min_bbox_size=min_bbox_size, min_area_ratio=min_area_ratio,
                         max_aspect_ratio=max_aspect_ratio, bbox_clip_border=bool(bbox_clip_border),
                         skip_filter=bool(skip_filter), use_kps=True)
        self.fill = tuple(float(v) for v in fill)

    def c_cfg(self, seed, gmax):
        c = L.YunetAffineCfg()
        c.max_rotate_degree, c.max_translate_ratio = float(self.max_rotate_degree), float(self.max_translate_ratio)
        c.scale_lo, c.scale_hi = (float(v) for v in self.scaling_ratio_range)
        c.max_shear_degree = float(self.max_shear_degree)
        c.min_bbox_size, c.min_area_ratio = float(self.min_bbox_size), float(self.min_area_ratio)
        c.max_aspect_ratio = float(self.max_aspect_ratio)
        for i, v in enumerate(self.fill):
            c.border_val[i] = v
        c.bbox_clip_border, c.skip_filter, c.gmax, c.seed = int(self.bbox_clip_border), int(self.skip_filter), gmax, \
            seed & 0xFFFFFFFF
        return c


@PIPELINES.register_module()
class MixUp(_Carrier):
    """transforms.py:2523-2783 with the reference's constructor and one keyword more, `use_kps`, as the reference added
    it to Mosaic: the partner's five landmarks are scaled, flipped (left / right swapped) and shifted with its boxes.
    Runs as yunet_aug_mixup_decide + yunet_aug_mixup_pixels on the finished batch tensor and GT, after RandomFlip (a POST
    PhotoMetricDistortion, RandomAffine) and in front of CutOut / Normalize; the partner is a raw image of the device
    store with its raw GT (MultiImageMixDataset's mix_results); its draws come from a sub-stream of the pipeline's
    generator (include/yunet_hip.h YUNET_MIXUP_SALT).  Its assertions are ValueErrors here."""

    def __init__(self, img_scale=(640, 640), ratio_range=(0.5, 1.5), flip_ratio=0.5, pad_val=114, max_iters=15,
                 min_bbox_size=5, min_area_ratio=0.2, max_aspect_ratio=20, bbox_clip_border=True, skip_filter=True,
                 use_kps=False):
        if not use_kps:
            raise NotImplementedError('MixUp(use_kps=False): the device pipeline always carries the five landmarks '
                                      '(LoadAnnotations(with_keypoints=True)); write use_kps=True')
        if not isinstance(img_scale, (list, tuple)) or len(img_scale) != 2 or not all(_is_number(v) for v in img_scale):
            raise ValueError(f'MixUp: img_scale={img_scale!r} must be (height, width)')
        if int(img_scale[0]) != int(img_scale[1]):
            raise NotImplementedError(f'MixUp(img_scale={tuple(img_scale)}): only the square canvas '
                                      '(img_scale=(D, D)) is built; the rectangular one is not')
        D = int(img_scale[0])
        if not 1 <= D <= L.AUG_MAX_EDGE // 2:
            raise ValueError(f'MixUp(img_scale=({D}, {D})): D must lie in [1, {L.AUG_MAX_EDGE // 2}]')
        if isinstance(pad_val, (list, tuple)):
            raise ValueError(f'MixUp: pad_val={pad_val!r} must be one value (a per-channel pad is not built)')
        if not isinstance(ratio_range, (list, tuple)) or len(ratio_range) != 2:
            raise ValueError(f'MixUp: ratio_range={ratio_range!r} must be (min, max)')
        for name, v in (('ratio_range', ratio_range[0]), ('ratio_range', ratio_range[1]), ('flip_ratio', flip_ratio),
                        ('pad_val', pad_val), ('min_bbox_size', min_bbox_size), ('min_area_ratio', min_area_ratio),
                        ('max_aspect_ratio', max_aspect_ratio)):
            if not _is_number(v) or not math.isfinite(float(v)):
                raise ValueError(f'MixUp: {name}={v!r} must be a finite number')
        if not 0 < ratio_range[0] <= ratio_range[1]:
            raise ValueError(f'MixUp: ratio_range={tuple(ratio_range)} must have 0 < min <= max')
        if D * float(ratio_range[1]) >= 2 ** 30:
            raise ValueError(f'MixUp: ratio_range={tuple(ratio_range)} scales the {D} canvas beyond 2^30 pixels')
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or max_iters < 1:
            raise ValueError(f'MixUp: max_iters={max_iters!r} must be an integer >= 1')
        super().__init__(img_scale=(D, D), ratio_range=tuple(float(v) for v in ratio_range), flip_ratio=flip_ratio,
                         pad_val=pad_val, max_iters=int(max_iters), min_bbox_size=min_bbox_size,
                         min_area_ratio=min_area_ratio, max_aspect_ratio=max_aspect_ratio,
                         bbox_clip_border=bool(bbox_clip_border), skip_filter=bool(skip_filter), use_kps=True)

    def c_cfg(self, seed, gmax):
        c = L.YunetMixupCfg()
        (c.ratio_lo, c.ratio_hi), c.flip_ratio, c.pad_val = self.ratio_range, float(self.flip_ratio), float(self.pad_val)
        c.min_bbox_size, c.min_area_ratio = float(self.min_bbox_size), float(self.min_area_ratio)
        c.max_aspect_ratio, c.img_scale, c.max_iters = float(self.max_aspect_ratio), self.img_scale[0], self.max_iters
        c.bbox_clip_border, c.skip_filter, c.gmax, c.seed = int(self.bbox_clip_border), int(self.skip_filter), gmax, \
            seed & 0xFFFFFFFF
        return c


def _mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def mosaic_partners(seed, iteration, n, m):
    """The three partner indices yunet_aug_mosaic_decide draws for image n of `iteration` over a store of m images: the
    draws are a pure function of (seed, iteration, n), so the host computes them ahead (a lazily decoding source
    decodes the partners before the batch that uses them) instead of waiting for the device."""
    k = _mix32((seed & 0xFFFFFFFF) ^ ((iteration * 0x27D4EB2F) & 0xFFFFFFFF))
    k = _mix32(_mix32(k ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)) ^ L.MOSAIC_SALT)
    return [(_mix32(k ^ ((c * 0x85EBCA6B + 0xC2B2AE35) & 0xFFFFFFFF)) * m) >> 32 for c in range(3)]


def mixup_partner(seed, iteration, n, counts, max_iters):
    """The store index yunet_aug_mixup_decide settles on as the partner of image n of `iteration`, over a store whose
    image i has counts[i] GT rows: up to max_iters draws, stopping at the first image with boxes.  A pure function of
    (seed, iteration, n) and the counts, so the host computes it ahead, as it does Mosaic's partners."""
    k = _mix32((seed & 0xFFFFFFFF) ^ ((iteration * 0x27D4EB2F) & 0xFFFFFFFF))
    k = _mix32(_mix32(k ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)) ^ L.MIXUP_SALT)
    i = 0
    for c in range(max_iters):
        i = (_mix32(k ^ ((c * 0x85EBCA6B + 0xC2B2AE35) & 0xFFFFFFFF)) * len(counts)) >> 32
        if counts[i] != 0:
            break
    return i


@PIPELINES.register_module()
class Normalize(_Carrier):
    def __init__(self, mean, std, to_rgb=True):
        if any(float(m) != 0.0 for m in mean) or any(float(s) != 1.0 for s in std) or to_rgb:
            raise NotImplementedError('the YuNet configs feed raw 0-255 BGR (mean 0, std 1, to_rgb=False)')
        super().__init__(mean=list(mean), std=list(std), to_rgb=to_rgb)


@PIPELINES.register_module()
class DefaultFormatBundle(_Carrier):
    def __init__(self, **kw):
        super().__init__()


@PIPELINES.register_module()
class Collect(_Carrier):
    def __init__(self, keys, meta_keys=None):
        super().__init__(keys=list(keys))


class DeviceGT(GTList):
    """GT of a device-augmented batch: `padded` [N, Gmax, ...] and `counts` [N] live on the device
    (what the loss step stages directly); the list items are the padded per-image views -- rows at
    or beyond counts[i] are zero."""


class StoreView:
    """Device tables of a decoded-source store of m images (what yunet_aug_gather reads): byte offsets int64 [m],
    (h, w) int32 [m,2], first GT row / GT count int32 [m], boxes fp32 [*,4], kps fp32 [*,15].  Optional, with ignore
    boxes in the store: first ignore row / ignore count int32 [m] and ign_boxes fp32 [*,4]."""

    def __init__(self, m, off, hw, goff, gcnt, boxes, kps, ioff=None, icnt=None, ign_boxes=None):
        self.m, self.off, self.hw, self.goff, self.gcnt, self.boxes, self.kps = int(m), off, hw, goff, gcnt, boxes, kps
        self.ioff, self.icnt, self.ign_boxes = ioff, icnt, ign_boxes


class SourceBatch:
    """A batch of decoded source images and their annotations, resident on the device:
    src uint8 (concatenated HWC images), src_off int64 [N], src_hw int32 [N,2],
    boxes fp32 [sum G,4], kps fp32 [sum G,5,3], gt_off int32 [N+1].
    Optional (gt_bboxes_ignore; DevicePipeline(ignore_rows=...)): ign_boxes fp32 [sum I,4], ign_off int32 [N+1].
    `view` / `idx` (Mosaic): the tables of the whole store the batch was picked from (StoreView, every image in `src`)
    and the batch's store indices, int32 [N] on the device; a batch made by from_lists is its own store."""

    def __init__(self, src, src_off, src_hw, boxes, kps, gt_off, view=None, idx=None, ign_boxes=None, ign_off=None):
        self.src, self.src_off, self.src_hw = src, src_off, src_hw
        self.boxes, self.kps, self.gt_off = boxes, kps, gt_off
        self.ign_boxes, self.ign_off = ign_boxes, ign_off
        self.n = int(src_hw.shape[0])
        self.view, self.idx = view, idx

    def store_view(self):
        """-> (StoreView, idx) addressing any image of the store.  Without a store: the batch itself, M = N."""
        if self.view is None:
            if self.src.device.type != 'cuda':
                return None, None
            goff = self.gt_off[:-1].contiguous()
            self.view = StoreView(self.n, self.src_off, self.src_hw, goff, (self.gt_off[1:] - goff).contiguous(),
                                  self.boxes, self.kps.reshape(-1, 15))
            self.idx = torch.arange(self.n, dtype=torch.int32, device=self.src.device)
        return self.view, self.idx

    @classmethod
    def from_lists(cls, images, gt_bboxes, gt_keypointss, device, gt_bboxes_ignore=None):
        """images: list of uint8 [h, w, 3] arrays / tensors (BGR as decoded); gt lists per image; gt_bboxes_ignore: a list
        of [I,4] arrays per image (None: the batch carries no ignore tables)."""
        imgs = [np.ascontiguousarray(np.asarray(im.cpu() if torch.is_tensor(im) else im, dtype=np.uint8))
                for im in images]
        for im in imgs:
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError('source images must be uint8 [h, w, 3]')
        sizes = np.array([im.size for im in imgs], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs]))
        hw = torch.tensor([[im.shape[0], im.shape[1]] for im in imgs], dtype=torch.int32)
        cnt = [int(np.asarray(b).shape[0]) for b in gt_bboxes]
        goff = torch.tensor(np.concatenate([[0], np.cumsum(cnt)]), dtype=torch.int32)
        tot = max(1, sum(cnt))
        boxes = torch.zeros(tot, 4)
        kps = torch.zeros(tot, 5, 3)
        if sum(cnt):
            boxes[:sum(cnt)] = torch.cat([torch.as_tensor(np.asarray(b), dtype=torch.float32).reshape(-1, 4)
                                          for b in gt_bboxes])
            kps[:sum(cnt)] = torch.cat([torch.as_tensor(np.asarray(k), dtype=torch.float32).reshape(-1, 5, 3)
                                        for k in gt_keypointss])
        d = torch.device(device)
        ign = {}
        if gt_bboxes_ignore is not None:
            if len(gt_bboxes_ignore) != len(imgs):
                raise ValueError(f'gt_bboxes_ignore: {len(gt_bboxes_ignore)} entries for {len(imgs)} images')
            ib, io = ragged_ignore(gt_bboxes_ignore)
            ign = dict(ign_boxes=torch.from_numpy(ib).to(d), ign_off=torch.from_numpy(io).to(d))
        return cls(src.to(d), torch.from_numpy(off).to(d), hw.to(d), boxes.to(d), kps.to(d), goff.to(d), **ign)


def ragged_ignore(per_image):
    """list of [I_i,4] arrays -> (boxes fp32 [max(1, sum I),4], off int32 [N+1]) on the host."""
    rows = [np.asarray(b.cpu() if torch.is_tensor(b) else b, dtype=np.float32).reshape(-1, 4) for b in per_image]
    off = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int32)
    boxes = np.concatenate(rows + [np.zeros((0 if off[-1] else 1, 4), np.float32)]).astype(np.float32)
    return np.ascontiguousarray(boxes), off


IGNORE_ROWS_MIN, IGNORE_ROWS_MAX = L.IGNORE_MIN_ROWS, L.IGNORE_MAX_BOXES


def ignore_capacity_rows(capacity):
    """Padded ignore rows per image for a capacity of `capacity` boxes: the smallest power of two >= max(capacity, 16),
    at most 1024 (what yunet_ignore_mark stages in LDS)."""
    if isinstance(capacity, bool) or int(capacity) != capacity or int(capacity) < 0:
        raise ValueError(f'an ignore capacity is an integer >= 0, got {capacity!r}')
    return K.ignore_capacity_rows(capacity)


MOSAIC_MAX_GT = 1024        # GT rows per image the engine's assign kernels are tested to
GT_ROWS_MIN = 64            # the default padded width; a capacity never goes below it
GT_ROWS_MAX = 4096          # yunet_assign_cfg stages Gmax 16-byte GT records in at most 64 KB of LDS


def gt_capacity_rows(max_count, mosaic=False, mixup=False):
    """Padded GT rows per source image for a capacity of `max_count` faces: the smallest power of two that is
    >= max(max_count, 64).  mosaic=True: at most MOSAIC_MAX_GT // 4, since the merged GT of four images has to stay
    within MOSAIC_MAX_GT rows (a larger image can then truncate a merged canvas, status 2).  mixup=True: MixUp appends
    one more image's rows, so the divisor is 5 with Mosaic and 2 without."""
    if isinstance(max_count, bool) or int(max_count) != max_count or int(max_count) < 1:
        raise ValueError(f'a GT capacity is an integer >= 1, got {max_count!r}')
    rows = GT_ROWS_MIN
    while rows < int(max_count):
        rows *= 2
    if mosaic or mixup:
        return min(rows, MOSAIC_MAX_GT // ((4 if mosaic else 1) + (1 if mixup else 0)))
    if rows > GT_ROWS_MAX:
        raise ValueError(f'a GT capacity of {int(max_count)} faces needs {rows} padded rows: the assign launch stages its '
                         f'GT rows in LDS and takes at most {GT_ROWS_MAX} (64 KB at 16 bytes a row)')
    return rows


def _ptr(t):
    """Device address of a tensor (None: NULL), as a c_void_p argument or descriptor field takes it."""
    return t.data_ptr() if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class DevicePipeline:
    """Builds from the reference's pipeline list and runs it as two kernel launches per batch."""

    ORDER = ['LoadImageFromFile', 'LoadAnnotations', 'RandomSquareCrop', 'Resize', 'RandomFlip',
             'Normalize', 'DefaultFormatBundle', 'Collect']
    # PhotoMetricDistortion may stand, once, at one of two places of ORDER: before index 2 (pre: on the source image,
    # the crop's pad fill is not distorted) or before index 5 (post: on the resized, flipped image, pad included)
    PHOTO_POSITIONS = {2: L.PHOTO_PRE, 5: L.PHOTO_POST}

    def __init__(self, pipeline, seed=0, gmax=64, pad_value=128.0, max_attempts=250, max_retries=64, ignore_rows=None):
        steps = [build_from_cfg(p, PIPELINES) if isinstance(p, dict) else p for p in pipeline]
        names = [type(s).__name__ for s in steps]
        # ignore boxes (gt_bboxes_ignore): None = off -- nothing is allocated or launched, the batch has no new key.
        # Otherwise the padded rows per image of batch['gt_bboxes_ignore'] (ignore_capacity_rows); one more launch,
        # yunet_aug_ignore, behind the decide.  It draws nothing: every other output keeps its bytes.
        self.ignore_rows = None
        if ignore_rows is not None:
            self.ignore_rows = ignore_capacity_rows(ignore_rows)
            if self.ignore_rows != int(ignore_rows):
                raise ValueError(f'ignore_rows={ignore_rows}: a power of two in [{IGNORE_ROWS_MIN}, {IGNORE_ROWS_MAX}] '
                                 '(pipelines.ignore_capacity_rows)')
            for step, why in (('Mosaic', "the reference's Mosaic drops ignore boxes itself"),
                              ('RandomAffine', 'ignore boxes through its matrix are not built yet'),
                              ('MixUp', "the reference's MixUp drops ignore boxes itself")):
                if step in names:
                    raise NotImplementedError(f'{step} together with ignore_capacity (ignore boxes in the batch): {why}')
        self.mixup, self.mixup_cfg, self.mixup_table, self._skip = None, None, None, frozenset()
        if 'MixUp' in names:
            at = names.index('MixUp')
            before = names[at - 1] if at else None
            if before == 'PhotoMetricDistortion' and names[max(at - 2, 0)] != 'RandomFlip':
                before = None
            if names.count('MixUp') > 1 or before not in ('RandomFlip', 'PhotoMetricDistortion', 'RandomAffine') \
                    or names[at + 1:at + 2] not in (['CutOut'], ['Normalize']):
                raise NotImplementedError(
                    'DevicePipeline runs MixUp once, after RandomFlip (after a PhotoMetricDistortion that follows '
                    'RandomFlip, and after RandomAffine if there is one) and immediately in front of CutOut or Normalize; '
                    f'got {names}')
            self.mixup = steps[at]          # its configuration is made below, once the GT rows per image are known
            steps, names = steps[:at] + steps[at + 1:], names[:at] + names[at + 1:]
        self.affine, self.affine_cfg, self.affine_table = None, None, None
        if 'RandomAffine' in names:
            at = names.index('RandomAffine')
            before = names[at - 1] if at else None
            if before == 'PhotoMetricDistortion' and names[max(at - 2, 0)] != 'RandomFlip':
                before = None
            if names.count('RandomAffine') > 1 or before not in ('RandomFlip', 'PhotoMetricDistortion') \
                    or names[at + 1:at + 2] not in (['CutOut'], ['Normalize']):
                raise NotImplementedError(
                    'DevicePipeline runs RandomAffine once, after RandomFlip (and after a PhotoMetricDistortion that '
                    f'follows RandomFlip) and immediately in front of CutOut or Normalize; got {names}')
            self.affine = steps[at]         # its configuration is made below, once the GT rows per image are known
            steps, names = steps[:at] + steps[at + 1:], names[:at] + names[at + 1:]
        self.cutout, self.cutout_cfg, self.cutout_holes = None, None, None
        if 'CutOut' in names:
            at = names.index('CutOut')
            if names.count('CutOut') > 1 or at == 0 or names[at + 1:at + 2] != ['Normalize'] \
                    or names[at - 1] not in ('RandomFlip', 'PhotoMetricDistortion'):
                raise NotImplementedError(
                    'DevicePipeline runs CutOut once, immediately in front of Normalize (after RandomFlip and after a '
                    f'PhotoMetricDistortion that follows RandomFlip); got {names}')
            self.cutout = steps[at]
            steps, names = steps[:at] + steps[at + 1:], names[:at] + names[at + 1:]
            self.cutout_cfg = self.cutout.c_cfg(seed)
        self.mosaic, self.mosaic_cfg, self.geom = None, None, None
        if 'Mosaic' in names:
            at = names.index('Mosaic')
            if names.count('Mosaic') > 1:
                raise NotImplementedError(f'DevicePipeline runs one Mosaic, got {names.count("Mosaic")} in {names}')
            if at == 0 or at + 1 >= len(names) or names[at - 1] != 'LoadAnnotations' \
                    or names[at + 1] not in ('RandomSquareCrop', 'PhotoMetricDistortion'):
                raise NotImplementedError('DevicePipeline runs Mosaic at one place, between LoadAnnotations and '
                                          f'RandomSquareCrop; got {names}')
            if names[at + 1] == 'PhotoMetricDistortion':
                raise NotImplementedError(
                    'PhotoMetricDistortion between Mosaic and RandomSquareCrop would distort the mosaic canvas, its '
                    'pad pixels included; that form is not built -- place it between RandomFlip and Normalize')
            if 4 * gmax > MOSAIC_MAX_GT:
                raise ValueError(f'Mosaic merges four images: gmax={gmax} gives {4 * gmax} GT rows per image, more than '
                                 f'the {MOSAIC_MAX_GT} the assignment kernels are tested to')
            self.mosaic = steps[at]
            steps, names = steps[:at] + steps[at + 1:], names[:at] + names[at + 1:]
        # one capacity for the whole pipeline: the rows of the merged GT and of the batch's padded GT
        rows = (4 if self.mosaic is not None else 1) * gmax + (gmax if self.mixup is not None else 0)
        if self.mixup is not None and rows > MOSAIC_MAX_GT:
            raise ValueError(f'MixUp appends one more image\'s rows{" to the four Mosaic merges" if self.mosaic else ""}: '
                             f'gmax={gmax} gives {rows} GT rows per image, more than the {MOSAIC_MAX_GT} the '
                             'assignment kernels are tested to')
        gmax = rows
        if self.mosaic is not None:
            self.mosaic_cfg = self.mosaic.c_cfg(seed, gmax)
        self.photo, self.photo_position, self.pparams = None, L.PHOTO_NONE, None
        if 'PhotoMetricDistortion' in names:
            at = names.index('PhotoMetricDistortion')
            rest = names[:at] + names[at + 1:]
            if names.count('PhotoMetricDistortion') > 1 or rest != self.ORDER or at not in self.PHOTO_POSITIONS:
                raise NotImplementedError(
                    'DevicePipeline runs PhotoMetricDistortion once, either between LoadAnnotations and '
                    'RandomSquareCrop (pre) or between RandomFlip and Normalize (post), in the list '
                    f'{self.ORDER}; got {names}')
            self.photo, self.photo_position = steps[at], self.PHOTO_POSITIONS[at]
            steps = steps[:at] + steps[at + 1:]
            names = rest
        if names != self.ORDER:
            raise NotImplementedError(f'DevicePipeline implements exactly {self.ORDER} (with an optional '
                                      'PhotoMetricDistortion before RandomSquareCrop or after RandomFlip and an '
                                      f'optional Mosaic before RandomSquareCrop); got {names}')
        self.steps = steps
        by = dict(zip(names, steps))
        if not by['LoadAnnotations'].with_keypoints:
            raise NotImplementedError('LoadAnnotations(with_keypoints=True) is required')
        # fixed size: out_size = S, out_sizes = [S].  square_range: out_size is None (there is no one size) and
        # out_sizes lists the S_n an image can draw, the multiples of 32 in [lo // 32 * 32, hi // 32 * 32]
        self.scale_range = by['Resize'].scale_range
        if self.scale_range is None:
            self.out_size = by['Resize'].img_scale[0]
            if self.out_size % 32:
                raise ValueError('Resize img_scale must be a multiple of 32 for the YuNet stack')
            self.out_sizes = [self.out_size]
        else:
            lo, hi = self.scale_range
            self.out_size = None
            self.out_sizes = list(range(lo // 32 * 32, hi // 32 * 32 + 1, 32))
        self.sizes = None            # square_range: S_n of the last batch (host int32 [N])
        choice = by['RandomSquareCrop'].crop_choice
        if not 1 <= len(choice) <= 8:
            raise NotImplementedError('crop_choice must have 1..8 entries')
        cfg = L.YunetAugCfg()
        cfg.out_size, cfg.n_choice = self.out_size or self.out_sizes[-1], len(choice)    # out_size: unused under square_range
        for i, c in enumerate(choice):
            cfg.crop_choice[i] = c
        cfg.flip_ratio, cfg.pad_value, cfg.seed = by['RandomFlip'].flip_ratio, pad_value, seed & 0xFFFFFFFF
        cfg.max_attempts, cfg.max_retries, cfg.gmax = max_attempts, max_retries, gmax
        self.cfg = cfg
        self.photo_cfg = self.photo.c_cfg(self.photo_position) if self.photo is not None else None
        self.gmax = gmax
        if self.affine is not None:
            self.affine_cfg = self.affine.c_cfg(seed, gmax)
        if self.mixup is not None:
            self.mixup_cfg = self.mixup.c_cfg(seed, gmax)
        self.params = None
        self._pixels = L.YunetAugPixels()       # the pixel pass's descriptor: the per-batch fields are filled in place
        self._pixels.position = self.photo_position
        self._mosaic_ptr = C.pointer(self.mosaic_cfg) if self.mosaic is not None else None

    SKIP_TYPE_KEYS = ('Mosaic', 'RandomAffine', 'MixUp')

    def update_skip_type_keys(self, skip_type_keys):
        """MultiImageMixDataset.update_skip_type_keys (dataset_wrappers.py:446-456): the named steps launch nothing from
        the next batch on.  Every step draws from a sub-stream of its own, so the batch is then, byte for byte, that of
        a pipeline built without them at the same seed and iteration; the padded GT keeps the capacity this pipeline
        was built with (the engine keeps its plan).  A name this pipeline does not hold is accepted, as by the
        reference; a name outside SKIP_TYPE_KEYS is not a step that can be switched off here."""
        assert all(isinstance(k, str) for k in skip_type_keys)
        bad = [k for k in skip_type_keys if k not in self.SKIP_TYPE_KEYS]
        if bad:
            raise NotImplementedError(f'skip_type_keys {bad}: the steps that can be switched off are {self.SKIP_TYPE_KEYS}')
        self._skip = frozenset(skip_type_keys)

    def _on(self, name):
        return getattr(self, name.lower() if name != 'RandomAffine' else 'affine') is not None and name not in self._skip

    def __call__(self, src, iteration, sizes=None):
        dev = src.src.device
        if dev.type != 'cuda':
            raise RuntimeError('DevicePipeline needs device-resident sources: HIP kernels only, no CPU fallback')
        mosaic, mixup = self._on('Mosaic'), self._on('MixUp')
        if not mosaic and not mixup:
            return self._run(src, iteration, dev, (src.src, src.src_off, None), sizes)
        view, idx = src.store_view()
        if view is None or idx is None:
            raise NotImplementedError(f'{"Mosaic" if mosaic else "MixUp"} needs sources that are resident on the device')
        pix = (src.src, view.off, None) if mosaic else (src.src, src.src_off, None)
        return self._run(src, iteration, dev, pix, sizes, store=(view, idx))

    def _run(self, src, iteration, dev, pix, sizes, store=None):
        """One batch on the current stream: decide -> sizes -> allocate -> photometric table -> pixel pass -> collate.
        `pix` = (buffer, offsets, rect), where the pixel pass reads: whole sources (rect None), a window buffer with its
        plan, or -- Mosaic, `store` = (StoreView, the batch's store indices) -- the whole store with its offset table.
        Mosaic: yunet_aug_mosaic_decide (partners, geometry, merged GT) comes first; the decide then runs on the merged
        GT with the canvas as its source image and the pixel pass resolves its taps through the geometry table.
        square_range: the batch is the [N, 3, Smax, Smax] canvas.  Image n sits in the top-left S_n x S_n corner, the
        rest is 0: DefaultFormatBundle wraps the image with padding_value=0, stack=True (formatting.py:202, 231) and
        mmcv's collate pads a group's images at the bottom and right up to the largest.  The value and the stacking are
        the reference's; the bottom / right placement is mmcv's rule, restated here without mmcv at hand."""
        n = src.n
        merged = self._mosaic_decide(store, n, iteration, dev) if self._on('Mosaic') else None
        if merged is None:
            self.geom = None
        gb, gk, cnt, params = self._decide(src, iteration, dev, merged)
        ign = self._ignore(src, params, dev) if self.ignore_rows is not None else None
        out_hw = 0
        if self.scale_range is not None:
            sizes = np.asarray(self.read_sizes(params) if sizes is None else sizes, dtype=np.int32)
            if sizes.shape != (n,) or not all(int(s) in self.out_sizes for s in sizes):
                raise RuntimeError(f'square_range sizes {sizes.tolist()} are not the S_n of this pipeline '
                                   f'({self.out_sizes})')
            self.sizes = sizes
            out_hw = int(sizes.max())
        edge = out_hw or self.out_size
        img = torch.empty(n, 3, edge, edge, device=dev, dtype=torch.float32)
        pp = self._photometric(n, iteration, dev) if self.photo is not None else None
        a = self._pixels            # position / mosaic were set with the configuration
        a.src, a.src_off, a.rect = (_ptr(t) for t in pix)
        a.src_hw, a.params, a.pparams = _ptr(src.src_hw if merged is None else merged[3]), _ptr(params), _ptr(pp)
        a.geom, a.out_hw = _ptr(self.geom if merged is not None else None), out_hw
        a.mosaic = self._mosaic_ptr if merged is not None else None
        L.check(L.load().yunet_aug_pixels(C.byref(a), C.byref(self.cfg), n, _ptr(img), _stream()), 'yunet_aug_pixels')
        self.affine_table, self.mixup_table = None, None        # a step that is skipped writes no table
        if self._on('RandomAffine'):
            img, gb, gk, cnt = self._affine(img, gb, gk, cnt, params if out_hw else None, iteration, dev)
        if self._on('MixUp'):
            gb, gk, cnt = self._mixup(store, src, img, gb, gk, cnt, params if out_hw else None, iteration, dev)
        if self.cutout is not None:
            self._cutout(img, params if out_hw else None, iteration, dev)
        return self._collate(img, gb, gk, cnt, params, dev, ign)

    def _ignore(self, src, params, dev):
        """yunet_aug_ignore on the current stream, behind the decide -> (padded ignore boxes [N,rows,4], counts [N]).  A
        source without ignore tables stands for no ignore box at all."""
        n, rows = src.n, self.ignore_rows
        ob = torch.empty(n, rows, 4, device=dev, dtype=torch.float32)
        oc = torch.empty(n, device=dev, dtype=torch.int32)
        off = src.ign_off if src.ign_off is not None else torch.zeros(n + 1, device=dev, dtype=torch.int32)
        L.check(L.load().yunet_aug_ignore(_ptr(params), _ptr(src.ign_boxes), _ptr(off), self.cfg.out_size, n, rows, _ptr(ob),
                                          _ptr(oc), _stream()), 'yunet_aug_ignore')
        return ob, oc

    def _affine(self, img, gb, gk, cnt, params, iteration, dev):
        """yunet_aug_affine_decide + yunet_aug_affine_pixels on the current stream -> (warped batch tensor, boxes,
        keypoints, counts): the warp cannot run in place, so each is a new tensor.  `params` as for _cutout.  The table
        [N, AFFINE_WORDS] float64 (draws, M, its inverse, rows before / after, edge) stays in `affine_table`."""
        n, edge = int(img.shape[0]), int(img.shape[-1])
        table = torch.empty(n, L.AFFINE_WORDS, device=dev, dtype=torch.float64)
        ob, ok, oc, out = torch.empty_like(gb), torch.empty_like(gk), torch.empty_like(cnt), torch.empty_like(img)
        lib, c = L.load(), self.affine_cfg
        L.check(lib.yunet_aug_affine_decide(C.byref(c), int(iteration) & 0xFFFFFFFF, n, edge, _ptr(params), _ptr(gb),
                                            _ptr(gk), _ptr(cnt), _ptr(ob), _ptr(ok), _ptr(oc), _ptr(table), _stream()),
                'yunet_aug_affine_decide')
        L.check(lib.yunet_aug_affine_pixels(_ptr(table), C.byref(c.border_val), n, edge, _ptr(params), _ptr(img),
                                            _ptr(out), _stream()), 'yunet_aug_affine_pixels')
        self.affine_table = table
        return out, ob, ok, oc

    def _mixup(self, store, src, img, gb, gk, cnt, params, iteration, dev):
        """yunet_aug_mixup_decide + yunet_aug_mixup_pixels on the current stream -> (boxes, keypoints, counts): the blend
        runs in place on the batch tensor, the GT goes into new tensors.  `store` = (StoreView, batch indices): the
        partner is any image of the store; `src.src` holds the store's pixels.  `params` as for _cutout.  The table
        [N, MIXUP_WORDS] float64 stays in `mixup_table`."""
        view, _ = store
        n, edge = int(img.shape[0]), int(img.shape[-1])
        table = torch.empty(n, L.MIXUP_WORDS, device=dev, dtype=torch.float64)
        ob, ok, oc = torch.empty_like(gb), torch.empty_like(gk), torch.empty_like(cnt)
        lib, c = L.load(), self.mixup_cfg
        L.check(lib.yunet_aug_mixup_decide(C.byref(c), int(iteration) & 0xFFFFFFFF, n, edge, _ptr(params), view.m,
                                           _ptr(view.hw), _ptr(view.goff), _ptr(view.gcnt), _ptr(view.boxes),
                                           _ptr(view.kps), _ptr(gb), _ptr(gk), _ptr(cnt), _ptr(ob), _ptr(ok), _ptr(oc),
                                           _ptr(table), _stream()), 'yunet_aug_mixup_decide')
        L.check(lib.yunet_aug_mixup_pixels(_ptr(table), c.img_scale, c.pad_val, n, edge, _ptr(params), view.m,
                                           _ptr(src.src), _ptr(view.off), _ptr(view.hw), _ptr(img), _stream()),
                'yunet_aug_mixup_pixels')
        self.mixup_table = table
        return ob, ok, oc

    def _cutout(self, img, params, iteration, dev):
        """yunet_aug_cutout on the current stream, in place on the batch tensor; `params`: the decide's table on a
        multi-scale canvas (the kernel reads each image's S_n from it), None at the fixed size.  The hole table
        [N, CUTOUT_WORDS] int32 stays in `cutout_holes`."""
        n, edge = int(img.shape[0]), int(img.shape[-1])
        holes = torch.empty(n, L.CUTOUT_WORDS, device=dev, dtype=torch.int32)
        L.check(L.load().yunet_aug_cutout(C.byref(self.cutout_cfg), int(iteration) & 0xFFFFFFFF, n, edge, _ptr(params),
                                          _ptr(img), _ptr(holes), _stream()), 'yunet_aug_cutout')
        self.cutout_holes = holes

    def _mosaic_decide(self, store, n, iteration, dev):
        """yunet_aug_mosaic_decide on the current stream -> merged = (boxes, keypoints, counts, hw): the merged GT,
        padded to gmax rows, and the size of each image's canvas (its own size when the mosaic was skipped)."""
        view, idx = store
        gm = self.gmax
        geom = torch.empty(n, L.MOSAIC_WORDS, device=dev, dtype=torch.int32)
        hw = torch.empty(n, 2, device=dev, dtype=torch.int32)
        mb = torch.empty(n, gm, 4, device=dev, dtype=torch.float32)
        mk = torch.empty(n, gm, 5, 3, device=dev, dtype=torch.float32)
        mc = torch.empty(n, device=dev, dtype=torch.int32)
        L.check(L.load().yunet_aug_mosaic_decide(
            _ptr(idx), n, view.m, _ptr(view.hw), _ptr(view.goff), _ptr(view.gcnt), _ptr(view.boxes), _ptr(view.kps),
            C.byref(self.mosaic_cfg), int(iteration) & 0xFFFFFFFF, _ptr(geom), _ptr(hw), _ptr(mb), _ptr(mk), _ptr(mc),
            _stream()), 'yunet_aug_mosaic_decide')
        self.geom, self.merged = geom, (mb, mk, mc, hw)
        return self.merged

    def _photometric(self, n, iteration, dev):
        """yunet_aug_photometric on the current stream, keyed like _decide -> the table [N, PHOTO_WORDS] fp32."""
        pp = torch.empty(n, L.PHOTO_WORDS, device=dev, dtype=torch.float32)
        L.check(L.load().yunet_aug_photometric(C.byref(self.photo_cfg), self.cfg.seed, int(iteration) & 0xFFFFFFFF, n,
                                               _ptr(pp), _stream()), 'yunet_aug_photometric')
        self.pparams = pp
        return pp

    def _decide(self, src, iteration, dev, merged=None):
        """yunet_aug_decide on the current stream -> (padded boxes, padded keypoints, counts, params).  The GT is src's
        ragged lists, or `merged` of _mosaic_decide: padded to gmax rows, its hw taking the place of the source sizes."""
        n = src.n
        gb = torch.empty(n, self.gmax, 4, device=dev, dtype=torch.float32)
        gk = torch.empty(n, self.gmax, 5, 3, device=dev, dtype=torch.float32)
        cnt = torch.empty(n, device=dev, dtype=torch.int32)
        params = torch.empty(n, 8, device=dev, dtype=torch.int32)
        if merged is None:
            boxes, kps, idx, hw, in_gmax = src.boxes, src.kps, src.gt_off, src.src_hw, 0
        else:
            boxes, kps, idx, hw, in_gmax = *merged, self.gmax
        lo, hi = self.scale_range or (0, 0)
        L.check(L.load().yunet_aug_decide(_ptr(hw), _ptr(boxes), _ptr(kps), _ptr(idx), in_gmax, C.byref(self.cfg),
                                          int(self.scale_range is not None), lo, hi, int(iteration) & 0xFFFFFFFF, n,
                                          _ptr(params), _ptr(gb), _ptr(gk), _ptr(cnt), _stream()), 'yunet_aug_decide')
        return gb, gk, cnt, params

    def read_sizes(self, params):
        """square_range: S_n [N] (params[:, 7]) on the host.  The batch tensor is [N, 3, max S_n, max S_n], so the host
        has to know the sizes before it can allocate: one N-word copy that waits for the decide kernel on the current
        stream (and for nothing else on the device).  WindowFeed makes this copy with its plan, iterations ahead, and
        hands the result to `windowed(sizes=...)`."""
        return params[:, 7].cpu().numpy()

    def _collate(self, img, gb, gk, cnt, params, dev, ign=None):
        n, S = img.shape[0], self.out_size
        self.params = params
        boxes, kps = DeviceGT(list(gb)), DeviceGT(list(gk))
        boxes.padded, boxes.counts = gb, cnt
        kps.padded, kps.counts = gk, cnt
        labels = GTList([torch.zeros(self.gmax, dtype=torch.int64, device=dev)] * n)
        if self.scale_range is not None:      # mmdet's Resize sets img_shape = pad_shape; collate leaves metas alone
            smax = int(img.shape[-1])
            metas = [dict(img_shape=(int(s), int(s), 3), pad_shape=(int(s), int(s), 3), batch_input_shape=(smax, smax))
                     for s in self.sizes]
        else:
            metas = [dict(img_shape=(S, S, 3), pad_shape=(S, S, 3), batch_input_shape=(S, S)) for _ in range(n)]
        out = dict(img=img, img_metas=metas, gt_bboxes=boxes, gt_labels=labels, gt_keypointss=kps)
        if ign is not None:      # the multi-scale canvas keeps image n in its top-left corner: the coordinates stand as they are
            out['gt_bboxes_ignore'] = DeviceGT(list(ign[0]))
            out['gt_bboxes_ignore'].padded, out['gt_bboxes_ignore'].counts = ign
        return out

    def window_plan(self, src, iteration, dev):
        """The source rectangles this pipeline's pixel pass will read at `iteration` (aug_decide is keyed by
        (seed, iteration, image), so this can run ahead of the iteration): -> (params [N,8], rect [N,4] int32
        (row0, col0, rows, cols), win_off [N+1] int64 byte offsets of a compact window buffer, win_off[N] = total).
        Runs on the current stream; `src` needs only src_hw / boxes / kps / gt_off on the device."""
        self.require_resident('a window plan')
        _, _, _, params = self._decide(src, iteration, dev)
        rect = torch.empty(src.n, 4, device=dev, dtype=torch.int32)
        off = torch.empty(src.n + 1, device=dev, dtype=torch.int64)
        L.check(L.load().yunet_aug_window_plan(_ptr(params), _ptr(src.src_hw), src.n, _ptr(rect), _ptr(off), _stream()),
                'yunet_aug_window_plan')
        return params, rect, off

    def windowed(self, src, iteration, win, rect, win_off, sizes=None):
        """The pipeline on a compact window buffer `win` (uint8, device) holding, at win_off[n], the rectangle
        rect[n] of image n (window_plan of the same iteration): bit-identical to __call__ on the full sources.
        square_range: `sizes` = params[:, 7] of that plan, already on the host (else read_sizes waits here)."""
        self.require_resident('a window buffer')
        dev = win.device
        if dev.type != 'cuda':
            raise RuntimeError('DevicePipeline needs a device-resident window buffer: HIP kernels only')
        return self._run(src, iteration, dev, (win, win_off, rect), sizes)

    def require_resident(self, what):
        """Mosaic reads four images of the store per output image; a feed that brings only the batch's own pixels (or
        windows of them) to the device cannot serve it."""
        for step, name in ((self.mosaic, 'Mosaic'), (self.mixup, 'MixUp')):
            if step is not None:
                raise NotImplementedError(f'{name} over {what}: the partner images\' pixels are not on the device; use '
                                          "resident sources (SourceStore(placement='device'), cache='device')")

    def check_plan_cache(self, max_plans=None):
        """square_range walks len(out_sizes) batch geometries, one engine plan each; beyond engine.MAX_PLANS every
        new geometry evicts a plan, and an eviction drains the device (Engine.get_plan)."""
        if max_plans is None:
            from . import engine
            max_plans = engine.MAX_PLANS
        if len(self.out_sizes) > max_plans:
            lo, hi = self.scale_range
            raise ValueError(f"Resize(img_scale=({lo}, {hi}), multiscale_mode='square_range') draws {len(self.out_sizes)} "
                             f'batch sizes but the engine keeps {max_plans} plans: narrow the range or set '
                             f'YUNET_MAX_PLANS >= {len(self.out_sizes)} in the environment')

    def check(self):
        """Synchronising status check of the last batch: raises like the reference would misbehave
        (it loops forever on an image whose boxes no crop window can contain)."""
        st = self.params[:, 6].cpu()
        if self.geom is not None:           # merged GT beyond gmax is truncated like the crop's: the same status
            ms = self.geom[:, L.MOSAIC_STATUS].cpu()
            empty = ((ms & 4) != 0).nonzero().flatten().tolist()
            if empty:
                raise ValueError(f'Mosaic: a sub-image of images {empty} resizes to an empty size (img_scale too small '
                                 'for its aspect ratio)')
            st = torch.where((st == 0) & ((ms & 2) != 0), torch.full_like(st, 2), st)
        if self.mixup_table is not None:    # and so are rows beyond it after MixUp appended the partner's
            xs = self.mixup_table[:, L.MIXUP_STATUS].cpu().to(torch.int64)
            empty = ((xs & 4) != 0).nonzero().flatten().tolist()
            if empty:
                raise ValueError(f'MixUp: the partner of images {empty} resizes to an empty size (img_scale or '
                                 'ratio_range too small for its aspect ratio)')
            st = torch.where((st == 0) & ((xs & 2) != 0).to(st.device), torch.full_like(st, 2), st)
        bad = (st == 1).nonzero().flatten().tolist()
        if bad:
            raise ValueError(f'RandomSquareCrop found no window containing a box centre for images {bad} '
                             '(images without GT must be filtered by the dataset, retinaface.py)')
        return (st == 2).nonzero().flatten().tolist()       # images whose GT was truncated to gmax
