#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/pipeline_multiscale.npz by running the UNMODIFIED reference
transform classes

    RandomSquareCrop -> Resize(img_scale=(lo, hi), multiscale_mode='square_range', keep_ratio=False) -> RandomFlip
    -> Normalize

per image on seeded synthetic sources, with numpy's random draws redirected to the counter-based generator of
oracle/pipeline_oracle.py (oracle/make_golden_pipeline.RedirectedRandom), as for tests/golden/pipeline_s*.npz.

    python tools/make_golden_multiscale.py          # needs the reference tree (oracle/ref_stub.py)

What the fixture pins: the position and bounds of Resize's extra draw (S_n per image, the number of draws), crop
windows, kept boxes, transformed boxes / keypoints and flip flags -- all from the reference's own code.  mmcv.imresize is
bound to pipeline_oracle.resize_linear (cv2 is absent), so the pixels are a consistency check of the interpolation only.
The collate (zero border up to the batch's largest image) is mmcv's and is not run here: tests/multiscale_ref.py.

Two sets, ranges (160, 320) and (320, 640); per image what pipeline_s*.npz stores (source shape and GT, not pixels;
boxes, keypoints; meta = cw, flip, draws, kept, S_n; an image digest and two 16 x 16 windows).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import multiscale_ref as M     # noqa: E402
import pipeline_oracle as P    # noqa: E402
import ref_stub                # noqa: E402
from make_golden_pipeline import RedirectedRandom   # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'pipeline_multiscale.npz')
#        set name     seed it  lo   hi   (h, w, g) per source
SETS = [('r160_320', 31, 2, 160, 320, [(120, 200, 3), (333, 250, 9), (97, 97, 1), (480, 640, 24), (400, 600, -1),
                                       (600, 400, -1), (300, 300, -2), (256, 384, 5), (500, 375, 12), (150, 150, 2)]),
        ('r320_640', 37, 9, 320, 640, [(768, 1024, 40), (500, 375, 2), (1024, 683, 64), (240, 320, 5), (333, 500, 1),
                                       (1024, 1024, 17), (683, 1024, 8), (600, 400, -1), (375, 500, 3)])]


def load_transforms():
    def imresize(img, size, return_scale=False, interpolation='bilinear', out=None, backend=None):
        h, w = img.shape[:2]
        assert size[0] == size[1] and interpolation == 'bilinear'
        r = P.resize_linear(img, size[0])
        return (r, size[0] / w, size[1] / h) if return_scale else r

    def imflip(img, direction='horizontal'):
        assert direction == 'horizontal'
        return np.flip(img, axis=1)

    return ref_stub.load_pipeline_transforms(imresize=imresize, imflip=imflip)


def run_reference(T, imgs, boxes, kps, seed, iteration, lo, hi):
    crop = T.RandomSquareCrop(crop_choice=M.CROP_CHOICE)
    resize = T.Resize(img_scale=(lo, hi), multiscale_mode='square_range', keep_ratio=False)
    flip = T.RandomFlip(flip_ratio=0.5)
    norm = T.Normalize(mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False)
    out = []
    with RedirectedRandom() as rr:
        for i, (im, b, k) in enumerate(zip(imgs, boxes, kps)):
            rr.st = P.Stream(seed, iteration, i)
            res = dict(img=im.astype(np.float32), img_shape=im.shape, ori_shape=im.shape,
                       img_fields=['img'], bbox_fields=['gt_bboxes'], keypoints_fields=['gt_keypointss'],
                       gt_bboxes=b.copy(), gt_labels=np.zeros(len(b), np.int64), gt_keypointss=k.copy())
            res = crop(res)
            cw = res['img'].shape[0]
            res = norm(flip(resize(res)))
            assert res['img_shape'] == res['pad_shape'] and res['img_shape'][0] == res['img_shape'][1]
            out.append(dict(img=np.ascontiguousarray(res['img'].transpose(2, 0, 1)).astype(np.float32),
                            boxes=res['gt_bboxes'].astype(np.float32), kps=res['gt_keypointss'].astype(np.float32),
                            cw=cw, flip=bool(res['flip']), draws=rr.st.ctr, S=int(res['img_shape'][0])))
    return out


def main():
    if not ref_stub.available():
        raise SystemExit('needs the reference tree')
    T = load_transforms()
    pack = {}
    for name, seed, iteration, lo, hi, shapes in SETS:
        rng = np.random.default_rng(seed)
        imgs, boxes, kps = zip(*[P.synth_image(rng, h, w, g) for h, w, g in shapes])
        ref = run_reference(T, imgs, boxes, kps, seed, iteration, lo, hi)
        sizes = [r['S'] for r in ref]
        # a re-seed must not make the tests vacuous
        assert len(shapes) >= 8 and len(set(sizes)) >= 3 and min(sizes) < max(sizes), (name, sizes)
        assert all(s in M.out_sizes(lo, hi) for s in sizes), (name, sizes)
        one = dict(seed=seed, iteration=iteration, lo=lo, hi=hi, n=len(shapes),
                   crop_choice=np.array(M.CROP_CHOICE, np.float64))
        for i, r in enumerate(ref):
            one[f'src_shape_{i}'] = np.array(imgs[i].shape[:2] + (int(imgs[i].astype(np.int64).sum()),), np.int64)
            one[f'src_g_{i}'] = np.int64(shapes[i][2])
            one[f'src_boxes_{i}'] = boxes[i]
            one[f'src_kps_{i}'] = kps[i]
            one[f'boxes_{i}'] = r['boxes']
            one[f'kps_{i}'] = r['kps']
            one[f'meta_{i}'] = np.array([r['cw'], int(r['flip']), r['draws'], len(r['boxes']), r['S']], np.int64)
            one[f'img_digest_{i}'], one[f'img_corner_{i}'], one[f'img_center_{i}'] = M.image_digest(r['img'])
        pack.update({f'{name}/{k}': v for k, v in one.items()})
        print(name, [(int(r['cw']), r['flip'], r['draws'], len(r['boxes']), r['S']) for r in ref])
    np.savez_compressed(OUT, **pack)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
