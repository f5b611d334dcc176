#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/ignore_cases.npz by running the UNMODIFIED reference transform
classes (mmdet/datasets/pipelines/transforms.py, loaded by oracle/ref_stub.load_pipeline_transforms as they are)

    RandomSquareCrop -> Resize(keep_ratio=False) -> RandomFlip

with `gt_bboxes_ignore` in bbox_fields beside `gt_bboxes`, on small sources whose ignore boxes are placed against each
image's crop window (tests/ignore_ref.craft).  numpy's random draws are redirected to the counter-based generator of
oracle/pipeline_oracle.py (oracle/make_golden_pipeline.RedirectedRandom), as for tests/golden/pipeline_s*.npz.

    python tools/make_golden_ignore.py          # needs the reference tree (oracle/ref_stub.py)

Two sets (tests/ignore_ref.SETS): 's64' = Resize(img_scale=(64, 64)), 'r32_96' = Resize(img_scale=(32, 96),
multiscale_mode='square_range').  A set is drawn at the first iteration at which it holds every hard case of
ignore_ref.hard_cases (an ignore box whose centre lies on the patch edge and is dropped, one clipped on two sides, a
flipped and an unflipped image with ignore boxes, an image without any, one that keeps more than ignore_ref.ROWS) and,
for the multi-scale set, at least two sizes S_n.

Fixture per set and image i (data only):
    iteration                          the iteration the set was drawn at
    boxes_<i>                          the source's GT boxes (pins the regenerated sources)
    ign_src_<i>      float32 [I,4]     the ignore boxes handed to the reference
    ign_<i>          float32 [K,4]     gt_bboxes_ignore as the reference leaves it (every kept row, beyond ROWS too)
    gt_<i>           float32 [G',4]    gt_bboxes as the reference leaves it
    meta_<i>         int64 [6]         left, top, cw, flip, S_n, draws
The tool refuses to write unless tests/ignore_ref.transform (the restatement) gives the reference's rows bit for bit and
the window, flip and size are the ones ignore_ref.decide names."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import ignore_ref as G         # noqa: E402
import pipeline_oracle as P    # noqa: E402
import ref_stub                # noqa: E402
from make_golden_pipeline import RedirectedRandom   # noqa: E402

OUT = G.GOLD
MAX_ITERATIONS = 400


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


def run_reference(T, items, seed, iteration, size):
    crop = T.RandomSquareCrop(crop_choice=G.CROP_CHOICE)
    if isinstance(size, int):
        resize = T.Resize(img_scale=(size, size), keep_ratio=False)
    else:
        resize = T.Resize(img_scale=tuple(size), multiscale_mode='square_range', keep_ratio=False)
    flip = T.RandomFlip(flip_ratio=0.5)
    out = []
    with RedirectedRandom() as rr:
        for i, it in enumerate(items):
            rr.st = P.Stream(seed, iteration, i)
            im = it['img']
            res = dict(img=im.astype(np.float32), img_shape=im.shape, ori_shape=im.shape, img_fields=['img'],
                       bbox_fields=['gt_bboxes', 'gt_bboxes_ignore'], keypoints_fields=['gt_keypointss'],
                       gt_bboxes=it['boxes'].copy(), gt_labels=np.zeros(len(it['boxes']), np.int64),
                       gt_keypointss=it['kps'].copy(), gt_bboxes_ignore=it['ign'].copy())
            res = crop(res)
            cw = res['img'].shape[0]
            res = flip(resize(res))
            out.append(dict(ign=np.asarray(res['gt_bboxes_ignore'], np.float32).reshape(-1, 4),
                            gt=np.asarray(res['gt_bboxes'], np.float32).reshape(-1, 4), cw=cw, flip=bool(res['flip']),
                            S=int(res['img_shape'][0]), draws=rr.st.ctr))
    return out


def main():
    if not ref_stub.available():
        raise SystemExit('needs the reference tree')
    T = load_transforms()
    pack = {}
    for name, (seed, base, size) in G.SETS.items():
        for iteration in range(base, base + MAX_ITERATIONS):
            items = G.build_set(name, iteration)
            ref = run_reference(T, items, seed, iteration, size)
            seen = G.hard_cases(items, [r['ign'] for r in ref])
            if all(seen.values()) and (isinstance(size, int) or len({r['S'] for r in ref}) >= 2):
                break
        else:
            raise SystemExit(f'{name}: no iteration below {base + MAX_ITERATIONS} holds every hard case ({seen})')
        for i, (it, r) in enumerate(zip(items, ref)):
            assert (r['cw'], r['flip'], r['S'], r['draws']) == (it['cw'], it['flip'], it['S'], it['draws']), (name, i)
            mine, _ = G.transform(it['ign'], it['left'], it['top'], it['cw'], it['S'], it['flip'])
            assert mine.dtype == r['ign'].dtype and np.array_equal(mine, r['ign']), (name, i)
            pack[f'{name}/boxes_{i}'] = it['boxes']
            pack[f'{name}/ign_src_{i}'] = it['ign']
            pack[f'{name}/ign_{i}'] = r['ign']
            pack[f'{name}/gt_{i}'] = r['gt']
            pack[f'{name}/meta_{i}'] = np.array([it['left'], it['top'], it['cw'], int(it['flip']), it['S'], it['draws']], np.int64)
        pack[f'{name}/iteration'] = np.int64(iteration)
        print(name, 'iteration', iteration, [(it['left'], it['top'], it['cw'], it['flip'], it['S'], len(r['ign']))
                                             for it, r in zip(items, ref)])
    np.savez_compressed(OUT, **pack)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
