#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/crowd_crop.npz by running the UNMODIFIED reference transform classes

    RandomSquareCrop -> Resize(img_scale=(64, 64), keep_ratio=False) -> RandomFlip

on two crowded synthetic sources (96 x 128 with 300 faces, 96 x 128 with 65), with numpy's random draws redirected to the
counter-based generator of oracle/pipeline_oracle.py (oracle/make_golden_pipeline.RedirectedRandom), as
tools/make_golden_multiscale.py does.

    python tools/make_golden_crowd.py          # needs the reference tree (oracle/ref_stub.py)

What the fixture pins: the crop window, the kept faces in order, their transformed boxes / keypoints, the flip flag and the
number of draws when a crop keeps MORE than 64 (and more than 128) faces -- the regime in which the padded GT width of the
device pipeline decides whether ground truth survives.  No pixels are stored: the sources are regenerated from the seed by
pipeline_oracle.synth_image (shape + byte sum stored to detect generator drift) and only their GT is read.

Per image: src_shape (h, w, byte sum), src_boxes, src_kps, boxes, kps, meta = (left, top, cw, flip, draws, kept).  The
window's left / top are the reference's own last randint draws (a side that equals the window draws nothing and is 0).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import pipeline_oracle as P    # noqa: E402
import ref_stub                # noqa: E402
from make_golden_pipeline import CROP_CHOICE, RedirectedRandom   # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'crowd_crop.npz')
SEED, ITERATION, S = 58, 3, 64      # seed 58: the crowd image keeps 272 of its 300 faces (flipped), the other all 65
SHAPES = [(96, 128, 300), (96, 128, 65)]


class RecordingRandom(RedirectedRandom):
    """RedirectedRandom that keeps the randint results of the current image."""

    def randint(self, low, high=None, size=None):
        v = super().randint(low, high, size)
        self.ints.append(int(v))
        return v


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


def run_reference(T, imgs, boxes, kps):
    crop = T.RandomSquareCrop(crop_choice=CROP_CHOICE)
    resize = T.Resize(img_scale=(S, S), keep_ratio=False)
    flip = T.RandomFlip(flip_ratio=0.5)
    out = []
    with RecordingRandom() as rr:
        for i, (im, b, k) in enumerate(zip(imgs, boxes, kps)):
            rr.st, rr.ints = P.Stream(SEED, ITERATION, i), []
            res = dict(img=im.astype(np.float32), img_shape=im.shape, ori_shape=im.shape,
                       img_fields=['img'], bbox_fields=['gt_bboxes'], keypoints_fields=['gt_keypointss'],
                       gt_bboxes=b.copy(), gt_labels=np.zeros(len(b), np.int64), gt_keypointss=k.copy())
            res = crop(res)
            cw = int(res['img'].shape[0])
            h, w = im.shape[:2]
            ints = list(rr.ints)
            top = 0 if h == cw else ints.pop()
            left = 0 if w == cw else ints.pop()
            res = flip(resize(res))
            out.append(dict(boxes=res['gt_bboxes'].astype(np.float32), kps=res['gt_keypointss'].astype(np.float32),
                            left=left, top=top, cw=cw, flip=bool(res['flip']), draws=rr.st.ctr))
    return out


def main():
    if not ref_stub.available():
        raise SystemExit('needs the reference tree')
    T = load_transforms()
    rng = np.random.default_rng(SEED)
    imgs, boxes, kps = zip(*[P.synth_image(rng, h, w, g) for h, w, g in SHAPES])
    ref = run_reference(T, imgs, boxes, kps)
    kept = [len(r['boxes']) for r in ref]
    # a re-seed must not make the tests vacuous: the crowd image keeps more than 128 faces but not all of them (the
    # compaction has gaps to close), the other one more than 64
    assert 128 < kept[0] < SHAPES[0][2] and kept[1] > 64, kept
    pack = dict(seed=SEED, iteration=ITERATION, S=S, n=len(SHAPES), crop_choice=np.array(CROP_CHOICE, np.float64))
    for i, r in enumerate(ref):
        pack[f'src_shape_{i}'] = np.array(imgs[i].shape[:2] + (int(imgs[i].astype(np.int64).sum()),), np.int64)
        pack[f'src_boxes_{i}'] = boxes[i]
        pack[f'src_kps_{i}'] = kps[i]
        pack[f'boxes_{i}'] = r['boxes']
        pack[f'kps_{i}'] = r['kps']
        pack[f'meta_{i}'] = np.array([r['left'], r['top'], r['cw'], int(r['flip']), r['draws'], len(r['boxes'])], np.int64)
    np.savez_compressed(OUT, **pack)
    print([(r['left'], r['top'], r['cw'], r['flip'], r['draws'], len(r['boxes'])) for r in ref])
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
