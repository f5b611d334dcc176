#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/photometric_*.npz by running the UNMODIFIED reference
PhotoMetricDistortion (mmdet/datasets/pipelines/transforms.py:1211-1312) inside the reference's own
RandomSquareCrop -> Resize -> RandomFlip -> Normalize chain, in both positions the device pipeline accepts:

    pre : PhotoMetricDistortion -> RandomSquareCrop -> Resize -> RandomFlip -> Normalize
    post: RandomSquareCrop -> Resize -> RandomFlip -> PhotoMetricDistortion -> Normalize

    python tools/make_golden_photometric.py          # needs the reference tree (oracle/ref_stub.py)

Stand-ins (the rest is the reference's own code, loaded by oracle/ref_stub.load_pipeline_transforms as it is):
  - numpy's random draws are redirected to the counter-based generator: np.random.choice / randint /
    random_sample to the main stream of (seed, iteration, image) while the crop and the flip draw, and
    np.random.randint / uniform / permutation to the photometric sub-stream (tests/photometric_ref.PhotoStream)
    while PhotoMetricDistortion runs;
  - mmcv.bgr2hsv / hsv2bgr are tests/photometric_ref's restatement of cv2.cvtColor's scalar float path (cv2 is
    absent), mmcv.imresize is oracle/pipeline_oracle.resize_linear -- so the pixels pin the device against these
    restatements, not against the cv2 binary.

Fixtures:
  photometric_pixels.npz   : 512 hard-case square images (photometric_ref.hard_case) with crop_choice=[1.0], so the
                             resize is the identity and the output is the distorted source itself; every one of the
                             2 x 2^5 (mode, flag) combinations occurs.  Per image: the reference's draw log (log,
                             log_off) and the sha256 of its pre / post outputs (sha); the first 4 outputs in full.
  photometric_pipeline.npz : seeded synthetic sources (pipeline_oracle.synth_image) at S = 64 with the shipped
                             crop_choice: boxes, keypoints, decisions, draw logs and output digests per position.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import photometric_ref as R    # noqa: E402
import pipeline_oracle as P    # noqa: E402
import ref_stub                # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
CROP_CHOICE = [0.5, 0.7, 0.9, 1.1, 1.3, 1.5]


class Redirect:
    """numpy.random's functions served from the stream in `st` (a pipeline_oracle.Stream or a PhotoStream)."""
    NAMES = ('choice', 'randint', 'random_sample', 'uniform', 'permutation')

    def __init__(self):
        self.st = None

    def __enter__(self):
        self.saved = {k: getattr(np.random, k) for k in self.NAMES}
        for k in self.NAMES:
            setattr(np.random, k, getattr(self, k))
        return self

    def __exit__(self, *a):
        for k, v in self.saved.items():
            setattr(np.random, k, v)

    def choice(self, a, size=None, replace=True, p=None):
        assert size is None and not isinstance(self.st, R.PhotoStream)
        if p is None:
            return a[self.st.choice_index(len(a))]
        cdf = np.cumsum(np.asarray(p, dtype=np.float64))
        cdf /= cdf[-1]
        return a[int(cdf.searchsorted(self.st.uniform(), side='right'))]

    def randint(self, low, high=None, size=None):
        assert size is None
        if isinstance(self.st, R.PhotoStream):
            return self.st.randint(low, high)
        assert high is not None
        return self.st.randint(int(low), int(high))

    def random_sample(self, size=None):
        assert size is None and not isinstance(self.st, R.PhotoStream)
        return self.st.uniform()

    def uniform(self, low=0.0, high=1.0, size=None):
        assert isinstance(self.st, R.PhotoStream), 'only PhotoMetricDistortion draws uniform here'
        return self.st.uniform(low, high, size)

    def permutation(self, x):
        assert isinstance(self.st, R.PhotoStream)
        return self.st.permutation(x)


def load_transforms():
    def imresize(img, size, return_scale=False, interpolation='bilinear', out=None, backend=None):
        h, w = img.shape[:2]
        assert size[0] == size[1] and interpolation == 'bilinear'
        r = P.resize_linear(img, size[0])
        return (r, size[0] / w, size[1] / h) if return_scale else r

    def imflip(img, direction='horizontal'):
        assert direction == 'horizontal'
        return np.flip(img, axis=1)

    T = ref_stub.load_pipeline_transforms(imresize=imresize, imflip=imflip)
    import mmcv
    mmcv.bgr2hsv, mmcv.hsv2bgr = R.bgr2hsv, R.hsv2bgr
    return T


def run_reference(T, srcs, seed, iteration, S, crop_choice, position, photo=None):
    """The reference chain on srcs [(img uint8, boxes, kps)] -> per image dict(img [3,S,S], boxes, kps, cw, flip,
    draws of the main stream, photometric draw log)."""
    crop = T.RandomSquareCrop(crop_choice=crop_choice)
    resize = T.Resize(img_scale=(S, S), keep_ratio=False)
    flip = T.RandomFlip(flip_ratio=0.5)
    norm = T.Normalize(mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False)
    pmd = T.PhotoMetricDistortion(**(photo or {}))
    out = []
    with Redirect() as rr:
        for i, (im, b, k) in enumerate(srcs):
            main, sub = P.Stream(seed, iteration, i), R.PhotoStream(seed, iteration, i)

            def distort(res):
                rr.st = sub
                res = pmd(res)
                rr.st = main
                return res
            rr.st = main
            res = dict(img=im.astype(np.float32), img_shape=im.shape, ori_shape=im.shape,
                       img_fields=['img'], bbox_fields=['gt_bboxes'], keypoints_fields=['gt_keypointss'],
                       gt_bboxes=b.copy(), gt_labels=np.zeros(len(b), np.int64), gt_keypointss=k.copy())
            if position == 'pre':
                res = distort(res)
            res = crop(res)
            cw = res['img'].shape[0]
            res = resize(res)
            res = flip(res)
            if position == 'post':
                res = distort(res)
            res = norm(res)
            assert res['img'].dtype == np.float32
            out.append(dict(img=np.ascontiguousarray(res['img'].transpose(2, 0, 1)),
                            boxes=res['gt_bboxes'].astype(np.float32), kps=res['gt_keypointss'].astype(np.float32),
                            cw=cw, flip=bool(res['flip']), draws=main.ctr, log=R.log_array(sub.log)))
    return out


def pixels_fixture(T):
    seed, iteration, n, S = 21, 4, 512, 32
    srcs = [R.hard_case(k, S) for k in range(n)]
    pack = dict(seed=seed, iteration=iteration, S=S, n=n, crop_choice=np.array([1.0]))
    sha = np.zeros((2, n, 32), np.uint8)            # [pre / post, image] sha256 of the output image
    meta = np.zeros((2, n, 4), np.int64)            # cw, flip, main-stream draws, kept boxes
    logs = None
    for p, position in enumerate(('pre', 'post')):
        ref = run_reference(T, srcs, seed, iteration, S, [1.0], position)
        for i, r in enumerate(ref):
            assert r['cw'] == S
            sha[p, i] = np.frombuffer(bytes.fromhex(R.digest(r['img'])), np.uint8)
            meta[p, i] = [r['cw'], int(r['flip']), r['draws'], len(r['boxes'])]
            if i < 4:
                pack[f'{position}_img_{i}'] = r['img']
        if logs is None:
            logs = [r['log'] for r in ref]
        assert all(np.array_equal(a, r['log']) for a, r in zip(logs, ref))
    combos = {R.combo(R.draw_table(seed, iteration, i)[0]) for i in range(n)}
    assert combos == set(range(64)), sorted(set(range(64)) - combos)
    pack.update(sha=sha, meta=meta, log=np.concatenate(logs),
                log_off=np.cumsum([0] + [len(x) for x in logs]).astype(np.int64))
    np.savez_compressed(os.path.join(OUT, 'photometric_pixels.npz'), **pack)
    print('photometric_pixels', n, 'images, all 64 combinations')


def pipeline_fixture(T):
    seed, iteration, S = 13, 9, 64
    shapes = [(120, 200, 3), (333, 250, 9), (97, 97, 1), (480, 640, 24), (400, 600, -1), (300, 300, -2),
              (256, 192, 5), (150, 150, 2)]
    rng = np.random.default_rng(seed)
    srcs = [P.synth_image(rng, h, w, g) for h, w, g in shapes]
    pack = dict(seed=seed, iteration=iteration, S=S, n=len(shapes), crop_choice=np.array(CROP_CHOICE, np.float64))
    for i, (im, b, k) in enumerate(srcs):
        pack[f'src_shape_{i}'] = np.array(im.shape[:2] + (int(im.astype(np.int64).sum()),), np.int64)
        pack[f'src_g_{i}'] = np.int64(shapes[i][2])
    for position in ('pre', 'post'):
        ref = run_reference(T, srcs, seed, iteration, S, CROP_CHOICE, position)
        for i, r in enumerate(ref):
            pack[f'{position}_sha_{i}'] = np.array(R.digest(r['img']))
            pack[f'{position}_corner_{i}'] = r['img'][:, :8, :8].copy()
            pack[f'{position}_boxes_{i}'] = r['boxes']
            pack[f'{position}_kps_{i}'] = r['kps']
            pack[f'{position}_meta_{i}'] = np.array([r['cw'], int(r['flip']), r['draws'], len(r['boxes'])], np.int64)
            pack[f'{position}_log_{i}'] = r['log']
        print(position, [(int(r['cw']), r['flip'], r['draws'], len(r['boxes'])) for r in ref])
    np.savez_compressed(os.path.join(OUT, 'photometric_pipeline.npz'), **pack)


def main():
    if not ref_stub.available():
        raise SystemExit('needs the reference tree')
    T = load_transforms()
    os.makedirs(OUT, exist_ok=True)
    pixels_fixture(T)
    pipeline_fixture(T)


if __name__ == '__main__':
    main()
