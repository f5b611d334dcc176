#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/mosaic_cases.npz by running the UNMODIFIED reference classes

    MultiImageMixDataset(dataset, pipeline=[Mosaic(img_scale=(S, S), use_kps=True, ...)])

(mmdet/datasets/dataset_wrappers.py:338-444, mmdet/datasets/pipelines/transforms.py:2218-2519) on seeded synthetic
sources (tests/mosaic_ref.py: SOURCES, CASES), with the `random` draws of transforms.py -- numpy's: the module says
`from numpy import random` -- redirected to the mosaic sub-stream of the counter-based generator
(tests/mosaic_ref.MosaicStream) and mmcv.imresize bound to the repository's cv2 float-bilinear restatement.

    python tools/make_golden_mosaic.py          # needs the reference tree (oracle/ref_stub.py)

What the fixture pins, all from the reference's own code: the order and bounds of the draws (partner indices, the prob
draw, the centre), the resized sizes, the paste / crop rectangles of _mosaic_combine, the merged boxes / keypoints after
clip, min_bbox_size filter and find_inside_bboxes, and which rows survive (the labels carry each row's index through
the reference's own filters).  Canvas pixels are kept as a digest: with imresize bound to the restatement they are a
consistency check of the paste, not an independent check of cv2.

Recorded inputs and results only; the uint8 sources are regenerated from their seed by the tests.
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import mosaic_ref as MR        # noqa: E402
import ref_stub                # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'mosaic_cases.npz')


class RedirectedRandom:
    """numpy.random.uniform / randint (what transforms.py calls `random`) served from a MosaicStream."""

    def __init__(self):
        self.st = None

    def __enter__(self):
        self.saved = (np.random.uniform, np.random.randint)
        np.random.uniform, np.random.randint = self.uniform, self.randint
        return self

    def __exit__(self, *a):
        np.random.uniform, np.random.randint = self.saved

    def uniform(self, low=0.0, high=1.0, size=None):
        assert size is None
        return self.st.py_uniform(low, high)

    def randint(self, low, high=None, size=None):
        assert size is None and high is not None
        return self.st.randint(int(low), int(high))


def load_reference(log):
    def imresize(img, size, return_scale=False, interpolation='bilinear', out=None, backend=None):
        assert interpolation == 'bilinear' and not return_scale and img.dtype == np.float32
        log['resized'].append((int(size[0]), int(size[1])))
        return MR.resize_wh(img, int(size[0]), int(size[1]))

    T = ref_stub.load_pipeline_transforms(imresize=imresize, imflip=lambda im, direction='horizontal': im[:, ::-1])
    T.find_inside_bboxes = importlib.import_module('mmdet.core.bbox.transforms').find_inside_bboxes
    b = sys.modules['mmdet.datasets.builder']
    if not hasattr(b, 'DATASETS'):
        b.DATASETS = type(b.PIPELINES)('dataset')
    if 'mmdet.datasets.coco' not in sys.modules:
        coco = types.ModuleType('mmdet.datasets.coco')
        coco.CocoDataset = type('CocoDataset', (), {})
        sys.modules['mmdet.datasets.coco'] = coco
    W = importlib.import_module('mmdet.datasets.dataset_wrappers')
    return T, W


class ListDataset:
    CLASSES = ('face',)

    def __init__(self, srcs):
        self.srcs = srcs
        self.calls = 0

    def __len__(self):
        return len(self.srcs)

    def __getitem__(self, i):
        # gt_labels = (which of the four fetches of this output image) * TAG + row: it rides through every filter of the
        # reference and says which rows of the concatenated GT survive, also when a partner is drawn twice
        img, b, k = self.srcs[i]
        tag, self.calls = self.calls * TAG, self.calls + 1
        return dict(img=img.astype(np.float32), img_shape=img.shape, gt_bboxes=b.copy(), gt_keypointss=k.copy(),
                    gt_labels=tag + np.arange(len(b), dtype=np.int64))


TAG = 1 << 20


def run_reference(T, W, log, case, srcs):
    ds = ListDataset(srcs)
    S = case['S']
    mix = W.MultiImageMixDataset(ds, pipeline=[dict(
        type='Mosaic', img_scale=(S, S), center_ratio_range=case['center'], min_bbox_size=case['min_bbox_size'],
        bbox_clip_border=case['clip'], skip_filter=case['skip_filter'], pad_val=case['pad_val'], prob=case['prob'],
        use_kps=True)])
    mosaic = mix.pipeline[0]
    assert type(mosaic) is T.Mosaic
    inner_indexes, inner_combine = mosaic.get_indexes, mosaic._mosaic_combine

    def get_indexes(dataset):           # recording wrappers around the reference's own bound methods
        log['partners'] = [int(i) for i in inner_indexes(dataset)]
        return log['partners']

    def combine(loc, centre, wh):
        paste, crop = inner_combine(loc, centre, wh)
        log['centre'] = (int(centre[0]), int(centre[1]))
        log['rects'].append([int(v) for v in paste] + [int(v) for v in crop])
        return paste, crop

    mosaic.get_indexes, mosaic._mosaic_combine = get_indexes, combine
    out = []
    with RedirectedRandom() as rr:
        for n, own in enumerate(case['idx']):
            log.update(resized=[], rects=[], centre=(0, 0), partners=None)
            rr.st = MR.MosaicStream(case['seed'], case['iteration'], n)
            ds.calls = 0
            res = mix[own]
            applied = len(log['rects']) == 4
            rows = [own] + log['partners']
            assert ds.calls == 4
            first = np.concatenate([[0], np.cumsum([len(srcs[i][1]) for i in rows])])
            kept = [int(first[int(lab) // TAG] + int(lab) % TAG) for lab in res['gt_labels']]
            geom = np.zeros((4, 11), np.int64)
            if applied:
                for q in range(4):
                    h, w = srcs[rows[q]][0].shape[:2]
                    rw, rh = log['resized'][q]
                    geom[q] = [h, w, rw, rh] + log['rects'][q][:4] + log['rects'][q][4:6] + [len(srcs[rows[q]][1])]
                assert res['img'].shape == (2 * S, 2 * S, 3) and res['img'].dtype == np.float32
            out.append(dict(partners=log['partners'], applied=applied, cx=log['centre'][0], cy=log['centre'][1],
                            draws=rr.st.ctr, geom=geom, boxes=res['gt_bboxes'].astype(np.float32),
                            kps=res['gt_keypointss'].astype(np.float32), kept=np.array(kept, np.int64),
                            canvas=res['img'] if applied else None))
    return out


def digest(canvas):
    c = canvas.astype(np.float64)
    return np.stack([c.sum((0, 1)), (c ** 2).sum((0, 1))])


def main():
    if not ref_stub.available():
        raise SystemExit('needs the reference tree')
    log = {}
    T, W = load_reference(log)
    stores = {w: MR.make_sources(w) for w in ('main', 'empty')}
    pack = {}
    for which, srcs in stores.items():
        for i, (img, b, k) in enumerate(srcs):
            pack[f'src/{which}/{i}/sum'] = np.int64(img.astype(np.int64).sum())
            pack[f'src/{which}/{i}/boxes'], pack[f'src/{which}/{i}/kps'] = b, k
    seen = dict(skipped=0, applied=0, empty_paste=0, dropped_inside=0, dropped_filter=0, degenerate=0, over64=0,
                empty_merged=0, absent_kps=0, unclipped=0)
    for row in MR.CASES:
        case = MR.case_dict(row)
        srcs = stores[case['store']]
        ref = run_reference(T, W, log, case, srcs)
        mine = MR.run_case(case, srcs)
        for n, (r, m) in enumerate(zip(ref, mine)):
            key = f"{case['name']}/{n}/"
            pack[key + 'meta'] = np.array(r['partners'] + [int(r['applied']), r['cx'], r['cy'], r['draws']], np.int64)
            pack[key + 'geom'], pack[key + 'boxes'], pack[key + 'kps'], pack[key + 'kept'] = \
                r['geom'], r['boxes'], r['kps'], r['kept']
            if r['applied']:
                pack[key + 'digest'] = digest(r['canvas'])
                pack[key + 'patch'] = r['canvas'][max(r['cy'] - 8, 0):r['cy'] + 8, max(r['cx'] - 8, 0):r['cx'] + 8].copy()
            # bookkeeping of the hard cases (asserted below: a re-seed must not make the tests vacuous)
            seen['applied' if r['applied'] else 'skipped'] += 1
            if r['applied']:
                g = r['geom']
                seen['empty_paste'] += int(((g[:, 6] <= g[:, 4]) | (g[:, 7] <= g[:, 5])).sum())
                total = int(g[:, 10].sum())
                seen['over64'] += int(len(r['boxes']) > 64)
                seen['empty_merged'] += int(len(r['boxes']) == 0)
                if case['skip_filter']:
                    seen['dropped_inside'] += total - len(r['boxes'])
                else:
                    full = MR.mosaic([srcs[i] for i in [case['idx'][n]] + r['partners']], r['cx'], r['cy'], case['S'],
                                     case['pad_val'], case['clip'], True, 0, with_image=False)
                    seen['dropped_filter'] += len(full['boxes']) - len(r['boxes'])
                b = r['boxes']
                if case['clip']:        # boxes the clip made degenerate (find_inside_bboxes then drops them)
                    c = m['clipped']
                    seen['degenerate'] += int(((c[:, 2] <= c[:, 0]) | (c[:, 3] <= c[:, 1])).sum())
                seen['absent_kps'] += int((r['kps'][:, :, 2] < 0).any(1).sum())
                seen['unclipped'] += int(((b < 0) | (b > 2 * case['S'])).any())
            # the restatement against the reference, here already (tests/test_mosaic.py repeats it from the file)
            assert r['partners'] == m['partners'] and r['applied'] == m['applied'], (key, r['partners'], m['partners'])
            assert (r['cx'], r['cy'], r['draws']) == (m['cx'], m['cy'], m['draws']), key
            assert np.array_equal(r['geom'], m['geom']), (key, r['geom'], m['geom'])
            assert np.array_equal(r['kept'], m['kept']), (key, r['kept'], m['kept'])
            assert r['boxes'].tobytes() == m['boxes'].astype(np.float32).tobytes(), key
            assert r['kps'].tobytes() == m['kps'].astype(np.float32).tobytes(), key
            if r['applied']:
                assert r['canvas'].tobytes() == m['canvas'].tobytes(), key
        print(case['name'], [(r['partners'], int(r['applied']), r['cx'], r['cy'], len(r['boxes'])) for r in ref])
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    np.savez_compressed(OUT, **pack)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
