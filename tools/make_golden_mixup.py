#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/mixup_cases.npz by running the UNMODIFIED reference MixUp
(mmdet/datasets/pipelines/transforms.py:2523-2783, loaded by oracle/ref_stub.load_pipeline_transforms as it is) over a
small store of images.

    python tools/make_golden_mixup.py          # needs the reference tree (oracle/ref_stub.py)

Stand-ins: numpy.random.randint / uniform are redirected to the MixUp sub-stream of the counter-based generator
(tests/mixup_ref.MixupStream, keyed by (seed, iteration, image)); mmcv.imresize (cv2 is not installed) is
mixup_ref.imresize, the float32 numpy restatement of cv2's float bilinear path -- the formulas of the pixel pass's Resize;
find_inside_bboxes (the stub leaves it empty) is the reference's own function.  The class is driven as
MultiImageMixDataset drives it: get_indexes(dataset) first, then __call__ with mix_results = [the raw partner sample].
The partner image is handed over as float32 (the device pipeline's image type), so the canvas holds float values and the
only truncations are the reference's two uint8 casts.  gt_labels carry row numbers (the partner's from 1000 on).

Fixture: the store (img_<i>, sboxes_<i>, skps_<i>, store_hw), and for every configuration of mixup_ref.CONFIGS and every
edge T of mixup_ref.EDGES (N_IMAGES images each):
    own_boxes_<T> / own_kps_<T> / own_counts_<T>   the images' GT before MixUp
    it_<cfg>_<T>                                   the iteration the case was drawn at
    draws_<cfg>_<T>   float64 [n, 20]              the values randint / uniform returned, NaN-padded
    table_<cfg>_<T>   float64 [n, WORDS]           mixup_ref.decide's table (checked against the reference's draws)
    boxes_<cfg>_<T>   float32 [n, R, 4], labels_<cfg>_<T> int64 [n, R] (-1 padded), rows_<cfg>_<T> [n]   the reference's
    out_<cfg>_<T>     uint8 [n, T, T, 3]           the reference's output images
    bar_pixels_<T>                                 4 x the largest distance of the float32 partner value from the float64
    ambiguous_<T>                                  share of the applied pixels with more than one admissible output
A case is drawn at the first iteration >= mixup_ref.ITERATION at which every row's decision is clear of its thresholds
by mixup_ref.MARGIN (mixup_ref.clearance).  The tool refuses to write unless the fixture holds the hard cases
(`hard_cases`), the reference's output lies in the admissible set at every pixel and the ambiguous share is within
mixup_ref.AMBIGUOUS_CAP.
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import mixup_ref as R          # noqa: E402
import ref_stub                # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'mixup_cases.npz')
ROWS = 2 * R.GMAX


class _Dataset:
    """What get_indexes reads of MultiImageMixDataset.dataset."""

    def __init__(self, store):
        self.store = store

    def __len__(self):
        return len(self.store['imgs'])

    def get_ann_info(self, i):
        return dict(bboxes=self.store['boxes'][i])


def load_reference():
    T = ref_stub.load_pipeline_transforms(imresize=R.imresize)
    T.find_inside_bboxes = importlib.import_module('mmdet.core.bbox.transforms').find_inside_bboxes
    return T


def run_reference(T, store, name, edge, iteration):
    """The reference class on the images of one case -> dict of arrays (see the module docstring)."""
    D, cfg = R.case_cfg(name, edge)
    op = T.MixUp(img_scale=(D, D), **cfg)
    own_b, _, own_c = R.own_inputs(edge)
    imgs = R.pattern(R.N_IMAGES, edge)
    n = R.N_IMAGES
    res = dict(draws=np.full((n, 20), np.nan), boxes=np.zeros((n, ROWS, 4), np.float32),
               labels=np.full((n, ROWS), -1, np.int64), rows=np.zeros(n, np.int32),
               out=np.zeros((n, edge, edge, 3), np.uint8), partner=np.zeros(n, np.int64))
    saved = np.random.randint, np.random.uniform
    try:
        for i in range(n):
            st = R.MixupStream(R.SEED, iteration, i)
            np.random.randint, np.random.uniform = st.py_randint, st.py_uniform
            p = op.get_indexes(_Dataset(store))
            g, gp = int(own_c[i]), len(store['boxes'][p])
            a = np.ascontiguousarray(imgs[i].transpose(1, 2, 0))
            r = op(dict(img=a.copy(), gt_bboxes=own_b[i, :g].copy(), gt_labels=np.arange(g, dtype=np.int64),
                        mix_results=[dict(img=store['imgs'][p].astype(np.float32), gt_bboxes=store['boxes'][p].copy(),
                                          gt_labels=1000 + np.arange(gp, dtype=np.int64))]))
            vals = [v for *_, v in st.log]
            res['draws'][i, :len(vals)] = vals
            k = len(r['gt_bboxes'])
            assert r['gt_bboxes'].dtype == np.float32 and k <= ROWS
            res['boxes'][i, :k], res['labels'][i, :k], res['rows'][i], res['partner'][i] = r['gt_bboxes'], r['gt_labels'], k, p
            if gp:
                assert r['img'].dtype == np.uint8
                res['out'][i] = r['img']
            else:
                assert r['img'] is not None and r['img'].dtype == np.float32 and np.array_equal(r['img'], a)
    finally:
        np.random.randint, np.random.uniform = saved
    return res


def restate(store, name, edge, iteration):
    """mixup_ref.decide for the images of one case -> (list of dicts, smallest clearance)."""
    D, cfg = R.case_cfg(name, edge)
    own_b, own_k, own_c = R.own_inputs(edge)
    outs, clear = [], np.inf
    for i in range(R.N_IMAGES):
        g = int(own_c[i])
        d = R.decide(R.SEED, iteration, i, store, own_b[i, :g], own_k[i, :g], edge, D, cfg)
        outs.append(d)
        if d['table'][R.APPLIED]:
            c = R.clearance(d['table'], store['boxes'][int(d['table'][R.PARTNER])], own_b[i, :g], cfg)
            clear = min(clear, float(c.min()) if len(c) else np.inf)
    return outs, clear


def pixel_figures(store, pack, edge, bar=None):
    """bar is None: the largest distance of the float32 partner value from the float64 one over the cases of an edge.
    Else: (pixels of applied images, those with more than one admissible output, those where the reference's output is
    outside the set)."""
    dist, total, multi, outside = 0.0, 0, 0, 0
    imgs = R.pattern(R.N_IMAGES, edge)
    for name in R.CONFIGS:
        D, cfg = R.case_cfg(name, edge)
        c = R.full(cfg)
        for i in range(R.N_IMAGES):
            t = pack[f'table_{name}_{edge}'][i]
            if not t[R.APPLIED]:
                continue
            im = store['imgs'][int(t[R.PARTNER])]
            b64, zero = R.partner_value(t, im, D, c['pad_val'], np.float64)
            if bar is None:
                b32, _ = R.partner_value(t, im, D, c['pad_val'], np.float32)
                dist = max(dist, float(np.abs(b32.astype(np.float64) - b64).max()))
                continue
            lo, hi = R.admissible(imgs[i].transpose(1, 2, 0), b64, zero, bar)
            out = pack[f'out_{name}_{edge}'][i].astype(np.float32)
            total += lo.size
            multi += int((lo != hi).sum())
            outside += int(((out < lo) | (out > hi)).sum())
    return dist if bar is None else (total, multi, outside)


def hard_cases(store, pack):
    """-> dict of what the fixture contains (tests/test_mixup.py asserts the same)."""
    seen = dict(flipped=False, unflipped=False, larger_both_offsets=False, smaller=False, same=False, later_draw=False,
                not_applied=False, clip_J=False, clip_T=False, outside=False, rule_size=False, rule_area=False,
                rule_aspect=False, unclipped=False)
    for e in R.EDGES:
        for name in R.CONFIGS:
            D, cfg = R.case_cfg(name, e)
            c = R.full(cfg)
            for i in range(R.N_IMAGES):
                t = pack[f'table_{name}_{e}'][i]
                if not t[R.APPLIED]:
                    seen['not_applied'] |= c['max_iters'] == 1
                    continue
                J = int(t[R.J_])
                seen['flipped'] |= bool(t[R.FLIP])
                seen['unflipped'] |= not t[R.FLIP]
                seen['larger_both_offsets'] |= J > e and t[R.XOFF] > 0 and t[R.YOFF] > 0
                seen['smaller'] |= J < e
                seen['same'] |= J == e and t[R.DRAWS] == t[R.INDEX_DRAWS] + 2
                seen['later_draw'] |= t[R.INDEX_DRAWS] > 1
                raw = store['boxes'][int(t[R.PARTNER])]
                b, cp = R.partner_boxes(t, raw, cfg)
                ok = R.rules(b, cp, np.float32(e), cfg)
                kept = ok.all(1)
                seen['outside'] |= bool((~ok[:, 0] & ok[:, 1:].all(1)).any())
                for k, rule in ((1, 'rule_size'), (2, 'rule_area'), (3, 'rule_aspect')):    # removed by this rule alone
                    seen[rule] |= bool((~ok[:, k] & np.delete(ok, k, 1).all(1)).any())
                if c['bbox_clip_border']:
                    scaled = np.asarray(raw, np.float32) * np.float32(t[R.SR])
                    seen['clip_J'] |= bool((kept & (scaled > J).any(1)).any())
                    seen['clip_T'] |= bool((kept & ((cp[:, 2] == e) | (cp[:, 3] == e)) & (b[:, 2:] - [t[R.XOFF], t[R.YOFF]] > e).any(1)).any())
                else:
                    seen['unclipped'] |= bool((kept & ((cp < 0) | (cp > e)).any(1)).any())
    return seen


def main():
    if not ref_stub.available():
        raise SystemExit('needs the reference tree')
    T = load_reference()
    store = R.store()
    pack = dict(seed=R.SEED, iteration=R.ITERATION, margin=R.MARGIN, configs=np.array(repr(R.CONFIGS)),
                store_hw=store['hw'])
    for i in range(len(store['imgs'])):
        pack[f'img_{i}'], pack[f'sboxes_{i}'], pack[f'skps_{i}'] = store['imgs'][i], store['boxes'][i], store['kps'][i]
    for e in R.EDGES:
        pack[f'own_boxes_{e}'], pack[f'own_kps_{e}'], pack[f'own_counts_{e}'] = R.own_inputs(e)
        for name in R.CONFIGS:
            for it in range(R.ITERATION, R.ITERATION + 200):
                outs, clear = restate(store, name, e, it)
                if clear > R.MARGIN:
                    break
            else:
                raise SystemExit(f'{name} edge {e}: no iteration clear of the thresholds')
            ref = run_reference(T, store, name, e, it)
            for i, d in enumerate(outs):        # the restatement against the unmodified class: draws, rows, bytes
                t, k = d['table'], int(ref['rows'][i])
                vals = ref['draws'][i][~np.isnan(ref['draws'][i])]
                assert len(vals) == t[R.DRAWS] and ref['partner'][i] == t[R.PARTNER], (name, e, i)
                assert k == len(d['boxes']) and np.array_equal(ref['labels'][i, :k], d['labels']), (name, e, i)
                assert ref['boxes'][i, :k].tobytes() == d['boxes'].tobytes(), (name, e, i)
            pack[f'it_{name}_{e}'] = it
            pack[f'table_{name}_{e}'] = np.stack([d['table'] for d in outs])
            for k in ('draws', 'boxes', 'labels', 'rows', 'out'):
                pack[f'{k}_{name}_{e}'] = ref[k]
    for e in R.EDGES:
        dist = pixel_figures(store, pack, e)
        bar = 4 * dist
        total, multi, outside = pixel_figures(store, pack, e, bar)
        pack[f'bar_pixels_{e}'], pack[f'ambiguous_{e}'] = bar, multi / total
        print(f'edge {e}: bar {bar:.3e}; {total} applied pixel values, {multi} ambiguous ({multi / total:.2%}), '
              f'{outside} of the reference outside the set')
        if not bar > 0 or outside or multi / total > R.AMBIGUOUS_CAP:
            raise SystemExit(f'edge {e}: the reference misses the pixel conditions')
    seen = hard_cases(store, pack)
    missing = [k for k, v in seen.items() if not v]
    if missing:
        raise SystemExit(f'seed {R.SEED}: the fixture lacks {missing}; choose another mixup_ref.SEED')
    np.savez_compressed(OUT, **pack)
    print('mixup_cases.npz', os.path.getsize(OUT), 'bytes;',
          {f'{n}_{e}': int(pack[f'it_{n}_{e}']) for n in R.CONFIGS for e in R.EDGES})


if __name__ == '__main__':
    main()
