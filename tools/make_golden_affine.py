#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/affine_cases.npz by running the UNMODIFIED reference RandomAffine
(mmdet/datasets/pipelines/transforms.py:2787-3001, loaded by oracle/ref_stub.load_pipeline_transforms as it is) on small
ground-truth sets.

    python tools/make_golden_affine.py          # needs the reference tree (oracle/ref_stub.py)

Stand-ins: numpy.random.uniform is redirected to the RandomAffine sub-stream of the counter-based generator
(tests/affine_ref.AffineStream, keyed by (seed, iteration, image)); cv2.warpPerspective (cv2 is not installed) is a
function that notes the matrix it is given and returns the image; find_inside_bboxes (the stub leaves it empty) is the
reference's own function behind a wrapper that notes its argument, so warp_bboxes is recorded for every row, not only
for the survivors.  gt_labels carry the row numbers, so the surviving labels are valid_index.

Fixture, for every configuration of affine_ref.CONFIGS and every edge of affine_ref.EDGES (N_IMAGES images each):
    boxes_<e> / kps_<e> / counts_<e>     the inputs (affine_ref.inputs), float32 / float32 / int32
    it_<cfg>_<e>                         the iteration the case was drawn at
    draws_<cfg>_<e>    float64 [n, 6]    the six values random.uniform returned
    M_<cfg>_<e>        float32 [n, 3, 3] warp_matrix as handed to cv2.warpPerspective
    wb_<cfg>_<e>       float32 [n, G, 4] warp_bboxes of every row (clipped under bbox_clip_border)
    valid_<cfg>_<e>    bool [n, G]       valid_index
    bar_matrix_<e>, bar_gt_<e>           2 x the largest deviation of M / wb above from affine_ref's float64 evaluation
    bar_pixels_<e>                       4 x the largest deviation of affine_ref.warp_pixels in float32 from float64
A case is drawn at the first iteration >= affine_ref.ITERATION at which every row's decision is clear of its thresholds
by affine_ref.MARGIN pixels (affine_ref.clearance); the tool refuses to write unless every bar is below MARGIN, so the
survivor sets cannot depend on the summation order, and unless the fixture holds the hard cases (`hard_cases`).
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import affine_ref as R         # noqa: E402
import ref_stub                # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'affine_cases.npz')


def load_reference(log):
    T = ref_stub.load_pipeline_transforms()
    inside = importlib.import_module('mmdet.core.bbox.transforms').find_inside_bboxes

    def find_inside_bboxes(bboxes, img_h, img_w):
        log['warp_bboxes'] = np.array(bboxes)
        return inside(bboxes, img_h, img_w)

    def warp_perspective(img, M, dsize=None, borderValue=None, **kw):
        assert not kw and tuple(dsize) == (img.shape[1], img.shape[0])
        log['M'] = np.array(M)
        return img
    T.find_inside_bboxes = find_inside_bboxes
    T.cv2.warpPerspective = warp_perspective
    return T


def run_reference(T, log, cfg, boxes, counts, edge, seed, iteration):
    """The reference class on the images of one edge -> (draws [n,6], M [n,3,3], wb [n,G,4], valid [n,G])."""
    cfg = {k: v for k, v in cfg.items()}
    op = T.RandomAffine(**cfg)
    n, G = boxes.shape[:2]
    draws, Ms = np.zeros((n, 6)), np.zeros((n, 3, 3), np.float32)
    wbs, valid = np.zeros((n, G, 4), np.float32), np.zeros((n, G), bool)
    saved = np.random.uniform
    try:
        for i in range(n):
            st = R.AffineStream(seed, iteration, i)
            np.random.uniform = st.py_uniform
            g = int(counts[i])
            log.clear()
            res = op(dict(img=np.zeros((edge, edge, 3), np.float32), bbox_fields=['gt_bboxes'],
                          gt_bboxes=boxes[i, :g].copy(), gt_labels=np.arange(g, dtype=np.int64)))
            assert st.ctr == 6 and log['M'].dtype == np.float32 and log['warp_bboxes'].dtype == np.float32
            draws[i] = [v for _, _, v in st.log]
            Ms[i], wbs[i, :g] = log['M'], log['warp_bboxes']
            valid[i, res['gt_labels']] = True
            assert np.array_equal(res['gt_bboxes'], wbs[i, :g][valid[i, :g]])
    finally:
        np.random.uniform = saved
    return draws, Ms, wbs, valid


def clear_of_thresholds(name, edge, boxes, counts, draws):
    cfg = R.CONFIGS[name]
    return min(float(R.clearance(boxes[i, :counts[i]], draws[i, 1], R.matrix(draws[i], edge, np.float64), edge, cfg).min())
               for i in range(len(counts)))


def deviations(pack, edge):
    """Largest distance of the reference's float32 results (matrix, boxes) and of the float32 pixel restatement from the
    float64 evaluation, over the cases of one edge."""
    dm = dg = dp = 0.0
    counts, boxes, imgs = pack[f'counts_{edge}'], pack[f'boxes_{edge}'], R.pattern(R.N_IMAGES, edge)
    for name, cfg in R.CONFIGS.items():
        c = R.full(cfg)
        for i in range(R.N_IMAGES):
            g, d = int(counts[i]), pack[f'draws_{name}_{edge}'][i]
            M64 = R.matrix(d, edge, np.float64)
            dm = max(dm, float(np.abs(pack[f'M_{name}_{edge}'][i] - M64).max()))
            wb64 = R.warp_boxes(M64, boxes[i, :g], edge, c['bbox_clip_border'])
            dg = max(dg, float(np.abs(pack[f'wb_{name}_{edge}'][i, :g] - wb64).max()))
            inv = R.inverse(pack[f'M_{name}_{edge}'][i])
            p64 = R.warp_pixels(imgs[i], inv, c['border_val'], np.float64)
            p32 = R.warp_pixels(imgs[i], inv, c['border_val'], np.float32)
            dp = max(dp, float(np.abs(p32 - p64).max()))
    return dm, dg, dp


def hard_cases(pack):
    """-> dict of what the fixture contains (tests/test_affine.py asserts the same)."""
    seen = dict(clip_left=False, clip_top=False, clip_right=False, clip_bottom=False, outside=False, rule_size=False,
                rule_area=False, rule_aspect=False, loses_all=False, keeps_all=False)
    for e in R.EDGES:
        counts, boxes = pack[f'counts_{e}'], pack[f'boxes_{e}']
        for name, cfg in R.CONFIGS.items():
            c = R.full(cfg)
            for i in range(R.N_IMAGES):
                g = int(counts[i])
                wb, valid = pack[f'wb_{name}_{e}'][i, :g], pack[f'valid_{name}_{e}'][i, :g]
                ok = R.rules(boxes[i, :g], wb, pack[f'draws_{name}_{e}'][i, 1], e, cfg)
                assert np.array_equal(ok.all(1), valid)
                seen['loses_all'] |= not valid.any()
                seen['keeps_all'] |= bool(valid.all()) and g == R.GMAX
                seen['outside'] |= bool((~ok[:, 0]).any())
                live = ok[:, 0]
                for k, rule in ((1, 'rule_size'), (2, 'rule_area'), (3, 'rule_aspect')):    # removed by this rule alone
                    others = np.delete(ok, k, 1).all(1)
                    seen[rule] |= bool((live & ~ok[:, k] & others).any())
                if c['bbox_clip_border']:
                    seen['clip_left'] |= bool((valid & (wb[:, 0] == 0)).any())
                    seen['clip_top'] |= bool((valid & (wb[:, 1] == 0)).any())
                    seen['clip_right'] |= bool((valid & (wb[:, 2] == e)).any())
                    seen['clip_bottom'] |= bool((valid & (wb[:, 3] == e)).any())
    return seen


def main():
    if not ref_stub.available():
        raise SystemExit('needs the reference tree')
    log = {}
    T = load_reference(log)
    pack = dict(seed=R.SEED, iteration=R.ITERATION, margin=R.MARGIN, configs=np.array(repr(R.CONFIGS)))
    for e in R.EDGES:
        boxes, kps, counts = R.inputs(e)
        pack[f'boxes_{e}'], pack[f'kps_{e}'], pack[f'counts_{e}'] = boxes, kps, counts
        for name, cfg in R.CONFIGS.items():
            for it in range(R.ITERATION, R.ITERATION + 200):
                draws, Ms, wbs, valid = run_reference(T, log, cfg, boxes, counts, e, R.SEED, it)
                if clear_of_thresholds(name, e, boxes, counts, draws) > R.MARGIN:
                    break
            else:
                raise SystemExit(f'{name} edge {e}: no iteration clear of the thresholds')
            pack[f'it_{name}_{e}'] = it
            pack[f'draws_{name}_{e}'], pack[f'M_{name}_{e}'] = draws, Ms
            pack[f'wb_{name}_{e}'], pack[f'valid_{name}_{e}'] = wbs, valid
    for e in R.EDGES:
        dm, dg, dp = deviations(pack, e)
        pack[f'bar_matrix_{e}'], pack[f'bar_gt_{e}'], pack[f'bar_pixels_{e}'] = 2 * dm, 2 * dg, 4 * dp
        print(f'edge {e}: bars matrix {2 * dm:.3e} gt {2 * dg:.3e} pixels {4 * dp:.3e}')
        if not 0 < 2 * dm < R.MARGIN or not 0 < 2 * dg < R.MARGIN or not dp > 0:
            raise SystemExit(f'edge {e}: a bar is zero or not below the margin {R.MARGIN}')
    seen = hard_cases(pack)
    missing = [k for k, v in seen.items() if not v]
    if missing:
        raise SystemExit(f'seed {R.SEED}: the fixture lacks {missing}; choose another affine_ref.SEED')
    np.savez_compressed(OUT, **pack)
    print('affine_cases.npz', os.path.getsize(OUT), 'bytes;',
          {f'{n}_{e}': int(pack[f'it_{n}_{e}']) for n in R.CONFIGS for e in R.EDGES})


if __name__ == '__main__':
    main()
