#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/cutout.npz by running the UNMODIFIED reference CutOut
(mmdet/datasets/pipelines/transforms.py:2143-2214, loaded by oracle/ref_stub.load_pipeline_transforms as it is) on
small float32 images.

    python tools/make_golden_cutout.py          # needs the reference tree (oracle/ref_stub.py)

Stand-ins: numpy.random.randint is redirected to the CutOut sub-stream of the counter-based generator
(tests/cutout_ref.CutoutStream, keyed by (seed, iteration, image)); the image is handed over as an ndarray subclass
that records the slices the reference assigns, so the hole rectangles in the fixture are the reference's own x1 / y1 /
x2 / y2, not a restatement.

Fixture, for every configuration of cutout_ref.CONFIGS and every edge of cutout_ref.EDGES (N_IMAGES images each, image
i of edge e at iteration ITERATION + EDGES.index(e)):
    in_<edge>            float32 [n, 3, e, e]   the input images (cutout_ref.pattern)
    holes_<cfg>_<edge>   int32 [n, WORDS]       n_holes, draws consumed, (x1, y1, x2, y2) per hole
    out_<cfg>_<edge>     float32 [n, 3, e, e]   the reference's output images
The tool refuses to write a fixture without the hard cases: a hole clipped at the right edge and one at the bottom edge
for every image edge, an image that draws 0 holes, an empty hole.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import cutout_ref as R         # noqa: E402
import ref_stub                # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'cutout.npz')


class Recorded(np.ndarray):
    """An image that notes the (y, x) slices assigned to it."""

    def __setitem__(self, key, value):
        ys, xs = key[0], key[1]
        self.assigned.append((int(xs.start), int(ys.start), int(xs.stop), int(ys.stop)))
        super().__setitem__(key, value)


def run_reference(T, cfg, imgs, seed, iteration):
    """The reference class on imgs float32 [n, 3, e, e] -> (tables int32 [n, WORDS], outputs [n, 3, e, e])."""
    op = T.CutOut(**cfg)
    tables, outs = np.zeros((len(imgs), R.WORDS), np.int32), np.empty_like(imgs)
    saved = np.random.randint
    try:
        for i, im in enumerate(imgs):
            st = R.CutoutStream(seed, iteration, i)
            np.random.randint = st.randint
            hwc = np.ascontiguousarray(im.transpose(1, 2, 0)).view(Recorded)
            hwc.assigned = []
            res = op(dict(img=hwc))
            n = st.log[0][2]
            assert len(hwc.assigned) == n and st.ctr == 1 + 3 * n
            tables[i, 0], tables[i, 1] = n, st.ctr
            tables[i, 2:2 + 4 * n] = np.array(hwc.assigned, np.int32).reshape(-1)
            outs[i] = np.asarray(res['img']).transpose(2, 0, 1)
    finally:
        np.random.randint = saved
    return tables, outs


def hard_cases(pack):
    """-> dict of what the fixture contains, from its tables alone (tests/test_cutout.py asserts the same)."""
    seen = dict(zero_holes=False, empty_hole=False)
    for e in R.EDGES:
        seen[f'right_{e}'] = seen[f'bottom_{e}'] = False
    for name in R.CONFIGS:
        for e in R.EDGES:
            for row in pack[f'holes_{name}_{e}']:
                seen['zero_holes'] |= row[0] == 0
                for j in range(row[0]):
                    x1, y1, x2, y2 = row[2 + 4 * j:6 + 4 * j]
                    seen['empty_hole'] |= x2 == x1 or y2 == y1
                    seen[f'right_{e}'] |= x2 == e and x1 < x2
                    seen[f'bottom_{e}'] |= y2 == e and y1 < y2
    return seen


def main():
    if not ref_stub.available():
        raise SystemExit('needs the reference tree')
    T = ref_stub.load_pipeline_transforms()
    pack = dict(seed=R.SEED, iteration=R.ITERATION, configs=np.array(repr(R.CONFIGS)))
    for k, e in enumerate(R.EDGES):
        imgs = R.pattern(R.N_IMAGES, e)
        pack[f'in_{e}'] = imgs
        for name, cfg in R.CONFIGS.items():
            pack[f'holes_{name}_{e}'], pack[f'out_{name}_{e}'] = run_reference(T, cfg, imgs, R.SEED, R.ITERATION + k)
    seen = hard_cases(pack)
    missing = [k for k, v in seen.items() if not v]
    if missing:
        raise SystemExit(f'seed {R.SEED}: the fixture lacks {missing}; choose another cutout_ref.SEED')
    np.savez_compressed(OUT, **pack)
    print('cutout.npz', os.path.getsize(OUT), 'bytes;', {n: int(sum(pack[f'holes_{n}_{e}'][:, 0].sum() for e in R.EDGES))
                                                          for n in R.CONFIGS}, 'holes')


if __name__ == '__main__':
    main()
