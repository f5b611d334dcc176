"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the reference TRAIN pipeline with
Resize(img_scale=(a, b), multiscale_mode='square_range', keep_ratio=False)  (mmdet/datasets/pipelines/transforms.py:99,
128-149, 226-228), built on oracle/pipeline_oracle.py.  Nothing in the product imports this.

Per image, in the order of the pipeline list:
  RandomSquareCrop   pipeline_oracle.decide_crop (its draws)
  Resize             ONE more draw, numpy.random.randint(lo, hi + 1), lo = min(img_scale), hi = max(img_scale);
                     S_n = edge // 32 * 32; then pipeline_oracle's resize arithmetic with S = S_n
  RandomFlip         one uniform
so the stream (seed, iteration, image) of a square_range run is NOT the fixed-size stream with a draw appended: the
flip uniform moves one counter on.  An image without a usable crop window (outside the reference's contract: it would
loop forever) still makes the Resize draw, so that its S_n is defined -- csrc/augment.hip does the same.

Collate: DefaultFormatBundle wraps the image with padding_value=0, stack=True (formatting.py:202, 231) and mmcv's
collate pads the images of a samples_per_gpu group at the bottom and right, with that value, up to the group's largest
shape: [N, 3, Smax, Smax], image n in the top-left S_n x S_n corner, 0.0 elsewhere.  Value and stacking are the
reference's; the bottom / right placement is mmcv's rule, restated without mmcv at hand (PARITY UNPINNED for that)."""
import os

import numpy as np

import pipeline_oracle as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CROP_CHOICE = [0.5, 0.7, 0.9, 1.1, 1.3, 1.5]


def out_sizes(lo, hi):
    """The S_n an image can draw: the multiples of 32 in [lo // 32 * 32, hi // 32 * 32]."""
    return list(range(lo // 32 * 32, hi // 32 * 32 + 1, 32))


def augment_image(img_u8, boxes, kps, seed, iteration, image, lo, hi, crop_choice, flip_ratio=0.5, pad=128.0):
    """One image through crop -> resize(square_range) -> flip.  -> dict(img [3,S_n,S_n] f32, boxes, kps,
    params = (left, top, cw, flip), mask, S, draws, status); status 1: no window, img is all `pad`, no GT."""
    h, w = img_u8.shape[:2]
    st = P.Stream(seed, iteration, image)
    dec = P.decide_crop(h, w, boxes, crop_choice, st)
    S = st.randint(lo, hi + 1) // 32 * 32                       # transforms.py:146-147
    if dec is None:
        return dict(img=np.full((3, S, S), pad, np.float32), boxes=boxes[:0], kps=kps[:0],
                    params=np.zeros(4, np.int32), mask=np.zeros(len(boxes), bool), S=S, draws=st.ctr, status=1)
    left, top, cw = dec
    b, k, mask = P.crop_gt(boxes, kps, left, top, cw)
    b, k = P.resize_gt(b, k, cw, S)
    flip = st.uniform() < flip_ratio
    im = P.resize_linear(P.crop_image(img_u8.astype(np.float32), left, top, cw, pad), S)
    if flip:
        b, k = P.flip_gt(b, k, S)
        im = im[:, ::-1]
    return dict(img=np.ascontiguousarray(im.transpose(2, 0, 1)), boxes=b, kps=k,
                params=np.array([left, top, cw, int(flip)], dtype=np.int32), mask=mask, S=S, draws=st.ctr, status=0)


def collate_canvas(results):
    """[N, 3, Smax, Smax]: image n in the top-left corner, zeros below and to the right."""
    smax = max(r['S'] for r in results)
    out = np.zeros((len(results), 3, smax, smax), np.float32)
    for i, r in enumerate(results):
        out[i, :, :r['S'], :r['S']] = r['img']
    return out


def image_digest(im):
    """What the fixtures keep of an output image [3, S, S] (as tests/golden/pipeline_s*.npz): per-channel sum and sum of
    squares in float64, the top-left 16 x 16 window and the 16 x 16 window at the centre."""
    S = im.shape[1]
    dig = np.stack([im.astype(np.float64).sum((1, 2)), (im.astype(np.float64) ** 2).sum((1, 2))])
    return dig, im[:, :16, :16].copy(), im[:, S // 2 - 8:S // 2 + 8, S // 2 - 8:S // 2 + 8].copy()


def load_case(name):
    """tests/golden/pipeline_multiscale.npz, set `name` -> (dict of that set's arrays, seed, iteration, lo, hi, sources);
    the uint8 sources are regenerated from the seed (pipeline_oracle.synth_image) and checked against the fixture."""
    z = np.load(os.path.join(GOLD, 'pipeline_multiscale.npz'))
    g = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + '/')}
    seed, it, lo, hi, n = (int(g[k]) for k in ('seed', 'iteration', 'lo', 'hi', 'n'))
    rng = np.random.default_rng(seed)
    srcs = []
    for i in range(n):
        h, w, total = [int(v) for v in g[f'src_shape_{i}']]
        img, boxes, kps = P.synth_image(rng, h, w, int(g[f'src_g_{i}']))
        assert int(img.astype(np.int64).sum()) == total, 'synthetic source drifted from the fixture'
        assert np.array_equal(boxes, g[f'src_boxes_{i}']) and np.array_equal(kps, g[f'src_kps_{i}'])
        srcs.append((img, boxes, kps))
    return g, seed, it, lo, hi, srcs


SETS = ('r160_320', 'r320_640')
