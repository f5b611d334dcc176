"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the reference's Mosaic(use_kps=True) under
MultiImageMixDataset (mmdet/datasets/pipelines/transforms.py:2218-2519, mmdet/datasets/dataset_wrappers.py:338-444),
built on oracle/pipeline_oracle.py.  Nothing in the product imports this; tools/make_golden_mosaic.py uses its generator
sub-stream to serve the reference's `random` draws, and tests/test_mosaic*.py compare it and the device against
tests/golden/mosaic_*.npz.

Per output image n of iteration it, draws from the sub-stream key mix32(stream_key(seed, it, n) ^ MOSAIC_SALT):
  3 x partner index in [0, M)   (get_indexes: numpy's randint(0, M), transforms.py:10 imports numpy's `random`)
  1 x uniform(0, 1) > prob      -> the image passes through unchanged
  2 x uniform(lo, hi)           -> center_x = int(. * S), center_y = int(. * S)
then per sub-image (top-left = the image itself, top-right, bottom-left, bottom-right): r = min(S / h, S / w), the cv2
float-bilinear resize to (int(w * r), int(h * r)), _mosaic_combine, paste; GT r * v + pad in float32 (a Python float
scalar against a float32 array), clip, min_bbox_size filter, find_inside_bboxes."""
import os

import numpy as np

import pipeline_oracle as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MOSAIC_SALT = 0x4D4F5341
CROP_CHOICE = [0.5, 0.7, 0.9, 1.1, 1.3, 1.5]


class MosaicStream(P.Stream):
    """The mosaic sub-stream of image (seed, iteration, image)."""

    def __init__(self, seed, iteration, image):
        self.key = P.mix32(P.stream_key(seed, iteration, image) ^ MOSAIC_SALT)
        self.ctr = 0

    def py_uniform(self, a, b):             # numpy.random.uniform(a, b) = a + (b - a) * random_sample()
        return a + (b - a) * self.uniform()


def draws(seed, iteration, image, m, S, prob=1.0, center_ratio_range=(0.5, 1.5)):
    """-> (partners [3], applied, center_x, center_y, draws consumed)."""
    st = MosaicStream(seed, iteration, image)
    partners = [st.randint(0, m) for _ in range(3)]
    if st.py_uniform(0, 1) > prob:
        return partners, False, 0, 0, st.ctr
    cx = int(st.py_uniform(*center_ratio_range) * S)
    cy = int(st.py_uniform(*center_ratio_range) * S)
    return partners, True, cx, cy, st.ctr


def combine(q, cx, cy, rw, rh, S):
    """_mosaic_combine for sub-image q (0..3) -> (paste x1, y1, x2, y2), (crop x1, y1, x2, y2)."""
    if q == 0:
        x1, y1, x2, y2 = max(cx - rw, 0), max(cy - rh, 0), cx, cy
        crop = rw - (x2 - x1), rh - (y2 - y1), rw, rh
    elif q == 1:
        x1, y1, x2, y2 = cx, max(cy - rh, 0), min(cx + rw, S * 2), cy
        crop = 0, rh - (y2 - y1), min(rw, x2 - x1), rh
    elif q == 2:
        x1, y1, x2, y2 = max(cx - rw, 0), cy, cx, min(S * 2, cy + rh)
        crop = rw - (x2 - x1), 0, rw, min(y2 - y1, rh)
    else:
        x1, y1, x2, y2 = cx, cy, min(cx + rw, S * 2), min(S * 2, cy + rh)
        crop = 0, 0, min(rw, x2 - x1), min(y2 - y1, rh)
    return (x1, y1, x2, y2), crop


def resize_wh(img, rw, rh):
    """pipeline_oracle.resize_linear to a rectangle: float32 bilinear, horizontal pass then vertical pass, no FMA."""
    h, w = img.shape[:2]
    sx, sx1, a0, a1 = P.linear_coeffs(rw, w)
    sy, sy1, b0, b1 = P.linear_coeffs(rh, h)
    img = img.astype(np.float32)
    rows = (img[:, sx] * a0[None, :, None] + img[:, sx1] * a1[None, :, None]).astype(np.float32)
    return (rows[sy] * b0[:, None, None] + rows[sy1] * b1[:, None, None]).astype(np.float32)


def mosaic(samples, cx, cy, S, pad_val=114, bbox_clip_border=True, skip_filter=True, min_bbox_size=0, with_image=True):
    """samples: four (img uint8 [h,w,3], boxes [G,4], kps [G,5,3]) in the sub-image order ->
    dict(canvas [2S,2S,3] f32 | None, boxes, kps, kept (indices into the concatenated GT), geom [4, 11] int64 rows
    (h, w, rw, rh, paste x1 y1 x2 y2, crop x1 y1, G), clipped = all boxes after the clip, before the filters)."""
    canvas = np.full((2 * S, 2 * S, 3), pad_val, np.float32) if with_image else None
    mb, mk, geom = [], [], []
    for q, (img, boxes, kps) in enumerate(samples):
        h, w = img.shape[:2]
        r = min(S / h, S / w)
        rw, rh = int(w * r), int(h * r)
        (x1, y1, x2, y2), (c1, c2, c3, c4) = combine(q, cx, cy, rw, rh, S)
        if with_image:
            canvas[y1:y2, x1:x2] = resize_wh(img, rw, rh)[c2:c4, c1:c3]
        b, k = boxes.astype(np.float32).copy(), kps.astype(np.float32).copy()
        if len(b):
            r32, pw, ph = np.float32(r), np.float32(x1 - c1), np.float32(y1 - c2)
            b[:, 0::2] = r32 * b[:, 0::2] + pw
            b[:, 1::2] = r32 * b[:, 1::2] + ph
            k[:, :, 0] = r32 * k[:, :, 0] + pw
            k[:, :, 1] = r32 * k[:, :, 1] + ph
        mb.append(b)
        mk.append(k)
        geom.append([h, w, rw, rh, x1, y1, x2, y2, c1, c2, len(b)])
    b, k = np.concatenate(mb, 0), np.concatenate(mk, 0)
    kept = np.arange(len(b))
    lim = np.float32(2 * S)
    if bbox_clip_border:
        b = np.clip(b, np.float32(0), lim)
        k[..., :2] = np.clip(k[..., :2], np.float32(0), lim)
    clipped = b.copy()
    if not skip_filter:
        ok = ((b[:, 2] - b[:, 0]) > np.float32(min_bbox_size)) & ((b[:, 3] - b[:, 1]) > np.float32(min_bbox_size))
        b, k, kept = b[ok], k[ok], kept[ok]
    ok = (b[:, 0] < lim) & (b[:, 2] > 0) & (b[:, 1] < lim) & (b[:, 3] > 0)
    return dict(canvas=canvas, boxes=b[ok], kps=k[ok], kept=kept[ok], geom=np.array(geom, np.int64), clipped=clipped)


def run_case(case, srcs, with_image=True):
    """The restatement over one fixture case (load_case) -> per output image a dict(partners, applied, cx, cy, draws,
    + mosaic(...) when applied, or the image's own boxes / kps when skipped)."""
    out = []
    m, S = len(srcs), case['S']
    for n, own in enumerate(case['idx']):
        partners, applied, cx, cy, nd = draws(case['seed'], case['iteration'], n, m, S, case['prob'], case['center'])
        r = dict(partners=partners, applied=applied, cx=cx, cy=cy, draws=nd)
        if applied:
            r.update(mosaic([srcs[i] for i in [own] + partners], cx, cy, S, case['pad_val'], case['clip'],
                            case['skip_filter'], case['min_bbox_size'], with_image))
        else:
            r.update(boxes=srcs[own][1], kps=srcs[own][2], kept=np.arange(len(srcs[own][1])), canvas=None,
                     geom=np.zeros((4, 11), np.int64))
        out.append(r)
    return out


# ---- the fixture ---------------------------------------------------------------------------------------------------
#          (h, w, g): g as pipeline_oracle.synth_image; 0 = no GT.  Portrait, landscape, smaller / larger than S, one with
#          more than 64 faces; 'edge' adds boxes that straddle the image border (the clip makes some degenerate).
SOURCES = [(120, 200, 3), (333, 250, 9), (97, 97, 1), (480, 640, 24), (400, 600, 0), (600, 400, -2), (300, 300, 0),
           (256, 384, 5), (500, 375, 70), (150, 150, 2), (160, 160, 7), (80, 160, 4)]
#          name         seed it  S    idx (the batch's store indices)  prob center        clip  skip_f min_bbox pad
CASES = [('default',     41, 3, 160, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], 1.0, (0.5, 1.5), True, True, 0, 114),
         ('lo_end',      42, 0, 160, [3, 8, 0, 10], 1.0, (0.5, 0.5), True, True, 0, 114),
         ('hi_end',      43, 1, 160, [3, 8, 1, 11], 1.0, (1.5, 1.5), True, True, 0, 114),
         ('corner0',     44, 2, 160, [8, 3, 4, 10], 1.0, (0.0, 0.0), True, True, 0, 114),
         ('corner2',     45, 2, 160, [8, 3, 6, 10], 1.0, (2.0, 2.0), True, True, 0, 114),
         ('filter',      46, 5, 160, [0, 1, 3, 5, 8, 9, 10, 7], 1.0, (0.5, 1.5), True, False, 6, 114),
         ('noclip',      47, 6, 160, [1, 3, 8, 7, 5, 10], 1.0, (0.25, 1.75), False, False, 2, 114),
         ('prob',        48, 7, 160, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], 0.5, (0.5, 1.5), True, True, 0, 114),
         ('big',         49, 8, 320, [8, 3, 1, 7, 10], 1.0, (0.5, 1.5), True, True, 0, 0),
         ('empty',       50, 9, 160, [0, 1], 1.0, (0.5, 1.5), True, True, 0, 114)]
EMPTY_SOURCES = [(200, 300, 0), (300, 200, 0), (160, 160, 0)]      # case 'empty': a store without any GT


def make_sources(which='main'):
    rng = np.random.default_rng(4242 if which == 'main' else 4343)
    out = []
    for h, w, g in (SOURCES if which == 'main' else EMPTY_SOURCES):
        if g == 0:
            img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
            out.append((img, np.zeros((0, 4), np.float32), np.zeros((0, 5, 3), np.float32)))
            continue
        img, b, k = P.synth_image(rng, h, w, g)
        if g > 4:       # boxes across the image border: after r * v + pad they straddle a paste edge or the canvas edge
            b[0, :2] -= 0.4 * min(h, w)
            b[1, 2:] += 0.6 * min(h, w)
            b[2] = [-50.0, -60.0, -4.0, -3.0]           # wholly outside, top-left
            b[3] = [w + 3.0, h + 2.0, w + 40.0, h + 50.0]
        out.append((img, b, k))
    return out


def case_dict(row):
    name, seed, it, S, idx, prob, center, clip, skip_filter, mb, pad = row
    return dict(name=name, seed=seed, iteration=it, S=S, idx=list(idx), prob=prob, center=tuple(center), clip=clip,
                skip_filter=skip_filter, min_bbox_size=mb, pad_val=pad, store='empty' if name == 'empty' else 'main')


def load_fixture():
    """tests/golden/mosaic_cases.npz -> (z, {store name: sources}); the uint8 sources are regenerated from the seed and
    checked against the byte sums and GT the fixture recorded."""
    z = np.load(os.path.join(GOLD, 'mosaic_cases.npz'))
    stores = {}
    for which in ('main', 'empty'):
        srcs = make_sources(which)
        for i, (img, b, k) in enumerate(srcs):
            assert int(img.astype(np.int64).sum()) == int(z[f'src/{which}/{i}/sum']), 'synthetic source drifted'
            assert np.array_equal(b, z[f'src/{which}/{i}/boxes']) and np.array_equal(k, z[f'src/{which}/{i}/kps'])
        stores[which] = srcs
    return z, stores
