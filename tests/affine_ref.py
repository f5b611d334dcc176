"""TEST INFRASTRUCTURE ONLY -- restatement of RandomAffine with landmarks as the device pipeline runs it
(mmdet/datasets/pipelines/transforms.py:2787-3001 of the reference; csrc/augment.hip aug_affine_decide_kernel and
aug_affine_pixels_kernel; include/yunet_hip.h YUNET_AFFINE_*).  Nothing in the product imports this.

Randomness.  The reference draws six numpy.random.uniform(a, b) per image.  Here they come from a SUB-STREAM of the
counter-based generator of oracle/pipeline_oracle.py: key mix32(stream_key(seed, iteration, image) ^ SALT), counter from
0, uniform(a, b) = a + (b - a) * (u32 / 2^32) in Python's doubles (mosaic_ref.MosaicStream.py_uniform).

Two evaluations of the same formulas.  `dtype=np.float64`: the yardstick -- trigonometry, factors, products, corners,
clip and the filter quantities all in doubles, nothing rounded on the way.  `dtype=np.float32`: the reference's (and the
kernel's) arithmetic -- the factors rounded to float32, the products, corners and filter quantities in float32.  The
tolerance of a comparison against the yardstick is a multiple of the distance between the two (tools/make_golden_affine.py
records it in the fixture).  The pixels are this project's own arithmetic: `warp_pixels` restates the kernel, in either
precision; cv2's 1/32-pixel coordinate table is not reproduced.
"""
import math

import numpy as np

import pipeline_oracle as P

SALT = 0x41464649                       # YUNET_AFFINE_SALT ("AFFI")
WORDS = 24                              # YUNET_AFFINE_WORDS, doubles
DRAWS, MAT, INV, ROWS_IN, ROWS_OUT, EDGE = 0, 6, 15, 21, 22, 23
DEFAULTS = dict(max_rotate_degree=10.0, max_translate_ratio=0.1, scaling_ratio_range=(0.5, 1.5), max_shear_degree=2.0,
                border_val=(114, 114, 114), min_bbox_size=2, min_area_ratio=0.2, max_aspect_ratio=20,
                bbox_clip_border=True, skip_filter=True)


def affine_key(seed, iteration, image):
    return P.mix32(P.stream_key(seed, iteration, image) ^ SALT)


class AffineStream(P.Stream):
    """The RandomAffine draws of one image behind numpy's uniform; `log` records (low, high, value) of every call."""

    def __init__(self, seed, iteration, image):
        super().__init__(seed, iteration, image)
        self.key = affine_key(seed, iteration, image)
        self.log = []

    def py_uniform(self, low=0.0, high=1.0, size=None):
        assert size is None
        v = low + (high - low) * self.uniform()
        self.log.append((low, high, v))
        return v


def full(cfg):
    return dict(DEFAULTS, **cfg)


def draws(seed, iteration, image, cfg):
    """The six draws in RandomAffine.__call__'s order -> float64 [6]: rotation degrees, scaling ratio, shear x / y degrees,
    translate x / y ratio (the reference multiplies the last two by width / height)."""
    c, st = full(cfg), AffineStream(seed, iteration, image)
    r, (lo, hi), s, t = c['max_rotate_degree'], c['scaling_ratio_range'], c['max_shear_degree'], c['max_translate_ratio']
    return np.array([st.py_uniform(-r, r), st.py_uniform(lo, hi), st.py_uniform(-s, s), st.py_uniform(-s, s),
                     st.py_uniform(-t, t), st.py_uniform(-t, t)], np.float64)


def matrix(d, S, dtype):
    """M = T @ Sh @ R @ Sc from the six draws for an S x S image.  float32: the reference's own construction (factors
    made with dtype=float32, products in float32 from the left, each entry summed from the left).  float64: the same
    formulas in doubles."""
    rad, xr, yr = math.radians(d[0]), math.radians(d[2]), math.radians(d[3])
    R = np.array([[np.cos(rad), -np.sin(rad), 0.], [np.sin(rad), np.cos(rad), 0.], [0., 0., 1.]], dtype)
    Sc = np.array([[d[1], 0., 0.], [0., d[1], 0.], [0., 0., 1.]], dtype)
    Sh = np.array([[1, np.tan(xr), 0.], [np.tan(yr), 1, 0.], [0., 0., 1.]], dtype)
    T = np.array([[1, 0., d[4] * S], [0., 1, d[5] * S], [0., 0., 1.]], dtype)

    def mm(a, b):
        return (a[:, 0:1] * b[0:1, :] + a[:, 1:2] * b[1:2, :]) + a[:, 2:3] * b[2:3, :]
    return mm(mm(mm(T, Sh), R), Sc)


def inverse(M):
    """The upper two rows of M^-1 in doubles (M affine: bottom row 0 0 1) -> float64 [6] (i00 i01 i02 i10 i11 i12)."""
    a, b, c, e, f, h = (float(v) for v in np.asarray(M, np.float64)[:2].reshape(-1))
    det = a * f - b * e
    return np.array([f / det, -b / det, (b * h - c * f) / det, -e / det, a / det, (c * e - a * h) / det], np.float64)


def warp_points(M, x, y):
    return (M[0, 0] * x + M[0, 1] * y) + M[0, 2], (M[1, 0] * x + M[1, 1] * y) + M[1, 2]


def warp_boxes(M, boxes, S, clip, raw=False):
    """boxes [G, 4] in M's dtype -> the axis-aligned hull of the four warped corners [G, 4], clipped to [0, S]
    (raw=True: also the hull before the clip)."""
    b = np.asarray(boxes, M.dtype).reshape(-1, 4)
    xs, ys = warp_points(M, b[:, [0, 0, 2, 2]], b[:, [1, 3, 3, 1]])
    hull = np.stack([xs.min(1), ys.min(1), xs.max(1), ys.max(1)], 1)
    out = hull.clip(0, S).astype(M.dtype) if clip else hull
    return (out, hull) if raw else out


def warp_kps(M, kps, S, clip):
    """kps [G, 5, 3] -> (x, y) through M, clipped to [0, S] as Resize._resize_keypoints clips; the third value stays."""
    k = np.asarray(kps, M.dtype).reshape(-1, 5, 3).copy()
    x, y = warp_points(M, k[:, :, 0].copy(), k[:, :, 1].copy())
    k[:, :, 0], k[:, :, 1] = (x.clip(0, S), y.clip(0, S)) if clip else (x, y)
    return k


def rules(boxes, wb, scale, S, cfg):
    """find_inside_bboxes and the three rules of filter_gt_bboxes for warped boxes wb of input boxes, in wb's dtype ->
    bool [G, 4]: inside, width / height, area ratio, aspect ratio (the last three True under skip_filter)."""
    c, dt = full(cfg), wb.dtype.type
    inside = (wb[:, 0] < S) & (wb[:, 2] > 0) & (wb[:, 1] < S) & (wb[:, 3] > 0)
    ok = np.ones((len(wb), 4), bool)
    ok[:, 0] = inside
    if not c['skip_filter']:
        ob = np.asarray(boxes, wb.dtype).reshape(-1, 4) * dt(scale)
        ow, oh = ob[:, 2] - ob[:, 0], ob[:, 3] - ob[:, 1]
        w, h = wb[:, 2] - wb[:, 0], wb[:, 3] - wb[:, 1]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            aspect = np.maximum(w / (h + dt(1e-16)), h / (w + dt(1e-16)))
            ok[:, 1] = (w > dt(c['min_bbox_size'])) & (h > dt(c['min_bbox_size']))
            ok[:, 2] = w * h / (ow * oh + dt(1e-16)) > dt(c['min_area_ratio'])
            ok[:, 3] = aspect < dt(c['max_aspect_ratio'])
    return ok


def clearance(boxes, scale, M64, S, cfg):
    """How far each row's decision is from flipping, in pixels of box-coordinate error -> float64 [G].  A quantity q
    compared with a threshold t counts |q - t| / k, k = how fast q moves per pixel of error in a warped coordinate
    (1 for an edge, 2 for a width, q * (2 / w + 2 / h) for the area and the aspect ratio).  A surviving row needs every
    comparison to hold by that much; a removed row needs one failing comparison that fails by that much."""
    c = full(cfg)
    wb, hull = warp_boxes(M64, boxes, S, c['bbox_clip_border'], raw=True)
    ok = rules(boxes, wb, scale, S, cfg)
    G = len(wb)
    dist = np.full((G, 4), np.inf)
    # the clip is monotonic, so the inside tests decide on the hull as they do on the clipped box
    edge = np.stack([S - hull[:, 0], hull[:, 2], S - hull[:, 1], hull[:, 3]], 1)
    dist[:, 0] = np.where(ok[:, 0], np.abs(edge).min(1), np.where(edge <= 0, -edge, -np.inf).max(1))
    if not c['skip_filter']:
        w, h = wb[:, 2] - wb[:, 0], wb[:, 3] - wb[:, 1]
        ob = np.asarray(boxes, np.float64).reshape(-1, 4) * scale
        with np.errstate(divide='ignore', invalid='ignore'):
            k = 2.0 / w + 2.0 / h
            ratio = w * h / ((ob[:, 2] - ob[:, 0]) * (ob[:, 3] - ob[:, 1]) + 1e-16)
            aspect = np.maximum(w / (h + 1e-16), h / (w + 1e-16))
            mb = float(c['min_bbox_size'])
            wh = np.stack([w - mb, h - mb], 1) / 2.0
            dist[:, 1] = np.where(ok[:, 1], np.abs(wh).min(1), np.where(wh <= 0, -wh, -np.inf).max(1))
            dist[:, 2] = np.abs(ratio - c['min_area_ratio']) / (ratio * k)
            dist[:, 3] = np.abs(aspect - c['max_aspect_ratio']) / (aspect * k)
        dist = np.nan_to_num(dist, nan=0.0)
    keep = ok.all(1)
    return np.where(keep, dist.min(1), np.where(ok, -np.inf, dist).max(1))


def decide(seed, iteration, image, boxes, kps, S, cfg, dtype=np.float64):
    """One image -> dict(draws, M, wb [G,4] warped boxes of every row, kps [G,5,3] of every row, valid bool [G])."""
    c = full(cfg)
    d = draws(seed, iteration, image, cfg)
    M = matrix(d, S, dtype)
    wb = warp_boxes(M, boxes, S, c['bbox_clip_border'])
    return dict(draws=d, M=M, wb=wb, kps=warp_kps(M, kps, S, c['bbox_clip_border']),
                valid=rules(boxes, wb, d[1], S, cfg).all(1))


def warp_pixels(img, inv, border_val, dtype, S=None):
    """The kernel's warp of img [3, E, E] (float32 values) by the inverse words `inv` [6], with coordinates, weights and
    the weighted sum in `dtype`; S: the image's own edge inside the E x E canvas (pixels at or beyond it are 0)."""
    E = img.shape[-1]
    S = E if S is None else S
    dt = dtype
    i = np.asarray(inv, np.float64).astype(np.float32).astype(dt)      # the kernel rounds the stored doubles to float32
    y, x = np.mgrid[:S, :S].astype(dt)
    sx = (i[0] * x + i[1] * y) + i[2]
    sy = (i[3] * x + i[4] * y) + i[5]
    live = (sx > -1) & (sx < S) & (sy > -1) & (sy < S)
    sx, sy = np.where(live, sx, 0), np.where(live, sy, 0)
    fx, fy = np.floor(sx), np.floor(sy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    ax, ay = (sx - fx).astype(dt), (sy - fy).astype(dt)
    one = dt(1)
    w = [(one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay]
    out = np.zeros((3, E, E), dt)
    bv = np.asarray(border_val, np.float32).astype(dt).reshape(3)
    src = np.asarray(img, np.float32).astype(dt)
    for c in range(3):
        taps = []
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            yy, xx = y0 + dy, x0 + dx
            inside = (yy >= 0) & (yy < S) & (xx >= 0) & (xx < S)
            taps.append(np.where(inside, src[c, yy.clip(0, S - 1), xx.clip(0, S - 1)], bv[c]))
        v = ((w[0] * taps[0] + w[1] * taps[1]) + w[2] * taps[2]) + w[3] * taps[3]
        v = np.where((ax == 0) & (ay == 0), taps[0], v)          # on the pixel grid: the pixel itself
        out[c, :S, :S] = np.where(live, v, bv[c])
    return out


# ------------------------------------------------------------------ the fixture's cases (tests/golden/affine_cases.npz)
SEED, ITERATION, N_IMAGES, EDGES, GMAX = 11, 2, 4, (32, 64), 8
MARGIN = 1e-3       # pixels: every decision of a fixture case is clear of its thresholds by this much; the bars stay below
CONFIGS = {
    'defaults': dict(),
    'filter': dict(skip_filter=False),
    'filter_tight': dict(skip_filter=False, max_rotate_degree=3.0, max_translate_ratio=0.3, min_area_ratio=0.5,
                         max_aspect_ratio=4),
    'unclipped': dict(bbox_clip_border=False, max_translate_ratio=0.3),
    'rotate': dict(max_rotate_degree=30.0, max_translate_ratio=0.0, scaling_ratio_range=(1.0, 1.0), max_shear_degree=0.0),
    'shear': dict(max_rotate_degree=0.0, max_translate_ratio=0.0, scaling_ratio_range=(1.0, 1.0), max_shear_degree=20.0),
    'translate': dict(max_rotate_degree=0.0, max_translate_ratio=0.5, scaling_ratio_range=(1.0, 1.0),
                      max_shear_degree=0.0),
}


def inputs(edge):
    """GT of the four images of an edge -> (boxes float32 [4, GMAX, 4], kps float32 [4, GMAX, 5, 3], counts int32 [4]),
    rows at and beyond the count 0.  Image 0: boxes around the centre; image 1: a box at every side, a large one, a
    corner one, a thin and a tiny one; image 2: random boxes; image 3: two tiny boxes in the far corner."""
    e, rng = float(edge), np.random.default_rng(1000 + edge)
    per = []
    c = rng.uniform(0.3 * e, 0.6 * e, (GMAX, 2))
    per.append(np.concatenate([c, c + rng.uniform(3.0, 0.15 * e, (GMAX, 2))], 1))
    per.append(np.array([[1.0, 0.4 * e, 0.2 * e, 0.6 * e], [0.4 * e, 0.5, 0.6 * e, 0.2 * e],
                         [0.8 * e, 0.4 * e, e - 1.0, 0.6 * e], [0.4 * e, 0.8 * e, 0.6 * e, e - 0.5],
                         [0.1 * e, 0.1 * e, 0.9 * e, 0.9 * e], [0.85 * e, 0.85 * e, e - 0.5, e - 0.5],
                         [0.3 * e, 0.2 * e, 0.3 * e + 3.0, 0.8 * e], [0.5 * e, 0.25 * e, 0.5 * e + 1.5, 0.25 * e + 1.25]]))
    c = rng.uniform(0.0, 0.8 * e, (6, 2))
    per.append(np.concatenate([c, np.minimum(c + rng.uniform(2.5, 0.4 * e, (6, 2)), e)], 1))
    per.append(np.array([[e - 3.0, e - 3.5, e - 1.5, e - 2.0], [e - 6.0, e - 2.0, e - 4.5, e - 0.5]]))
    boxes, kps = np.zeros((N_IMAGES, GMAX, 4), np.float32), np.zeros((N_IMAGES, GMAX, 5, 3), np.float32)
    counts = np.array([len(b) for b in per], np.int32)
    for i, b in enumerate(per):
        g = len(b)
        boxes[i, :g] = b
        t = rng.uniform(0.0, 1.0, (g, 5, 2))
        kps[i, :g, :, 0] = b[:, None, 0] + t[:, :, 0] * (b[:, None, 2] - b[:, None, 0])
        kps[i, :g, :, 1] = b[:, None, 1] + t[:, :, 1] * (b[:, None, 3] - b[:, None, 1])
        kps[i, :g, :, 2] = np.array([1.0, 0.0, -1.0])[np.arange(g) % 3][:, None]
        kps[i, :g][kps[i, :g, :, 2] < 0, :2] = -1.0         # a face without landmarks: (-1, -1, -1) rows
    return boxes, kps, counts


def pattern(n, edge):
    """Input images float32 [n, 3, edge, edge]: a sawtooth in x and y, every value k + 0.25, none equal to 114."""
    i, c, y, x = np.ogrid[:n, :3, :edge, :edge]
    return ((i * 13 + c * 29 + y * 7 + x * 3) % 199 + 1.25).astype(np.float32)
