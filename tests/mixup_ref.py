"""TEST INFRASTRUCTURE ONLY -- restatement of MixUp with landmarks as the device pipeline runs it
(mmdet/datasets/pipelines/transforms.py:2523-2783 of the reference; csrc/augment.hip aug_mixup_decide_kernel and
aug_mixup_pixels_kernel; include/yunet_hip.h YUNET_MIXUP_*).  Nothing in the product imports this.

Randomness.  The reference draws numpy.random.randint / uniform.  Here they come from a SUB-STREAM of the counter-based
generator of oracle/pipeline_oracle.py: key mix32(stream_key(seed, iteration, image) ^ SALT), counter from 0.

The boxes are single float32 operations, so `decide` is compared byte for byte with the unmodified class.  The pixels
have two evaluations of the same formulas (`partner_value`): float32 -- cv2's float bilinear path as the kernel and the
fixture's `imresize` stand-in compute it -- and float64, the yardstick.  A pixel's admissible outputs follow from the
yardstick and a bar (`admissible`); tools/make_golden_mixup.py records the bar per edge.
"""
import numpy as np

import pipeline_oracle as P

SALT = 0x4D495855                       # YUNET_MIXUP_SALT ("MIXU")
WORDS = 18                              # YUNET_MIXUP_WORDS, doubles
(PARTNER, APPLIED, INDEX_DRAWS, JIT, FLIP, J_, RW, RH, XOFF, YOFF, SX, SY, ROWS_IN, ROWS_OUT, STATUS, EDGE, DRAWS,
 SR) = range(WORDS)
DEFAULTS = dict(ratio_range=(0.5, 1.5), flip_ratio=0.5, pad_val=114, max_iters=15, min_bbox_size=5, min_area_ratio=0.2,
                max_aspect_ratio=20, bbox_clip_border=True, skip_filter=True)
KP_FLIP = [1, 0, 2, 4, 3]               # RandomFlip.keypoints_flip


def mixup_key(seed, iteration, image):
    return P.mix32(P.stream_key(seed, iteration, image) ^ SALT)


class MixupStream(P.Stream):
    """The MixUp draws of one image behind numpy's randint / uniform; `log` records every call."""

    def __init__(self, seed, iteration, image):
        super().__init__(seed, iteration, image)
        self.key = mixup_key(seed, iteration, image)
        self.log = []

    def py_randint(self, low, high=None, size=None):
        assert size is None and high is not None
        v = int(self.randint(int(low), int(high)))
        self.log.append(('randint', low, high, v))
        return v

    def py_uniform(self, low=0.0, high=1.0, size=None):
        assert size is None
        v = low + (high - low) * self.uniform()
        self.log.append(('uniform', low, high, v))
        return v


def full(cfg):
    c = dict(DEFAULTS, **cfg)
    c.pop('use_kps', None)
    return c


# ------------------------------------------------------------------ geometry and GT
def geometry(seed, iteration, image, counts, hw, T, D, cfg):
    """The draws and the integer / double geometry of one image over a store with `counts` GT rows and sizes `hw` ->
    a table row float64 [WORDS] (ROWS_* / STATUS left 0)."""
    c, st = full(cfg), MixupStream(seed, iteration, image)
    t = np.zeros(WORDS)
    for _ in range(c['max_iters']):
        partner = st.py_randint(0, len(counts))
        if counts[partner] != 0:
            break
    t[PARTNER], t[INDEX_DRAWS], t[EDGE] = partner, st.ctr, T
    if counts[partner] != 0:
        h, w = (int(v) for v in hw[partner])
        jit = st.py_uniform(*c['ratio_range'])
        flip = st.py_uniform(0, 1) > c['flip_ratio']
        sr = min(D / h, D / w)
        rw, rh, J = int(w * sr), int(h * sr), int(D * jit)
        sr *= jit
        t[APPLIED], t[JIT], t[FLIP], t[J_], t[RW], t[RH], t[SR] = 1, jit, flip, J, rw, rh, sr
        t[SX], t[SY] = 1.0 / (float(rw) / float(w)), 1.0 / (float(rh) / float(h))
        if max(J, T) > T:
            t[YOFF] = st.py_randint(0, max(J, T) - T)
            t[XOFF] = st.py_randint(0, max(J, T) - T)
    t[DRAWS] = st.ctr
    return t


def partner_boxes(t, boxes, cfg, dtype=np.float32):
    """Raw partner boxes [G, 4] -> (before the offsets, after them), each [G, 4] in `dtype`: scale, clip to [0, J], flip,
    then the copy minus the offsets clipped to [0, T] -- one rounded operation each in float32."""
    c, dt = full(cfg), dtype
    J, T = dt(t[J_]), dt(t[EDGE])
    b = np.asarray(boxes, dt).reshape(-1, 4) * dt(t[SR])
    if c['bbox_clip_border']:
        b = b.clip(dt(0), J)
    if t[FLIP]:
        b[:, 0::2] = J - b[:, 0::2][:, ::-1]
    cp = b.copy()
    cp[:, 0::2] -= dt(t[XOFF])
    cp[:, 1::2] -= dt(t[YOFF])
    if c['bbox_clip_border']:
        cp = cp.clip(dt(0), T)
    return b, cp


def partner_kps(t, kps, cfg, dtype=np.float32):
    """Raw partner landmarks [G, 5, 3] -> [G, 5, 3]: (x, y) as the boxes; flipped: x = J - x with the points permuted."""
    c, dt = full(cfg), dtype
    J, T = dt(t[J_]), dt(t[EDGE])
    k = np.asarray(kps, dt).reshape(-1, 5, 3).copy()
    xy = k[:, :, :2] * dt(t[SR])
    if c['bbox_clip_border']:
        xy = xy.clip(dt(0), J)
    if t[FLIP]:
        k, xy = k[:, KP_FLIP], xy[:, KP_FLIP]
        xy[:, :, 0] = J - xy[:, :, 0]
    xy[:, :, 0] -= dt(t[XOFF])
    xy[:, :, 1] -= dt(t[YOFF])
    if c['bbox_clip_border']:
        xy = xy.clip(dt(0), T)
    k[:, :, :2] = xy
    return k


def rules(b, cp, T, cfg):
    """-> bool [G, 4]: find_inside_bboxes, then the three rules of _filter_box_candidates(before, after) (True under
    skip_filter), in the dtype of the boxes."""
    c, dt = full(cfg), cp.dtype.type
    ok = np.ones((len(cp), 4), bool)
    ok[:, 0] = (cp[:, 0] < T) & (cp[:, 2] > 0) & (cp[:, 1] < T) & (cp[:, 3] > 0)
    if not c['skip_filter']:
        w1, h1 = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        w2, h2 = cp[:, 2] - cp[:, 0], cp[:, 3] - cp[:, 1]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            ar = np.maximum(w2 / (h2 + dt(1e-16)), h2 / (w2 + dt(1e-16)))
            ok[:, 1] = (w2 > dt(c['min_bbox_size'])) & (h2 > dt(c['min_bbox_size']))
            ok[:, 2] = w2 * h2 / (w1 * h1 + dt(1e-16)) > dt(c['min_area_ratio'])
            ok[:, 3] = ar < dt(c['max_aspect_ratio'])
    return ok


def clearance(t, boxes, own, cfg):
    """How far every row's decision is from flipping, in pixels of box-coordinate error, evaluated in float64 -> float64
    [G_own + G] (affine_ref.clearance's measure: 1 per edge, 2 per width, q * (2 / w + 2 / h) for the two ratios)."""
    c, T = full(cfg), float(t[EDGE])
    b, cp = partner_boxes(t, boxes, dict(cfg, bbox_clip_border=False), np.float64)      # the clips are monotonic
    bc, cpc = partner_boxes(t, boxes, cfg, np.float64)
    ok = rules(bc, cpc, T, cfg)
    allb = np.concatenate([np.asarray(own, np.float64).reshape(-1, 4), cp])
    edge = np.stack([T - allb[:, 0], allb[:, 2], T - allb[:, 1], allb[:, 3]], 1)
    inside = (edge > 0).all(1)
    dist = np.full((len(allb), 4), np.inf)
    dist[:, 0] = np.where(inside, np.abs(edge).min(1), np.where(edge <= 0, -edge, -np.inf).max(1))
    g0 = len(allb) - len(cp)
    okk = np.ones((len(allb), 4), bool)
    okk[:, 0] = inside
    okk[g0:] = ok
    assert np.array_equal(ok[:, 0], inside[g0:])
    if not c['skip_filter'] and len(cp):
        w, h = cpc[:, 2] - cpc[:, 0], cpc[:, 3] - cpc[:, 1]
        with np.errstate(divide='ignore', invalid='ignore'):
            k = 2.0 / w + 2.0 / h
            ratio = w * h / ((bc[:, 2] - bc[:, 0]) * (bc[:, 3] - bc[:, 1]) + 1e-16)
            aspect = np.maximum(w / (h + 1e-16), h / (w + 1e-16))
            wh = np.stack([w - float(c['min_bbox_size']), h - float(c['min_bbox_size'])], 1) / 2.0
            d = dist[g0:]
            d[:, 1] = np.where(ok[:, 1], np.abs(wh).min(1), np.where(wh <= 0, -wh, -np.inf).max(1))
            d[:, 2] = np.abs(ratio - c['min_area_ratio']) / (ratio * k)
            d[:, 3] = np.abs(aspect - c['max_aspect_ratio']) / (aspect * k)
        dist = np.nan_to_num(dist, nan=0.0)
    keep = okk.all(1)
    return np.where(keep, dist.min(1), np.where(okk, -np.inf, dist).max(1))


def decide(seed, iteration, image, store, own_boxes, own_kps, T, D, cfg, gmax=None):
    """One image as the kernel has it -> dict(table, boxes [R, 4], kps [R, 5, 3], labels [R]): `store` = dict(hw, boxes,
    kps) with per-image lists; the labels are row numbers, the partner's from 1000 on.  gmax: rows beyond it dropped."""
    counts = [len(b) for b in store['boxes']]
    t = geometry(seed, iteration, image, counts, store['hw'], T, D, cfg)
    ob = np.asarray(own_boxes, np.float32).reshape(-1, 4)
    ok_ = np.asarray(own_kps, np.float32).reshape(-1, 5, 3)
    t[ROWS_IN] = len(ob)
    if not t[APPLIED]:
        boxes, kps, labels = ob, ok_, np.arange(len(ob))
    else:
        p = int(t[PARTNER])
        b, cp = partner_boxes(t, store['boxes'][p], cfg)
        keep = rules(b, cp, np.float32(T), cfg)[:, 1:].all(1)
        boxes = np.concatenate([ob, cp[keep]])
        kps = np.concatenate([ok_, partner_kps(t, store['kps'][p], cfg)[keep]])
        labels = np.concatenate([np.arange(len(ob)), 1000 + np.nonzero(keep)[0]])
        inside = (boxes[:, 0] < T) & (boxes[:, 2] > 0) & (boxes[:, 1] < T) & (boxes[:, 3] > 0)
        boxes, kps, labels = boxes[inside], kps[inside], labels[inside]
    t[ROWS_OUT] = len(boxes)
    if gmax is not None and len(boxes) > gmax:
        t[STATUS] = 2
        boxes, kps, labels = boxes[:gmax], kps[:gmax], labels[:gmax]
    return dict(table=t, boxes=boxes, kps=kps, labels=labels)


# ------------------------------------------------------------------ pixels
def coeffs(dst_n, scale, src, dtype):
    """cv2's float INTER_LINEAR coefficients of destination coordinates 0..dst_n-1 at coordinate scale `scale` (a double)
    -> (s0, s1, w0, w1).  float32: f = (float)((d + 0.5) * scale - 0.5) and float32 weights, pipeline_oracle.linear_coeffs;
    float64: the same formulas without the roundings."""
    d = np.arange(dst_n, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(dtype)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(dtype)).astype(dtype)
    lo = s < 0
    f[lo], s[lo] = 0, 0
    hi = s >= src - 1
    f[hi], s[hi] = 0, src - 1
    return s, np.minimum(s + 1, src - 1), (dtype(1) - f).astype(dtype), f


def resize(img, w, h, dtype=np.float32):
    """img [H, W, c] -> [h, w, c] in `dtype`: horizontal pass, then vertical pass, every product and sum rounded once."""
    H, W = img.shape[:2]
    sx, sx1, a0, a1 = coeffs(w, 1.0 / (float(w) / float(W)), W, dtype)
    sy, sy1, b0, b1 = coeffs(h, 1.0 / (float(h) / float(H)), H, dtype)
    img = np.asarray(img).astype(dtype)
    rows = (img[:, sx] * a0[None, :, None] + img[:, sx1] * a1[None, :, None]).astype(dtype)
    return (rows[sy] * b0[:, None, None] + rows[sy1] * b1[:, None, None]).astype(dtype)


def imresize(img, size, **kw):
    """The stand-in for mmcv.imresize(img, (w, h)) handed to the reference class: `resize` in float32."""
    assert not kw
    return resize(img, int(size[0]), int(size[1]), np.float32)


def partner_value(t, img, D, pad_val, dtype):
    """b of every destination pixel of an applied image, before its truncation -> (b [T, T, 3] in `dtype`, zero bool
    [T, T]: the pixels of padded_img's zero padding, where b is 0 by definition).  `img` the raw partner, uint8 HWC."""
    T, J, rw, rh = (int(t[k]) for k in (EDGE, J_, RW, RH))
    canvas = np.full((D, D, 3), pad_val, dtype)
    canvas[:rh, :rw] = resize(img, rw, rh, dtype)
    out = resize(canvas, J, J, dtype)
    if t[FLIP]:
        out = out[:, ::-1]
    P_ = max(J, T)
    padded = np.zeros((P_, P_, 3), dtype)
    padded[:J, :J] = out
    zero = np.ones((P_, P_), bool)
    zero[:J, :J] = False
    y, x = int(t[YOFF]), int(t[XOFF])
    return padded[y:y + T, x:x + T], zero[y:y + T, x:x + T]


def blend(a, k):
    """trunc(sat(0.5f * a + 0.5f * k)) in float32: a [..] float32, k integer-valued."""
    v = np.float32(0.5) * np.asarray(a, np.float32) + np.float32(0.5) * np.asarray(k, np.float32)
    return np.trunc(np.clip(v, np.float32(0), np.float32(255)))


def admissible(a, b64, zero, bar):
    """The admissible outputs of every pixel: {blend(a, k) : trunc(b64 - bar) <= k <= trunc(b64 + bar)} -> (lo, hi)
    float32, every integer between them attained (blend is monotonic in k and moves by at most 1 per k).  Where `zero`,
    k = 0.  a [T, T, 3] HWC."""
    klo = np.where(zero[..., None], 0.0, np.trunc(np.maximum(b64 - bar, 0.0)))
    khi = np.where(zero[..., None], 0.0, np.trunc(np.maximum(b64 + bar, 0.0)))
    return blend(a, klo), blend(a, khi)


# ------------------------------------------------------------------ the fixture's cases (tests/golden/mixup_cases.npz)
SEED, ITERATION, N_IMAGES, EDGES, GMAX = 5, 1, 6, (32, 64), 8
MARGIN = 1e-3       # pixels: every decision of a fixture case is clear of its thresholds by this much
AMBIGUOUS_CAP = 0.10
STORE_HW = ((58, 62), (62, 58), (24, 28), (44, 42), (30, 26), (54, 60))         # (h, w); images 2 and 4 have no boxes
# D: the img_scale of the case; None: D = T (with ratio_range (1, 1): J == T, no offset is drawn)
CONFIGS = {
    'defaults': dict(D=48),
    'same': dict(D=None, ratio_range=(1.0, 1.0)),
    'small': dict(D=32, ratio_range=(0.5, 0.9), flip_ratio=0.3),
    'large': dict(D=64, ratio_range=(1.1, 1.5), flip_ratio=0.7),
    'one_iter': dict(D=48, max_iters=1),
    'filter': dict(D=48, skip_filter=False, min_bbox_size=3),
    'filter_aspect': dict(D=64, skip_filter=False, min_bbox_size=0.5, min_area_ratio=0.02, max_aspect_ratio=3),
    'filter_area': dict(D=64, skip_filter=False, min_bbox_size=0.5, min_area_ratio=0.7, max_aspect_ratio=100,
                        ratio_range=(1.0, 1.5)),
    'unclipped': dict(D=64, bbox_clip_border=False, ratio_range=(0.8, 1.5)),
}


def case_cfg(name, T):
    """-> (D, the MixUp keywords of the case without D)."""
    c = dict(CONFIGS[name])
    D = c.pop('D')
    return (T if D is None else D), c


def store():
    """The store of six uint8 images with their raw GT -> dict(hw, imgs, boxes, kps): noise images (few values of b sit
    near an integer), at most 8 rows each, boxes of every kind: large, small, thin, at the border."""
    rng = np.random.default_rng(77)
    imgs, boxes, kps = [], [], []
    for i, (h, w) in enumerate(STORE_HW):
        base = rng.integers(0, 256, (h // 4 + 2, w // 4 + 2, 3)).astype(np.float64)
        imgs.append(np.clip(resize(base, w, h, np.float64) + rng.uniform(-6, 6, (h, w, 3)), 0, 255).astype(np.uint8))
        if i in (2, 4):
            b = np.zeros((0, 4))
        else:
            g = (8, 5, 0, 7, 0, 6)[i]
            c = rng.uniform(0.0, 0.75, (g, 2)) * (w, h)
            wh = rng.uniform(0.08, 0.5, (g, 2)) * (w, h)
            b = np.concatenate([c, np.minimum(c + wh, (w, h))], 1)
            b[0] = [0.0, 0.1 * h, 0.3 * w, 0.6 * h]                             # at the left border
            b[1] = [0.55 * w, 0.5 * h, float(w), float(h)]                      # in the bottom-right corner
            b[2] = [0.4 * w, 0.2 * h, 0.4 * w + 1.6, 0.7 * h]                   # thin
            b[3] = [0.6 * w, 0.15 * h, 0.6 * w + 1.2, 0.15 * h + 1.1]           # tiny
        b = b.astype(np.float32)
        t = rng.uniform(0.0, 1.0, (len(b), 5, 2))
        k = np.zeros((len(b), 5, 3), np.float32)
        k[:, :, 0] = b[:, None, 0] + t[:, :, 0] * (b[:, None, 2] - b[:, None, 0])
        k[:, :, 1] = b[:, None, 1] + t[:, :, 1] * (b[:, None, 3] - b[:, None, 1])
        k[:, :, 2] = np.array([1.0, 0.0, -1.0])[np.arange(len(b)) % 3][:, None]
        k[k[:, :, 2] < 0, :2] = -1.0
        boxes.append(b)
        kps.append(k)
    return dict(hw=np.array(STORE_HW, np.int32), imgs=imgs, boxes=boxes, kps=kps)


def own_inputs(T):
    """The images' own GT before MixUp -> (boxes float32 [N_IMAGES, GMAX, 4], kps, counts): rows inside [0, T]; image 3
    has none."""
    rng = np.random.default_rng(2000 + T)
    boxes, kps = np.zeros((N_IMAGES, GMAX, 4), np.float32), np.zeros((N_IMAGES, GMAX, 5, 3), np.float32)
    counts = np.array([3, 8, 1, 0, 5, 2], np.int32)
    for i, g in enumerate(counts):
        c = rng.uniform(0.0, 0.7 * T, (g, 2))
        b = np.concatenate([c, np.minimum(c + rng.uniform(2.0, 0.4 * T, (g, 2)), T)], 1)
        boxes[i, :g] = b
        t = rng.uniform(0.0, 1.0, (g, 5, 2))
        kps[i, :g, :, 0] = b[:, None, 0] + t[:, :, 0] * (b[:, None, 2] - b[:, None, 0])
        kps[i, :g, :, 1] = b[:, None, 1] + t[:, :, 1] * (b[:, None, 3] - b[:, None, 1])
        kps[i, :g, :, 2] = 1.0
    return boxes, kps, counts


def pattern(n, edge):
    """The images before MixUp, float32 [n, 3, edge, edge]: a sawtooth, every value k + 0.25 within [1, 200]."""
    i, c, y, x = np.ogrid[:n, :3, :edge, :edge]
    return ((i * 13 + c * 29 + y * 7 + x * 3) % 199 + 1.25).astype(np.float32)
