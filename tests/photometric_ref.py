"""TEST INFRASTRUCTURE ONLY -- numpy restatement of PhotoMetricDistortion as the device pipeline runs it
(mmdet/datasets/pipelines/transforms.py:1211-1312 of the reference; csrc/augment.hip aug_photometric_kernel /
photo_pixel; include/yunet_hip.h YUNET_PHOTO_*).  Nothing in the product imports this.

Randomness.  The reference draws from numpy's global stream.  Here the draws come from a SUB-STREAM of the
counter-based generator of oracle/pipeline_oracle.py: key mix32(stream_key(seed, iteration, image) ^ SALT), counter
from 0 -- so the crop / flip draws of the main stream are the same whether or not, and wherever, the transform sits.
`PhotoStream` serves numpy's randint(2) / uniform(a, b) / permutation(3) from it:
  randint(2)      = u32 >> 31 (floor(u * 2));
  uniform(a, b)   = a + (b - a) * (u32 / 2^32) in double (numpy's legacy random_uniform), a Python float;
  permutation(3)  = numpy's legacy Fisher-Yates: i = 2 then 1, j = floor(u * (i + 1)), swap(arr[i], arr[j]).
`draw_table` follows PhotoMetricDistortion.__call__'s call order (conditional draws included) and writes the
per-image table of yunet_aug_photometric.

Pixels.  numpy >= 2 treats the Python float of np.random.uniform as a weak scalar on the float32 image: every
parameter is rounded to fp32 once and each image operation is one fp32 operation.  mmcv.bgr2hsv / hsv2bgr are
cv2.cvtColor on float32; cv2 is not available here, so `bgr2hsv` / `hsv2bgr` restate OpenCV's published SCALAR float
path (RGB2HSV_f / HSV2RGB_f, hrange 360).  PARITY UNPINNED against the cv2 binary (its SIMD path and compiler
contraction are not reproduced); the device kernel is bit-exact against THIS restatement, and the restatement runs
inside the unmodified reference class (tools/make_golden_photometric.py, tests/golden/photometric_*.npz).
"""
import hashlib

import numpy as np

import pipeline_oracle as P

SALT = 0x50484D44                       # YUNET_PHOTO_SALT ("PHMD")
WORDS = 16                              # YUNET_PHOTO_WORDS
(BRIGHT, DELTA, MODE, CONTRAST, ALPHA, SAT, SAT_F, HUE, HUE_D, SWAP, PERM, DRAWS) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13
DEFAULTS = dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18)
FLT_EPSILON = np.float32(np.finfo(np.float32).eps)
F32 = np.float32


def photo_key(seed, iteration, image):
    return P.mix32(P.stream_key(seed, iteration, image) ^ SALT)


class PhotoStream(P.Stream):
    """The photometric draws of one image, numpy's API; `log` records (kind, value) of every call."""

    def __init__(self, seed, iteration, image):
        super().__init__(seed, iteration, image)
        self.key = photo_key(seed, iteration, image)
        self.log = []

    def randint(self, low, high=None, size=None):
        assert size is None
        if high is None:
            low, high = 0, low
        v = super().randint(int(low), int(high))
        self.log.append((0, float(v)))
        return v

    def uniform(self, low=0.0, high=1.0, size=None):
        assert size is None
        low, high = float(low), float(high)
        v = low + (high - low) * (self.next_u32() / 4294967296.0)
        self.log.append((1, v))
        return v

    def permutation(self, x):
        assert int(x) == 3
        arr = np.arange(3)
        for i in (2, 1):
            j = P.bounded(self.next_u32(), i + 1)
            arr[i], arr[j] = arr[j], arr[i]
        self.log.append((2, float(arr[0] * 9 + arr[1] * 3 + arr[2])))
        return arr


def log_array(log):
    """A PhotoStream log as a [k, 2] float64 array (kind, value) -- the fixture format."""
    return np.array(log, np.float64).reshape(-1, 2)


def draw_table(seed, iteration, image, brightness_delta=32, contrast_range=(0.5, 1.5),
               saturation_range=(0.5, 1.5), hue_delta=18):
    """PhotoMetricDistortion.__call__'s draws for one image -> (table float32 [WORDS], PhotoStream)."""
    st = PhotoStream(seed, iteration, image)
    t = np.zeros(WORDS, np.float32)
    if st.randint(2):
        t[BRIGHT], t[DELTA] = 1, st.uniform(-brightness_delta, brightness_delta)
    mode = st.randint(2)
    t[MODE] = mode
    if mode == 1 and st.randint(2):
        t[CONTRAST], t[ALPHA] = 1, st.uniform(*contrast_range)
    if st.randint(2):
        t[SAT], t[SAT_F] = 1, st.uniform(*saturation_range)
    if st.randint(2):
        t[HUE], t[HUE_D] = 1, st.uniform(-hue_delta, hue_delta)
    if mode == 0 and st.randint(2):
        t[CONTRAST], t[ALPHA] = 1, st.uniform(*contrast_range)
    perm = np.arange(3)
    if st.randint(2):
        t[SWAP] = 1
        perm = st.permutation(3)
    t[PERM:PERM + 3] = perm
    t[DRAWS] = st.ctr
    return t, st


def combo(t):
    """Index 0..63 of (mode, brightness, contrast, saturation, hue, swap) of a table."""
    return int(t[MODE]) * 32 + int(t[BRIGHT]) * 16 + int(t[CONTRAST]) * 8 + int(t[SAT]) * 4 + int(t[HUE]) * 2 + \
        int(t[SWAP])


# ------------------------------------------------------------------ cv2.cvtColor, float32, scalar path
def bgr2hsv(img):
    """RGB2HSV_f (hrange 360): [..., 3] float32 BGR -> HSV (h degrees, s, v)."""
    img = np.asarray(img, np.float32)
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = r.copy()
    v = np.where(v < g, g, v)
    v = np.where(v < b, b, v)
    vmin = r.copy()
    vmin = np.where(vmin > g, g, vmin)
    vmin = np.where(vmin > b, b, vmin)
    diff = (v - vmin).astype(np.float32)
    s = (diff / (np.abs(v) + FLT_EPSILON)).astype(np.float32)
    d = (60.0 / (diff + FLT_EPSILON).astype(np.float64)).astype(np.float32)
    h = np.where(v == r, (g - b) * d, np.where(v == g, (b - r) * d + F32(120), (r - g) * d + F32(240)))
    h = np.where(h < 0, h + F32(360), h).astype(np.float32)
    return np.stack([h, s, v], -1).astype(np.float32)


SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def hsv2bgr(img):
    """HSV2RGB_f (hrange 360): [..., 3] float32 HSV -> BGR."""
    img = np.asarray(img, np.float32)
    h = (img[..., 0] * (F32(6) / F32(360))).astype(np.float32)
    s, v = img[..., 1], img[..., 2]
    neg = h < 0
    while (m := neg & (h < 0)).any():
        h = np.where(m, h + F32(6), h)
    while (m := ~neg & (h >= 6)).any():
        h = np.where(m, h - F32(6), h)
    fl = np.floor(h)
    sector = fl.astype(np.int64)
    h = (h - fl).astype(np.float32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, F32(0), h)
    one = F32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], -1).astype(np.float32)
    idx = SECTOR[sector]                                            # [..., 3] table entries for (b, g, r)
    out = np.take_along_axis(tab, idx, -1)
    out = np.where((s == 0)[..., None], v[..., None], out)
    return out.astype(np.float32)


def distort(img, t):
    """PhotoMetricDistortion's pixel arithmetic with the draws of table t: float32 [..., 3] BGR -> float32."""
    img = np.array(img, np.float32)
    if t[BRIGHT]:
        img += t[DELTA]
    if t[MODE] == 1 and t[CONTRAST]:
        img *= t[ALPHA]
    img = bgr2hsv(img)
    if t[SAT]:
        img[..., 1] *= t[SAT_F]
    if t[HUE]:
        img[..., 0] += t[HUE_D]
        img[..., 0][img[..., 0] > 360] -= 360
        img[..., 0][img[..., 0] < 0] += 360
    img = hsv2bgr(img)
    if t[MODE] == 0 and t[CONTRAST]:
        img *= t[ALPHA]
    if t[SWAP]:
        img = img[..., t[PERM:PERM + 3].astype(np.int64)]
    return np.ascontiguousarray(img, dtype=np.float32)


def augment_image(img_u8, boxes, kps, seed, iteration, image, S, crop_choice, position, photo=None, flip_ratio=0.5,
                  pad=128.0):
    """pipeline_oracle.augment_image with PhotoMetricDistortion at position 'pre' (on the float source, before the
    crop's pad fill) or 'post' (on the resized, flipped image).  -> its dict + 'table'."""
    t, _ = draw_table(seed, iteration, image, **(photo or {}))
    if position == 'pre':
        r = P.augment_image(distort(np.asarray(img_u8, np.float32), t), boxes, kps, seed, iteration, image, S,
                            crop_choice, flip_ratio, pad)
    elif position == 'post':
        r = P.augment_image(img_u8, boxes, kps, seed, iteration, image, S, crop_choice, flip_ratio, pad)
        r['img'] = np.ascontiguousarray(distort(r['img'].transpose(1, 2, 0), t).transpose(2, 0, 1))
    else:
        raise ValueError(position)
    r['table'] = t
    return r


def digest(img):
    """sha256 of a float32 image's bytes (C order): the fixtures pin outputs bit for bit through it."""
    return hashlib.sha256(np.ascontiguousarray(img, dtype=np.float32).tobytes()).hexdigest()


# ------------------------------------------------------------------ sources that hit the hard cases
def hard_image(k, side=32):
    """A side x side uint8 BGR image: greys (s = 0), v == r == g / v == r == b / v == g == b ties, the six sector
    boundaries (pure and half hues at several levels), hues just above 0 and just below 360 (wrap at both ends),
    extremes 0 / 255 (brightness and contrast push them out of [0, 255]); the rest random (seeded by k)."""
    rng = np.random.default_rng(1000 + k)
    px = []
    for v in (0, 1, 2, 64, 127, 128, 200, 254, 255):
        px.append((v, v, v))
    for hi in (255, 200, 128, 17, 1):
        for lo in (0, hi // 2, max(hi - 1, 0)):
            px += [(lo, hi, hi), (hi, lo, hi), (hi, hi, lo)]                  # ties of the max (b, g, r order)
            px += [(lo, lo, hi), (lo, hi, lo), (hi, lo, lo)]                  # ties of the min
            px += [(hi, lo, hi), (lo, hi, hi), (hi, hi, lo)]
    for hi in (255, 180, 90):
        px += [(0, 1, hi), (1, 0, hi), (0, 2, hi), (2, 0, hi)]                # h just above 0 / just below 360
        px += [(hi, 1, 0), (hi, 0, 1), (1, hi, 0), (0, hi, 1)]                # around 120 / 240
        px += [(hi // 2, 0, hi), (0, hi // 2, hi), (0, hi, hi // 2), (hi, hi // 2, 0)]
    px = np.array(px, np.uint8)
    img = rng.integers(0, 256, (side * side, 3), dtype=np.uint8)
    n = min(len(px), side * side)
    img[:n] = np.roll(px, k, axis=0)[:n]
    return img.reshape(side, side, 3)


def hard_case(k, side=32):
    """(image, boxes, kps) of hard_image(k) with one centred face, so that crop_choice=[1.0] keeps the whole square
    image: the resize is then the identity and the output pixels are the distorted source pixels themselves."""
    img = hard_image(k, side)
    c = side / 2
    boxes = np.array([[c - 4, c - 4, c + 4, c + 4]], np.float32)
    kps = np.full((1, 5, 3), -1.0, np.float32)
    kps[0, :, :2] = np.array([[c - 2, c - 2], [c + 2, c - 2], [c, c], [c - 2, c + 2], [c + 2, c + 2]], np.float32)
    kps[0, :, 2] = 1.0
    return img, boxes, kps
