"""TEST INFRASTRUCTURE ONLY -- pure-Python restatement of CutOut as the device pipeline runs it
(mmdet/datasets/pipelines/transforms.py:2143-2214 of the reference; csrc/augment.hip aug_cutout_kernel;
include/yunet_hip.h YUNET_CUTOUT_*).  Nothing in the product imports this.

Randomness.  The reference draws from numpy's global stream.  Here the draws come from a SUB-STREAM of the
counter-based generator of oracle/pipeline_oracle.py: key mix32(stream_key(seed, iteration, image) ^ SALT), counter
from 0 (the construction of photometric_ref.PhotoStream), one u32 per numpy.random.randint(lo, hi) =
lo + ((u32 * (hi - lo)) >> 32).  `holes` follows CutOut.__call__'s call order and writes the per-image table row of
yunet_aug_cutout; `fill` stores the table's holes into a planar image.
"""
import numpy as np

import pipeline_oracle as P

SALT = 0x4355544F                       # YUNET_CUTOUT_SALT ("CUTO")
MAX_HOLES = 16                          # YUNET_CUTOUT_MAX_HOLES
WORDS = 2 + 4 * MAX_HOLES               # YUNET_CUTOUT_WORDS


def cutout_key(seed, iteration, image):
    return P.mix32(P.stream_key(seed, iteration, image) ^ SALT)


class CutoutStream(P.Stream):
    """The CutOut draws of one image behind numpy's randint; `log` records (low, high, value) of every call."""

    def __init__(self, seed, iteration, image):
        super().__init__(seed, iteration, image)
        self.key = cutout_key(seed, iteration, image)
        self.log = []

    def randint(self, low, high=None, size=None):
        assert size is None
        if high is None:
            low, high = 0, low
        v = super().randint(int(low), int(high))
        self.log.append((int(low), int(high), v))
        return v


def normalise(cfg):
    """A CutOut constructor dict -> (n_lo, n_hi, with_ratio, candidates, fill[3]) the way the reference's __init__ reads
    it (an int n_holes is the interval (n, n); a candidate that is not a list is one candidate)."""
    n = cfg['n_holes']
    n_lo, n_hi = n if isinstance(n, tuple) else (n, n)
    with_ratio = cfg.get('cutout_ratio') is not None
    cands = cfg['cutout_ratio'] if with_ratio else cfg['cutout_shape']
    if not isinstance(cands, list):
        cands = [cands]
    fill = cfg.get('fill_in', (0, 0, 0))
    fill = [fill] * 3 if np.isscalar(fill) else list(fill)
    return n_lo, n_hi, with_ratio, cands, np.array(fill, np.float32)


def holes(seed, iteration, image, w, h, cfg):
    """CutOut.__call__'s draws for one w x h image -> the table row int32 [WORDS]."""
    n_lo, n_hi, with_ratio, cands, _ = normalise(cfg)
    st = CutoutStream(seed, iteration, image)
    row = np.zeros(WORDS, np.int32)
    n = st.randint(n_lo, n_hi + 1)
    for j in range(n):
        x1 = st.randint(0, w)
        y1 = st.randint(0, h)
        index = st.randint(0, len(cands))
        if with_ratio:
            cw, ch = int(cands[index][0] * w), int(cands[index][1] * h)
        else:
            cw, ch = cands[index]
        row[2 + 4 * j:6 + 4 * j] = [x1, y1, min(max(x1 + cw, 0), w), min(max(y1 + ch, 0), h)]
    row[0], row[1] = n, st.ctr
    return row


def fill(img, row, fill_in):
    """img float32 [3, H, W] (a copy is returned) with the holes of table row `row` stored: img[c, y1:y2, x1:x2] =
    fill_in[c]."""
    out = img.copy()
    for j in range(int(row[0])):
        x1, y1, x2, y2 = (int(v) for v in row[2 + 4 * j:6 + 4 * j])
        out[:, y1:y2, x1:x2] = np.asarray(fill_in, np.float32).reshape(3, 1, 1)
    return out


def mask(row, edge):
    """bool [edge, edge]: the pixels inside any hole of the table row."""
    m = np.zeros((edge, edge), bool)
    for j in range(int(row[0])):
        x1, y1, x2, y2 = (int(v) for v in row[2 + 4 * j:6 + 4 * j])
        m[y1:y2, x1:x2] = True
    return m


# ------------------------------------------------------------------ the fixture's cases (tests/golden/cutout.npz)
SEED, ITERATION, N_IMAGES, EDGES = 5, 3, 8, (32, 64, 96)
CONFIGS = {
    'fixed_shape': dict(n_holes=3, cutout_shape=(10, 7)),
    'range_shapes': dict(n_holes=(0, 4), cutout_shape=[(4, 4), (20, 9), (0, 5), (40, 40)], fill_in=114),
    'fixed_ratio': dict(n_holes=2, cutout_ratio=(0.25, 0.4), fill_in=(1.5, 127.0, 255.0)),
    'range_ratios': dict(n_holes=(0, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.2), (0.01, 0.5)], fill_in=(114, 114, 114)),
    'full_ratios': dict(n_holes=16, cutout_ratio=[(1 / 3, 0.7), (0.29, 0.57), (0.1, 0.1), (0.6, 0.05), (1.0, 0.02),
                                                  (0.15, 0.15), (0.07, 0.9), (0.5, 0.5)], fill_in=7),
}


def pattern(n, edge):
    """Input images float32 [n, 3, edge, edge]: every value is k + 0.25, so none equals a fill value of CONFIGS."""
    i, c, y, x = np.ogrid[:n, :3, :edge, :edge]
    return ((i * 11 + c * 7 + y * 3 + x * 5) % 251 + 1.25).astype(np.float32)
