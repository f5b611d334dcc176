"""TEST INFRASTRUCTURE ONLY -- numpy restatement of mmcv.ops.soft_nms for one class and offset 0.

PARITY UNPINNED: mmcv is a compiled package that is neither installed nor part of the reference tree; the semantics are
restated from mmcv 1.3.17's `softnms_cpu` (as oracle/detect_oracle.py restates the greedy NMS).  Two forms:

  soft_nms_swap   the literal sequential form: arrays, a strict-'<' scan for the maximum of [i, n), a swap into place i,
                  the decay of (i, n) with removed entries swapped to the end;
  soft_nms_live   the form the kernel implements (csrc/detect.hip: soft_rounds): a live set, per round the arg-max of the
                  current scores (ties: lower index), a decay of every other live candidate, death below min_score.

Both are parameterised by dtype.  With dtype = float32 every operation is a single fp32 rounding in the order of
detect.hip's nms_iou and the kernel's `score *= weight`, so the naive and linear methods are bit-comparable with the
device; the gaussian weight goes through exp and is compared to a tolerance against the float64 run.

`Guard` measures, on a float64 run, how far every decision of the run is from its boundary -- a comparison of two
implementations is only meaningful where the smallest margin exceeds what their arithmetic can differ by:
  (a) gap_rel     relative gap between the two largest live scores at every selection,
  (b) iou_margin  |IoU - iou_threshold| over every evaluated pair (naive and linear only),
  (c) min_margin  |score - min_score| / min_score of every updated score.
"""
import numpy as np

METHODS = {'naive': 0, 'linear': 1, 'gaussian': 2}
U32 = 2.0 ** -24          # unit roundoff of fp32


class Guard:
    def __init__(self):
        self.gap_rel = self.iou_margin = self.min_margin = np.inf

    def ok(self, least=1e-4):
        return self.gap_rel >= least and self.iou_margin >= least and self.min_margin >= least

    def __repr__(self):
        return f'Guard(gap_rel={self.gap_rel:.3g}, iou_margin={self.iou_margin:.3g}, min_margin={self.min_margin:.3g})'


def iou_one_to_many(a, b):
    """a [4], b [K,4] (one dtype) -> IoU [K]: inter / (area_a + area_b - inter), the operation order of nms_iou()."""
    left, right = np.maximum(a[0], b[:, 0]), np.minimum(a[2], b[:, 2])
    top, bottom = np.maximum(a[1], b[:, 1]), np.minimum(a[3], b[:, 3])
    zero = a.dtype.type(0)
    width, height = np.maximum(right - left, zero), np.maximum(bottom - top, zero)
    inter = width * height
    sa = (a[2] - a[0]) * (a[3] - a[1])
    sb = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(invalid='ignore', divide='ignore'):
        return inter / (sa + sb - inter)


def weights(ovr, iou_thr, sigma, method):
    """The decay factor of every evaluated pair, in ovr's dtype."""
    t = ovr.dtype.type
    one = np.ones_like(ovr)
    if method == 'naive':
        return np.where(ovr >= t(iou_thr), t(0), one)
    if method == 'linear':
        return np.where(ovr >= t(iou_thr), one - ovr, one)
    if method == 'gaussian':
        return np.exp(-(ovr * ovr) / t(sigma))
    raise ValueError(method)


def soft_nms_live(boxes, scores, iou_thr=0.3, sigma=0.5, min_score=1e-3, method='linear', score_thr=-np.inf,
                  max_out=None, dtype=np.float32, guard=None):
    """-> (keep [n] int64 indices into the input, scores [n] dtype): the live-set form.  Candidates: score >= score_thr
    (fp32 inputs compared as given, before any decay)."""
    boxes32, scores32 = np.asarray(boxes, np.float32), np.asarray(scores, np.float32)
    b, s = boxes32.astype(dtype), scores32.astype(dtype)
    live = scores32 >= np.float32(score_thr)
    max_out = len(s) if max_out is None or max_out < 0 else max_out
    keep, out = [], []
    while live.any() and len(keep) < max_out:
        cur = np.where(live, s, -np.inf)
        m = int(np.argmax(cur))                     # first maximum: the lower index wins a tie
        if guard is not None and live.sum() > 1:
            second = np.partition(cur, -2)[-2]
            guard.gap_rel = min(guard.gap_rel, float((cur[m] - second) / abs(cur[m])))
        keep.append(m)
        out.append(s[m])
        live[m] = False
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        ovr = iou_one_to_many(b[m], b[idx])
        s[idx] = s[idx] * weights(ovr, iou_thr, sigma, method)
        if guard is not None:
            if method != 'gaussian':
                guard.iou_margin = min(guard.iou_margin, float(np.nanmin(np.abs(ovr - iou_thr))))
            guard.min_margin = min(guard.min_margin, float(np.min(np.abs(s[idx] - min_score)) / min_score))
        live[idx[s[idx] < dtype(min_score)]] = False
    return np.asarray(keep, np.int64), np.asarray(out, dtype)


def soft_nms_swap(boxes, scores, iou_thr=0.3, sigma=0.5, min_score=1e-3, method='linear', score_thr=-np.inf,
                  dtype=np.float32):
    """-> (keep, scores): the literal sequential form of softnms_cpu, scalar by scalar."""
    boxes32, scores32 = np.asarray(boxes, np.float32), np.asarray(scores, np.float32)
    cand = np.nonzero(scores32 >= np.float32(score_thr))[0]
    b = boxes32[cand].astype(dtype)
    x1, y1, x2, y2 = (b[:, c].copy() for c in range(4))
    sc = scores32[cand].astype(dtype)
    ind = cand.astype(np.int64).copy()
    t, zero, one = dtype, dtype(0), dtype(1)
    n, i = len(sc), 0
    while i < n:
        m = i
        for pos in range(i + 1, n):                 # strict '<': the first position holding the maximum
            if sc[m] < sc[pos]:
                m = pos
        for arr in (x1, y1, x2, y2, sc, ind):
            arr[i], arr[m] = arr[m], arr[i]
        iarea = (x2[i] - x1[i]) * (y2[i] - y1[i])
        pos = i + 1
        while pos < n:
            w = max(min(x2[i], x2[pos]) - max(x1[i], x1[pos]), zero)
            h = max(min(y2[i], y2[pos]) - max(y1[i], y1[pos]), zero)
            inter = w * h
            with np.errstate(invalid='ignore', divide='ignore'):
                ovr = inter / (iarea + (x2[pos] - x1[pos]) * (y2[pos] - y1[pos]) - inter)
            weight = one
            if method == 'naive':
                if ovr >= t(iou_thr):
                    weight = zero
            elif method == 'linear':
                if ovr >= t(iou_thr):
                    weight = one - ovr
            elif method == 'gaussian':
                weight = np.exp(-(ovr * ovr) / t(sigma))
            else:
                raise ValueError(method)
            sc[pos] = sc[pos] * weight
            if sc[pos] < t(min_score):
                for arr in (x1, y1, x2, y2, sc, ind):
                    arr[pos], arr[n - 1] = arr[n - 1], arr[pos]
                n -= 1
                pos -= 1
            pos += 1
        i += 1
    return ind[:n].copy(), sc[:n].copy()


def cluster_fixture(seed, K=96, centres=6):
    """K boxes in `centres` overlapping clusters with scores in (0.02, 1): (boxes [K,4], scores [K]) fp32.  Checked for
    seeds 0-5 at iou_threshold 0.3, sigma 0.5: every margin of Guard >= 2.6e-4 for all three methods and min_score
    1e-3 / 0.05 (the tests assert >= 1e-4 before they compare anything)."""
    r = np.random.RandomState(seed)
    c = r.uniform(40, 280, (centres, 2))
    sz = r.uniform(16, 64, centres)
    k = r.randint(0, centres, K)
    ctr = c[k] + r.normal(0, 0.12, (K, 2)) * sz[k, None]
    wh = sz[k, None] * np.exp(r.normal(0, 0.15, (K, 2)))
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
    scores = r.uniform(0.02, 1, K).astype(np.float32)
    return boxes, scores


def grid_plus_cluster(rows, cols, seed, x0=1000.0):
    """rows x cols disjoint 6-pixel boxes on an 8-pixel pitch (far from the clusters: IoU 0 with everything else), then the
    cluster fixture appended.  Grid scores are a shuffled geometric ladder from 0.3 down to 0.02: neighbouring scores are a
    fixed relative step apart (1.7e-4 at 128 x 128), and the clusters' best boxes come first, so that the first rounds
    decay their neighbours before the grid fills the remaining rows."""
    r = np.random.RandomState(1000 + seed)
    n = rows * cols
    yy, xx = np.divmod(np.arange(n), cols)
    gx, gy = x0 + 8.0 * xx, 8.0 * yy
    grid = np.stack([gx, gy, gx + 6.0, gy + 6.0], 1).astype(np.float32)
    ladder = 0.3 * (0.02 / 0.3) ** (np.arange(n) / max(n - 1, 1))
    gs = ladder[r.permutation(n)].astype(np.float32)
    cb, cs = cluster_fixture(seed)
    return np.concatenate([grid, cb]), np.concatenate([gs, cs])
