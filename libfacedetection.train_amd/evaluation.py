"""WIDER-Face average precision (easy / medium / hard) of a prediction set.

Reference: mmdet/core/evaluation/widerface.py:152-347 (`norm_score`, `image_eval`,
`img_pr_info`, `dataset_pr_info`, `voc_ap`, `wider_evaluation`), called by
tools/test_widerface.py:177 as ``wider_evaluation(results, gt_path, 0.5)``.

Same inputs and the same float64 arithmetic, organised per image as array operations instead
of the reference's per-prediction Python loop over a multiprocessing pool:

* the IoU of every (prediction, GT) pair is one matrix (the "+1" pixel convention of the
  protocol: w = x2 - x1 + 1);
* the greedy matching is sequential only through "has this kept GT been hit before", which
  is a first-occurrence mask + cumulative sum;
* the 1000-threshold precision / recall counters of an image come from one boolean
  [threshold, prediction] matrix.

`pred` is {event: {image name: float array [n, 5] = x, y, w, h, score}} (rows in descending
score, as get_bboxes delivers them); `gt_path` holds the four protocol files
wider_{face,easy,medium,hard}_val.mat.

Both protocols have an integer stage (matching, first hits, prefix sums, counting) and a short floating-point
tail (precision / recall / area).  The integer stage is `wider_pr_counts` / `tpfp_default`; the default runs it on the
host in numpy, `device=<a CUDA device>` runs it in csrc/score.hip (kernels.score_wider / kernels.score_map_tpfp) on
the packed set and reads the counters back -- the same integers, so the same APs.  The tail stays on the host; for the
mAP, `rank='device'` also ranks the detections and builds the precision curve there (curve_device).
"""
import os

import numpy as np

THRESH_NUM = 1000


# ------------------------------------------------------------------------------- ground truth
def load_wider_gt(gt_dir):
    """-> list of events: dict(name, images=[dict(name, boxes [g,4] xywh float64,
    keep={'easy'|'medium'|'hard': 1-based index array})])."""
    from scipy.io import loadmat
    face = loadmat(os.path.join(gt_dir, 'wider_face_val.mat'))
    subsets = {k: loadmat(os.path.join(gt_dir, f'wider_{k}_val.mat'))['gt_list']
               for k in ('easy', 'medium', 'hard')}
    events = []
    for i in range(len(face['event_list'])):
        ev = dict(name=str(face['event_list'][i][0][0]), images=[])
        files, boxes = face['file_list'][i][0], face['face_bbx_list'][i][0]
        for j in range(len(files)):
            keep = {k: np.asarray(subsets[k][i][0][j][0]).reshape(-1).astype(np.int64) for k in subsets}
            ev['images'].append(dict(name=str(files[j][0][0]),
                                     boxes=np.asarray(boxes[j][0], dtype=np.float64).reshape(-1, 4),
                                     keep=keep))
        events.append(ev)
    return events


# --------------------------------------------------------------------------------- predictions
def read_predictions(pred_dir):
    """The per-image text files tools/test_widerface.py --save-preds writes
    (<event>/<image>.txt: name, count, then `x y w h score` rows) -> the `pred` dict."""
    pred = {}
    for event in sorted(os.listdir(pred_dir)):
        edir = os.path.join(pred_dir, event)
        if not os.path.isdir(edir):
            continue
        cur = {}
        for fn in sorted(os.listdir(edir)):
            with open(os.path.join(edir, fn)) as f:
                lines = f.read().splitlines()
            name = lines[0].split('/')[-1]
            rows = [[float(v) for v in ln.split(' ')] for ln in lines[2:] if ln.strip()]
            cur[name[:-4] if name.endswith('.jpg') else name] = \
                np.asarray(rows, dtype=np.float64).reshape(-1, 5)
        pred[event] = cur
    return pred


def write_predictions(pred_dir, event, image_name, boxes_xyxy_score):
    """One image in the protocol's text format (tools/test_widerface.py:150-165)."""
    os.makedirs(os.path.join(pred_dir, event), exist_ok=True)
    b = np.asarray(boxes_xyxy_score, dtype=np.float64).reshape(-1, 5)
    with open(os.path.join(pred_dir, event, image_name + '.txt'), 'w') as f:
        f.write(f'{event}/{image_name}.jpg\n{b.shape[0]}\n')
        for r in b:
            f.write('%.5f %.5f %.5f %.5f %g\n' % (r[0], r[1], r[2] - r[0], r[3] - r[1], r[4]))


def collect_wider_results(dets, dataset, pred_dir=None):
    """Per-image results of single_gpu_test ([[dets [n, 5]]] in dataset order) -> the `pred` dict of wider_evaluation
    ({event: {image stem: x y w h score}}); with pred_dir also the protocol's text files (write_predictions)."""
    pred = {}
    for i, res in enumerate(dets):
        name = dataset.data_infos[i]['filename']
        res = res[0] if isinstance(res, (list, tuple)) else res
        event, fn = name.split('/')[-2], name.split('/')[-1]
        stem = fn[:-4] if fn.endswith('.jpg') else os.path.splitext(fn)[0]
        xywh = np.array(res, copy=True)
        xywh[:, 2] -= xywh[:, 0]
        xywh[:, 3] -= xywh[:, 1]
        pred.setdefault(event, {})[stem] = xywh.astype(np.float64)
        if pred_dir is not None:
            write_predictions(pred_dir, event, stem, res)
    return pred


def write_aps(out_dir, aps):
    """The `aps` file of tools/test_widerface.py: easy,medium,hard on one line."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'aps'), 'w') as f:
        f.write('%f,%f,%f\n' % (aps[0], aps[1], aps[2]))


def norm_score(pred):
    """Min-max normalisation of every score over the WHOLE prediction set, in place
    (widerface.py:152-174)."""
    lo, hi = 2.0, -1.0
    for ev in pred.values():
        for v in ev.values():
            if len(v):
                lo, hi = min(lo, float(np.min(v[:, -1]))), max(hi, float(np.max(v[:, -1])))
    return _apply_norm(pred, lo, hi)


def _apply_norm(pred, lo, hi):
    diff = hi - lo
    for ev in pred.values():
        for v in ev.values():
            if len(v):
                v[:, -1] = (v[:, -1] - lo).astype(np.float64) / diff
    return pred


# --------------------------------------------------------------------------------- one image
def pairwise_iou_xywh(pred, gt):
    """[n_pred, n_gt] IoU with the protocol's inclusive-pixel convention (widerface.py:39-52)."""
    p = np.asarray(pred, dtype=np.float64)
    g = np.asarray(gt, dtype=np.float64)
    px2, py2 = p[:, 0] + p[:, 2], p[:, 1] + p[:, 3]
    gx2, gy2 = g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]
    w = np.minimum(gx2[None, :], px2[:, None]) - np.maximum(g[None, :, 0], p[:, None, 0]) + 1
    h = np.minimum(gy2[None, :], py2[:, None]) - np.maximum(g[None, :, 1], p[:, None, 1]) + 1
    inter = w * h
    ga = (gx2 - g[:, 0] + 1) * (gy2 - g[:, 1] + 1)
    pa = (px2 - p[:, 0] + 1) * (py2 - p[:, 1] + 1)
    o = inter / (ga[None, :] + pa[:, None] - inter)
    o[(w <= 0) | (h <= 0)] = 0
    return o


def image_eval(pred, gt, keep_flag, iou_thresh):
    """Greedy matching of one image (widerface.py:177-215).

    keep_flag[g] = 1 for the GTs of the current difficulty subset.  Returns
    pred_recall[h] = subset GTs recalled by predictions 0..h, and proposal[h] = -1 for
    predictions whose best GT lies outside the subset (not counted as false positives), else 1."""
    n = pred.shape[0]
    iou = pairwise_iou_xywh(pred[:, :4], gt)
    best = iou.argmax(axis=1)
    hit = iou[np.arange(n), best] >= iou_thresh
    in_subset = keep_flag[best] == 1
    proposal = np.where(hit & ~in_subset, -1.0, 1.0)
    counted = hit & in_subset
    first = np.zeros(n, dtype=bool)
    if counted.any():
        idx = np.nonzero(counted)[0]
        _, first_pos = np.unique(best[idx], return_index=True)     # first prediction per GT
        first[idx[first_pos]] = True
    return np.cumsum(first).astype(np.float64), proposal


def img_pr_info(scores, proposal, pred_recall, thresh_num=THRESH_NUM):
    """[thresh_num, 2] = (#counted predictions, #recalled GTs) at score thresholds
    1 - (t+1)/thresh_num (widerface.py:218-239): taken at the LAST prediction whose score
    passes the threshold."""
    thresh = np.array([1 - (t + 1) / thresh_num for t in range(thresh_num)])
    ok = scores[None, :] >= thresh[:, None]
    any_ok = ok.any(axis=1)
    last = scores.shape[0] - 1 - np.argmax(ok[:, ::-1], axis=1)
    cum_prop = np.cumsum(proposal == 1).astype(np.float64)
    out = np.zeros((thresh_num, 2))
    out[any_ok, 0] = cum_prop[last[any_ok]]
    out[any_ok, 1] = pred_recall[last[any_ok]]
    return out


def voc_ap(rec, prec):
    """Area under the precision envelope (widerface.py:250-268)."""
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


# ----------------------------------------------------------------------------------- dataset
SUBSETS = ('easy', 'medium', 'hard')


def _score_device(device):
    """The torch device of the device scorer; anything but a usable GPU raises (no silent host path)."""
    import torch
    dev = torch.device(device)
    if dev.type != 'cuda' or not torch.cuda.is_available():
        raise RuntimeError(f'scoring on device {device!r} needs a GPU: HIP kernels only, no CPU fallback')
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def _upload(dev, arrays):
    """Host arrays -> device tensors of the same dtypes and shapes through ONE copy (8-byte aligned sections of one
    byte buffer)."""
    import torch
    arrays = [np.ascontiguousarray(a) for a in arrays]
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 7) // 8 * 8
    buf = np.zeros(max(total, 8), dtype=np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    d = torch.from_numpy(buf).to(dev)
    return [d[o:o + a.nbytes].view(getattr(torch, a.dtype.name)).view(a.shape) for a, o in zip(arrays, offs)]


def pack_wider(pred, events):
    """The packed form the device scorer takes: (pred [P,5] fp64, pred_off int64 [I+1], gt [G,4] fp64, gt_off int64
    [I+1], gt_bits uint8 [G], count_face int64 [3]), images in protocol order.  Predictions of images no event lists
    follow as images without ground truths: they take part in the score range, as in norm_score, and in nothing else."""
    rows, boxes, bits, pn, gn, used = [], [], [], [], [], set()
    count_face = np.zeros(3, dtype=np.int64)

    def rows_of(info, where):
        a = np.asarray(info)
        if len(a) == 0:
            return np.zeros((0, 5))
        if a.dtype != np.float64 or a.ndim != 2 or a.shape[1] != 5:
            raise TypeError(f'device scorer: predictions of {where} are {a.dtype} {a.shape}; it takes float64 [n, 5] '
                            '(what collect_wider_results and read_predictions deliver)')
        return a

    for ev in events:
        plist = pred[ev['name']]
        for im in ev['images']:
            a = rows_of(plist[im['name']], im['name'])
            used.add((ev['name'], im['name']))
            g = np.asarray(im['boxes'], dtype=np.float64).reshape(-1, 4)
            b = np.zeros(g.shape[0], dtype=np.uint8)
            for s, setting in enumerate(SUBSETS):
                keep = im['keep'][setting]
                count_face[s] += len(keep)
                if len(keep):
                    b[keep - 1] |= np.uint8(1 << s)
            rows.append(a)
            boxes.append(g)
            bits.append(b)
            pn.append(len(a))
            gn.append(len(g))
    for en, plist in pred.items():
        for name, info in plist.items():
            if (en, name) not in used and len(info):
                rows.append(rows_of(info, name))
                pn.append(len(info))
                gn.append(0)
    cat = lambda parts, width, dt: np.concatenate(parts).astype(dt, copy=False) if parts else np.zeros((0, width), dt)
    off = lambda n: np.concatenate([[0], np.cumsum(np.asarray(n, dtype=np.int64))]).astype(np.int64)
    return (cat(rows, 5, np.float64), off(pn), cat(boxes, 4, np.float64), off(gn),
            np.concatenate(bits) if bits else np.zeros(0, np.uint8), count_face)


def _thresholds(thresh_num=THRESH_NUM):
    return np.array([1 - (t + 1) / thresh_num for t in range(thresh_num)])


def wider_pr_counts(pred, events, iou_thresh=0.5, device=None):
    """The integer stage of the protocol -> (counts int64 [3, 1000, 2], count_face int64 [3]): per subset (easy,
    medium, hard) and score threshold, (#counted predictions, #recalled GTs) summed over the images, and the number of
    GTs of the subset.  `pred` scores are normalised in place (norm_score).  device=None: numpy on the host; a CUDA
    device: csrc/score.hip on the packed set (one upload, the counters read back) -- the same integers."""
    events = load_wider_gt(events) if isinstance(events, (str, os.PathLike)) else events
    if device is not None:
        return _wider_pr_counts_device(pred, events, iou_thresh, _score_device(device))
    pred = norm_score(pred)
    counts = np.zeros((3, THRESH_NUM, 2), dtype=np.int64)
    count_face = np.zeros(3, dtype=np.int64)
    for s, setting in enumerate(SUBSETS):
        pr = np.zeros((THRESH_NUM, 2))
        for ev in events:
            plist = pred[ev['name']]
            for im in ev['images']:
                info = plist[im['name']]
                keep = im['keep'][setting]
                count_face[s] += len(keep)
                if len(im['boxes']) == 0 or len(info) == 0:
                    continue
                flag = np.zeros(im['boxes'].shape[0], dtype=np.int64)
                if len(keep):
                    flag[keep - 1] = 1
                info = np.asarray(info, dtype=np.float64)
                rec, prop = image_eval(info, im['boxes'], flag, iou_thresh)
                pr += img_pr_info(info[:, 4], prop, rec)
        counts[s] = pr                    # sums of 0 / 1 flags: integers far below 2^53, exact in either type
    return counts, count_face


def _wider_pr_counts_device(pred, events, iou_thresh, dev):
    import torch
    from . import kernels as K
    rows, poff, boxes, goff, bits, count_face = pack_wider(pred, events)
    with torch.cuda.device(dev):
        d = _upload(dev, [rows, poff, boxes, goff, _thresholds(), bits])
        counts, minmax = K.score_wider(d[0], d[1], d[2], d[3], d[5], d[4], iou_thresh)
        counts, minmax = counts.cpu().numpy(), minmax.cpu().numpy()
    _apply_norm(pred, float(minmax[0]), float(minmax[1]))      # the caller sees the host path's side effect
    return counts, count_face


def wider_aps_from_counts(counts, count_face, return_curves=False):
    """The floating-point tail: precision / recall per threshold and the area under the envelope, per subset."""
    aps, curves = [], []
    for s in range(3):
        pr = np.asarray(counts[s], dtype=np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            precision = pr[:, 1] / pr[:, 0]
            recall = pr[:, 1] / int(count_face[s])
        aps.append(float(voc_ap(recall, precision)))
        curves.append(np.stack([precision, recall], 1))
    return (aps, curves) if return_curves else aps


def wider_evaluation(pred, gt_path, iou_thresh=0.5, return_curves=False, device=None):
    """-> [AP_easy, AP_medium, AP_hard] (widerface.py:271-347).  `pred` scores are normalised in
    place, as in the reference.  device: where the integer stage runs (wider_pr_counts)."""
    counts, count_face = wider_pr_counts(pred, gt_path, iou_thresh, device=device)
    return wider_aps_from_counts(counts, count_face, return_curves)


# ============================================================================ mAP (EvalHook during training)
# What `EvalHook` reports while training (mmdet/apis/train.py:226-232 -> mmdet/core/evaluation/eval_hooks.py:24-66
# -> CustomDataset.evaluate, mmdet/datasets/custom.py:310-367 -> eval_map, mmdet/core/evaluation/mean_ap.py:522-686):
# VOC-style average precision of the single face class at IoU 0.5, "area" mode, ignored GT boxes neither matched
# nor counted.  Restated for one class, without the multiprocessing pool; same arithmetic and dtypes.
def bbox_overlaps_np(b1, b2, eps=1e-6):
    """mmdet/core/evaluation/bbox_overlaps.py:5-65 (mode 'iou', no legacy +1): float32 [n, k]."""
    b1, b2 = np.asarray(b1, dtype=np.float32).reshape(-1, 4), np.asarray(b2, dtype=np.float32).reshape(-1, 4)
    if b1.shape[0] * b2.shape[0] == 0:
        return np.zeros((b1.shape[0], b2.shape[0]), dtype=np.float32)
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    xs, ys = np.maximum(b1[:, None, 0], b2[None, :, 0]), np.maximum(b1[:, None, 1], b2[None, :, 1])
    xe, ye = np.minimum(b1[:, None, 2], b2[None, :, 2]), np.minimum(b1[:, None, 3], b2[None, :, 3])
    overlap = np.maximum(xe - xs, 0) * np.maximum(ye - ys, 0)
    union = np.maximum(a1[:, None] + a2[None, :] - overlap, np.float32(eps))
    return (overlap / union).astype(np.float32)


def tpfp_default(dets, gts, gts_ignore, iou_thr=0.5):
    """mean_ap.py:168-267 without area ranges: (tp, fp) float32 [m] for the detections [m, 5] of one image.
    A detection whose best-overlapping GT is an ignored box is neither; a second hit on a covered GT is fp."""
    m = dets.shape[0]
    tp, fp = np.zeros(m, dtype=np.float32), np.zeros(m, dtype=np.float32)
    ignore = np.concatenate([np.zeros(gts.shape[0], dtype=bool), np.ones(gts_ignore.shape[0], dtype=bool)])
    allgt = np.vstack([gts.reshape(-1, 4), gts_ignore.reshape(-1, 4)])
    if allgt.shape[0] == 0:
        fp[...] = 1
        return tp, fp
    ious = bbox_overlaps_np(dets[:, :4], allgt)
    best, arg = ious.max(axis=1), ious.argmax(axis=1)
    covered = np.zeros(allgt.shape[0], dtype=bool)
    for i in np.argsort(-dets[:, -1]):
        if best[i] >= iou_thr:
            g = arg[i]
            if not ignore[g]:
                if not covered[g]:
                    covered[g] = True
                    tp[i] = 1
                else:
                    fp[i] = 1
        else:
            fp[i] = 1
    return tp, fp


def average_precision_area(recalls, precisions):
    """mean_ap.py:13-57, mode 'area' (float32 accumulator like the reference)."""
    mrec = np.hstack((np.zeros(1, recalls.dtype), recalls, np.ones(1, recalls.dtype)))
    mpre = np.hstack((np.zeros(1, recalls.dtype), precisions, np.zeros(1, recalls.dtype)))
    for i in range(mpre.shape[0] - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    ind = np.where(mrec[1:] != mrec[:-1])[0]
    return np.float32(np.sum((mrec[ind + 1] - mrec[ind]) * mpre[ind + 1]))


def tpfp_device(dets, gts, igns, iou_thr, device):
    """tpfp_default of every image in one pass of csrc/score.hip: dets / gts / igns are per-image lists of float32
    [n, 5] / [g, 4] / [k, 4] -> (tp, fp) float32 [sum n] in row order.  The visiting order of an image is the host's
    np.argsort(-score), so ties fall as they do in tpfp_default; iou_thr is compared as float32, as numpy compares a
    float32 array with a Python float."""
    import torch
    from . import kernels as K
    dev = _score_device(device)
    off = lambda n: np.concatenate([[0], np.cumsum(np.asarray(n, dtype=np.int64))]).astype(np.int64)
    alld = np.concatenate(dets) if dets else np.zeros((0, 5), np.float32)
    if alld.shape[0] == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    allg = np.concatenate([np.vstack([g, k]) for g, k in zip(gts, igns)])
    order = np.concatenate([np.argsort(-d[:, -1]) for d in dets]).astype(np.int32)
    kept = np.asarray([g.shape[0] for g in gts], dtype=np.int32)
    with torch.cuda.device(dev):
        d = _upload(dev, [off([x.shape[0] for x in dets]), off([g.shape[0] + k.shape[0] for g, k in zip(gts, igns)]),
                          alld, allg, kept, order])
        tp, fp = K.score_map_tpfp(d[2], d[0], d[3], d[1], d[4], d[5], float(np.float32(iou_thr)))
        both = torch.stack([tp, fp]).cpu().numpy()
    return both[0], both[1]


def check_rank(rank, on_device):
    """The `rank` option of eval_map_single_class / RetinaFaceDataset.evaluate / EvalHook: None, or 'device' together
    with a device scorer."""
    if rank not in (None, 'device'):
        raise ValueError(f"rank={rank!r}; None (the host ranks the detections) or 'device'")
    if rank == 'device' and not on_device:
        raise ValueError("rank='device' ranks the detections in csrc/score.hip: it needs the device scorer "
                         "(device=<a CUDA device>, EvalHook: score='device')")
    return rank


def curve_device(dets, gts, igns, iou_thr, device):
    """The whole per-detection part of eval_map_single_class in csrc/score.hip, on one upload of the packed set: the
    visiting order of every image (kernels.score_rank_images), tp / fp (kernels.score_map_tpfp), the ranking of all
    detections (kernels.score_rank_global) and the curve (kernels.score_map_curve) -> float32 [4, sum n] in ranked
    order, read back in one copy: cumulative tp, cumulative fp, precision, and the reverse running maximum of the
    precision (the envelope average_precision_area walks).  Both orders are descending score with ties in row order,
    np.argsort(-s, kind='stable'); scores are finite (no NaN, no -0.0)."""
    import torch
    from . import kernels as K
    dev = _score_device(device)
    off = lambda n: np.concatenate([[0], np.cumsum(np.asarray(n, dtype=np.int64))]).astype(np.int64)
    alld = np.concatenate(dets) if dets else np.zeros((0, 5), np.float32)
    if alld.shape[0] == 0:
        return np.zeros((4, 0), np.float32)
    if alld.shape[0] >= K.RANK_CURVE_MAX:
        raise ValueError(f"rank='device' takes fewer than {K.RANK_CURVE_MAX} detections (fp32 counts stay exact), "
                         f'got {alld.shape[0]}')
    allg = np.concatenate([np.vstack([g, k]) for g, k in zip(gts, igns)])
    kept = np.asarray([g.shape[0] for g in gts], dtype=np.int32)
    with torch.cuda.device(dev):
        d = _upload(dev, [off([x.shape[0] for x in dets]), off([g.shape[0] + k.shape[0] for g, k in zip(gts, igns)]),
                          alld, allg, kept])
        order = K.score_rank_images(d[2], d[0])
        tp, fp = K.score_map_tpfp(d[2], d[0], d[3], d[1], d[4], order, float(np.float32(iou_thr)))
        return K.score_map_curve(tp, fp, K.score_rank_global(d[2])).cpu().numpy()


def area_from_envelope(recalls, envelope):
    """average_precision_area given the envelope (max(precisions[k:]) per k) instead of the precisions: the same
    array of terms, summed by the same numpy call."""
    mrec = np.hstack((np.zeros(1, recalls.dtype), recalls, np.ones(1, recalls.dtype)))
    mpre = np.hstack((np.zeros(1, recalls.dtype), envelope, np.zeros(1, recalls.dtype)))
    ind = np.where(mrec[1:] != mrec[:-1])[0]
    return np.float32(np.sum((mrec[ind + 1] - mrec[ind]) * mpre[ind + 1]))


def eval_map_single_class(det_results, annotations, iou_thr=0.5, device=None, rank=None):
    """eval_map (mean_ap.py:522-686) for one class.  det_results: per image [[n, 5] array] (the per-class
    list of a detector's simple_test) or the [n, 5] array itself; annotations: per image dict(bboxes, labels,
    bboxes_ignore, labels_ignore) as RetinaFaceDataset.get_ann_info returns.  -> (mAP, dict(num_gts, num_dets,
    recall, precision, ap)).  device: a CUDA device takes tp / fp from the device scorer (tpfp_device) instead of
    tpfp_default; the ranking, the cumulative sums and the area stay on the host.  rank='device' (with a device) moves
    those too (curve_device): the host forms the recalls and sums the area's terms, vectorised, and nothing else.  Its
    tie rule is the stable one -- descending score, ties in concatenation order -- where the host path's default
    np.argsort is not stable beyond small arrays: on tied scores the two may order, and so score, differently."""
    assert len(det_results) == len(annotations)
    check_rank(rank, device is not None)
    dets = [np.asarray(d[0] if isinstance(d, (list, tuple)) else d, dtype=np.float32).reshape(-1, 5) for d in det_results]
    gtl = [np.asarray(ann['bboxes'], dtype=np.float32).reshape(-1, 4) for ann in annotations]
    ignl = [np.asarray(ann.get('bboxes_ignore', np.zeros((0, 4))), dtype=np.float32).reshape(-1, 4) for ann in annotations]
    num_gts = sum(g.shape[0] for g in gtl)
    eps = np.finfo(np.float32).eps
    if rank == 'device':
        tp, _, precisions, envelope = curve_device(dets, gtl, ignl, iou_thr, device)
        recalls = tp / np.maximum(np.array([num_gts]), eps)
        ap = area_from_envelope(recalls, envelope)
        res = dict(num_gts=num_gts, num_dets=int(tp.shape[0]), recall=recalls, precision=precisions, ap=ap)
        return (float(ap) if num_gts > 0 else 0.0), res
    if device is not None:
        tps, fps = [[v] for v in tpfp_device(dets, gtl, ignl, iou_thr, device)]
    else:
        tps, fps = [], []
        for d, gts, ign in zip(dets, gtl, ignl):
            t, f = tpfp_default(d, gts, ign, iou_thr)
            tps.append(t)
            fps.append(f)
    alld = np.vstack(dets) if dets else np.zeros((0, 5), dtype=np.float32)
    order = np.argsort(-alld[:, -1])
    tp = np.cumsum(np.hstack(tps)[order]) if alld.shape[0] else np.zeros(0, dtype=np.float32)
    fp = np.cumsum(np.hstack(fps)[order]) if alld.shape[0] else np.zeros(0, dtype=np.float32)
    recalls = tp / np.maximum(np.array([num_gts]), eps)      # float64, like the reference's int array / float32 eps
    precisions = tp / np.maximum(tp + fp, eps)
    ap = average_precision_area(recalls, precisions)
    res = dict(num_gts=num_gts, num_dets=int(alld.shape[0]), recall=recalls, precision=precisions, ap=ap)
    return (float(ap) if num_gts > 0 else 0.0), res


def prepare_test_image(img_bgr, scale, device, resize='cv2'):
    """The test pipeline of the shipped configs on the device (configs/yunet_n.py:57-86: MultiScaleFlipAug(
    img_scale, flip=False) -> Resize(keep_ratio=True) -> Normalize(mean 0, std 1) -> Pad(size_divisor 32)):
    uint8 [h, w, 3] -> (float32 [1, 3, H, W] on the device, img_meta).  mmcv.imrescale semantics for the size
    (factor = min(long / long_edge, short / short_edge), rounded); scale None keeps the original size.
    The image is resized while it is still uint8, as the reference does, in cv2.resize's fixed-point arithmetic
    (imresize.resize_linear_u8); resize='float' is the fp32 bilinear this function used before (A/B only)."""
    import torch
    import torch.nn.functional as F
    from . import imresize
    h, w = img_bgr.shape[:2]
    x8 = torch.from_numpy(np.ascontiguousarray(img_bgr)).to(device)
    if scale is None:
        nh, nw = h, w
        x = x8.permute(2, 0, 1)[None].float()
    else:
        nw, nh = imresize.rescale_size(w, h, scale)
        if resize == 'cv2' and x8.dtype == torch.uint8:
            x = imresize.resize_linear_u8(x8, (nw, nh)).permute(2, 0, 1)[None].float()
        else:
            x = F.interpolate(x8.permute(2, 0, 1)[None].float(), size=(nh, nw), mode='bilinear', align_corners=False)
    ph = max(nh, 0 if scale is None else scale[0] if nh <= scale[0] else nh)
    pw = max(nw, 0 if scale is None else scale[1] if nw <= scale[1] else nw)
    ph, pw = (ph + 31) // 32 * 32, (pw + 31) // 32 * 32
    x = F.pad(x, (0, pw - nw, 0, ph - nh)).contiguous()
    sf = np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32)
    meta = dict(ori_shape=(h, w, 3), img_shape=(nh, nw, 3), pad_shape=(ph, pw, 3), scale_factor=sf,
                flip=False, flip_direction='horizontal')
    return x, meta


def _batched(samples_per_gpu, pipeline, cache, group_by=None):
    """True when single_gpu_test / multi_gpu_test are asked for the batched device path (test_pipeline.run_test);
    the defaults keep the per-image path."""
    if int(samples_per_gpu) < 1:
        raise ValueError(f'samples_per_gpu must be >= 1, got {samples_per_gpu}')
    if group_by is not None:
        from .grouped_eval import check_group_by
        check_group_by(group_by)
    return int(samples_per_gpu) > 1 or pipeline is not None or cache is not None or group_by is not None


def _run_batched(model, dataset, device, indices, scale, samples_per_gpu, pipeline, cache, log, group_by=None,
                 max_batch_pixels='default'):
    from . import grouped_eval
    from . import test_pipeline as TP
    pipe = pipeline if isinstance(pipeline, TP.DeviceTestPipeline) else TP.DeviceTestPipeline(pipeline, scale=scale)
    source = TP.source_for(dataset, cache, device)
    return grouped_eval.run_test(model, dataset, device, indices, pipe, source, samples_per_gpu, log=log, group_by=group_by,
                       max_batch_pixels=max_batch_pixels)


def single_gpu_test(model, dataset, device, scale=(640, 640), max_images=None, samples_per_gpu=1, pipeline=None,
                    cache=None, log=None, group_by=None, max_batch_pixels='default'):
    """mmdet/apis/test.py single_gpu_test for this path: eval-mode forward + get_bboxes(rescale=True) per image
    of a test-mode RetinaFaceDataset -> [[dets [n, 5]]] per image (boxes in original-image coordinates).

    samples_per_gpu > 1, pipeline (the config's test pipeline list, or a DeviceTestPipeline) or cache ('device':
    the decoded images stay in a device store kept on the dataset) select the batched device path
    (test_pipeline.run_test): consecutive images in batches of samples_per_gpu, the last batch short, results in
    dataset order.  `scale` is the view when the pipeline names none.

    group_by='canvas' selects that path too and batches the images by their padded shape instead
    (grouped_eval.group_batches): every batch's canvas is each of its images' own pad_shape, so the detections are
    those of samples_per_gpu=1 -- the per-image protocol, e.g. WIDER "in origin size" -- in fewer forwards.
    max_batch_pixels caps the canvas pixels of a grouped batch (default samples_per_gpu * 1024 * 1024, None: no
    cap).  The results stay in dataset order."""
    import torch
    was_training = model.training
    model.eval()
    out = []
    n = len(dataset) if max_images is None else min(len(dataset), max_images)
    with torch.no_grad():
        if _batched(samples_per_gpu, pipeline, cache, group_by):
            out = _run_batched(model, dataset, device, list(range(n)), scale, samples_per_gpu, pipeline, cache, log,
                               group_by, max_batch_pixels)
        else:
            for i in range(n):
                img, meta = prepare_test_image(dataset.load_image(i), scale, device)
                meta['ori_filename'] = dataset.data_infos[i]['filename']
                out.append(model(return_loss=False, rescale=True, img=[img], img_metas=[[meta]])[0])
    if was_training:
        model.train()
    return out


def multi_gpu_test(model, dataset, device, scale=(640, 640), max_images=None, group=None, samples_per_gpu=1,
                   pipeline=None, cache=None, log=None, group_by=None, max_batch_pixels='default'):
    """mmdet/apis/test.py multi_gpu_test for this path (what the reference's DistEvalHook runs): rank r takes the
    images r, r + world, r + 2 world, ...; the per-image results are gathered and put back in dataset order
    (collect_results).  Returns the full list on rank 0 and None on the other ranks.  samples_per_gpu / pipeline /
    cache / group_by / max_batch_pixels: as single_gpu_test, over the rank's own list (the images are sharded
    first and grouped inside the rank's shard)."""
    import torch
    import torch.distributed as dist
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    was_training = model.training
    model.eval()
    n = len(dataset) if max_images is None else min(len(dataset), max_images)
    part = []
    with torch.no_grad():
        if _batched(samples_per_gpu, pipeline, cache, group_by):
            part = _run_batched(model, dataset, device, list(range(rank, n, world)), scale, samples_per_gpu, pipeline,
                                cache, log, group_by, max_batch_pixels)
        else:
            for i in range(rank, n, world):
                img, meta = prepare_test_image(dataset.load_image(i), scale, device)
                meta['ori_filename'] = dataset.data_infos[i]['filename']
                part.append(model(return_loss=False, rescale=True, img=[img], img_metas=[[meta]])[0])
    if was_training:
        model.train()
    parts = [None] * world
    dist.all_gather_object(parts, part, group=group)
    if rank != 0:
        return None
    out = [None] * n
    for r, p in enumerate(parts):
        for k, res in enumerate(p):
            out[r + k * world] = res
    return out
