"""GPU: the ranking and the curve of the mAP protocol on the device (csrc/score.hip through
eval_map_single_class(rank='device')) against the host path, which tests/test_eval_map.py pins to the unmodified
reference.  Every comparison is equality: the orders are permutations, the cumulative counts integers below 2^24 (exact
in fp32), the precision one correctly rounded fp32 division and its envelope a maximum.

On tied scores the host path's default np.argsort is not stable, so there the yardstick is a restatement of it here
with kind='stable' in both argsort calls (per image in tpfp_default, and the global ranking): the device's tie rule."""
import os

import numpy as np
import pytest
import torch

import test_score_gpu as TS

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the stable restatement
def tpfp_stable(dets, gts, gts_ignore, iou_thr):
    """evaluation.tpfp_default with np.argsort(..., kind='stable')."""
    import yunet_amd.evaluation as E
    m = dets.shape[0]
    tp, fp = np.zeros(m, dtype=np.float32), np.zeros(m, dtype=np.float32)
    ignore = np.concatenate([np.zeros(gts.shape[0], dtype=bool), np.ones(gts_ignore.shape[0], dtype=bool)])
    allgt = np.vstack([gts.reshape(-1, 4), gts_ignore.reshape(-1, 4)])
    if allgt.shape[0] == 0:
        fp[...] = 1
        return tp, fp
    ious = E.bbox_overlaps_np(dets[:, :4], allgt)
    best, arg = ious.max(axis=1), ious.argmax(axis=1)
    covered = np.zeros(allgt.shape[0], dtype=bool)
    for i in np.argsort(-dets[:, -1], kind='stable'):
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


def eval_stable(dets, anns, iou_thr):
    """evaluation.eval_map_single_class(device=None) with the stable order in both places."""
    import yunet_amd.evaluation as E
    d = [np.asarray(x[0], dtype=np.float32).reshape(-1, 5) for x in dets]
    gtl = [np.asarray(a['bboxes'], dtype=np.float32).reshape(-1, 4) for a in anns]
    ignl = [np.asarray(a['bboxes_ignore'], dtype=np.float32).reshape(-1, 4) for a in anns]
    num_gts = sum(g.shape[0] for g in gtl)
    both = [tpfp_stable(x, g, k, iou_thr) for x, g, k in zip(d, gtl, ignl)]
    alld = np.vstack(d)
    order = np.argsort(-alld[:, -1], kind='stable')
    tp = np.cumsum(np.hstack([b[0] for b in both])[order]) if alld.shape[0] else np.zeros(0, dtype=np.float32)
    fp = np.cumsum(np.hstack([b[1] for b in both])[order]) if alld.shape[0] else np.zeros(0, dtype=np.float32)
    eps = np.finfo(np.float32).eps
    recalls = tp / np.maximum(np.array([num_gts]), eps)
    precisions = tp / np.maximum(tp + fp, eps)
    ap = E.average_precision_area(recalls, precisions)
    res = dict(num_gts=num_gts, num_dets=int(alld.shape[0]), recall=recalls, precision=precisions, ap=ap)
    return (float(ap) if num_gts > 0 else 0.0), res


def same(got, want):
    (ga, gr), (wa, wr) = got, want
    assert ga == wa and type(ga) is type(wa), (ga, wa)
    assert gr['num_gts'] == wr['num_gts'] and gr['num_dets'] == wr['num_dets']
    assert gr['ap'] == wr['ap'] and type(gr['ap']) is type(wr['ap']) is np.float32
    for k in ('recall', 'precision'):
        assert gr[k].dtype == wr[k].dtype and gr[k].shape == wr[k].shape, k
        assert np.array_equal(gr[k], wr[k]), (k, np.nonzero(gr[k] != wr[k])[0][:5])


def orders(dets):
    """(order of entry a, rank of entry b) of a set, as numpy arrays, and the packed scores with their offsets."""
    from yunet_amd import kernels as K
    d = [np.asarray(x[0], dtype=np.float32).reshape(-1, 5) for x in dets]
    off = np.concatenate([[0], np.cumsum([x.shape[0] for x in d])]).astype(np.int64)
    alld = torch.from_numpy(np.ascontiguousarray(np.vstack(d))).to(DEV)
    order = K.score_rank_images(alld, torch.from_numpy(off).to(DEV))
    rank = K.score_rank_global(alld)
    return order.cpu().numpy(), rank.cpu().numpy(), np.vstack(d)[:, 4], off


def check_orders(dets):
    order, rank, s, off = orders(dets)
    assert order.dtype == rank.dtype == np.int32
    assert np.array_equal(rank, np.argsort(-s, kind='stable'))
    for i in range(len(off) - 1):
        assert np.array_equal(order[off[i]:off[i + 1]], np.argsort(-s[off[i]:off[i + 1]], kind='stable')), i


# ------------------------------------------------------------------------------------------------------ the sets
GRID = 1 << 20          # k / 2^20 is a float32 for every k below it: distinct integers are distinct scores


def boxes_for(rng, counts, hit=0.75, no_box=(), n_ignored=2):
    """Per image: kept and ignored boxes and counts[i] detections (jittered copies of the boxes with probability `hit`,
    stray boxes otherwise), scores left at zero.  Images in no_box have no box at all."""
    dets, anns = [], []
    for i, n in enumerate(counts):
        g, k = (0, 0) if i in no_box else (int(rng.integers(1, 7)), int(rng.integers(0, n_ignored + 1)))
        xy = rng.uniform(0, 300, (g + k, 2))
        box = np.concatenate([xy, xy + rng.uniform(8, 90, (g + k, 2))], 1).astype(np.float32)
        d = np.concatenate([rng.uniform(400, 700, (n, 2)), rng.uniform(5, 60, (n, 2))], 1)
        d[:, 2:] += d[:, :2]
        if g + k:
            near = rng.uniform(size=n) < hit
            pick = rng.integers(0, g + k, n)
            d[near] = (box[pick] + rng.normal(0, 3.0, (n, 4)))[near]
        dets.append([np.concatenate([d, np.zeros((n, 1))], 1).astype(np.float32)])
        anns.append(dict(bboxes=box[:g], labels=np.zeros(g, np.int64), bboxes_ignore=box[g:],
                         labels_ignore=np.zeros(k, np.int64)))
    return dets, anns


def set_scores(dets, scores):
    scores = np.asarray(scores, dtype=np.float32)
    assert scores.shape[0] == sum(d[0].shape[0] for d in dets)
    at = 0
    for d in dets:
        d[0][:, 4] = scores[at:at + d[0].shape[0]]
        at += d[0].shape[0]
    return dets


def distinct_scores(rng, n):
    s = (rng.choice(np.arange(1, GRID), n, replace=False) / GRID).astype(np.float32)
    assert np.unique(s).shape[0] == n, 'the scores are drawn without replacement from a grid of float32 values'
    return s


def spread(total, most=211):
    """Per-image counts that sum to `total`: images of `most` detections, the remainder, one image without any."""
    counts = [most] * (total // most) + ([total % most] if total % most else [])
    return counts[:1] + [0] + counts[1:]


def tie_free(seed, counts, **kw):
    rng = np.random.default_rng(seed)
    dets, anns = boxes_for(rng, counts, **kw)
    return set_scores(dets, distinct_scores(rng, sum(counts))), anns


# ------------------------------------------------------------------------------------------------ 1. tie-free sets
@pytest.mark.parametrize('iou_thr', [0.5, 0.55])
@pytest.mark.parametrize('seed', [0, 1])
def test_tie_free_sets_equal_the_host_path(seed, iou_thr):
    import yunet_amd.evaluation as E
    counts = [int(v) for v in np.random.default_rng(100 + seed).integers(0, 60, 24)]
    counts[2], counts[5], counts[9] = 0, 300, 1
    dets, anns = tie_free(seed, counts, no_box=(3, 11))
    assert sum(a['bboxes_ignore'].shape[0] for a in anns) > 0 and anns[3]['bboxes'].shape[0] == 0 and counts[3] > 0
    host = E.eval_map_single_class(dets, anns, iou_thr)
    got = E.eval_map_single_class(dets, anns, iou_thr, device=DEV, rank='device')
    same(got, host)
    same(got, E.eval_map_single_class(dets, anns, iou_thr, device=DEV, rank=None))
    same(got, eval_stable(dets, anns, iou_thr))
    assert 0.0 < host[0] < 1.0 and host[1]['precision'].min() < host[1]['precision'].max()
    check_orders(dets)


# --------------------------------------------------------------------------------------------------- 2. tied sets
@pytest.mark.parametrize('iou_thr', [0.5, 0.55])
@pytest.mark.parametrize('seed', [0, 1])
def test_tied_sets_equal_the_stable_restatement(seed, iou_thr):
    """The sets of tests/test_score_gpu.py: scores rounded to one decimal in every other image, duplicates of one box at
    equal scores."""
    import yunet_amd.evaluation as E
    dets, anns = TS.map_set(seed)
    s = np.concatenate([d[0][:, 4] for d in dets])
    assert np.unique(s).shape[0] < s.shape[0] // 2, 'the set is made of ties'
    check_orders(dets)
    want = eval_stable(dets, anns, iou_thr)
    same(E.eval_map_single_class(dets, anns, iou_thr, device=DEV, rank='device'), want)
    assert 0.0 < want[0] < 1.0


# ------------------------------------------------------------------------------------------------ 3. hazard sizes
def hazards():
    """name -> (dets, anns, tie_free).  The sizes follow the kernels' constants: the rows of an image ranked in LDS at
    once, and the tile of the radix sort and of the scans."""
    from yunet_amd import kernels as K
    cap, tile = K.RANK_SEG_CAP, K.RANK_RADIX_TILE
    out = {}
    # per-image counts either side of the LDS variant's capacity, and an image several times that, among small ones
    for n in (cap - 1, cap, cap + 1, 3 * cap + 77):
        out[f'{n}_in_one_image'] = tie_free(n, [7, 0, n, 1, 30]) + (True,)
    # totals either side of a tile
    out['1_in_all'] = tie_free(2, [0, 1, 0]) + (True,)
    for D in (tile - 1, tile, tile + 1, 2 * tile + 1815):
        out[f'{D}_in_all'] = tie_free(D, spread(D)) + (True,)
    rng = np.random.default_rng(5)
    counts = [40, 0, cap + 5, 3, 300]
    D = sum(counts)
    dets, anns = boxes_for(rng, counts)
    out['all_scores_equal'] = (set_scores(dets, np.full(D, 0.625)), anns, False)
    dets, anns = boxes_for(rng, counts)
    out['ascending_scores'] = (set_scores(dets, np.sort(distinct_scores(rng, D))), anns, True)
    dets, anns = boxes_for(rng, counts)
    out['descending_scores'] = (set_scores(dets, np.sort(distinct_scores(rng, D))[::-1]), anns, True)
    # negative and positive scores (logits): the key's two branches
    dets, anns = boxes_for(rng, counts)
    out['signed_scores'] = (set_scores(dets, distinct_scores(rng, D) * 16 - 8), anns, True)
    # every kept box has an exact copy among the detections: the last recall is 1, no trailing term
    dets, anns = boxes_for(rng, [30, 0, 50, 9], no_box=(1,))
    for d, a in zip(dets, anns):
        g = a['bboxes'].shape[0]
        d[0][:g, :4] = a['bboxes']
    out['last_recall_is_one'] = (set_scores(dets, distinct_scores(rng, 89)), anns, True)
    # ... and a set that misses boxes: the trailing term (1 - recall[-1]) * 0
    dets, anns = boxes_for(rng, [2, 0, 3, 1], hit=0.5)
    out['last_recall_below_one'] = (set_scores(dets, distinct_scores(rng, 6)), anns, True)
    dets, anns = boxes_for(rng, [30, 0, 50, 9], hit=0.0)
    out['no_true_positive'] = (set_scores(dets, distinct_scores(rng, 89)), anns, True)
    return out


HAZARDS = None


def hazard(name=None):
    global HAZARDS
    if HAZARDS is None:
        HAZARDS = hazards()
    return HAZARDS if name is None else HAZARDS[name]


HAZARD_NAMES = ['1023_in_one_image', '1024_in_one_image', '1025_in_one_image', '3149_in_one_image', '1_in_all',
                '4095_in_all', '4096_in_all', '4097_in_all', '10007_in_all', 'all_scores_equal', 'ascending_scores',
                'descending_scores', 'signed_scores', 'last_recall_is_one', 'last_recall_below_one', 'no_true_positive']


def test_hazard_list_follows_the_kernel_constants():
    assert sorted(hazard()) == sorted(HAZARD_NAMES)
    for name in HAZARD_NAMES:
        dets = hazard(name)[0]
        if name.endswith('_in_one_image'):
            assert max(d[0].shape[0] for d in dets) == int(name.split('_')[0])
        if name.endswith('_in_all'):
            assert sum(d[0].shape[0] for d in dets) == int(name.split('_')[0])


@pytest.mark.parametrize('name', HAZARD_NAMES)
def test_hazard_set(name):
    import yunet_amd.evaluation as E
    dets, anns, distinct = hazard(name)
    check_orders(dets)
    want = eval_stable(dets, anns, 0.5)
    got = E.eval_map_single_class(dets, anns, 0.5, device=DEV, rank='device')
    same(got, want)
    if distinct:                                    # no ties: the host path itself is the yardstick
        same(got, E.eval_map_single_class(dets, anns, 0.5))
    rec, prec = want[1]['recall'], want[1]['precision']
    if name == 'last_recall_is_one':
        assert rec[-1] == 1.0
    elif name == 'no_true_positive':
        assert want[1]['num_gts'] > 0 and not rec.any() and not prec.any() and got[0] == 0.0
    else:
        assert 0.0 < rec[-1] < 1.0 and got[0] > 0.0


def test_empty_sets():
    import yunet_amd.evaluation as E
    none = np.zeros((0, 5), np.float32)
    box = dict(bboxes=np.array([[0, 0, 5, 5]], np.float32), bboxes_ignore=np.zeros((0, 4), np.float32))
    noann = dict(bboxes=np.zeros((0, 4), np.float32), bboxes_ignore=np.zeros((0, 4), np.float32))
    for dets, anns in (([[none]], [box]), ([[none], [none]], [noann, box]), ([], [])):
        same(E.eval_map_single_class(dets, anns, 0.5, device=DEV, rank='device'), E.eval_map_single_class(dets, anns, 0.5))
    # detections, and no box anywhere: fp for every row, num_gts 0
    d = [[np.array([[0, 0, 5, 5, 0.3], [1, 1, 9, 9, 0.8]], np.float32)]]
    same(E.eval_map_single_class(d, [noann], 0.5, device=DEV, rank='device'), E.eval_map_single_class(d, [noann], 0.5))


# ------------------------------------------------------------------------------------------------- 4. determinism
def test_two_runs_give_identical_bytes():
    import yunet_amd.evaluation as E
    dets, anns, _ = hazard('all_scores_equal')
    tied, tanns = TS.map_set(3)
    for ds, an in ((dets, anns), (tied, tanns), hazard('10007_in_all')[:2]):
        d = [np.asarray(x[0], dtype=np.float32) for x in ds]
        gts, ign = [a['bboxes'] for a in an], [a['bboxes_ignore'] for a in an]
        first = E.curve_device(d, gts, ign, 0.5, DEV)
        again = E.curve_device(d, gts, ign, 0.5, DEV)
        assert first.dtype == np.float32 and first.shape == (4, sum(x.shape[0] for x in d))
        assert first.tobytes() == again.tobytes()
        o1, r1, _, _ = orders(ds)
        o2, r2, _, _ = orders(ds)
        assert o1.tobytes() == o2.tobytes() and r1.tobytes() == r2.tobytes()


# ------------------------------------------------------------------------------------------------- 5. end to end
def test_dataset_evaluate_ranks_on_the_device():
    import yunet_amd
    dets, anns = tie_free(7, [int(v) for v in np.random.default_rng(7).integers(0, 50, 16)])
    ds = yunet_amd.datasets.RetinaFaceDataset.__new__(yunet_amd.datasets.RetinaFaceDataset)
    ds.get_ann_info = lambda i: anns[i]
    host = ds.evaluate(dets, metric='mAP', iou_thr=[0.5, 0.55])
    dev = ds.evaluate(dets, metric='mAP', iou_thr=[0.5, 0.55], device=DEV, rank='device')
    assert dict(dev) == dict(host) and list(dev) == ['AP50', 'AP55', 'mAP'] and 0.0 < host['mAP'] < 1.0
    assert ds.evaluate(dets, metric='mAP', device=DEV, rank='device')['mAP'] == ds.evaluate(dets, metric='mAP')['mAP']


def test_eval_hook_ranks_on_the_device(tmp_path):
    import yunet_amd
    import yunet_amd.runner as R
    ds = TS.face_set(tmp_path, 6, 31)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    cfg.merge_from_dict(dict(
        data=dict(samples_per_gpu=8, val_dataloader=dict(samples_per_gpu=4),
                  val=dict(type='RetinaFaceDataset', ann_file=ds.ann_file, img_prefix=ds.img_prefix, cache='device',
                           pipeline=[dict(type='MultiScaleFlipAug', img_scale=(320, 320), flip=False, transforms=[])])),
        evaluation=dict(interval=1, metric='mAP', score='device', rank='device'),
        runner=dict(type='EpochBasedRunner', max_epochs=1), checkpoint_config=None, work_dir=str(tmp_path / 'work'),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')])))
    cfg.optimizer['lr'] = 1e-5
    model = yunet_amd.build_detector(cfg.model)
    model.load_state_dict(torch.load(TS.TRAINED, map_location='cpu', weights_only=False)['state_dict'], strict=True)
    seen = []
    scored = yunet_amd.evaluation.eval_map_single_class
    yunet_amd.evaluation.eval_map_single_class = lambda *a, **k: (seen.append((k.get('device'), k.get('rank'))),
                                                                  scored(*a, **k))[1]
    try:
        hist = R.train_detector(model, R.SyntheticWiderFace((160, 160), 8, iters_per_epoch=1), cfg, validate=True,
                                device='cuda', log=lambda line: None)
    finally:
        yunet_amd.evaluation.eval_map_single_class = scored
    val = [h for h in hist if h.get('mode') == 'val']
    assert len(val) == 1 and val[0]['mAP'] > 0.2, val
    assert len(seen) == 1 and torch.device(seen[0][0]).type == 'cuda' and seen[0][1] == 'device'
    # the same model (the evaluation ran after the last update) through the host scorer and through the device ranking
    how = dict(scale=(320, 320), samples_per_gpu=4, cache='device',
               pipeline=[dict(type='MultiScaleFlipAug', img_scale=(320, 320), flip=False, transforms=[])])
    logged = {}
    for name, kw in (('host', {}), ('device', dict(score='device', rank='device'))):
        run = TS.StubRunner(model)
        R.EvalHook(ds, **kw, **how)._evaluate(run)
        logged[name] = (run.log_buffer[0]['mAP'], [l for l in run.lines if l.startswith('Epoch(val)')])
    assert logged['host'] == logged['device']
    assert logged['device'][0] == val[0]['mAP'] and len(logged['device'][1]) == 1
