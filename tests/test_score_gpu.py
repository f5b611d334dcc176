"""GPU: the device scorer (csrc/score.hip through evaluation.py's device=...) against the host functions, which
tests/test_evaluation.py pins to the unmodified reference.  Every comparison is equality: the scorer's outputs are
integers (row indices, flags, counts), and the APs are the host's arithmetic on those integers."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as Hh
import wider_fixture as WF

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAINED = os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth')
LIVE_STORED = os.path.join(ROOT, 'tests', 'golden', 'wider_eval_live_reference.npz')


def both(events, pred, iou=0.5):
    """(host counts, device counts, count_face) + the in-place normalisation is the same on both paths."""
    import yunet_amd.evaluation as E
    ph, pd = copy.deepcopy(pred), copy.deepcopy(pred)
    with np.errstate(all='ignore'):
        ch, fh = E.wider_pr_counts(ph, events, iou)
        cd, fd = E.wider_pr_counts(pd, events, iou, device=DEV)
    assert cd.dtype == np.int64 and cd.shape == (3, 1000, 2) and np.array_equal(fh, fd)
    for ev in ph:
        for name in ph[ev]:
            assert np.array_equal(ph[ev][name], pd[ev][name], equal_nan=True), (ev, name)
    return ch, cd, fh


# ------------------------------------------------------------------------------------------------ 1. fixture sets
@pytest.mark.parametrize('seed', [0, 1, 2, 5, 6])
def test_fixture_sets_equal_host_and_reference(seed):
    import yunet_amd.evaluation as E
    if seed < 3:
        g = Hh.load_golden('wider_eval.npz')
        ne, ni = [int(v) for v in g[f'cfg_{seed}']]
        ref = g[f'aps_{seed}']
    else:
        ne, ni = 3, 6
        with np.load(LIVE_STORED) as z:
            ref = z[str(seed)]
    events, pred = WF.synth_events(seed, n_events=ne, imgs_per_event=ni)
    ch, cd, face = both(events, pred)
    assert np.array_equal(ch, cd)
    host = E.wider_evaluation(copy.deepcopy(pred), events, 0.5)
    dev = E.wider_evaluation(copy.deepcopy(pred), events, 0.5, device=DEV)
    assert np.allclose(dev, host, rtol=0, atol=0), (dev, host)
    assert np.allclose(dev, ref, rtol=0, atol=1e-12), (dev, ref)
    assert np.allclose(E.wider_aps_from_counts(cd, face), host, rtol=0, atol=0)


# ------------------------------------------------------------------------------------- 2. one image per hazard
def _gts(rng, g):
    xy = rng.integers(0, 400, (g, 2))
    wh = rng.integers(8, 90, (g, 2))
    return np.concatenate([xy, wh], 1).astype(np.float64)


def _preds(rng, gt, n, order='desc'):
    """n rows: jittered copies of random GTs (several per GT: later ones must not count) and stray boxes."""
    pick = rng.integers(0, len(gt), n)
    box = gt[pick] + rng.normal(0, 0.15, (n, 4)) * gt[pick][:, [2, 3, 2, 3]]
    stray = rng.uniform(size=n) < 0.25
    box[stray] = np.concatenate([rng.uniform(0, 450, (n, 2)), rng.uniform(6, 80, (n, 2))], 1)[stray]
    sc = rng.uniform(0.02, 0.99, n)
    sc = np.sort(sc)[::-1] if order == 'desc' else np.sort(sc) if order == 'asc' else sc
    return np.concatenate([box, sc[:, None]], 1)


def _keep_by_size(gt):
    size = gt[:, 2]
    return dict(easy=np.nonzero(size >= 50)[0] + 1, medium=np.nonzero(size >= 20)[0] + 1,
                hard=np.nonzero(size >= 0)[0] + 1)


def hazards():
    from yunet_amd import kernels as K
    rng = np.random.default_rng(11)
    B, CH = K.SCORE_BLOCK, K.SCORE_GT_CHUNK
    out = {}

    def add(name, gt, pred, keep=None):
        gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
        keep = _keep_by_size(gt) if keep is None else {k: np.asarray(v, dtype=np.int64) for k, v in keep.items()}
        out[name] = (dict(name=name, boxes=gt, keep=keep), np.asarray(pred, dtype=np.float64).reshape(-1, 5))

    g5 = _gts(rng, 5)
    add('no_predictions', g5, np.zeros((0, 5)))
    add('no_ground_truths', np.zeros((0, 4)), _preds(rng, g5, 4))
    add('empty_subsets', g5, _preds(rng, g5, 9), dict(easy=[], medium=[], hard=[1, 2, 3, 4, 5]))
    add('one_prediction', g5, _preds(rng, g5, 1))
    for n in (B - 1, B, B + 1, 2 * B + 1):
        g = _gts(rng, 12)
        add(f'{n}_predictions', g, _preds(rng, g, n))
    g = _gts(rng, CH + 1)
    p = _preds(rng, g, 40)
    p[:6, :4] = g[[CH, CH, CH - 1, 0, CH, CH - 1]]          # hits on the boxes either side of the chunk boundary
    add('chunk_plus_one_ground_truths', g, p)
    g = _gts(rng, 7)
    add('ascending_scores', g, _preds(rng, g, 60, 'asc'))
    add('shuffled_scores', g, _preds(rng, g, 300, 'shuffled'))
    # two ground truths with the same IoU, bit for bit, to every prediction: the first index wins.  Only the second is
    # "easy", so the other choice would count differently
    add('equal_iou_first_index', [[10, 10, 40, 50], [10, 10, 40, 50], [200, 200, 30, 30]],
        [[12, 11, 40, 50, 0.9], [10, 10, 40, 50, 0.8], [9, 12, 38, 47, 0.7], [200, 201, 30, 30, 0.6]],
        dict(easy=[2, 3], medium=[2, 3], hard=[1, 2, 3]))
    # IoU = 50 / 100 exactly: a hit at iou_thresh 0.5
    add('iou_exactly_half', [[0, 0, 9, 9]], [[0, 0, 4, 9, 0.8], [50, 50, 9, 9, 0.3]], dict(easy=[1], medium=[1], hard=[1]))
    # normalised scores 1, 0.5 and 0 sit on table values (thr[499] = 0.5, thr[999] = 0)
    add('scores_on_table_values', g5, np.concatenate([g5[[0, 1, 2]], [[1.0], [0.5], [0.0]]], 1))
    add('all_scores_equal', g5, np.concatenate([g5[[0, 1, 1, 3]], np.full((4, 1), 0.625)], 1))
    add('three_on_one_ground_truth', [[100, 100, 60, 60]],
        [[101, 100, 60, 60, 0.9], [100, 102, 59, 60, 0.7], [99, 100, 60, 61, 0.5], [300, 300, 20, 20, 0.4]],
        dict(easy=[1], medium=[1], hard=[1]))
    return out


HAZARDS = None


def hazard(name=None):
    global HAZARDS
    if HAZARDS is None:
        HAZARDS = hazards()
    return HAZARDS if name is None else HAZARDS[name]


HAZARD_NAMES = ['no_predictions', 'no_ground_truths', 'empty_subsets', 'one_prediction', '255_predictions',
                '256_predictions', '257_predictions', '513_predictions', 'chunk_plus_one_ground_truths',
                'ascending_scores', 'shuffled_scores', 'equal_iou_first_index', 'iou_exactly_half',
                'scores_on_table_values', 'all_scores_equal', 'three_on_one_ground_truth']


def test_hazard_list_follows_the_kernel_constants():
    assert sorted(hazard()) == sorted(HAZARD_NAMES)


@pytest.mark.parametrize('name', HAZARD_NAMES)
def test_hazard_image_alone(name):
    im, pred = hazard(name)
    events = [dict(name='ev', images=[im])]
    ch, cd, _ = both(events, {'ev': {name: pred}})
    assert np.array_equal(ch, cd), np.argwhere(ch != cd)[:5]
    if name in ('equal_iou_first_index', 'iou_exactly_half', 'three_on_one_ground_truth', 'scores_on_table_values'):
        assert ch.any(), 'the case must count something to mean something'
    if name == 'all_scores_equal':
        assert not ch.any()                        # 0 / 0: NaN passes no threshold


def test_hazard_images_in_a_mixed_set():
    events, pred = WF.synth_events(4, n_events=2, imgs_per_event=5)
    names = list(HAZARD_NAMES)
    for k, name in enumerate(names):               # spread over the events, between the fixture's images
        im, p = hazard(name)
        ev = events[k % 2]
        ev['images'].insert((3 * k) % (len(ev['images']) + 1), im)
        pred[ev['name']][name] = p
    ch, cd, _ = both(events, pred)
    assert np.array_equal(ch, cd), np.argwhere(ch != cd)[:5]
    # run to run: the same integers
    _, again, _ = both(events, pred)
    assert np.array_equal(cd, again)
    # another iou threshold, and a prediction entry no event lists (it only moves the score range)
    pred['elsewhere'] = {'x': np.array([[1., 2., 30., 40., 1.75]])}
    ch, cd, _ = both(events, pred, iou=0.4)
    assert np.array_equal(ch, cd)


# ------------------------------------------------------------------------------------- 3. the matching stage alone
def test_matching_stage_equals_argmax_and_threshold():
    import yunet_amd.evaluation as E
    from yunet_amd import kernels as K
    rng = np.random.default_rng(0)
    images, pred = [], {}
    for k in range(50):
        g, n = int(rng.integers(1, 8)), int(rng.integers(1, 30))
        gt = np.concatenate([rng.uniform(0, 100, (g, 2)), rng.uniform(5, 60, (g, 2))], 1).round()
        pick = rng.integers(0, g, n)
        pr = gt[pick] + rng.normal(0, 4, (n, 4))
        pred[f'im{k}'] = np.concatenate([pr, np.sort(rng.uniform(0, 1, (n, 1)), 0)[::-1]], 1)
        images.append(dict(name=f'im{k}', boxes=gt, keep=dict(easy=np.zeros(0, np.int64), medium=np.zeros(0, np.int64),
                                                               hard=np.arange(1, g + 1))))
    im, p = hazard('chunk_plus_one_ground_truths')
    images.append(im)
    pred[im['name']] = p
    rows, poff, boxes, goff, _, _ = E.pack_wider({'ev': pred}, [dict(name='ev', images=images)])
    d = [torch.from_numpy(a).to(DEV) for a in (rows, poff, boxes, goff)]
    best, hit, first = [t.cpu().numpy() for t in K.score_wider_match(*d, 0.5)]
    some_hit = False
    for i, im in enumerate(images):
        iou = E.pairwise_iou_xywh(pred[im['name']][:, :4], im['boxes'])
        want = iou.argmax(axis=1)
        want_hit = iou[np.arange(len(want)), want] >= 0.5
        assert np.array_equal(best[poff[i]:poff[i + 1]], want), i
        assert np.array_equal(hit[poff[i]:poff[i + 1]].astype(bool), want_hit), i
        want_first = np.full(len(im['boxes']), 2 ** 31 - 1)
        for r in np.nonzero(want_hit)[0][::-1]:
            want_first[want[r]] = r
        assert np.array_equal(first[goff[i]:goff[i + 1]], want_first), i
        some_hit |= bool(want_hit.any()) and not bool(want_hit.all())
    assert some_hit


# ------------------------------------------------------------------------------------------------------- 4. mAP
def map_set(seed, n_img=12):
    """Detections (float32 xyxy + score) and annotations with ignored boxes; one image without any box, one without
    detections, tied scores inside images, several detections per box."""
    rng = np.random.default_rng(seed)
    dets, anns = [], []
    for i in range(n_img):
        g, k = (0, 0) if i == 3 else (int(rng.integers(1, 7)), int(rng.integers(0, 3)))
        xy = rng.uniform(0, 300, (g + k, 2))
        box = np.concatenate([xy, xy + rng.uniform(8, 90, (g + k, 2))], 1).astype(np.float32)
        n = 0 if i == 5 else int(rng.integers(1, 40)) if i != 7 else 300
        if g + k:
            pick = rng.integers(0, g + k, n)
            d = box[pick] + rng.normal(0, 3.0, (n, 4)).astype(np.float32)
        else:
            d = rng.uniform(0, 300, (n, 4)).astype(np.float32)
        sc = np.round(rng.uniform(0.02, 1.0, n), 1 if i % 2 else 6)             # one decimal: many ties
        dets.append([np.concatenate([d, sc[:, None]], 1).astype(np.float32)])
        anns.append(dict(bboxes=box[:g], labels=np.zeros(g, np.int64), bboxes_ignore=box[g:],
                         labels_ignore=np.zeros(k, np.int64)))
    # duplicates of one kept box at tied scores, and an IoU of exactly 110 / 200 = float32(0.55)
    dets.append([np.array([[0, 0, 20, 10, 0.5], [0, 0, 20, 10, 0.5], [0, 0, 11, 10, 0.5], [0, 0, 20, 10, 0.9],
                           [0, 0, 10, 10, 0.7]], np.float32)])
    anns.append(dict(bboxes=np.array([[0, 0, 20, 10]], np.float32), labels=np.zeros(1, np.int64),
                     bboxes_ignore=np.zeros((0, 4), np.float32), labels_ignore=np.zeros(0, np.int64)))
    return dets, anns


@pytest.mark.parametrize('iou_thr', [0.5, 0.55])
@pytest.mark.parametrize('seed', [0, 1])
def test_map_tpfp_equals_tpfp_default(seed, iou_thr):
    import yunet_amd.evaluation as E
    dets, anns = map_set(seed)
    d = [x[0] for x in dets]
    gts = [a['bboxes'] for a in anns]
    ign = [a['bboxes_ignore'] for a in anns]
    tp, fp = E.tpfp_device(d, gts, ign, iou_thr, DEV)
    want = [E.tpfp_default(x, g, k, iou_thr) for x, g, k in zip(d, gts, ign)]
    wtp, wfp = np.hstack([w[0] for w in want]), np.hstack([w[1] for w in want])
    assert tp.dtype == fp.dtype == np.float32
    assert np.array_equal(tp, wtp) and np.array_equal(fp, wfp)
    assert wtp.any() and wfp.any() and ((wtp + wfp) == 0).any()         # all three outcomes occur
    host, hres = E.eval_map_single_class(dets, anns, iou_thr)
    dev, dres = E.eval_map_single_class(dets, anns, iou_thr, device=DEV)
    assert dev == host and dres['ap'] == hres['ap'] and dres['num_gts'] == hres['num_gts']
    assert np.array_equal(dres['recall'], hres['recall']) and np.array_equal(dres['precision'], hres['precision'])


def test_map_edge_sets_and_dataset_evaluate():
    import yunet_amd
    import yunet_amd.evaluation as E
    none = np.zeros((0, 5), np.float32)
    noann = dict(bboxes=np.zeros((0, 4), np.float32), bboxes_ignore=np.zeros((0, 4), np.float32))
    # no detections at all; detections but no box anywhere (fp for every row)
    assert E.eval_map_single_class([[none]], [noann], 0.5, device=DEV)[0] == E.eval_map_single_class([[none]], [noann], 0.5)[0]
    d = [np.array([[0, 0, 5, 5, 0.3], [1, 1, 9, 9, 0.8]], np.float32)]
    tp, fp = E.tpfp_device(d, [noann['bboxes']], [noann['bboxes_ignore']], 0.5, DEV)
    assert np.array_equal(tp, [0, 0]) and np.array_equal(fp, [1, 1])
    # more boxes than one LDS chunk
    from yunet_amd import kernels as K
    rng = np.random.default_rng(3)
    g = K.SCORE_GT_CHUNK + 1
    xy = rng.uniform(0, 2000, (g, 2))
    box = np.concatenate([xy, xy + rng.uniform(8, 60, (g, 2))], 1).astype(np.float32)
    det = np.concatenate([box[[g - 1, g - 1, 0, g - 2]] + np.float32(0.5), [[0.9], [0.8], [0.7], [0.6]]], 1).astype(np.float32)
    tp, fp = E.tpfp_device([det], [box[:g - 1]], [box[g - 1:]], 0.5, DEV)
    wtp, wfp = E.tpfp_default(det, box[:g - 1], box[g - 1:], 0.5)
    assert np.array_equal(tp, wtp) and np.array_equal(fp, wfp)
    # RetinaFaceDataset.evaluate passes the device through
    dets, anns = map_set(2)
    ds = yunet_amd.datasets.RetinaFaceDataset.__new__(yunet_amd.datasets.RetinaFaceDataset)
    ds.get_ann_info = lambda i: anns[i]
    host = ds.evaluate(dets, iou_thr=[0.5, 0.55])
    dev = ds.evaluate(dets, iou_thr=[0.5, 0.55], device=DEV)
    assert dict(dev) == dict(host) and list(dev) == ['AP50', 'AP55', 'mAP'] and 0.0 < host['mAP'] < 1.0


# ------------------------------------------------------------------------------------------------ 5. end to end
def face_set(tmp_path, n, seed):
    """The synthetic protocol fixture of the test-pipeline tests: painted faces as lossless files + a labelv2 list."""
    from PIL import Image
    import yunet_amd
    import yunet_amd.synthetic as S
    b = S.make_batch(n, 320, 320, seed, structured=True)
    os.makedirs(tmp_path / 'img', exist_ok=True)
    lines = []
    for i in range(n):
        im = np.ascontiguousarray(b['img'][i].permute(1, 2, 0).clamp(0, 255).byte().numpy())
        Image.fromarray(im[:, :, ::-1].copy()).save(tmp_path / 'img' / f'{i}.png')
        lines.append(f'# {i}.png {im.shape[1]} {im.shape[0]}')
        for box in b['gt_bboxes'][i]:
            lines.append('%.2f %.2f %.2f %.2f' % tuple(float(v) for v in box))
    (tmp_path / 'img.txt').write_text('\n'.join(lines) + '\n')
    return yunet_amd.build_dataset(dict(type='RetinaFaceDataset', ann_file=str(tmp_path / 'img.txt'),
                                        img_prefix=str(tmp_path / 'img'), test_mode=True))


class StubRunner:
    """What EvalHook._evaluate reads of a runner."""

    def __init__(self, model):
        self.model, self.device, self.rank, self.epoch, self.iter = model, torch.device('cuda'), 0, 0, 0
        self.log_buffer, self.lines = [], []

    def logger(self, line):
        self.lines.append(line)


def test_eval_hook_scores_on_the_device(tmp_path):
    import yunet_amd
    import yunet_amd.runner as R
    ds = face_set(tmp_path, 6, 31)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    cfg.merge_from_dict(dict(
        data=dict(samples_per_gpu=8, val_dataloader=dict(samples_per_gpu=4),
                  val=dict(type='RetinaFaceDataset', ann_file=ds.ann_file, img_prefix=ds.img_prefix, cache='device',
                           pipeline=[dict(type='MultiScaleFlipAug', img_scale=(320, 320), flip=False, transforms=[])])),
        evaluation=dict(interval=1, metric='mAP', score='device'), runner=dict(type='EpochBasedRunner', max_epochs=1),
        checkpoint_config=None, work_dir=str(tmp_path / 'work'),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')])))
    cfg.optimizer['lr'] = 1e-5
    model = yunet_amd.build_detector(cfg.model)
    model.load_state_dict(torch.load(TRAINED, map_location='cpu', weights_only=False)['state_dict'], strict=True)
    seen = []
    scored = yunet_amd.evaluation.eval_map_single_class
    yunet_amd.evaluation.eval_map_single_class = lambda *a, **k: (seen.append(k.get('device')), scored(*a, **k))[1]
    try:
        lines = []
        hist = R.train_detector(model, R.SyntheticWiderFace((160, 160), 8, iters_per_epoch=1), cfg, validate=True,
                                device='cuda', log=lines.append)
    finally:
        yunet_amd.evaluation.eval_map_single_class = scored
    val = [h for h in hist if h.get('mode') == 'val']
    assert len(val) == 1 and val[0]['mAP'] > 0.2, val
    assert len(seen) == 1 and seen[0] is not None and torch.device(seen[0]).type == 'cuda'
    # the same model (the evaluation ran after the last update) through EvalHook() and EvalHook(score='device')
    how = dict(scale=(320, 320), samples_per_gpu=4, cache='device',
               pipeline=[dict(type='MultiScaleFlipAug', img_scale=(320, 320), flip=False, transforms=[])])
    logged = {}
    for score in (None, 'host', 'device'):
        run = StubRunner(model)
        R.EvalHook(ds, score=score, **how)._evaluate(run)
        logged[score] = (run.log_buffer[0]['mAP'], [l for l in run.lines if l.startswith('Epoch(val)')])
    assert logged[None] == logged['host'] == logged['device']
    assert logged['device'][0] == val[0]['mAP'] and len(logged['device'][1]) == 1
    assert model.training


def test_widerface_tool_scores_on_the_device(tmp_path):
    from PIL import Image
    import detect_oracle as D
    events, _ = WF.synth_events(7, n_events=2, imgs_per_event=3)
    rng = np.random.default_rng(0)
    lines = []
    for ev in events:
        os.makedirs(tmp_path / 'images' / ev['name'], exist_ok=True)
        for im in ev['images']:
            h, w = int(rng.integers(200, 420)), int(rng.integers(260, 520))
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(
                tmp_path / 'images' / ev['name'] / (im['name'] + '.jpg'))
            lines.append(f"# {ev['name']}/{im['name']}.jpg {w} {h}")
            for b in im['boxes']:
                lines.append('%d %d %d %d' % (b[0], b[1], b[0] + b[2], b[1] + b[3]))
    os.makedirs(tmp_path / 'labelv2' / 'val', exist_ok=True)
    (tmp_path / 'labelv2' / 'val' / 'labelv2.txt').write_text('\n'.join(lines) + '\n')
    WF.write_mats(events, str(tmp_path / 'labelv2' / 'val' / 'gt'))
    arch, sd = D.make_state('n', 5, size=160)
    torch.save(dict(state_dict=sd, meta={}), tmp_path / 'ck.pth')
    cfg = open(os.path.join(ROOT, 'configs', 'yunet_n.py')).read() + f"""
data = dict(samples_per_gpu=1, test=dict(type='RetinaFaceDataset', samples_per_gpu=4,
            ann_file={str(tmp_path / 'labelv2' / 'val' / 'labelv2.txt')!r},
            img_prefix={str(tmp_path / 'images')!r}, pipeline=[]))
"""
    (tmp_path / 'cfg.py').write_text(cfg)
    text = {}
    for score in ('host', 'device'):
        out = tmp_path / f'out_{score}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'widerface_batched.py'), str(tmp_path / 'cfg.py'),
                            str(tmp_path / 'ck.pth'), '--out', str(out), '--mode', '320', '--thr', '0.3', '--score', score],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-1500:]
        text[score] = (open(out / 'aps').read(), [l for l in r.stdout.splitlines() if l.startswith('APS:')])
    assert text['host'] == text['device'] and len(text['host'][0].strip().split(',')) == 3
