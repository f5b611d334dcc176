"""-m gpu: Soft-NMS on the device (csrc/detect.hip: detect_soft_kernel, through yunet_soft_nms / yunet_detect_soft)
against the numpy restatement of mmcv's softnms_cpu (tests/soft_nms_ref.py; mmcv parity itself is unpinned, see there).

Every comparison is preceded by the restatement's Guard: the fixture keeps each decision of the run (score order, IoU vs
iou_threshold, score vs min_score) at least 1e-4 (relative) from its boundary.  A guard failure is a broken fixture.

naive / linear scores are compared BIT FOR BIT with the float32 restatement: nms_iou and `score *= weight` are the same
sequence of single-rounded fp32 operations on both sides (detect.hip is built with -ffp-contract=off).  gaussian scores
are compared with the float64 restatement to a derived bound, GAUSS_PER_ROUND below."""
import functools

import numpy as np
import pytest
import torch

import soft_nms_ref as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
IOU_THR, SIGMA = 0.3, 0.5
U = S.U32
# gaussian: the bound on a row that follows r selections is r * (expf's error + the multiply's rounding), relative, against the
# float64 restatement on the same fp32 inputs: expf is within 1 ulp = 2 u (HIP math API, single precision exp), the multiply
# into the score rounds once (u).  The first row is the input score itself and is exact.
# This leaves out the fp32 rounding of expf's ARGUMENT -(ovr * ovr) / sigma (34 roundings on the way, amplified by
# |argument| <= 1 / sigma: up to 34 u / sigma more per round in the worst case); the narrower bound is the one asserted.
# Measured on an MI355X: the worst row reaches 0.16 of it (set 1, row 9: 2.2 u against 27 u).
GAUSS_PER_ROUND = (2.0 + 1.0) * U


def _run(boxes, scores, method, min_score, counts=None, score_thr=float('-inf'), max_out=None):
    import yunet_amd.kernels as K
    b = torch.from_numpy(np.ascontiguousarray(boxes)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(scores)).to(DEV)
    c = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    dets, keep, cnt = K.soft_nms(b, s, IOU_THR, SIGMA, min_score, method, score_thr=score_thr, max_out=max_out, counts=c)
    torch.cuda.synchronize()
    return dets.cpu().numpy(), keep.cpu().numpy(), cnt.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(key, method, min_score, max_out=None):
    """(boxes, scores, keep, fp32 scores, fp64 scores) of a named fixture, guard asserted; computed once per process."""
    boxes, scores = _fixture(key)
    g = S.Guard()
    k64, s64 = S.soft_nms_live(boxes, scores, IOU_THR, SIGMA, min_score, method, max_out=max_out, dtype=np.float64, guard=g)
    assert g.ok(1e-4), f'broken fixture {key} {method} {min_score}: {g}'
    k32, s32 = S.soft_nms_live(boxes, scores, IOU_THR, SIGMA, min_score, method, max_out=max_out)
    assert np.array_equal(k32, k64)
    return boxes, scores, k32, s32, s64


def _fixture(key):
    kind, arg = key
    if kind == 'cluster':                       # (seed, count): the first `count` boxes of a cluster fixture
        b, s = S.cluster_fixture(arg[0])
        return b[:arg[1]], s[:arg[1]]
    if kind == 'low_third':                     # a third of the scores start below min_score = 0.05
        b, s = S.cluster_fixture(arg)
        s = s.copy()
        s[::3] *= np.float32(0.045)
        return b, s
    if kind == 'all_low':
        b, s = S.cluster_fixture(arg)
        return b, s * np.float32(0.045)
    if kind == 'grid':
        return S.grid_plus_cluster(arg[0], arg[1], arg[2])
    raise KeyError(key)


def _check_rows(dets, keep, count, ref, method, what):
    boxes, scores, k32, s32, s64 = ref
    assert count == len(k32), (what, count, len(k32))
    assert np.array_equal(keep[:count], k32), f'{what}: selection or order differs'
    assert np.array_equal(dets[:count, :4], boxes[k32]), f'{what}: boxes'
    got = dets[:count, 4]
    if method == 'gaussian':
        rel = np.abs(got.astype(np.float64) - s64) / s64
        bound = np.arange(count) * GAUSS_PER_ROUND                # row r follows r selections
        print(f'{what}: gaussian max rel err {rel.max():.3g}; worst rel / bound = '
              f'{float(np.max(rel[1:] / bound[1:])) if count > 1 else 0.0:.3f}')
        assert np.all(rel <= bound), (what, float(rel.max()))
    else:
        assert np.array_equal(got.view(np.uint32), s32.view(np.uint32)), f'{what}: score bits'
    assert np.all(np.diff(got) <= 0)


@pytest.mark.parametrize('min_score', [1e-3, 0.05])
@pytest.mark.parametrize('method', ['naive', 'linear', 'gaussian'])
def test_explicit_candidates_lds_keys(method, min_score):
    """Three sets in one launch with per-set counts 96 / 40 / 1."""
    counts = [96, 40, 1]
    sets = [S.cluster_fixture(seed) for seed in (0, 1, 2)]
    dets, keep, cnt = _run(np.stack([b for b, _ in sets]), np.stack([s for _, s in sets]), method, min_score, counts=counts)
    for n, c in enumerate(counts):
        ref = _reference(('cluster', (n, c)), method, min_score)
        _check_rows(dets[n], keep[n], int(cnt[n]), ref, method, f'set {n}')
    assert int(cnt[2]) == 1 and int(cnt[0]) > int(cnt[2])


def test_score_thr_below_min_score():
    """score_thr = -inf, min_score = 0.05, a third of the scores below it: those candidates vanish after round one (the
    min_score test also runs where the weight was 1), and the first selection is never filtered."""
    ref = _reference(('low_third', 0), 'linear', 0.05)
    boxes, scores = ref[0], ref[1]
    dets, keep, cnt = _run(boxes[None], scores[None], 'linear', 0.05)
    _check_rows(dets[0], keep[0], int(cnt[0]), ref, 'linear', 'low third')
    low = set(np.nonzero(scores < 0.05)[0].tolist())
    assert len(low) >= 32 and not (set(keep[0, :int(cnt[0])].tolist()) & low)
    ref = _reference(('all_low', 0), 'linear', 0.05)
    dets, keep, cnt = _run(ref[0][None], ref[1][None], 'linear', 0.05)
    assert int(cnt[0]) == 1 and int(keep[0, 0]) == int(np.argmax(ref[1]))
    _check_rows(dets[0], keep[0], 1, ref, 'linear', 'all low')


@pytest.mark.parametrize('max_out', [128, None])
def test_boxes_above_the_lds_box_cache(max_out):
    """K = 1500 + 96 > DET_BOX_CAP (1024): sorted boxes beyond the cache are read from the global scratch.  max_out = None
    runs every round, so candidates ranked beyond the cache are selected and decayed too (with 128 only the arg-max and
    the decay pass touch them)."""
    ref = _reference(('grid', (30, 50, 3)), 'linear', 1e-3, max_out)
    dets, keep, cnt = _run(ref[0][None], ref[1][None], 'linear', 1e-3, max_out=max_out)
    _check_rows(dets[0], keep[0], int(cnt[0]), ref, 'linear', f'grid 30x50 max_out={max_out}')
    n_cluster = int((keep[0, :int(cnt[0])] >= 1500).sum())
    assert n_cluster >= 10 and (max_out is None or int(cnt[0]) == 128)
    if max_out is None:
        rank = np.argsort(np.argsort(-ref[1], kind='stable'), kind='stable')          # initial score rank of every candidate
        assert int(cnt[0]) > 1500 and (rank[keep[0, :int(cnt[0])]] >= 1024).sum() > 400


def test_keys_in_the_global_scratch():
    """K = 128 * 128 + 96 = 16480 candidates: padn = 32768 > DET_LDS_KEYS, the keys live in the global scratch.
    max_out = 128 bounds the rounds."""
    ref = _reference(('grid', (128, 128, 3)), 'linear', 1e-3, 128)
    assert len(ref[1]) > 16384
    dets, keep, cnt = _run(ref[0][None], ref[1][None], 'linear', 1e-3, max_out=128)
    _check_rows(dets[0], keep[0], int(cnt[0]), ref, 'linear', 'grid 128x128')
    assert int(cnt[0]) == 128 and int((keep[0] >= 128 * 128).sum()) >= 10


def test_naive_equals_greedy_nms():
    """method='naive' zeroes what greedy NMS suppresses: same keep, count and dets bytes as kernels.nms at the same
    threshold (the guard keeps every IoU away from the threshold, so '>=' and '>' agree)."""
    import yunet_amd.kernels as K
    sets = [S.cluster_fixture(seed) for seed in (0, 1, 2)]
    for n in range(3):
        _reference(('cluster', (n, 96)), 'naive', 1e-3)            # asserts the guard
    b = torch.from_numpy(np.stack([x for x, _ in sets])).to(DEV)
    s = torch.from_numpy(np.stack([x for _, x in sets])).to(DEV)
    d0, k0, c0 = K.nms(b, s, IOU_THR)
    d1, k1, c1 = K.soft_nms(b, s, IOU_THR, SIGMA, 1e-3, 'naive')
    torch.cuda.synchronize()
    assert torch.equal(c0, c1)
    for n in range(3):
        m = int(c0[n])
        assert 5 <= m <= 9
        assert torch.equal(k0[n, :m], k1[n, :m]) and d0[n, :m].cpu().numpy().tobytes() == d1[n, :m].cpu().numpy().tobytes()


# ---- the fused path: head outputs -> yunet_detect_soft ------------------------------------------------------------------
H, W, STRIDES = 64, 96, [8, 16, 32]
SIZES = [(8, 12), (4, 6), (2, 3)]
SCORE_THR = 0.02


def fused_case(seed, n=2):
    """flat [n, 126, 16] whose decoded boxes are exact on both sides (dw = dh = 0: width = height = stride; centre offsets
    in 1/8 strides) and overlap in clusters: the priors of every 3 x 3 block of a level are pulled 3/4 of a stride towards
    the block's centre, +- 1/8 of jitter.  Scores are a shuffled geometric ladder: 60 priors from 0.9 down to 0.03 (above
    score_thr), the rest at 0.005."""
    g = torch.Generator().manual_seed(seed)
    P = sum(h * w for h, w in SIZES)
    flat = torch.zeros(n, P, 16)
    pull = torch.cat([torch.stack([-(torch.arange(w).repeat(h) % 3 - 1) * 0.75,
                                   -(torch.arange(h).repeat_interleave(w) % 3 - 1) * 0.75], -1) for h, w in SIZES])
    flat[..., 1:3] = pull + torch.randint(-1, 2, (n, P, 2), generator=g).float() / 8.0
    flat[..., 6:16] = torch.randint(-16, 17, (n, P, 10), generator=g).float() / 8.0
    ladder = 0.9 * (0.03 / 0.9) ** (torch.arange(60).float() / 59)
    target = torch.full((n, P), 0.005)
    for i in range(n):
        target[i, torch.randperm(P, generator=g)[:60]] = ladder[torch.randperm(60, generator=g)]
    obj = torch.full((n, P), 9.0)
    flat[..., 0] = torch.logit(target / torch.sigmoid(obj))
    flat[..., 5] = obj
    return flat


def fused_reference(flat, method, min_score):
    """The restatement on the oracle's decode: per image (keep -> prior index, fp32 scores, boxes, landmarks)."""
    import yunet_oracle as O
    priors = O.grid_priors(SIZES, STRIDES)
    boxes = O.bbox_decode(priors, flat[..., 1:5]).numpy()
    scores = (flat[..., 0].sigmoid() * flat[..., 5].sigmoid()).numpy()
    out = []
    for i in range(flat.shape[0]):
        g = S.Guard()
        k64, _ = S.soft_nms_live(boxes[i], scores[i], IOU_THR, SIGMA, min_score, method, score_thr=SCORE_THR,
                                 dtype=np.float64, guard=g)
        assert g.ok(1e-4), f'broken fused fixture, image {i}: {g}'
        assert abs(scores[i] - SCORE_THR).min() > 1e-3
        k, s = S.soft_nms_live(boxes[i], scores[i], IOU_THR, SIGMA, min_score, method, score_thr=SCORE_THR)
        assert np.array_equal(k, k64)
        pr = priors[k]
        q = flat[i, k, 6:16]
        kd = torch.cat([q[:, 2 * t:2 * t + 2] * pr[:, 2:] + pr[:, :2] for t in range(5)], -1).numpy()
        out.append((k, s, boxes[i][k], kd, int((scores[i] >= SCORE_THR).sum())))
    return out


def test_fused_detect_soft():
    """yunet_detect_soft on crafted head outputs: selection, boxes and the landmark rows of the selected priors equal the
    restatement on the oracle's decode; count is checked, rows at and beyond it are ignored.
    Scores pass through two sigmoids on each side (expf within 1 ulp = 2 u, the add and the divide: 4 u each; their product
    9 u; both sides 18 u) and then through the same weights (the boxes are exact, so nms_iou agrees bit for bit), each
    multiply rounding once per side: row r is within (18 + 2 r) u."""
    import yunet_amd.kernels as K
    flat = fused_case(1)
    ref = fused_reference(flat, 'linear', 0.05)               # 38 and 37 of the 60 candidates survive, a dozen of them decayed
    dets, kps, cnt = K.detect(flat.to(DEV), SIZES, STRIDES, SCORE_THR, soft=dict(iou_thr=IOU_THR, sigma=SIGMA, min_score=0.05,
                                                                                method='linear'))
    torch.cuda.synchronize()
    dets, kps, cnt = dets.cpu().numpy(), kps.cpu().numpy(), cnt.cpu().numpy()
    for i, (k, s, b, kd, ncand) in enumerate(ref):
        c = int(cnt[i])
        assert ncand == 60 and c == len(k) and 20 <= c < ncand, (i, c, len(k), ncand)
        assert np.array_equal(dets[i, :c, :4], b), f'image {i}: boxes / order'
        assert np.array_equal(kps[i, :c], kd), f'image {i}: landmarks of the selected priors'
        rel = np.abs(dets[i, :c, 4].astype(np.float64) - s) / s
        assert np.all(rel <= (18 + 2 * np.arange(c)) * U), (i, float(rel.max()))


# ---- the Python surface ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_and_views():
    import os
    import yunet_amd
    import yunet_amd.synthetic as Y
    sd = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'yunet_n_synth_trained.pth'),
                    map_location='cpu', weights_only=False)['state_dict']
    cfg = yunet_amd.Config.fromfile('configs/yunet_n.py')
    model = yunet_amd.build_detector(cfg.model)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    img = Y.make_batch(1, H, W, 31, structured=True)['img'].to(DEV).contiguous()
    meta = dict(img_shape=(H, W, 3), scale_factor=np.ones(4, np.float32), flip=False, flip_direction='horizontal')
    flipped = dict(meta, flip=True)
    return model, img, img.flip(-1).contiguous(), meta, flipped


SOFT_CFG = dict(type='soft_nms', iou_threshold=0.3, sigma=0.5, min_score=1e-3, method='linear')
SOFT_KW = dict(iou_thr=0.3, sigma=0.5, min_score=1e-3, method='linear')


def _union(model, views, metas, score_thr):
    """The mapped-back candidates of every view (score >= score_thr, no suppression), as YuNet.aug_test collects them."""
    import yunet_amd.kernels as K
    from yunet_amd.yunet import bbox_mapping_back
    eng = model._ensure_engine(torch.device(DEV))
    boxes, scores = [], []
    for v, m in zip(views, metas):
        flat = eng.forward_eval(v.float().contiguous())
        d, _, c = K.detect(flat, eng.plan.sizes, model.bbox_head.strides, score_thr, iou_thr=2.0, with_kps=False)
        d = d[0, :int(c[0])]
        boxes.append(bbox_mapping_back(d[:, :4], m))
        scores.append(d[:, 4])
    return torch.cat(boxes)[None].contiguous(), torch.cat(scores)[None].contiguous()


@pytest.mark.parametrize('kind', ['soft_nms', 'nms'])
def test_surface_simple_test_and_aug_test(kind, monkeypatch):
    """simple_test / aug_test with test_cfg.nms.type = 'soft_nms' equal kernels.detect(soft=...) / kernels.soft_nms on the
    same inputs; with type = 'nms' they equal calls that never mention `soft` (the parent commit's calls)."""
    import yunet_amd.kernels as K
    model, img, img_flip, meta, meta_flip = _model_and_views()
    nms_cfg = dict(SOFT_CFG) if kind == 'soft_nms' else dict(type='nms', iou_threshold=0.45)
    test_cfg = dict(model.test_cfg, nms=nms_cfg)
    monkeypatch.setattr(model, 'test_cfg', test_cfg)
    monkeypatch.setattr(model.bbox_head, 'test_cfg', test_cfg)
    thr = test_cfg['score_thr']
    eng = model._ensure_engine(torch.device(DEV))
    flat = eng.forward_eval(img)
    assert [tuple(s) for s in eng.plan.sizes] == SIZES
    if kind == 'soft_nms':
        d, k, c = K.detect(flat, eng.plan.sizes, model.bbox_head.strides, thr, max_out=-1, soft=SOFT_KW)
    else:
        d, k, c = K.detect(flat, eng.plan.sizes, model.bbox_head.strides, thr, 0.45, -1)
    res, lmk = model.simple_test(img, [meta], with_landmarks=True)
    c = int(c[0])
    assert c >= 1 and res[0][0].tobytes() == d[0, :c].cpu().numpy().tobytes()
    assert lmk[0].tobytes() == k[0, :c].cpu().numpy().tobytes()
    boxes, scores = _union(model, [img, img_flip], [meta, meta_flip], thr)
    assert boxes.shape[1] >= 2
    if kind == 'soft_nms':
        d, _, c = K.soft_nms(boxes, scores, max_out=-1, **SOFT_KW)
    else:
        d, _, c = K.nms(boxes, scores, 0.45, max_out=-1)
    out = model.forward_test([img, img_flip], [[meta], [meta_flip]])[0][0]
    assert out.tobytes() == d[0, :int(c[0])].cpu().numpy().tobytes()
    if kind == 'soft_nms':
        # Soft-NMS keeps decayed neighbours that greedy NMS deletes: never fewer rows than the greedy merge
        _, _, c_greedy = K.nms(boxes, scores, 0.3, max_out=-1)
        assert int(c[0]) >= int(c_greedy[0])
