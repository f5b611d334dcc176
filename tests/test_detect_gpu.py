"""-m gpu: test-time path on the device -- eval-mode forward (BatchNorm on running statistics)
and get_bboxes (scores, threshold, decode, NMS in csrc/detect.hip) -- against fixtures from the
unmodified reference `simple_test` and against the CPU oracle.

Scores / boxes go through expf on both sides, so values are compared to 1e-5 / 1e-3 px and the
fixtures were selected with every decision (score threshold, IoU threshold, score order) at
least 2e-5 / 2e-5 / 2e-7 away from its boundary; detections are matched in score order."""
import os

import numpy as np
import pytest
import torch

import crafted as C
import detect_oracle as D
from test_detect_oracle import load_case

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def build_model(kind, sd):
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(f'configs/yunet_{kind}.py')
    model = yunet_amd.build_detector(cfg.model)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval()


def assert_same_dets(got, ref, box_atol=2e-3):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.allclose(got[:, 4], ref[:, 4], rtol=2e-5, atol=1e-7)
    assert np.allclose(got[:, :4], ref[:, :4], rtol=1e-5, atol=box_atol)


@pytest.mark.parametrize('name', ['detect_s_160.npz', 'detect_n_320.npz'])
def test_simple_test_vs_reference_fixture(name):
    g, arch, sd, img = load_case(name)
    model = build_model(str(g['kind']), sd)
    n = img.shape[0]
    metas = [dict(img_shape=img.shape[2:] + (3,), scale_factor=np.ones(4, np.float32)) for _ in range(n)]
    res, lmk = model.simple_test(img.to(DEV), metas, with_landmarks=True)
    assert len(res) == n
    flat, sizes = D.eval_flat(img, sd, arch)
    oracle = D.get_bboxes(flat, sizes, arch['strides'], 0.02, 0.45)
    for i in range(n):
        assert len(res[i]) == 1 and res[i][0].dtype == np.float32          # bbox2result, one class
        assert_same_dets(res[i][0], g[f'dets_{i}'])
        assert np.allclose(lmk[i], oracle[i][1].numpy(), rtol=1e-5, atol=2e-3)
    # forward(return_loss=False) with the mmdet list-of-one convention ends in the same place
    res2 = model(img=[img.to(DEV)], img_metas=[metas], return_loss=False)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(res, res2))
    with pytest.raises(RuntimeError, match='eval'):
        model.train().simple_test(img.to(DEV), metas)


@pytest.mark.parametrize('kind,size,n', [('s', 160, 4), ('n', 320, 2)])
def test_eval_forward_vs_oracle(kind, size, n):
    """BatchNorm on running statistics through the train-mode kernels (synthesised sums)."""
    arch, sd = D.make_state(kind, 5, size)
    img = D.structured_images(n, size, 9)
    model = build_model(kind, sd)
    eng = model._ensure_engine(torch.device(DEV))
    rm0 = eng.params.running_mean.clone()
    flat = eng.forward_eval(img.to(DEV).contiguous()).cpu()
    ref, _ = D.eval_flat(img, sd, arch)
    assert float((flat - ref).abs().max()) <= 2e-4 * max(1.0, float(ref.abs().max()))
    assert torch.equal(rm0, eng.params.running_mean), 'eval forward must not touch running statistics'


def _run_detect(flat, h, w, **kw):
    import yunet_amd.kernels as k
    dets, kps, cnt = k.detect(flat.to(DEV).contiguous(), C.featmap_sizes(h, w), [8, 16, 32], **kw)
    torch.cuda.synchronize()
    return dets.cpu(), kps.cpu(), cnt.cpu()


def _stable(flat, h, w):
    ds, di, dt = D.stability(flat, C.featmap_sizes(h, w), [8, 16, 32], 0.02, 0.45)
    return ds > 1e-5 and di > 1e-5 and dt > 1e-7


def exact_heads(n, P, seed):
    """Head outputs whose decoded boxes are exactly representable (dw = dh = 0 -> w = h = stride,
    centre offsets in 1/8 steps) and whose scores are 1e-4 apart and >= 1e-3 away from the
    threshold: every NMS decision is then bit-identical on both sides, whatever the ulp of expf."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.zeros(n, P, 16)
    flat[..., 1:3] = torch.randint(-12, 13, (n, P, 2), generator=g).float() / 8.0
    flat[..., 6:16] = torch.randint(-16, 17, (n, P, 10), generator=g).float() / 8.0
    obj = torch.full((n, P), 9.0)
    so = torch.sigmoid(obj)
    target = torch.stack([torch.randperm(P, generator=g) for _ in range(n)]).float() * 1e-4 + 0.0215
    low = torch.rand(n, P, generator=g) < 0.25                      # a quarter below the threshold
    target[low] = target[low] * 0.02 + 0.001
    target = target.clamp(max=0.97)
    flat[..., 0] = torch.logit((target / so).clamp(1e-6, 1 - 1e-6))
    flat[..., 5] = obj
    return flat


@pytest.mark.parametrize('h,w,n,seed', [pytest.param(h, h, n, seed, id=f'{h}-{n}-{seed}')
                                         for h, n, seed in [(160, 6, 1), (320, 3, 2), (640, 2, 3), (1024, 2, 4),
                                                            (1280, 1, 5)]] +
                         [(1120, 1664, 1, 6), (704, 1024, 2, 7), (160, 1024, 2, 8), (1024, 160, 2, 9)])
def test_detect_kernel_vs_oracle_exact_geometry(h, w, n, seed):
    """Thousands of candidates per image with heavy overlap (K exceeds the LDS box cache at 640):
    the survivors, their order and their boxes must be identical to the oracle's.
    1024: P = 21504 > 16384 priors (origin-size WIDER images, tools/test_widerface.py --mode 2) with
    ~16.1 k candidates -- compacted through the scratch, sorted in LDS; 1280: P = 33600 with ~25 k
    candidates -- more than the LDS holds, sorted in the global scratch.  Rectangles, the test-time geometries
    (tools/test_widerface.py): 1120 x 1664 (--mode 1, P = 38220, the largest), original sizes padded to 32 (--mode 2)
    with odd stride-32 levels, and a tall and a wide strip."""
    sizes = C.featmap_sizes(h, w)
    P = sum(a * b for a, b in sizes)
    if (h, w) == (1120, 1664):
        assert P == 38220
    flat = exact_heads(n, P, seed)
    dets, kps, cnt = _run_detect(flat, h, w)
    ref = D.get_bboxes(flat, sizes, [8, 16, 32], 0.02, 0.45)
    for i in range(n):
        c = int(cnt[i])
        assert c == len(ref[i][0]), (i, c, len(ref[i][0]))
        assert torch.equal(dets[i, :c, :4], ref[i][0][:, :4]), f'boxes / order differ (image {i})'
        assert torch.allclose(dets[i, :c, 4], ref[i][0][:, 4], rtol=2e-5, atol=1e-7)
        assert torch.equal(kps[i, :c], ref[i][1])
    cand = int(((flat[..., 0].sigmoid() * flat[..., 5].sigmoid()) >= 0.02).sum())
    assert int(cnt.sum()) < 0.95 * cand and int(cnt.max()) > 100      # some suppression (heavy: fixtures)


def test_detect_kernel_vs_oracle_random_heads():
    """Unconstrained random head outputs (boxes from 0.3x to 8x the stride) on a draw whose
    decisions are away from their thresholds."""
    h, n = 160, 6
    P = sum(a * b for a, b in C.featmap_sizes(h, h))
    g = torch.Generator().manual_seed(4)
    for attempt in range(40):
        flat = torch.randn(n, P, 16, generator=g)
        flat[..., 0] = flat[..., 0] * 2.0 - 1.5
        flat[..., 3:5] = flat[..., 3:5] * 0.7 + 0.6
        if _stable(flat, h, h):
            break
    else:
        pytest.skip('no stable random draw')
    dets, kps, cnt = _run_detect(flat, h, h)
    ref = D.get_bboxes(flat, C.featmap_sizes(h, h), [8, 16, 32], 0.02, 0.45)
    for i in range(n):
        c = int(cnt[i])
        assert c == len(ref[i][0]), (i, c, len(ref[i][0]))
        assert_same_dets(dets[i, :c].numpy(), ref[i][0].numpy())
        assert np.allclose(kps[i, :c].numpy(), ref[i][1].numpy(), rtol=1e-5, atol=2e-3)


def test_detect_edge_cases():
    h = 160
    P = sum(a * b for a, b in C.featmap_sizes(h, h))
    # nothing above the threshold -> count 0
    flat = torch.zeros(2, P, 16)
    flat[..., 0] = -10.0
    _, _, cnt = _run_detect(flat, h, h)
    assert cnt.tolist() == [0, 0]
    # identical boxes everywhere on one level: one survivor per distinct box; max_out truncates
    flat = torch.zeros(1, P, 16)
    flat[..., 0] = torch.linspace(3.0, -1.0, P)          # strictly decreasing scores
    flat[..., 5] = 4.0
    flat[..., 3:5] = 5.0                                  # huge boxes: everything overlaps
    dets, _, cnt = _run_detect(flat, h, h)
    ref = D.get_bboxes(flat, C.featmap_sizes(h, h), [8, 16, 32], 0.02, 0.45)
    assert int(cnt[0]) == len(ref[0][0])
    dets2, _, cnt2 = _run_detect(flat, h, h, max_out=3)
    assert int(cnt2[0]) == min(3, int(cnt[0]))
    assert torch.equal(dets2[0, :int(cnt2[0])], dets[0, :int(cnt2[0])])
    # a level table that does not add up to P is rejected, like any unsupported shape
    import yunet_amd.kernels as k
    from yunet_amd._lib import YunetHipError
    with pytest.raises(YunetHipError):
        k.detect(torch.zeros(1, 777, 16, device=DEV), C.featmap_sizes(160, 160), [8, 16, 32])


def test_detect_full_batch_properties():
    """BASELINE batch (256 x 320x320): survivors are sorted, pairwise IoU <= thr, every dropped
    candidate overlaps a higher-scored survivor (the defining properties of greedy NMS)."""
    h, n = 320, 256
    P = sum(a * b for a, b in C.featmap_sizes(h, h))
    flat = exact_heads(n, P, 5)
    dets, _, cnt = _run_detect(flat, h, h)
    assert int(cnt.min()) > 0
    for i in (0, 17, 255):
        c = int(cnt[i])
        d = dets[i, :c]
        assert bool((d[:-1, 4] >= d[1:, 4]).all())
        for j in range(min(c - 1, 40)):
            assert float(D.nms_iou(d[j, :4], d[j + 1:, :4]).max()) <= 0.45 + 1e-6
        ref = D.get_bboxes(flat[i:i + 1], C.featmap_sizes(h, h), [8, 16, 32], 0.02, 0.45)[0][0]
        assert torch.equal(d[:, :4], ref[:, :4])


def test_nms_kernel_vs_oracle_and_counts():
    """yunet_nms (explicit boxes + scores, the merge step of aug_test) == the oracle's greedy NMS:
    kept indices, order, boxes; per-set element counts; score threshold; max_out."""
    import yunet_amd.kernels as k
    g = torch.Generator().manual_seed(3)
    n, K = 3, 3000
    xy = torch.randint(0, 160, (n, K, 2), generator=g).float()
    wh = torch.randint(4, 40, (n, K, 2), generator=g).float()
    boxes = torch.cat([xy, xy + wh], -1).contiguous()
    scores = (torch.stack([torch.randperm(K, generator=g) for _ in range(n)]).float() + 1) / (K + 1)
    counts = torch.tensor([K, 1234, 1], dtype=torch.int32)
    dets, keep, cnt = k.nms(boxes.to(DEV), scores.to(DEV), 0.45, counts=counts.to(DEV))
    torch.cuda.synchronize()
    for i in range(n):
        c = int(counts[i])
        ref = D.nms_greedy(boxes[i, :c], scores[i, :c], 0.45)
        m = int(cnt[i])
        assert m == len(ref)
        assert torch.equal(keep[i, :m].cpu().long(), ref)
        assert torch.equal(dets[i, :m, :4].cpu(), boxes[i, ref]) and torch.equal(dets[i, :m, 4].cpu(), scores[i, ref])
    # threshold + max_out
    dets, keep, cnt = k.nms(boxes[:1].to(DEV), scores[:1].to(DEV), 0.45, score_thr=0.5, max_out=7)
    sel = torch.nonzero(scores[0] >= 0.5).squeeze(1)
    ref = sel[D.nms_greedy(boxes[0, sel], scores[0, sel], 0.45)][:7]
    assert int(cnt[0]) == 7 and torch.equal(keep[0, :7].cpu().long(), ref)
    # iou_thr >= 1: nothing suppressed, everything out in score order
    dets, keep, cnt = k.nms(boxes[:1].to(DEV), scores[:1].to(DEV), 2.0)
    assert int(cnt[0]) == K and torch.equal(keep[0].cpu().long(), torch.sort(scores[0], descending=True).indices)
    # signed scores (raw logits; score_thr defaults to -inf): the sort key is order-preserving over the whole
    # fp32 range -- raw float bits would put every negative score first, in reversed order
    signed = (scores[:1] - 0.5) * 8.0
    signed[0, 0], signed[0, 1] = float('-inf'), -0.0
    dets, keep, cnt = k.nms(boxes[:1].to(DEV), signed.to(DEV), 0.45)
    ref = D.nms_greedy(boxes[0], signed[0], 0.45)
    m = int(cnt[0])
    assert m == len(ref) and torch.equal(keep[0, :m].cpu().long(), ref)
    assert torch.equal(dets[0, :m, 4].cpu(), signed[0, ref])


def test_aug_test_single_view_twice_equals_simple_test():
    """Two identical views: the union holds every candidate twice with equal scores; one NMS over
    the union keeps the first copy and suppresses the second (IoU 1), i.e. exactly simple_test."""
    arch, sd = D.make_state('n', 5, size=160)
    model = build_model('n', sd)
    img = D.structured_images(1, 320, 9).to(DEV)
    meta = dict(img_shape=(320, 320, 3), scale_factor=[1.0, 1.0, 1.0, 1.0], flip=False, flip_direction='horizontal')
    one = model.simple_test(img, [meta])[0][0]
    two = model.forward_test([img, img], [[meta], [dict(meta)]])[0][0]
    assert one.shape[0] > 5 and np.array_equal(one, two)
    # a second view at half the resolution maps back into the same frame: boxes stay inside it
    small = torch.nn.functional.interpolate(img, scale_factor=0.5, mode='bilinear', align_corners=False)
    m2 = dict(img_shape=(160, 160, 3), scale_factor=[0.5, 0.5, 0.5, 0.5], flip=True, flip_direction='horizontal')
    both = model.forward_test([img, small.contiguous()], [[meta], [m2]], rescale=True)[0][0]
    assert both.shape[1] == 5 and both.shape[0] >= 1
    assert np.all(np.diff(both[:, 4]) <= 0), 'descending score'
    assert np.isfinite(both).all() and (both[:, 2] > both[:, 0]).all() and (both[:, 3] > both[:, 1]).all()


def test_widerface_tool_end_to_end(tmp_path):
    """tools/test_widerface.py on a synthetic dataset in the protocol's own formats (labelv2 list, image
    files, wider_*_val.mat): decode -> resize / pad -> eval forward -> get_bboxes(rescale) -> prediction
    files -> APs; --eval-only over the saved files reproduces the same APs."""
    import subprocess
    import sys
    from PIL import Image
    import wider_fixture as WF
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
    cfg = open('configs/yunet_n.py').read() + f"""
data = dict(samples_per_gpu=1, test=dict(type='RetinaFaceDataset',
            ann_file={str(tmp_path / 'labelv2' / 'val' / 'labelv2.txt')!r},
            img_prefix={str(tmp_path / 'images')!r}, pipeline=[]))
"""
    (tmp_path / 'cfg.py').write_text(cfg)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    aps = {}
    for mode in (2, 320):
        out = tmp_path / f'out{mode}'
        r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'test_widerface.py'), str(tmp_path / 'cfg.py'),
                            str(tmp_path / 'ck.pth'), '--out', str(out), '--save-preds', '--mode', str(mode), '--thr', '0.3'],
                           capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-1500:]
        aps[mode] = [float(v) for v in open(out / 'aps').read().strip().split(',')]
        assert len(aps[mode]) == 3 and all(0.0 <= v <= 1.0 for v in aps[mode])
        assert sum(len(os.listdir(out / e['name'])) for e in events) == 6
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'test_widerface.py'), str(tmp_path / 'cfg.py'),
                        '--eval-only', str(tmp_path / 'out2'), '--out', str(tmp_path / 'again')],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-1500:]
    again = [float(v) for v in open(tmp_path / 'again' / 'aps').read().strip().split(',')]
    assert again == pytest.approx(aps[2], abs=2e-4)          # text files keep 5 decimals


def test_eval_hook_runs_during_training(tmp_path):
    """train_detector(validate=True) with `evaluation = dict(interval=1, metric='mAP')`: after every epoch the
    EvalHook runs the eval-mode detector over the validation list (device test pipeline + get_bboxes), calls
    dataset.evaluate and logs AP50 / mAP; training continues in train mode afterwards.  A detector trained for a
    couple of thousand iterations on the structured synthetic faces (the bench fixture) scores a non-trivial AP
    on images painted the same way."""
    from PIL import Image
    import yunet_amd
    import yunet_amd.runner as R
    import yunet_amd.synthetic as S
    sd = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'yunet_n_synth_trained.pth'),
                    map_location='cpu', weights_only=False)['state_dict']        # 2000 SGD iterations on such faces
    b = S.make_batch(6, 320, 320, 31, structured=True)
    os.makedirs(tmp_path / 'img')
    lines = []
    for i in range(6):
        arr = b['img'][i].permute(1, 2, 0).clamp(0, 255).byte().numpy()           # BGR planes -> HWC
        Image.fromarray(arr[:, :, ::-1].copy()).save(tmp_path / 'img' / f'{i}.png')
        lines.append(f'# {i}.png 320 320')
        for box in b['gt_bboxes'][i]:
            lines.append('%.2f %.2f %.2f %.2f' % tuple(float(v) for v in box))
    (tmp_path / 'val.txt').write_text('\n'.join(lines) + '\n')
    cfg = yunet_amd.Config.fromfile('configs/yunet_n.py')
    cfg.merge_from_dict(dict(
        data=dict(samples_per_gpu=8, val=dict(type='RetinaFaceDataset', ann_file=str(tmp_path / 'val.txt'),
                                              img_prefix=str(tmp_path / 'img'),
                                              pipeline=[dict(type='MultiScaleFlipAug', img_scale=(320, 320), flip=False, transforms=[])])),
        evaluation=dict(interval=1, metric='mAP'), runner=dict(type='EpochBasedRunner', max_epochs=2),
        checkpoint_config=None, work_dir=str(tmp_path / 'work'),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')])))
    cfg.optimizer['lr'] = 1e-5
    model = yunet_amd.build_detector(cfg.model)
    model.load_state_dict(sd, strict=True)
    src = R.SyntheticWiderFace((160, 160), 8, iters_per_epoch=2)
    lines_out = []
    hist = R.train_detector(model, src, cfg, validate=True, device='cuda', log=lines_out.append)
    val = [h for h in hist if h.get('mode') == 'val']
    assert [v['epoch'] for v in val] == [1, 2] and all(set(v) >= {'AP50', 'mAP'} for v in val)
    assert all(0.0 <= v['mAP'] <= 1.0 for v in val) and val[0]['mAP'] > 0.2, val
    assert any(l.startswith('Epoch(val) [1][6]') for l in lines_out)
    assert model.training and len([h for h in hist if h.get('mode') != 'val']) == 4
