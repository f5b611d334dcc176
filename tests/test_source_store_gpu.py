"""-m gpu: the decoded-source store (source_store.py, csrc/source.hip) -- yunet_aug_gather against the store's contents,
yunet_aug_window_plan against its numpy restatement, the windowed pixel pass and both cached feeds bit-identical to the
plain pipeline."""
import numpy as np
import pytest
import torch

from test_pipeline_gpu import make_pipe

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _sources(seed=0):
    """10 images of mixed sizes; image 3 has one box, image 6 has 70 (> gmax 64), image 8 is larger than any window."""
    import yunet_amd.synthetic as S
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    sizes = [(120, 160), (200, 96), (64, 64), (150, 150), (97, 211), (256, 180), (180, 256), (48, 300), (333, 77),
             (128, 128)]
    counts = [3, 5, 2, 1, 8, 4, 70, 2, 6, 3]
    out = []
    for (h, w), g in zip(sizes, counts):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        b, _, k = S.make_gt(1, h, w, gen, 128)
        b, k = b[0].numpy(), k[0].numpy()
        reps = -(-g // max(1, len(b)))
        out.append((img, np.tile(b, (reps, 1))[:g].copy(), np.tile(k, (reps, 1, 1))[:g].copy()))
    return out


def _store(srcs, placement='device'):
    from yunet_amd.source_store import SourceStore
    st = SourceStore([s[0].shape[:2] for s in srcs], placement=placement, device=DEV)
    for i in np.random.default_rng(1).permutation(len(srcs)):        # stored out of order
        st.put(int(i), *srcs[i])
    return st


def _same(a, b):
    assert torch.equal(a['img'], b['img'])
    assert torch.equal(a['gt_bboxes'].padded, b['gt_bboxes'].padded)
    assert torch.equal(a['gt_bboxes'].counts, b['gt_bboxes'].counts)
    assert torch.equal(a['gt_keypointss'].padded, b['gt_keypointss'].padded)


def test_gather_equals_store_contents_and_pipeline_matches_from_lists():
    from yunet_amd.pipelines import SourceBatch
    srcs = _sources()
    st = _store(srcs)
    idx = [6, 3, 3, 0, 9, 6, 8, 1, 2, 5, 4, 7, 3]
    sb = st.batch(idx)
    torch.cuda.synchronize()
    cnt = [len(srcs[i][1]) for i in idx]
    assert sb.gt_off.cpu().tolist() == np.concatenate([[0], np.cumsum(cnt)]).tolist()
    assert sb.src_hw.cpu().numpy().tolist() == [list(srcs[i][0].shape[:2]) for i in idx]
    assert sb.src_off.cpu().numpy().tolist() == st.offsets[idx].tolist()
    assert torch.equal(sb.boxes.cpu(), torch.from_numpy(np.concatenate([srcs[i][1] for i in idx])))
    assert torch.equal(sb.kps.cpu(), torch.from_numpy(np.concatenate([srcs[i][2] for i in idx])))
    for n, i in enumerate(idx):         # the store's pixels at the gathered offsets
        o, (h, w) = int(sb.src_off[n]), srcs[i][0].shape[:2]
        assert np.array_equal(sb.src[o:o + h * w * 3].cpu().numpy(), srcs[i][0].reshape(-1))
    ref = SourceBatch.from_lists([srcs[i][0] for i in idx], [srcs[i][1] for i in idx], [srcs[i][2] for i in idx], DEV)
    for it in (0, 3):
        a, b = make_pipe(96, 5)(st.batch(idx), it), make_pipe(96, 5)(ref, it)
        torch.cuda.synchronize()
        _same(a, b)


def test_gather_large_batch():
    """N = 4096 (16 scan tiles), one stored image picked over and over with ragged neighbours."""
    srcs = _sources(2)
    st = _store(srcs)
    idx = np.random.default_rng(3).integers(0, len(srcs), 4096)
    sb = st.batch(idx)
    cnt = np.array([len(srcs[i][1]) for i in idx])
    assert sb.gt_off.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum(cnt)]).tolist()
    assert torch.equal(sb.kps.cpu(), torch.from_numpy(np.concatenate([srcs[i][2] for i in idx])))


def test_window_plan_matches_numpy_restatement():
    import ctypes as C
    import yunet_amd._lib as L
    from yunet_amd.source_store import window_plan_np
    hw = np.array([[100, 80], [50, 60], [40, 40], [90, 70], [30, 200], [64, 64]], dtype=np.int32)
    params = np.zeros((6, 8), dtype=np.int32)
    params[:, :3] = [[-10, 5, 50],       # left < 0
                     [10, -20, 45],      # top < 0
                     [-30, -25, 120],    # window larger than both sides
                     [7, 9, 0],          # cw == 0: no window found
                     [-5, -40, 45],      # wider window than the image is high
                     [64, 0, 10]]        # misses the image: empty
    rect, off = window_plan_np(params, hw)
    assert rect[0].tolist() == [5, 0, 50, 40] and rect[1].tolist() == [0, 10, 25, 45]
    assert rect[2].tolist() == [0, 0, 40, 40] and rect[3].tolist() == [0, 0, 0, 0] and rect[5].tolist() == [0] * 4
    d_params, d_hw = torch.from_numpy(params).to(DEV), torch.from_numpy(hw).to(DEV)
    d_rect = torch.full((6, 4), -7, dtype=torch.int32, device=DEV)
    d_off = torch.full((7,), -7, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    L.check(L.load().yunet_aug_window_plan(p(d_params), p(d_hw), 6, p(d_rect), p(d_off),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'plan')
    assert d_rect.cpu().numpy().tolist() == rect.tolist()
    assert d_off.cpu().numpy().tolist() == off.tolist()


def _window_buffer(src, rect, off):
    """The compact window buffer built on the device by slicing the full sources."""
    parts = []
    for n in range(src.n):
        y0, x0, rh, rw = (int(v) for v in rect[n])
        h, w = (int(v) for v in src.src_hw[n])
        o = int(src.src_off[n])
        im = src.src[o:o + h * w * 3].view(h, w, 3)
        parts.append(im[y0:y0 + rh, x0:x0 + rw].reshape(-1))
    buf = torch.cat(parts + [torch.zeros(1, dtype=torch.uint8, device=DEV)])
    assert buf.numel() - 1 == int(off[-1])
    return buf


def test_windowed_pixels_bit_identical_with_and_without_flip():
    from yunet_amd.pipelines import SourceBatch
    from yunet_amd.source_store import window_plan_np
    srcs = _sources(4)
    # an image without GT: no window (cw == 0), zero bytes, an all-pad output
    srcs.append((np.full((70, 90, 3), 9, np.uint8), np.zeros((0, 4), np.float32), np.zeros((0, 5, 3), np.float32)))
    src = SourceBatch.from_lists([s[0] for s in srcs], [s[1] for s in srcs], [s[2] for s in srcs], DEV)
    flips, neg = set(), False
    for it in range(4):
        pipe = make_pipe(64, 11)
        full = pipe(src, it)
        params, rect, off = pipe.window_plan(src, it, torch.device(DEV))
        assert torch.equal(params, pipe.params)
        r_np, o_np = window_plan_np(params.cpu().numpy(), src.src_hw.cpu().numpy())
        assert rect.cpu().numpy().tolist() == r_np.tolist() and off.cpu().numpy().tolist() == o_np.tolist()
        win = _window_buffer(src, rect.cpu(), off.cpu())
        out = pipe.windowed(src, it, win, rect, off)
        torch.cuda.synchronize()
        _same(full, out)
        pr = params.cpu().numpy()
        flips |= set(pr[pr[:, 2] > 0, 3].tolist())
        neg |= bool(((pr[:, 0] < 0) | (pr[:, 1] < 0)).any())
        assert pr[-1, 2] == 0 and rect[-1].cpu().tolist() == [0, 0, 0, 0]
        assert torch.all(out['img'][-1] == 128.0)
        assert int(off[-1]) < sum(s[0].size for s in srcs)
    assert flips == {0, 1} and neg


def test_synthetic_window_feed_equals_resident():
    import os
    import yunet_amd
    import yunet_amd.runner as R
    from yunet_amd.source_store import window_plan_np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yunet_amd.Config.fromfile(os.path.join(root, 'configs', 'yunet_s.py'))
    kw = dict(samples_per_gpu=12, pool=5, seed=3, src_hw=((300, 420), (512, 384), (200, 200)))
    a = R.SyntheticSourceImages(cfg.train_pipeline, **kw)
    b = R.SyntheticSourceImages(cfg.train_pipeline, host_fed='window', timing=True, **kw)
    totals = []
    for it in range(7):
        ba, bb = a.batch(it, DEV), b.batch(it, DEV)
        torch.cuda.synchronize()
        _same(ba, bb)
        _, off = window_plan_np(a.pipe.params.cpu().numpy(), a._src.src_hw.cpu().numpy())
        totals.append(int(off[-1]))
    rep = b.report(skip=0)
    assert rep['batches_timed'] == 7 and rep['h2d_ms'] > 0 and rep['pipeline_ms'] > 0
    assert rep['h2d_bytes'] == sum(totals) / len(totals)
    assert rep['h2d_bytes'] < rep['src_bytes'] == a._src.src.numel()


def _write_labelv2(root, n=20, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    (root / 'images').mkdir()
    lines = []
    for i in range(n):
        h, w = int(rng.integers(40, 120)), int(rng.integers(40, 120))
        arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        name = f'images/img_{i:02d}.png'
        Image.fromarray(arr).save(root / name)
        lines.append(f'# {name} {w} {h}')
        for _ in range(int(rng.integers(1, 5))):
            bw, bh = float(rng.integers(8, w // 2)), float(rng.integers(8, h // 2))
            x1, y1 = float(rng.integers(0, w - bw)), float(rng.integers(0, h - bh))
            kp = ' '.join(f'{x1 + bw * fx:.1f} {y1 + bh * fy:.1f} 0.0' for fx, fy in
                          ((.3, .3), (.7, .3), (.5, .5), (.35, .75), (.65, .75)))
            lines.append(f'{x1} {y1} {x1 + bw} {y1 + bh} {kp} 0.9')
    (root / 'labelv2.txt').write_text('\n'.join(lines) + '\n')
    return str(root / 'labelv2.txt'), str(root)


def test_retinaface_cache_bit_identical_and_decodes_once(tmp_path):
    from collections import Counter
    from yunet_amd.datasets import RetinaFaceDataset, RetinaFaceSource
    from test_pipeline_gpu import REF_PIPELINE
    ann, prefix = _write_labelv2(tmp_path)
    pipeline = [dict(p) for p in REF_PIPELINE]
    pipeline[3]['img_scale'] = (64, 64)
    srcs, calls = {}, {}
    for cache in (None, 'device', 'host'):
        ds = RetinaFaceDataset(ann, img_prefix=prefix, pipeline=pipeline)
        c = calls[cache] = Counter()
        orig = ds.load_image

        def counted(i, orig=orig, c=c):
            c[i] += 1
            return orig(i)
        ds.load_image = counted
        srcs[cache] = RetinaFaceSource(ds, pipeline, samples_per_gpu=4, seed=2, workers=2, cache=cache)
    ipe = srcs[None].iters_per_epoch
    assert ipe >= 4
    for it in range(2 * ipe):
        outs = {k: s.batch(it, DEV) for k, s in srcs.items()}
        torch.cuda.synchronize()
        _same(outs[None], outs['device'])
        _same(outs[None], outs['host'])
    n = len(srcs[None].ds)
    for cache in ('device', 'host'):
        assert set(calls[cache]) == set(range(n)) and set(calls[cache].values()) == {1}, calls[cache]
    assert sum(calls[None].values()) >= 2 * ipe * 4
