"""-m gpu: RandomAffine with landmarks in the device train pipeline (csrc/augment.hip aug_affine_decide_kernel /
aug_affine_pixels_kernel through yunet_aug_affine_decide / yunet_aug_affine_pixels and DevicePipeline) against the
fixture made by the unmodified reference class and the float64 restatement (tests/affine_ref.py).

Draws, survivor sets, order, counts and cleared rows are compared exactly; matrix, boxes and keypoints within the bars
recorded in the fixture (twice the reference's own float32 distance from the float64 evaluation); drawn pixels within
the recorded pixel bar (four times the float32 restatement's distance from the float64 one); hand-made warps exactly."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import affine_ref as R
from test_affine import AFF, BASE, CUT, MOSAIC, PMD, cases, golden
from test_cutout_gpu import batch_of, sources

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = dict(AFF, max_rotate_degree=0.0, max_translate_ratio=0.0, scaling_ratio_range=(1.0, 1.0), max_shear_degree=0.0)
STRONG = dict(AFF, max_rotate_degree=30.0, max_translate_ratio=0.2, border_val=(3.0, 114.0, 250.5))
HOLES = dict(CUT, fill_in=(1.0, 2.0, 3.0))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_decide(cfg, seed, iteration, boxes, kps, counts, edge, params=None):
    """yunet_aug_affine_decide on padded GT (numpy) -> (out boxes, out kps, out counts, table) on the host; the outputs
    start as -7 so that every row the kernel has to clear shows."""
    import yunet_amd._lib as L
    from yunet_amd.pipelines import RandomAffine
    n, gmax = boxes.shape[:2]
    c = RandomAffine(use_kps=True, **cfg).c_cfg(seed, gmax)
    ib, ik = torch.from_numpy(boxes).to(DEV), torch.from_numpy(kps.reshape(n, gmax, 15)).to(DEV)
    ic = torch.from_numpy(counts).to(DEV)
    ob, ok = torch.full_like(ib, -7.0), torch.full_like(ik, -7.0)
    oc = torch.full_like(ic, -7)
    table = torch.full((n, L.AFFINE_WORDS), -7.0, dtype=torch.float64, device=DEV)
    rc = L.load().yunet_aug_affine_decide(C.byref(c), iteration, n, edge, _p(params), _p(ib), _p(ik), _p(ic), _p(ob), _p(ok),
                                          _p(oc), _p(table), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(ib.cpu(), torch.from_numpy(boxes)) and torch.equal(ic.cpu(), torch.from_numpy(counts))
    return ob.cpu().numpy(), ok.cpu().numpy().reshape(n, gmax, 5, 3), oc.cpu().numpy(), table


def run_pixels(table, border_val, img, params=None):
    import yunet_amd._lib as L
    out = torch.full_like(img, -7.0)
    rc = L.load().yunet_aug_affine_pixels(_p(table), C.byref((C.c_float * 3)(*border_val)), img.shape[0], img.shape[-1],
                                          _p(params), _p(img), _p(out), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out


# ------------------------------------------------------------------ the decide entry against the fixture
@pytest.mark.parametrize('name,edge', cases())
def test_decide_against_the_reference_fixture(name, edge):
    g, cfg = golden(), R.CONFIGS[name]
    it = int(g[f'it_{name}_{edge}'])
    boxes, kps, counts = g[f'boxes_{edge}'], g[f'kps_{edge}'], g[f'counts_{edge}']
    bar_m, bar_g = float(g[f'bar_matrix_{edge}']), float(g[f'bar_gt_{edge}'])
    ob, ok, oc, table = run_decide(cfg, R.SEED, it, boxes, kps, counts, edge)
    t = table.cpu().numpy()
    assert t[:, R.DRAWS:R.DRAWS + 6].tobytes() == g[f'draws_{name}_{edge}'].tobytes(), 'draws'
    worst = [0.0, 0.0, 0.0, 0.0]
    for i in range(R.N_IMAGES):
        c = int(counts[i])
        valid = g[f'valid_{name}_{edge}'][i, :c]
        r = R.decide(R.SEED, it, i, boxes[i, :c], kps[i, :c], edge, cfg, np.float64)
        M = t[i, R.MAT:R.MAT + 9].reshape(3, 3)
        assert np.array_equal(M, M.astype(np.float32).astype(np.float64)) and np.array_equal(M[2], [0, 0, 1])
        worst[0] = max(worst[0], np.abs(M - r['M']).max())
        worst[1] = max(worst[1], np.abs(M - g[f'M_{name}_{edge}'][i]).max())
        assert np.allclose(t[i, R.INV:R.INV + 6], R.inverse(M), rtol=1e-12, atol=1e-12)
        k = int(valid.sum())
        assert oc[i] == k and (t[i, R.ROWS_IN], t[i, R.ROWS_OUT], t[i, R.EDGE]) == (c, k, edge), f'image {i}: counts'
        assert not ob[i, k:].any() and not ok[i, k:].any(), f'image {i}: rows at and beyond the count are 0'
        if k:       # survivors in order: row j of the output is the j-th valid row of the input
            worst[2] = max(worst[2], np.abs(ob[i, :k] - r['wb'][valid]).max())
            worst[3] = max(worst[3], np.abs(ok[i, :k, :, :2] - r['kps'][valid][:, :, :2]).max())
            assert np.array_equal(ok[i, :k, :, 2], kps[i, :c][valid][:, :, 2]), f'image {i}: the third value is untouched'
            assert np.abs(ob[i, :k] - r['wb'][valid]).max() <= bar_g, f'image {i}: boxes, survivors or their order'
            assert np.abs(ok[i, :k, :, :2] - r['kps'][valid][:, :, :2]).max() <= bar_g, f'image {i}: keypoints'
    print(f'{name} edge {edge}: |M - M64| {worst[0]:.3e} (bar {bar_m:.3e}), |M - M_ref| {worst[1]:.3e}, '
          f'boxes {worst[2]:.3e} keypoints {worst[3]:.3e} (bar {bar_g:.3e})')
    assert worst[0] <= bar_m


def test_decide_compacts_more_rows_than_a_wave_in_order():
    """200 rows (four steps of the 64-lane loop), every third one far outside: the survivors keep their order across the
    steps, rows beyond the count are cleared, and a count above gmax is clamped."""
    gmax, edge = 200, 64
    rng = np.random.default_rng(3)
    boxes = np.zeros((2, gmax, 4), np.float32)
    xy = rng.uniform(8, 40, (2, gmax, 2))
    boxes[:, :, :2], boxes[:, :, 2:] = xy, xy + rng.uniform(3, 12, (2, gmax, 2))
    boxes[:, ::3] += 500.0
    kps = np.zeros((2, gmax, 5, 3), np.float32)
    kps[:, :, :, 0], kps[:, :, :, 1] = boxes[:, :, None, 0] + 1, boxes[:, :, None, 1] + 1
    kps[:, :, :, 2] = np.arange(gmax, dtype=np.float32)[None, :, None]        # the row number rides along
    counts = np.array([gmax + 50, 130], np.int32)
    cfg = dict(max_rotate_degree=0.0, max_translate_ratio=0.0, scaling_ratio_range=(1.0, 1.0), max_shear_degree=0.0)
    ob, ok, oc, table = run_decide(cfg, 1, 0, boxes, kps, counts, edge)
    for i, c in enumerate((gmax, 130)):
        keep = [j for j in range(c) if j % 3]
        assert oc[i] == len(keep) and ok[i, :len(keep), 0, 2].tolist() == keep
        assert np.array_equal(ob[i, :len(keep)], boxes[i, keep]) and not ob[i, len(keep):].any() and not ok[i, len(keep):].any()
    assert table[:, R.ROWS_IN].tolist() == [gmax, 130]


# ------------------------------------------------------------------ the pixel entry
def test_hand_made_tables_warp_exactly():
    import yunet_amd._lib as L
    E, bv = 32, (3.0, 114.0, 250.5)
    img = torch.from_numpy(R.pattern(6, E)).to(DEV)
    inv = [[1, 0, -3, 0, 1, 2],             # M shifts by (+3, -2)
           [0, -1, E - 1, 1, 0, 0],         # a quarter turn about the centre: torch.rot90
           [1, 0, 0.5, 0, 1, 0],            # half a pixel: the average of the two neighbours
           [1, 0, 1000, 0, 1, 0],           # every tap outside
           [1, 0, -E, 0, 1, 1e30],          # outside on the left by exactly one image, y beyond any int
           [1, 0, 0, 0, 1, 0]]              # the identity
    table = torch.zeros(6, L.AFFINE_WORDS, dtype=torch.float64)
    table[:, L.AFFINE_INV:L.AFFINE_INV + 6] = torch.tensor(inv, dtype=torch.float64)
    out = run_pixels(table.to(DEV), bv, img)
    border = torch.tensor(bv, device=DEV).reshape(3, 1, 1).expand(3, E, E)
    want = border.clone()
    want[:, :E - 2, 3:] = img[0, :, 2:, :E - 3]
    assert torch.equal(out[0], want), 'integer translation'
    assert torch.equal(out[1], torch.rot90(img[1], 1, (1, 2))), 'quarter turn'
    right = torch.cat([img[2, :, :, 1:], border[:, :, :1]], 2)
    assert torch.equal(out[2], 0.5 * img[2] + 0.5 * right), 'half-pixel shift'
    assert torch.equal(out[3], border) and torch.equal(out[4], border), 'all taps outside'
    assert torch.equal(out[5], img[5]), 'identity'


@pytest.mark.parametrize('edge', R.EDGES)
def test_drawn_matrices_against_the_float64_restatement(edge):
    g = golden()
    bar = float(g[f'bar_pixels_{edge}'])
    boxes, kps, counts = g[f'boxes_{edge}'], g[f'kps_{edge}'], g[f'counts_{edge}']
    imgs = R.pattern(R.N_IMAGES, edge)
    dimg = torch.from_numpy(imgs).to(DEV)
    worst = 0.0
    for name, cfg in R.CONFIGS.items():
        bv = R.full(cfg)['border_val']
        _, _, _, table = run_decide(cfg, R.SEED, int(g[f'it_{name}_{edge}']), boxes, kps, counts, edge)
        out = run_pixels(table, bv, dimg).cpu().numpy()
        t = table.cpu().numpy()
        for i in range(R.N_IMAGES):
            want = R.warp_pixels(imgs[i], t[i, R.INV:R.INV + 6], bv, np.float64)
            d = float(np.abs(out[i] - want).max())
            worst = max(worst, d)
            assert d <= bar, f'{name} image {i}: {d:.3e} > {bar:.3e}'
    print(f'edge {edge}: pixels within {worst:.3e} of the float64 restatement (bar {bar:.3e})')


def test_canvas_reads_each_images_edge_from_params():
    """A 64 x 64 canvas whose images have S_n in {32, 64}: the translation scales with S_n, the warp stays inside the
    S_n corner and the rest of the canvas is 0."""
    g, cfg, sizes, it = golden(), R.CONFIGS['translate'], [32, 64, 64, 32], 9
    boxes, kps, counts = R.inputs(64)
    canvas = np.zeros((4, 3, 64, 64), np.float32)
    for n, s in enumerate(sizes):
        canvas[n, :, :s, :s] = R.pattern(4, s)[n]
    params = torch.zeros(4, 8, dtype=torch.int32)
    params[:, 7] = torch.tensor(sizes, dtype=torch.int32)
    params = params.to(DEV)
    ob, ok, oc, table = run_decide(cfg, 5, it, boxes, kps, counts, 64, params=params)
    out = run_pixels(table, (114.0, 114.0, 114.0), torch.from_numpy(canvas).to(DEV), params=params).cpu().numpy()
    t = table.cpu().numpy()
    for n, s in enumerate(sizes):
        d = R.draws(5, it, n, cfg)
        assert t[n, R.DRAWS:R.DRAWS + 6].tobytes() == d.tobytes() and t[n, R.EDGE] == s
        assert np.abs(t[n, R.MAT:R.MAT + 9].reshape(3, 3) - R.matrix(d, s, np.float64)).max() <= float(g[f'bar_matrix_{s}'])
        want = R.warp_pixels(canvas[n], t[n, R.INV:R.INV + 6], (114, 114, 114), np.float64, S=s)
        assert np.abs(out[n] - want).max() <= float(g[f'bar_pixels_{s}']), f'image {n} (S_n = {s})'
        assert not out[n, :, s:, :].any() and not out[n, :, :, s:].any()
        assert ob[n, :oc[n]].max(initial=0) <= s and ok[n, :oc[n], :, :2].max(initial=0) <= s
        assert (out[n, :, :s, :s] == 114).any()


# ------------------------------------------------------------------ the whole pipeline
def pipeline_list(S, affine=None, cutout=None, photo=False, mosaic=False, resize=None):
    lst = [dict(p) for p in BASE]
    lst[3] = dict(type='Resize', keep_ratio=False, **(resize or dict(img_scale=(S, S))))
    tail = ([dict(PMD)] if photo else []) + ([dict(affine)] if affine else []) + ([dict(cutout)] if cutout else [])
    lst[5:5] = tail
    if mosaic:
        lst.insert(2, dict(MOSAIC, img_scale=(S, S)))
    return lst


FEEDS = {'fixed 32': dict(S=32), 'fixed 64': dict(S=64),
         'square_range': dict(S=64, resize=dict(img_scale=(32, 64), multiscale_mode='square_range')),
         'square_range, mixed': dict(S=96, resize=dict(img_scale=(32, 96), multiscale_mode='square_range')),
         'mosaic': dict(S=64, mosaic=True), 'post photometric': dict(S=64, photo=True),
         'cutout behind': dict(S=64, cutout=HOLES),
         'all': dict(S=64, photo=True, mosaic=True, cutout=HOLES)}


@pytest.mark.parametrize('feed', list(FEEDS))
def test_identity_configuration_changes_no_byte(feed):
    from yunet_amd.pipelines import DevicePipeline
    kw, srcs = FEEDS[feed], sources()
    pa = DevicePipeline(pipeline_list(affine=IDENTITY, **kw), seed=7, gmax=8)
    pp = DevicePipeline(pipeline_list(**kw), seed=7, gmax=8)
    seen = set()
    for it in (0, 5):
        a, b = pa(batch_of(srcs), it), pp(batch_of(srcs), it)
        torch.cuda.synchronize()
        assert pa.check() == pp.check() and pp.affine_table is None
        assert a['img'].cpu().numpy().tobytes() == b['img'].cpu().numpy().tobytes()
        for key in ('gt_bboxes', 'gt_keypointss'):
            assert a[key].padded.cpu().numpy().tobytes() == b[key].padded.cpu().numpy().tobytes()
            assert torch.equal(a[key].counts, b[key].counts) and a[key].padded.shape[1] == pa.gmax
        assert a['img_metas'] == b['img_metas']
        t = pa.affine_table.cpu().numpy()
        eye = np.eye(3).reshape(-1)
        assert (np.abs(t[:, R.MAT:R.MAT + 9]) == eye).all() and (np.abs(t[:, R.INV:R.INV + 6]) == eye[:6]).all()
        assert np.array_equal(t[:, R.ROWS_OUT], a['gt_bboxes'].counts.cpu().numpy())
        if 'resize' in kw:
            assert np.array_equal(t[:, R.EDGE], pa.sizes) and a['img'].shape[-1] == pa.sizes.max()
            seen |= set(pa.sizes.tolist())
            img = a['img'].cpu().numpy()
            for n, s in enumerate(pa.sizes):
                assert not img[n, :, s:, :].any() and not img[n, :, :, s:].any()
        if 'cutout' in kw:
            assert pa.cutout_holes.cpu().numpy().tobytes() == pp.cutout_holes.cpu().numpy().tobytes()
            assert int(pa.cutout_holes[:, 0].sum()) > 0
    assert 'mixed' not in feed or len(seen) > 1, 'images smaller than the canvas: the border that has to stay 0'


def test_step_leaves_the_other_draws_alone_and_repeats():
    """A non-trivial configuration between a POST PhotoMetricDistortion and CutOut, under Mosaic: windows, flips,
    photometric table, mosaic geometry and CutOut holes are byte-equal to the run without the step; the images differ;
    the same (seed, iteration) gives the same bytes, another iteration another table; the table is the restated one."""
    from yunet_amd.pipelines import DevicePipeline
    g = golden()
    srcs, S, seed = sources(), 64, 11
    kw = dict(S=S, photo=True, mosaic=True, cutout=HOLES)
    pa = DevicePipeline(pipeline_list(affine=STRONG, **kw), seed=seed, gmax=8)
    pp = DevicePipeline(pipeline_list(**kw), seed=seed, gmax=8)
    tables = []
    for it in (1, 2):
        a, b = pa(batch_of(srcs), it), pp(batch_of(srcs), it)
        t = pa.affine_table.clone()
        again = pa(batch_of(srcs), it)
        torch.cuda.synchronize()
        for name in ('params', 'pparams', 'geom', 'cutout_holes'):
            assert getattr(pa, name).cpu().numpy().tobytes() == getattr(pp, name).cpu().numpy().tobytes(), name
        assert not torch.equal(a['img'], b['img'])
        assert torch.equal(a['img'], again['img']) and torch.equal(t, pa.affine_table)
        for key in ('gt_bboxes', 'gt_keypointss'):
            assert torch.equal(a[key].padded, again[key].padded) and torch.equal(a[key].counts, again[key].counts)
        t = t.cpu().numpy()
        cfg = {k: v for k, v in STRONG.items() if k not in ('type', 'use_kps')}
        for n in range(len(srcs)):
            d = R.draws(seed, it, n, cfg)
            assert t[n, R.DRAWS:R.DRAWS + 6].tobytes() == d.tobytes()
            assert np.abs(t[n, R.MAT:R.MAT + 9].reshape(3, 3) - R.matrix(d, S, np.float64)).max() <= float(g[f'bar_matrix_{S}'])
        # the GT the step was given is the GT of the list without it
        assert np.array_equal(t[:, R.ROWS_IN], b['gt_bboxes'].counts.cpu().numpy())
        cnt = a['gt_bboxes'].counts.cpu().numpy()
        assert np.array_equal(t[:, R.ROWS_OUT], cnt) and (cnt <= t[:, R.ROWS_IN]).all()
        gb = a['gt_bboxes'].padded.cpu().numpy()
        assert gb.min() >= 0 and gb.max() <= S and all(not gb[n, c:].any() for n, c in enumerate(cnt))
        # holes are cut into the warped image: fill_in inside the table's holes
        holes, img = pa.cutout_holes.cpu().numpy(), a['img'].cpu().numpy()
        for n in range(len(srcs)):
            for j in range(int(holes[n, 0])):
                x1, y1, x2, y2 = holes[n, 2 + 4 * j:6 + 4 * j]
                assert (img[n, :, y1:y2, x1:x2] == np.array(HOLES['fill_in'], np.float32).reshape(3, 1, 1)).all()
        tables.append(t)
    assert not np.array_equal(tables[0], tables[1])


def test_forward_train_with_an_image_that_lost_every_row():
    import yunet_amd
    from yunet_amd.optim import FusedSGD
    from yunet_amd.pipelines import DevicePipeline
    srcs = sources()
    away = dict(AFF, max_rotate_degree=0.0, max_translate_ratio=1.0, scaling_ratio_range=(1.0, 1.0), max_shear_degree=0.0)
    pipe = DevicePipeline(pipeline_list(160, affine=away), seed=2)
    batch = None
    for it in range(32):        # translations up to a whole image: soon one image's faces all leave
        batch = pipe(batch_of(srcs), it)
        cnt = batch['gt_bboxes'].counts.cpu().numpy()
        if (cnt == 0).any() and (cnt > 0).any():
            break
    else:
        pytest.fail('no batch with an emptied image in 32 iterations')
    empty = int(np.flatnonzero(cnt == 0)[0])
    assert not batch['gt_bboxes'].padded[empty].any() and not batch['gt_keypointss'].padded[empty].any()
    torch.manual_seed(0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    model = yunet_amd.build_detector(cfg.model).to(DEV).train()
    opt = FusedSGD(model, lr=1e-4, momentum=0.9, weight_decay=5e-4)
    out = model.train_step(batch, opt)
    opt.zero_grad()
    out['loss'].backward()
    opt.step()
    torch.cuda.synchronize()
    logs = {k: float(v) for k, v in out['log_vars'].items()}
    assert all(np.isfinite(v) for v in logs.values()), logs
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


# ------------------------------------------------------------------ end to end
def test_train_cli_runs_with_random_affine(tmp_path):
    spec = importlib.util.spec_from_file_location('yunet_train_tool_affine', os.path.join(ROOT, 'tools', 'train.py'))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    cfg = tmp_path / 'yunet_s_affine.py'
    cfg.write_text(open(os.path.join(ROOT, 'configs', 'yunet_s.py')).read() + '''
train_pipeline[3]['img_scale'] = (160, 160)
train_pipeline.insert(5, dict(type='RandomAffine', max_rotate_degree=20.0, use_kps=True))
train_pipeline.insert(6, dict(type='CutOut', n_holes=(0, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.2)], fill_in=(114, 114, 114)))
''')
    work = tmp_path / 'w'
    hist = T.main([str(cfg), '--work-dir', str(work), '--seed', '3', '--no-validate', '--max-iters', '3',
                   '--cfg-options', 'data.samples_per_gpu=4', 'data.train.type=SyntheticSourceImages',
                   'data.train.pool=4', 'log_config.interval=1'])
    losses = [h['loss'] for h in hist if 'loss' in h]
    assert len(losses) >= 3 and all(np.isfinite(losses)), hist
    assert 'RandomAffine' in open(work / 'yunet_s_affine.py').read()
    pipe = T.main.last_source.pipe
    assert pipe.affine is not None and pipe.cutout is not None and pipe.out_size == 160
    t = pipe.affine_table.cpu().numpy()
    assert t.shape == (4, R.WORDS) and (np.abs(t[:, R.DRAWS]) <= 20).all() and (t[:, R.EDGE] == 160).all()
    assert (t[:, R.ROWS_OUT] <= t[:, R.ROWS_IN]).all() and np.abs(t[:, R.MAT:R.MAT + 9]).max() > 0
