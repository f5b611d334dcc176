"""-m gpu: CutOut in the device train pipeline (csrc/augment.hip aug_cutout_kernel through yunet_aug_cutout and
DevicePipeline) against the fixture made by the unmodified reference class and the pure-Python restatement
(tests/cutout_ref.py).  Every comparison is of integers or bytes."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import cutout_ref as R
import pipeline_oracle as P
from test_cutout import BASE, CUT, MOSAIC, PMD, cases, golden
from test_source_store_gpu import _window_buffer

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8
FILL = (3.0, 114.0, 250.5)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(cfg, seed, iteration, img, params=None, n=None, edge=None):
    """yunet_aug_cutout in place on img [N, 3, E, E] -> (status, table int32 [N, WORDS] on the host)."""
    import yunet_amd._lib as L
    from yunet_amd.pipelines import CutOut
    c = cfg if isinstance(cfg, L.YunetCutoutCfg) else CutOut(**cfg).c_cfg(seed)
    holes = torch.full((img.shape[0], L.CUTOUT_WORDS), -7, dtype=torch.int32, device=DEV)
    rc = L.load().yunet_aug_cutout(C.byref(c), iteration, img.shape[0] if n is None else n,
                                   img.shape[-1] if edge is None else edge, _p(params), _p(img), _p(holes), _stream())
    torch.cuda.synchronize()
    return rc, holes.cpu().numpy()


# ------------------------------------------------------------------ the entry point alone
@pytest.mark.parametrize('name,edge,iteration', cases())
def test_fixed_size_tensor_equals_the_reference_fixture(name, edge, iteration):
    """E = 32 / 64 / 96, every image's edge E: table and pixels are the reference's, byte for byte."""
    g = golden()
    img = torch.from_numpy(g[f'in_{edge}']).to(DEV)
    rc, table = launch(R.CONFIGS[name], R.SEED, iteration, img)
    assert rc == 0
    assert np.array_equal(table, g[f'holes_{name}_{edge}'])
    assert img.cpu().numpy().tobytes() == g[f'out_{name}_{edge}'].tobytes()


@pytest.mark.parametrize('name', list(R.CONFIGS))
def test_canvas_reads_each_images_edge_from_params(name):
    """A 96 x 96 canvas whose images have S_n in {32, 64, 96} (params[:, 7]): image n's table is that of an S_n image, the
    pixels inside its holes are fill_in, every other value -- the zero border included -- is unchanged."""
    cfg = R.CONFIGS[name]
    fill = R.normalise(cfg)[4]
    sizes = [32, 64, 96, 96, 64, 32, 32, 96]
    canvas = np.zeros((N, 3, 96, 96), np.float32)
    for n, s in enumerate(sizes):
        canvas[n, :, :s, :s] = R.pattern(N, s)[n]
    params = torch.zeros(N, 8, dtype=torch.int32)
    params[:, 7] = torch.tensor(sizes, dtype=torch.int32)
    img = torch.from_numpy(canvas).to(DEV)
    rc, table = launch(cfg, 31, 6, img, params=params.to(DEV))
    assert rc == 0
    got = img.cpu().numpy()
    for n, s in enumerate(sizes):
        row = R.holes(31, 6, n, s, s, cfg)
        assert np.array_equal(table[n], row), f'image {n} (S_n = {s})'
        assert got[n].tobytes() == R.fill(canvas[n], row, fill).tobytes(), f'image {n} (S_n = {s})'
        assert not got[n, :, s:, :].any() and not got[n, :, :, s:].any()
        assert row[2:].reshape(-1, 4).max(initial=0) <= s


def test_entry_point_refuses_before_any_launch():
    import yunet_amd._lib as L
    from yunet_amd.pipelines import CutOut
    img = torch.full((4, 3, 32, 32), 9.0, device=DEV)
    good = dict(n_holes=(1, 3), cutout_ratio=[(0.5, 0.5), (0.25, 0.25)], fill_in=1)

    def cfg(**fields):
        c = CutOut(**good).c_cfg(0)
        for k, v in fields.items():
            if k == 'cand':
                c.cand[1][0] = v
            elif k == 'fill':
                c.fill[2] = v
            else:
                setattr(c, k, v)
        return c
    bad = {'n_lo > n_hi': cfg(n_lo=4), 'n_lo < 0': cfg(n_lo=-1), 'too many holes': cfg(n_hi=L.CUTOUT_MAX_HOLES + 1),
           'no candidate': cfg(n_cand=0), 'too many candidates': cfg(n_cand=L.CUTOUT_MAX_CANDIDATES + 1),
           'negative candidate': cfg(cand=-0.5), 'nan candidate': cfg(cand=float('nan')),
           'inf candidate': cfg(cand=float('inf')), 'nan fill': cfg(fill=float('nan'))}
    for what, c in bad.items():
        rc, table = launch(c, 0, 0, img)
        assert rc == L.EINVAL and (table == -7).all(), what
    for what, kw in {'N = 0': dict(n=0), 'N < 0': dict(n=-3), 'E = 0': dict(edge=0),
                     'E too large': dict(edge=L.AUG_MAX_EDGE + 1)}.items():
        rc, table = launch(cfg(), 0, 0, img, **kw)
        assert rc == L.EINVAL and (table == -7).all(), what
    lib = L.load()
    holes = torch.zeros(4, L.CUTOUT_WORDS, dtype=torch.int32, device=DEV)
    c = cfg()
    assert lib.yunet_aug_cutout(None, 0, 4, 32, None, _p(img), _p(holes), _stream()) == L.EINVAL
    assert lib.yunet_aug_cutout(C.byref(c), 0, 4, 32, None, None, _p(holes), _stream()) == L.EINVAL
    assert lib.yunet_aug_cutout(C.byref(c), 0, 4, 32, None, _p(img), None, _stream()) == L.EINVAL
    torch.cuda.synchronize()
    assert bool((img == 9.0).all()) and not holes.any()
    with pytest.raises(L.YunetHipError, match='yunet_aug_cutout'):
        L.check(lib.yunet_aug_cutout(C.byref(cfg(n_lo=4)), 0, 4, 32, None, _p(img), _p(holes), _stream()),
                'yunet_aug_cutout')
    rc, table = launch(cfg(), 0, 0, img)          # and the good configuration runs
    assert rc == 0 and (table[:, 0] >= 1).all() and bool((img == 1.0).any())


# ------------------------------------------------------------------ the whole pipeline
def sources(seed=4):
    rng = np.random.default_rng(seed)
    shapes = [(40, 56), (90, 70), (64, 64), (57, 83), (75, 41), (48, 88), (66, 52), (81, 60)]
    return [P.synth_image(rng, h, w, 1 + i % 3) for i, (h, w) in enumerate(shapes)]


def batch_of(srcs):
    from yunet_amd.pipelines import SourceBatch
    return SourceBatch.from_lists([s[0] for s in srcs], [s[1] for s in srcs], [s[2] for s in srcs], DEV)


def pipeline_list(S, cutout=None, photo=False, mosaic=False, resize=None):
    lst = [dict(p) for p in BASE]
    lst[3] = dict(type='Resize', keep_ratio=False, **(resize or dict(img_scale=(S, S))))
    if cutout is not None:
        lst.insert(5, dict(cutout))
    if photo:
        lst.insert(5, dict(PMD))
    if mosaic:
        lst.insert(2, dict(MOSAIC, img_scale=(S, S)))
    return lst


HOLES = dict(CUT, fill_in=FILL)


def check_against_plain(with_c, plain, pipe, it, edge_of):
    """The batch of the list with CutOut against the same list without it: same GT, images equal outside the table's
    holes and fill_in inside."""
    for key in ('gt_bboxes', 'gt_keypointss'):
        assert with_c[key].padded.cpu().numpy().tobytes() == plain[key].padded.cpu().numpy().tobytes()
        assert torch.equal(with_c[key].counts, plain[key].counts)
    a, b = with_c['img'].cpu().numpy(), plain['img'].cpu().numpy()
    table = pipe.cutout_holes.cpu().numpy()
    holes = 0
    for n in range(a.shape[0]):
        s = edge_of(n)
        assert np.array_equal(table[n], R.holes(pipe.cfg.seed, it, n, s, s, HOLES)), f'image {n}'
        assert a[n].tobytes() == R.fill(b[n], table[n], FILL).tobytes(), f'image {n}'
        holes += int(table[n, 0])
    assert holes > 0
    return table


@pytest.mark.parametrize('S', [32, 64])
@pytest.mark.parametrize('photo', [False, True])
def test_pipeline_with_cutout_against_the_list_without(S, photo):
    from yunet_amd.pipelines import DevicePipeline
    srcs = sources()
    pc = DevicePipeline(pipeline_list(S, HOLES, photo=photo), seed=7)
    pp = DevicePipeline(pipeline_list(S, photo=photo), seed=7)
    for it in (0, 5):
        a, b = pc(batch_of(srcs), it), pp(batch_of(srcs), it)
        torch.cuda.synchronize()
        assert pc.check() == [] and pp.cutout_holes is None
        assert pc.params.cpu().numpy().tobytes() == pp.params.cpu().numpy().tobytes()
        if photo:
            assert pc.pparams.cpu().numpy().tobytes() == pp.pparams.cpu().numpy().tobytes()
        check_against_plain(a, b, pc, it, lambda n: S)
        assert a['img'].shape == (N, 3, S, S)


def test_pipeline_multiscale_canvas_keeps_its_zero_border():
    from yunet_amd.pipelines import DevicePipeline
    srcs = sources()
    resize = dict(img_scale=(32, 96), multiscale_mode='square_range')
    pc = DevicePipeline(pipeline_list(96, HOLES, resize=resize), seed=3)
    pp = DevicePipeline(pipeline_list(96, resize=resize), seed=3)
    a, b = pc(batch_of(srcs), 2), pp(batch_of(srcs), 2)
    torch.cuda.synchronize()
    assert torch.equal(pc.params, pp.params) and len(set(pc.sizes.tolist())) > 1
    check_against_plain(a, b, pc, 2, lambda n: int(pc.sizes[n]))
    img = a['img'].cpu().numpy()
    for n, s in enumerate(pc.sizes):
        assert not img[n, :, s:, :].any() and not img[n, :, :, s:].any()


def test_feeds_share_the_table_and_repeat():
    """Resident __call__, windowed(...) on a window plan and a Mosaic list: one cutout table per (seed, iteration);
    resident and windowed images byte-identical; the same call twice the same bytes; another iteration another table."""
    from yunet_amd.pipelines import DevicePipeline
    srcs, S, seed = sources(), 64, 11
    src = batch_of(srcs)
    pipe = DevicePipeline(pipeline_list(S, HOLES), seed=seed)
    tables = []
    for it in (1, 2):
        full = pipe(src, it)
        t_res = pipe.cutout_holes.clone()
        again = pipe(src, it)
        torch.cuda.synchronize()
        assert torch.equal(full['img'], again['img']) and torch.equal(t_res, pipe.cutout_holes)
        params, rect, off = pipe.window_plan(src, it, torch.device(DEV))
        win = _window_buffer(src, rect.cpu(), off.cpu())
        out = pipe.windowed(src, it, win, rect, off)
        torch.cuda.synchronize()
        assert out['img'].cpu().numpy().tobytes() == full['img'].cpu().numpy().tobytes()
        assert torch.equal(pipe.cutout_holes, t_res)
        assert torch.equal(out['gt_bboxes'].padded, full['gt_bboxes'].padded)
        pm = DevicePipeline(pipeline_list(S, HOLES, mosaic=True), seed=seed)
        pn = DevicePipeline(pipeline_list(S, mosaic=True), seed=seed)
        m, plain = pm(batch_of(srcs), it), pn(batch_of(srcs), it)
        torch.cuda.synchronize()
        assert torch.equal(pm.cutout_holes, t_res) and torch.equal(pm.geom, pn.geom)
        check_against_plain(m, plain, pm, it, lambda n: S)
        want = np.stack([R.holes(seed, it, n, S, S, HOLES) for n in range(N)])
        assert np.array_equal(t_res.cpu().numpy(), want)
        tables.append(want)
    assert not np.array_equal(tables[0], tables[1])


# ------------------------------------------------------------------ end to end
def test_train_cli_runs_with_cutout(tmp_path):
    spec = importlib.util.spec_from_file_location('yunet_train_tool_cutout', os.path.join(ROOT, 'tools', 'train.py'))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    cfg = tmp_path / 'yunet_s_cutout.py'
    cfg.write_text(open(os.path.join(ROOT, 'configs', 'yunet_s.py')).read() + '''
train_pipeline[3]['img_scale'] = (160, 160)
train_pipeline.insert(5, dict(type='CutOut', n_holes=(0, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.2)], fill_in=(114, 114, 114)))
''')
    work = tmp_path / 'w'
    hist = T.main([str(cfg), '--work-dir', str(work), '--seed', '3', '--no-validate', '--max-iters', '3',
                   '--cfg-options', 'data.samples_per_gpu=4', 'data.train.type=SyntheticSourceImages',
                   'data.train.pool=4', 'log_config.interval=1'])
    losses = [h['loss'] for h in hist if 'loss' in h]
    assert len(losses) >= 3 and all(np.isfinite(losses)), hist
    assert 'CutOut' in open(work / 'yunet_s_cutout.py').read()
    pipe = T.main.last_source.pipe
    assert pipe.cutout is not None and pipe.out_size == 160
    table = pipe.cutout_holes.cpu().numpy()
    assert table.shape == (4, R.WORDS) and (table[:, 0] <= 4).all() and (table[:, 2:] <= 160).all()
