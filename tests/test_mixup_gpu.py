"""-m gpu: MixUp with landmarks and the mode switch in the device train pipeline (csrc/augment.hip
aug_mixup_decide_kernel / aug_mixup_pixels_kernel through yunet_aug_mixup_decide / yunet_aug_mixup_pixels and
DevicePipeline) against the fixture made by the unmodified reference class and the restatement (tests/mixup_ref.py).

Tables, draws, counts, order, cleared rows and boxes are compared byte for byte (the boxes with the reference's own);
landmarks byte for byte with mixup_ref's float32 evaluation; every output byte of the blend lies in the admissible set of
tests/test_mixup.py (the float64 partner value and the bar recorded in the fixture); hand-made cases exactly."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import mixup_ref as R
from test_affine import AFF, CUT, MOSAIC
from test_cutout_gpu import batch_of, sources
from test_mixup import MIX, cases, golden, golden_store
from test_photometric import BASE, PMD

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 2 * R.GMAX


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def store_of(imgs, boxes, kps):
    """-> (SourceBatch holding the images as its own store, its StoreView)."""
    from yunet_amd.pipelines import SourceBatch
    src = SourceBatch.from_lists(imgs, boxes, kps, DEV)
    return src, src.store_view()[0]


def run_decide(cfg, D, seed, iteration, view, boxes, kps, counts, edge, params=None):
    """yunet_aug_mixup_decide on padded GT (numpy) -> (out boxes, out kps, out counts, table) -- the first three on the
    host; the outputs start as -7 so that every row the kernel has to clear shows."""
    import yunet_amd._lib as L
    from yunet_amd.pipelines import MixUp
    n, gmax = boxes.shape[:2]
    c = MixUp(img_scale=(D, D), use_kps=True, **cfg).c_cfg(seed, gmax)
    ib, ik = torch.from_numpy(boxes).to(DEV), torch.from_numpy(kps.reshape(n, gmax, 15)).to(DEV)
    ic = torch.from_numpy(counts).to(DEV)
    ob, ok, oc = torch.full_like(ib, -7.0), torch.full_like(ik, -7.0), torch.full_like(ic, -7)
    table = torch.full((n, L.MIXUP_WORDS), -7.0, dtype=torch.float64, device=DEV)
    rc = L.load().yunet_aug_mixup_decide(C.byref(c), iteration, n, edge, _p(params), view.m, _p(view.hw), _p(view.goff),
                                         _p(view.gcnt), _p(view.boxes), _p(view.kps), _p(ib), _p(ik), _p(ic), _p(ob), _p(ok),
                                         _p(oc), _p(table), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(ib.cpu(), torch.from_numpy(boxes)) and torch.equal(ic.cpu(), torch.from_numpy(counts))
    return ob.cpu().numpy(), ok.cpu().numpy().reshape(n, gmax, 5, 3), oc.cpu().numpy(), table


def run_pixels(table, D, pad, img, src, view, params=None):
    """yunet_aug_mixup_pixels in place on a copy of img -> the copy."""
    import yunet_amd._lib as L
    out = img.clone()
    rc = L.load().yunet_aug_mixup_pixels(_p(table), D, float(pad), img.shape[0], img.shape[-1], _p(params), view.m,
                                         _p(src.src), _p(view.off), _p(view.hw), _p(out), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out


def padded_own(g, edge, rows=ROWS):
    b, k, c = g[f'own_boxes_{edge}'], g[f'own_kps_{edge}'], g[f'own_counts_{edge}']
    pb, pk = np.zeros((len(c), rows, 4), np.float32), np.zeros((len(c), rows, 5, 3), np.float32)
    pb[:, :b.shape[1]], pk[:, :b.shape[1]] = b, k
    return pb, pk, c


# ------------------------------------------------------------------ the two entries against the fixture
@pytest.mark.parametrize('name,edge', cases())
def test_decide_against_the_reference_fixture(name, edge):
    g = golden()
    s, (D, cfg), it = golden_store(g), R.case_cfg(name, edge), int(g[f'it_{name}_{edge}'])
    src, view = store_of(s['imgs'], s['boxes'], s['kps'])
    pb, pk, counts = padded_own(g, edge)
    ob, ok, oc, table = run_decide(cfg, D, R.SEED, it, view, pb, pk, counts, edge)
    t = table.cpu().numpy()
    assert t.tobytes() == g[f'table_{name}_{edge}'].tobytes(), 'table: partner, draws, geometry, rows'
    for i in range(R.N_IMAGES):
        c = int(counts[i])
        d = R.decide(R.SEED, it, i, s, pb[i, :c], pk[i, :c], edge, D, cfg)
        k = int(g[f'rows_{name}_{edge}'][i])
        assert oc[i] == k == len(d['boxes']), f'image {i}: count'
        assert ob[i, :k].tobytes() == g[f'boxes_{name}_{edge}'][i, :k].tobytes(), f'image {i}: boxes, survivors or their order'
        assert ok[i, :k].tobytes() == d['kps'].tobytes(), f'image {i}: landmarks'
        assert not ob[i, k:].any() and not ok[i, k:].any(), f'image {i}: rows at and beyond the count are 0'


@pytest.mark.parametrize('edge', R.EDGES)
def test_pixels_lie_in_the_admissible_set(edge):
    """The tables of the fixture, all configurations of an edge: every output byte of an applied image is admissible,
    integer-valued and within [0, 255]; an image that is not applied keeps its bytes, signed zeros included."""
    g = golden()
    s, bar = golden_store(g), float(g[f'bar_pixels_{edge}'])
    src, view = store_of(s['imgs'], s['boxes'], s['kps'])
    a = R.pattern(R.N_IMAGES, edge)
    a[:, :, 3, 5], a[:, :, 4, 5] = -0.0, 0.0
    img = torch.from_numpy(a).to(DEV)
    applied = others = 0
    for name in R.CONFIGS:
        D, cfg = R.case_cfg(name, edge)
        pad = R.full(cfg)['pad_val']
        table = torch.from_numpy(g[f'table_{name}_{edge}']).to(DEV)
        out = run_pixels(table, D, pad, img, src, view).cpu().numpy()
        for i, t in enumerate(g[f'table_{name}_{edge}']):
            if not t[R.APPLIED]:
                assert out[i].tobytes() == a[i].tobytes(), f'{name} image {i}: not applied, the bytes stay'
                others += 1
                continue
            b64, zero = R.partner_value(t, s['imgs'][int(t[R.PARTNER])], D, pad, np.float64)
            lo, hi = R.admissible(a[i].transpose(1, 2, 0), b64, zero, bar)
            o = out[i].transpose(1, 2, 0)
            assert ((o >= lo) & (o <= hi)).all(), f'{name} image {i}: {int(((o < lo) | (o > hi)).sum())} bytes outside'
            assert np.array_equal(o, np.trunc(o)) and o.min() >= 0 and o.max() <= 255
            applied += 1
    assert applied and others


# ------------------------------------------------------------------ hand-made exact cases
def _exact_case(T, D, flip_ratio, a=None, seed=3):
    """One partner image D x D with a box, ratio_range (1, 1): every tap falls on the grid.  -> (a, partner CHW float32,
    out, table row) on the host."""
    rng = np.random.default_rng(10 * T + D)
    partner = rng.integers(0, 256, (D, D, 3), dtype=np.uint8)
    box = np.array([[2.0, 3.0, D - 2.0, D - 1.0]], np.float32)
    kps = np.zeros((1, 5, 3), np.float32)
    src, view = store_of([partner], [box], [kps])
    a = R.pattern(2, T) if a is None else a
    cfg = dict(ratio_range=(1.0, 1.0), flip_ratio=flip_ratio)
    pb, pk = np.zeros((2, 4, 4), np.float32), np.zeros((2, 4, 5, 3), np.float32)
    _, _, oc, table = run_decide(cfg, D, seed, 0, view, pb, pk, np.zeros(2, np.int32), T)
    out = run_pixels(table, D, 114, torch.from_numpy(a).to(DEV), src, view).cpu().numpy()
    t = table.cpu().numpy()
    assert (t[:, R.APPLIED] == 1).all() and (t[:, R.J_] == D).all() and (t[:, R.RW] == D).all() and (oc == 1).all()
    return a, partner.transpose(2, 0, 1).astype(np.float32), out, t


def test_exact_unflipped_and_flipped():
    T = 32
    a, p, out, t = _exact_case(T, T, flip_ratio=1.0)        # uniform(0, 1) > 1 never holds
    assert not t[:, R.FLIP].any() and (t[:, R.DRAWS] == 3).all()
    for n in range(2):
        assert out[n].tobytes() == R.blend(a[n], p).tobytes()
    a, p, out, t = _exact_case(T, T, flip_ratio=-1.0)       # and > -1 always
    assert t[:, R.FLIP].all()
    flipped = torch.flip(torch.from_numpy(p), dims=[-1]).numpy()
    for n in range(2):
        assert out[n].tobytes() == R.blend(a[n], flipped).tobytes()


def test_exact_twice_the_edge_with_drawn_offsets():
    T, D = 32, 64
    for seed in (3, 4):
        a, p, out, t = _exact_case(T, D, flip_ratio=1.0, seed=seed)
        assert (t[:, R.DRAWS] == 5).all() and t[:, [R.XOFF, R.YOFF]].max() > 0 and t[:, [R.XOFF, R.YOFF]].max() < D - T
        for n in range(2):
            x, y = int(t[n, R.XOFF]), int(t[n, R.YOFF])
            assert out[n].tobytes() == R.blend(a[n], p[:, y:y + T, x:x + T]).tobytes()


def test_exact_half_the_edge_leaves_half_of_a_outside_the_partner():
    T, D = 32, 16
    a, p, out, t = _exact_case(T, D, flip_ratio=-1.0)
    full = np.zeros((3, T, T), np.float32)
    full[:, :D, :D] = p[:, :, ::-1]
    for n in range(2):
        assert out[n].tobytes() == R.blend(a[n], full[None][0]).tobytes()
        assert np.array_equal(out[n, :, D:, :], np.trunc(np.float32(0.5) * a[n, :, D:, :]))


def test_exact_values_outside_the_byte_range_saturate():
    T = 32
    a = R.pattern(2, T)
    a[0, :, :8], a[0, :, 8:16], a[1, :, :4] = 700.5, -300.25, 255.0
    a, p, out, _ = _exact_case(T, T, flip_ratio=1.0, a=a)
    want = np.trunc(np.clip(np.float32(0.5) * a + np.float32(0.5) * p[None], 0, 255))
    assert out.tobytes() == want.tobytes() and (out[0, :, :8] == 255).all() and (out[0, :, 8:16] == 0).all()


# ------------------------------------------------------------------ rows
def test_decide_compacts_more_rows_than_a_wave_in_order_and_reports_truncation():
    """130 own rows (three steps of the 64-lane loop), every third one outside, then a partner of 70 rows: survivors in
    order across the steps and across the two sources.  With a capacity below the survivors: status 2 through check()."""
    from yunet_amd.pipelines import DevicePipeline
    T, D, own, gp = 64, 64, 130, 70
    rng = np.random.default_rng(5)
    partner = rng.integers(0, 256, (D, D, 3), dtype=np.uint8)
    xy = rng.uniform(4, 40, (gp, 2))
    pboxes = np.concatenate([xy, xy + rng.uniform(3, 12, (gp, 2))], 1).astype(np.float32)
    pkps = np.zeros((gp, 5, 3), np.float32)
    pkps[:, :, 2] = 1000 + np.arange(gp)[:, None]
    src, view = store_of([partner], [pboxes], [pkps])
    cfg = dict(ratio_range=(1.0, 1.0), flip_ratio=1.0)
    for gmax in (256, 140):
        boxes, kps = np.zeros((2, gmax, 4), np.float32), np.zeros((2, gmax, 5, 3), np.float32)
        n_own = min(own, gmax)
        xy = rng.uniform(4, 40, (2, n_own, 2))
        boxes[:, :n_own, :2], boxes[:, :n_own, 2:] = xy, xy + rng.uniform(3, 12, (2, n_own, 2))
        boxes[:, :n_own:3] += 500.0
        kps[:, :n_own, :, 2] = np.arange(n_own, dtype=np.float32)[None, :, None]        # the row number rides along
        counts = np.array([n_own, 70], np.int32)
        ob, ok, oc, table = run_decide(cfg, D, 1, 0, view, boxes, kps, counts, T)
        t = table.cpu().numpy()
        for i, c in enumerate(counts):
            keep = [j for j in range(c) if j % 3] + [1000 + j for j in range(gp)]
            assert t[i, R.ROWS_IN] == c and t[i, R.ROWS_OUT] == len(keep) and t[i, R.STATUS] == (2 if len(keep) > gmax else 0)
            k = min(len(keep), gmax)
            assert oc[i] == k and ok[i, :k, 0, 2].tolist() == keep[:k]
            own_kept = [j for j in range(c) if j % 3]
            assert np.array_equal(ob[i, :len(own_kept)], boxes[i, own_kept])
            assert np.array_equal(ob[i, len(own_kept):k], pboxes[:k - len(own_kept)])
            assert not ob[i, k:].any() and not ok[i, k:].any()
        if gmax == 140:
            assert t[:, R.STATUS].tolist() == [2, 0]
            pipe = DevicePipeline(BASE, seed=1)
            pipe.params, pipe.mixup_table = torch.zeros(2, 8, dtype=torch.int32, device=DEV), table
            assert pipe.check() == [0]


def test_multiscale_canvas_touches_each_corner_only():
    """S_n in {32, 64} in one batch: the border stays 0 and each corner equals the fixed-size run at S_n."""
    g = golden()
    s = golden_store(g)
    src, view = store_of(s['imgs'], s['boxes'], s['kps'])
    sizes = np.array([32, 64, 64, 32, 32, 64], np.int32)
    params = torch.zeros(R.N_IMAGES, 8, dtype=torch.int32, device=DEV)
    params[:, 7] = torch.from_numpy(sizes).to(DEV)
    D, cfg = 48, dict(max_iters=2)
    fixed = {}
    for e in R.EDGES:
        pb, pk, c = padded_own(g, e)
        ob, ok, oc, table = run_decide(cfg, D, 9, 4, view, pb, pk, c, e)
        img = torch.from_numpy(R.pattern(R.N_IMAGES, e)).to(DEV)
        fixed[e] = (ob, ok, oc, table.cpu().numpy(), run_pixels(table, D, 114, img, src, view).cpu().numpy(), pb, pk, c)
    pb, pk, c = (np.stack([fixed[int(e)][k][i] for i, e in enumerate(sizes)]) for k in (5, 6, 7))
    ob, ok, oc, table = run_decide(cfg, D, 9, 4, view, pb, pk, c.astype(np.int32), 64, params=params)
    canvas = np.zeros((R.N_IMAGES, 3, 64, 64), np.float32)
    for i, e in enumerate(sizes):
        canvas[i, :, :e, :e] = R.pattern(R.N_IMAGES, int(e))[i]
    out = run_pixels(table, D, 114, torch.from_numpy(canvas).to(DEV), src, view, params=params).cpu().numpy()
    t = table.cpu().numpy()
    assert t[:, R.APPLIED].any() and np.array_equal(t[:, R.EDGE], sizes)
    for i, e in enumerate(sizes):
        f = fixed[int(e)]
        assert t[i].tobytes() == f[3][i].tobytes() and oc[i] == f[2][i]
        assert ob[i].tobytes() == f[0][i].tobytes() and ok[i].tobytes() == f[1][i].tobytes()
        assert out[i, :, :e, :e].tobytes() == f[4][i].tobytes(), f'image {i}: the corner is the fixed-size run'
        assert not out[i, :, e:, :].any() and not out[i, :, :, e:].any(), f'image {i}: the border stays 0'


# ------------------------------------------------------------------ the whole pipeline
HOLES = dict(CUT, fill_in=(1.0, 2.0, 3.0))
STRONG = dict(AFF, max_rotate_degree=30.0, max_translate_ratio=0.2)


def pipeline_list(S, mix=None, photo=False, mosaic=False, affine=None, cutout=None, resize=None):
    lst = [dict(p) for p in BASE]
    lst[3] = dict(type='Resize', keep_ratio=False, **(resize or dict(img_scale=(S, S))))
    lst[5:5] = ([dict(PMD)] if photo else []) + ([dict(affine)] if affine else []) + ([dict(mix)] if mix else []) + \
        ([dict(cutout)] if cutout else [])
    if mosaic:
        lst.insert(2, dict(MOSAIC, img_scale=(S, S)))
    return lst


def gt_rows(batch):
    """The rows below the count, per image, as bytes (pipelines of different capacities pad differently)."""
    cnt = batch['gt_bboxes'].counts.cpu().numpy()
    b, k = batch['gt_bboxes'].padded.cpu().numpy(), batch['gt_keypointss'].padded.cpu().numpy()
    assert all(not b[n, c:].any() and not k[n, c:].any() for n, c in enumerate(cnt))
    return cnt.tolist(), [b[n, :c].tobytes() + k[n, :c].tobytes() for n, c in enumerate(cnt)]


def test_step_leaves_the_other_draws_alone_and_repeats():
    from yunet_amd.pipelines import DevicePipeline
    srcs, S, seed = sources(), 64, 11
    kw = dict(S=S, photo=True, mosaic=True, affine=STRONG, cutout=HOLES)
    mix = dict(MIX, img_scale=(48, 48))
    pm = DevicePipeline(pipeline_list(mix=mix, **kw), seed=seed, gmax=8)
    pp = DevicePipeline(pipeline_list(**kw), seed=seed, gmax=8)
    assert (pm.gmax, pp.gmax) == (40, 32)
    tables = []
    for it in (1, 2):
        a, b = pm(batch_of(srcs), it), pp(batch_of(srcs), it)
        t = pm.mixup_table.clone()
        again = pm(batch_of(srcs), it)
        torch.cuda.synchronize()
        assert pm.check() == [] and pp.mixup_table is None
        for name in ('params', 'pparams', 'geom', 'affine_table', 'cutout_holes'):
            assert getattr(pm, name).cpu().numpy().tobytes() == getattr(pp, name).cpu().numpy().tobytes(), name
        assert not torch.equal(a['img'], b['img'])
        assert torch.equal(a['img'], again['img']) and torch.equal(t, pm.mixup_table)
        assert gt_rows(a) == gt_rows(again) and a['gt_bboxes'].padded.shape[1] == 40
        t = t.cpu().numpy()
        hw = [s[0].shape[:2] for s in srcs]
        counts = [len(s[1]) for s in srcs]
        cfg = {k: v for k, v in mix.items() if k not in ('type', 'use_kps', 'img_scale')}
        for n in range(len(srcs)):
            want = R.geometry(seed, it, n, counts, hw, S, 48, cfg)
            skip = [R.ROWS_IN, R.ROWS_OUT, R.STATUS]
            assert np.delete(t[n], skip).tobytes() == np.delete(want, skip).tobytes(), f'image {n}: table'
        # the GT the step was given is the GT of the list without it, and it comes first in the step's output
        cb, rb = gt_rows(b)
        ca, _ = gt_rows(a)
        assert t[:, R.ROWS_IN].tolist() == cb and t[:, R.ROWS_OUT].tolist() == ca and t[:, R.APPLIED].all()
        ga, gb = a['gt_bboxes'].padded.cpu().numpy(), b['gt_bboxes'].padded.cpu().numpy()
        for n in range(len(srcs)):
            inside = (gb[n, :cb[n], 0] < S) & (gb[n, :cb[n], 2] > 0) & (gb[n, :cb[n], 1] < S) & (gb[n, :cb[n], 3] > 0)
            assert np.array_equal(ga[n, :int(inside.sum())], gb[n, :cb[n]][inside])
        assert sum(ca) > sum(cb), 'the partners bring rows'
        # holes are cut into the blended image: fill_in inside the table's holes; elsewhere whole numbers
        holes, img = pm.cutout_holes.cpu().numpy(), a['img'].cpu().numpy()
        for n in range(len(srcs)):
            for j in range(int(holes[n, 0])):
                x1, y1, x2, y2 = holes[n, 2 + 4 * j:6 + 4 * j]
                assert (img[n, :, y1:y2, x1:x2] == np.array(HOLES['fill_in'], np.float32).reshape(3, 1, 1)).all()
        assert np.array_equal(img, np.trunc(img)) and img.min() >= 0 and img.max() <= 255
        tables.append(t)
    assert not np.array_equal(tables[0], tables[1])


def test_skipped_steps_launch_nothing_and_give_the_bytes_of_the_list_without_them():
    from yunet_amd.pipelines import DevicePipeline
    srcs, S, seed = sources(), 64, 5
    kw = dict(S=S, photo=True, cutout=HOLES)
    pm = DevicePipeline(pipeline_list(mix=dict(MIX, img_scale=(48, 48)), mosaic=True, affine=STRONG, **kw), seed=seed, gmax=8)
    pp = DevicePipeline(pipeline_list(**kw), seed=seed, gmax=8)
    first = pm(batch_of(srcs), 3)
    assert pm.mixup_table is not None and pm.geom is not None
    first_img, first_gt = first['img'].clone(), gt_rows(first)
    pm.update_skip_type_keys(('Mosaic', 'RandomAffine', 'MixUp'))
    a, b = pm(batch_of(srcs), 3), pp(batch_of(srcs), 3)
    torch.cuda.synchronize()
    assert pm.mixup_table is None and pm.geom is None and pm.affine_table is None, 'a skipped step writes no table'
    assert a['img'].cpu().numpy().tobytes() == b['img'].cpu().numpy().tobytes()
    assert gt_rows(a) == gt_rows(b) and pm.check() == pp.check() == []
    assert a['gt_bboxes'].padded.shape[1] == a['gt_keypointss'].padded.shape[1] == pm.gmax == 40 and pp.gmax == 8
    assert a['gt_labels'][0].shape[0] == 40
    for name in ('params', 'pparams', 'cutout_holes'):
        assert getattr(pm, name).cpu().numpy().tobytes() == getattr(pp, name).cpu().numpy().tobytes(), name
    # one step skipped: the list without that step
    pm.update_skip_type_keys(['MixUp'])
    pa = DevicePipeline(pipeline_list(mosaic=True, affine=STRONG, **kw), seed=seed, gmax=10)      # 4 * 10: the same capacity
    a, b = pm(batch_of(srcs), 3), pa(batch_of(srcs), 3)
    assert torch.equal(a['img'], b['img']) and gt_rows(a) == gt_rows(b) and pm.mixup_table is None
    assert torch.equal(pm.geom, pa.geom) and torch.equal(pm.affine_table, pa.affine_table)
    pm.update_skip_type_keys(())
    again = pm(batch_of(srcs), 3)
    torch.cuda.synchronize()
    assert torch.equal(again['img'], first_img) and gt_rows(again) == first_gt and pm.mixup_table is not None


def test_forward_train_through_the_whole_recipe_with_an_image_that_lost_every_row():
    """Mosaic -> ... -> RandomAffine -> MixUp -> CutOut -> Normalize on a resident store.  The translation empties an
    image's own rows and the size rule removes the partner's small faces, so some images end with no row at all."""
    import yunet_amd
    from yunet_amd.optim import FusedSGD
    from yunet_amd.pipelines import DevicePipeline
    srcs = sources()
    away = dict(AFF, max_rotate_degree=0.0, max_translate_ratio=1.0, scaling_ratio_range=(1.0, 1.0), max_shear_degree=0.0)
    mix = dict(MIX, img_scale=(160, 160), skip_filter=False, min_bbox_size=30.0)
    pipe = DevicePipeline(pipeline_list(160, mix=mix, mosaic=True, affine=away, cutout=HOLES), seed=2)
    for it in range(48):
        batch = pipe(batch_of(srcs), it)
        cnt = batch['gt_bboxes'].counts.cpu().numpy()
        t = pipe.mixup_table.cpu().numpy()
        if (cnt == 0).any() and (t[:, R.ROWS_OUT] > t[:, R.ROWS_IN]).any():
            break
    else:
        pytest.fail('no batch with an emptied image and a partner row in 48 iterations')
    assert t[:, R.APPLIED].all()
    assert pipe.check() == []
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
def _train_tool(tag):
    spec = importlib.util.spec_from_file_location(f'yunet_train_tool_{tag}', os.path.join(ROOT, 'tools', 'train.py'))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    return T


RECIPE = '''
train_pipeline[3]['img_scale'] = (160, 160)
train_pipeline.insert(2, dict(type='Mosaic', img_scale=(160, 160), use_kps=True))
train_pipeline.insert(6, dict(type='RandomAffine', max_rotate_degree=20.0, use_kps=True))
train_pipeline.insert(7, dict(type='MixUp', img_scale=(160, 160), use_kps=True))
train_pipeline.insert(8, dict(type='CutOut', n_holes=(0, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.2)], fill_in=(114, 114, 114)))
'''


def test_train_cli_runs_with_mixup(tmp_path):
    T = _train_tool('mixup')
    cfg = tmp_path / 'yunet_s_mixup.py'
    cfg.write_text(open(os.path.join(ROOT, 'configs', 'yunet_s.py')).read() + RECIPE)
    work = tmp_path / 'w'
    hist = T.main([str(cfg), '--work-dir', str(work), '--seed', '3', '--no-validate', '--max-iters', '3',
                   '--cfg-options', 'data.samples_per_gpu=4', 'data.train.type=SyntheticSourceImages',
                   'data.train.pool=4', 'log_config.interval=1'])
    losses = [h['loss'] for h in hist if 'loss' in h]
    assert len(losses) >= 3 and all(np.isfinite(losses)), hist
    assert 'MixUp' in open(work / 'yunet_s_mixup.py').read()
    pipe = T.main.last_source.pipe
    assert pipe.mixup is not None and pipe.mosaic is not None and pipe.affine is not None and pipe.gmax == 5 * 64
    t = pipe.mixup_table.cpu().numpy()
    assert t.shape == (4, R.WORDS) and t[:, R.APPLIED].any() and (t[:, R.EDGE] == 160).all()
    live = t[:, R.APPLIED] == 1
    assert ((t[live, R.J_] >= 80) & (t[live, R.J_] <= 240)).all() and (t[:, R.ROWS_OUT] >= t[:, R.ROWS_IN]).any()


def test_mode_switch_hook_in_a_three_epoch_run(tmp_path):
    """max_epochs 3, num_last_epochs 1: the switch comes at the start of the second epoch (epoch + 1 == 3 - 1), read from
    the log lines and from mixup_table no longer being written."""
    from yunet_amd.runner import HOOKS, Hook
    seen, lines = [], []

    class Watch(Hook):
        def before_run(self, runner):
            log = runner.logger
            runner.logger = lambda m, *a, **k: (lines.append((runner.epoch, m)), log(m, *a, **k))[1]

        def after_train_iter(self, runner):
            pipe = runner.data_loader.dataset.pipe
            seen.append((runner.epoch, pipe.mixup_table is not None, pipe.geom is not None, pipe._on('RandomAffine'),
                         tuple(runner.data_batch['gt_bboxes'].padded.shape[1:])))
    T = _train_tool('mode_switch')
    cfg = tmp_path / 'yunet_s_switch.py'
    cfg.write_text(open(os.path.join(ROOT, 'configs', 'yunet_s.py')).read() + RECIPE + """
custom_hooks = [dict(type='MixupTestWatch'), dict(type='YOLOXModeSwitchHook', num_last_epochs=1)]
runner = dict(type='EpochBasedRunner', max_epochs=3)
""")
    HOOKS['MixupTestWatch'] = Watch
    try:
        hist = T.main([str(cfg), '--work-dir', str(tmp_path / 'w'), '--seed', '3', '--no-validate',
                       '--cfg-options', 'data.samples_per_gpu=4', 'data.train.type=SyntheticSourceImages',
                       'data.train.pool=4', 'data.train.iters_per_epoch=2', 'log_config.interval=1'])
    finally:
        del HOOKS['MixupTestWatch']
    switch = [(e, m) for e, m in lines if 'now!' in str(m)]
    assert switch == [(1, 'No mosaic and mixup aug now!'), (1, 'Add additional L1 loss now!')]
    assert [s[0] for s in seen] == [0, 0, 1, 1, 2, 2]
    assert [s[1:4] for s in seen] == [(True, True, True)] * 2 + [(False, False, False)] * 4
    assert {s[4] for s in seen} == {(5 * 64, 4)}, 'the padded GT keeps its capacity: the engine keeps its plan'
    pipe = T.main.last_source.pipe
    assert pipe._skip == {'Mosaic', 'RandomAffine', 'MixUp'} and pipe.mixup_table is None
    losses = [h['loss'] for h in hist if 'loss' in h]
    assert len(losses) >= 6 and all(np.isfinite(losses)), hist
