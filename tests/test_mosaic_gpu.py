"""-m gpu: Mosaic(use_kps=True) on the device, through the C ABI and DevicePipeline, reading only tests/golden/:
(a) yunet_aug_mosaic_decide against the fixture the unmodified reference classes made (geometry and counts exact,
merged GT bit for bit, order preserved, truncation); (b) the canvas through the pixel pass's tap function
(yunet_aug_mosaic_canvas) against the CPU composition of tests/mosaic_ref.py, bit for bit, pad pixels included; (c) the
whole pipeline against the EXISTING pipeline run on a store that holds the materialised canvases and the merged GT as
ordinary source images, and against the numpy restatement of crop / resize / flip on the float canvas; (d) prob = 0
against the pipeline without Mosaic; (e) a short training run.  Every case is one bounded pass: no retries."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import mosaic_ref as MR
import pipeline_oracle as P
from test_mosaic import LOAD, mosaic_list, tail

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_store(srcs):
    from yunet_amd.source_store import SourceStore
    store = SourceStore([s[0].shape[:2] for s in srcs], placement='device', device=DEV)
    for i, (img, b, k) in enumerate(srcs):
        store.put(i, img, b, k)
    return store


def mosaic_cfg(case, gmax):
    from yunet_amd.pipelines import Mosaic
    m = Mosaic(img_scale=(case['S'], case['S']), center_ratio_range=case['center'], min_bbox_size=case['min_bbox_size'],
               bbox_clip_border=case['clip'], skip_filter=case['skip_filter'], pad_val=case['pad_val'], prob=case['prob'],
               use_kps=True)
    return m.c_cfg(case['seed'], gmax)


def run_decide(case, srcs, gmax, canvas=False):
    """yunet_aug_mosaic_decide (and yunet_aug_mosaic_canvas) through the C ABI -> numpy arrays."""
    from yunet_amd import _lib as L
    lib = L.load()
    sb = make_store(srcs).batch(case['idx'])
    view, idx = sb.store_view()
    n, cfg = sb.n, mosaic_cfg(case, gmax)
    geom = torch.full((n, L.MOSAIC_WORDS), -7, device=DEV, dtype=torch.int32)
    hw = torch.empty(n, 2, device=DEV, dtype=torch.int32)
    mb = torch.full((n, gmax, 4), -7.0, device=DEV)
    mk = torch.full((n, gmax, 5, 3), -7.0, device=DEV)
    mc = torch.empty(n, device=DEV, dtype=torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.yunet_aug_mosaic_decide(p(idx), n, view.m, p(view.hw), p(view.goff), p(view.gcnt), p(view.boxes),
                                        p(view.kps), C.byref(cfg), case['iteration'], p(geom), p(hw), p(mb), p(mk), p(mc),
                                        stream), 'yunet_aug_mosaic_decide')
    out = dict(geom=geom, hw=hw, boxes=mb, kps=mk, count=mc)
    if canvas:
        E = 2 * case['S']
        buf = torch.full((n * E * E * 3 + 64,), -7.0, device=DEV)
        L.check(lib.yunet_aug_mosaic_canvas(p(sb.src), p(view.off), p(geom), C.byref(cfg), n, p(buf), stream), 'canvas')
        torch.cuda.synchronize()
        assert float(buf[n * E * E * 3:].min()) == -7.0 == float(buf[n * E * E * 3:].max()), 'wrote past the canvases'
        out['canvas'] = buf[:n * E * E * 3].view(n, E, E, 3)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ (a) the decide kernel against the reference fixture
@pytest.mark.parametrize('row', MR.CASES, ids=[r[0] for r in MR.CASES])
def test_mosaic_decide_vs_reference_fixture(row):
    from yunet_amd import _lib as L
    z, stores = MR.load_fixture()
    case = MR.case_dict(row)
    srcs, gmax = stores[case['store']], 256
    got = run_decide(case, srcs, gmax)
    for n, own in enumerate(case['idx']):
        key = f"{case['name']}/{n}/"
        meta, fg = [int(v) for v in z[key + 'meta']], z[key + 'geom']
        g = got['geom'][n]
        applied = meta[3]
        assert [int(g[L.MOSAIC_APPLIED]), int(g[L.MOSAIC_CX]), int(g[L.MOSAIC_CY]), int(g[L.MOSAIC_DRAWS])] == meta[3:], key
        assert int(g[L.MOSAIC_STATUS]) == 0
        if applied:
            for q in range(4):
                w = g[L.MOSAIC_QUAD + q * L.MOSAIC_QWORDS:][:L.MOSAIC_QWORDS]
                assert int(w[L.MOSAIC_Q_IDX]) == ([own] + meta[:3])[q], key
                assert [int(v) for v in w[1:11]] == [int(v) for v in fg[q, :10]], (key, q, w[:11], fg[q])
                sc = w[L.MOSAIC_Q_SX:L.MOSAIC_Q_SX + 4].view(np.float64)
                assert sc[0] == 1.0 / (float(fg[q, 2]) / float(fg[q, 1])) and sc[1] == 1.0 / (float(fg[q, 3]) / float(fg[q, 0]))
            assert got['hw'][n].tolist() == [2 * case['S']] * 2
        else:
            assert got['hw'][n].tolist() == list(srcs[own][0].shape[:2])
            assert int(g[L.MOSAIC_QUAD + L.MOSAIC_Q_IDX]) == own
        fb, fk = z[key + 'boxes'], z[key + 'kps']
        k = len(fb)
        assert int(got['count'][n]) == k == int(g[L.MOSAIC_KEPT]), key
        assert got['boxes'][n, :k].tobytes() == fb.tobytes(), key + 'boxes'
        assert got['kps'][n, :k].tobytes() == fk.tobytes(), key + 'kps'
        assert not got['boxes'][n, k:].any() and not got['kps'][n, k:].any(), 'rows beyond the count are zero'


def test_merged_gt_beyond_gmax_is_truncated_and_flagged():
    """The first gmax rows, in order, and status 2 -- what the crop's compaction does with kept > gmax."""
    from yunet_amd import _lib as L
    z, stores = MR.load_fixture()
    case = MR.case_dict(MR.CASES[0])
    got = run_decide(case, stores['main'], 16)
    flagged = 0
    for n in range(len(case['idx'])):
        fb, fk = z[f'default/{n}/boxes'], z[f'default/{n}/kps']
        k = min(16, len(fb))
        assert int(got['count'][n]) == k and int(got['geom'][n, L.MOSAIC_KEPT]) == len(fb)
        assert int(got['geom'][n, L.MOSAIC_STATUS]) == (2 if len(fb) > 16 else 0)
        assert got['boxes'][n, :k].tobytes() == fb[:k].tobytes() and got['kps'][n, :k].tobytes() == fk[:k].tobytes()
        assert not got['boxes'][n, k:].any()
        flagged += len(fb) > 16
    assert flagged >= 3


def test_bad_arguments_are_rejected_on_the_host():
    """No launch: an index outside the store (IndexError from the batch builder), a bad configuration (EINVAL)."""
    from yunet_amd import _lib as L
    _, stores = MR.load_fixture()
    store = make_store(stores['main'])
    for bad in ([0, len(store)], [-1, 2]):
        with pytest.raises(IndexError):
            store.batch(bad)
    lib = L.load()
    case = MR.case_dict(MR.CASES[0])
    one = torch.zeros(64, device=DEV, dtype=torch.int32)
    p = C.c_void_p(one.data_ptr())
    for field, val in (('center_hi', 2.5), ('center_lo', -0.1), ('prob', 1.5), ('img_scale', 0), ('gmax', 0)):
        cfg = mosaic_cfg(case, 64)
        setattr(cfg, field, val)
        assert lib.yunet_aug_mosaic_decide(p, 1, 1, p, p, p, p, p, C.byref(cfg), 0, p, p, p, p, p, None) == L.EINVAL
    cfg = mosaic_cfg(case, 64)
    assert lib.yunet_aug_mosaic_decide(p, 1, 0, p, p, p, p, p, C.byref(cfg), 0, p, p, p, p, p, None) == L.EINVAL
    assert lib.yunet_aug_mosaic_decide(p, 0, 1, p, p, p, p, p, C.byref(cfg), 0, p, p, p, p, p, None) == L.EINVAL


# ------------------------------------------------------------------ (b) the canvas through the tap function
@pytest.mark.parametrize('row', MR.CASES, ids=[r[0] for r in MR.CASES])
def test_canvas_vs_cpu_composition(row):
    _, stores = MR.load_fixture()
    case = MR.case_dict(row)
    srcs = stores[case['store']]
    got = run_decide(case, srcs, 256, canvas=True)['canvas']
    ref = MR.run_case(case, srcs)
    for n, r in enumerate(ref):
        want = r['canvas'] if r['applied'] else np.full_like(got[n], case['pad_val'])
        assert got[n].shape == want.shape
        assert got[n].tobytes() == want.tobytes(), (case['name'], n, float(np.abs(got[n] - want).max()))


# ------------------------------------------------------------------ (c) the whole pipeline
PHOTO = dict(type='PhotoMetricDistortion', brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
             hue_delta=18)
LISTS = {'fixed': dict(resize=dict(img_scale=(160, 160), keep_ratio=False)),
         'square_range': dict(resize=dict(img_scale=(96, 224), multiscale_mode='square_range', keep_ratio=False)),
         'post_photo': dict(resize=dict(img_scale=(160, 160), keep_ratio=False), photo='post')}


def plain_list(resize, photo=None):
    lst = LOAD + tail(resize)
    if photo == 'post':
        lst.insert(5, dict(PHOTO))
    return lst


def unit_ratio_sources(rng, n, S):
    """Sources whose longer side is S: the keep-ratio resize of Mosaic is the identity, so the canvas holds uint8 values
    and can be stored as an ordinary source image."""
    srcs = []
    for i in range(n):
        short = int(rng.integers(S // 3, S + 1))
        h, w = (S, short) if i % 2 else (short, S)
        srcs.append(P.synth_image(rng, h, w, int(rng.integers(1, 14))))
    return srcs


def same_batch(a, b):
    assert a['img'].shape == b['img'].shape and torch.equal(a['img'], b['img'])
    for k in ('gt_bboxes', 'gt_keypointss'):
        assert torch.equal(a[k].padded, b[k].padded), k
        assert torch.equal(a[k].counts, b[k].counts), k
    assert a['img_metas'] == b['img_metas']


@pytest.mark.parametrize('name', list(LISTS))
def test_pipeline_equals_existing_pipeline_on_materialised_canvases(name):
    """DevicePipeline([... Mosaic ...]) on a resident store == the pipeline WITHOUT Mosaic on a store whose images are
    the canvases (composed on the CPU from the same draws) and whose GT is the merged GT: the later stages see the
    canvas as their source.  Batch image, GT, counts, metas and decide params bit-identical."""
    from yunet_amd.pipelines import DevicePipeline, SourceBatch
    S, seed, it, n = 128, 21, 4, 12
    rng = np.random.default_rng(77)
    srcs = unit_ratio_sources(rng, 9, S)
    idx = [int(i) for i in rng.integers(0, len(srcs), n)]
    mosaic = dict(type='Mosaic', img_scale=(S, S), use_kps=True, prob=0.75, pad_val=114)
    kw = LISTS[name]
    pm = DevicePipeline(mosaic_list(mosaic, kw['resize'], kw.get('photo')), seed=seed, gmax=64)
    a = pm(make_store(srcs).batch(idx), it)
    torch.cuda.synchronize()
    assert pm.check() == []
    case = dict(seed=seed, iteration=it, S=S, idx=idx, prob=0.75, center=(0.5, 1.5), clip=True, skip_filter=True,
                min_bbox_size=0, pad_val=114)
    ref = MR.run_case(case, srcs)
    assert 0 < sum(r['applied'] for r in ref) < n, 'both outcomes of the prob draw'
    imgs, boxes, kps = [], [], []
    for own, r in zip(idx, ref):
        if r['applied']:
            assert np.array_equal(r['canvas'], np.rint(r['canvas'])) and r['canvas'].min() >= 0 and r['canvas'].max() <= 255
            imgs.append(r['canvas'].astype(np.uint8))
        else:
            imgs.append(srcs[own][0])
        boxes.append(r['boxes'])
        kps.append(r['kps'])
    pe = DevicePipeline(plain_list(kw['resize'], kw.get('photo')), seed=seed, gmax=256)
    b = pe(SourceBatch.from_lists(imgs, boxes, kps, DEV), it)
    torch.cuda.synchronize()
    same_batch(a, b)
    assert torch.equal(pm.params, pe.params)
    assert int(a['gt_bboxes'].counts.sum()) > 0 and a['gt_bboxes'].padded.shape[1] == 256


def test_pipeline_vs_numpy_outer_stage_on_the_float_canvas():
    """General resize ratios (the canvas is not integer-valued): the batch image == crop (pad 128) -> cv2 float bilinear
    -> flip of the CPU-composed float canvas under the params the device decided, bit for bit; the GT == the crop /
    resize / flip arithmetic of oracle/pipeline_oracle.py on the merged GT."""
    from yunet_amd.pipelines import DevicePipeline
    _, stores = MR.load_fixture()
    srcs = stores['main']
    S, out, seed, it = 160, 128, 5, 2
    idx = list(range(len(srcs)))
    pm = DevicePipeline(mosaic_list(dict(type='Mosaic', img_scale=(S, S), use_kps=True),
                                    dict(img_scale=(out, out), keep_ratio=False)), seed=seed, gmax=64)
    a = pm(make_store(srcs).batch(idx), it)
    torch.cuda.synchronize()
    params, img = pm.params.cpu().numpy(), a['img'].cpu().numpy()
    gb, gk, cnt = (t.cpu().numpy() for t in (a['gt_bboxes'].padded, a['gt_keypointss'].padded, a['gt_bboxes'].counts))
    case = dict(seed=seed, iteration=it, S=S, idx=idx, prob=1.0, center=(0.5, 1.5), clip=True, skip_filter=True,
                min_bbox_size=0, pad_val=114)
    checked = 0
    for n, r in enumerate(MR.run_case(case, srcs)):
        left, top, cw, flip = (int(v) for v in params[n, :4])
        st = P.Stream(seed, it, n)
        dec = P.decide_crop(2 * S, 2 * S, r['boxes'], MR.CROP_CHOICE, st)
        if dec is None:                     # a mosaic without GT: no window, as for a source image without GT
            assert cw == 0 and int(params[n, 6]) == 1
            continue
        assert dec == (left, top, cw) and int(params[n, 6]) == 0
        checked += 1
        assert (st.uniform() < 0.5) == bool(flip)
        im = P.resize_linear(P.crop_image(r['canvas'], left, top, cw, 128.0), out)
        b, k, _ = P.crop_gt(r['boxes'], r['kps'], left, top, cw)
        b, k = P.resize_gt(b, k, cw, out)
        if flip:
            im = im[:, ::-1]
            b, k = P.flip_gt(b, k, out)
        assert img[n].tobytes() == np.ascontiguousarray(im.transpose(2, 0, 1)).tobytes(), n
        assert int(cnt[n]) == len(b) and gb[n, :len(b)].tobytes() == b.tobytes() and gk[n, :len(b)].tobytes() == k.tobytes()
    assert checked >= 10


# ------------------------------------------------------------------ (d) prob = 0
@pytest.mark.parametrize('name', list(LISTS))
def test_prob_zero_is_the_pipeline_without_mosaic(name):
    """Every image skipped: the batch is the one the list without Mosaic gives -- the crop / size / flip / photometric
    sub-streams do not move when Mosaic is present."""
    from yunet_amd import _lib as L
    from yunet_amd.pipelines import DevicePipeline
    _, stores = MR.load_fixture()
    srcs = [s for s in stores['main'] if len(s[1])]
    idx = [0, 3, 3, 1, 5, 2, 7, 4, 6]
    kw = LISTS[name]
    store = make_store(srcs)
    pm = DevicePipeline(mosaic_list(dict(type='Mosaic', img_scale=(160, 160), use_kps=True, prob=0.0), kw['resize'],
                                    kw.get('photo')), seed=9, gmax=64)
    pe = DevicePipeline(plain_list(kw['resize'], kw.get('photo')), seed=9, gmax=256)
    for it in (0, 5):
        a, b = pm(store.batch(idx), it), pe(store.batch(idx), it)
        torch.cuda.synchronize()
        same_batch(a, b)
        assert torch.equal(pm.params, pe.params)
        assert not pm.geom[:, L.MOSAIC_APPLIED].any() and (pm.geom[:, L.MOSAIC_DRAWS] == 4).all()
        if pm.photo is not None:
            assert torch.equal(pm.pparams, pe.pparams)


def test_mosaic_changes_the_batch_and_is_deterministic():
    from yunet_amd.pipelines import DevicePipeline
    _, stores = MR.load_fixture()
    store = make_store(stores['main'])
    idx = list(range(12))
    pm = DevicePipeline(mosaic_list(dict(type='Mosaic', img_scale=(160, 160), use_kps=True),
                                    dict(img_scale=(160, 160), keep_ratio=False)), seed=2)
    a = pm(store.batch(idx), 1)
    ga = pm.geom.clone()
    b = pm(store.batch(idx), 1)
    torch.cuda.synchronize()
    same_batch(a, b)
    assert torch.equal(ga, pm.geom)
    c = pm(store.batch(idx), 2)
    assert not torch.equal(a['img'], c['img']) and not torch.equal(ga[:, 1:3], pm.geom[:, 1:3])
    assert float(a['img'].min()) >= 0.0 and float(a['img'].max()) <= 255.0


# ------------------------------------------------------------------ (e) a short training run
def test_train_cli_runs_with_mosaic(tmp_path):
    """tools/train.py on synthetic resident sources with the MultiImageMixDataset spelling: finite losses, a clean
    pipeline status, and the engine planning for the four-image GT capacity."""
    spec = importlib.util.spec_from_file_location('yunet_train_tool_mosaic', os.path.join(ROOT, 'tools', 'train.py'))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    cfg = tmp_path / 'yunet_s_mosaic.py'
    cfg.write_text(open(os.path.join(ROOT, 'configs', 'yunet_s.py')).read() + '''
data['train'] = dict(type='MultiImageMixDataset',
                     dataset=dict(type='SyntheticSourceImages', pipeline=train_pipeline[:2], pool=6,
                                  src_hw=((300, 420), (512, 384), (200, 200))),
                     pipeline=[dict(type='Mosaic', img_scale=(320, 320), use_kps=True, prob=0.9)] + train_pipeline[2:])
''')
    hist = T.main([str(cfg), '--work-dir', str(tmp_path / 'w'), '--seed', '3', '--no-validate', '--max-iters', '4',
                   '--cfg-options', 'data.samples_per_gpu=8', 'log_config.interval=1'])
    losses = [h['loss'] for h in hist if 'loss' in h]
    assert len(losses) >= 4 and all(np.isfinite(losses)), hist
    src = T.main.last_source
    assert src.pipe.mosaic is not None and src.pipe.gmax == 256
    assert src.pipe.check() == []
    assert int(src.pipe.geom[:, 0].sum()) > 0, 'the last batch holds mosaics'
    out = src.batch(9, 'cuda')         # the engine plans by the padded GT's row count (Engine.get_plan)
    torch.cuda.synchronize()
    assert out['gt_bboxes'].padded.shape[1] == 256 and out['gt_keypointss'].padded.shape[1] == 256
