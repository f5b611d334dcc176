"""CPU: Mosaic(use_kps=True) -- the numpy restatement tests/mosaic_ref.py against tests/golden/mosaic_cases.npz (made
by the unmodified reference Mosaic / MultiImageMixDataset classes, tools/make_golden_mosaic.py): integers exact, floats
bit for bit; the live reference classes against the same fixture where the reference tree is available; the host-side
partner draw; and the config surface (MultiImageMixDataset spelling, flat list, refusals)."""
import os
import sys

import numpy as np
import pytest

import mosaic_ref as MR
import pipeline_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOAD = [dict(type='LoadImageFromFile', to_float32=True),
        dict(type='LoadAnnotations', with_bbox=True, with_keypoints=True)]
MOSAIC = dict(type='Mosaic', img_scale=(320, 320), use_kps=True)
PHOTO = dict(type='PhotoMetricDistortion')


def tail(resize=None):
    return [dict(type='RandomSquareCrop', crop_choice=MR.CROP_CHOICE),
            dict(type='Resize', **(resize or dict(img_scale=(320, 320), keep_ratio=False))),
            dict(type='RandomFlip', flip_ratio=0.5),
            dict(type='Normalize', mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False),
            dict(type='DefaultFormatBundle'),
            dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_keypointss'])]


def mosaic_list(mosaic=None, resize=None, photo=None):
    lst = LOAD + [dict(mosaic or MOSAIC)] + tail(resize)
    if photo == 'post':
        lst.insert(6, dict(PHOTO))
    return lst


def check_against_fixture(z, case, n, r):
    key = f"{case['name']}/{n}/"
    meta = [int(v) for v in z[key + 'meta']]
    assert r['partners'] == meta[:3], key
    assert [int(r['applied']), r['cx'], r['cy'], r['draws']] == meta[3:], key
    assert np.array_equal(np.asarray(r['geom'], np.int64), z[key + 'geom']), key
    assert np.array_equal(np.asarray(r['kept'], np.int64), z[key + 'kept']), key
    for name in ('boxes', 'kps'):
        got = np.ascontiguousarray(r[name], dtype=np.float32)
        assert got.shape == z[key + name].shape and got.tobytes() == z[key + name].tobytes(), key + name
    if r['applied'] and r.get('canvas') is not None:
        c = r['canvas'].astype(np.float64)
        assert np.array_equal(np.stack([c.sum((0, 1)), (c ** 2).sum((0, 1))]), z[key + 'digest']), key
        cx, cy = r['cx'], r['cy']
        assert r['canvas'][max(cy - 8, 0):cy + 8, max(cx - 8, 0):cx + 8].tobytes() == z[key + 'patch'].tobytes(), key


@pytest.mark.parametrize('row', MR.CASES, ids=[r[0] for r in MR.CASES])
def test_restatement_reproduces_the_reference_fixture(row):
    z, stores = MR.load_fixture()
    case = MR.case_dict(row)
    out = MR.run_case(case, stores[case['store']])
    assert len(out) == len(case['idx'])
    for n, r in enumerate(out):
        check_against_fixture(z, case, n, r)


def test_fixture_contains_the_hard_cases():
    """What the generator asserts when it writes the file, read back from the file: a change of seed must not leave the
    comparisons vacuous."""
    z, stores = MR.load_fixture()
    seen = dict(skipped=0, applied=0, empty_paste=0, over64=0, empty_merged=0, absent=0, dropped=0, unclipped=0, twice=0)
    shapes = set()
    for row in MR.CASES:
        case = MR.case_dict(row)
        for n, own in enumerate(case['idx']):
            key = f"{case['name']}/{n}/"
            meta, g, b = z[key + 'meta'], z[key + 'geom'], z[key + 'boxes']
            seen['applied' if meta[3] else 'skipped'] += 1
            if not meta[3]:
                continue
            seen['empty_paste'] += int(((g[:, 6] <= g[:, 4]) | (g[:, 7] <= g[:, 5])).sum())
            seen['over64'] += int(len(b) > 64)
            seen['empty_merged'] += int(len(b) == 0)
            seen['absent'] += int((z[key + 'kps'][:, :, 2] < 0).any())
            seen['dropped'] += int(g[:, 10].sum()) - len(b)
            seen['unclipped'] += int(((b < 0) | (b > 2 * case['S'])).any())
            seen['twice'] += int(len(set(meta[:3].tolist() + [own])) < 4)
            for h, w, rw, rh in g[:, :4]:
                shapes.add(('portrait' if h > w else 'landscape' if w > h else 'square',
                            'larger' if max(h, w) > case['S'] else 'smaller' if max(h, w) < case['S'] else 'equal'))
    assert all(v > 0 for v in seen.values()), seen
    assert {('portrait', 'larger'), ('landscape', 'larger'), ('landscape', 'smaller'), ('square', 'smaller')} <= shapes
    centres = {tuple(z[f'{name}/0/meta'][4:6]) for name in ('lo_end', 'hi_end', 'corner0', 'corner2')}
    assert centres == {(80, 80), (240, 240), (0, 0), (320, 320)}


def test_live_reference_classes_against_the_fixture():
    """The unmodified reference classes, run now, give the file (where the reference tree is available)."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import ref_stub
    if not ref_stub.available():
        pytest.skip('reference tree not available')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_golden_mosaic as G
    log = {}
    T, W = G.load_reference(log)
    z, stores = MR.load_fixture()
    for row in MR.CASES:
        case = MR.case_dict(row)
        for n, r in enumerate(G.run_reference(T, W, log, case, stores[case['store']])):
            check_against_fixture(z, case, n, r)


def test_host_partner_draw_is_the_sub_stream():
    """pipelines.mosaic_partners (what a lazily decoding source uses to decode partners ahead) is the first three
    draws of the mosaic sub-stream, which the fixture pins against the reference's get_indexes."""
    from yunet_amd import _lib as L
    from yunet_amd.pipelines import mosaic_partners
    assert L.MOSAIC_SALT == MR.MOSAIC_SALT
    z, _ = MR.load_fixture()
    for row in MR.CASES:
        case = MR.case_dict(row)
        m = len(MR.SOURCES if case['store'] == 'main' else MR.EMPTY_SOURCES)
        for n in range(len(case['idx'])):
            want = [int(v) for v in z[f"{case['name']}/{n}/meta"][:3]]
            assert mosaic_partners(case['seed'], case['iteration'], n, m) == want
    for m in (1, 7, 12880):
        assert all(0 <= j < m for n in range(50) for j in mosaic_partners(3, 9, n, m))
    # the other sub-streams do not move: the crop stream of an image is keyed without the salt
    assert MR.MosaicStream(5, 6, 7).key != P.Stream(5, 6, 7).key


def test_header_constants_match_the_binding():
    import re
    from yunet_amd import _lib as L
    txt = open(os.path.join(ROOT, 'include', 'yunet_hip.h')).read()
    defs = {k: int(v, 0) for k, v in re.findall(r'#define\s+(YUNET_MOSAIC_\w+)\s+(0x[0-9A-Fa-f]+|\d+)', txt)}
    for name, val in defs.items():
        assert getattr(L, name[len('YUNET_'):]) == val, name
    assert len(defs) >= 20 and L.MOSAIC_QUAD + 4 * L.MOSAIC_QWORDS == L.MOSAIC_WORDS


# ------------------------------------------------------------------ config surface
def test_flat_list_parses():
    from yunet_amd.pipelines import DevicePipeline, Mosaic
    pipe = DevicePipeline(mosaic_list(), seed=3, gmax=64)
    assert isinstance(pipe.mosaic, Mosaic) and pipe.gmax == 256 and pipe.cfg.gmax == 256
    c = pipe.mosaic_cfg
    assert (c.img_scale, c.gmax, c.center_lo, c.center_hi, c.prob, c.pad_val, c.skip_filter, c.bbox_clip_border) == \
        (320, 256, 0.5, 1.5, 1.0, 114.0, 1, 1)
    assert [type(s).__name__ for s in pipe.steps] == DevicePipeline.ORDER
    ms = DevicePipeline(mosaic_list(resize=dict(img_scale=(160, 320), multiscale_mode='square_range', keep_ratio=False)))
    assert ms.mosaic is not None and ms.scale_range == (160, 320)
    post = DevicePipeline(mosaic_list(photo='post'))
    assert post.mosaic is not None and post.photo is not None
    assert DevicePipeline(LOAD + tail()).mosaic is None
    m = Mosaic(img_scale=(640, 640), center_ratio_range=(0.25, 1.75), min_bbox_size=4, bbox_clip_border=False,
               skip_filter=False, pad_val=0, prob=0.5, use_kps=True)
    c = m.c_cfg(7, 128)
    assert (c.img_scale, c.center_lo, c.center_hi, c.min_bbox_size, c.bbox_clip_border, c.skip_filter, c.pad_val, c.prob,
            c.seed, c.gmax) == (640, 0.25, 1.75, 4.0, 0, 0, 0.0, 0.5, 7, 128)


def test_wrong_places_and_arguments_raise():
    from yunet_amd.pipelines import DevicePipeline, Mosaic
    t = tail()
    wrong = [[dict(MOSAIC)] + LOAD + t,                                   # before the loading steps
             LOAD[:1] + [dict(MOSAIC)] + LOAD[1:] + t,                    # between them
             LOAD + t[:1] + [dict(MOSAIC)] + t[1:],                       # after RandomSquareCrop
             LOAD + t[:3] + [dict(MOSAIC)] + t[3:],                       # after RandomFlip
             LOAD + t + [dict(MOSAIC)]]                                   # last
    for lst in wrong:
        with pytest.raises(NotImplementedError, match='between LoadAnnotations and RandomSquareCrop'):
            DevicePipeline(lst)
    with pytest.raises(NotImplementedError, match='one Mosaic'):
        DevicePipeline(LOAD + [dict(MOSAIC), dict(MOSAIC)] + t)
    with pytest.raises(NotImplementedError, match='use_kps=False'):
        DevicePipeline(mosaic_list(dict(type='Mosaic', img_scale=(320, 320))))
    with pytest.raises(NotImplementedError, match='use_kps=False'):
        Mosaic(use_kps=False)
    with pytest.raises(NotImplementedError, match='square canvas'):
        Mosaic(img_scale=(320, 640), use_kps=True)
    with pytest.raises(NotImplementedError, match='distort the mosaic canvas'):      # PRE photometric on the canvas
        DevicePipeline(LOAD + [dict(MOSAIC), dict(PHOTO)] + t)
    with pytest.raises(NotImplementedError):                                         # photometric before Mosaic
        DevicePipeline(LOAD + [dict(PHOTO), dict(MOSAIC)] + t)
    with pytest.raises(ValueError, match='1024'):
        DevicePipeline(mosaic_list(), gmax=512)
    assert DevicePipeline(mosaic_list(), gmax=256).gmax == 1024
    for bad in (dict(center_ratio_range=(0.5, 2.5)), dict(center_ratio_range=(1.0, 0.5)), dict(prob=1.5),
                dict(img_scale=(0, 0)), dict(pad_val=float('nan'))):
        with pytest.raises(ValueError):
            Mosaic(use_kps=True, **bad)


def test_non_resident_sources_raise():
    import yunet_amd.runner as R
    from yunet_amd.datasets import RetinaFaceSource
    from yunet_amd.pipelines import DevicePipeline
    from yunet_amd.source_store import SourceStore, WindowFeed
    lst = mosaic_list()
    R.SyntheticSourceImages(lst, samples_per_gpu=2)                                    # resident: accepted
    for kw in (dict(host_fed=True), dict(host_fed='window'), dict(host_fed='window', host_fetch='kernel')):
        with pytest.raises(NotImplementedError, match='not on the device'):
            R.SyntheticSourceImages(lst, samples_per_gpu=2, **kw)
    for cache in (None, 'host'):
        with pytest.raises(NotImplementedError, match='not on the device'):
            RetinaFaceSource(dataset=None, pipeline=lst, cache=cache)                  # raised before the dataset is read
    pipe = DevicePipeline(lst)
    with pytest.raises(NotImplementedError, match='not on the device'):
        WindowFeed(pipe, SourceStore([(4, 4)], placement='host', device='cpu'), 64)
    with pytest.raises(NotImplementedError, match='not on the device'):
        pipe.window_plan(None, 0, 'cpu')
    with pytest.raises(NotImplementedError, match='not on the device'):
        pipe.windowed(None, 0, None, None, None)


def test_multi_image_mix_dataset_spelling(tmp_path):
    """The reference's own spelling: the wrapper registered as a dataset, and tools/train.py's source builder flattening
    it into the list DevicePipeline takes."""
    import yunet_amd
    from yunet_amd.builder import DATASETS
    from yunet_amd.datasets import MultiImageMixDataset, flatten_multi_image_mix
    from yunet_amd.pipelines import DevicePipeline
    assert DATASETS.get('MultiImageMixDataset') is MultiImageMixDataset
    inner = dict(type='RetinaFaceDataset', ann_file='a.txt', img_prefix='imgs/', pipeline=LOAD)
    wrapper = dict(type='MultiImageMixDataset', dataset=inner, pipeline=[dict(MOSAIC)] + tail(), cache='device')
    flat = flatten_multi_image_mix(wrapper)
    assert flat['type'] == 'RetinaFaceDataset' and flat['cache'] == 'device' and flat['ann_file'] == 'a.txt'
    assert [p['type'] for p in flat['pipeline']] == [p['type'] for p in mosaic_list()]
    assert DevicePipeline(flat['pipeline']).mosaic is not None
    assert inner['pipeline'] == LOAD, 'the wrapped configuration is not edited in place'
    with pytest.raises(RuntimeError, match='dynamic_scale'):
        flatten_multi_image_mix(dict(wrapper, dynamic_scale=(320, 320)))
    with pytest.raises(NotImplementedError, match='skip_type_keys'):
        flatten_multi_image_mix(dict(wrapper, skip_type_keys=['Mosaic']))
    # tools/train.py: the wrapper around the synthetic decoded sources builds a resident source with Mosaic in its pipeline
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as T
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    cfg.merge_from_dict({'data.train': dict(type='MultiImageMixDataset',
                                            dataset=dict(type='SyntheticSourceImages', pipeline=LOAD, pool=8),
                                            pipeline=[dict(MOSAIC)] + tail())})
    src = T.build_source(cfg, 0, 1, 0)
    assert type(src).__name__ == 'SyntheticSourceImages' and src.pipe.mosaic is not None and src.pool == 8
    cfg.data.train['host_fed'] = True
    with pytest.raises(NotImplementedError, match='not on the device'):
        T.build_source(cfg, 0, 1, 0)
