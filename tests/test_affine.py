"""CPU: RandomAffine with landmarks in the device train pipeline -- the restatement (tests/affine_ref.py) against the
fixture made by the unmodified reference class (tools/make_golden_affine.py), the constructor's refusals, the place
DevicePipeline accepts, the entry points' refusals and the C layout of YunetAffineCfg.

Tolerances come from the fixture: bar_matrix / bar_gt are twice the largest distance of the reference's own float32
matrix / boxes from the float64 evaluation of the same formulas (another float32 summation order is as valid as the
reference's), bar_pixels four times the distance of the float32 pixel restatement from the float64 one."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import affine_ref as R
from test_photometric import BASE, PMD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'affine_cases.npz')
HEADER = os.path.join(ROOT, 'include', 'yunet_hip.h')
MOSAIC = dict(type='Mosaic', img_scale=(640, 640), use_kps=True)
CUT = dict(type='CutOut', n_holes=(0, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.2)])
AFF = dict(type='RandomAffine', use_kps=True)


def golden():
    g = np.load(GOLD)
    assert str(g['configs']) == repr(R.CONFIGS) and int(g['seed']) == R.SEED and float(g['margin']) == R.MARGIN, \
        'tests/golden/affine_cases.npz was made from other cases than affine_ref.CONFIGS'
    return g


def cases():
    return [(name, e) for name in R.CONFIGS for e in R.EDGES]


def with_affine(at, base=BASE, **kw):
    cfg = [dict(p) for p in base]
    cfg.insert(at, dict(AFF, **kw))
    return cfg


# ------------------------------------------------------------------ restatement vs fixture
def test_fixture_inputs_are_the_restated_inputs():
    g = golden()
    for e in R.EDGES:
        boxes, kps, counts = R.inputs(e)
        assert g[f'boxes_{e}'].tobytes() == boxes.tobytes() and g[f'kps_{e}'].tobytes() == kps.tobytes()
        assert np.array_equal(g[f'counts_{e}'], counts) and counts.max() == R.GMAX and boxes.shape[0] == R.N_IMAGES
        for i, c in enumerate(counts):
            assert not boxes[i, c:].any() and not kps[i, c:].any()
            assert (boxes[i, :c, 2] > boxes[i, :c, 0]).all() and (boxes[i, :c, 3] > boxes[i, :c, 1]).all()


@pytest.mark.parametrize('name,edge', cases())
def test_restatement_against_the_reference_fixture(name, edge):
    """Draws bit-equal; the float32 restatement and the reference's matrix / boxes within the bar of the float64
    evaluation; survivors identical in float32 and in float64; every decision clear of its thresholds by more than the
    bar (the condition under which the survivor set cannot depend on the summation order)."""
    g, cfg = golden(), R.CONFIGS[name]
    it = int(g[f'it_{name}_{edge}'])
    boxes, kps, counts = g[f'boxes_{edge}'], g[f'kps_{edge}'], g[f'counts_{edge}']
    bar_m, bar_g = float(g[f'bar_matrix_{edge}']), float(g[f'bar_gt_{edge}'])
    print(f'{name} edge {edge}: iteration {it}, bar matrix {bar_m:.3e}, bar gt {bar_g:.3e}')
    assert 0 < bar_m < R.MARGIN and 0 < bar_g < R.MARGIN
    for i in range(R.N_IMAGES):
        c = int(counts[i])
        want_d, want_M = g[f'draws_{name}_{edge}'][i], g[f'M_{name}_{edge}'][i]
        want_wb, want_v = g[f'wb_{name}_{edge}'][i, :c], g[f'valid_{name}_{edge}'][i, :c]
        r64 = R.decide(R.SEED, it, i, boxes[i, :c], kps[i, :c], edge, cfg, np.float64)
        r32 = R.decide(R.SEED, it, i, boxes[i, :c], kps[i, :c], edge, cfg, np.float32)
        assert r64['draws'].tobytes() == want_d.tobytes(), f'image {i}: draws'
        assert want_M.dtype == np.float32 and np.array_equal(want_M[2], [0, 0, 1])
        dev = [np.abs(want_M - r64['M']).max(), np.abs(r32['M'] - r64['M']).max(),
               np.abs(want_wb - r64['wb']).max(initial=0), np.abs(r32['wb'] - r64['wb']).max(initial=0),
               np.abs(r32['kps'] - r64['kps']).max(initial=0)]
        print(f'  image {i}: |M_ref - M64| {dev[0]:.3e} |M32 - M64| {dev[1]:.3e} |wb_ref - wb64| {dev[2]:.3e} '
              f'|wb32 - wb64| {dev[3]:.3e} |kps32 - kps64| {dev[4]:.3e}')
        assert dev[0] <= bar_m / 2 and dev[1] <= bar_m and dev[2] <= bar_g / 2 and dev[3] <= bar_g and dev[4] <= bar_g
        assert np.array_equal(r64['valid'], want_v) and np.array_equal(r32['valid'], want_v), f'image {i}: survivors'
        assert r32['M'].dtype == np.float32 and r32['wb'].dtype == np.float32 and r32['kps'].dtype == np.float32
        assert np.array_equal(r32['kps'][:, :, 2], kps[i, :c, :, 2])
        clear = R.clearance(boxes[i, :c], want_d[1], r64['M'], edge, cfg)
        assert clear.min() > R.MARGIN > max(bar_m, bar_g), f'image {i}: a decision within {clear.min():.2e} of flipping'


def test_fixture_contains_the_hard_cases():
    g = golden()
    seen = dict(clip_left=False, clip_top=False, clip_right=False, clip_bottom=False, outside=False, rule_size=False,
                rule_area=False, rule_aspect=False, loses_all=False, keeps_all=False)
    for name, e in cases():
        cfg = R.full(R.CONFIGS[name])
        counts, boxes = g[f'counts_{e}'], g[f'boxes_{e}']
        for i in range(R.N_IMAGES):
            c = int(counts[i])
            wb, valid = g[f'wb_{name}_{e}'][i, :c], g[f'valid_{name}_{e}'][i, :c]
            ok = R.rules(boxes[i, :c], wb, g[f'draws_{name}_{e}'][i, 1], e, cfg)
            seen['loses_all'] |= not valid.any()
            seen['keeps_all'] |= bool(valid.all()) and c == R.GMAX
            seen['outside'] |= bool((~ok[:, 0]).any())
            for k, rule in ((1, 'rule_size'), (2, 'rule_area'), (3, 'rule_aspect')):
                seen[rule] |= bool((ok[:, 0] & ~ok[:, k] & np.delete(ok, k, 1).all(1)).any())
            if cfg['bbox_clip_border']:
                for k, (col, at) in dict(clip_left=(0, 0), clip_top=(1, 0), clip_right=(2, e), clip_bottom=(3, e)).items():
                    seen[k] |= bool((valid & (wb[:, col] == at)).any())
            else:
                assert name == 'unclipped'
    assert all(seen.values()), seen
    assert (g['wb_unclipped_32'] < 0).any() or (g['wb_unclipped_32'] > 32).any()        # really not clipped
    # the one-factor settings leave the other factors the identity
    assert np.array_equal(g['M_translate_64'][:, :2, :2], np.broadcast_to(np.eye(2, dtype=np.float32), (4, 2, 2)))
    assert not g['M_rotate_64'][:, :2, 2].any() and not g['M_shear_64'][:, :2, 2].any()
    assert np.array_equal(g['M_shear_64'][:, 0, 0], np.ones(4, np.float32))


def test_pixel_restatement_and_its_bar():
    """The float32 restatement stays within a quarter of the recorded bar of the float64 one on the fixture's cases, and
    equals hand-made cases exactly: identity, an integer shift, all taps outside."""
    g = golden()
    for e in R.EDGES:
        bar = float(g[f'bar_pixels_{e}'])
        imgs, worst = R.pattern(R.N_IMAGES, e), 0.0
        for name in R.CONFIGS:
            bv = R.full(R.CONFIGS[name])['border_val']
            for i in range(R.N_IMAGES):
                inv = R.inverse(g[f'M_{name}_{e}'][i])
                worst = max(worst, float(np.abs(R.warp_pixels(imgs[i], inv, bv, np.float32).astype(np.float64)
                                                - R.warp_pixels(imgs[i], inv, bv, np.float64)).max()))
        print(f'edge {e}: pixel bar {bar:.3e}, float32 restatement within {worst:.3e}')
        assert 0 < worst <= bar / 4 * (1 + 1e-12) and bar < 0.05
    img = R.pattern(1, 32)[0]
    assert R.warp_pixels(img, [1, 0, 0, 0, 1, 0], (1, 2, 3), np.float32).tobytes() == img.tobytes()
    out = R.warp_pixels(img, [1, 0, -3, 0, 1, 2], (1, 2, 3), np.float32)       # M shifts by (+3, -2)
    assert np.array_equal(out[:, :30, 3:], img[:, 2:, :29])
    assert (out[:, 30:, :] == np.array([1, 2, 3], np.float32).reshape(3, 1, 1)).all() and (out[0, :, :3] == 1).all()
    out = R.warp_pixels(img, [1, 0, 500, 0, 1, 0], (1, 2, 3), np.float32, S=16)
    assert (out[1, :16, :16] == 2).all() and not out[:, 16:].any() and not out[:, :, 16:].any()


def test_sub_stream_is_keyed_apart_and_leaves_the_other_streams_alone():
    import cutout_ref
    import mosaic_ref
    import photometric_ref
    import pipeline_oracle as P
    st = R.AffineStream(9, 4, 2)
    assert st.key == P.mix32(P.stream_key(9, 4, 2) ^ R.SALT)
    keys = {st.key, P.Stream(9, 4, 2).key, photometric_ref.photo_key(9, 4, 2), cutout_ref.cutout_key(9, 4, 2),
            mosaic_ref.MosaicStream(9, 4, 2).key}
    assert len(keys) == 5 and len({R.SALT, cutout_ref.SALT, 0x50484D44, 0x4D4F5341}) == 4
    # the draws of the other sub-streams are functions of their own key alone: pinned values from before the new salt
    assert cutout_ref.holes(cutout_ref.SEED, cutout_ref.ITERATION + 1, 0, 64, 64, dict(n_holes=3, cutout_shape=(10, 7))).tolist()[:6] == \
        np.load(os.path.join(ROOT, 'tests', 'golden', 'cutout.npz'))['holes_fixed_shape_64'][0, :6].tolist()
    d = R.draws(9, 4, 2, {})
    assert st.ctr == 0 and len(d) == 6 and -10 <= d[0] <= 10 and 0.5 <= d[1] <= 1.5 and abs(d[4]) <= 0.1
    assert d.tobytes() == R.draws(9, 4, 2, {}).tobytes() and d.tobytes() != R.draws(9, 5, 2, {}).tobytes()
    assert R.draws(9, 4, 2, dict(max_rotate_degree=0.0))[0] == 0.0


def test_restatement_equals_the_live_reference():
    """Where the reference tree is available: the unmodified class, fed from the sub-stream, on cases beyond the fixture."""
    import ref_stub
    if not ref_stub.available():
        pytest.skip('reference tree not available')
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_affine', os.path.join(ROOT, 'tools', 'make_golden_affine.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    log = {}
    T = tool.load_reference(log)
    ours = inspect.signature(__import__('yunet_amd.pipelines', fromlist=['RandomAffine']).RandomAffine.__init__).parameters
    theirs = inspect.signature(T.RandomAffine.__init__).parameters
    assert [(k, v.default) for k, v in ours.items()] == [(k, v.default) for k, v in theirs.items()] + [('use_kps', False)]
    cfg = dict(max_rotate_degree=25.0, max_translate_ratio=0.2, skip_filter=False)
    boxes, kps, counts = R.inputs(64)
    draws, Ms, wbs, valid = tool.run_reference(T, log, cfg, boxes, counts, 64, 77, 12)
    g = golden()
    for i in range(R.N_IMAGES):
        c = int(counts[i])
        r = R.decide(77, 12, i, boxes[i, :c], kps[i, :c], 64, cfg, np.float64)
        assert r['draws'].tobytes() == draws[i].tobytes()
        assert np.abs(Ms[i] - r['M']).max() <= float(g['bar_matrix_64'])
        assert np.abs(wbs[i, :c] - r['wb']).max() <= float(g['bar_gt_64'])


# ------------------------------------------------------------------ constructor
def test_constructor_refusals_name_the_argument():
    from yunet_amd.pipelines import RandomAffine
    import yunet_amd._lib as L
    ok = RandomAffine(use_kps=True)
    assert ok.max_rotate_degree == 10.0 and ok.scaling_ratio_range == (0.5, 1.5) and ok.fill == (114.0, 114.0, 114.0)
    assert ok.border == (0, 0) and ok.skip_filter is True and ok.bbox_clip_border is True and ok.use_kps is True
    assert RandomAffine(border_val=7, use_kps=True, border=[0, 0]).fill == (7.0, 7.0, 7.0)
    assert RandomAffine(max_rotate_degree=-5, max_shear_degree=0, max_translate_ratio=1, use_kps=True).max_rotate_degree == -5
    bad = [
        (dict(max_translate_ratio=-0.1), 'max_translate_ratio'),
        (dict(max_translate_ratio=1.5), 'max_translate_ratio'),
        (dict(scaling_ratio_range=(1.5, 0.5)), 'scaling_ratio_range'),
        (dict(scaling_ratio_range=(0.0, 0.5)), 'scaling_ratio_range'),
        (dict(scaling_ratio_range=(-1.0, 0.5)), 'scaling_ratio_range'),
        (dict(scaling_ratio_range=(0.5, 1.0, 1.5)), 'scaling_ratio_range'),
        (dict(scaling_ratio_range=1.0), 'scaling_ratio_range'),
        (dict(scaling_ratio_range=(0.5, float('inf'))), 'scaling_ratio_range'),
        (dict(max_rotate_degree=float('nan')), 'max_rotate_degree'),
        (dict(max_rotate_degree='ten'), 'max_rotate_degree'),
        (dict(max_shear_degree=float('inf')), 'max_shear_degree'),
        (dict(max_shear_degree=L.AFFINE_MAX_SHEAR), 'YUNET_AFFINE_MAX_SHEAR'),
        (dict(max_translate_ratio=float('nan')), 'max_translate_ratio'),
        (dict(min_bbox_size=float('nan')), 'min_bbox_size'),
        (dict(min_area_ratio=float('inf')), 'min_area_ratio'),
        (dict(max_aspect_ratio=float('nan')), 'max_aspect_ratio'),
        (dict(border_val=(1, 2)), 'border_val'),
        (dict(border_val=(1, 2, float('nan'))), 'border_val'),
        (dict(border_val='grey'), 'border_val'),
        (dict(border=(0, 0, 0)), 'border'),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            RandomAffine(use_kps=True, **kw)
    with pytest.raises(NotImplementedError, match='use_kps=True'):
        RandomAffine()
    for border in ((-160, -160), (0, 8), [4, 0]):
        with pytest.raises(NotImplementedError, match=r'border=\(0, 0\)'):
            RandomAffine(border=border, use_kps=True)
    with pytest.raises(NotImplementedError, match='DevicePipeline'):
        RandomAffine(use_kps=True)({})


def test_c_cfg_carries_the_configuration():
    from yunet_amd.pipelines import RandomAffine
    c = RandomAffine(max_rotate_degree=15, max_translate_ratio=0.25, scaling_ratio_range=(0.75, 1.25), max_shear_degree=3,
                     border_val=(1.5, 2, 3), min_bbox_size=4, min_area_ratio=0.5, max_aspect_ratio=8,
                     bbox_clip_border=False, skip_filter=False, use_kps=True).c_cfg(0x1FFFFFFFF, 256)
    assert (c.max_rotate_degree, c.max_translate_ratio, c.scale_lo, c.scale_hi, c.max_shear_degree) == \
        (15.0, 0.25, 0.75, 1.25, 3.0)
    assert (c.min_bbox_size, c.min_area_ratio, c.max_aspect_ratio, list(c.border_val)) == (4.0, 0.5, 8.0, [1.5, 2.0, 3.0])
    assert (c.bbox_clip_border, c.skip_filter, c.gmax, c.seed) == (0, 0, 256, 0xFFFFFFFF)


def test_entry_points_refuse_on_the_host():
    """Every YUNET_EINVAL of the two entries is decided before any launch, so it shows without a GPU (the pointers are
    never dereferenced)."""
    from yunet_amd.pipelines import RandomAffine
    import yunet_amd._lib as L
    lib = L.load()
    a, b = C.c_void_p(4096), C.c_void_p(8192)

    def decide(c, n=4, edge=32, ins=(a, a, a), outs=(b, b, b), table=b):
        return lib.yunet_aug_affine_decide(C.byref(c) if c is not None else None, 0, n, edge, None, *ins, *outs, table, None)

    def cfg(**fields):
        c = RandomAffine(use_kps=True).c_cfg(0, 8)
        for k, v in fields.items():
            if k == 'border_val':
                c.border_val[1] = v
            else:
                setattr(c, k, v)
        return c
    nan, inf = float('nan'), float('inf')
    for what, c in {'translate < 0': cfg(max_translate_ratio=-0.5), 'translate > 1': cfg(max_translate_ratio=1.5),
                    'translate nan': cfg(max_translate_ratio=nan), 'scale 0': cfg(scale_lo=0.0),
                    'scale lo > hi': cfg(scale_lo=2.0), 'scale inf': cfg(scale_hi=inf), 'rotate nan': cfg(max_rotate_degree=nan),
                    'rotate inf': cfg(max_rotate_degree=inf), 'shear 45': cfg(max_shear_degree=45.0),
                    'shear -60': cfg(max_shear_degree=-60.0), 'shear nan': cfg(max_shear_degree=nan),
                    'size nan': cfg(min_bbox_size=nan), 'area inf': cfg(min_area_ratio=inf),
                    'aspect nan': cfg(max_aspect_ratio=nan), 'border nan': cfg(border_val=nan), 'gmax 0': cfg(gmax=0),
                    'gmax large': cfg(gmax=4097)}.items():
        assert decide(c) == L.EINVAL, what
    assert decide(None) == L.EINVAL and decide(cfg(), n=0) == L.EINVAL and decide(cfg(), n=-1) == L.EINVAL
    assert decide(cfg(), edge=0) == L.EINVAL and decide(cfg(), edge=L.AUG_MAX_EDGE + 1) == L.EINVAL
    for k in range(3):
        assert decide(cfg(), ins=tuple(None if j == k else a for j in range(3))) == L.EINVAL
        assert decide(cfg(), outs=tuple(None if j == k else b for j in range(3))) == L.EINVAL
        assert decide(cfg(), outs=tuple(a if j == k else b for j in range(3))) == L.EINVAL, 'an output that is its input'
    assert decide(cfg(), table=None) == L.EINVAL

    def pixels(table=a, bv=(114.0, 114.0, 114.0), n=4, edge=32, src=a, dst=b):
        return lib.yunet_aug_affine_pixels(table, C.byref((C.c_float * 3)(*bv)) if bv is not None else None, n, edge, None,
                                           src, dst, None)
    assert pixels(table=None) == L.EINVAL and pixels(bv=None) == L.EINVAL and pixels(src=None) == L.EINVAL
    assert pixels(dst=None) == L.EINVAL and pixels(dst=a) == L.EINVAL, 'the warp cannot run in place'
    assert pixels(n=0) == L.EINVAL and pixels(n=-2) == L.EINVAL and pixels(edge=0) == L.EINVAL
    assert pixels(edge=L.AUG_MAX_EDGE + 1) == L.EINVAL and pixels(bv=(1.0, nan, 3.0)) == L.EINVAL
    assert pixels(bv=(inf, 0.0, 0.0)) == L.EINVAL
    assert pixels(n=1 << 20, edge=L.AUG_MAX_EDGE) == L.EINVAL, 'more workgroups than a launch takes'


# ------------------------------------------------------------------ DevicePipeline
def test_device_pipeline_accepts_affine_at_its_place():
    from yunet_amd.pipelines import CutOut, DevicePipeline, RandomAffine
    plain = DevicePipeline(BASE, seed=1)
    assert plain.affine is None and plain.affine_cfg is None and plain.affine_table is None
    post = BASE[:5] + [PMD] + BASE[5:]
    lists = {'plain': with_affine(5),
             'post pmd': with_affine(6, base=post),
             'pre pmd': with_affine(6, base=BASE[:2] + [PMD] + BASE[2:]),
             'cutout': with_affine(5, base=BASE[:5] + [CUT] + BASE[5:]),
             'post pmd, cutout': with_affine(6, base=BASE[:5] + [PMD, CUT] + BASE[5:]),
             'mosaic': with_affine(6, base=BASE[:2] + [MOSAIC] + BASE[2:]),
             'mosaic, post pmd, cutout': with_affine(7, base=BASE[:2] + [MOSAIC] + BASE[2:5] + [PMD, CUT] + BASE[5:])}
    for what, cfg in lists.items():
        names = [c['type'] for c in cfg]
        at = names.index('RandomAffine')
        assert names[at + 1] == ('CutOut' if 'cutout' in what else 'Normalize'), what
        pipe = DevicePipeline(cfg, seed=1)
        assert isinstance(pipe.affine, RandomAffine) and pipe.affine_cfg.seed == 1 and pipe.affine_table is None, what
        assert pipe.affine_cfg.gmax == pipe.gmax == (256 if 'mosaic' in what else 64), what
        assert [type(s).__name__ for s in pipe.steps] == DevicePipeline.ORDER, what
        assert (pipe.photo is not None) == ('pmd' in what) and (pipe.mosaic is not None) == ('mosaic' in what)
        assert isinstance(pipe.cutout, CutOut) == ('cutout' in what), what
    ms = [dict(p) for p in with_affine(5)]
    ms[3] = dict(type='Resize', img_scale=(320, 640), multiscale_mode='square_range', keep_ratio=False)
    assert DevicePipeline(ms, seed=1, gmax=128).affine_cfg.gmax == 128


def test_device_pipeline_refuses_every_other_place():
    from yunet_amd.pipelines import DevicePipeline
    post = BASE[:5] + [PMD] + BASE[5:]
    cut = BASE[:5] + [CUT] + BASE[5:]
    wrong = {'before RandomFlip': with_affine(4),
             'before a POST PhotoMetricDistortion': with_affine(5, base=post),
             'after a PRE PhotoMetricDistortion': with_affine(3, base=BASE[:2] + [PMD] + BASE[2:]),
             'on the source image': with_affine(2),
             'after CutOut': with_affine(6, base=cut),
             'after Normalize': with_affine(6),
             'first': with_affine(0),
             'last': with_affine(len(BASE)),
             'twice': with_affine(5, base=with_affine(5)),
             'twice, apart': with_affine(4, base=with_affine(5))}
    for what, cfg in wrong.items():
        with pytest.raises(NotImplementedError, match='RandomAffine once, after RandomFlip'):
            DevicePipeline(cfg, seed=1)
    # the lists without it keep their own messages, and CutOut keeps its rule behind RandomAffine
    with pytest.raises(NotImplementedError, match=r'DevicePipeline implements exactly'):
        DevicePipeline(BASE[:4] + BASE[5:], seed=1)
    with pytest.raises(NotImplementedError, match='CutOut once, immediately in front of Normalize'):
        DevicePipeline(with_affine(6, base=BASE[:4] + [CUT] + BASE[4:]), seed=1)
    with pytest.raises(NotImplementedError, match='use_kps=True'):
        DevicePipeline(BASE[:5] + [dict(type='RandomAffine')] + BASE[5:], seed=1)
    with pytest.raises(NotImplementedError, match=r'border=\(0, 0\)'):
        DevicePipeline(with_affine(5, border=(-160, -160)), seed=1)


# ------------------------------------------------------------------ header / ctypes
def test_header_constants_and_struct_layout(tmp_path):
    import yunet_amd._lib as L
    txt = open(HEADER).read()
    defs = dict(re.findall(r'#define\s+(YUNET_AFFINE_\w+)\s+([\w.]+)', txt))
    assert int(defs['YUNET_AFFINE_SALT'].rstrip('u'), 16) == L.AFFINE_SALT == R.SALT
    assert bytes.fromhex('%08X' % L.AFFINE_SALT) == b'AFFI'
    assert int(defs['YUNET_AFFINE_WORDS']) == L.AFFINE_WORDS == R.WORDS == 24
    assert float(defs['YUNET_AFFINE_MAX_SHEAR']) == L.AFFINE_MAX_SHEAR == 45.0
    for name, ours, ref in (('DRAWS', L.AFFINE_DRAWS, R.DRAWS), ('M', L.AFFINE_M, R.MAT), ('INV', L.AFFINE_INV, R.INV),
                            ('ROWS_IN', L.AFFINE_ROWS_IN, R.ROWS_IN), ('ROWS_OUT', L.AFFINE_ROWS_OUT, R.ROWS_OUT),
                            ('EDGE', L.AFFINE_EDGE, R.EDGE)):
        assert int(defs[f'YUNET_AFFINE_{name}']) == ours == ref, name
    assert {'yunet_aug_affine_decide', 'yunet_aug_affine_pixels'} <= set(L.EXPORTED)
    assert L.load().yunet_abi_version() == 12                                               # additive: the number stays
    assert L._SIGNATURES['yunet_aug_affine_decide'][1][0] is C.POINTER(L.YunetAffineCfg)
    assert len(L._SIGNATURES['yunet_aug_affine_decide'][1]) == 13 and len(L._SIGNATURES['yunet_aug_affine_pixels'][1]) == 8
    fields = [f for f, _ in L.YunetAffineCfg._fields_]
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yunet_hip.h"\n'
                   'int main(){printf("%zu", sizeof(YunetAffineCfg));'
                   + ''.join(f'printf(" %zu", offsetof(YunetAffineCfg, {f}));' for f in fields) + 'return 0;}')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = L.YunetAffineCfg
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
