"""CPU: MixUp with landmarks and the YOLOX mode switch in the device train pipeline -- the restatement (tests/mixup_ref.py)
against the fixture made by the unmodified reference class (tools/make_golden_mixup.py), the constructor's refusals, the
place DevicePipeline accepts, the GT capacity, the entry points' refusals, the C layout of YunetMixupCfg, and
skip_type_keys through the wrapper, the sources and YOLOXModeSwitchHook.

Boxes, labels and draws are compared byte for byte: every step of the reference's box arithmetic is one float32
operation.  The pixels have no byte reference (cv2 is not at hand and its resize of the uint8 canvas is not pinned): a
pixel's admissible outputs are {trunc(0.5 a + 0.5 k) : trunc(b64 - bar) <= k <= trunc(b64 + bar)}, b64 the partner value
evaluated in float64 and bar four times the largest distance of the float32 evaluation from it over the fixture."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mixup_ref as R
from test_affine import AFF, CUT, MOSAIC
from test_photometric import BASE, PMD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'mixup_cases.npz')
HEADER = os.path.join(ROOT, 'include', 'yunet_hip.h')
MIX = dict(type='MixUp', img_scale=(320, 320), use_kps=True)


def golden():
    g = np.load(GOLD)
    assert str(g['configs']) == repr(R.CONFIGS) and int(g['seed']) == R.SEED and float(g['margin']) == R.MARGIN, \
        'tests/golden/mixup_cases.npz was made from other cases than mixup_ref.CONFIGS'
    return g


def cases():
    return [(name, e) for name in R.CONFIGS for e in R.EDGES]


def with_mix(at, base=BASE, **kw):
    cfg = [dict(p) for p in base]
    cfg.insert(at, dict(MIX, **kw))
    return cfg


def golden_store(g):
    n = len(g['store_hw'])
    return dict(hw=g['store_hw'], imgs=[g[f'img_{i}'] for i in range(n)], boxes=[g[f'sboxes_{i}'] for i in range(n)],
                kps=[g[f'skps_{i}'] for i in range(n)])


# ------------------------------------------------------------------ restatement vs fixture
def test_fixture_inputs_are_the_restated_inputs():
    g, s = golden(), R.store()
    assert np.array_equal(g['store_hw'], s['hw']) and len(s['imgs']) == 6
    assert sum(len(b) == 0 for b in s['boxes']) >= 2 and max(len(b) for b in s['boxes']) <= 8
    for i, im in enumerate(s['imgs']):
        assert im.dtype == np.uint8 and im.shape == (*R.STORE_HW[i], 3) and 24 <= min(im.shape[:2]) and max(im.shape[:2]) <= 64
        assert np.array_equal(g[f'img_{i}'], im) and g[f'sboxes_{i}'].tobytes() == s['boxes'][i].tobytes()
        assert g[f'skps_{i}'].tobytes() == s['kps'][i].tobytes()
    assert {h > w for h, w in R.STORE_HW} == {True, False}, 'both aspect ratios'
    for e in R.EDGES:
        b, k, c = R.own_inputs(e)
        assert g[f'own_boxes_{e}'].tobytes() == b.tobytes() and g[f'own_kps_{e}'].tobytes() == k.tobytes()
        assert np.array_equal(g[f'own_counts_{e}'], c)


@pytest.mark.parametrize('name,edge', cases())
def test_restatement_against_the_reference_fixture(name, edge):
    """Draws, partner, J, rw / rh and offsets equal the reference's; boxes and survivor sets are byte-equal to the
    unmodified class; every decision is clear of its thresholds on the reference's own numbers."""
    g = golden()
    store, (D, cfg), it = golden_store(g), R.case_cfg(name, edge), int(g[f'it_{name}_{edge}'])
    own_b, own_k, own_c = g[f'own_boxes_{edge}'], g[f'own_kps_{edge}'], g[f'own_counts_{edge}']
    for i in range(R.N_IMAGES):
        c = int(own_c[i])
        d = R.decide(R.SEED, it, i, store, own_b[i, :c], own_k[i, :c], edge, D, cfg)
        t = d['table']
        assert t.tobytes() == g[f'table_{name}_{edge}'][i].tobytes(), f'image {i}: table'
        drawn = g[f'draws_{name}_{edge}'][i]
        drawn = drawn[~np.isnan(drawn)]
        assert len(drawn) == t[R.DRAWS] and drawn[int(t[R.INDEX_DRAWS]) - 1] == t[R.PARTNER], f'image {i}: draws'
        if t[R.APPLIED]:
            n = int(t[R.INDEX_DRAWS])
            assert drawn[n] == t[R.JIT] and (drawn[n + 1] > R.full(cfg)['flip_ratio']) == bool(t[R.FLIP])
            assert t[R.J_] == int(D * t[R.JIT]) and len(drawn) == n + 2 + (2 if t[R.J_] > edge else 0)
            if t[R.J_] > edge:
                assert (drawn[n + 2], drawn[n + 3]) == (t[R.YOFF], t[R.XOFF]), 'y_offset is drawn first'
            h, w = store['hw'][int(t[R.PARTNER])]
            assert max(t[R.RW], t[R.RH]) in (D, D - 1) and abs(t[R.RW] / t[R.RH] - w / h) < 0.1
        k = int(g[f'rows_{name}_{edge}'][i])
        assert k == len(d['boxes']) == t[R.ROWS_OUT] and np.array_equal(g[f'labels_{name}_{edge}'][i, :k], d['labels'])
        assert g[f'boxes_{name}_{edge}'][i, :k].tobytes() == d['boxes'].tobytes(), f'image {i}: boxes'
        assert d['kps'].shape == (k, 5, 3) and d['kps'].dtype == np.float32
        own = d['labels'] < 1000
        assert d['kps'][own].tobytes() == own_k[i, :c][d['labels'][own]].tobytes(), 'own landmarks are copied'
        if t[R.APPLIED]:
            p = int(t[R.PARTNER])
            raw = store['kps'][p][d['labels'][~own] - 1000]
            src = raw[:, R.KP_FLIP] if t[R.FLIP] else raw
            assert np.array_equal(d['kps'][~own][:, :, 2], src[:, :, 2]), 'the third value rides along, permuted on a flip'
            if R.full(cfg)['bbox_clip_border']:
                assert d['kps'][~own][:, :, :2].min(initial=0) >= 0 and d['kps'][~own][:, :, :2].max(initial=0) <= edge
            # the reference's own surviving boxes decide as recorded, by the margin
            clear = R.clearance(t, store['boxes'][p], own_b[i, :c], cfg)
            assert clear.min(initial=np.inf) > R.MARGIN, f'image {i}: a decision within {R.MARGIN} of its threshold'
            b, cp = R.partner_boxes(t, store['boxes'][p], cfg)
            kept = R.rules(b, cp, np.float32(edge), cfg).all(1)
            assert g[f'boxes_{name}_{edge}'][i, :k][~own].tobytes() == cp[kept].tobytes()


def test_fixture_contains_the_hard_cases():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    g = golden()
    seen = dict(flipped=False, unflipped=False, larger=False, smaller=False, same=False, later_draw=False,
                not_applied=False, clip_J=False, clip_T=False, outside=False, size=False, area=False, aspect=False,
                unclipped=False)
    store = golden_store(g)
    for name, e in cases():
        D, cfg = R.case_cfg(name, e)
        c = R.full(cfg)
        assert D in (32, 48, 64) and e in (32, 64)
        for t in g[f'table_{name}_{e}']:
            if not t[R.APPLIED]:
                seen['not_applied'] |= c['max_iters'] == 1
                assert t[R.DRAWS] == t[R.INDEX_DRAWS] == c['max_iters'] or t[R.INDEX_DRAWS] == c['max_iters']
                continue
            J = int(t[R.J_])
            seen['flipped'] |= bool(t[R.FLIP])
            seen['unflipped'] |= not t[R.FLIP]
            seen['larger'] |= J > e and t[R.XOFF] > 0 and t[R.YOFF] > 0
            seen['smaller'] |= J < e
            seen['same'] |= J == e and t[R.DRAWS] == t[R.INDEX_DRAWS] + 2
            seen['later_draw'] |= t[R.INDEX_DRAWS] > 1
            raw = store['boxes'][int(t[R.PARTNER])]
            b, cp = R.partner_boxes(t, raw, cfg)
            ok = R.rules(b, cp, np.float32(e), cfg)
            kept = ok.all(1)
            seen['outside'] |= bool((~ok[:, 0] & ok[:, 1:].all(1)).any())
            for k, rule in ((1, 'size'), (2, 'area'), (3, 'aspect')):
                seen[rule] |= bool((~ok[:, k] & np.delete(ok, k, 1).all(1)).any())
            if c['bbox_clip_border']:
                scaled = np.asarray(raw, np.float32) * np.float32(t[R.SR])
                seen['clip_J'] |= bool((kept & (scaled > J).any(1)).any())
                seen['clip_T'] |= bool((kept & ((cp[:, 2] == e) | (cp[:, 3] == e))
                                        & (b[:, 2:] - [t[R.XOFF], t[R.YOFF]] > e).any(1)).any())
            else:
                seen['unclipped'] |= bool((kept & ((cp < 0) | (cp > e)).any(1)).any())
    assert all(seen.values()), {k for k, v in seen.items() if not v}


@pytest.mark.parametrize('edge', R.EDGES)
def test_pixel_yardstick_and_its_bar(edge):
    """The bar is four times the float32 restatement's distance from the float64 one; the reference's own output lies in
    the admissible set at every pixel; at most a tenth of the applied pixels have more than one admissible output."""
    g = golden()
    store, bar = golden_store(g), float(g[f'bar_pixels_{edge}'])
    imgs = R.pattern(R.N_IMAGES, edge)
    dist, total, multi = 0.0, 0, 0
    for name in R.CONFIGS:
        D, cfg = R.case_cfg(name, edge)
        for i, t in enumerate(g[f'table_{name}_{edge}']):
            out = g[f'out_{name}_{edge}'][i]
            if not t[R.APPLIED]:
                assert not out.any()
                continue
            im = store['imgs'][int(t[R.PARTNER])]
            b64, zero = R.partner_value(t, im, D, R.full(cfg)['pad_val'], np.float64)
            b32, zero32 = R.partner_value(t, im, D, R.full(cfg)['pad_val'], np.float32)
            assert np.array_equal(zero, zero32) and zero.any() == (t[R.J_] < edge) and not b64[zero].any()
            dist = max(dist, float(np.abs(b32.astype(np.float64) - b64).max()))
            a = imgs[i].transpose(1, 2, 0)
            lo, hi = R.admissible(a, b64, zero, bar)
            assert ((out >= lo) & (out <= hi)).all(), f'{name} image {i}: the reference is outside the admissible set'
            assert np.array_equal(out, R.blend(a, np.trunc(b32))), 'the fixture is the float32 evaluation, truncated twice'
            total += lo.size
            multi += int((lo != hi).sum())
    assert 0 < bar == 4 * dist
    share = multi / total
    print(f'edge {edge}: bar {bar:.3e}, {share:.2%} of {total} applied pixel values have more than one admissible output')
    assert share == float(g[f'ambiguous_{edge}']) and share <= R.AMBIGUOUS_CAP == 0.10


def test_sub_stream_is_keyed_apart():
    import affine_ref
    import pipeline_oracle as P
    keys = {R.mixup_key(3, 4, 5), affine_ref.affine_key(3, 4, 5), P.stream_key(3, 4, 5)}
    assert len(keys) == 3 and R.SALT not in (0x50484D44, 0x4D4F5341, 0x4355544F, 0x41464649)
    from yunet_amd.pipelines import mixup_partner
    counts = [3, 0, 0, 2, 0, 1]
    for it in range(6):
        for n in range(4):
            for iters in (1, 15):
                t = R.geometry(9, it, n, counts, [(32, 32)] * 6, 32, 32, dict(max_iters=iters))
                assert mixup_partner(9, it, n, counts, iters) == t[R.PARTNER]


# ------------------------------------------------------------------ constructor
def test_constructor_carries_the_reference_arguments_and_refuses():
    from yunet_amd.builder import PIPELINES
    from yunet_amd.pipelines import MixUp, _Carrier
    import yunet_amd._lib as L
    assert PIPELINES.get('MixUp') is MixUp and issubclass(MixUp, _Carrier)
    m = MixUp(img_scale=(64, 64), use_kps=True)
    assert m.cfg == dict(img_scale=(64, 64), ratio_range=(0.5, 1.5), flip_ratio=0.5, pad_val=114, max_iters=15,
                         min_bbox_size=5, min_area_ratio=0.2, max_aspect_ratio=20, bbox_clip_border=True, skip_filter=True,
                         use_kps=True)
    with pytest.raises(NotImplementedError, match=r'MixUp\(use_kps=False\).*write use_kps=True'):
        MixUp(img_scale=(64, 64))
    with pytest.raises(NotImplementedError, match='only the square canvas'):
        MixUp(img_scale=(64, 96), use_kps=True)
    for D in (0, -32, L.AUG_MAX_EDGE // 2 + 1):
        with pytest.raises(ValueError, match='D must lie in'):
            MixUp(img_scale=(D, D), use_kps=True)
    MixUp(img_scale=(L.AUG_MAX_EDGE // 2,) * 2, use_kps=True)
    nan, inf = float('nan'), float('inf')
    bad = [dict(ratio_range=(0.0, 1.0)), dict(ratio_range=(-1.0, 1.0)), dict(ratio_range=(1.5, 0.5)),
           dict(ratio_range=(0.5, inf)), dict(ratio_range=(nan, 1.0)), dict(ratio_range=(0.5,)), dict(flip_ratio=nan),
           dict(pad_val=inf), dict(pad_val=(114, 114, 114)), dict(pad_val=[114.0] * 3), dict(min_bbox_size=nan),
           dict(min_area_ratio=inf), dict(max_aspect_ratio=nan), dict(max_iters=0), dict(max_iters=-3),
           dict(max_iters=2.5), dict(ratio_range=(0.5, 1e9))]
    for kw in bad:
        with pytest.raises(ValueError, match='MixUp'):
            MixUp(img_scale=(64, 64), use_kps=True, **kw)
    with pytest.raises(NotImplementedError, match='executed inside DevicePipeline'):
        m(dict())


def test_c_cfg_carries_the_configuration():
    from yunet_amd.pipelines import MixUp
    c = MixUp(img_scale=(48, 48), ratio_range=(0.75, 1.25), flip_ratio=0.25, pad_val=7, max_iters=3, min_bbox_size=1.5,
              min_area_ratio=0.4, max_aspect_ratio=9, bbox_clip_border=False, skip_filter=False, use_kps=True
              ).c_cfg(0x1FFFFFFFF, 77)
    assert (c.ratio_lo, c.ratio_hi, c.flip_ratio, c.pad_val, c.img_scale, c.max_iters) == (0.75, 1.25, 0.25, 7.0, 48, 3)
    assert (c.min_bbox_size, c.min_area_ratio, c.max_aspect_ratio) == (1.5, np.float32(0.4), 9.0)
    assert (c.bbox_clip_border, c.skip_filter, c.gmax, c.seed) == (0, 0, 77, 0xFFFFFFFF)


def test_entry_points_refuse_on_the_host():
    """Every YUNET_EINVAL of the two entries is decided before any launch, so it shows without a GPU (the pointers are
    never dereferenced)."""
    from yunet_amd.pipelines import MixUp
    import yunet_amd._lib as L
    lib = L.load()
    a, b = C.c_void_p(4096), C.c_void_p(8192)

    def decide(c, n=4, edge=32, m=6, store=(a,) * 5, ins=(a, a, a), outs=(b, b, b), table=b):
        return lib.yunet_aug_mixup_decide(C.byref(c) if c is not None else None, 0, n, edge, None, m, *store, *ins, *outs,
                                          table, None)

    def cfg(**fields):
        c = MixUp(img_scale=(64, 64), use_kps=True).c_cfg(0, 8)
        for k, v in fields.items():
            setattr(c, k, v)
        return c
    nan, inf = float('nan'), float('inf')
    for what, c in {'ratio 0': cfg(ratio_lo=0.0), 'lo > hi': cfg(ratio_lo=2.0), 'hi inf': cfg(ratio_hi=inf),
                    'lo nan': cfg(ratio_lo=nan), 'hi huge': cfg(ratio_hi=1e9), 'flip nan': cfg(flip_ratio=nan),
                    'pad nan': cfg(pad_val=nan), 'size inf': cfg(min_bbox_size=inf), 'area nan': cfg(min_area_ratio=nan),
                    'aspect nan': cfg(max_aspect_ratio=nan), 'D 0': cfg(img_scale=0),
                    'D large': cfg(img_scale=L.AUG_MAX_EDGE // 2 + 1), 'iters 0': cfg(max_iters=0), 'gmax 0': cfg(gmax=0),
                    'gmax large': cfg(gmax=4097)}.items():
        assert decide(c) == L.EINVAL, what
    assert decide(None) == L.EINVAL and decide(cfg(), n=0) == L.EINVAL and decide(cfg(), n=-1) == L.EINVAL
    assert decide(cfg(), edge=0) == L.EINVAL and decide(cfg(), edge=L.AUG_MAX_EDGE + 1) == L.EINVAL
    assert decide(cfg(), m=0) == L.EINVAL and decide(cfg(), m=-4) == L.EINVAL
    for k in range(5):
        assert decide(cfg(), store=tuple(None if j == k else a for j in range(5))) == L.EINVAL
    for k in range(3):
        assert decide(cfg(), ins=tuple(None if j == k else a for j in range(3))) == L.EINVAL
        assert decide(cfg(), outs=tuple(None if j == k else b for j in range(3))) == L.EINVAL
        assert decide(cfg(), outs=tuple(a if j == k else b for j in range(3))) == L.EINVAL, 'an output that is its input'
    assert decide(cfg(), table=None) == L.EINVAL

    def pixels(table=a, D=64, pad=114.0, n=4, edge=32, m=6, store=(a, a, a), img=b):
        return lib.yunet_aug_mixup_pixels(table, D, pad, n, edge, None, m, *store, img, None)
    assert pixels(table=None) == L.EINVAL and pixels(img=None) == L.EINVAL
    for k in range(3):
        assert pixels(store=tuple(None if j == k else a for j in range(3))) == L.EINVAL
    assert pixels(n=0) == L.EINVAL and pixels(n=-2) == L.EINVAL and pixels(m=0) == L.EINVAL
    assert pixels(edge=0) == L.EINVAL and pixels(edge=L.AUG_MAX_EDGE + 1) == L.EINVAL
    assert pixels(D=0) == L.EINVAL and pixels(D=L.AUG_MAX_EDGE // 2 + 1) == L.EINVAL
    assert pixels(pad=nan) == L.EINVAL and pixels(pad=inf) == L.EINVAL
    assert pixels(n=1 << 20, edge=L.AUG_MAX_EDGE) == L.EINVAL, 'more workgroups than a launch takes'


# ------------------------------------------------------------------ DevicePipeline
def test_device_pipeline_accepts_mixup_at_its_place():
    from yunet_amd.pipelines import DevicePipeline, MixUp
    plain = DevicePipeline(BASE, seed=1)
    assert plain.mixup is None and plain.mixup_cfg is None and plain.mixup_table is None and plain.gmax == 64
    post = BASE[:5] + [PMD] + BASE[5:]
    lists = {'plain': with_mix(5),
             'post pmd': with_mix(6, base=post),
             'pre pmd': with_mix(6, base=BASE[:2] + [PMD] + BASE[2:]),
             'cutout': with_mix(5, base=BASE[:5] + [CUT] + BASE[5:]),
             'affine': with_mix(6, base=BASE[:5] + [AFF] + BASE[5:]),
             'post pmd, affine, cutout': with_mix(7, base=BASE[:5] + [PMD, AFF, CUT] + BASE[5:]),
             'mosaic': with_mix(6, base=BASE[:2] + [MOSAIC] + BASE[2:]),
             'mosaic, affine, cutout': with_mix(7, base=BASE[:2] + [MOSAIC] + BASE[2:5] + [AFF, CUT] + BASE[5:])}
    for what, cfg in lists.items():
        names = [c['type'] for c in cfg]
        assert names[names.index('MixUp') + 1] == ('CutOut' if 'cutout' in what else 'Normalize'), what
        pipe = DevicePipeline(cfg, seed=1)
        assert isinstance(pipe.mixup, MixUp) and pipe.mixup_cfg.seed == 1 and pipe.mixup_table is None, what
        rows = 5 * 64 if 'mosaic' in what else 2 * 64
        assert pipe.mixup_cfg.gmax == pipe.gmax == pipe.cfg.gmax == rows, what
        assert [type(s).__name__ for s in pipe.steps] == DevicePipeline.ORDER, what
        assert (pipe.mosaic is not None) == ('mosaic' in what) and (pipe.affine is not None) == ('affine' in what)
        if pipe.mosaic is not None:
            assert pipe.mosaic_cfg.gmax == rows
        if pipe.affine is not None:
            assert pipe.affine_cfg.gmax == rows
    assert DevicePipeline.ORDER == ['LoadImageFromFile', 'LoadAnnotations', 'RandomSquareCrop', 'Resize', 'RandomFlip',
                                    'Normalize', 'DefaultFormatBundle', 'Collect']


def test_device_pipeline_refuses_every_other_place():
    from yunet_amd.pipelines import DevicePipeline
    post = BASE[:5] + [PMD] + BASE[5:]
    cut = BASE[:5] + [CUT] + BASE[5:]
    aff = BASE[:5] + [AFF] + BASE[5:]
    wrong = {'before RandomFlip': with_mix(4),
             'before a POST PhotoMetricDistortion': with_mix(5, base=post),
             'after a PRE PhotoMetricDistortion': with_mix(3, base=BASE[:2] + [PMD] + BASE[2:]),
             'on the source image': with_mix(2),
             'before RandomAffine': with_mix(5, base=aff),
             'after CutOut': with_mix(6, base=cut),
             'after Normalize': with_mix(6),
             'first': with_mix(0),
             'last': with_mix(len(BASE)),
             'twice': with_mix(5, base=with_mix(5)),
             'twice, apart': with_mix(4, base=with_mix(5))}
    for what, cfg in wrong.items():
        with pytest.raises(NotImplementedError, match='MixUp once, after RandomFlip'):
            DevicePipeline(cfg, seed=1)
    # CutOut and RandomAffine keep their own rules on the list with MixUp taken out
    with pytest.raises(NotImplementedError, match='CutOut once, immediately in front of Normalize'):
        DevicePipeline(with_mix(5, base=BASE[:5] + [CUT, CUT] + BASE[5:]), seed=1)
    with pytest.raises(NotImplementedError, match='RandomAffine once, after RandomFlip'):
        DevicePipeline(with_mix(7, base=BASE[:5] + [AFF, AFF] + BASE[5:]), seed=1)
    with pytest.raises(NotImplementedError, match='use_kps=True'):
        DevicePipeline(BASE[:5] + [dict(type='MixUp', img_scale=(64, 64))] + BASE[5:], seed=1)
    # the lists without it keep their own messages
    with pytest.raises(NotImplementedError, match=r'DevicePipeline implements exactly'):
        DevicePipeline(BASE[:4] + BASE[5:], seed=1)
    with pytest.raises(NotImplementedError, match='RandomAffine once, after RandomFlip'):
        DevicePipeline(BASE[:4] + [AFF] + BASE[4:], seed=1)
    with pytest.raises(ValueError, match=r'gmax=300 gives 1200 GT rows'):
        DevicePipeline(BASE[:2] + [MOSAIC] + BASE[2:], seed=1, gmax=300)


def test_gt_capacity_counts_the_partner_rows():
    from yunet_amd.pipelines import MOSAIC_MAX_GT, DevicePipeline, gt_capacity_rows
    assert gt_capacity_rows(10) == 64 and gt_capacity_rows(300, mosaic=True) == 256         # as before
    assert gt_capacity_rows(10, mixup=True) == 64 and gt_capacity_rows(2000, mixup=True) == MOSAIC_MAX_GT // 2
    assert gt_capacity_rows(100, mosaic=True, mixup=True) == 128
    assert gt_capacity_rows(300, mosaic=True, mixup=True) == MOSAIC_MAX_GT // 5 == 204
    assert DevicePipeline(with_mix(5), seed=1, gmax=512).gmax == 1024
    with pytest.raises(ValueError, match='gives 1026 GT rows'):
        DevicePipeline(with_mix(5), seed=1, gmax=513)
    both = with_mix(6, base=BASE[:2] + [MOSAIC] + BASE[2:])
    assert DevicePipeline(both, seed=1, gmax=204).gmax == 1020
    with pytest.raises(ValueError, match='gives 1025 GT rows'):
        DevicePipeline(both, seed=1, gmax=205)


def test_mixup_needs_resident_sources():
    from yunet_amd.datasets import RetinaFaceSource
    from yunet_amd.pipelines import DevicePipeline
    from yunet_amd.runner import SyntheticSourceImages
    from yunet_amd.source_store import SourceStore, WindowFeed
    lst = with_mix(5)
    for host_fed in (True, 'window'):
        with pytest.raises(NotImplementedError, match="MixUp over host-fed sources.*not on the device"):
            SyntheticSourceImages(lst, host_fed=host_fed)
    for cache in (None, 'host'):
        with pytest.raises(NotImplementedError, match=r'MixUp over RetinaFaceSource\(cache=.*not on the device'):
            RetinaFaceSource(dataset=None, pipeline=lst, cache=cache)
    pipe = DevicePipeline(lst)
    with pytest.raises(NotImplementedError, match='MixUp over a window feed.*not on the device'):
        WindowFeed(pipe, SourceStore([(4, 4)], placement='host', device='cpu'), 64)
    with pytest.raises(NotImplementedError, match='not on the device'):
        pipe.window_plan(None, 0, 'cpu')
    with pytest.raises(NotImplementedError, match='not on the device'):
        pipe.windowed(None, 0, None, None, None)


# ------------------------------------------------------------------ skip_type_keys and the hook
def test_skip_type_keys_from_the_wrapper_to_the_pipeline():
    import yunet_amd
    from yunet_amd.datasets import MultiImageMixDataset, flatten_multi_image_mix
    from yunet_amd.pipelines import DevicePipeline

    class Inner:
        CLASSES = ('face',)

        def __len__(self):
            return 3
    w = MultiImageMixDataset(Inner(), [dict(MOSAIC)], skip_type_keys=['Mosaic'])
    assert w._skip_type_keys == ['Mosaic'] and len(w) == 3
    w.update_skip_type_keys(('Mosaic', 'MixUp'))
    assert w._skip_type_keys == ('Mosaic', 'MixUp')
    with pytest.raises(AssertionError):
        w.update_skip_type_keys([dict(type='Mosaic')])
    with pytest.raises(AssertionError):
        MultiImageMixDataset(Inner(), [dict(MOSAIC)], skip_type_keys=[1])
    load = [dict(p) for p in BASE[:2]]
    tail = with_mix(5, base=[dict(MOSAIC)] + BASE[2:5] + [AFF] + BASE[5:])
    wrapper = dict(type='MultiImageMixDataset', dataset=dict(type='SyntheticSourceImages', pipeline=load, pool=8),
                   pipeline=tail)
    from yunet_amd.datasets import split_skip_type_keys
    assert 'skip_type_keys' not in flatten_multi_image_mix(wrapper) and split_skip_type_keys(wrapper) == (wrapper, None)
    keyed = dict(wrapper, skip_type_keys=('Mosaic', 'MixUp'))
    rest, keys = split_skip_type_keys(keyed)
    assert keys == ['Mosaic', 'MixUp'] and rest == wrapper and 'skip_type_keys' in keyed
    assert flatten_multi_image_mix(rest)['pool'] == 8
    with pytest.raises(NotImplementedError, match='split_skip_type_keys'):     # the flat configuration has no place for them
        flatten_multi_image_mix(keyed)
    with pytest.raises(AssertionError):
        split_skip_type_keys(dict(wrapper, skip_type_keys=[3]))
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as T
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    cfg.merge_from_dict({'data.train': dict(wrapper, skip_type_keys=['Mosaic', 'MixUp'])})
    src = T.build_source(cfg, 0, 1, 0)
    assert src.dataset is src and src.pipe._skip == {'Mosaic', 'MixUp'} and src.pipe.gmax == 5 * 64
    assert src.pipe._on('RandomAffine') and not src.pipe._on('Mosaic') and not src.pipe._on('MixUp')
    src.update_skip_type_keys(())
    assert src.pipe._skip == frozenset() and src.pipe._on('Mosaic') and src.pipe._on('MixUp')
    pipe = DevicePipeline(BASE, seed=1)
    pipe.update_skip_type_keys(('Mosaic', 'RandomAffine', 'MixUp'))       # names the list does not hold are accepted
    assert not pipe._on('Mosaic')
    for bad in (['CutOut'], ('Mosaic', 'RandomFlip'), ['YOLOXHSVRandomAug']):
        with pytest.raises(NotImplementedError, match='skip_type_keys'):
            pipe.update_skip_type_keys(bad)
    with pytest.raises(AssertionError):
        pipe.update_skip_type_keys([0])


def test_mode_switch_hook_switches_at_the_references_epoch():
    from yunet_amd.hooks import YOLOXModeSwitchHook
    from yunet_amd.runner import HOOKS
    assert HOOKS['YOLOXModeSwitchHook'] is YOLOXModeSwitchHook
    h = YOLOXModeSwitchHook()
    assert h.num_last_epochs == 15 and h.skip_type_keys == ('Mosaic', 'RandomAffine', 'MixUp')

    class Obj:
        pass
    for max_epochs, last in ((300, 15), (3, 1), (5, 4), (4, 4)):
        calls, lines = [], []
        runner, runner.model, runner.data_loader = Obj(), Obj(), Obj()
        runner.model.bbox_head = Obj()
        runner.data_loader.dataset = Obj()
        runner.data_loader.dataset.update_skip_type_keys = calls.append
        runner.logger, runner.max_epochs = lines.append, max_epochs
        hook = YOLOXModeSwitchHook(num_last_epochs=last, skip_type_keys=('Mosaic', 'MixUp'))
        switched = []
        for epoch in range(max_epochs):
            runner.epoch = epoch
            hook.before_train_epoch(runner)
            if calls and not switched:
                switched.append(epoch)
        want = [e for e in range(max_epochs) if e + 1 == max_epochs - last]           # the reference's arithmetic
        assert switched == want, (max_epochs, last)
        if want:
            assert calls == [('Mosaic', 'MixUp')] and runner.model.bbox_head.use_l1 is True
            assert lines == ['No mosaic and mixup aug now!', 'Add additional L1 loss now!']
        else:
            assert not calls and not lines and not hasattr(runner.model.bbox_head, 'use_l1')


def test_runner_names_its_data_loader():
    import inspect
    from yunet_amd.runner import EpochBasedRunner
    src = inspect.getsource(EpochBasedRunner.train)
    assert src.index('self.data_loader = data_source') < src.index("call_hook('before_train_epoch')")


# ------------------------------------------------------------------ header / ctypes
def test_header_constants_and_struct_layout(tmp_path):
    import yunet_amd._lib as L
    txt = open(HEADER).read()
    defs = dict(re.findall(r'#define\s+(YUNET_MIXUP_\w+)\s+([\w.]+)', txt))
    assert int(defs['YUNET_MIXUP_SALT'].rstrip('u'), 16) == L.MIXUP_SALT == R.SALT
    assert bytes.fromhex('%08X' % L.MIXUP_SALT) == b'MIXU'
    assert int(defs['YUNET_MIXUP_WORDS']) == L.MIXUP_WORDS == R.WORDS == 18
    names = ('PARTNER', 'APPLIED', 'INDEX_DRAWS', 'JIT', 'FLIP', 'J', 'RW', 'RH', 'XOFF', 'YOFF', 'SX', 'SY', 'ROWS_IN',
             'ROWS_OUT', 'STATUS', 'EDGE', 'DRAWS', 'SR')
    for k, name in enumerate(names):
        assert int(defs[f'YUNET_MIXUP_{name}']) == getattr(L, f'MIXUP_{name}') == k, name
    assert (R.PARTNER, R.J_, R.SR) == (0, 5, 17)
    assert {'yunet_aug_mixup_decide', 'yunet_aug_mixup_pixels'} <= set(L.EXPORTED)
    assert L.load().yunet_abi_version() == 12                                               # additive: the number stays
    assert L._SIGNATURES['yunet_aug_mixup_decide'][1][0] is C.POINTER(L.YunetMixupCfg)
    assert len(L._SIGNATURES['yunet_aug_mixup_decide'][1]) == 19 and len(L._SIGNATURES['yunet_aug_mixup_pixels'][1]) == 12
    fields = [f for f, _ in L.YunetMixupCfg._fields_]
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yunet_hip.h"\n'
                   'int main(){printf("%zu", sizeof(YunetMixupCfg));'
                   + ''.join(f'printf(" %zu", offsetof(YunetMixupCfg, {f}));' for f in fields) + 'return 0;}')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = L.YunetMixupCfg
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
