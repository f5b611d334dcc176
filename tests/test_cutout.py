"""CPU: CutOut in the device train pipeline -- the pure-Python restatement (tests/cutout_ref.py) against the fixture made
by the unmodified reference class (tools/make_golden_cutout.py), against the live reference where its tree is
available, the constructor's refusals, the place DevicePipeline accepts, and the C layout of YunetCutoutCfg."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cutout_ref as R
from test_photometric import BASE, PMD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'cutout.npz')
HEADER = os.path.join(ROOT, 'include', 'yunet_hip.h')
MOSAIC = dict(type='Mosaic', img_scale=(640, 640), use_kps=True)
CUT = dict(type='CutOut', n_holes=(0, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.2)])


def golden():
    g = np.load(GOLD)
    assert str(g['configs']) == repr(R.CONFIGS) and int(g['seed']) == R.SEED and int(g['iteration']) == R.ITERATION, \
        'tests/golden/cutout.npz was made from other cases than cutout_ref.CONFIGS'
    return g


def cases():
    """(configuration name, edge, iteration) of every table of the fixture."""
    return [(name, e, R.ITERATION + k) for name in R.CONFIGS for k, e in enumerate(R.EDGES)]


def with_cutout(at, base=BASE, **kw):
    cfg = [dict(p) for p in base]
    cfg.insert(at, dict(CUT, **kw))
    return cfg


# ------------------------------------------------------------------ restatement vs fixture
@pytest.mark.parametrize('name', list(R.CONFIGS))
def test_restated_tables_and_pixels_equal_the_reference_fixture(name):
    g = golden()
    cfg = R.CONFIGS[name]
    fill = R.normalise(cfg)[4]
    for k, e in enumerate(R.EDGES):
        imgs = g[f'in_{e}']
        assert np.array_equal(imgs, R.pattern(R.N_IMAGES, e)) and imgs.dtype == np.float32
        want_t, want_o = g[f'holes_{name}_{e}'], g[f'out_{name}_{e}']
        for i in range(R.N_IMAGES):
            row = R.holes(R.SEED, R.ITERATION + k, i, e, e, cfg)
            assert row.dtype == np.int32 and np.array_equal(row, want_t[i]), f'{name} edge {e} image {i}: table'
            assert R.fill(imgs[i], row, fill).tobytes() == want_o[i].tobytes(), f'{name} edge {e} image {i}: pixels'


def test_fixture_contains_the_hard_cases():
    g = golden()
    zero = empty = False
    right, bottom, sizes = set(), set(), set()
    for name, e, _ in cases():
        n_lo, n_hi = R.normalise(R.CONFIGS[name])[:2]
        for row in g[f'holes_{name}_{e}']:
            n = int(row[0])
            assert n_lo <= n <= n_hi and row[1] == 1 + 3 * n and not row[2 + 4 * n:].any()
            zero |= n == 0
            sizes.add((name, n))
            for j in range(n):
                x1, y1, x2, y2 = (int(v) for v in row[2 + 4 * j:6 + 4 * j])
                assert 0 <= x1 <= x2 <= e and 0 <= y1 <= y2 <= e and x1 < e and y1 < e
                empty |= x2 == x1 or y2 == y1
                if x2 == e and x1 < x2:
                    right.add(e)
                if y2 == e and y1 < y2:
                    bottom.add(e)
    assert zero, 'no image of the fixture draws 0 holes'
    assert empty, 'no empty hole in the fixture'
    assert right == set(R.EDGES) and bottom == set(R.EDGES), 'a clipped hole per edge and image size'
    for name in ('range_shapes', 'range_ratios'):       # a range really draws different counts
        assert len({n for c, n in sizes if c == name}) >= 3
    assert int(0.01 * 96) == 0 and (0.01, 0.5) in R.CONFIGS['range_ratios']['cutout_ratio']    # a ratio that truncates to 0
    assert R.MAX_HOLES in {n for _, n in sizes}


def test_sub_stream_is_keyed_apart_from_the_other_streams():
    import photometric_ref
    import pipeline_oracle as P
    st = R.CutoutStream(9, 4, 2)
    assert st.key == P.mix32(P.stream_key(9, 4, 2) ^ R.SALT)
    assert len({st.key, P.Stream(9, 4, 2).key, photometric_ref.photo_key(9, 4, 2)}) == 3
    # the index and count draws are made with one candidate / a fixed count too: 1 + 3 * n_holes draws
    assert R.holes(1, 2, 3, 64, 64, dict(n_holes=5, cutout_shape=(3, 3)))[1] == 16


def test_restatement_equals_the_live_reference():
    """Where the reference tree is available: the unmodified class, fed from the sub-stream, on cases beyond the fixture."""
    import ref_stub
    if not ref_stub.available():
        pytest.skip('reference tree not available')
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_cutout', os.path.join(ROOT, 'tools', 'make_golden_cutout.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    T = ref_stub.load_pipeline_transforms()
    ours = inspect.signature(__import__('yunet_amd.pipelines', fromlist=['CutOut']).CutOut.__init__).parameters
    theirs = inspect.signature(T.CutOut.__init__).parameters
    assert [(k, v.default) for k, v in ours.items()] == [(k, v.default) for k, v in theirs.items()]
    cfg = dict(n_holes=(1, 6), cutout_ratio=[(0.3, 0.3), (0.55, 0.1)], fill_in=(3, 2, 1))
    imgs = R.pattern(6, 48)
    tables, outs = tool.run_reference(T, cfg, imgs, 77, 12)
    for i in range(6):
        row = R.holes(77, 12, i, 48, 48, cfg)
        assert np.array_equal(row, tables[i]) and np.array_equal(R.fill(imgs[i], row, (3, 2, 1)), outs[i])


# ------------------------------------------------------------------ constructor
def test_constructor_refusals_name_the_argument():
    from yunet_amd.pipelines import CutOut
    import yunet_amd._lib as L
    ok = CutOut(3, cutout_shape=(10, 7))
    assert ok.n_holes == (3, 3) and ok.candidates == [(10, 7)] and not ok.with_ratio and ok.fill == (0.0, 0.0, 0.0)
    ok = CutOut((0, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.2)], fill_in=114)
    assert ok.n_holes == (0, 4) and ok.with_ratio and len(ok.candidates) == 2 and ok.fill == (114.0, 114.0, 114.0)
    assert CutOut(L.CUTOUT_MAX_HOLES, cutout_shape=[(1, 1)] * L.CUTOUT_MAX_CANDIDATES).n_holes[1] == L.CUTOUT_MAX_HOLES
    bad = [
        (dict(n_holes=1), 'cutout_shape or cutout_ratio'),
        (dict(n_holes=1, cutout_shape=(2, 2), cutout_ratio=(0.1, 0.1)), 'cutout_shape or cutout_ratio'),
        (dict(n_holes=(2, 2), cutout_shape=(2, 2)), 'n_holes'),
        (dict(n_holes=(3, 1), cutout_shape=(2, 2)), 'n_holes'),
        (dict(n_holes=(-1, 2), cutout_shape=(2, 2)), 'n_holes'),
        (dict(n_holes=(1, 2, 3), cutout_shape=(2, 2)), 'n_holes'),
        (dict(n_holes=1.5, cutout_shape=(2, 2)), 'n_holes'),
        (dict(n_holes=-1, cutout_shape=(2, 2)), 'n_holes'),
        (dict(n_holes=1, cutout_shape=5), 'cutout_shape'),
        (dict(n_holes=1, cutout_shape=(2, 2, 2)), 'cutout_shape'),
        (dict(n_holes=1, cutout_shape=[(2, 2), (3,)]), 'cutout_shape'),
        (dict(n_holes=1, cutout_shape=(-2, 2)), 'cutout_shape'),
        (dict(n_holes=1, cutout_shape=(2.5, 2)), 'cutout_shape'),
        (dict(n_holes=1, cutout_ratio=0.5), 'cutout_ratio'),
        (dict(n_holes=1, cutout_ratio=(0.1, float('nan'))), 'cutout_ratio'),
        (dict(n_holes=1, cutout_ratio=[(0.1, 0.1), (float('inf'), 0.1)]), 'cutout_ratio'),
        (dict(n_holes=1, cutout_ratio=(-0.1, 0.1)), 'cutout_ratio'),
        (dict(n_holes=1, cutout_shape=(2, 2), fill_in=(1, 2)), 'fill_in'),
        (dict(n_holes=1, cutout_shape=(2, 2), fill_in=(1, 2, float('nan'))), 'fill_in'),
        (dict(n_holes=1, cutout_shape=(2, 2), fill_in='black'), 'fill_in'),
        # the two limits of this build
        (dict(n_holes=L.CUTOUT_MAX_HOLES + 1, cutout_shape=(2, 2)), 'YUNET_CUTOUT_MAX_HOLES'),
        (dict(n_holes=(0, L.CUTOUT_MAX_HOLES + 1), cutout_shape=(2, 2)), 'YUNET_CUTOUT_MAX_HOLES'),
        (dict(n_holes=1, cutout_shape=[(1, 1)] * (L.CUTOUT_MAX_CANDIDATES + 1)), 'YUNET_CUTOUT_MAX_CANDIDATES'),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            CutOut(**kw)
    with pytest.raises(NotImplementedError, match='DevicePipeline'):
        CutOut(1, cutout_shape=(2, 2))({})


def test_c_cfg_carries_the_configuration():
    from yunet_amd.pipelines import CutOut
    c = CutOut((1, 3), cutout_ratio=[(0.1, 0.25), (0.5, 1 / 3)], fill_in=(1.5, 2, 3)).c_cfg(0x1FFFFFFFF)
    assert (c.n_lo, c.n_hi, c.n_cand, c.with_ratio, c.seed) == (1, 3, 2, 1, 0xFFFFFFFF)
    assert [tuple(c.cand[i]) for i in range(2)] == [(0.1, 0.25), (0.5, 1 / 3)] and list(c.fill) == [1.5, 2.0, 3.0]
    c = CutOut(2, cutout_shape=(10, 7)).c_cfg(3)
    assert (c.n_lo, c.n_hi, c.n_cand, c.with_ratio) == (2, 2, 1, 0) and tuple(c.cand[0]) == (10.0, 7.0)


def test_entry_point_refuses_on_the_host():
    """Every YUNET_EINVAL of yunet_aug_cutout is decided before any launch, so it shows without a GPU (the pointers are
    never dereferenced)."""
    from yunet_amd.pipelines import CutOut
    import yunet_amd._lib as L
    lib = L.load()
    ptr = C.c_void_p(4096)

    def call(c, n=4, edge=32, img=ptr, holes=ptr):
        return lib.yunet_aug_cutout(C.byref(c) if c is not None else None, 0, n, edge, None, img, holes, None)

    def cfg(**fields):
        c = CutOut((1, 3), cutout_ratio=[(0.5, 0.5), (0.25, 0.25)]).c_cfg(0)
        for k, v in fields.items():
            if k == 'cand':
                c.cand[1][1] = v
            else:
                setattr(c, k, v)
        return c
    for what, c in {'n0 > n1': cfg(n_lo=4), 'n0 < 0': cfg(n_lo=-1), 'holes': cfg(n_hi=L.CUTOUT_MAX_HOLES + 1),
                    'no candidate': cfg(n_cand=0), 'candidates': cfg(n_cand=L.CUTOUT_MAX_CANDIDATES + 1),
                    'negative': cfg(cand=-1.0), 'nan': cfg(cand=float('nan')), 'inf': cfg(cand=float('inf'))}.items():
        assert call(c) == L.EINVAL, what
    assert call(None) == L.EINVAL and call(cfg(), n=0) == L.EINVAL and call(cfg(), n=-1) == L.EINVAL
    assert call(cfg(), edge=0) == L.EINVAL and call(cfg(), edge=L.AUG_MAX_EDGE + 1) == L.EINVAL
    assert call(cfg(), img=None) == L.EINVAL and call(cfg(), holes=None) == L.EINVAL


# ------------------------------------------------------------------ DevicePipeline
def test_device_pipeline_accepts_cutout_in_front_of_normalize():
    from yunet_amd.pipelines import CutOut, DevicePipeline
    plain = DevicePipeline(BASE, seed=1)
    assert plain.cutout is None and plain.cutout_cfg is None and plain.cutout_holes is None
    lists = {'plain': with_cutout(5),
             'post pmd': with_cutout(6, base=BASE[:5] + [PMD] + BASE[5:]),
             'pre pmd': with_cutout(6, base=BASE[:2] + [PMD] + BASE[2:]),
             'mosaic': with_cutout(6, base=BASE[:2] + [MOSAIC] + BASE[2:]),
             'mosaic, post pmd': with_cutout(7, base=BASE[:2] + [MOSAIC] + BASE[2:5] + [PMD] + BASE[5:])}
    for what, cfg in lists.items():
        assert cfg[[c['type'] for c in cfg].index('CutOut') + 1]['type'] == 'Normalize', what
        pipe = DevicePipeline(cfg, seed=1)
        assert isinstance(pipe.cutout, CutOut) and pipe.cutout_cfg.n_hi == 4 and pipe.cutout_cfg.seed == 1, what
        assert [type(s).__name__ for s in pipe.steps] == DevicePipeline.ORDER, what
        assert (pipe.photo is not None) == ('pmd' in what) and (pipe.mosaic is not None) == ('mosaic' in what)
    assert DevicePipeline.ORDER == [c['type'] for c in BASE]
    ms = [dict(p) for p in with_cutout(5)]
    ms[3] = dict(type='Resize', img_scale=(320, 640), multiscale_mode='square_range', keep_ratio=False)
    assert DevicePipeline(ms, seed=1).cutout is not None


def test_device_pipeline_refuses_every_other_place():
    from yunet_amd.pipelines import DevicePipeline
    post = BASE[:5] + [PMD] + BASE[5:]
    wrong = {'before RandomFlip': with_cutout(4),
             'before a POST PhotoMetricDistortion': with_cutout(5, base=post),
             'on the source image': with_cutout(2),
             'after Normalize': with_cutout(6),
             'first': with_cutout(0),
             'last': with_cutout(len(BASE)),
             'twice': with_cutout(5, base=with_cutout(5)),
             'twice, apart': with_cutout(4, base=with_cutout(5))}
    for what, cfg in wrong.items():
        with pytest.raises(NotImplementedError, match='CutOut once, immediately in front of Normalize'):
            DevicePipeline(cfg, seed=1)
    # a list without CutOut keeps its own messages
    with pytest.raises(NotImplementedError, match=r'DevicePipeline implements exactly'):
        DevicePipeline(BASE[:4] + BASE[5:], seed=1)
    with pytest.raises(KeyError):
        DevicePipeline(BASE[:5] + [dict(type='CutOutt', n_holes=1, cutout_shape=(2, 2))] + BASE[5:], seed=1)


# ------------------------------------------------------------------ header / ctypes
def test_header_constants_and_struct_layout(tmp_path):
    import yunet_amd._lib as L
    txt = open(HEADER).read()
    defs = dict(re.findall(r'#define\s+(YUNET_CUTOUT_\w+)\s+(\w+)', txt))
    assert int(defs['YUNET_CUTOUT_SALT'].rstrip('u'), 16) == L.CUTOUT_SALT == R.SALT
    assert int(defs['YUNET_CUTOUT_WORDS']) == L.CUTOUT_WORDS == R.WORDS == 2 + 4 * L.CUTOUT_MAX_HOLES
    assert int(defs['YUNET_CUTOUT_MAX_HOLES']) == L.CUTOUT_MAX_HOLES == R.MAX_HOLES and L.CUTOUT_MAX_HOLES in (16, 32)
    assert int(defs['YUNET_CUTOUT_MAX_CANDIDATES']) == L.CUTOUT_MAX_CANDIDATES == 8
    assert bytes.fromhex('%08X' % L.CUTOUT_SALT) == b'CUTO'
    assert 'yunet_aug_cutout' in L.EXPORTED and L.load().yunet_abi_version() == 12       # additive: the number stays
    assert L._SIGNATURES['yunet_aug_cutout'][1][0] is C.POINTER(L.YunetCutoutCfg)
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yunet_hip.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu\\n",sizeof(YunetCutoutCfg),offsetof(YunetCutoutCfg,n_cand),'
                   'offsetof(YunetCutoutCfg,with_ratio),offsetof(YunetCutoutCfg,cand),offsetof(YunetCutoutCfg,fill),'
                   'offsetof(YunetCutoutCfg,seed));return 0;}')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = L.YunetCutoutCfg
    assert got == [C.sizeof(T), T.n_cand.offset, T.with_ratio.offset, T.cand.offset, T.fill.offset, T.seed.offset]
