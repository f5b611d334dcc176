"""CPU: PhotoMetricDistortion in the device train pipeline -- the numpy restatement (tests/photometric_ref.py) against
the fixtures made by the unmodified reference class (tools/make_golden_photometric.py), against the live reference
where its tree is available, the config surface of DevicePipeline, and the C layout of YunetPhotoCfg."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import photometric_ref as R
import pipeline_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
BASE = [
    dict(type='LoadImageFromFile', to_float32=True),
    dict(type='LoadAnnotations', with_bbox=True, with_keypoints=True),
    dict(type='RandomSquareCrop', crop_choice=[0.5, 0.7, 0.9, 1.1, 1.3, 1.5]),
    dict(type='Resize', img_scale=(640, 640), keep_ratio=False),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_bboxes_ignore', 'gt_keypointss']),
]
PMD = dict(type='PhotoMetricDistortion')


def with_photo(at, **kw):
    cfg = [dict(p) for p in BASE]
    cfg.insert(at, dict(PMD, **kw))
    return cfg


def pipeline_case():
    g = np.load(os.path.join(GOLD, 'photometric_pipeline.npz'))
    seed, it, S, n = int(g['seed']), int(g['iteration']), int(g['S']), int(g['n'])
    rng = np.random.default_rng(seed)
    srcs = []
    for i in range(n):
        h, w, total = [int(v) for v in g[f'src_shape_{i}']]
        img, boxes, kps = P.synth_image(rng, h, w, int(g[f'src_g_{i}']))
        assert int(img.astype(np.int64).sum()) == total, 'synthetic source drifted from the fixture'
        srcs.append((img, boxes, kps))
    return g, seed, it, S, srcs


def pixels_case():
    g = np.load(os.path.join(GOLD, 'photometric_pixels.npz'))
    n, S = int(g['n']), int(g['S'])
    return g, int(g['seed']), int(g['iteration']), S, [R.hard_case(k, S) for k in range(n)]


def sha_hex(row):
    return bytes(row.tobytes()).hex()


# ------------------------------------------------------------------ restatement vs fixtures
def test_restated_draws_equal_the_reference_call_log():
    g, seed, it, _, srcs = pixels_case()
    log, off = g['log'], g['log_off']
    combos = set()
    for i in range(len(srcs)):
        t, st = R.draw_table(seed, it, i)
        assert np.array_equal(R.log_array(st.log), log[off[i]:off[i + 1]]), f'draws differ (image {i})'
        assert int(t[R.DRAWS]) == st.ctr
        perm = t[R.PERM:R.PERM + 3]
        assert sorted(perm.tolist()) == [0, 1, 2] and (t[R.SWAP] or perm.tolist() == [0, 1, 2])
        combos.add(R.combo(t))
    assert combos == set(range(64)), 'every (mode, flag) combination must occur in the fixture'


@pytest.mark.parametrize('p,position', [(0, 'pre'), (1, 'post')])
def test_restated_pixels_equal_the_reference_fixture(p, position):
    g, seed, it, S, srcs = pixels_case()
    bad = []
    for i, (img, b, k) in enumerate(srcs):
        r = R.augment_image(img, b, k, seed, it, i, S, [1.0], position)
        assert [int(r['params'][2]), int(r['params'][3])] == g['meta'][p, i, :2].tolist()
        if i < 4:
            assert np.array_equal(r['img'], g[f'{position}_img_{i}'])
        if R.digest(r['img']) != sha_hex(g['sha'][p, i]):
            bad.append(i)
    assert not bad, f'{position}: images differ from the reference {bad}'


def test_hard_cases_are_hit():
    """The fixture's sources contain what the issue lists: s = 0, ties of the max, both hue wraps, values pushed out
    of [0, 255], sector boundaries."""
    _, seed, it, S, srcs = pixels_case()
    hsv = R.bgr2hsv(srcs[0][0].astype(np.float32)).reshape(-1, 3)
    assert (hsv[:, 1] == 0).any()
    px = srcs[0][0].reshape(-1, 3).astype(np.int64)
    assert ((px[:, 2] == px[:, 1]) & (px[:, 1] > px[:, 0])).any()            # v == r == g
    assert ((hsv[:, 0] > 355) & (hsv[:, 1] > 0)).any() and ((hsv[:, 0] > 0) & (hsv[:, 0] < 5)).any()
    assert np.isin(hsv[:, 0], [0, 60, 120, 180, 240, 300]).sum() > 20
    lo = hi = wrap = 0
    for i, (img, _, _) in enumerate(srcs):
        t, _ = R.draw_table(seed, it, i)
        x = img.astype(np.float32)
        if t[R.BRIGHT]:
            x = x + t[R.DELTA]
        if t[R.MODE] == 1 and t[R.CONTRAST]:
            x = x * t[R.ALPHA]
        lo += int((x < 0).any())
        hi += int((x > 255).any())
        if t[R.HUE]:
            h = R.bgr2hsv(x)[..., 0] + t[R.HUE_D]
            wrap += int((h > 360).any()) + int((h < 0).any())
    assert lo and hi and wrap


@pytest.mark.parametrize('position', ['pre', 'post'])
def test_restated_pipeline_equals_the_reference_fixture(position):
    g, seed, it, S, srcs = pipeline_case()
    for i, (img, b, k) in enumerate(srcs):
        r = R.augment_image(img, b, k, seed, it, i, S, g['crop_choice'], position)
        cw, flip, draws, kept = [int(v) for v in g[f'{position}_meta_{i}']]
        assert (int(r['params'][2]), int(r['params'][3]), len(r['boxes'])) == (cw, flip, kept)
        assert np.array_equal(r['boxes'], g[f'{position}_boxes_{i}']) and np.array_equal(r['kps'], g[f'{position}_kps_{i}'])
        _, st = R.draw_table(seed, it, i)
        assert np.array_equal(R.log_array(st.log), g[f'{position}_log_{i}'])
        assert np.array_equal(r['img'][:, :8, :8], g[f'{position}_corner_{i}'])
        assert R.digest(r['img']) == str(g[f'{position}_sha_{i}']), f'{position}: image {i} differs'
        # the sub-stream: crop / flip / GT as without the transform
        r0 = P.augment_image(img, b, k, seed, it, i, S, g['crop_choice'])
        assert np.array_equal(r0['params'], r['params']) and np.array_equal(r0['boxes'], r['boxes'])
        assert np.array_equal(r0['kps'], r['kps'])


def test_hsv_round_trip_restatement_properties():
    """Grey pixels go through unchanged, a pure hue lands on its sector boundary, and the round trip changes low bits
    (the reason the device pass runs it unconditionally)."""
    grey = np.array([[0, 0, 0], [128, 128, 128], [-5.5, -5.5, -5.5], [300, 300, 300]], np.float32)
    hsv = R.bgr2hsv(grey)
    assert np.all(hsv[:, 1] == 0) and np.array_equal(R.hsv2bgr(hsv), grey)
    pure = np.array([[0, 0, 255], [0, 255, 255], [0, 255, 0], [255, 255, 0], [255, 0, 0], [255, 0, 255]], np.float32)
    assert np.allclose(R.bgr2hsv(pure)[:, 0], [0, 60, 120, 180, 240, 300], atol=1e-3)
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 300, (4096, 3)).astype(np.float32)
    y = R.hsv2bgr(R.bgr2hsv(x))
    assert np.allclose(x, y, rtol=1e-5, atol=1e-3) and not np.array_equal(x, y)


# ------------------------------------------------------------------ the live reference
def _tool():
    spec = importlib.util.spec_from_file_location('make_golden_photometric',
                                                  os.path.join(ROOT, 'tools', 'make_golden_photometric.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ref_available():
    import ref_stub
    return ref_stub.available()


@pytest.mark.skipif(not _ref_available(), reason='reference tree not available')
@pytest.mark.parametrize('position', ['pre', 'post'])
def test_restatement_equals_the_live_reference(position):
    """The unmodified reference class under the redirect, on fresh sources and non-default arguments: same draws,
    bit-identical pixels (numpy's weak-scalar fp32 arithmetic included)."""
    tool = _tool()
    T = tool.load_transforms()
    rng = np.random.default_rng(77)
    srcs = [P.synth_image(rng, int(rng.integers(60, 300)), int(rng.integers(60, 300)), int(rng.integers(1, 6)))
            for _ in range(12)] + [R.hard_case(k) for k in range(20)]
    photo = dict(brightness_delta=50, contrast_range=(0.3, 1.9), saturation_range=(0.1, 2.5), hue_delta=90)
    seed, it, S = 5, 31, 64
    ref = tool.run_reference(T, srcs, seed, it, S, tool.CROP_CHOICE, position, photo)
    for i, ((img, b, k), r) in enumerate(zip(srcs, ref)):
        mine = R.augment_image(img, b, k, seed, it, i, S, tool.CROP_CHOICE, position, photo)
        _, st = R.draw_table(seed, it, i, **photo)
        assert np.array_equal(R.log_array(st.log), r['log'])
        assert np.array_equal(mine['boxes'], r['boxes']) and np.array_equal(mine['kps'], r['kps'])
        assert np.array_equal(mine['img'], r['img']), f'{position}: image {i} differs from the live reference'


@pytest.mark.skipif(not _ref_available(), reason='reference tree not available')
def test_carrier_defaults_equal_the_reference_constructor():
    tool = _tool()
    T = tool.load_transforms()
    from yunet_amd.pipelines import PhotoMetricDistortion
    ref = {k: v.default for k, v in inspect.signature(T.PhotoMetricDistortion.__init__).parameters.items()
           if k != 'self'}
    ours = {k: v.default for k, v in inspect.signature(PhotoMetricDistortion.__init__).parameters.items()
            if k != 'self'}
    assert ours == ref == R.DEFAULTS


def test_carrier_defaults_and_attributes():
    from yunet_amd.builder import PIPELINES
    from yunet_amd.registry import build_from_cfg
    t = build_from_cfg(dict(PMD), PIPELINES)
    assert (t.brightness_delta, t.contrast_range, t.saturation_range, t.hue_delta) == (32, (0.5, 1.5), (0.5, 1.5), 18)
    assert (t.contrast_lower, t.contrast_upper, t.saturation_lower, t.saturation_upper) == (0.5, 1.5, 0.5, 1.5)
    with pytest.raises(NotImplementedError, match='inside DevicePipeline'):
        t({})


# ------------------------------------------------------------------ config surface
def test_device_pipeline_accepts_the_two_positions():
    import yunet_amd._lib as L
    from yunet_amd.pipelines import DevicePipeline
    pre = DevicePipeline(with_photo(2, hue_delta=10))
    post = DevicePipeline(with_photo(5, contrast_range=(0.8, 1.2)))
    assert pre.photo_position == L.PHOTO_PRE and post.photo_position == L.PHOTO_POST
    assert pre.photo_cfg.hue_delta == 10.0 and pre.photo_cfg.position == L.PHOTO_PRE
    assert (post.photo_cfg.contrast_lower, post.photo_cfg.contrast_upper) == (0.8, 1.2)
    assert [type(s).__name__ for s in pre.steps] == DevicePipeline.ORDER == [type(s).__name__ for s in post.steps]
    plain = DevicePipeline([dict(p) for p in BASE])
    assert plain.photo is None and plain.photo_cfg is None and plain.photo_position == L.PHOTO_NONE
    for a, b in ((pre, plain), (post, plain)):
        assert bytes(a.cfg) == bytes(b.cfg)           # crop / resize / flip configuration unchanged


@pytest.mark.parametrize('at', [0, 1, 3, 4, 6, 7, 8])
def test_device_pipeline_rejects_other_positions(at):
    from yunet_amd.pipelines import DevicePipeline
    with pytest.raises(NotImplementedError, match='between LoadAnnotations and RandomSquareCrop.*between RandomFlip '
                                                  'and Normalize'):
        DevicePipeline(with_photo(at))


def test_device_pipeline_rejects_a_second_instance():
    from yunet_amd.pipelines import DevicePipeline
    cfg = with_photo(5)
    cfg.insert(2, dict(PMD))
    with pytest.raises(NotImplementedError, match='once'):
        DevicePipeline(cfg)
    cfg = with_photo(5)
    cfg.insert(5, dict(PMD))
    with pytest.raises(NotImplementedError, match='once'):
        DevicePipeline(cfg)


@pytest.mark.parametrize('kw', [dict(brightness_delta=-1), dict(hue_delta=-0.5), dict(contrast_range=(1.5, 0.5)),
                                dict(saturation_range=(2.0, 1.0)), dict(hue_delta=400),
                                dict(brightness_delta=float('nan')), dict(contrast_range=(0.5, float('inf')))])
def test_device_pipeline_rejects_nonsensical_arguments(kw):
    from yunet_amd.pipelines import DevicePipeline
    with pytest.raises(ValueError):
        DevicePipeline(with_photo(5, **kw))


# ------------------------------------------------------------------ C ABI
def test_photo_cfg_matches_c_layout(tmp_path):
    import yunet_amd._lib as L
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yunet_hip.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",sizeof(YunetPhotoCfg),'
                   'offsetof(YunetPhotoCfg,brightness_delta),offsetof(YunetPhotoCfg,contrast_upper),'
                   'offsetof(YunetPhotoCfg,saturation_lower),offsetof(YunetPhotoCfg,saturation_upper),'
                   'offsetof(YunetPhotoCfg,hue_delta),offsetof(YunetPhotoCfg,position),'
                   'offsetof(YunetPhotoCfg,reserved_));return 0;}')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = L.YunetPhotoCfg
    assert got == [C.sizeof(S), S.brightness_delta.offset, S.contrast_upper.offset, S.saturation_lower.offset,
                   S.saturation_upper.offset, S.hue_delta.offset, S.position.offset, S.reserved_.offset]


def test_photo_constants_match_the_header():
    import yunet_amd._lib as L
    txt = open(os.path.join(ROOT, 'include', 'yunet_hip.h')).read()
    d = {k: int(v, 0) for k, v in re.findall(r'#define\s+YUNET_PHOTO_(\w+)\s+(0x[0-9A-Fa-f]+|\d+)u?\s', txt)}
    assert (d['NONE'], d['PRE'], d['POST']) == (L.PHOTO_NONE, L.PHOTO_PRE, L.PHOTO_POST)
    assert d['SALT'] == L.PHOTO_SALT == R.SALT and d['WORDS'] == L.PHOTO_WORDS == R.WORDS
    for name in ('BRIGHT', 'DELTA', 'MODE', 'CONTRAST', 'ALPHA', 'SAT', 'SAT_F', 'HUE', 'HUE_D', 'SWAP', 'PERM',
                 'DRAWS'):
        assert d[name] == getattr(L, 'PHOTO_' + name) == getattr(R, name), name
