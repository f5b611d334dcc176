"""CPU: the host side of the batched device test pipeline (yunet_amd.test_pipeline): parsing of the reference's
test pipeline list, the geometry against evaluation.prepare_test_image (the per-image path, the yardstick), batch
order / rank sharding, and the C ABI additions."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import yunet_amd
from yunet_amd import evaluation as E
from yunet_amd import test_pipeline as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inner(**over):
    """The transforms of the reference's MultiScaleFlipAug (its configs/yunet_n.py, data.val / data.test)."""
    t = dict(Resize=dict(type='Resize', keep_ratio=True), RandomFlip=dict(type='RandomFlip', flip_ratio=0.0),
             Normalize=dict(type='Normalize', mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False),
             Pad=dict(type='Pad', size=(640, 640), pad_val=0), ImageToTensor=dict(type='ImageToTensor', keys=['img']),
             Collect=dict(type='Collect', keys=['img']))
    for k, v in over.items():
        if v is None:
            del t[k]
        else:
            t[k] = v
    return list(t.values())


def full(transforms=None, **msfa):
    m = dict(type='MultiScaleFlipAug', img_scale=(640, 640), flip=False,
             transforms=inner() if transforms is None else transforms)
    m.update(msfa)
    if m.get('scale_factor') is not None:
        m.pop('img_scale')
    return [dict(type='LoadImageFromFile'), m]


# ----------------------------------------------------------------------------------------------- 1. parsing
@pytest.mark.parametrize('kind', ['n', 's'])
def test_shipped_and_reference_lists_build(kind):
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    data = cfg.get('data') or {}
    for split in ('val', 'test'):          # whatever test-side list a shipped config carries must build
        if data.get(split) is not None and data[split].get('pipeline') is not None:
            TP.DeviceTestPipeline(list(data[split]['pipeline']))
    p = TP.DeviceTestPipeline(full())      # the list of the reference's data.val / data.test
    assert p.views == [((640, 640), False)] and p.pad == ('size', (640, 640))
    assert p.pad_fixed_size == (640, 640) and p.pad_size_divisor is None
    q = TP.DeviceTestPipeline(full(inner(Pad=dict(type='Pad', size_divisor=32), ImageToTensor=dict(type='DefaultFormatBundle')),
                                   scale_factor=1.0))
    assert q.views == [(1.0, False)] and q.pad == ('divisor', 32) and q.batched_bundle and q.pad_size_divisor == 32
    # today's configs: no list, or a MultiScaleFlipAug with no transforms -> prepare_test_image's own rule
    for lst in (None, [], [dict(type='MultiScaleFlipAug', img_scale=(320, 320), flip=False, transforms=[])]):
        e = TP.DeviceTestPipeline(lst, scale=(320, 320))
        assert e.views == [((320, 320), False)] and e.pad == ('scale',)


def test_view_order_is_the_reference_loop():
    p = TP.DeviceTestPipeline(full(img_scale=[(640, 640), (320, 320)], flip=True))
    assert p.views == [((640, 640), False), ((640, 640), True), ((320, 320), False), ((320, 320), True)]
    assert [p.meta(300, 400, v)['flip'] for v in range(4)] == [False, True, False, True]


@pytest.mark.parametrize('lst,exc,match', [
    (full(inner(Normalize=dict(type='Normalize', mean=[104., 117., 123.], std=[1., 1., 1.], to_rgb=False))),
     NotImplementedError, 'raw 0-255 BGR'),
    (full(inner(Normalize=dict(type='Normalize', mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=True))),
     NotImplementedError, 'raw 0-255 BGR'),
    (full(inner(Resize=dict(type='Resize', keep_ratio=False))), NotImplementedError, 'keep_ratio'),
    (full(flip=True, flip_direction='vertical'), NotImplementedError, 'horizontal'),
    (full(flip=True, flip_direction=['horizontal', 'vertical']), NotImplementedError, 'horizontal'),
    (full(inner(Pad=dict(type='Pad', size=(640, 640), pad_val=114))), NotImplementedError, 'pad_val'),
    (full(inner(Pad=dict(type='Pad', pad_to_square=True))), NotImplementedError, 'pad_to_square'),
    (full(inner(Pad=dict(type='Pad', pad_val=0))), ValueError, 'size and size_divisor'),
    (full(inner() + [dict(type='Albu')]), NotImplementedError, 'Albu'),
    (full(inner() + [dict(type='Pad', size=(640, 640))]), NotImplementedError, 'Pad appears 2 times'),
    (full() + [dict(type='MultiScaleFlipAug', img_scale=(640, 640))], NotImplementedError, 'appears 2 times'),
    (full()[:1] + [dict(type='Resize', keep_ratio=True)], NotImplementedError, 'Resize'),
    (full(inner(Resize=None)), NotImplementedError, 'needs Resize'),
    (full(list(reversed(inner()))), NotImplementedError, 'order'),
    (full(inner(RandomFlip=None), flip=True), ValueError, 'flips nothing'),
    ([dict(type='LoadImageFromFile'), dict(type='MultiScaleFlipAug', transforms=inner())], ValueError, 'exactly one'),
    ([dict(type='MultiScaleFlipAug', img_scale=(640, 640), scale_factor=0.5, transforms=inner())], ValueError, 'exactly one'),
])
def test_rejected_forms_raise_with_the_reason(lst, exc, match):
    with pytest.raises(exc, match=match):
        TP.DeviceTestPipeline(lst)


def test_sources_other_than_device_or_none_raise():
    with pytest.raises(ValueError, match='host-placement'):
        TP.TestSource(None, cache='host', device='cuda')
    with pytest.raises(ValueError, match='samples_per_gpu'):
        TP.batches_of(range(4), 0)


# ---------------------------------------------------------------------------------------------- 2. geometry
SIZES = [(480, 640), (640, 480), (500, 500), (641, 333), (333, 641), (1, 1000), (1000, 1), (31, 33), (33, 31), (100, 150),
         (700, 700), (1385, 1024), (768, 1024), (1024, 768), (2000, 3001), (3001, 2000), (640, 640), (1280, 1280),
         (320, 320), (1100, 1650), (1650, 1100), (1101, 1651), (639, 641), (17, 4000)]
MODES = [(640, 640), (1100, 1650), None, (320, 320)]


@pytest.mark.parametrize('mode', MODES)
def test_geometry_equals_prepare_test_image(mode):
    """nh, nw, pad_shape, scale_factor of every form of the list that stands for the mode -- the empty list (today's
    configs), the reference's list as its tool rewrites it for the mode -- equal the per-image path's metas."""
    if mode is None:
        spelled = full(inner(Pad=dict(type='Pad', size=None, size_divisor=32)), scale_factor=1.0)
    else:
        spelled = full(inner(Pad=dict(type='Pad', size=mode, pad_val=0)), img_scale=mode)
    pipes = [TP.DeviceTestPipeline(None, scale=mode), TP.DeviceTestPipeline(spelled)]
    for h, w in SIZES:
        if mode is not None and min(int(h * min(max(mode) / max(h, w), min(mode) / min(h, w)) + 0.5),
                                    int(w * min(max(mode) / max(h, w), min(mode) / min(h, w)) + 0.5)) < 1:
            for p in pipes:
                with pytest.raises(ValueError, match='empty size'):
                    p.geometry(h, w)
            continue
        x, want = E.prepare_test_image(np.zeros((h, w, 3), np.uint8), mode, 'cpu')
        for p in pipes:
            got = p.meta(h, w)
            nh, nw, ph, pw = p.geometry(h, w)
            assert (nh, nw, 3) == want['img_shape'] and (ph, pw, 3) == want['pad_shape'], (h, w, mode, got, want)
            assert tuple(x.shape) == (1, 3, ph, pw)
            for k, v in want.items():
                assert k in got, k
                if isinstance(v, np.ndarray):
                    assert got[k].dtype == v.dtype and np.array_equal(got[k], v), (k, h, w, mode)
                else:
                    assert got[k] == v, (k, h, w, mode)
            assert p.canvas([(h, w)]) == (ph, pw)


def test_geometry_of_a_float_scale_factor():
    """mmcv.imrescale with a float: each side int(side * f + 0.5); Pad(size_divisor=32)."""
    p = TP.DeviceTestPipeline(full(inner(Pad=dict(type='Pad', size_divisor=32)), scale_factor=0.5))
    for h, w in SIZES:
        nh, nw = int(h * 0.5 + 0.5), int(w * 0.5 + 0.5)
        if min(nh, nw) < 1:
            with pytest.raises(ValueError, match='empty size'):
                p.geometry(h, w)
            continue
        m = p.meta(h, w)
        assert m['img_shape'] == (nh, nw, 3) and m['pad_shape'] == ((nh + 31) // 32 * 32, (nw + 31) // 32 * 32, 3)
        assert np.array_equal(m['scale_factor'], np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32))
        assert m['pad_fixed_size'] is None and m['pad_size_divisor'] == 32


def test_batch_canvas_is_the_largest_padded_shape():
    p = TP.DeviceTestPipeline(None, scale=None)
    assert p.canvas([(100, 150), (333, 64), (32, 500)]) == (352, 512)
    q = TP.DeviceTestPipeline(full())
    assert q.canvas([(100, 150), (333, 64), (32, 500)]) == (640, 640)


# ------------------------------------------------------------------------------------- 3. batches and shards
@pytest.mark.parametrize('B', [1, 3, 8])
@pytest.mark.parametrize('world', [1, 2, 4])
@pytest.mark.parametrize('n', [1, 7, 23, 50])
def test_batches_cover_every_image_once_in_dataset_order(B, world, n):
    parts = []
    for r in range(world):
        mine = TP.shard_indices(n, r, world)
        assert mine == list(range(r, n, world))
        batches = TP.batches_of(mine, B)
        assert all(1 <= len(b) <= B for b in batches) and all(len(b) == B for b in batches[:-1])
        assert [i for b in batches for i in b] == mine           # consecutive images of the rank's list
        parts.append([('result', i) for b in batches for i in b])
    assert sorted(i for p in parts for _, i in p) == list(range(n))
    assert TP.reassemble(parts, n, world) == [('result', i) for i in range(n)]


def test_plan_batches_falls_back_to_one_image_per_batch():
    """Origin-size evaluation: more batch geometries than the engine keeps plans -> B = 1, with the reason logged;
    a fixed-size mode keeps its batches."""
    rng = np.random.default_rng(0)
    hw = {i: (int(rng.integers(100, 1400)), int(rng.integers(100, 1400))) for i in range(200)}
    said = []
    origin = TP.DeviceTestPipeline(None, scale=None)
    got = TP.plan_batches(origin, hw, list(range(200)), 4, max_plans=16, log=said.append)
    assert got == [[i] for i in range(200)] and len(said) == 1 and 'batch geometries' in said[0]
    fixed = TP.DeviceTestPipeline(None, scale=(640, 640))
    got = TP.plan_batches(fixed, hw, list(range(199)), 4, max_plans=16, log=said.append)
    assert len(got) == 50 and len(got[-1]) == 3 and len(said) == 1
    # plans the engine holds for other shapes (training) share the cache: two eval geometries + 15 others > 16
    train = [(256, 320 + 32 * k, 320 + 32 * k) for k in range(15)]
    got = TP.plan_batches(fixed, hw, list(range(199)), 4, max_plans=16, log=said.append, resident=train)
    assert got == [[i] for i in range(199)] and len(said) == 2 and '15 held by other shapes' in said[1]
    # the run's own geometries, resident from an earlier firing, do not count twice
    own = [(4, 640, 640), (3, 640, 640)] + train[:14]
    got = TP.plan_batches(fixed, hw, list(range(199)), 4, max_plans=16, log=said.append, resident=own)
    assert len(got) == 50 and len(said) == 2


def test_dataset_says_when_samples_per_gpu_reaches_it_unread(tmp_path):
    (tmp_path / 'l.txt').write_text('# a.jpg 10 10\n')
    with pytest.warns(UserWarning, match='reached the dataset unread'):
        yunet_amd.build_dataset(dict(type='RetinaFaceDataset', ann_file=str(tmp_path / 'l.txt'), test_mode=True,
                                     samples_per_gpu=4))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        yunet_amd.build_dataset(dict(type='RetinaFaceDataset', ann_file=str(tmp_path / 'l.txt'), test_mode=True,
                                     samples_per_gpu=1))


def test_wider_result_helpers(tmp_path):
    class DS:
        data_infos = [dict(filename='0--Parade/a.jpg'), dict(filename='1--X/b.png')]
    dets = [[np.array([[1., 2., 4., 6., 0.9]], np.float32)], [np.zeros((0, 5), np.float32)]]
    pred = E.collect_wider_results(dets, DS, str(tmp_path / 'p'))
    assert np.array_equal(pred['0--Parade']['a'], [[1., 2., 3., 4., np.float32(0.9)]]) and pred['1--X']['b'].shape == (0, 5)
    assert dets[0][0][0, 2] == 4.0          # the caller's arrays are not changed
    back = E.read_predictions(str(tmp_path / 'p'))
    assert np.allclose(back['0--Parade']['a'], pred['0--Parade']['a']) and back['1--X']['b'].shape == (0, 5)
    E.write_aps(str(tmp_path / 'o'), [0.5, 0.25, 0.125])
    assert open(tmp_path / 'o' / 'aps').read() == '0.500000,0.250000,0.125000\n'


# ------------------------------------------------------------------------------------------------ 4. C ABI
def test_abi_carries_the_new_entries():
    import yunet_amd._lib as L
    lib = L.load()
    assert lib.yunet_abi_version() == 12
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'yunet_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(?:int|size_t)\s+(yunet_\w+)\s*\(', txt))
    for name in ('yunet_test_pixels', 'yunet_rescale_dets'):
        assert name in declared and name in L.EXPORTED and hasattr(lib, name)
    # entry-point checks: bad sizes are refused before anything is launched (no GPU is touched)
    assert lib.yunet_test_pixels(None, None, None, None, 1, 32, 32, None, None) == L.EINVAL
    one = (8 * 1024)
    buf = (np.zeros(one, np.uint8)).ctypes.data
    for n, hc, wc in ((0, 32, 32), (1, 0, 32), (1, 32, 30), (1, 32, 0), (1, 32, L.AUG_MAX_EDGE + 4), (70000, 32, 32)):
        assert lib.yunet_test_pixels(buf, buf, buf, buf, n, hc, wc, buf, None) == L.EINVAL, (n, hc, wc)
    assert lib.yunet_rescale_dets(None, None, None, None, 1, 8, None) == L.EINVAL
    assert lib.yunet_rescale_dets(buf, None, buf, buf, 0, 8, None) == L.EINVAL
    assert lib.yunet_rescale_dets(buf, None, buf, buf, 1, -1, None) == L.EINVAL


HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
def test_pixel_kernel_has_no_scratch_and_no_serialised_load_loop(tmp_path):
    """The unit as the Makefile builds it: 0 scratch in both kernels, and the static scan of tools/dbg/serial_loads.py
    (the one tests/test_isa_guard.py runs over the older units) finds no loop that waits out each load on its own."""
    src = os.path.join(ROOT, 'libfacedetection.train_amd', 'csrc', 'test_pipeline.hip')
    out = str(tmp_path / 'tp.s')
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-w', '-S',
                        '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-o', out, src],
                       check=True, capture_output=True, text=True, timeout=600)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    assert len(scratch) == 2 and scratch == [0, 0], r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location('serial_loads', os.path.join(ROOT, 'tools', 'dbg', 'serial_loads.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bad = [f for f in mod.scan(out) if f[1] >= 10]
    assert not bad, bad
