"""CPU: batches grouped by padded canvas (yunet_amd.grouped_eval.plan_batches(group_by='canvas')): the partition,
its order, the pixel cap, rank sharding, the numbers of WIDER-Face val at origin size (tests/golden/
wider_val_sizes.npy: the (h, w) of the 3226 images of labelv2/val/labelv2.txt, in list order) and the errors."""
import os
from collections import Counter, OrderedDict

import numpy as np
import pytest

from yunet_amd import grouped_eval as GE
from yunet_amd import test_pipeline as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = os.path.join(ROOT, 'tests', 'golden', 'wider_val_sizes.npy')


def origin_pipe():
    """Origin size as the reference's tool rewrites the list for it: scale_factor 1.0, Pad(size_divisor=32)."""
    return TP.DeviceTestPipeline([dict(type='LoadImageFromFile'), dict(
        type='MultiScaleFlipAug', scale_factor=1.0, flip=False,
        transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.0),
                    dict(type='Normalize', mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False),
                    dict(type='Pad', size_divisor=32, pad_val=0), dict(type='ImageToTensor', keys=['img']),
                    dict(type='Collect', keys=['img'])])])


def up32(v):
    return (int(v) + 31) // 32 * 32


def wider_hw():
    a = np.load(SIZES)
    assert a.dtype == np.int16 and a.shape == (3226, 2)
    return [(int(h), int(w)) for h, w in a]


def geoms(pipe, hw, batches):
    return {(len(b),) + pipe.canvas([hw[i] for i in b]) for b in batches}


def parent_plan_batches(pipe, hw, indices, samples_per_gpu, max_plans, log=None, resident=()):
    """plan_batches as it stood before group_by, restated: consecutive batches, or one image per batch when their
    geometries do not fit the plan cache."""
    indices = list(indices)
    batches = [indices[k:k + samples_per_gpu] for k in range(0, len(indices), samples_per_gpu)]
    if samples_per_gpu > 1:
        g = geoms(pipe, hw, batches)
        others = len({tuple(r) for r in resident} - g)
        if len(g) + others > max_plans:
            if log is not None:
                log(f'test pipeline: samples_per_gpu={samples_per_gpu} gives {len(g)} batch geometries but the engine '
                    f'keeps {max_plans} plans ({others} held by other shapes) -- running one image per batch (use a '
                    f'fixed-size mode, or set YUNET_MAX_PLANS)')
            batches = [[i] for i in indices]
    return batches


def test_default_is_the_consecutive_planner_with_its_fallback_and_log_line():
    rng = np.random.default_rng(0)
    hw = {i: (int(rng.integers(100, 1400)), int(rng.integers(100, 1400))) for i in range(200)}
    train = [(256, 320 + 32 * k, 320 + 32 * k) for k in range(15)]
    for pipe in (TP.DeviceTestPipeline(None, scale=None), TP.DeviceTestPipeline(None, scale=(640, 640))):
        for B in (1, 4):
            for resident in ((), train):
                for kw in ({}, dict(group_by=None), dict(group_by=None, max_batch_pixels=1)):
                    want_said, got_said = [], []
                    want = parent_plan_batches(pipe, hw, range(199), B, 16, want_said.append, resident)
                    got = GE.plan_batches(pipe, hw, list(range(199)), B, max_plans=16, log=got_said.append,
                                          resident=resident, **kw)
                    assert got == want and got_said == want_said
    # more geometries than max_plans: the fallback and its line are there
    said = []
    got = GE.plan_batches(TP.DeviceTestPipeline(None, scale=None), hw, list(range(200)), 4, max_plans=16, log=said.append)
    assert got == [[i] for i in range(200)] and len(said) == 1 and 'batch geometries' in said[0]


@pytest.mark.parametrize('B', [1, 2, 5, 16])
@pytest.mark.parametrize('cap', ['default', None, 64 * 96, 2 * 64 * 96, 3 * 96 * 128 + 7])
def test_grouped_batches_partition_the_indices(B, cap):
    rng = np.random.default_rng(3)
    pipe = origin_pipe()
    hs, ws = [33, 50, 64, 65, 90, 96, 128], [40, 50, 64, 90, 96, 100]
    hw = {i: (hs[int(rng.integers(len(hs)))], ws[int(rng.integers(len(ws)))]) for i in range(0, 140, 2)}
    indices = [int(i) for i in rng.permutation(list(hw))]
    said = []
    batches = GE.plan_batches(pipe, hw, indices, B, max_plans=2, log=said.append, group_by='canvas', max_batch_pixels=cap)
    assert not said, 'the grouped mode never falls back'
    assert sorted(i for b in batches for i in b) == sorted(indices)                      # every index exactly once
    key = lambda i: (up32(hw[i][0]), up32(hw[i][1]))                                     # noqa: E731
    assert all(key(i) == pipe.geometry(*hw[i])[2:] for i in indices)
    runs = OrderedDict()
    for b in batches:
        assert len({key(i) for i in b}) == 1                                             # one padded shape per batch
        c = key(b[0])
        assert pipe.canvas([hw[i] for i in b]) == c                                      # which is the batch canvas
        if c in runs:
            assert next(reversed(runs)) == c, 'a canvas occupies one consecutive run of batches'
        runs.setdefault(c, []).append(b)
    order = list(runs)
    assert order == sorted(order, key=lambda c: (-c[0] * c[1], c[0], c[1]))              # area down, ties by (ph, pw)
    assert any(a[0] * a[1] == b[0] * b[1] for a, b in zip(order, order[1:])), 'the set must have a tie in area'
    for c, bs in runs.items():
        assert [i for b in bs for i in b] == [i for i in indices if key(i) == c]         # the order of `indices`
        eff = B if cap is None else max(1, min(B, (B * 1024 * 1024 if cap == 'default' else cap) // (c[0] * c[1])))
        assert all(len(b) == eff for b in bs[:-1]) and 1 <= len(bs[-1]) <= eff


def test_wider_val_at_origin_size():
    hw, pipe = wider_hw(), origin_pipe()
    idx = list(range(len(hw)))
    assert all(w == 1024 for _, w in hw)
    per_canvas = Counter((up32(h), up32(w)) for h, w in hw)
    assert len(per_canvas) == 66 and per_canvas.most_common(2) == [((704, 1024), 768), ((768, 1024), 545)]
    assert sum(1 for v in per_canvas.values() if v == 1) == 13
    batches = GE.plan_batches(pipe, hw, idx, 16, group_by='canvas', max_batch_pixels=None)
    assert len(batches) == 238 == sum(-(-v // 16) for v in per_canvas.values())
    assert len({pipe.geometry(*hw[b[0]])[2:] for b in batches}) == 66
    assert len(geoms(pipe, hw, batches)) == 93
    assert sorted(i for b in batches for i in b) == idx
    said = []
    flat = GE.plan_batches(pipe, hw, idx, 16, max_plans=16, log=said.append)
    assert flat == [[i] for i in idx] and len(said) == 1 and '42 batch geometries' in said[0]


def test_default_pixel_cap_on_wider_val():
    hw, pipe = wider_hw(), origin_pipe()
    B, cap = 16, 16 * 1024 * 1024
    batches = GE.plan_batches(pipe, hw, list(range(len(hw))), B, group_by='canvas')
    assert batches == GE.plan_batches(pipe, hw, list(range(len(hw))), B, group_by='canvas', max_batch_pixels=cap)
    per_canvas = Counter((up32(h), up32(w)) for h, w in hw)
    want = 0
    for (ph, pw), n in per_canvas.items():
        eff = max(1, min(B, cap // (ph * pw)))
        want += (n + eff - 1) // eff
    assert len(batches) == want and want > 238
    for b in batches:
        ph, pw = up32(hw[b[0]][0]), up32(hw[b[0]][1])
        assert len(b) == 1 or len(b) * ph * pw <= cap
    tall = [i for i, (h, w) in enumerate(hw) if up32(h) == 5568]
    assert len(tall) == 1 and [tall[0]] in batches and batches[0] == [tall[0]]           # largest canvas first, alone
    assert sorted(i for b in batches for i in b) == list(range(len(hw)))


class FakeSet:
    """What run_test reads of a dataset, a source, a pipeline's output and a model, without a GPU: an "image" is its
    index, a batch's "tensor" the list of its indices, a result names its image, its batch and its canvas."""

    def __init__(self, hw):
        self.data_infos = [dict(filename=f'{i}.jpg', height=h, width=w) for i, (h, w) in enumerate(hw)]
        self.pipe = origin_pipe()
        self.views = self.pipe.views
        self.geometry = self.pipe.geometry
        self.fetched, self.ahead, self.batches, self.released = [], [], [], 0

    def reserve(self, indices):
        self.reserved = list(indices)

    def fetch(self, idx, ahead=()):
        self.fetched.append(list(idx))
        self.ahead.append(list(ahead))
        return list(idx)

    def release_workers(self):
        self.released += 1

    def pipe_call(self, fetched, view=0, filenames=None):
        assert view == 0 and filenames == [self.data_infos[i]['filename'] for i in fetched]
        metas = [self.pipe.meta(self.data_infos[i]['height'], self.data_infos[i]['width']) for i in fetched]
        return fetched, metas

    __call__ = pipe_call

    def model(self, return_loss=False, rescale=True, img=None, img_metas=None):
        assert not return_loss and rescale and len(img) == 1 and len(img_metas[0]) == len(img[0])
        shapes = {m['pad_shape'] for m in img_metas[0]}
        assert len(shapes) == 1, 'a grouped batch has one padded shape'
        self.batches.append(list(img[0]))
        return [('result', i, tuple(img[0]), m['pad_shape'][:2]) for i, m in zip(img[0], img_metas[0])]


@pytest.mark.parametrize('n', [1, 2, 11, 300])
@pytest.mark.parametrize('world', [1, 2])
def test_run_test_returns_the_order_of_indices_per_rank(n, world):
    """run_test itself, with a stand-in for the device side: the batches run in the planned order, decode-ahead names
    the next planned batch, every result returns to the position of its image in the rank's list, and reassemble of
    the per-rank lists gives dataset order."""
    hw = wider_hw()
    parts = []
    for r in range(world):
        fake = FakeSet(hw[:n])
        mine = TP.shard_indices(n, r, world)
        planned = GE.plan_batches(fake.pipe, hw, mine, 4, group_by='canvas')
        assert sorted(i for b in planned for i in b) == mine                             # only the rank's own images
        out = GE.run_test(fake.model, fake, 'cpu', mine, fake, fake, 4, group_by='canvas')
        assert fake.batches == planned == fake.fetched and fake.reserved == mine and fake.released == 1
        assert fake.ahead == (planned[1:] + [[]] if planned else [])
        assert [res[1] for res in out] == mine                                           # the order of `indices`
        for i, res in zip(mine, out):
            assert i in res[2] and res[3] == (up32(hw[i][0]), up32(hw[i][1]))
        parts.append(out)
    whole = TP.reassemble(parts, n, world)
    assert [res[1] for res in whole] == list(range(n))
    if n == 300:
        assert any(b != sorted(b) or b[0] > planned[k + 1][0] for k, b in enumerate(planned[:-1])), 'the plan must permute'


def test_run_test_with_a_repeated_and_shuffled_list():
    hw = wider_hw()[:40]
    fake = FakeSet(hw)
    order = [7, 2, 39, 2, 0, 15, 7, 31, 1]
    out = GE.run_test(fake.model, fake, 'cpu', order, fake, fake, 2, group_by='canvas', max_batch_pixels=None)
    assert [res[1] for res in out] == order and len(fake.batches) < len(order)


def test_bad_values_raise():
    hw, pipe = {0: (50, 90), 1: (64, 96)}, origin_pipe()
    for bad in ('shape', 'Canvas', True, 1):
        with pytest.raises(ValueError, match='group_by'):
            GE.plan_batches(pipe, hw, [0, 1], 2, group_by=bad)
        with pytest.raises(ValueError, match='group_by'):
            GE.run_test(None, None, 'cuda', [0, 1], pipe, None, 2, group_by=bad)
    with pytest.raises(ValueError, match='samples_per_gpu'):
        GE.plan_batches(pipe, hw, [0, 1], 0, group_by='canvas')
    with pytest.raises(ValueError, match='max_batch_pixels'):
        GE.plan_batches(pipe, hw, [0, 1], 2, group_by='canvas', max_batch_pixels=0)


def test_multi_view_with_group_by_raises():
    views = TP.DeviceTestPipeline([dict(type='MultiScaleFlipAug', img_scale=[(320, 320), (160, 160)], flip=True,
                                        transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                                                    dict(type='Pad', size_divisor=32)])])
    assert len(views.views) == 4
    with pytest.raises(NotImplementedError, match='one image per view'):
        GE.run_test(None, None, 'cuda', [0, 1], views, None, 2, group_by='canvas')


def test_eval_hook_reads_group_by_when_it_is_made():
    import yunet_amd.runner as R
    hook = R.EvalHook(None, samples_per_gpu=2, group_by='canvas')
    assert hook.group_by == 'canvas' and hook.max_batch_pixels == 'default'
    assert R.EvalHook(None).group_by is None
    with pytest.raises(ValueError, match='group_by'):
        R.EvalHook(None, samples_per_gpu=2, group_by='rows')
    with pytest.raises(ValueError, match='max_batch_pixels'):
        R.EvalHook(None, samples_per_gpu=2, group_by='canvas', max_batch_pixels=0)


def test_tool_takes_the_group_options():
    import importlib.util
    spec = importlib.util.spec_from_file_location('widerface_batched', os.path.join(ROOT, 'tools', 'widerface_batched.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    own, rest = mod.own_parser().parse_known_args(['cfg.py', 'ck.pth', '--group', 'canvas', '--max-batch-pixels', '4096'])
    assert own.group == 'canvas' and own.max_batch_pixels == 4096 and rest == ['cfg.py', 'ck.pth']
    own, _ = mod.own_parser().parse_known_args(['--max-batch-pixels', 'none'])
    assert own.max_batch_pixels == 'none'
    own, _ = mod.own_parser().parse_known_args(['cfg.py', 'ck.pth'])
    assert own.group is None and own.max_batch_pixels is None
    with pytest.raises(SystemExit):
        mod.own_parser().parse_known_args(['--group', 'rows'])


def test_dataset_says_when_group_by_reaches_it_unread(tmp_path):
    import warnings
    import yunet_amd
    (tmp_path / 'l.txt').write_text('# a.jpg 10 10\n')
    with pytest.warns(UserWarning, match='group_by=.canvas. reached the dataset unread'):
        yunet_amd.build_dataset(dict(type='RetinaFaceDataset', ann_file=str(tmp_path / 'l.txt'), test_mode=True,
                                     group_by='canvas'))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        yunet_amd.build_dataset(dict(type='RetinaFaceDataset', ann_file=str(tmp_path / 'l.txt'), test_mode=True))
