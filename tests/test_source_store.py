"""CPU: the decoded-source store's bookkeeping, the numpy restatement of the window plan on hand-made params, and the
config plumbing of cache= / host_fed='window' (no GPU calls)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_store_capacity_and_offsets():
    from yunet_amd.source_store import SourceStore
    st = SourceStore([(10, 20), (3, 4), (7, 7)], placement='host', device='cpu')
    assert len(st) == 3 and st.nbytes == 3 * (200 + 12 + 49)
    assert st.offsets.tolist() == [0, 600, 636] and st.hw.tolist() == [[10, 20], [3, 4], [7, 7]]
    assert st.image_bytes.tolist() == [600, 36, 147]
    assert not any(st.has(i) for i in range(3)) and st.data is None        # nothing allocated before the first put
    with pytest.raises(ValueError, match='expected uint8'):
        st.put(1, np.zeros((4, 3, 3), np.uint8), np.zeros((1, 4)), np.zeros((1, 5, 3)))
    with pytest.raises(ValueError, match='keypoint rows'):
        st.put(1, np.zeros((3, 4, 3), np.uint8), np.zeros((2, 4)), np.zeros((1, 5, 3)))
    with pytest.raises(IndexError):
        st.put(3, np.zeros((3, 4, 3), np.uint8), np.zeros((1, 4)), np.zeros((1, 5, 3)))
    assert not st.has(1)


def test_store_rejects_bad_arguments():
    from yunet_amd.source_store import SourceStore
    with pytest.raises(ValueError, match='placement'):
        SourceStore([(4, 4)], placement='disk')
    with pytest.raises(ValueError):
        SourceStore([(0, 4)])
    with pytest.raises(ValueError):
        SourceStore([])


def test_window_plan_restatement_on_hand_made_params():
    from yunet_amd.source_store import window_plan_np
    hw = [[100, 80], [50, 60], [40, 40], [90, 70], [64, 64], [20, 30]]
    params = np.zeros((6, 8), np.int32)
    params[:, :4] = [[-10, 5, 50, 0],        # left < 0: cols [0, 40)
                     [10, -20, 45, 1],       # top < 0: rows [0, 25)
                     [-30, -25, 120, 0],     # a window larger than both sides: the whole image
                     [7, 9, 0, 0],           # cw == 0: nothing
                     [64, 0, 10, 0],         # window beside the image: nothing
                     [3, 4, 10, 1]]          # inside
    rect, off = window_plan_np(params, hw)
    assert rect.tolist() == [[5, 0, 50, 40], [0, 10, 25, 45], [0, 0, 40, 40], [0, 0, 0, 0], [0, 0, 0, 0],
                             [4, 3, 10, 10]]
    sizes = [50 * 40 * 3, 25 * 45 * 3, 40 * 40 * 3, 0, 0, 300]
    assert off.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert rect.dtype == np.int32 and off.dtype == np.int64


def test_window_plan_covers_every_tap():
    """The rectangle holds every in-image tap of the pixel pass (lin_coef restated in the oracle) over random windows."""
    import pipeline_oracle as P
    from yunet_amd.source_store import window_plan_np
    rng = np.random.default_rng(0)
    for _ in range(200):
        h, w, S = int(rng.integers(8, 90)), int(rng.integers(8, 90)), int(rng.choice([16, 32, 64]))
        cw = int(rng.integers(1, 2 * max(h, w)))
        left, top = int(rng.integers(-cw, w)), int(rng.integers(-cw, h))
        (y0, x0, rh, rw), = window_plan_np([[left, top, cw, 0, 0, 0, 0, 0]], [[h, w]])[0].tolist()
        s0, s1, _, _ = P.linear_coeffs(S, cw)
        xs = {left + int(s) for s in np.concatenate([s0, s1])}
        ys = {top + int(s) for s in np.concatenate([s0, s1])}
        xs_in = {x for x in xs if 0 <= x < w}
        ys_in = {y for y in ys if 0 <= y < h}
        if not (xs_in and ys_in):       # no tap inside the image: nothing is read
            continue
        for x in xs_in:
            assert x0 <= x < x0 + rw
        for y in ys_in:
            assert y0 <= y < y0 + rh


def _train_tool():
    spec = importlib.util.spec_from_file_location('yunet_train_tool_cache', os.path.join(ROOT, 'tools', 'train.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _labelv2(tmp_path):
    (tmp_path / 'a.jpg').write_bytes(b'')
    (tmp_path / 'labelv2.txt').write_text('# a.jpg 64 48\n1 2 30 40 ' + ' '.join(['5 6 0.0'] * 5) + ' 0.9\n')
    return str(tmp_path / 'labelv2.txt')


@pytest.mark.parametrize('cache', [None, 'device', 'host'])
def test_build_source_forwards_cache(tmp_path, cache):
    import yunet_amd
    T = _train_tool()
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    cfg.data.train.type = 'RetinaFaceDataset'
    cfg.data.train.ann_file = _labelv2(tmp_path)
    cfg.data.train.img_prefix = str(tmp_path)
    cfg.data.samples_per_gpu = 1
    if cache is not None:
        cfg.data.train.cache = cache
    src = T.build_source(cfg, 0, 1, 0)
    assert src.cache == cache and src.store is None          # nothing decoded before the first batch


def test_build_source_rejects_unknown_cache(tmp_path):
    import yunet_amd
    from yunet_amd.datasets import RetinaFaceDataset, RetinaFaceSource
    T = _train_tool()
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    cfg.data.train.type = 'RetinaFaceDataset'
    cfg.data.train.ann_file = _labelv2(tmp_path)
    cfg.data.train.img_prefix = str(tmp_path)
    cfg.data.train.cache = 'disk'
    with pytest.raises(ValueError, match='cache'):
        T.build_source(cfg, 0, 1, 0)
    ds = RetinaFaceDataset(cfg.data.train.ann_file, img_prefix=str(tmp_path), pipeline=cfg.train_pipeline)
    with pytest.raises(ValueError, match='cache'):
        RetinaFaceSource(ds, cfg.train_pipeline, samples_per_gpu=1, cache=True)


@pytest.mark.parametrize('bad', ['yes', 'windows', 2])
def test_synthetic_sources_reject_unknown_host_fed(bad):
    import yunet_amd
    import yunet_amd.runner as R
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    with pytest.raises(ValueError, match='host_fed'):
        R.SyntheticSourceImages(cfg.train_pipeline, host_fed=bad)
    for ok in (False, True, 'window'):
        assert R.SyntheticSourceImages(cfg.train_pipeline, host_fed=ok).host_fed == ok
