"""CPU: the Soft-NMS restatement (tests/soft_nms_ref.py) is consistent with itself, test_cfg.nms = dict(type='soft_nms')
is parsed with mmcv's keys and defaults, and the library exports the two entry points.  No kernel runs here."""
import numpy as np
import pytest

import soft_nms_ref as S

SEEDS = range(6)
METHODS = ('naive', 'linear', 'gaussian')
MIN_SCORES = (1e-3, 0.05)


@pytest.mark.parametrize('seed', SEEDS)
def test_restatement_forms_agree_bit_for_bit(seed):
    """The sequential swap form of softnms_cpu and the live-set form the kernel implements select the same candidates
    with the same fp32 score bits; emitted scores never increase; the fixture keeps every decision >= 1e-4 from its
    boundary (so float32 and float64 runs select in the same order)."""
    boxes, scores = S.cluster_fixture(seed)
    for method in METHODS:
        for min_score in MIN_SCORES:
            g = S.Guard()
            k64, s64 = S.soft_nms_live(boxes, scores, min_score=min_score, method=method, dtype=np.float64, guard=g)
            assert g.ok(1e-4), (seed, method, min_score, g)
            k_live, s_live = S.soft_nms_live(boxes, scores, min_score=min_score, method=method)
            k_swap, s_swap = S.soft_nms_swap(boxes, scores, min_score=min_score, method=method)
            assert np.array_equal(k_live, k_swap), (seed, method, min_score)
            assert s_live.dtype == np.float32 and np.array_equal(s_live.view(np.uint32), s_swap.view(np.uint32))
            assert np.all(np.diff(s_live) <= 0), 'emitted scores are non-increasing'
            assert np.array_equal(k_live, k64) and np.allclose(s_live, s64, rtol=1e-6, atol=0)
            assert 5 <= len(k_live) < len(scores)                    # something is suppressed, something survives


def test_score_thr_below_min_score_semantics():
    """A candidate that starts below min_score survives only as the first selection (the min_score test runs for every
    live candidate after every round, also where the weight was 1)."""
    boxes = np.array([[0, 0, 10, 10], [100, 0, 110, 10], [200, 0, 210, 10]], np.float32)      # disjoint
    for form in (S.soft_nms_live, S.soft_nms_swap):
        keep, sc = form(boxes, np.array([0.5, 0.01, 0.2], np.float32), min_score=0.05)
        assert keep.tolist() == [0, 2] and sc.tolist() == [np.float32(0.5), np.float32(0.2)]
        keep, sc = form(boxes, np.array([0.03, 0.01, 0.02], np.float32), min_score=0.05)
        assert keep.tolist() == [0] and sc.tolist() == [np.float32(0.03)]      # the first selection is never filtered


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return 'dets', 'kps', 'count'


@pytest.fixture
def head(monkeypatch):
    import yunet_amd
    import yunet_amd.kernels as K
    cfg = yunet_amd.Config.fromfile('configs/yunet_n.py')
    rec = _Recorder()
    monkeypatch.setattr(K, 'detect', rec)
    return yunet_amd.build_detector(cfg.model).bbox_head, rec


SIZES = [(8, 12), (4, 6), (2, 3)]


def test_config_soft_nms_defaults_and_keys(head):
    h, rec = head
    out = h._detect_flat('flat', SIZES, dict(score_thr=0.05, nms=dict(type='soft_nms'), max_per_img=7))
    assert out == ('dets', 'kps', 'count')
    (args, kw), = rec.calls
    assert args == ('flat', SIZES, h.strides, 0.05) and kw['max_out'] == 7
    assert kw['soft'] == dict(iou_thr=0.3, sigma=0.5, min_score=1e-3, method='linear')          # mmcv.ops.soft_nms defaults
    rec.calls.clear()
    h._detect_flat('flat', SIZES, dict(nms=dict(type='soft_nms', iou_threshold=0.4, sigma=0.25, min_score=0.01, method='gaussian',
                                                offset=0, class_agnostic=True, split_thr=10000)))
    (args, kw), = rec.calls
    assert args[3] == 0.02 and kw['max_out'] == -1
    assert kw['soft'] == dict(iou_thr=0.4, sigma=0.25, min_score=0.01, method='gaussian')


def test_config_soft_nms_rejections(head):
    h, rec = head
    with pytest.raises(ValueError, match='cubic'):
        h._detect_flat('flat', SIZES, dict(nms=dict(type='soft_nms', method='cubic')))
    with pytest.raises(ValueError, match='max_num'):
        h._detect_flat('flat', SIZES, dict(nms=dict(type='soft_nms', max_num=100)))
    with pytest.raises(NotImplementedError, match='offset'):
        h._detect_flat('flat', SIZES, dict(nms=dict(type='soft_nms', offset=1)))
    with pytest.raises(NotImplementedError, match='nms_match'):
        h._detect_flat('flat', SIZES, dict(nms=dict(type='nms_match')))
    assert rec.calls == []


def test_config_greedy_nms_call_is_unchanged(head):
    h, rec = head
    h._detect_flat('flat', SIZES, dict(score_thr=0.1, nms=dict(type='nms', iou_threshold=0.6), max_per_img=5))
    h._detect_flat('flat', SIZES, dict(nms=dict(iou_threshold=0.5)))
    h._detect_flat('flat', SIZES, dict())
    assert rec.calls == [(('flat', SIZES, h.strides, 0.1, 0.6, 5), {}),
                         (('flat', SIZES, h.strides, 0.02, 0.5, -1), {}),
                         (('flat', SIZES, h.strides, 0.02, 0.45, -1), {})]


def test_cfg_options_reach_the_head_through_the_batched_tool():
    """tools/widerface_batched.py takes --cfg-options as tools/train.py does (its own parser strips them before the
    per-image tool's parser sees the rest), and the merged test_cfg reaches the head untouched."""
    import importlib.util
    import os
    import yunet_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('widerface_batched', os.path.join(root, 'tools', 'widerface_batched.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    own, rest = tool.own_parser().parse_known_args(['configs/yunet_n.py', 'x.pth', '--mode', '0', '--cfg-options',
                                                    'model.test_cfg.nms.type=soft_nms', 'model.test_cfg.nms.iou_threshold=0.3'])
    assert rest == ['configs/yunet_n.py', 'x.pth', '--mode', '0']
    assert tool.own_parser().parse_known_args(['configs/yunet_n.py', 'x.pth'])[0].cfg_options is None
    cfg = yunet_amd.Config.fromfile(rest[0])
    cfg.merge_from_dict(own.cfg_options)
    model = yunet_amd.build_detector(cfg.model)
    assert dict(model.test_cfg['nms']) == dict(type='soft_nms', iou_threshold=0.3)
    assert dict(model.bbox_head.test_cfg['nms']) == dict(type='soft_nms', iou_threshold=0.3)
    assert 'cfg.merge_from_dict(b.cfg_options)' in open(os.path.join(root, 'tools', 'widerface_batched.py')).read()


def test_make_soft_nms_struct():
    import yunet_amd._lib as L
    import yunet_amd.kernels as K
    c = K.make_soft_nms()
    assert (c.method, c.iou_thr, c.sigma, c.min_score) == (L.SOFTNMS_LINEAR, np.float32(0.3), 0.5, np.float32(1e-3))
    assert [K.make_soft_nms(method=m).method for m in ('naive', 'linear', 'gaussian')] == [0, 1, 2]
    with pytest.raises(ValueError, match='cubic'):
        K.make_soft_nms(method='cubic')


def test_library_exports_soft_nms_entry_points():
    import ctypes as C
    import yunet_amd._lib as L
    lib = L.load()
    assert hasattr(lib, 'yunet_detect_soft') and hasattr(lib, 'yunet_soft_nms')
    assert 'yunet_detect_soft' in L.EXPORTED and 'yunet_soft_nms' in L.EXPORTED
    assert lib.yunet_abi_version() == 12                       # additions only: the ABI number stays
    assert C.sizeof(L.YunetSoftNms) == 16
    # argument validation happens before anything touches a device
    ok = L.YunetSoftNms(L.SOFTNMS_LINEAR, 0.3, 0.5, 1e-3)
    one = C.c_void_p(16)                                        # non-null placeholders; never dereferenced on these paths

    def nms(cfg):
        return lib.yunet_soft_nms(one, one, None, 1, 4, -1e30, cfg, 4, one, None, one, one, None)
    assert nms(None) == L.EINVAL
    for bad in (L.YunetSoftNms(3, 0.3, 0.5, 1e-3), L.YunetSoftNms(-1, 0.3, 0.5, 1e-3),
                L.YunetSoftNms(L.SOFTNMS_GAUSSIAN, 0.3, 0.0, 1e-3), L.YunetSoftNms(L.SOFTNMS_GAUSSIAN, 0.3, float('nan'), 1e-3),
                L.YunetSoftNms(L.SOFTNMS_LINEAR, float('inf'), 0.5, 1e-3), L.YunetSoftNms(L.SOFTNMS_NAIVE, 0.3, 0.5, float('nan'))):
        assert nms(C.byref(bad)) == L.EINVAL
    assert lib.yunet_soft_nms(one, one, None, 1, 4, -1e30, C.byref(ok), 0, one, None, one, one, None) == L.EINVAL   # max_out < 1
    lv = L.YunetLevels()
    assert lib.yunet_detect_soft(one, C.byref(lv), 1, 4, 0.02, None, 4, one, None, one, one, None) == L.EINVAL
