"""CPU: the integer stage of the WIDER protocol as a function of its own (evaluation.wider_pr_counts +
wider_aps_from_counts == wider_evaluation, pinned to the reference's APs) and the plumbing of the device scorer's
options (EvalHook(score=...), tools/widerface_batched.py --score, device=... without a GPU)."""
import copy
import importlib.util
import os
import re
import warnings

import numpy as np
import pytest

import helpers as Hh
import wider_fixture as WF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_counts_then_aps_equal_wider_evaluation(seed):
    import yunet_amd.evaluation as E
    g = Hh.load_golden('wider_eval.npz')
    ne, ni = [int(v) for v in g[f'cfg_{seed}']]
    events, pred = WF.synth_events(seed, n_events=ne, imgs_per_event=ni)
    mine = copy.deepcopy(pred)
    counts, count_face = E.wider_pr_counts(mine, events, 0.5)
    assert counts.dtype == np.int64 and counts.shape == (3, 1000, 2)
    assert count_face.dtype == np.int64 and count_face.shape == (3,)
    assert [int(v) for v in count_face] == [sum(len(im['keep'][k]) for ev in events for im in ev['images'])
                                            for k in ('easy', 'medium', 'hard')]
    aps = E.wider_aps_from_counts(counts, count_face)
    whole = copy.deepcopy(pred)
    want = E.wider_evaluation(whole, events, 0.5)
    assert np.allclose(aps, want, rtol=0, atol=0), (aps, want)
    assert np.allclose(aps, g[f'aps_{seed}'], rtol=0, atol=1e-12), (aps, g[f'aps_{seed}'])
    # both leave the scores normalised in place, to the same values
    for ev in pred:
        for name in pred[ev]:
            assert np.array_equal(mine[ev][name], whole[ev][name])
    # the counters are what the curves are made of
    _, curves = E.wider_evaluation(copy.deepcopy(pred), events, 0.5, return_curves=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        for s in range(3):
            assert np.array_equal(curves[s][:, 1], counts[s, :, 1] / int(count_face[s]), equal_nan=True)
            assert np.array_equal(curves[s][:, 0], counts[s, :, 1] / counts[s, :, 0], equal_nan=True)


def test_pack_wider_layout():
    """The packed set the device scorer takes: protocol order, subset bits, predictions no event lists at the end."""
    import yunet_amd.evaluation as E
    events, pred = WF.synth_events(1, n_events=2, imgs_per_event=4)
    pred['stray'] = {'x': np.array([[1., 2., 3., 4., 7.5]])}
    rows, poff, boxes, goff, bits, count_face = E.pack_wider(pred, events)
    ims = [(ev, im) for ev in events for im in ev['images']]
    assert poff.dtype == goff.dtype == np.int64 and len(poff) == len(goff) == len(ims) + 2
    for i, (ev, im) in enumerate(ims):
        assert np.array_equal(rows[poff[i]:poff[i + 1]], pred[ev['name']][im['name']])
        assert np.array_equal(boxes[goff[i]:goff[i + 1]], im['boxes'])
        for s, k in enumerate(('easy', 'medium', 'hard')):
            flag = np.zeros(len(im['boxes']), dtype=bool)
            flag[im['keep'][k] - 1] = True
            assert np.array_equal((bits[goff[i]:goff[i + 1]] >> s) & 1, flag)
    assert np.array_equal(rows[poff[-2]:], pred['stray']['x']) and goff[-1] == goff[-2]
    assert rows.dtype == boxes.dtype == np.float64 and bits.dtype == np.uint8
    with pytest.raises(TypeError, match='float64'):
        E.pack_wider({ev['name']: {im['name']: np.ones((2, 5), np.float32) for im in ev['images']} for ev in events},
                     events)


def test_eval_hook_score_option():
    import yunet_amd.runner as R
    with pytest.raises(ValueError, match='bogus'):
        R.EvalHook(None, score='bogus')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert R.EvalHook(None).score is None
        assert R.EvalHook(None, score=None, iou_thr=0.5).score is None
        assert R.EvalHook(None, score='host').score == 'host'
        assert R.EvalHook(None, score='device').score == 'device'
    with pytest.warns(UserWarning, match='rule'):          # every other unknown key: warned about and dropped, as before
        R.EvalHook(None, score='device', rule='greater')


def test_tool_parses_score():
    spec = importlib.util.spec_from_file_location('widerface_batched', os.path.join(ROOT, 'tools', 'widerface_batched.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    p = tool.own_parser()
    a, rest = p.parse_known_args(['cfg.py', 'ck.pth', '--score', 'device', '--mode', '320'])
    assert a.score == 'device' and a.cache is None and rest == ['cfg.py', 'ck.pth', '--mode', '320']
    assert p.parse_known_args(['cfg.py'])[0].score == 'host'
    with pytest.raises(SystemExit):
        p.parse_known_args(['--score', 'numpy'])


def test_device_scorer_without_a_gpu_raises():
    """device=... never falls back to the host path: a CPU device, or a CUDA device on a machine without one, raises."""
    import torch
    import yunet_amd
    import yunet_amd.evaluation as E
    events, pred = WF.synth_events(0)
    bad = ['cpu'] + ([] if torch.cuda.is_available() else ['cuda'])
    dets = [np.array([[0., 0., 10., 10., 0.9]], np.float32)]
    anns = [dict(bboxes=np.array([[0., 0., 10., 10.]], np.float32), bboxes_ignore=np.zeros((0, 4), np.float32))]
    for dev in bad:
        before = copy.deepcopy(pred)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            E.wider_evaluation(pred, events, 0.5, device=dev)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            E.wider_pr_counts(pred, events, device=dev)
        assert all(np.array_equal(pred[e][k], before[e][k]) for e in pred for k in pred[e]), 'nothing was scored'
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            E.eval_map_single_class(dets, anns, 0.5, device=dev)
        ds = yunet_amd.datasets.RetinaFaceDataset.__new__(yunet_amd.datasets.RetinaFaceDataset)
        ds.get_ann_info = lambda i: anns[i]
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            ds.evaluate(dets, device=dev)
        assert ds.evaluate(dets)['mAP'] == 1.0


def test_score_entry_points_refuse_bad_arguments_without_a_launch():
    import ctypes as C
    import yunet_amd._lib as L
    from yunet_amd import kernels as K
    lib = L.load()
    assert K.SCORE_GT_CHUNK == L.SCORE_GT_CHUNK and K.SCORE_BLOCK == L.SCORE_BLOCK
    defs = dict(re.findall(r'#define\s+(YUNET_SCORE_\w+)\s+(\d+)\s', open(os.path.join(ROOT, 'include', 'yunet_hip.h')).read()))
    assert {k: int(v) for k, v in defs.items()} == dict(YUNET_SCORE_BLOCK=L.SCORE_BLOCK, YUNET_SCORE_GT_CHUNK=L.SCORE_GT_CHUNK,
                                                       YUNET_SCORE_MAX_THRESH=L.SCORE_MAX_THRESH)
    buf = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert lib.yunet_score_wider(buf, None, buf, buf, buf, 1, 1, 1, 0.5, buf, 1000, buf, buf, buf, buf, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_wider(buf, buf, buf, buf, buf, 1, 1, 1, 0.5, buf, 1025, buf, buf, buf, buf, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_wider(buf, buf, buf, buf, buf, 1, 2 ** 31, 1, 0.5, buf, 1000, buf, buf, buf, buf, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_wider(buf, buf, buf, buf, buf, -1, 1, 1, 0.5, buf, 1000, buf, buf, buf, buf, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_wider_match(buf, buf, None, buf, 1, 1, 1, 0.5, buf, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_wider_match(buf, buf, buf, buf, 0, 0, 0, 0.5, buf, buf, buf, None) == 0
    assert lib.yunet_score_map_tpfp(buf, buf, buf, buf, None, buf, 1, 1, 1, 0.5, buf, buf, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_map_tpfp(buf, buf, buf, buf, buf, buf, 1, 1, 2 ** 31, 0.5, buf, buf, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_map_tpfp(buf, buf, buf, buf, buf, buf, 1, 0, 1, 0.5, buf, buf, buf, buf, None) == 0
