"""CPU: the plumbing of the device ranking of the mAP protocol (eval_map_single_class(rank='device'), csrc/score.hip's
yunet_score_rank_* / yunet_score_map_curve): the option's errors, the new symbols and constants in header, library and
ctypes table with the ABI number unchanged, the entry points' argument checks without a launch, and the default path
on the stored results of the unmodified reference."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import test_eval_map as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'yunet_hip.h')
NEW = ('yunet_score_rank_scratch_bytes', 'yunet_score_rank_images', 'yunet_score_rank_global', 'yunet_score_map_curve')


def _one_image():
    dets = [np.array([[0., 0., 10., 10., 0.9], [0., 0., 10., 10.5, 0.8]], np.float32)]
    anns = [dict(bboxes=np.array([[0., 0., 10., 10.], [20., 20., 30., 30.]], np.float32),
                 bboxes_ignore=np.zeros((0, 4), np.float32))]
    return dets, anns


def test_rank_option_errors():
    import yunet_amd
    import yunet_amd.evaluation as E
    dets, anns = _one_image()
    with pytest.raises(ValueError, match="rank='device'"):
        E.eval_map_single_class(dets, anns, 0.5, rank='device')              # no device: nothing to rank on
    with pytest.raises(ValueError, match='bogus'):
        E.eval_map_single_class(dets, anns, 0.5, rank='bogus')
    with pytest.raises(ValueError, match='host'):
        E.eval_map_single_class(dets, anns, 0.5, device='cuda', rank='host')  # refused before any device is touched
    ds = yunet_amd.datasets.RetinaFaceDataset.__new__(yunet_amd.datasets.RetinaFaceDataset)
    ds.get_ann_info = lambda i: anns[i]
    with pytest.raises(ValueError, match="rank='device'"):
        ds.evaluate(dets, rank='device')
    with pytest.raises(ValueError, match='bogus'):
        ds.evaluate(dets, rank='bogus')
    assert ds.evaluate(dets) == ds.evaluate(dets, rank=None) and ds.evaluate(dets)['mAP'] == 0.5
    # with a device that is no GPU the device scorer's own error comes first: no host fallback, also for an empty set
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        E.eval_map_single_class(dets, anns, 0.5, device='cpu', rank='device')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        E.eval_map_single_class([np.zeros((0, 5), np.float32)], anns, 0.5, device='cpu', rank='device')


def test_eval_hook_rank_option():
    import yunet_amd.runner as R
    for kw in (dict(rank='device'), dict(score='host', rank='device'), dict(score=None, rank='device')):
        with pytest.raises(ValueError, match="score='device'"):
            R.EvalHook(None, **kw)
    for kw in (dict(score='device', rank='bogus'), dict(rank='host')):
        with pytest.raises(ValueError, match='rank='):
            R.EvalHook(None, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                  # the key is the hook's own now: not "unsupported and ignored"
        hook = R.EvalHook(None, score='device', rank='device')
        assert hook.rank == 'device' and hook.score == 'device'
        assert R.EvalHook(None, score='device').rank is None and R.EvalHook(None).rank is None


def test_symbols_constants_and_abi():
    import yunet_amd._lib as L
    from yunet_amd import kernels as K
    lib = L.load()
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r'\b(?:int|size_t)\s+(yunet_\w+)\s*\(', txt))
    for name in NEW:
        assert name in declared and name in L.EXPORTED and hasattr(lib, name), name
    assert lib.yunet_abi_version() == 12
    defs = {k: int(v) for k, v in re.findall(r'#define\s+(YUNET_RANK_\w+)\s+(\d+)\s', open(HEADER).read())}
    assert defs == dict(YUNET_RANK_SEG_CAP=L.RANK_SEG_CAP, YUNET_RANK_RADIX_TILE=L.RANK_RADIX_TILE,
                        YUNET_RANK_CURVE_MAX=L.RANK_CURVE_MAX)
    assert (K.RANK_SEG_CAP, K.RANK_RADIX_TILE, K.RANK_CURVE_MAX) == (L.RANK_SEG_CAP, L.RANK_RADIX_TILE, L.RANK_CURVE_MAX)
    assert L.RANK_CURVE_MAX == 2 ** 24 and L.RANK_SEG_CAP % L.SCORE_BLOCK == 0 and L.RANK_RADIX_TILE % L.SCORE_BLOCK == 0


def test_entry_points_refuse_bad_arguments_without_a_launch():
    import yunet_amd._lib as L
    lib = L.load()
    buf = C.c_void_p(C.addressof(C.create_string_buffer(64)) + 7 & ~7)
    odd = C.c_void_p(buf.value + 4)
    assert lib.yunet_score_rank_images(buf, buf, 1, 2 ** 31, buf, None) == L.EINVAL
    assert lib.yunet_score_rank_images(buf, buf, -1, 1, buf, None) == L.EINVAL
    assert lib.yunet_score_rank_images(buf, None, 1, 1, buf, None) == L.EINVAL
    assert lib.yunet_score_rank_images(None, None, 0, 0, None, None) == 0
    assert lib.yunet_score_rank_global(buf, 2 ** 31, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_rank_global(buf, 1, buf, None, None) == L.EINVAL
    assert lib.yunet_score_rank_global(buf, 1, buf, odd, None) == L.EINVAL
    assert lib.yunet_score_rank_global(None, 0, None, None, None) == 0
    assert lib.yunet_score_map_curve(buf, buf, buf, 2 ** 24, buf, buf, buf, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_map_curve(buf, buf, buf, -1, buf, buf, buf, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_map_curve(buf, buf, None, 1, buf, buf, buf, buf, buf, None) == L.EINVAL
    assert lib.yunet_score_map_curve(buf, buf, buf, 1, buf, buf, buf, buf, odd, None) == L.EINVAL
    assert lib.yunet_score_map_curve(None, None, None, 0, None, None, None, None, None, None) == 0
    # three [D] words and the [256][tiles] histogram; the curve's per-tile sums and maxima fit in it
    for D in (1, L.RANK_RADIX_TILE, L.RANK_RADIX_TILE + 1, 10 ** 6):
        tiles = -(-D // L.RANK_RADIX_TILE)
        got = lib.yunet_score_rank_scratch_bytes(D)
        assert got >= 4 * (3 * D + 256 * tiles) and got >= 12 * tiles
    assert lib.yunet_score_rank_scratch_bytes(-1) == 0 and lib.yunet_score_rank_scratch_bytes(2 ** 31) == 0


def test_area_from_envelope_is_average_precision_area():
    """The vectorised tail of the device path forms the terms average_precision_area forms: the same float32."""
    import yunet_amd.evaluation as E
    rng = np.random.default_rng(0)
    for n, full in ((0, False), (1, True), (40, False), (333, True)):
        tp = np.cumsum(rng.uniform(size=n) < 0.4).astype(np.float32)
        fp = (np.arange(1, n + 1) - tp).astype(np.float32)
        num_gts = int(tp[-1]) if (full and n) else int(tp[-1]) + 3 if n else 2
        recalls = tp / np.maximum(np.array([num_gts]), np.finfo(np.float32).eps)
        prec = tp / np.maximum(tp + fp, np.finfo(np.float32).eps)
        env = np.maximum.accumulate(prec[::-1])[::-1]
        want, got = E.average_precision_area(recalls, prec), E.area_from_envelope(recalls, env)
        assert got.dtype == want.dtype == np.float32 and got == want
        if n and tp[-1] > 0:
            assert (recalls[-1] == 1.0) == full          # with and without the trailing term


@pytest.mark.parametrize('seed', TM.SEEDS)
def test_default_path_is_untouched(seed):
    """Without `rank` (and with rank=None) eval_map_single_class returns what it returned before: the stored results
    of the unmodified reference on the fixture of tests/test_eval_map.py."""
    import yunet_amd.evaluation as E
    with np.load(TM.STORED) as z:
        ref = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(f'{seed}/')}
    dets, anns = TM._case(np.random.default_rng(seed))
    for thr in TM.THRS:
        for kw in ({}, dict(rank=None), dict(device=None, rank=None)):
            got, res = E.eval_map_single_class(dets, anns, thr, **kw)
            assert got == pytest.approx(float(ref[f'{thr}/mean_ap']), abs=1e-7)
            assert res['num_gts'] == ref[f'{thr}/num_gts'] and res['num_dets'] == ref[f'{thr}/num_dets']
            assert res['recall'].dtype == np.float64 and res['precision'].dtype == np.float32
            assert isinstance(res['ap'], np.float32)
            assert np.array_equal(res['recall'], ref[f'{thr}/recall'])
            assert np.array_equal(res['precision'], ref[f'{thr}/precision'])
