"""-m gpu: bench.py's timed window, --dump-outputs and a plain run without --full.  `steps` / `ms_per_step` describe
exactly the --steps steps that were timed, and the dump holds what the last of them handed its caller (losses,
gradients, updated state), with the same inputs -- hence the same outputs up to the summation order of the fp64
atomics -- from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ['--steps', '3', '--warmup', '1', '--batch', '32', '--no-cpu-baseline', '--no-roofline', '--no-other-configs',
        '--no-exact-bwd', '--no-gpu-eager']


def _bench(out_dir, args=ARGS):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *args, '--dump-outputs', str(out_dir)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}


def test_bench_times_exactly_the_requested_steps_and_dumps_the_last_one(tmp_path):
    import torch
    import yunet_amd
    res, got = _bench(tmp_path / 'a')
    assert res['steps'] == 3 and res['ms_per_step'] > 0
    assert res['value'] == pytest.approx(32 * 1000.0 / res['ms_per_step'], rel=1e-2)

    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    model = yunet_amd.build_detector(cfg.model)
    want = {'loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps', 'loss', 'momentum_buffer'}
    want |= {f'grad.{k}' for k, _ in model.named_parameters()} | {f'state.{k}' for k in model.state_dict()}
    assert set(got) == want
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), k
    for k, v in model.state_dict().items():
        assert got[f'state.{k}'].shape == tuple(v.shape), k
    assert float(got['loss']) == pytest.approx(res['final_loss'], abs=1e-4)
    assert float(got['loss']) == pytest.approx(sum(float(got[k]) for k in ('loss_cls', 'loss_bbox', 'loss_obj',
                                                                            'loss_kps')), rel=1e-5)
    assert any(np.abs(v).max() > 0 for k, v in got.items() if k.startswith('grad.'))
    fixture = torch.load(os.path.join(ROOT, 'tests', 'golden', 'yunet_n_synth_trained.pth'), map_location='cpu',
                         weights_only=False)['state_dict']
    w = 'backbone.model0.conv1.weight'
    assert not np.array_equal(got[f'state.{w}'], fixture[w].numpy())      # the dump is after the SGD updates

    _, again = _bench(tmp_path / 'b')
    for k, v in got.items():
        scale = float(np.abs(v).max()) if v.size else 0.0
        assert np.abs(again[k].astype(np.float64) - v).max(initial=0.0) <= 1e-5 * scale + 1e-9, k


def test_plain_run_measures_the_headline_only(tmp_path):
    """Without --full (and without any --no-* switch) the run is set-up, warm-up, the timed window, the dump and the
    line: none of the side measurements that --full adds after the window."""
    res, got = _bench(tmp_path / 'plain', ['--steps', '2', '--warmup', '1', '--batch', '32'])
    assert {'metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'final_loss'} <= set(res)
    assert res['steps'] == 2 and res['warmup'] == 1 and res['dtype'] == 'f32' and res['higher_is_better'] is True
    assert not {'roofline', 'kernels', 'families', 'exact_fp32_bwd', 'other_configs', 'cpu_baseline'} & set(res), res
    assert float(got['loss']) == pytest.approx(res['final_loss'], abs=1e-4)
