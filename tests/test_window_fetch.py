"""CPU: the configuration of the kernel window fetch (WindowFeed fetch=, host_fetch= of both window sources, tools/train.py
and tools/train_e2e.py forwarding) and a static guard on yunet_fetch_windows' device code (no GPU calls)."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path.split('/')))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _cfg():
    import yunet_amd
    return yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))


def _labelv2(tmp_path):
    (tmp_path / 'a.jpg').write_bytes(b'')
    (tmp_path / 'labelv2.txt').write_text('# a.jpg 64 48\n1 2 30 40 ' + ' '.join(['5 6 0.0'] * 5) + ' 0.9\n')
    return str(tmp_path / 'labelv2.txt')


@pytest.mark.parametrize('bad', ['DMA', 'device', 1, True])
def test_window_feed_rejects_unknown_fetch(bad):
    from yunet_amd.source_store import SourceStore, WindowFeed
    st = SourceStore([(4, 4)], placement='host', device='cpu')
    with pytest.raises(ValueError, match='fetch'):
        WindowFeed(None, st, 64, fetch=bad)


def test_synthetic_sources_host_fetch_config():
    import yunet_amd.runner as R
    pipe = _cfg().train_pipeline
    for bad in ('DMA', 'window', 2):
        with pytest.raises(ValueError, match='host_fetch'):
            R.SyntheticSourceImages(pipe, host_fed='window', host_fetch=bad)
    for host_fed in (False, True):
        for fetch in ('dma', 'kernel'):
            with pytest.raises(ValueError, match='host_fetch'):
                R.SyntheticSourceImages(pipe, host_fed=host_fed, host_fetch=fetch)
    for fetch in (None, 'dma', 'kernel'):
        assert R.SyntheticSourceImages(pipe, host_fed='window', host_fetch=fetch).host_fetch == fetch
    assert R.SyntheticSourceImages(pipe).host_fetch is None


def test_retinaface_source_host_fetch_config(tmp_path):
    from yunet_amd.datasets import RetinaFaceDataset, RetinaFaceSource
    cfg = _cfg()
    ds = RetinaFaceDataset(_labelv2(tmp_path), img_prefix=str(tmp_path), pipeline=cfg.train_pipeline)
    for cache in (None, 'device'):
        with pytest.raises(ValueError, match='host_fetch'):
            RetinaFaceSource(ds, cfg.train_pipeline, samples_per_gpu=1, cache=cache, host_fetch='kernel')
    with pytest.raises(ValueError, match='host_fetch'):
        RetinaFaceSource(ds, cfg.train_pipeline, samples_per_gpu=1, cache='host', host_fetch='zero-copy')
    for fetch in (None, 'dma', 'kernel'):
        src = RetinaFaceSource(ds, cfg.train_pipeline, samples_per_gpu=1, cache='host', host_fetch=fetch)
        assert src.host_fetch == fetch and src.store is None


@pytest.mark.parametrize('fetch', [None, 'dma', 'kernel'])
def test_train_tool_forwards_host_fetch(tmp_path, fetch):
    T = _load('yunet_train_tool_fetch', 'tools/train.py')
    cfg = _cfg()
    cfg.data.train.type = 'RetinaFaceDataset'
    cfg.data.train.ann_file = _labelv2(tmp_path)
    cfg.data.train.img_prefix = str(tmp_path)
    cfg.data.train.cache = 'host'
    cfg.data.samples_per_gpu = 1
    if fetch is not None:
        cfg.data.train.host_fetch = fetch
    assert T.build_source(cfg, 0, 1, 0).host_fetch == fetch
    cfg = _cfg()
    cfg.data.train.type = 'SyntheticSourceImages'
    cfg.data.train.host_fed = 'window'
    if fetch is not None:
        cfg.data.train.host_fetch = fetch
    assert T.build_source(cfg, 0, 1, 0).host_fetch == fetch
    cfg.data.train.host_fed = True
    if fetch is not None:
        with pytest.raises(ValueError, match='host_fetch'):
            T.build_source(cfg, 0, 1, 0)


def test_train_e2e_has_the_kernel_window_mode(monkeypatch, capsys):
    import torch
    E = _load('yunet_train_e2e_fetch', 'tools/train_e2e.py')
    seen = []

    class FakeTrain:
        @staticmethod
        def main(argv):
            seen.append(argv)
            return [dict(time=0.01, loss=1.0)] * 4
    monkeypatch.setattr(E, 'load_train_tool', lambda: FakeTrain)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, 'empty_cache', lambda *a, **k: None)
    monkeypatch.setattr('sys.argv', ['train_e2e.py', '--iters', '4', '--modes', 'host_fed,host_window_kernel'])
    E.main()
    assert len(seen) == 2
    assert 'data.train.host_fed=True' in seen[0] and not any('host_fetch' in a for a in seen[0])
    assert 'data.train.host_fed=window' in seen[1] and 'data.train.host_fetch=kernel' in seen[1]
    assert '"host_window_kernel"' in capsys.readouterr().out


def _fetch_kernel_asm(tmp_path):
    out = str(tmp_path / 'source.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-w', '-S', '--cuda-device-only',
                    '-o', out, os.path.join(ROOT, 'libfacedetection.train_amd', 'csrc', 'source.hip')], check=True,
                   capture_output=True, timeout=600)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
def test_fetch_kernel_issues_its_loads_before_waiting(tmp_path):
    """tools/dbg/serial_loads.py finds no loop in the fetch kernel that waits out every load, and the kernel's main copy
    path issues 16 16-byte loads per thread with no vmcnt wait between them."""
    path = _fetch_kernel_asm(tmp_path)
    scan = _load('serial_loads_fetch', 'tools/dbg/serial_loads.py').scan
    assert not [x for x in scan(path) if 'fetch_windows' in x[3]]
    text = open(path).read()
    m = re.search(r'^(_Z\w*fetch_windows_kernel\w*):[^\n]*\n(.*?)s_endpgm', text, flags=re.S | re.M)
    assert m, 'fetch_windows_kernel not found in the assembly'
    run = best = 0
    for line in m.group(2).split('\n'):
        s = line.strip()
        if s.startswith('global_load_dwordx4'):
            run += 1
            best = max(best, run)
        elif s.startswith('s_waitcnt') and 'vmcnt' in s:
            run = 0
    assert best >= 16, best
