"""CPU: the GT capacity of RetinaFaceSource -- the row rule (pipelines.gt_capacity_rows), the source's constructor on a
label file with crowded images (rows in use, the start-up warning), the config surface of tools/train.py, and the oracle's
crop on more than 64 kept faces against a fixture made by the unmodified reference (tools/make_golden_crowd.py)."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

import pipeline_oracle as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
CFG = os.path.join(ROOT, 'configs', 'yunet_n.py')
GOLD = os.path.join(HERE, 'golden', 'crowd_crop.npz')
COUNTS = [2, 70, 300]


def write_labels(path, counts=COUNTS, w=160, h=128, prefix='im'):
    """A labelv2 file whose image i carries counts[i] faces on a w x h image (a grid of 6 px boxes; no landmarks)."""
    lines = []
    for i, c in enumerate(counts):
        lines.append(f'# {prefix}{i}.png {w} {h}')
        for g in range(c):
            x, y = 2 + 7 * (g % 22), 2 + 7 * (g // 22)
            lines.append(f'{x} {y} {x + 6} {y + 6} ' + ' '.join(['-1'] * 15))
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return str(path)


def ref_pipeline():
    import yunet_amd
    return yunet_amd.Config.fromfile(CFG).data.train.pipeline


def make_source(tmp_path, **kw):
    from yunet_amd.datasets import RetinaFaceDataset, RetinaFaceSource
    ds = RetinaFaceDataset(write_labels(tmp_path / 'l.txt'), img_prefix=str(tmp_path))
    return RetinaFaceSource(ds, kw.pop('pipeline', None) or ref_pipeline(), samples_per_gpu=3, workers=0, **kw)


def test_row_rule_table():
    from yunet_amd.pipelines import gt_capacity_rows
    for count, rows in [(1, 64), (64, 64), (65, 128), (300, 512), (1968, 2048), (4096, 4096)]:
        assert gt_capacity_rows(count) == rows
    with pytest.raises(ValueError, match='LDS'):
        gt_capacity_rows(4097)
    assert gt_capacity_rows(300, mosaic=True) == 256 and gt_capacity_rows(65, mosaic=True) == 128
    assert gt_capacity_rows(4097, mosaic=True) == 256
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            gt_capacity_rows(bad)


def test_default_source_caps_at_64_and_says_so(tmp_path, caplog):
    with caplog.at_level(logging.WARNING):
        src = make_source(tmp_path)
    assert src.pipe.gmax == 64 and src.gt_rows == 64
    lines = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(lines) == 1, lines
    assert '2 images' in lines[0] and '300' in lines[0] and '242 faces' in lines[0] and 'gt_capacity' in lines[0]
    assert src.truncated() == (0, 0)                      # nothing ran: no device is touched
    # max_gt keeps its meaning, 300 -> 128 included
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        assert make_source(tmp_path, max_gt=300).pipe.gmax == 128
    assert '1 images' in caplog.records[0].getMessage() and '172 faces' in caplog.records[0].getMessage()


def test_capacity_from_the_dataset_and_as_a_number(tmp_path, caplog):
    with caplog.at_level(logging.WARNING):
        src = make_source(tmp_path, gt_capacity='dataset')
        assert src.pipe.gmax == 512 and src.pipe.cfg.gmax == 512
        assert make_source(tmp_path, gt_capacity=300).pipe.gmax == 512
    assert not caplog.records
    with caplog.at_level(logging.WARNING):
        assert make_source(tmp_path, gt_capacity=100).pipe.gmax == 128
    assert len(caplog.records) == 1 and '1 images' in caplog.records[0].getMessage()
    with pytest.raises(ValueError, match='max_gt'):
        make_source(tmp_path, gt_capacity='dataset', max_gt=128)
    with pytest.raises(ValueError, match='max_gt'):
        make_source(tmp_path, gt_capacity=100, max_gt=300)
    for bad in ('all', 0, 5000):
        with pytest.raises(ValueError):
            make_source(tmp_path, gt_capacity=bad)


def test_capacity_counts_only_the_rows_get_ann_info_returns(tmp_path):
    """Ignored faces (min_size) are not GT rows: 70 faces of 6 px under min_size=7 leave nothing to size for."""
    from yunet_amd.datasets import RetinaFaceDataset, gt_counts
    path = write_labels(tmp_path / 'l.txt')
    assert gt_counts(RetinaFaceDataset(path)) == COUNTS
    assert gt_counts(RetinaFaceDataset(path, min_size=7)) == [0, 0, 0]


def mosaic_pipeline():
    p = [dict(t) for t in ref_pipeline()]
    return p[:2] + [dict(type='Mosaic', img_scale=(320, 320), use_kps=True)] + p[2:]


def test_mosaic_limits_the_rows_per_image_to_256(tmp_path, caplog):
    with caplog.at_level(logging.WARNING):
        src = make_source(tmp_path, pipeline=mosaic_pipeline(), gt_capacity='dataset', cache='device')
    assert src.gt_rows == 256 and src.pipe.gmax == 1024
    msg = [r.getMessage() for r in caplog.records]
    assert len(msg) == 1 and '1 images' in msg[0] and '44 faces' in msg[0] and 'Mosaic' in msg[0]
    assert make_source(tmp_path, pipeline=mosaic_pipeline(), cache='device').pipe.gmax == 256      # the default: 4 x 64


# ---------------------------------------------------------------------------------------------------- tools/train.py
def built_sources(tmp_path, monkeypatch, options, extra_cfg=''):
    """tools/train.py main() up to the hand-over, on a config whose data.train is a RetinaFaceDataset over the label file."""
    import train as TT
    write_labels(tmp_path / 'l.txt')
    cfg_path = tmp_path / 'yunet_n.py'
    cfg_path.write_text(open(CFG).read() + f"""
data['train'] = dict(type='RetinaFaceDataset', ann_file={str(tmp_path / 'l.txt')!r}, img_prefix={str(tmp_path)!r},
                     pipeline=train_pipeline)
data['samples_per_gpu'] = 3
""" + extra_cfg)
    seen = {}

    def fake_train(model, ds, cfg, **kw):
        seen.update(ds=ds, cfg=cfg, kw=kw)
        return []

    monkeypatch.setattr(TT.R, 'train_detector', fake_train)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda i: None)
    TT.main([str(cfg_path), '--work-dir', str(tmp_path / 'w'), '--no-validate'] + (['--cfg-options'] + options if options else []))
    return seen


def test_train_tool_passes_the_key_on(tmp_path, monkeypatch):
    seen = built_sources(tmp_path, monkeypatch, ['data.train.gt_capacity=dataset'])
    assert type(seen['ds']).__name__ == 'RetinaFaceSource' and seen['ds'].pipe.gmax == 512
    assert len(seen['kw']['extra_hooks']) == 1
    assert built_sources(tmp_path, monkeypatch, ['data.train.gt_capacity=100'])['ds'].pipe.gmax == 128
    assert built_sources(tmp_path, monkeypatch, [])['ds'].pipe.gmax == 64


def test_train_tool_passes_the_key_on_through_multi_image_mix(tmp_path, monkeypatch):
    wrap = """
_inner = dict(data['train'])
_inner['pipeline'] = _inner['pipeline'][:2]
data['train'] = dict(type='MultiImageMixDataset', dataset=_inner, cache='device',
                     pipeline=[dict(type='Mosaic', img_scale=(320, 320), use_kps=True)] + data['train']['pipeline'][2:])
"""
    seen = built_sources(tmp_path, monkeypatch, ['data.train.dataset.gt_capacity=dataset'], wrap)
    assert seen['ds'].pipe.mosaic is not None and seen['ds'].gt_rows == 256 and seen['ds'].pipe.gmax == 1024
    seen = built_sources(tmp_path, monkeypatch, ['data.train.dataset.gt_capacity=100'], wrap)
    assert seen['ds'].gt_rows == 128 and seen['ds'].pipe.gmax == 512
    assert built_sources(tmp_path, monkeypatch, [], wrap)['ds'].pipe.gmax == 256


def test_train_tool_passes_the_key_on_to_the_validation_source(tmp_path, monkeypatch):
    val = f"""
data['val'] = dict(type='RetinaFaceDataset', ann_file={str(tmp_path / 'l.txt')!r}, img_prefix={str(tmp_path)!r},
                   test_mode=True, pipeline=[])
"""
    seen = built_sources(tmp_path, monkeypatch, ["workflow=[('train',1),('val',1)]", 'data.val.gt_capacity=dataset'], val)
    train, valsrc = seen['ds']
    assert train.pipe.gmax == 64 and valsrc.pipe.gmax == 512
    import train as TT
    assert TT.val_source_config(seen['cfg'])['gt_capacity'] == 'dataset'


class _Src:
    class pipe:
        gmax = 64

    def __init__(self):
        self.t = (0, 0)

    def truncated(self):
        return self.t


def test_truncation_report_is_silent_until_rows_are_lost(caplog):
    import train as TT

    class Runner:
        epoch = 0
    src = _Src()
    hook = TT.TruncatedGtReport([src, object()], ['data.train', 'data.val'])
    with caplog.at_level(logging.WARNING):
        hook.after_train_epoch(Runner())
        assert not caplog.records
        src.t = (3, 250)
        hook.after_train_epoch(Runner())
        assert len(caplog.records) == 1
        m = caplog.records[0].getMessage()
        assert '250 GT faces' in m and '3 images' in m and 'data.train.gt_capacity=dataset' in m
        hook.after_run(Runner())                          # nothing new since the last report
        assert len(caplog.records) == 1


# ---------------------------------------------------------------------------------------------------- the golden
def load_crowd():
    g = np.load(GOLD)
    rng = np.random.default_rng(int(g['seed']))
    srcs = []
    for i in range(int(g['n'])):
        h, w, total = (int(v) for v in g[f'src_shape_{i}'])
        im, b, k = P.synth_image(rng, h, w, len(g[f'src_boxes_{i}']))
        assert int(im.astype(np.int64).sum()) == total and np.array_equal(b, g[f'src_boxes_{i}']), 'generator drift'
        srcs.append((im, g[f'src_boxes_{i}'], g[f'src_kps_{i}']))
    return g, srcs


def test_oracle_crop_on_crowded_images_vs_reference_golden():
    g, srcs = load_crowd()
    seed, it, S = int(g['seed']), int(g['iteration']), int(g['S'])
    kept_all = []
    for i, (im, boxes, kps) in enumerate(srcs):
        left, top, cw, flip, draws, kept = (int(v) for v in g[f'meta_{i}'])
        st = P.Stream(seed, it, i)
        assert P.decide_crop(im.shape[0], im.shape[1], boxes, g['crop_choice'], st) == (left, top, cw)
        b, k, mask = P.crop_gt(boxes, kps, left, top, cw)
        assert int(mask.sum()) == kept
        b, k = P.resize_gt(b, k, cw, S)
        assert (st.uniform() < 0.5) == bool(flip) and st.ctr == draws
        if flip:
            b, k = P.flip_gt(b, k, S)
        assert np.array_equal(b, g[f'boxes_{i}']) and np.array_equal(k, g[f'kps_{i}'])
        kept_all.append(kept)
    assert kept_all[0] > 128 and kept_all[1] > 64 and len(srcs[0][1]) == 300 and len(srcs[1][1]) == 65
