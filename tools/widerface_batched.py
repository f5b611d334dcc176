#!/usr/bin/env python
"""tools/test_widerface.py through the batched device test pipeline (yunet_amd/test_pipeline.py): the same command line
(CONFIG CHECKPOINT [--out DIR] [--save-preds] [--thr T] [--mode M] [--gt-path D] [--max-images N]) plus `--cache device`,
`--score {host,device}`, `--group canvas`, `--max-batch-pixels N|none` and `--cfg-options K=V ...` (the overrides of
tools/train.py, e.g. model.test_cfg.nms.type=soft_nms model.test_cfg.nms.iou_threshold=0.3; after the positional arguments).

`data.test.samples_per_gpu` is read as the reference's tool reads it (default 1) and `data.test.pipeline` is rewritten
for --mode as the reference's tool does (img_scale of the MultiScaleFlipAug, the size of its Pad; an empty list is the
pipeline evaluation.prepare_test_image hard-codes).  One kernel launch prepares a batch and the detections of a batch
leave the device together; `--cache device` decodes into a device store first.  Origin size (--mode 2) has more batch
geometries than the engine keeps plans: with consecutive batches it runs one image per batch, with the reason printed;
`--group canvas` (or `data.test.group_by = 'canvas'`) batches the images by their padded shape instead, which gives
every image the tensor of the per-image protocol -- the same detections in fewer forwards (`--max-batch-pixels` caps
the canvas pixels of such a batch, default samples_per_gpu * 1024 * 1024).  The prediction files and
the `aps` file are those of tools/test_widerface.py (at one image per batch, text for text); use that tool for
`--eval-only`.
"""
import argparse
import copy
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def per_image_tool():
    """tools/test_widerface.py as a module: its argument parser and its --mode table are used as they are."""
    spec = importlib.util.spec_from_file_location('widerface_per_image', os.path.join(ROOT, 'tools', 'test_widerface.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def mode_pipeline(pipeline, scale):
    """The reference's rewrite of data.test.pipeline for --mode (tools/test_widerface.py:77-96 there): img_scale of the
    MultiScaleFlipAug and the size of its Pad; origin size = scale_factor 1.0 and Pad(size_divisor=32).  A copy."""
    out = copy.deepcopy([dict(t) for t in (pipeline or [])])
    for t in out:
        if t.get('type') == 'MultiScaleFlipAug':
            t['img_scale'] = scale
            t.pop('scale_factor', None)
            if scale is None:
                t['scale_factor'] = 1.0
            t['transforms'] = [dict(x) for x in t.get('transforms') or []]
            for x in t['transforms']:
                if x.get('type') == 'Pad':
                    x['size'], x['size_divisor'] = (scale, None) if scale is not None else (None, 32)
    return out


def own_parser():
    """The options this tool adds to those of tools/test_widerface.py."""
    own = argparse.ArgumentParser(add_help=False)
    own.add_argument('--cache', default=None, choices=['device'],
                     help="'device': decode into a device store and feed the batches from it")
    own.add_argument('--score', default='host', choices=['host', 'device'],
                     help="where the WIDER APs are scored: numpy on the host, or the HIP scorer on the GPU (same APs)")
    own.add_argument('--group', default=None, choices=['canvas'],
                     help="'canvas': batch images of one padded shape together (also data.test.group_by); the per-image "
                          'detections in fewer forwards')
    own.add_argument('--max-batch-pixels', type=lambda v: 'none' if v.lower() == 'none' else int(v), default=None,
                     metavar='N|none',
                     help="canvas pixels a grouped batch may hold, 'none' for no cap (also data.test.max_batch_pixels; "
                          'default samples_per_gpu * 1024 * 1024)')
    from yunet_amd.registry import DictAction
    own.add_argument('--cfg-options', nargs='+', action=DictAction,
                     help='override settings of the config, key.sub=value (e.g. model.test_cfg.nms.type=soft_nms)')
    return own


def main():
    tool = per_image_tool()
    own = own_parser()
    b, rest = own.parse_known_args()
    if '-h' in rest or '--help' in rest:
        own.print_help()
    sys.argv = [sys.argv[0]] + rest
    a = tool.parse_args()
    if a.eval_only:
        raise SystemExit('--eval-only scores saved files: use tools/test_widerface.py')
    if not a.checkpoint:
        raise SystemExit('a checkpoint is required')
    import torch
    import yunet_amd
    from yunet_amd import evaluation as E
    from yunet_amd.test_pipeline import DeviceTestPipeline
    cfg = yunet_amd.Config.fromfile(a.config)
    if b.cfg_options is not None:
        cfg.merge_from_dict(b.cfg_options)
    tcfg = dict(cfg.data.test)
    gt_path = a.gt_path or os.path.join(os.path.dirname(tcfg['ann_file']), 'gt')
    if a.thr != -1.:
        cfg.model.test_cfg.score_thr = a.thr
    dev = torch.device('cuda', 0)
    model = yunet_amd.build_detector(cfg.model)
    ck = torch.load(a.checkpoint, map_location='cpu', weights_only=False)
    model.load_state_dict(ck['state_dict'] if 'state_dict' in ck else ck, strict=True)
    model.to(dev).eval()
    tcfg['test_mode'] = True
    spg = int(tcfg.pop('samples_per_gpu', 1))          # as the reference reads it (tools/test_widerface.py:101-104 there)
    group_by = tcfg.pop('group_by', None)               # the command line wins over the config
    cap = tcfg.pop('max_batch_pixels', 'default')
    group_by = b.group if b.group is not None else group_by
    cap = b.max_batch_pixels if b.max_batch_pixels is not None else cap
    cap = None if cap == 'none' else cap
    ds = yunet_amd.build_dataset(tcfg)
    scale = tool.target_scale(a.mode)
    pipe = DeviceTestPipeline(mode_pipeline(tcfg.get('pipeline') or [], scale), scale=scale)
    dets = E.single_gpu_test(model, ds, dev, scale, a.max_images, samples_per_gpu=spg, pipeline=pipe, cache=b.cache,
                             log=print, group_by=group_by, max_batch_pixels=cap)
    results = E.collect_wider_results(dets, ds, a.out if a.save_preds else None)
    aps = E.wider_evaluation(results, gt_path, 0.5, device=dev if b.score == 'device' else None)
    E.write_aps(a.out, aps)
    print('APS:', aps)


if __name__ == '__main__':
    main()
