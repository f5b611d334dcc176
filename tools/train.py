#!/usr/bin/env python
"""Train YuNet on MI355X -- the command line of the reference's tools/train.py (tools/train.py:24-104):

    CONFIG [--work-dir DIR] [--resume-from CKPT] [--auto-resume] [--no-validate]
           [--gpu-id N | --gpus N | --gpu-ids N ...] [--seed S] [--diff-seed] [--deterministic | --deterministic-fast]
           [--cfg-options K=V ... | --options K=V ...] [--launcher {none,pytorch,slurm,mpi}] [--local_rank R]
           [--auto-scale-lr]

Multi-GPU (one process per GPU, RCCL):
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
      tools/train.py configs/yunet_n.py --launcher pytorch
"""
import argparse
import logging
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import yunet_amd  # noqa: E402
from yunet_amd import runner as R  # noqa: E402
from yunet_amd.parallel import get_dist_info, init_dist  # noqa: E402
from yunet_amd.registry import DictAction  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Train a detector')
    p.add_argument('config', help='train config file path')
    p.add_argument('--work-dir', help='the dir to save logs and models')
    p.add_argument('--resume-from', help='the checkpoint file to resume from')
    p.add_argument('--auto-resume', action='store_true', help='resume from the latest checkpoint automatically')
    p.add_argument('--no-validate', action='store_true', help='whether not to evaluate the checkpoint during training')
    g = p.add_mutually_exclusive_group()
    g.add_argument('--gpus', type=int, help='(deprecated, use --gpu-id) number of gpus (non-distributed training)')
    g.add_argument('--gpu-ids', type=int, nargs='+', help='(deprecated, use --gpu-id) ids of gpus (non-distributed training)')
    g.add_argument('--gpu-id', type=int, default=0, help='id of gpu to use (non-distributed training)')
    p.add_argument('--seed', type=int, default=None, help='random seed')
    p.add_argument('--diff-seed', action='store_true', help='different seeds for different ranks')
    p.add_argument('--deterministic', action='store_true',
                   help='bit-reproducible training step: the same seed, state, build and device model give the same bytes '
                        '(losses, gradients, parameters, BN buffers); one process, fp32 storage; about 1.3x the step time')
    p.add_argument('--deterministic-fast', action='store_true',
                   help="the same contract on the order-fixed forms of the default mode's kernels (cfg.deterministic = 'fast'): "
                        'other bytes than --deterministic, a lower cost; wins over --deterministic when both are given')
    p.add_argument('--options', nargs='+', action=DictAction, help='(deprecated) use --cfg-options')
    p.add_argument('--cfg-options', nargs='+', action=DictAction,
                   help='override settings of the config: key=value pairs, key="[a,b]" or key=a,b for lists, '
                        'nested lists / tuples like key="[(a,b),(c,d)]"; no white space')
    p.add_argument('--launcher', choices=['none', 'pytorch', 'slurm', 'mpi'], default='none', help='job launcher')
    p.add_argument('--local_rank', '--local-rank', type=int, default=0)
    p.add_argument('--auto-scale-lr', action='store_true', help='enable automatically scaling LR')
    p.add_argument('--max-iters', type=int, default=None, help='stop early (smoke runs; not in the reference)')
    a = p.parse_args(argv)
    if 'LOCAL_RANK' not in os.environ:
        os.environ['LOCAL_RANK'] = str(a.local_rank)
    if a.options and a.cfg_options:
        raise ValueError('--options and --cfg-options cannot be both specified, '
                         '--options is deprecated in favor of --cfg-options')
    if a.options:
        warnings.warn('--options is deprecated in favor of --cfg-options')
        a.cfg_options = a.options
    return a


def prepare_config(args):
    """tools/train.py:107-160: config file + command-line overrides -> the configuration of the run."""
    cfg = yunet_amd.Config.fromfile(args.config)
    R.update_data_root(cfg)                       # MMDET_DATASETS (tools/train.py:112-113)
    if args.cfg_options is not None:
        cfg.merge_from_dict(args.cfg_options)
    if args.auto_scale_lr:
        asl = cfg.get('auto_scale_lr')
        if asl is not None and 'enable' in asl and 'base_batch_size' in asl:
            asl['enable'] = True
        else:
            warnings.warn('Can not find "auto_scale_lr" or "auto_scale_lr.enable" or '
                          '"auto_scale_lr.base_batch_size" in your configuration file.')
    # work_dir is determined in this priority: CLI > segment in file > filename
    if args.work_dir is not None:
        cfg['work_dir'] = args.work_dir
    elif cfg.get('work_dir', None) is None:
        cfg['work_dir'] = os.path.join('./work_dirs', os.path.splitext(os.path.basename(args.config))[0])
    if args.resume_from is not None:
        cfg['resume_from'] = args.resume_from
    cfg['auto_resume'] = args.auto_resume
    if args.deterministic:
        cfg['deterministic'] = True                 # the config key of the mode: the dumped config records it
    if args.deterministic_fast:
        cfg['deterministic'] = 'fast'
    if args.gpus is not None:
        cfg['gpu_ids'] = [0]
        warnings.warn('`--gpus` is deprecated because we only support single GPU mode in non-distributed '
                      'training. Use `gpus=1` now.')
    if args.gpu_ids is not None:
        cfg['gpu_ids'] = args.gpu_ids[0:1]
        warnings.warn('`--gpu-ids` is deprecated, please use `--gpu-id`. Because we only support single GPU mode '
                      'in non-distributed training. Use the first GPU in `gpu_ids` now.')
    if args.gpus is None and args.gpu_ids is None:
        cfg['gpu_ids'] = [args.gpu_id]
    return cfg


VAL_SEED_OFFSET = 1000003      # the validation source's seed stream: the train source's seed + this constant


def build_source(cfg, rank, world, seed, dcfg=None):
    """The data source named by dcfg.type (the role of build_dataset + build_dataloader); dcfg = the dataset config to
    build, cfg.data.train by default."""
    dcfg = cfg.data.train if dcfg is None else dcfg
    if dcfg.get('type') == 'MultiImageMixDataset':      # Mosaic: the wrapped dataset with the two pipeline lists as one
        from yunet_amd.datasets import flatten_multi_image_mix, split_skip_type_keys
        dcfg, keys = split_skip_type_keys(dcfg)         # skip_type_keys go to the source, which switches those steps off
        dcfg = type(dcfg)(flatten_multi_image_mix(dcfg))
        if keys is not None:
            dcfg['skip_type_keys'] = keys
    kw = {k: v for k, v in dcfg.items() if k != 'type'}
    if dcfg.get('type') == 'SyntheticWiderFace':
        return R.SyntheticWiderFace(samples_per_gpu=cfg.data.samples_per_gpu, rank=rank, **kw)
    if dcfg.get('type') == 'SyntheticSourceImages':      # device-side reference pipeline
        return R.SyntheticSourceImages(samples_per_gpu=cfg.data.samples_per_gpu, rank=rank, seed=seed, **kw)
    if dcfg.get('type') == 'RetinaFaceDataset':          # labelv2 annotations + image files (PIL decode)
        from yunet_amd.datasets import RetinaFaceSource
        cache = dcfg.get('cache')                        # data.train.cache=device|host: decode once (SourceStore)
        if cache not in (None, 'device', 'host'):
            raise ValueError(f"data.train.cache must be device or host (or unset), got {cache!r}")      # (data.val.cache: the workflow's source)
        host_fetch = dcfg.get('host_fetch')              # data.train.host_fetch=dma|kernel (cache=host only)
        gt_capacity = dcfg.get('gt_capacity')            # data.train.gt_capacity=dataset|N: padded GT rows (RetinaFaceSource)
        if isinstance(gt_capacity, str) and gt_capacity.isdigit():
            gt_capacity = int(gt_capacity)
        ignore_capacity = dcfg.get('ignore_capacity')    # data.train.ignore_capacity=dataset|N: gt_bboxes_ignore in the batch
        if isinstance(ignore_capacity, str) and ignore_capacity.isdigit():
            ignore_capacity = int(ignore_capacity)
        dataset = yunet_amd.build_dataset(dcfg)
        return RetinaFaceSource(dataset, dcfg['pipeline'], samples_per_gpu=cfg.data.samples_per_gpu, rank=rank,
                                world=world, seed=seed, cache=cache, host_fetch=host_fetch, gt_capacity=gt_capacity,
                                skip_type_keys=dcfg.get('skip_type_keys'), ignore_capacity=ignore_capacity)
    raise SystemExit('data sources: RetinaFaceDataset (labelv2 + image files, augmented on the GPU; also wrapped in '
                     'MultiImageMixDataset for Mosaic), '
                     'SyntheticWiderFace (ready batches) or SyntheticSourceImages (decoded synthetic '
                     'sources + the reference train pipeline on the GPU)')


def val_source_config(cfg):
    """The dataset config of a workflow's validation source (the reference's tools/train.py:214-217): a copy of data.val
    with data.train's pipeline -- the flattened list when data.train is a MultiImageMixDataset -- and no test_mode."""
    import copy
    if cfg.data.get('val') is None:
        raise ValueError(f"workflow {cfg.workflow!r} has a second entry, which takes its batches from data.val with "
                         f"data.train's pipeline: the config has no data.val")
    train = cfg.data.train
    if train.get('type') == 'MultiImageMixDataset':
        from yunet_amd.datasets import flatten_multi_image_mix, split_skip_type_keys
        train = flatten_multi_image_mix(split_skip_type_keys(train)[0])
    val = copy.deepcopy(dict(cfg.data.val))
    val['pipeline'] = copy.deepcopy(train['pipeline'])
    val.pop('test_mode', None)
    return type(cfg.data.train)(val)


def build_sources(cfg, rank, world, seed):
    """One source per workflow entry: the training source, and for a two-entry workflow the validation source, built like
    the first (samples_per_gpu, sampler rule, cache / host_fetch handling) from val_source_config on its own seed stream."""
    sources = [build_source(cfg, rank, world, seed)]
    if len(cfg.get('workflow', [('train', 1)])) == 2:
        sources.append(build_source(cfg, rank, world, seed + VAL_SEED_OFFSET, dcfg=val_source_config(cfg)))
    return sources


class TruncatedGtReport(R.Hook):
    """After every training / validation epoch (and at the end of a run cut short): one WARNING per source whose batches
    lost GT rows to the padded width since the last report (RetinaFaceSource.truncated()).  Silent otherwise."""

    def __init__(self, sources, names):
        self.sources = [(n, s) for n, s in zip(names, sources) if hasattr(s, 'truncated')]
        self.seen = {n: (0, 0) for n, _ in self.sources}

    def after_epoch(self, runner):
        for name, src in self.sources:
            images, rows = src.truncated()          # the one host read per epoch
            d_images, d_rows = images - self.seen[name][0], rows - self.seen[name][1]
            self.seen[name] = (images, rows)
            if d_images or d_rows:
                logging.getLogger('yunet_amd.datasets').warning(
                    f'epoch {runner.epoch + 1}: {name} lost {d_rows} GT faces of {d_images} images to the {src.pipe.gmax} '
                    f'padded GT rows (they train as background) -- {name}.gt_capacity=dataset keeps them')

    after_run = after_epoch


def main(argv=None):
    args = parse_args(argv)
    cfg = prepare_config(args)
    distributed = args.launcher != 'none'
    if distributed:
        init_dist(args.launcher, **cfg.get('dist_params', dict(backend='nccl')))
        cfg['gpu_ids'] = list(range(get_dist_info()[1]))
    else:
        torch.cuda.set_device(cfg['gpu_ids'][0])
    rank, world = get_dist_info()
    os.makedirs(os.path.abspath(cfg['work_dir']), exist_ok=True)
    if rank == 0:
        cfg.dump(os.path.join(cfg['work_dir'], os.path.basename(args.config)))      # tools/train.py:171
    timestamp = time.strftime('%Y%m%d_%H%M%S', time.localtime())
    seed = args.seed if args.seed is not None else 0
    seed = seed + rank if args.diff_seed else seed
    if args.deterministic or args.deterministic_fast:
        # (mmdet/apis/train.py: set_random_seed(seed, deterministic=...))
        R.set_random_seed(seed, deterministic='fast' if args.deterministic_fast else True)
    else:
        torch.manual_seed(seed)
    cfg['seed'] = seed
    model = yunet_amd.build_detector(cfg.model)
    model.init_weights()
    sources = build_sources(cfg, rank, world, args.seed if args.seed is not None else 0)
    ds = sources[0] if len(sources) == 1 else sources      # a one-entry workflow hands over the source itself, as before
    main.last_source = sources[0]              # (measurement tools read the source's own timing: tools/train_e2e.py)
    meta = dict(config=cfg.pretty_text, seed=seed, exp_name=os.path.basename(args.config), CLASSES=('face',))
    hist = R.train_detector(model, ds, cfg, distributed=distributed, validate=not args.no_validate,
                            timestamp=timestamp, meta=meta, max_iters=args.max_iters,
                            extra_hooks=[TruncatedGtReport(sources, ['data.train', 'data.val'])])
    dump = os.environ.get('YUNET_DUMP_PARAM_SUM')
    if dump:
        # launcher tests: every rank leaves a checksum of its parameters (data-parallel ranks must end identical)
        with torch.no_grad():
            flat = torch.cat([p.detach().double().reshape(-1) for p in model.parameters()])
            text = f'{float(flat.sum())!r} {float(flat.abs().sum())!r} {float((flat * flat).sum())!r}'
        with open(os.path.join(dump, f'param_sum_rank{rank}.txt'), 'w') as f:
            f.write(text)
    return hist


if __name__ == '__main__':
    main()
