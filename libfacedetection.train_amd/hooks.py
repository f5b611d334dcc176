"""The reference's custom training hooks (mmdet/core/hook/) that a YuNet config can name in `custom_hooks`:

    ExpMomentumEMAHook, LinearMomentumEMAHook   (ema.py)       exponential moving average of the model
    YuNetSampleSizeStatisticsHook               (yunet_sample_size_statistics_hook.py)  GT box-size histogram
    CheckInvalidLossHook                        (checkloss_hook.py)  the loss must stay finite
    YOLOXModeSwitchHook                         (yolox_mode_switch_hook.py)  Mosaic / RandomAffine / MixUp off for the last epochs

Semantics are the reference's; what differs is where the per-iteration work runs.  On a model bound to the fused
engine the EMA update is ONE launch over the flat parameter / BN buffers and their flat EMA mirror
(yunet_ema_update, FlatParams.enable_ema), and the box-size histogram is one launch over the padded device GT
(yunet_box_size_hist) whose grid is read back once per dump -- no per-tensor loop, no per-box host sync.  A model
without an engine (a plain nn.Module) takes the reference's per-tensor loop.
"""
import json
import math
import os
from datetime import datetime

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .runner import HOOKS, Hook


def _unwrap(model):
    return model.module if hasattr(model, 'module') else model


class BaseEMAHook(Hook):
    """mmdet/core/hook/ema.py BaseEMAHook:  ema = (1 - momentum) * ema + momentum * value  every `interval`
    iterations for every floating-point state_dict entry (parameters only with skip_buffers=True), kept as
    `ema_<name with '.' -> '_'>` buffers of the unwrapped model; the live and EMA values are swapped at every epoch
    end (so CheckpointHook / EvalHook registered after this hook see the EMA) and back at the next epoch's start."""

    def __init__(self, momentum=0.0002, interval=1, skip_buffers=False, resume_from=None, momentum_fun=None):
        assert 0 < momentum < 1
        self.momentum = momentum
        self.skip_buffers = skip_buffers
        self.interval = interval
        self.checkpoint = resume_from
        self.momentum_fun = momentum_fun

    def before_run(self, runner):
        model = _unwrap(runner.model)
        self.param_ema_buffer = {}
        entries = dict(model.named_parameters()) if self.skip_buffers else model.state_dict()
        for name, value in entries.items():
            buffer_name = f"ema_{name.replace('.', '_')}"
            self.param_ema_buffer[name] = buffer_name
            model.register_buffer(buffer_name, value.data.clone())
        if hasattr(model, 'bind_ema'):
            model.bind_ema()             # an engine that already exists takes the buffers into its mirror now
        if self.checkpoint is not None:
            runner.resume(self.checkpoint)

    def get_momentum(self, runner):
        return self.momentum_fun(runner.iter) if self.momentum_fun else self.momentum

    def _mirror(self, model):
        """The engine's (fp32 pairs, other pairs) of live / EMA flat buffers, or None for a model without an engine.
        The engine binds lazily (first forward, after before_run) and again after a move: its mirror is always
        (re)made from the ema_ buffers by bind_engine."""
        eng = getattr(model, 'engine', None)
        if eng is None or not model._bound():
            return None
        f32, other = eng.params.ema_pairs()
        if not f32 and not model.bind_ema():
            raise RuntimeError('EMA hook: the engine-bound model has no ema_ buffers (before_run did not run?)')
        return eng.params.ema_pairs()

    def _entries(self, model):
        live = dict(model.named_parameters()) if self.skip_buffers else model.state_dict()
        return live, dict(model.named_buffers())

    def after_train_iter(self, runner):
        if (runner.iter + 1) % self.interval != 0:
            return
        momentum = self.get_momentum(runner)
        model = _unwrap(runner.model)
        mirror = self._mirror(model)
        if mirror is not None:
            K.ema_update(mirror[0], momentum)          # num_batches_tracked (int64) is never averaged
            return
        live, bufs = self._entries(model)
        with torch.no_grad():
            for name, buffer_name in self.param_ema_buffer.items():
                parameter = live[name]
                if parameter.dtype.is_floating_point:
                    bufs[buffer_name].mul_(1 - momentum).add_(parameter.data, alpha=momentum)

    def after_train_epoch(self, runner):
        self._swap_ema_parameters(runner)

    def before_train_epoch(self, runner):
        self._swap_ema_parameters(runner)

    def _swap_ema_parameters(self, runner):
        model = _unwrap(runner.model)
        mirror = self._mirror(model)
        with torch.no_grad():
            if mirror is not None:
                # the flat buffers hold exactly the entries (the head's structurally-zero rows are zero on both sides)
                for value, ema in mirror[0] + mirror[1]:
                    temp = value.clone()
                    value.copy_(ema)
                    ema.copy_(temp)
                return
            live, bufs = self._entries(model)
            for name, buffer_name in self.param_ema_buffer.items():
                value, ema = live[name], bufs[buffer_name]
                temp = value.data.clone()
                value.data.copy_(ema.data)
                ema.data.copy_(temp)


class ExpMomentumEMAHook(BaseEMAHook):
    """momentum(x) = (1 - momentum) * exp(-(1 + x) / total_iter) + momentum."""

    def __init__(self, total_iter=2000, **kwargs):
        super().__init__(**kwargs)
        self.momentum_fun = lambda x: (1 - self.momentum) * math.exp(-(1 + x) / total_iter) + self.momentum


class LinearMomentumEMAHook(BaseEMAHook):
    """momentum(x) = min(momentum ** interval, (1 + x) / (warm_up + x))."""

    def __init__(self, warm_up=100, **kwargs):
        super().__init__(**kwargs)
        self.momentum_fun = lambda x: min(self.momentum ** self.interval, (1 + x) / (warm_up + x))


class YuNetSampleSizeStatisticsHook(Hook):
    """mmdet/core/hook/yunet_sample_size_statistics_hook.py: a histogram of the (int(w), int(h)) sizes of the GT boxes
    as the augmented batches reach the model, dumped to work_dir/out_file at the start of every save_interval-th epoch
    (keys in first-seen order: iteration, then image, then box).

    Device batches (GTList.padded / .counts on the GPU): one yunet_box_size_hist launch per iteration into a
    persistent int64 grid over [0, W] x [0, H] of the first batch's image size (count + first-seen key per bin); a box
    outside the grid is kept in a device spill list with its fp32 (w, h), and the dump converts those on the host.
    The grid is read back once per dump.  Host batches take the reference's loop.  The state is not checkpointed
    (nor is it in the reference)."""

    SPILL_CAP = 1 << 16

    def __init__(self, out_file, save_interval=50):
        self.out_file = out_file
        self.save_interval = save_interval
        self.batch_size = 0
        self.shapeless2 = 0
        self._dev = None                                 # device grid state (allocated at the first device batch)
        self._host = {}                                  # tag -> [count, first key] of host batches
        self._host_total = self._host_noimg = 0

    def before_run(self, runner):
        self.out_file = os.path.join(runner.work_dir, self.out_file)

    def before_epoch(self, runner):
        self.epoch = runner.epoch
        if (self.epoch + 1) % self.save_interval == 0:
            self.dump_json()

    def before_train_iter(self, runner):
        batch = runner.data_batch
        gt = batch['gt_bboxes']
        self.batch_size = len(gt)
        padded, counts = getattr(gt, 'padded', None), getattr(gt, 'counts', None)
        if padded is not None and padded.is_cuda:
            self._device_batch(batch, padded, counts, runner.iter)
        else:
            self._host_batch(gt, runner.iter)

    def _device_batch(self, batch, padded, counts, it):
        if self._dev is None:
            img = batch.get('img')
            if img is not None:
                H, W = int(img.shape[-2]), int(img.shape[-1])
            else:
                H, W = batch['img_metas'][0]['pad_shape'][:2]
            dev = padded.device
            self._dev = dict(count=torch.zeros(H + 1, W + 1, dtype=torch.int64, device=dev),
                             first=torch.full((H + 1, W + 1), -1, dtype=torch.int64, device=dev),
                             totals=torch.zeros(4, dtype=torch.int64, device=dev),
                             spill=torch.zeros(self.SPILL_CAP, 2, dtype=torch.int64, device=dev))
        d = self._dev
        K.box_size_hist(padded.contiguous(), counts.to(torch.int32).contiguous(), it, d['count'], d['first'],
                        d['totals'], d['spill'])

    def _host_batch(self, gt, it):
        k = 0
        for gt_bboxes in gt:
            if len(gt_bboxes.shape) < 2:
                self.shapeless2 += 1
            elif gt_bboxes.shape[0] == 0:
                self._host_noimg += 1
            else:
                for gt_bbox in gt_bboxes.cpu():
                    w, h = int(gt_bbox[2] - gt_bbox[0]), int(gt_bbox[3] - gt_bbox[1])
                    self._add(self._host, f'{w},{h}', 1, (it << 32) | k)
                    self._host_total += 1
                    k += 1

    @staticmethod
    def _add(acc, tag, count, key):
        e = acc.get(tag)
        if e is None:
            acc[tag] = [count, key]
        else:
            e[0] += count
            e[1] = min(e[1], key)

    def statistics(self):
        """(data in first-seen order, Total_sample, Noimg) so far: one device-to-host copy of the grid state."""
        acc = {t: list(v) for t, v in self._host.items()}
        total, noimg = self._host_total, self._host_noimg
        d = self._dev
        if d is not None:
            h1, w1 = d['count'].shape
            flat = torch.cat([d['count'].view(-1), d['first'].view(-1), d['totals'], d['spill'].view(-1)]).cpu().numpy()
            nb = h1 * w1
            cnt, first, tot, spill = flat[:nb], flat[nb:2 * nb], flat[2 * nb:2 * nb + 4], flat[2 * nb + 4:]
            if tot[L.HIST_STATUS] & (L.HIST_OVERFLOW | L.HIST_BAD_COUNT):
                raise RuntimeError(f'YuNetSampleSizeStatisticsHook: device statistics incomplete (status '
                                   f'{int(tot[L.HIST_STATUS])}: more than {self.SPILL_CAP} boxes outside the size grid, '
                                   f'or a GT count outside [0, Gmax])')
            total += int(tot[L.HIST_TOTAL])
            noimg += int(tot[L.HIST_NOIMG])
            for i in np.nonzero(cnt)[0]:
                h, w = divmod(int(i), w1)
                self._add(acc, f'{w},{h}', int(cnt[i]), int(first[i]))
            sp = spill.reshape(-1, 2)[:int(tot[L.HIST_SPILLED])]
            if len(sp):
                wh = np.ascontiguousarray(sp[:, 1]).view(np.uint32).reshape(-1, 2).view(np.float32)
                for (key, _), (w, h) in zip(sp.tolist(), wh.tolist()):
                    self._add(acc, f'{int(w)},{int(h)}', 1, int(key))
        data = {t: c for t, (c, _) in sorted(acc.items(), key=lambda kv: kv[1][1])}
        return data, total, noimg

    def dump_json(self):
        data, total, noimg = self.statistics()
        with open(self.out_file, 'w') as f:
            json.dump({'datetime:': str(datetime.now()), 'Batch_size': self.batch_size, 'Total_sample': total,
                       'Noimg': noimg, 'Shapeless2': self.shapeless2, 'data': data}, f)


class CheckInvalidLossHook(Hook):
    """mmdet/core/hook/checkloss_hook.py: every `interval` iterations the loss must be finite.  The logged loss is a
    lazily copied scalar here; it is resolved only on the iterations that are checked."""

    def __init__(self, interval=50):
        self.interval = interval

    def after_train_iter(self, runner):
        if not self.every_n_iters(runner, self.interval):
            return
        out = runner.outputs
        lazy = (out.get('log_vars') or {}).get('loss')
        try:
            value = float(lazy if lazy is not None else out['loss'])
        except RuntimeError:             # a distributed step's log_vars before backward: the local loss
            value = float(out['loss'])
        if not math.isfinite(value):
            runner.logger('loss become infinite or NaN!')
            raise AssertionError('loss become infinite or NaN!')


class YOLOXModeSwitchHook(Hook):
    """mmdet/core/hook/yolox_mode_switch_hook.py: at the start of epoch max_epochs - num_last_epochs (counted from 1) the
    steps named by skip_type_keys are switched off in the data source (DevicePipeline.update_skip_type_keys: they launch
    nothing from then on) and bbox_head.use_l1 is set, as the reference sets it -- YuNet_Head never reads that attribute,
    in the reference or here.  The reference's lines that restart a DataLoader with persistent workers have nothing to
    act on: the pipeline runs in this process, so the switch holds from the next batch."""

    def __init__(self, num_last_epochs=15, skip_type_keys=('Mosaic', 'RandomAffine', 'MixUp')):
        self.num_last_epochs = num_last_epochs
        self.skip_type_keys = skip_type_keys

    def before_train_epoch(self, runner):
        if (runner.epoch + 1) == runner.max_epochs - self.num_last_epochs:
            runner.logger('No mosaic and mixup aug now!')
            runner.data_loader.dataset.update_skip_type_keys(self.skip_type_keys)
            runner.logger('Add additional L1 loss now!')
            _unwrap(runner.model).bbox_head.use_l1 = True


CUSTOM_HOOKS = dict(ExpMomentumEMAHook=ExpMomentumEMAHook, LinearMomentumEMAHook=LinearMomentumEMAHook,
                    YuNetSampleSizeStatisticsHook=YuNetSampleSizeStatisticsHook,
                    CheckInvalidLossHook=CheckInvalidLossHook, YOLOXModeSwitchHook=YOLOXModeSwitchHook)
HOOKS.update(CUSTOM_HOOKS)            # custom_hooks=[dict(type=...)] of a config (runner.register_training_hooks)
