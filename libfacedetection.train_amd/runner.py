"""Minimal training loop standing in for the mmcv runner the reference drives
(mmdet/apis/train.py:117-246; mmcv EpochBasedRunner + OptimizerHook + StepLrUpdaterHook +
CheckpointHook + TextLoggerHook are un-vendored).

Per iteration, exactly the reference's order: lr hook -> model.train_step(batch, optimizer)
-> optimizer.zero_grad() -> loss.backward() -> optimizer.step() -> log buffer.
"""
import math
import os
import time
import warnings

import torch

from . import synthetic
from .engine import det_level
from .optim import build_optimizer
from .parallel import build_ddp, get_dist_info


class LrSchedule:
    """lr_config = dict(policy=..., warmup=..., warmup_iters, warmup_ratio, ...) of mmcv's LrUpdaterHook family
    (mmcv/runner/hooks/lr_updater.py, un-vendored: restated from its published formulas, SURVEY App. C -- the shipped
    configs use policy='step' with by-epoch steps and a linear by-iteration warm-up, configs/yunet_n.py:4-10, and that
    case is the one checked against the shipped checkpoint's optimizer state).

    policy: 'step' (step int | list, gamma, min_lr) | 'fixed' | 'exp' (gamma) | 'poly' (power, min_lr) |
            'inv' (gamma, power) | 'CosineAnnealing' (min_lr | min_lr_ratio);  by_epoch (default True) selects the
    progress variable (epoch / iteration) of the regular schedule;  warmup: None | 'constant' | 'linear' | 'exp',
    always by iteration (mmcv's default warmup_by_epoch=False)."""

    POLICIES = ('step', 'fixed', 'exp', 'poly', 'inv', 'CosineAnnealing')

    def __init__(self, base_lr, step=None, gamma=0.1, warmup=None, warmup_iters=0, warmup_ratio=0.1, policy='step',
                 by_epoch=True, min_lr=None, min_lr_ratio=None, power=1.0, warmup_by_epoch=False, **unknown):
        if policy not in self.POLICIES:
            raise NotImplementedError(f'lr policy {policy!r}: implemented are {self.POLICIES}')
        if warmup not in (None, 'constant', 'linear', 'exp'):
            raise ValueError(f'"{warmup}" is not a supported type for warming up, valid types are "constant", "linear" '
                             f'and "exp"')
        # an option this restatement does not implement must not be swallowed: the schedule would silently differ from
        # mmcv's
        if warmup_by_epoch:
            raise NotImplementedError('lr_config: warmup_by_epoch=True is not implemented (warm-up runs by iteration)')
        if unknown:
            raise NotImplementedError(f'lr_config: unsupported option(s) {sorted(unknown)} for policy {policy!r}')
        if policy == 'step' and isinstance(gamma, (list, tuple)):
            raise NotImplementedError('lr_config: a per-step gamma list is not implemented')
        if policy == 'step' and step is None:
            raise ValueError('lr policy "step" needs step=<int | list>')
        if policy == 'CosineAnnealing' and (min_lr is None) == (min_lr_ratio is None):
            raise ValueError('CosineAnnealing: exactly one of min_lr / min_lr_ratio')
        self.base_lr, self.policy, self.by_epoch = base_lr, policy, by_epoch
        self.step = step if isinstance(step, int) or step is None else list(step)
        self.gamma, self.power, self.min_lr, self.min_lr_ratio = gamma, power, min_lr, min_lr_ratio
        self.warmup, self.warmup_iters, self.warmup_ratio = warmup, warmup_iters, warmup_ratio

    def regular_lr(self, epoch, it, max_epochs=None, max_iters=None):
        progress = epoch if self.by_epoch else it
        max_progress = max_epochs if self.by_epoch else max_iters
        b = self.base_lr
        if self.policy == 'fixed':
            return b
        if self.policy == 'step':
            k = progress // self.step if isinstance(self.step, int) else sum(1 for s in self.step if progress >= s)
            lr = b * self.gamma ** k
            return max(lr, self.min_lr) if self.min_lr is not None else lr
        if self.policy == 'exp':
            return b * self.gamma ** progress
        if self.policy == 'inv':
            return b * (1 + self.gamma * progress) ** (-self.power)
        if max_progress is None:
            raise ValueError(f'lr policy {self.policy!r} needs the run length (max_epochs / max_iters)')
        if self.policy == 'poly':
            m = self.min_lr or 0.0
            return (b - m) * (1 - progress / max_progress) ** self.power + m
        target = b * self.min_lr_ratio if self.min_lr_ratio is not None else self.min_lr
        return target + 0.5 * (b - target) * (math.cos(math.pi * progress / max_progress) + 1)

    def lr_at(self, epoch, it, max_epochs=None, max_iters=None):
        lr = self.regular_lr(epoch, it, max_epochs, max_iters)
        if self.warmup is not None and it < self.warmup_iters:
            if self.warmup == 'constant':
                lr = lr * self.warmup_ratio
            elif self.warmup == 'linear':
                k = (1 - it / self.warmup_iters) * (1 - self.warmup_ratio)
                lr = lr * (1 - k)
            else:
                lr = lr * self.warmup_ratio ** (1 - it / self.warmup_iters)
        return lr


class StepLrWarmup(LrSchedule):
    """The shipped schedule (policy='step', linear warm-up); kept as a name for tools/make_trained_fixture.py."""

    def __init__(self, base_lr, step, gamma=0.1, warmup='linear', warmup_iters=0, warmup_ratio=0.1, policy='step', **kw):
        super().__init__(base_lr, step=step, gamma=gamma, warmup=warmup, warmup_iters=warmup_iters,
                         warmup_ratio=warmup_ratio, policy=policy, **kw)


class SyntheticWiderFace:
    """Endless synthetic WIDER-Face-shaped batches; stands in for
    RetinaFaceDataset + the cv2 pipeline, which need the WIDER images (out of scope)."""

    def __init__(self, img_scale=(640, 640), samples_per_gpu=16, iters_per_epoch=403, rank=0,
                 max_gt=synthetic.MAX_GT, resident=0, **_):
        self.h, self.w = img_scale[1], img_scale[0]
        self.bs, self.iters_per_epoch, self.rank, self.max_gt = \
            samples_per_gpu, iters_per_epoch, rank, max_gt
        # resident = k > 0: k batches are generated once, kept on the device and cycled (what bench.py feeds: the step
        # with inputs already in HBM); 0: a fresh batch is drawn on the host every iteration
        self.resident, self._pool = int(resident), {}

    def batch(self, it, device=None):
        if self.resident > 0 and device is not None:
            k = it % self.resident
            if k not in self._pool:
                b = synthetic.make_batch(self.bs, self.h, self.w, synthetic.batch_seed(self.rank, k), self.max_gt)
                self._pool[k] = synthetic.to_device(b, device)
            return self._pool[k]
        b = synthetic.make_batch(self.bs, self.h, self.w, synthetic.batch_seed(self.rank, it),
                                 self.max_gt)
        return synthetic.to_device(b, device) if device is not None else b


class SyntheticSourceImages:
    """Synthetic DECODED sources (uint8 HWC at WIDER-like sizes, ragged GT) pushed through the reference's train
    pipeline on the GPU (pipelines.DevicePipeline: RandomSquareCrop -> Resize -> RandomFlip -> collate) every iteration
    -- the role of RetinaFaceDataset + the cv2 worker processes, minus image decoding.

    host_fed=False: the decoded sources stay resident in HBM (WIDER-Face train, 12 880 images, is ~30 GB decoded: it
    fits 288 GB many times over), an iteration costs the two pipeline launches.
    host_fed=True : the sources live in PINNED HOST memory and every iteration's batch is uploaded on a copy stream into
    one of two device buffers while the previous step runs (what a host data loader has to pay: the decoded uint8
    source of an image is 1 - 2.4 MB, more than its 320 x 320 fp32 crop).
    host_fed='window': the same pinned sources as a host SourceStore; per batch only the rectangle of each image that
    the crop can read travels (source_store.WindowFeed: plans made two iterations ahead, 2D copies on a copy stream,
    the pixel pass on the window buffer) -- outputs bit-identical to the other modes.  host_fetch (host_fed='window'
    only): None or 'dma' = one hipMemcpy2DAsync per rectangle after a host wait on the plan; 'kernel' = the GPU reads
    the rectangles from the pinned store itself (yunet_fetch_windows), no host wait.
    `timing=True` records events around the upload and the pipeline (`report()`)."""

    def __init__(self, pipeline, samples_per_gpu=16, iters_per_epoch=403, rank=0, pool=64,
                 src_hw=((768, 1024), (1024, 683), (500, 375), (683, 1024)), max_gt=synthetic.MAX_GT,
                 seed=0, host_fed=False, timing=False, host_fetch=None, skip_type_keys=None, **_):
        from .pipelines import DevicePipeline
        self.pipe = DevicePipeline(pipeline, seed=seed + 7919 * rank, gmax=64 if max_gt <= 64 else 128)
        self.pipe.check_plan_cache()
        if skip_type_keys is not None:
            self.pipe.update_skip_type_keys(skip_type_keys)
        self.bs, self.iters_per_epoch, self.rank = samples_per_gpu, iters_per_epoch, rank
        self.pool, self.src_hw, self.max_gt, self.seed = pool, src_hw, max_gt, seed
        if host_fed not in (False, True, 'window'):
            raise ValueError(f"host_fed must be False, True or 'window', got {host_fed!r}")
        self.host_fed, self.timing = (host_fed if host_fed == 'window' else bool(host_fed)), bool(timing)
        if host_fetch not in (None, 'dma', 'kernel'):
            raise ValueError(f"host_fetch must be 'dma' or 'kernel' (or unset), got {host_fetch!r}")
        if host_fetch is not None and self.host_fed != 'window':
            raise ValueError(f"host_fetch applies to host_fed='window' only, not host_fed={host_fed!r}")
        self.host_fetch = host_fetch
        if self.host_fed:
            self.pipe.require_resident(f'host-fed sources (host_fed={host_fed!r})')
        self._src = None
        self._ev = []

    @property
    def dataset(self):
        """What a hook reaches as runner.data_loader.dataset: the object that takes update_skip_type_keys."""
        return self

    def update_skip_type_keys(self, skip_type_keys):
        """MultiImageMixDataset.update_skip_type_keys: forwarded to the device pipeline."""
        self.pipe.update_skip_type_keys(skip_type_keys)

    def _pool_sources(self):
        import numpy as np
        rng = np.random.default_rng(self.seed + 1000 * self.rank)
        gen = torch.Generator().manual_seed(self.seed + 1000 * self.rank)
        imgs, boxes, kps = [], [], []
        for i in range(self.pool):
            h, w = self.src_hw[i % len(self.src_hw)]
            imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            b, _, k = synthetic.make_gt(1, h, w, gen, self.max_gt)
            boxes.append(b[0])
            kps.append(k[0])
        return imgs, boxes, kps, [i % self.pool for i in range(self.bs)]

    def _build(self, device):
        from .pipelines import SourceBatch
        imgs, boxes, kps, idx = self._pool_sources()
        if self.pipe.mosaic is not None or self.pipe.mixup is not None:     # partners come from the pool, not the batch
            from .source_store import SourceStore
            store = SourceStore([im.shape[:2] for im in imgs], placement='device', device=device)
            for i, im in enumerate(imgs):
                store.put(i, im, boxes[i], kps[i])
            return store.batch(idx)
        return SourceBatch.from_lists([imgs[i] for i in idx], [boxes[i] for i in idx],
                                      [kps[i] for i in idx], 'cpu' if self.host_fed else device)

    def _build_host_fed(self, device):
        """Pinned host copy of the batch's sources + two device buffers + the copy stream."""
        from .pipelines import SourceBatch
        host = self._build(device)
        self._host_src = host.src.pin_memory()
        meta = [t.to(device) for t in (host.src_off, host.src_hw, host.boxes, host.kps, host.gt_off)]
        self._bufs = [torch.empty_like(self._host_src, device=device) for _ in range(2)]
        self._views = [SourceBatch(b, *meta) for b in self._bufs]
        self._copy = torch.cuda.Stream(device=device)
        self._uploaded = [None, None]          # event: buffer b holds iteration's sources
        self._consumed = [None, None]          # event: the pipeline that read buffer b has run
        self._pending = {}

    def _build_window(self, device):
        """The pool as a pinned host SourceStore (batch = store indices, with repeats when bs > pool) + a WindowFeed whose
        two window buffers hold a whole batch (a window never exceeds its image)."""
        from .source_store import SourceStore, WindowFeed
        imgs, boxes, kps, idx = self._pool_sources()
        store = SourceStore([im.shape[:2] for im in imgs], placement='host', device=device)
        for i, im in enumerate(imgs):
            store.put(i, im, boxes[i], kps[i])
        self._idx = idx
        self._batch_bytes = int(store.image_bytes[idx].sum())
        self._feed = WindowFeed(self.pipe, store, self._batch_bytes, timing=self.timing, fetch=self.host_fetch or 'dma')

    def _window_batch(self, it, device):
        if self._src is None:
            self._src = True
            self._build_window(device)
        f = self._feed
        for k in (it, it + 1):              # start-up / a caller that jumps: plans before the first upload waits
            if not f.planned(k) and not f.uploaded(k):
                f.plan(k, self._idx)
        if not f.uploaded(it):
            f.upload(it)
        cur = torch.cuda.current_stream()
        p0 = self._mark(cur)
        out, h2d = f.run(it)
        if self.timing:
            done = self._mark(cur)
            self._ev.append((h2d, (p0, done)))
        if not f.uploaded(it + 1):
            f.upload(it + 1)                # the next batch's windows travel while this step runs
        if not f.planned(it + 2):
            f.plan(it + 2, self._idx)       # its plan is done long before batch(it + 1) waits for it
        return out

    def _upload(self, it):
        b = it % 2
        with torch.cuda.stream(self._copy):
            if self._consumed[b] is not None:
                self._copy.wait_event(self._consumed[b])
            e0 = torch.cuda.Event(enable_timing=self.timing)
            e0.record(self._copy)
            self._bufs[b].copy_(self._host_src, non_blocking=True)
            e1 = torch.cuda.Event(enable_timing=self.timing)
            e1.record(self._copy)
        self._uploaded[b] = e1
        self._pending[it] = (e0, e1)

    def batch(self, it, device=None):
        if device is None:
            raise RuntimeError('SyntheticSourceImages augments on the GPU: a device is required')
        if self.host_fed == 'window':
            return self._window_batch(it, device)
        cur = torch.cuda.current_stream()
        if not self.host_fed:
            if self._src is None:
                self._src = self._build(device)
            # (the two pipeline launches on a side stream under the previous step were measured: 4.96 -> 4.98 ms per
            #  iteration, nothing -- the step's persistent kernels fill the GPU, the pipeline's 0.31 ms is work, not latency)
            p0 = self._mark(cur)
            out = self.pipe(self._src, it)
            if self.timing:
                self._ev.append((None, (p0, self._mark(cur))))
            return out
        if self._src is None:
            self._src = True
            self._build_host_fed(device)
        if it not in self._pending:
            self._upload(it)
        b = it % 2
        h2d = self._pending.pop(it)
        cur.wait_event(self._uploaded[b])
        p0 = self._mark(cur)
        out = self.pipe(self._views[b], it)
        done = torch.cuda.Event(enable_timing=self.timing)
        done.record(cur)
        self._consumed[b] = done
        if self.timing:
            self._ev.append((h2d, (p0, done)))
        self._upload(it + 1)                   # the next batch travels while this step runs
        return out

    def _mark(self, stream):
        if not self.timing:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        return e

    def report(self, skip=5):
        """Mean milliseconds per batch of the upload and of the two pipeline launches (timing=True; synchronises)."""
        if not self.timing:
            return {}
        torch.cuda.synchronize()
        ev = self._ev[skip:]
        out = {'batches_timed': len(ev)}
        h = [hd[0].elapsed_time(hd[1]) for (hd, _) in ev if hd is not None]
        p = [a.elapsed_time(b) for (_, (a, b)) in ev if a is not None]
        if h:
            out['h2d_ms'] = sum(h) / len(h)
            if self.host_fed == 'window':         # mean bytes actually copied per batch, next to the whole sources
                nb = [float(hd[2]) for (hd, _) in ev]       # fetch='kernel': a device scalar (synchronised above)
                out['h2d_bytes'] = sum(nb) / len(nb)
                out['src_bytes'] = self._batch_bytes
            else:
                out['h2d_bytes'] = int(self._host_src.numel())
            out['h2d_GBs'] = out['h2d_bytes'] / (out['h2d_ms'] * 1e-3) / 1e9
        if p:
            out['pipeline_ms'] = sum(p) / len(p)
        self._ev = []
        return out


def save_checkpoint(model, optimizer, path, meta):
    """Reference format: torch.save({'meta', 'state_dict', 'optimizer'})."""
    target = model.module if hasattr(model, 'module') else model
    sd = {k: v.detach().cpu() for k, v in target.state_dict().items()}
    torch.save(dict(meta=meta, state_dict=sd, optimizer=optimizer.state_dict()), path)


def load_model_state(target, sd, strict=True):
    """target.load_state_dict(sd, strict) that skips the EMA hooks' `ema_*` entries only one side has, with a warning
    (yunet.skip_ema_entries; YuNet registers it on itself, any other module gets it for this call).  Every other key
    stays strict."""
    from .yunet import skip_ema_entries
    handle = target.register_load_state_dict_post_hook(skip_ema_entries)
    try:
        return target.load_state_dict(sd, strict=strict)
    finally:
        handle.remove()


def load_checkpoint(model, path, optimizer=None, strict=True):
    ck = torch.load(path, map_location='cpu', weights_only=False)
    target = model.module if hasattr(model, 'module') else model
    load_model_state(target, ck['state_dict'] if 'state_dict' in ck else ck, strict=strict)
    if optimizer is not None:
        if isinstance(ck.get('optimizer'), dict):
            optimizer.load_state_dict(ck['optimizer'])
        else:
            import warnings
            warnings.warn(f'{path}: no optimizer state in the checkpoint, momentum restarts from zero')
    return ck.get('meta', {})


# ================================================================================ hooks / runner
PRIORITY = dict(HIGHEST=0, VERY_HIGH=10, HIGH=30, ABOVE_NORMAL=40, NORMAL=50, BELOW_NORMAL=60, LOW=70,
                VERY_LOW=90, LOWEST=100)


class Hook:
    """mmcv.runner.Hook: the stage methods an EpochBasedRunner calls."""
    stages = ('before_run', 'before_train_epoch', 'before_train_iter', 'after_train_iter',
              'after_train_epoch', 'before_val_epoch', 'before_val_iter', 'after_val_iter', 'after_val_epoch', 'after_run')

    def before_run(self, runner): pass                    # noqa: E704
    def after_run(self, runner): pass                     # noqa: E704
    def before_epoch(self, runner): pass                  # noqa: E704
    def after_epoch(self, runner): pass                   # noqa: E704
    def before_iter(self, runner): pass                   # noqa: E704
    def after_iter(self, runner): pass                    # noqa: E704

    def before_train_epoch(self, runner):
        self.before_epoch(runner)

    def after_train_epoch(self, runner):
        self.after_epoch(runner)

    def before_train_iter(self, runner):
        self.before_iter(runner)

    def after_train_iter(self, runner):
        self.after_iter(runner)

    # the validation epochs of a workflow (EpochBasedRunner.val), mapped onto the generic stages as mmcv's base class does
    def before_val_epoch(self, runner):
        self.before_epoch(runner)

    def after_val_epoch(self, runner):
        self.after_epoch(runner)

    def before_val_iter(self, runner):
        self.before_iter(runner)

    def after_val_iter(self, runner):
        self.after_iter(runner)

    def every_n_iters(self, runner, n):
        return (runner.iter + 1) % n == 0 if n > 0 else False

    def every_n_epochs(self, runner, n):
        return (runner.epoch + 1) % n == 0 if n > 0 else False


class StepLrUpdaterHook(Hook):
    """lr_config = dict(policy='step', ...) (configs/yunet_n.py:4-10): sets the lr of every param group
    before each iteration (by-epoch steps, by-iteration linear warm-up).  The same hook carries the other policies of
    LrSchedule (mmcv names them {Fixed,Exp,Poly,Inv,CosineAnnealing}LrUpdaterHook)."""

    def __init__(self, base_lr=None, **cfg):
        self.cfg, self.base_lr, self.sched = cfg, base_lr, None
        self._scheds = {}

    def before_run(self, runner):
        base = self.base_lr if self.base_lr is not None else runner.optimizer.param_groups[0].get(
            'initial_lr', runner.optimizer.param_groups[0]['lr'])
        self.sched = LrSchedule(base, **self.cfg)
        self._scheds = {base: self.sched}

    def _sched_of(self, group):
        """mmcv: every group follows the schedule from its OWN initial_lr (a min_lr or a warm-up is no plain multiple of
        the base schedule); an explicit base_lr of the hook overrides that for all groups."""
        base = self.base_lr if self.base_lr is not None else group.get('initial_lr', group['lr'])
        if base not in self._scheds:
            self._scheds[base] = LrSchedule(base, **self.cfg)
        return self._scheds[base]

    def before_train_iter(self, runner):
        args = (runner.epoch, runner.iter, getattr(runner, 'max_epochs', None), getattr(runner, 'max_iters', None))
        for g in runner.optimizer.param_groups:
            g['lr'] = self._sched_of(g).lr_at(*args)


class OptimizerHook(Hook):
    """optimizer_config = dict(grad_clip=None | dict(max_norm=, norm_type=2)): zero_grad -> backward -> [clip] -> step
    (mmcv OptimizerHook).  With a fused optimizer (optim.py) clipping is the norm kernel in front of the update kernel,
    two launches and no host sync; `grad_norm` joins the iteration's log_vars as a device scalar that a logger reads when
    it fires.  Any other optimizer goes through torch.nn.utils.clip_grad_norm_."""

    def __init__(self, grad_clip=None, **_):
        self.grad_clip = grad_clip

    def before_run(self, runner):
        if hasattr(runner.optimizer, 'set_grad_clip'):
            runner.optimizer.set_grad_clip(self.grad_clip)

    def _fused_clip(self, runner):
        return self.grad_clip is not None and getattr(runner.optimizer, 'grad_clip', None) is not None

    def _log_grad_norm(self, runner):
        log_vars = runner.outputs.get('log_vars')
        if log_vars is not None:
            log_vars['grad_norm'] = runner.optimizer.grad_norm

    def after_train_iter(self, runner):
        runner.optimizer.zero_grad()
        runner.outputs['loss'].backward()
        if self.grad_clip is not None and not self._fused_clip(runner):
            params = [p for p in runner.model.parameters() if p.requires_grad and p.grad is not None]
            norm = torch.nn.utils.clip_grad_norm_(params, **self.grad_clip)
            if runner.outputs.get('log_vars') is not None:
                runner.outputs['log_vars']['grad_norm'] = norm
        runner.optimizer.step()
        if self._fused_clip(runner):
            self._log_grad_norm(runner)


class Fp16OptimizerHook(OptimizerHook):
    """cfg.fp16 = dict(loss_scale=512.) (mmdet/apis/train.py:181-185 -> mmcv Fp16OptimizerHook).
    The reference's mixed precision is fp16 storage with loss scaling.  On MI355X the reduced
    precision mode of this path is bf16 activation storage + bf16 matrix instructions in forward with
    fp32 gradients and master weights (BASELINE.json configs[2]); bf16 keeps fp32's exponent range,
    so the loss scale is applied and removed exactly (a power of two) and only the overflow check of
    `loss_scale='dynamic'` ever changes anything: a step with non-finite gradients is skipped and the
    scale halves, 2000 clean steps double it (mmcv LossScaler defaults)."""

    def __init__(self, grad_clip=None, loss_scale=512., distributed=True, **_):
        super().__init__(grad_clip)
        self.dynamic = loss_scale == 'dynamic' or isinstance(loss_scale, dict)
        init = 2. ** 16 if loss_scale == 'dynamic' else (loss_scale.get('init_scale', 2. ** 16)
                                                          if isinstance(loss_scale, dict) else float(loss_scale))
        self.scale, self.growth_interval, self._good = float(init), 2000, 0

    def before_run(self, runner):
        super().before_run(runner)
        target = runner.model.module if hasattr(runner.model, 'module') else runner.model
        target.set_precision('bf16')

    def after_train_iter(self, runner):
        runner.optimizer.zero_grad()
        (runner.outputs['loss'] * self.scale).backward()
        self._unscale_and_step(runner)

    def _unscale_and_step(self, runner):
        """What follows the scaled backward: finite check, scale removal, [clip], step, dynamic-scale bookkeeping.
        Returns whether the update was applied."""
        opt = runner.optimizer
        target = runner.model.module if hasattr(runner.model, 'module') else runner.model
        grad = target.engine.params.grad
        # mmcv's GradScaler-based hook skips a step with non-finite gradients for static scales too
        # (only a dynamic scale is then halved)
        if not bool(torch.isfinite(grad).all()):
            if self.dynamic:
                self.scale = max(self.scale / 2.0, 1.0)
                self._good = 0
            return False                                       # skip the step, like LossScaler
        fused_clip = self._fused_clip(runner)
        if hasattr(opt, 'grad_scale') and (self.grad_clip is None or fused_clip):
            # fused optimizers: folded into the update kernel, and into the norm kernel, which therefore measures the
            # UNSCALED gradient
            opt.grad_scale = 1.0 / self.scale
        else:
            # clipping measures the norm of the UNSCALED gradient (max_norm must not shrink by the loss
            # scale): remove the scale in place first
            grad.mul_(1.0 / self.scale)
            if hasattr(opt, 'grad_scale'):
                opt.grad_scale = 1.0
        if self.grad_clip is not None and not fused_clip:
            params = [p for p in runner.model.parameters() if p.requires_grad and p.grad is not None]
            torch.nn.utils.clip_grad_norm_(params, **self.grad_clip)
        opt.step()
        if fused_clip:
            self._log_grad_norm(runner)
        if self.dynamic:
            self._good += 1
            if self._good % self.growth_interval == 0:
                self.scale *= 2.0
        return True


def _unwrap(model):
    return model.module if hasattr(model, 'module') else model


class GradientCumulativeOptimizerHook(OptimizerHook):
    """optimizer_config = dict(type='GradientCumulativeOptimizerHook', cumulative_iters=k [, grad_clip=...]) (mmcv >= 1.3.9):
    k iterations of (loss / loss_factor).backward() onto the same gradient, then [clip] -> step -> zero_grad.  There is no
    zero_grad in front of each backward: before_run switches gradient accumulation on in the model
    (YuNet.set_grad_accumulation), so the fused backward adds to .grad; the backward right after a zero_grad overwrites and
    costs nothing extra.

    Schedule, fixed at the first after_train_iter: start_iter = runner.iter, residual = max_iters - start_iter,
    divisible_iters = residual // k * k, remainder_iters = residual - divisible_iters.  loss_factor is k while
    runner.iter < start_iter + divisible_iters and remainder_iters afterwards; an update happens at every_n_iters(runner, k)
    and at the last iteration of the run.
    Deviation from mmcv, on purpose: mmcv compares the absolute runner.iter with divisible_iters, which counts from the
    starting iteration -- after a resume its last `start_iter` full windows would already be divided by remainder_iters
    (by zero when the residual is a multiple of k).  Here the comparison is relative to start_iter; a run that starts at
    iteration 0 is mmcv's exactly.  The update boundaries stay on the absolute iteration count, as in mmcv: a resumed
    iteration that is no multiple of k makes the first window shorter (its gradient is still divided by k), which is what
    the warning says.

    With a fused optimizer clipping is the norm kernel and the update kernel on the accumulated gradient; `grad_norm` joins
    log_vars on the iterations that update.  BatchNorm statistics are those of each micro-batch: k micro-batches are not
    one large batch unless every BatchNorm layer is frozen (the second warning).  At world size > 1 every micro-step keeps
    its gradient all-reduce, like mmcv's hook under MMDistributedDataParallel."""

    def __init__(self, cumulative_iters=1, grad_clip=None):
        if not isinstance(cumulative_iters, int) or isinstance(cumulative_iters, bool) or cumulative_iters <= 0:
            raise TypeError(f'cumulative_iters only accepts positive int, but got {type(cumulative_iters)} instead.')
        super().__init__(grad_clip)
        self.cumulative_iters = cumulative_iters
        self.start_iter = self.divisible_iters = self.remainder_iters = 0
        self.initialized = False

    def before_run(self, runner):
        super().before_run(runner)
        target = _unwrap(runner.model)
        if hasattr(target, 'set_grad_accumulation'):
            target.set_grad_accumulation(True)

    @staticmethod
    def has_batch_norm(module):
        """A BatchNorm layer that normalises with batch statistics (a layer in eval() is the same under micro-batching)."""
        return any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training for m in module.modules())

    def _warn(self, runner, msg):
        warn = getattr(runner.logger, 'warning', None)
        (warn if warn is not None else runner.logger)(msg)

    def _init(self, runner):
        k = self.cumulative_iters
        if runner.iter % k != 0:
            self._warn(runner, 'Resume iter number is not divisible by cumulative_iters in GradientCumulativeOptimizerHook, '
                               'which means the gradient of some iters is lost and the result may be influenced slightly.')
        if k > 1 and self.has_batch_norm(runner.model):
            self._warn(runner, 'GradientCumulativeOptimizerHook may slightly decrease performance if the model has '
                               'BatchNorm layers.')
        self.start_iter = runner.iter
        residual = runner.max_iters - runner.iter
        self.divisible_iters = residual // k * k
        self.remainder_iters = residual - self.divisible_iters
        self.initialized = True

    def loss_factor(self, runner):
        if not self.initialized:
            self._init(runner)
        return self.cumulative_iters if runner.iter < self.start_iter + self.divisible_iters else self.remainder_iters

    def is_boundary(self, runner):
        return self.every_n_iters(runner, self.cumulative_iters) or runner.iter + 1 == runner.max_iters

    def after_train_iter(self, runner):
        (runner.outputs['loss'] / self.loss_factor(runner)).backward()
        if not self.is_boundary(runner):
            return
        if self.grad_clip is not None and not self._fused_clip(runner):
            params = [p for p in runner.model.parameters() if p.requires_grad and p.grad is not None]
            norm = torch.nn.utils.clip_grad_norm_(params, **self.grad_clip)
            if runner.outputs.get('log_vars') is not None:
                runner.outputs['log_vars']['grad_norm'] = norm
        runner.optimizer.step()
        if self._fused_clip(runner):
            self._log_grad_norm(runner)
        runner.optimizer.zero_grad()


class GradientCumulativeFp16OptimizerHook(GradientCumulativeOptimizerHook, Fp16OptimizerHook):
    """GradientCumulativeOptimizerHook under cfg.fp16 (bf16 activation storage with loss scaling, Fp16OptimizerHook):
    (loss * scale / loss_factor).backward() every iteration; the finite check, the scale's removal, clipping and the update
    run on the accumulated gradient at the boundary only.  A non-finite total skips the update and halves a dynamic scale;
    the gradient is zeroed either way, so the next window starts fresh.  The scale changes at boundaries only: every
    micro-batch of a window carries the same one."""

    def __init__(self, cumulative_iters=1, loss_scale=512., grad_clip=None, distributed=True):
        GradientCumulativeOptimizerHook.__init__(self, cumulative_iters, grad_clip)
        Fp16OptimizerHook.__init__(self, grad_clip, loss_scale, distributed)

    def after_train_iter(self, runner):          # (before_run: both bases' -- accumulation on, grad_clip, bf16 storage)
        (runner.outputs['loss'] * self.scale / self.loss_factor(runner)).backward()
        if not self.is_boundary(runner):
            return
        self._unscale_and_step(runner)
        runner.optimizer.zero_grad()


class CheckpointHook(Hook):
    """checkpoint_config = dict(interval=N) : epoch_{k}.pth + a `latest.pth` copy (rank 0)."""

    def __init__(self, interval=1, by_epoch=True, max_keep_ckpts=-1, **_):
        self.interval, self.by_epoch, self.max_keep = interval, by_epoch, max_keep_ckpts

    def after_train_epoch(self, runner):
        if runner.rank != 0 or not runner.work_dir or not self.every_n_epochs(runner, self.interval):
            return
        runner.save_checkpoint(runner.work_dir, f'epoch_{runner.epoch + 1}.pth')
        if self.max_keep > 0:
            old = runner.epoch + 1 - self.max_keep * self.interval
            path = os.path.join(runner.work_dir, f'epoch_{old}.pth')
            if old > 0 and os.path.exists(path):
                os.remove(path)


class EvalHook(Hook):
    """mmdet/core/evaluation/eval_hooks.py:24-66 on this path: every `interval` epochs (by_epoch) or iterations the
    detector runs in eval mode over the validation set (the device test pipeline + get_bboxes), rank 0 calls
    dataset.evaluate(results, metric=...) and files the numbers in the log (runner.log_buffer entries tagged
    mode='val').  The shipped configs set interval=1001 (> max_epochs): the hook is registered, as in the reference,
    and never fires there.  Distributed (DistEvalHook): the images are sharded over the ranks and the results gathered
    on rank 0 (evaluation.multi_gpu_test), as the reference does -- no rank idles behind a barrier.
    `evaluation = dict(..., score='device')` scores the gathered detections on rank 0's GPU instead of in numpy;
    with `rank='device'` beside it the GPU also ranks them and builds the precision curve (evaluation.curve_device)."""

    def __init__(self, dataset, interval=1, by_epoch=True, metric='mAP', start=None, scale=(640, 640),
                 max_images=None, save_best=None, distributed=False, samples_per_gpu=1, pipeline=None, cache=None,
                 score=None, group_by=None, max_batch_pixels='default', rank=None, **eval_kwargs):
        self.dataset, self.interval, self.by_epoch, self.metric = dataset, int(interval), by_epoch, metric
        self.start, self.scale, self.max_images, self.distributed = start, scale, max_images, distributed
        # the batched device test pipeline (evaluation.single_gpu_test): data.val_dataloader.samples_per_gpu, the
        # data.val.pipeline list (parsed once, here, so that an unsupported form raises before training starts) and
        # data.val.cache; the defaults keep the per-image path
        self.samples_per_gpu, self.cache = int(samples_per_gpu), cache
        # data.val_dataloader.group_by ('canvas': batches of one padded shape, grouped_eval.group_batches) and
        # max_batch_pixels, checked here for the same reason
        from .grouped_eval import batch_pixel_cap, check_group_by
        self.group_by = check_group_by(group_by)
        batch_pixel_cap(self.samples_per_gpu, max_batch_pixels)
        self.max_batch_pixels = max_batch_pixels
        if pipeline is not None:
            from .test_pipeline import DeviceTestPipeline
            pipeline = DeviceTestPipeline(pipeline, scale=scale)
        self.pipeline = pipeline
        # where dataset.evaluate scores the detections: 'device' = the runner's GPU (csrc/score.hip), None / 'host' = numpy
        if score not in (None, 'host', 'device'):
            raise ValueError(f"EvalHook: score={score!r}; 'host' or 'device'")
        self.score = score
        from .evaluation import check_rank
        self.rank = check_rank(rank, score == 'device')
        self.eval_kwargs = {k: v for k, v in eval_kwargs.items() if k in ('iou_thr',)}
        dropped = sorted(k for k in eval_kwargs if k not in self.eval_kwargs)
        if save_best is not None:
            dropped.append('save_best')
        if dropped:      # (mmcv's EvalHook options this path does not implement: say so instead of dropping them silently)
            warnings.warn(f'EvalHook: evaluation options {dropped} are not supported on this path and are ignored')
        self.best, self.results = None, []

    def _should(self, runner, count):
        if self.start is not None and count < self.start:
            return False
        return count > 0 and count % self.interval == 0

    def after_train_epoch(self, runner):
        if self.by_epoch and self._should(runner, runner.epoch + 1):
            self._evaluate(runner)

    def after_train_iter(self, runner):
        if not self.by_epoch and self._should(runner, runner.iter + 1):
            self._evaluate(runner)

    def _evaluate(self, runner):
        from .evaluation import multi_gpu_test, single_gpu_test
        target = runner.model.module if hasattr(runner.model, 'module') else runner.model
        dev = torch.device(runner.device) if not isinstance(runner.device, torch.device) else runner.device
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        sharded = self.distributed and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        how = dict(samples_per_gpu=self.samples_per_gpu, pipeline=self.pipeline, cache=self.cache, log=runner.logger)
        if self.group_by is not None:
            how.update(group_by=self.group_by, max_batch_pixels=self.max_batch_pixels)
        if sharded:
            # BatchNorm running statistics are per rank (no SyncBN, broadcast_buffers=False): the reference's
            # DistEvalHook broadcasts rank 0's running_var / running_mean before multi_gpu_test
            # (mmdet/core/evaluation/eval_hooks.py:101-107) so that every shard is evaluated by the SAME model --
            # the one rank 0 checkpoints.  Here the buffers of all layers are two flat tensors.
            broadcast_bn_buffers(target)
            dets = multi_gpu_test(target, self.dataset, dev, self.scale, self.max_images, **how)      # None off rank 0
        else:
            dets = single_gpu_test(target, self.dataset, dev, self.scale, self.max_images, **how) if runner.rank == 0 else None
        if dets is not None:
            where = dict(device=dev) if self.score == 'device' else {}
            if self.rank is not None:
                where['rank'] = self.rank
            res = self.dataset.evaluate(dets, metric=self.metric, **where, **self.eval_kwargs)
            done = runner.iter if self.by_epoch else runner.iter + 1          # iterations completed so far
            entry = dict(mode='val', epoch=runner.epoch + 1, iter=done, **{k: float(v) for k, v in res.items()})
            runner.log_buffer.append(entry)
            self.results.append(entry)
            runner.logger('Epoch(val) [%d][%d]\t%s' % (runner.epoch + 1, len(dets),
                                                       ', '.join(f'{k}: {float(v):.4f}' for k, v in res.items())))
            if self.best is None or res.get('mAP', 0.0) > self.best:
                self.best = res.get('mAP', 0.0)


def broadcast_bn_buffers(model, src=0):
    """dist.broadcast of every BatchNorm running_var / running_mean from rank `src` (DistEvalHook._do_evaluate,
    mmdet/core/evaluation/eval_hooks.py:101-107).  Returns the number of tensors sent (0 without a process group)."""
    if not (torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1):
        return 0
    eng = getattr(model, 'engine', None)
    if eng is not None:          # the fused path: all layers' buffers live in two flat device tensors
        bufs = [eng.params.running_var, eng.params.running_mean]
    else:                        # a model that has not been bound to a device yet: its module buffers
        bufs = [b for n, b in model.named_buffers() if n.endswith('running_var') or n.endswith('running_mean')]
    gloo = torch.distributed.get_backend() != 'nccl'
    for b in bufs:
        if gloo and b.is_cuda:   # CPU process group (tests, ranks sharing one GPU): through the host
            h = b.detach().cpu()
            torch.distributed.broadcast(h, src)
            b.copy_(h)
        else:
            torch.distributed.broadcast(b, src)
    return len(bufs)


class LoggerHook(Hook):
    def __init__(self, interval=50, by_epoch=True, **_):
        self.interval, self.by_epoch = interval, by_epoch
        self._t0 = None

    def before_run(self, runner):
        self._t0 = time.time()

    def after_train_iter(self, runner):
        if not self.every_n_iters(runner, self.interval):
            return
        # log_vars are lazily copied device scalars backed by a 256-row staging ring: freeze them
        # into python floats when they are logged, never keep the lazy objects
        lv = {k: float(v) for k, v in runner.outputs['log_vars'].items()}
        dt = (time.time() - self._t0) / self.interval
        self._t0 = time.time()
        rec = dict(lv, iter=runner.iter + 1, epoch=runner.epoch + 1, lr=runner.current_lr()[0], time=dt)
        if not runner.log_buffer or runner.log_buffer[-1].get('mode') == 'val' or runner.log_buffer[-1]['iter'] != rec['iter']:
            runner.log_buffer.append(rec)            # once per iteration, however many logger hooks
        if runner.rank == 0:
            self.log(runner, rec)

    def after_val_epoch(self, runner):
        """The epoch mean of a validation epoch (EpochBasedRunner.val): one entry in runner.log_buffer, however many
        logger hooks, with the conventions of the EvalHook entry -- epoch = training epochs completed, iter = iterations
        completed."""
        mean = runner.val_epoch_mean()
        if mean is None:
            return
        rec = dict(mode='val', epoch=runner.epoch, iter=runner.iter, **mean)
        if not runner._val_logged:
            runner._val_logged = True
            runner.log_buffer.append(rec)
        if runner.rank == 0:
            self.log_val(runner, rec)

    def log(self, runner, rec):
        raise NotImplementedError

    def log_val(self, runner, rec):
        pass


class TextLoggerHook(LoggerHook):
    def log_val(self, runner, rec):
        keys = [k for k in rec if k not in ('mode', 'iter', 'epoch')]
        runner.logger('Epoch(val) [%d][%d]\t%s' % (rec['epoch'], runner.val_iters, ', '.join(f'{k}: {rec[k]:.4f}' for k in keys)))

    def log(self, runner, rec):
        keys = [k for k in rec if k not in ('iter', 'epoch', 'lr', 'time')]
        runner.logger(f"Epoch [{rec['epoch']}][{rec['iter']}] lr: {rec['lr']:.3e}, time: {rec['time']:.4f}, " +
                      ', '.join(f'{k}: {rec[k]}' if isinstance(rec[k], tuple) else f'{k}: {rec[k]:.4f}' for k in keys))


class YuNetTextLoggerHook(TextLoggerHook):
    """mmdet/core/hook/yunet_text_logger_hook.py: TextLoggerHook plus `image_scale`, the (h, w) of the current batch's
    first image (img_metas[0]['img_shape'][:2], lines 43-44) -- what changes from line to line under
    Resize(multiscale_mode='square_range').  The key goes into this hook's own line, not into runner.log_buffer."""

    def log(self, runner, rec):
        shape = runner.data_batch['img_metas'][0]['img_shape'][:2]
        super().log(runner, dict(rec, image_scale=tuple(int(v) for v in shape)))


class TensorboardLoggerHook(LoggerHook):
    """configs/yunet_n.py:14-17.  Writes TensorBoard event files directly (tfevents record framing +
    Event / Summary protobuf wire format, masked CRC-32C) -- no tensorboard package needed."""

    def __init__(self, log_dir=None, interval=50, **kw):
        super().__init__(interval, **kw)
        self.log_dir, self.writer = log_dir, None

    def before_run(self, runner):
        super().before_run(runner)
        if runner.rank == 0:
            from .tb_events import EventWriter
            d = self.log_dir or os.path.join(runner.work_dir or '.', 'tf_logs')
            self.writer = EventWriter(d)

    def log(self, runner, rec):
        if self.writer is None:
            return
        for k, v in rec.items():
            if k not in ('iter', 'epoch'):
                self.writer.add_scalar(('train/' + k) if k != 'lr' else 'learning_rate', v, rec['iter'])
        self.writer.flush()

    def log_val(self, runner, rec):
        if self.writer is None:
            return
        for k, v in rec.items():
            if k not in ('mode', 'iter', 'epoch'):
                self.writer.add_scalar('val/' + k, v, rec['iter'])
        self.writer.flush()

    def after_run(self, runner):
        if self.writer is not None:
            self.writer.close()


HOOKS = dict(TextLoggerHook=TextLoggerHook, YuNetTextLoggerHook=YuNetTextLoggerHook,
             TensorboardLoggerHook=TensorboardLoggerHook, CheckpointHook=CheckpointHook, OptimizerHook=OptimizerHook,
             Fp16OptimizerHook=Fp16OptimizerHook, GradientCumulativeOptimizerHook=GradientCumulativeOptimizerHook,
             GradientCumulativeFp16OptimizerHook=GradientCumulativeFp16OptimizerHook)


class EpochBasedRunner:
    """The slice of mmcv.runner.EpochBasedRunner the reference's train_detector drives
    (mmdet/apis/train.py:169-246): register_training_hooks / register_hook / resume /
    load_checkpoint / run, and per iteration  before_train_iter hooks -> model.train_step ->
    after_train_iter hooks (OptimizerHook: zero_grad, backward, step; GradientCumulativeOptimizerHook: backward, and
    step + zero_grad every k iterations)."""

    def __init__(self, model, optimizer=None, work_dir=None, logger=print, meta=None, max_epochs=None,
                 max_iters=None):
        self.model, self.optimizer, self.work_dir, self.logger = model, optimizer, work_dir, logger
        self.meta = dict(meta or {})
        self.rank, self.world_size = get_dist_info()
        self._max_epochs, self._max_iters = max_epochs, max_iters
        self.epoch, self.iter, self.inner_iter = 0, 0, 0
        self.hooks, self.outputs, self.log_buffer = [], None, []
        self.data_source, self.device, self.data_batch = None, 'cuda', None
        self.mode = 'train'                     # 'train' | 'val': the workflow entry that is running
        self.val_sums = self.val_keys = self._val_mean = None
        self.val_iters, self._val_logged = 0, False

    @property
    def max_epochs(self):
        return self._max_epochs

    @property
    def max_iters(self):
        """mmcv EpochBasedRunner: max_epochs * len(data_loader) once the data source is known."""
        if self._max_iters is not None:
            return self._max_iters
        per = getattr(self.data_source, 'iters_per_epoch', None)
        return self._max_epochs * per if (self._max_epochs is not None and per) else None

    def current_lr(self):
        return [g['lr'] for g in self.optimizer.param_groups]

    def register_hook(self, hook, priority='NORMAL'):
        hook.priority = PRIORITY[priority] if isinstance(priority, str) else int(priority)
        pos = len(self.hooks)
        while pos > 0 and self.hooks[pos - 1].priority > hook.priority:
            pos -= 1
        self.hooks.insert(pos, hook)

    def register_training_hooks(self, lr_config, optimizer_config=None, checkpoint_config=None, log_config=None,
                                momentum_config=None, custom_hooks_config=None):
        if lr_config is not None:
            cfg = dict(lr_config)
            policy = cfg.pop('policy', 'step')
            if policy not in LrSchedule.POLICIES:
                raise NotImplementedError(f'lr policy {policy!r}: implemented are {LrSchedule.POLICIES}')
            self.register_hook(StepLrUpdaterHook(policy=policy, **cfg), 'VERY_HIGH')
        if isinstance(optimizer_config, Hook):
            self.register_hook(optimizer_config, 'ABOVE_NORMAL')
        else:
            oc = dict(optimizer_config or {})
            self.register_hook(HOOKS[oc.pop('type', 'OptimizerHook')](**oc), 'ABOVE_NORMAL')
        if checkpoint_config is not None:
            self.register_hook(CheckpointHook(**checkpoint_config), 'NORMAL')
        if log_config is not None:
            for h in log_config.get('hooks', [dict(type='TextLoggerHook')]):
                h = dict(h)
                self.register_hook(HOOKS[h.pop('type')](interval=log_config.get('interval', 50), **h), 'VERY_LOW')
        for h in custom_hooks_config or []:
            h = dict(h)
            prio = h.pop('priority', 'NORMAL')
            self.register_hook(HOOKS[h.pop('type')](**h), prio)

    def call_hook(self, stage):
        for h in self.hooks:
            getattr(h, stage)(self)

    def save_checkpoint(self, out_dir, filename, create_latest=True):
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, filename)
        save_checkpoint(self.model, self.optimizer, path, dict(self.meta, epoch=self.epoch + 1, iter=self.iter))
        if create_latest:
            import shutil
            shutil.copyfile(path, os.path.join(out_dir, 'latest.pth'))

    def load_checkpoint(self, path):
        return load_checkpoint(self.model, path)

    def resume(self, path):
        m = load_checkpoint(self.model, path, self.optimizer)
        self.epoch, self.iter = m.get('epoch', 0), m.get('iter', 0)
        self.logger(f'resumed epoch {self.epoch}, iter {self.iter} from {path}')

    def train(self, data_source):
        self.model.train()
        self.data_loader = data_source          # mmcv's EpochBasedRunner.train: what the hooks reach as runner.data_loader
        self.call_hook('before_train_epoch')
        for i in range(data_source.iters_per_epoch):
            self.inner_iter = i
            # mmcv's EpochBasedRunner.train: the batch is runner.data_batch before the before_train_iter hooks run
            self.data_batch = data_source.batch(self.iter, self.device)
            self.call_hook('before_train_iter')
            self.outputs = self.model.train_step(self.data_batch, self.optimizer)
            self.call_hook('after_train_iter')
            self.data_batch = None
            self.iter += 1
            if self._max_iters is not None and self.iter >= self._max_iters:
                return False
        self.call_hook('after_train_epoch')
        self.epoch += 1
        return True

    @staticmethod
    def check_workflow(workflow):
        """-> [(mode, n)]: a list of ('train' | 'val', positive int) with at least one 'train' entry (mmcv's loop ends on
        the epoch count, which only training moves).  Anything else: ValueError naming the entry."""
        if not isinstance(workflow, (list, tuple)) or not workflow:
            raise ValueError(f"workflow {workflow!r}: a non-empty list of ('train' | 'val', positive int) entries")
        out = []
        for entry in workflow:
            ok = isinstance(entry, (list, tuple)) and len(entry) == 2 and entry[0] in ('train', 'val') and \
                isinstance(entry[1], int) and not isinstance(entry[1], bool) and entry[1] > 0
            if not ok:
                raise ValueError(f"workflow entry {entry!r}: expected ('train' | 'val', positive int)")
            out.append((entry[0], entry[1]))
        if not any(m == 'train' for m, _ in out):
            raise ValueError(f"workflow {workflow!r}: no ('train', n) entry -- the run would never reach max_epochs")
        return out

    @staticmethod
    def val_pass_index(workflow, epoch, entry, rep):
        """The number of validation epochs the workflow completed before repetition `rep` of its entry `entry`, reached with
        `epoch` training epochs done -- counted from epoch 0 of the run, so a resumed run continues the sequence.
        With T training and V validation epochs per cycle, t and v of them in front of the entry:
        cycles = max(0, ceil((epoch - t) / T)) (whole cycles behind us; ceil: the last 'train' entry of a run may stop short
        at max_epochs), index = cycles * V + v + rep."""
        per_t = sum(n for m, n in workflow if m == 'train')
        per_v = sum(n for m, n in workflow if m == 'val')
        pre_t = sum(n for m, n in workflow[:entry] if m == 'train')
        pre_v = sum(n for m, n in workflow[:entry] if m == 'val')
        cycles = max(0, -((pre_t - epoch) // per_t))
        return cycles * per_v + pre_v + rep

    def val(self, data_source, pass_index=0):
        """One validation epoch (mmcv EpochBasedRunner.val): the model in eval(), autograd off, every batch through
        model.val_step -- the same loss dict as a training step, BatchNorm on the running statistics, nothing updated.
        `iter` and `epoch` do not move.  Pass `pass_index` draws data_source.batch(pass_index * iters_per_epoch + i).
        value * num_samples of every logged scalar and num_samples are summed on the device in fp64 (plain torch ops, no
        host read per iteration); val_epoch_mean() is sum(v n) / sum(n), mmcv's LogBuffer.average."""
        self.model.eval()
        self.mode = 'val'
        self.val_sums, self.val_keys, self.val_iters = None, None, data_source.iters_per_epoch
        self._val_mean, self._val_logged = None, False
        per = data_source.iters_per_epoch
        with torch.no_grad():
            self.call_hook('before_val_epoch')
            for i in range(per):
                self.inner_iter = i
                self.data_batch = data_source.batch(pass_index * per + i, self.device)
                self.call_hook('before_val_iter')
                self.outputs = self.model.val_step(self.data_batch, self.optimizer)
                self._val_accumulate(self.outputs)
                self.call_hook('after_val_iter')
                self.data_batch = None
            if self.val_sums is not None and self.world_size > 1 and torch.distributed.is_initialized():
                # one collective per validation epoch: [sum(v n) x k | sum(n)] over the ranks
                t = self.val_sums
                if t.is_cuda and torch.distributed.get_backend() != 'nccl':      # CPU process group: through the host
                    h = t.cpu()
                    torch.distributed.all_reduce(h)
                    t.copy_(h)
                else:
                    torch.distributed.all_reduce(t)
            self.call_hook('after_val_epoch')
        return True

    def _val_accumulate(self, outputs):
        log_vars = outputs.get('log_vars') or {}
        if not log_vars:
            return
        n = outputs.get('num_samples', 1)
        vec = outputs.get('log_tensor')          # the logged scalars as one device tensor, in log_vars' order (YuNet.val_step)
        if vec is None:                          # any other model: its log_vars are host numbers
            vec = torch.tensor([float(v) for v in log_vars.values()], dtype=torch.float64)
        if self.val_sums is None:
            self.val_keys = list(log_vars)
            self.val_sums = torch.zeros(len(self.val_keys) + 1, device=vec.device, dtype=torch.float64)
        k = len(self.val_keys)
        self.val_sums[:k] += vec[:k].to(torch.float64) * n
        self.val_sums[k] += n

    def val_epoch_mean(self):
        """{key: sum(value * num_samples) / sum(num_samples)} of the validation epoch that just ran (python floats; the one
        host read of the epoch), or None when its steps logged nothing."""
        if self.val_sums is None:
            return None
        if self._val_mean is None:
            k = len(self.val_keys)
            self._val_mean = dict(zip(self.val_keys, (self.val_sums[:k] / self.val_sums[k]).tolist()))
        return self._val_mean

    def run(self, data_sources, workflow=(('train', 1),), device='cuda'):
        """mmcv's EpochBasedRunner.run: cycle through the (mode, n) entries of `workflow`, source i serving entry i, until
        `epoch` reaches max_epochs; a 'train' entry stops early there, a 'val' entry that follows the last training epoch
        still runs.  A run cut by max_iters inside an epoch ends at once (no validation epoch follows)."""
        self.device = device
        workflow = self.check_workflow(workflow)
        sources = list(data_sources) if isinstance(data_sources, (list, tuple)) else [data_sources]
        if len(sources) != len(workflow):
            raise ValueError(f'{len(sources)} data source(s) for a workflow of {len(workflow)} entries {workflow!r}: one source '
                             f'per entry')
        self.data_source = sources[[m for m, _ in workflow].index('train')]     # max_iters: the length of a training epoch
        self.call_hook('before_run')
        go = True
        while go and self.epoch < self._max_epochs:
            for i, (mode, n) in enumerate(workflow):
                for rep in range(n):
                    if mode == 'train':
                        if self.epoch >= self._max_epochs:
                            break
                        self.mode = 'train'
                        go = self.train(sources[i])
                    else:
                        self.val(sources[i], self.val_pass_index(workflow, self.epoch, i, rep))
                    if not go:
                        break
                if not go:
                    break
        self.call_hook('after_run')
        return self.log_buffer


def find_latest_checkpoint(path, suffix='pth'):
    """mmdet/utils/misc.py:11-42: `latest.pth` if present, else the checkpoint with the largest
    trailing number (epoch_12.pth, iter_5000.pth)."""
    import glob
    import warnings
    if not os.path.exists(path):
        warnings.warn('The path of checkpoints does not exist.')
        return None
    if os.path.exists(os.path.join(path, f'latest.{suffix}')):
        return os.path.join(path, f'latest.{suffix}')
    best, best_path = -1, None
    for ck in glob.glob(os.path.join(path, f'*.{suffix}')):
        try:
            n = int(os.path.basename(ck).split('_')[-1].split('.')[0])
        except ValueError:
            continue
        if n > best:
            best, best_path = n, ck
    if best_path is None:
        warnings.warn('There are no checkpoints in the path.')
    return best_path


def update_data_root(cfg, log=print):
    """mmdet/utils/misc.py:45-76 (called first thing by tools/train.py:113 and tools/test.py:138): with the
    environment variable MMDET_DATASETS set, every string under cfg.data that contains cfg.data_root gets that part
    replaced by the variable's value, and cfg.data_root becomes that value.  Like the reference, nested dicts are
    walked, lists (pipelines) are not."""
    dst = os.environ.get('MMDET_DATASETS')
    if dst is None or cfg.get('data_root') is None or cfg.get('data') is None:
        return cfg
    log(f'MMDET_DATASETS has been set to be {dst}.Using {dst} as data root.')
    src = cfg['data_root']

    def walk(node):
        for k, v in list(node.items()):
            if isinstance(v, dict):
                walk(v)
            elif isinstance(v, str) and src in v:
                node[k] = v.replace(src, dst)
    walk(cfg['data'])
    cfg['data_root'] = dst
    return cfg


def auto_scale_lr(cfg, distributed, log=print):
    """mmdet/apis/train.py:71-113: the linear scaling rule, applied when the config carries
    `auto_scale_lr = dict(enable=True, base_batch_size=B)` (tools/train.py --auto-scale-lr switches `enable` on):
    optimizer.lr *= (GPUs x samples_per_gpu) / B.  Returns the learning rate in effect."""
    asl = cfg.get('auto_scale_lr')
    if not asl or not asl.get('enable', False):
        log('Automatic scaling of learning rate (LR) has been disabled.')
        return cfg.optimizer['lr']
    base = asl.get('base_batch_size')
    if base is None:
        return cfg.optimizer['lr']
    if distributed:
        from .parallel import get_dist_info
        num_gpus = get_dist_info()[1]
    else:
        num_gpus = len(cfg.get('gpu_ids') or [0])
    data = cfg.get('data') or {}
    spg = (data.get('train_dataloader') or {}).get('samples_per_gpu', data.get('samples_per_gpu'))
    batch = num_gpus * spg
    log(f'Training with {num_gpus} GPU(s) with {spg} samples per GPU. The total batch size is {batch}.')
    if batch != base:
        scaled = (batch / base) * cfg.optimizer['lr']
        log(f"LR has been automatically scaled from {cfg.optimizer['lr']} to {scaled}")
        cfg.optimizer['lr'] = scaled
    else:
        log(f"The batch size match the base batch size: {base}, will not scaling the LR ({cfg.optimizer['lr']}).")
    return cfg.optimizer['lr']


_DETERMINISTIC = False       # set_random_seed(seed, deterministic=True | 'fast'): read by train_detector


def set_random_seed(seed, deterministic=False):
    """mmdet/apis/train.py:196-214: seed python's, numpy's and torch's generators.  `deterministic` -- cuDNN's
    deterministic mode in the reference -- selects the bit-reproducible training step of the fused engine
    (YuNet.set_deterministic) for every model train_detector builds afterwards.  As in the reference, where False leaves
    the cuDNN flags alone, a later set_random_seed(seed) does not switch the mode off; cfg.deterministic = True is the
    per-run spelling.  'fast' selects the fast deterministic level (YuNet.set_deterministic('fast'))."""
    import random
    import numpy as np
    global _DETERMINISTIC
    deterministic = det_level(deterministic)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    if deterministic:
        _DETERMINISTIC = deterministic


def wants_deterministic(cfg):
    """cfg.deterministic = True | 'fast', or set_random_seed(seed, deterministic=...) earlier in this process: the level
    (False | True | 'fast'); the config's own spelling wins."""
    return det_level(cfg.get('deterministic', False)) or _DETERMINISTIC


CUMULATIVE_HOOKS = ('GradientCumulativeOptimizerHook', 'GradientCumulativeFp16OptimizerHook')


def optimizer_hook_config(cfg, distributed=False):
    """What train_detector hands register_training_hooks as optimizer_config: with cfg.fp16 the fp16 hook itself
    (mmdet/apis/train.py:181-185) -- GradientCumulativeFp16OptimizerHook when optimizer_config.type names a cumulative hook,
    Fp16OptimizerHook otherwise -- and without it the config dict, whose `type` the runner looks up in HOOKS."""
    fp16_cfg = cfg.get('fp16', None)
    opt_cfg = dict(cfg.get('optimizer_config') or {})
    if fp16_cfg is None:
        return opt_cfg
    if opt_cfg.get('type') in CUMULATIVE_HOOKS:
        opt_cfg.pop('type')
        return GradientCumulativeFp16OptimizerHook(**opt_cfg, **fp16_cfg, distributed=distributed)
    return Fp16OptimizerHook(**opt_cfg, **fp16_cfg, distributed=distributed)


def train_detector(model, dataset, cfg, distributed=False, validate=False, timestamp=None,
                   meta=None, max_iters=None, device='cuda', log=print, extra_hooks=()):
    """mmdet/apis/train.py:117-246 surface: DDP wrap, optimizer, EpochBasedRunner, fp16 / optimizer /
    lr / checkpoint / logger hooks from the config, auto-resume / resume / load_from, run.
    extra_hooks: Hook objects of the caller, registered after the config's at priority LOWEST.
    Returns the logged history (one dict of python floats per logging interval)."""
    if wants_deterministic(cfg):
        if cfg.get('fp16', None) is not None or \
                dict(cfg.get('optimizer_config') or {}).get('type') == 'GradientCumulativeFp16OptimizerHook':
            raise NotImplementedError('deterministic training with cfg.fp16 (bf16 activation storage): the deterministic mode '
                                      'covers the fp32 storage build only')
        model.set_deterministic(wants_deterministic(cfg))
    model = model.to(device)
    model.train()
    if distributed:
        model = build_ddp(model, device, device_ids=[torch.cuda.current_device()],
                          broadcast_buffers=False)
    auto_scale_lr(cfg, distributed, log if cfg.get('auto_scale_lr') else (lambda *a: None))
    optimizer = build_optimizer(model, cfg.optimizer)
    runner = EpochBasedRunner(model, optimizer, cfg.get('work_dir'), log, meta,
                              max_epochs=cfg.runner['max_epochs'], max_iters=max_iters)
    optimizer_config = optimizer_hook_config(cfg, distributed)
    log_config = cfg.get('log_config')
    if max_iters is not None and max_iters <= 64 and log_config is not None:
        log_config = dict(log_config, interval=1)          # short smoke runs: log every iteration
    runner.register_training_hooks(cfg.lr_config, optimizer_config, cfg.get('checkpoint_config'), log_config,
                                   cfg.get('momentum_config'), cfg.get('custom_hooks'))
    # EvalHook (mmdet/apis/train.py:204-232): validate=True and a validation set in the config
    if validate and cfg.get('data') is not None and cfg.get('data').get('val') is not None:
        from .builder import build_dataset
        val_cfg = dict(cfg.get('data')['val'])
        val_cfg['test_mode'] = True
        eval_cfg = dict(cfg.get('evaluation', {}))
        eval_cfg['by_epoch'] = dict(cfg.runner).get('type', 'EpochBasedRunner') != 'IterBasedRunner'
        scale = None
        for t in val_cfg.get('pipeline') or []:
            if t.get('type') == 'MultiScaleFlipAug' and t.get('img_scale') is not None:      # (scale_factor lists: the parser)
                scale = tuple(t['img_scale']) if not isinstance(t['img_scale'], list) else tuple(t['img_scale'][0])
        # mmdet/apis/train.py:206-222: data.val_dataloader.samples_per_gpu (default 1).  A value above 1, a
        # data.val.cache, or a val pipeline that spells its transforms out runs the batched device test pipeline,
        # built from that list; otherwise (the shipped configs) the per-image path, which reads img_scale only
        val_loader = cfg.get('data').get('val_dataloader') or {}
        val_spg = int(val_loader.get('samples_per_gpu', 1))
        grouped = {k: val_loader[k] for k in ('group_by', 'max_batch_pixels') if k in val_loader}
        val_cache = val_cfg.pop('cache', None)
        val_pipe = val_cfg.get('pipeline') or []
        spelled = any(t.get('type') == 'MultiScaleFlipAug' and t.get('transforms') for t in val_pipe)
        batched = dict(samples_per_gpu=val_spg, cache=val_cache, **grouped,
                       pipeline=list(val_pipe) if (spelled or val_spg > 1 or val_cache is not None
                                                   or grouped.get('group_by') is not None) else None)
        if os.path.exists(val_cfg.get('ann_file', '')):
            runner.register_hook(EvalHook(build_dataset(val_cfg), scale=scale or (640, 640), distributed=distributed,
                                          **batched, **eval_cfg), 'LOW')
        else:
            log(f"validate: {val_cfg.get('ann_file')} not found -- no EvalHook registered")
    for h in extra_hooks:
        runner.register_hook(h, 'LOWEST')
    resume_from = cfg.get('resume_from')
    if not resume_from and cfg.get('auto_resume') and cfg.get('work_dir'):
        resume_from = find_latest_checkpoint(cfg.work_dir)
    if resume_from:
        runner.resume(resume_from)
    elif cfg.get('load_from'):
        runner.load_checkpoint(cfg.load_from)
    # `dataset`: one source, or one per workflow entry (tools/train.py builds the second from data.val for a two-entry workflow)
    sources = list(dataset) if isinstance(dataset, (list, tuple)) else [dataset]
    return runner.run(sources, cfg.get('workflow', [('train', 1)]), device=device)


# the reference's custom hooks (mmdet/core/hook/: EMA, box-size statistics, loss check) register themselves in HOOKS
from . import hooks  # noqa: E402,F401
