"""YuNet detector shell (mmdet/models/detectors/yunet.py:9-86, single_stage.py:17-57,
base.py:168-252) whose `forward_train` is the fused MI355X engine.

The registered sub-modules own the `nn.Parameter`s under the reference's state_dict names;
on first use on a GPU every parameter / buffer is re-pointed to a view of the engine's flat
buffers, so checkpoints load with `strict=True`, `model.parameters()` works with any
optimizer, and the kernels see one contiguous 303 KB (n) / 218 KB (s) block.
"""
import os
import warnings
from collections import OrderedDict

import torch
import torch.nn as nn

from .builder import DETECTORS, build_backbone, build_head, build_neck
from .engine import YuNetEngine, det_level
from .sim_ota_assigner import pad_ignore


class _LogRecord:
    """The five logged scalars of ONE iteration: filled by an asynchronous device-to-host copy,
    frozen into python floats the first time one of them is read (the pinned staging row is
    reused 256 iterations later)."""

    def __init__(self, model, row):
        self.model, self.row, self.event, self.vals = model, row, None, None

    def resolve(self):
        if self.vals is None:
            if self.event is None:
                # world > 1: the averaged values arrive with the gradient all-reduce of backward.
                # A collective issued from here would only be entered by the rank that reads the
                # value (rank 0 logs) and hang, so refuse instead.
                raise RuntimeError('log_vars of a distributed training step are available after '
                                   'loss.backward() (they travel with the gradient all-reduce)')
            self.event.synchronize()
            self.vals = [float(v) for v in self.row[:5]]
            self.model = self.row = None
        return self.vals


def bbox_mapping_back(bboxes, meta):
    """Boxes of one test-time view -> original image coordinates
    (mmdet/core/bbox/transforms.py:22-48, 63-72): un-flip with the view's img_shape, then divide
    by its scale_factor."""
    b = bboxes.clone()
    if meta.get('flip', False):
        direction = meta.get('flip_direction', 'horizontal')
        h, w = meta['img_shape'][:2]
        if direction not in ('horizontal', 'vertical', 'diagonal'):
            raise ValueError(f'flip_direction {direction!r}')
        if direction in ('horizontal', 'diagonal'):
            b[:, 0], b[:, 2] = w - bboxes[:, 2], w - bboxes[:, 0]
        if direction in ('vertical', 'diagonal'):
            b[:, 1], b[:, 3] = h - bboxes[:, 3], h - bboxes[:, 1]
    sf = torch.as_tensor(meta['scale_factor'], dtype=b.dtype, device=b.device).reshape(-1)
    return b / (sf if sf.numel() == 4 else sf[:1])


def skip_ema_entries(module, incompatible_keys):
    """load_state_dict post-hook: `ema_*` entries (the EMA hooks' buffers, hooks.BaseEMAHook) that only the checkpoint
    or only the model has are dropped from the unexpected / missing keys, with a warning naming how many -- what mmcv's
    load_checkpoint(strict=False) gives the reference for an EMA checkpoint loaded into a model without the hook, or a
    resume that runs before the hook's before_run (which is why the hook has its own resume_from).  Any other mismatch
    still fails a strict load."""
    extra = [k for k in incompatible_keys.unexpected_keys if k.startswith('ema_')]
    missing = [k for k in incompatible_keys.missing_keys if k.startswith('ema_')]
    if not extra and not missing:
        return
    for k in extra:
        incompatible_keys.unexpected_keys.remove(k)
    for k in missing:
        incompatible_keys.missing_keys.remove(k)
    warnings.warn(f'{type(module).__name__}.load_state_dict: {len(extra)} unexpected and {len(missing)} missing '
                  f'ema_* entries skipped (EMA hook state)')


class LazyScalar:
    """A logged loss value that is copied to the host asynchronously and only waited for
    when somebody reads it (the reference calls .item() five times per iteration,
    base.py:210-215, stalling the stream each time)."""

    def __init__(self, record, index):
        self._rec, self._i = record, index

    def __float__(self):
        return self._rec.resolve()[self._i]

    def item(self):
        return float(self)

    def __format__(self, spec):
        return format(float(self), spec)

    def __repr__(self):
        return repr(float(self))

    def __add__(self, o):
        return float(self) + o
    __radd__ = __add__

    def __mul__(self, o):
        return float(self) * o
    __rmul__ = __mul__


class _EngineStep(torch.autograd.Function):
    """Autograd node standing for the whole fused step: forward already ran in the engine;
    backward launches the backward op list, which writes straight into the flat gradient
    buffer the parameters' .grad tensors are views of."""

    @staticmethod
    def forward(ctx, anchor, model, losses, img=None):
        """-> loss_cls, loss_bbox, loss_obj, loss_kps and their total (written by the finalize
        kernel): train_step backpropagates the total directly, no tensor arithmetic in between.
        `img`: the caller's image when it asked for a gradient (the step ran on an input_grad plan)."""
        ctx.model = model
        ctx.img_meta = None if img is None else (img.dtype, img.dim() == 4 and not img.is_contiguous()
                                                 and img.is_contiguous(memory_format=torch.channels_last))
        ctx.set_materialize_grads(False)      # undefined output grads stay None: backward()'s fast path below
        out = losses.detach().clone()
        return out[0], out[1], out[2], out[3], out[4]

    @staticmethod
    def backward(ctx, g0, g1, g2, g3, gt):
        model = ctx.model
        eng = model.engine
        if g0 is None and g1 is None and g2 is None and g3 is None and gt is not None:
            # loss = total: one upstream scalar scales all 16 head channels
            eng.scale_buffer().copy_(gt.expand(16))
        else:
            z = eng.scale_buffer().new_zeros(())
            gs = [(g if g is not None else z) + (gt if gt is not None else z) for g in (g0, g1, g2, g3)]
            eng.scale_buffer().copy_(torch.stack([gs[0]] + [gs[1]] * 4 + [gs[2]] + [gs[3]] * 10))
        # kernels + (world > 1) the bucketed gradient all-reduce; .grad None (a first backward, zero_grad(set_to_none=True)):
        # nothing to accumulate onto (engine.set_grad_accumulation)
        eng.backward(fresh=model._sentinel[1].grad is None)
        model._after_backward()
        if ctx.img_meta is None:
            return None, None, None
        # the image gradient the backward list just wrote (a fresh tensor: autograd may keep it as img.grad), in the
        # image's dtype and memory format
        dimg = eng.input_grad_out
        eng.input_grad_out = None
        if not ctx.needs_input_grad[3]:
            return None, None, None, None
        dtype, channels_last = ctx.img_meta
        dimg = dimg.to(dtype)
        if channels_last:
            dimg = dimg.contiguous(memory_format=torch.channels_last)
        return None, None, None, dimg


@DETECTORS.register_module()
class YuNet(nn.Module):
    def __init__(self, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None, init_cfg=None):
        super().__init__()
        self.backbone = build_backbone(backbone)
        if neck is not None:
            self.neck = build_neck(neck)
        bbox_head = dict(bbox_head)
        bbox_head.update(train_cfg=train_cfg, test_cfg=test_cfg)
        self.bbox_head = build_head(bbox_head)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.fp16_enabled = False
        self.engine = None
        self._world, self._group = 1, None
        self._anchor = None
        self.init_weights(pretrained)
        # checkpoints with the EMA hooks' ema_* entries load everywhere a YuNet is loaded (train, test, export tools)
        self.register_load_state_dict_post_hook(skip_ema_entries)

    # ------------------------------------------------------------------ mmdet surface
    @property
    def with_neck(self):
        return hasattr(self, 'neck') and self.neck is not None

    @property
    def with_bbox(self):
        return hasattr(self, 'bbox_head') and self.bbox_head is not None

    def init_weights(self, pretrained=None):
        self.backbone.init_weights(pretrained=pretrained)
        if self.with_neck:
            self.neck.init_weights()
        self.bbox_head.init_weights()

    def extract_feat(self, img):
        x = self.backbone(img)
        return self.neck(x) if self.with_neck else x

    def feature_test(self, img):
        return self.bbox_head(self.extract_feat(img))

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    def forward_test(self, imgs, img_metas, **kwargs):
        """mmdet/models/detectors/base.py:132-167: one augmentation -> simple_test, several
        (MultiScaleFlipAug) -> aug_test."""
        if isinstance(imgs, (list, tuple)):
            if len(imgs) != 1:
                return self.aug_test(imgs, img_metas, **kwargs)
            imgs, img_metas = imgs[0], img_metas[0]
        return self.simple_test(imgs, img_metas, **kwargs)

    @torch.no_grad()
    def aug_test(self, imgs, img_metas, rescale=False):
        """Test-time augmentation (mmdet/models/detectors/single_stage.py:135-157 ->
        dense_test_mixins.py:41-114): every augmented view (scale and / or flip) of ONE image is
        run through the eval forward, its candidates (score >= score_thr, decoded, no NMS) are
        mapped back to the original image (bbox_mapping_back: un-flip with the view's img_shape,
        divide by its scale_factor), the union is suppressed once (batched_nms) and cut to
        max_per_img.  rescale=False multiplies the result by the first view's scale_factor.

        Note on the reference: YuNet_Head.get_bboxes accepts with_nms but ignores it
        (yunet_head.py:298, 410-415), so its mixin path hands already-suppressed [n,5] tensors to
        bbox_mapping_back, whose view(-1, 4) then fails; this implements the behaviour the mixin
        documents (with_nms=False per view)."""
        if self.training:
            raise RuntimeError('aug_test requires model.eval()')
        cfg = self.test_cfg
        if cfg is None:
            raise ValueError('test_cfg (score_thr, nms.iou_threshold, max_per_img) is required')
        from . import kernels as K
        from .yunet_head import soft_nms_args
        nms_cfg = cfg.get('nms', dict(type='nms', iou_threshold=0.45))
        # the merge is Soft-NMS when the config says so (the same keys as the head's own path); validated before any launch
        soft = soft_nms_args(nms_cfg) if nms_cfg.get('type', 'nms') == 'soft_nms' else None
        boxes, scores = [], []
        for img, metas in zip(imgs, img_metas):
            if img.shape[0] != 1:
                raise ValueError('aug_test: one image per view (samples_per_gpu=1, as in the reference)')
            if not img.is_cuda:
                raise RuntimeError('YuNet.aug_test needs CUDA (ROCm) tensors: HIP kernels only, no CPU fallback')
            eng = self._ensure_engine(img.device)
            flat = eng.forward_eval(img.float().contiguous())
            dets, _, cnt = K.detect(flat, eng.plan.sizes, self.bbox_head.strides, cfg.get('score_thr', 0.02),
                                    iou_thr=2.0, with_kps=False)          # IoU <= 1: no suppression
            d = dets[0, :int(cnt[0])]
            b = bbox_mapping_back(d[:, :4], metas[0])
            boxes.append(b)
            scores.append(d[:, 4])
        boxes, scores = torch.cat(boxes), torch.cat(scores)
        if boxes.shape[0] == 0:
            return [[torch.zeros(0, 5).numpy()]]
        if soft is not None:
            dets, _, cnt = K.soft_nms(boxes[None].contiguous(), scores[None].contiguous(),
                                      max_out=cfg.get('max_per_img', -1), **soft)
        else:
            dets, _, cnt = K.nms(boxes[None].contiguous(), scores[None].contiguous(),
                                 nms_cfg.get('iou_threshold', 0.45), max_out=cfg.get('max_per_img', -1))
        out = dets[0, :int(cnt[0])].clone()
        if not rescale:
            sf0 = torch.as_tensor(img_metas[0][0]['scale_factor'], dtype=torch.float32, device=out.device).reshape(-1)
            out[:, :4] *= (sf0 if sf0.numel() == 4 else sf0[:1])
        return [[out.cpu().numpy()]]

    @torch.no_grad()
    def simple_test(self, img, img_metas, rescale=False, with_landmarks=False):
        """mmdet/models/detectors/yunet.py:53-81: eval-mode forward -> get_bboxes -> bbox2result:
        per image a one-element list (one class) with an [n, 5] float32 array
        (x1, y1, x2, y2, score), descending score.  with_landmarks=True also returns the decoded
        5-point landmarks [n, 10] per image."""
        if self.training:
            raise RuntimeError('simple_test requires model.eval() (BatchNorm on running statistics)')
        if not img.is_cuda:
            raise RuntimeError('YuNet.simple_test needs a CUDA (ROCm) tensor: HIP kernels only, no CPU fallback')
        eng = self._ensure_engine(img.device)
        flat = eng.forward_eval(img.float().contiguous())
        dets, lmk = self.bbox_head.get_bboxes_batch(flat, eng.plan.sizes, img_metas, rescale=rescale)
        out = [[d] for d in dets]                                  # bbox2result, num_classes = 1
        return (out, lmk) if with_landmarks else out

    # ------------------------------------------------------------------ engine binding
    def arch(self):
        bb, hd = self.backbone, self.bbox_head
        # (raises on a reduction, loss type or parameter the fused loss step does not implement)
        # loss_cls / loss_obj / loss_kps: dict(type=, **parameters), present only beside the default terms
        terms = hd.loss_term_specs() if hd.loss_cfg().terms is not None else {}
        # ignore regions: the key is present only when the assigner's ignore_iof_thr is on
        thr = getattr(hd.assigner, 'ignore_iof_thr', -1.0)
        if thr >= 0:
            terms = dict(terms, ignore_iof_thr=thr)
        return dict(
            **terms,
            stage_channels=bb.stage_channels, downsample_idx=bb.downsample_idx, out_idx=bb.out_idx,
            neck_channels=self.neck.in_channels, neck_out_idx=self.neck.out_idx,
            feat_channels=hd.feat_channels, shared_stacked_convs=hd.shared_stack_convs,
            stacked_convs=hd.stacked_convs, kps_num=hd.NK, strides=hd.strides,
            loss_bbox=type(hd.loss_bbox).__name__, loss_bbox_weight=hd.loss_bbox.loss_weight,
            loss_bbox_eps=hd.loss_bbox.eps, loss_bbox_smooth_point=getattr(hd.loss_bbox, 'smooth_point', 0.1),
            loss_bbox_mode=getattr(hd.loss_bbox, 'mode', None),
            loss_cls_weight=hd.loss_cls.loss_weight, loss_obj_weight=hd.loss_obj.loss_weight,
            loss_kps_weight=hd.loss_kps.loss_weight, kps_beta=getattr(hd.loss_kps, 'beta', 1.0),            center_radius=hd.assigner.center_radius if hd.assigner is not None else 2.5,
            candidate_topk=getattr(hd.assigner, 'candidate_topk', 10), iou_weight=getattr(hd.assigner, 'iou_weight', 3.0),
            cls_weight=getattr(hd.assigner, 'cls_weight', 1.0))

    def set_precision(self, precision):
        """'fp32' (default) or 'bf16': bf16 activation storage + bf16 matrix instruction in the forward
        pointwise convs, fp32 gradients / master weights / loss step (BASELINE.json configs[2]; the
        reference's analogue is fp16 training, mmdet/apis/train.py:181-185 -> Fp16OptimizerHook)."""
        if precision not in ('fp32', 'bf16'):
            raise ValueError(f"precision {precision!r}: 'fp32' or 'bf16'")
        if precision == 'bf16' and getattr(self, '_deterministic', False):
            raise NotImplementedError(f"precision='bf16' with deterministic={self._deterministic!r}: the deterministic mode covers the fp32 "
                                      'storage build only')
        self._precision = precision
        self.fp16_enabled = precision != 'fp32'
        if self.engine is not None:
            self.engine.set_precision(precision)

    def set_deterministic(self, flag=True):
        """Bit-reproducible training step (engine.YuNetEngine.deterministic): same inputs, same state, same build and same
        device model give the same losses, gradients, parameters and BatchNorm buffers, byte for byte -- one process,
        world size 1, fp32 storage.  Plans built before the call keep their mode; the next step builds its own.
        False | True | 'fast': 'fast' keeps the kernels of the default mode (their order-fixed forms) instead of the
        exact-fp32 tile kernels -- the same contract at a lower cost, other bytes than True."""
        flag = det_level(flag)
        if flag and getattr(self, '_precision', 'fp32') == 'bf16':
            raise NotImplementedError(f"deterministic={flag!r} with precision='bf16': the deterministic mode covers the fp32 "
                                      'storage build only')
        self._deterministic = flag
        if self.engine is not None:
            self.engine.set_deterministic(flag)

    def set_grad_accumulation(self, flag=True):
        """Gradient accumulation (engine.YuNetEngine.set_grad_accumulation): with it on, backward() adds to the parameters'
        .grad as PyTorch does, so k calls of (loss / k).backward() without a zero_grad() in between leave the gradient of the
        k micro-batches together -- of any geometry; the flat gradient is shared by all plans.  A backward that follows
        optimizer.zero_grad(), or finds .grad None, costs nothing extra.  Off (default): .grad is overwritten.
        BatchNorm statistics stay those of each micro-batch (README)."""
        self._grad_accum = bool(flag)
        if self.engine is not None:
            self.engine.set_grad_accumulation(flag)

    def set_data_parallel(self, world_size, group=None):
        """Called by YuNetDistributedDataParallel: one process per GPU, RCCL collectives."""
        self._world, self._group = world_size, group
        if self.engine is not None:
            self.engine.world_size, self.engine.process_group = world_size, group
            self.engine.plans.clear()
            self.engine.disable_oneshot()
            self._maybe_oneshot()

    def _maybe_oneshot(self):
        """YUNET_ONESHOT_AR=1: the step's collectives through peer-mapped inboxes (oneshot.py) instead of the process
        group; kept only if it reproduces the group's all-gather bit for bit."""
        if self._world > 1 and os.environ.get('YUNET_ONESHOT_AR') == '1' and self.engine is not None:
            if not self.engine.enable_oneshot(verify=True):
                warnings.warn('YUNET_ONESHOT_AR=1: the one-shot all-reduce failed its self-check; '
                              'staying on the process group collectives')

    def _bound(self):
        if self.engine is None:
            return False
        w = self.backbone.model0.conv1.weight
        return w.data_ptr() == self.engine.params.view('backbone.model0.conv1.weight').data_ptr()

    def bind_engine(self, device):
        """(Re)create the engine on `device` and re-point every parameter/buffer into it."""
        sd = {k: v.detach().clone() for k, v in self.state_dict().items()}
        eng = YuNetEngine(self.arch(), device, self._world, self._group)
        eng.set_precision(getattr(self, '_precision', 'fp32'))
        eng.set_deterministic(getattr(self, '_deterministic', False))
        eng.set_grad_accumulation(getattr(self, '_grad_accum', False))
        eng.params.load_state_dict(sd)
        fp = eng.params
        for name, p in self.named_parameters():
            p.data = fp.view(name)
            p.grad = fp.view(name, of=fp.grad)
        # what the freeze signature is read from at every step (_sync_frozen): the modules' own flags
        self._params = list(self.named_parameters())
        self._bn_mods = [(bn_name, self.get_submodule(bn_name)) for bn_name in fp.layout.bn_names]
        self._frozen_sig = ((), ())
        self._sentinel = self._params[0]
        for i, bn_name in enumerate(fp.layout.bn_names):
            mod = self.get_submodule(bn_name)
            o, c = fp.bn_offset[bn_name], fp.bn_channels[i]
            mod._buffers['running_mean'] = fp.running_mean[o:o + c]
            mod._buffers['running_var'] = fp.running_var[o:o + c]
            mod._buffers['num_batches_tracked'] = fp.num_batches_tracked[i]
        self.engine = eng
        self.bind_ema()
        self._maybe_oneshot()
        self._anchor = torch.zeros(1, device=device, requires_grad=True)
        self._log_host = torch.zeros(256, 8, dtype=torch.float32).pin_memory()
        self._log_iter = 0
        self._log_pending = None
        return eng

    @staticmethod
    def ema_name(key):
        """Buffer name of the EMA copy of state_dict entry `key` (mmdet/core/hook/ema.py: '.' -> '_')."""
        return 'ema_' + key.replace('.', '_')

    def bind_ema(self):
        """Re-point the EMA hooks' `ema_*` buffers (hooks.BaseEMAHook.before_run: one per state_dict entry, or per
        parameter with skip_buffers=True) into the engine's flat EMA mirror (FlatParams.enable_ema), the way
        bind_engine re-points the parameters and BN buffers: one fused launch then updates all of them, and
        state_dict() carries them under the reference's names.  The values the buffers hold -- registered before the
        engine existed, loaded from a checkpoint, or those of a previous binding -- are copied in.  Returns whether a
        mirror is bound (False: no engine, or no ema_ buffers)."""
        eng = self.engine
        if eng is None:
            return False
        fp = eng.params
        params = [n for n, _ in self.named_parameters()]
        bufs = [f'{bn}.{k}' for bn in fp.layout.bn_names for k in ('running_mean', 'running_var', 'num_batches_tracked')]
        hp = [self.ema_name(k) in self._buffers for k in params]
        hb = [self.ema_name(k) in self._buffers for k in bufs]
        if not any(hp) and not any(hb):
            return False
        if not all(hp) or (any(hb) and not all(hb)):
            raise RuntimeError('ema_ buffers for a part of the state_dict only: the EMA mirror covers every parameter '
                               '(and every BatchNorm buffer, or none of them)')
        keys = params + (bufs if all(hb) else [])
        old = {k: self._buffers[self.ema_name(k)] for k in keys}
        fp.enable_ema(buffers=all(hb))
        with torch.no_grad():
            for k in keys:
                v = fp.ema_view(k)
                v.copy_(old[k].reshape(v.shape))
                self._buffers[self.ema_name(k)] = v
        return True

    # ------------------------------------------------------------------ logged scalars
    def _log_copy(self, rec, src):
        """src[0:5] (device) -> the record's pinned row, on a side stream; the main stream
        (the backward / optimizer kernels that follow) never waits for it."""
        side = getattr(self, '_log_stream', None)
        if side is None:
            side = self._log_stream = torch.cuda.Stream(device=src.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            rec.row[:5].copy_(src[:5], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        rec.event = ev
        self._log_last_event = ev         # the next step's loss kernels overwrite src: see forward_train

    def _log_fetch_now(self, rec):
        eng = self.engine
        vec = eng.plan.losses[:5].clone()
        if eng.world_size > 1:
            eng._allreduce_mean(vec)
        self._log_copy(rec, vec)
        vec.record_stream(self._log_stream)
        if self._log_pending is rec:
            self._log_pending = None

    def _ensure_engine(self, device):
        if not self._bound() or self.engine.device != device:
            self.bind_engine(device)
        return self.engine

    def _sync_frozen(self, eng):
        """Fine-tuning: the engine honours the modules' own flags.  A BatchNorm2d with training == False under
        model.train() is frozen (running statistics in, nothing written back); a parameter with requires_grad == False
        takes no gradient (.grad None) and no update.  Read at every step -- two short walks, nothing else while the
        signature stays what it was -- and handed to the engine, whose plans are keyed by it."""
        sig = (tuple(n for n, m in self._bn_mods if not m.training),
               tuple(n for n, p in self._params if not p.requires_grad))
        if sig == self._frozen_sig:
            return
        self._frozen_sig = sig
        eng.set_frozen(*sig)
        frozen = set(sig[1])
        for name, p in self._params:
            p.grad = None if name in frozen else eng.params.view(name, of=eng.params.grad)
        self._sentinel = next(((n, p) for n, p in self._params if n not in frozen), self._params[0])

    def frozen_parameters(self):
        """[(name, parameter)] of the parameters the last forward_train found with requires_grad == False: the ones whose
        range of the flat gradient that step left at zero.  The fused optimizers give exactly these no update.  None before
        an engine is bound (nothing was read yet)."""
        sig = getattr(self, '_frozen_sig', None)
        if sig is None:
            return None
        frozen = set(sig[1])
        return [(n, p) for n, p in self._params if n in frozen] if frozen else []

    def _after_backward(self):
        eng = self.engine
        rec = self._log_pending
        if rec is not None and eng.world_size > 1:
            # the world-averaged logged scalars arrived in the head of the gradient buffer
            self._log_pending = None
            self._log_copy(rec, eng.params.log_head)
        name, w = self._sentinel                        # the first parameter that takes a gradient
        if w.requires_grad and (w.grad is None or w.grad.data_ptr() != eng.params.view(name, of=eng.params.grad).data_ptr()):
            frozen = self._frozen_sig[1]
            for name, p in self.named_parameters():     # zero_grad(set_to_none=True) happened
                p.grad = None if name in frozen else eng.params.view(name, of=eng.params.grad)

    # ------------------------------------------------------------------ training path
    def forward_train(self, img, img_metas, gt_bboxes, gt_labels, gt_keypointss=None,
                      gt_bboxes_ignore=None):
        """Same signature / returned dict as mmdet/models/detectors/yunet.py:21-51."""
        if not img.is_cuda:
            raise RuntimeError('YuNet.forward_train needs a CUDA (ROCm) tensor: the training '
                               'path is implemented as HIP kernels only, there is no CPU fallback')
        if gt_keypointss is None:
            raise ValueError('the shipped configs train with use_kps=True: gt_keypointss is required')
        eng = self._ensure_engine(img.device)
        if self.training:
            self._sync_frozen(eng)
        # (model.eval(): the modules' flags are NOT read -- every BatchNorm says eval there, and syncing that would build an
        # all-frozen plan with activation buffers of its own; the validation step runs on the plan of the engine's current key)
        ev = getattr(self, '_log_last_event', None)
        if ev is not None:
            # the previous step's logged scalars are copied to the host on a side stream from buffers
            # this step overwrites (a 20-byte copy issued milliseconds ago: never an actual wait)
            torch.cuda.current_stream().wait_event(ev)
            self._log_last_event = None
        # ignore regions: passed on only when the assigner's ignore_iof_thr is on (off: accepted and unused, as before)
        ign = self._ignore_args(eng, gt_bboxes_ignore, len(img), img.device)
        if not self.training:
            # the workflow's validation step (runner.EpochBasedRunner.val): the reference's forward_train under eval() --
            # BatchNorm on the running statistics, the same four losses, nothing written back.  The tensors carry no graph.
            l = eng.forward_val(img.float().contiguous(), gt_bboxes, gt_keypointss, *ign).detach().clone()
            out = dict(loss_cls=l[0], loss_bbox=l[1], loss_obj=l[2], loss_kps=l[3])
            self._last = (out, l[4], l[:5])
            return out
        # an image that asks for a gradient selects the plan whose backward ends with it
        want_dimg = torch.is_grad_enabled() and img.requires_grad
        eng.set_input_grad(want_dimg)
        if want_dimg:
            losses = eng.forward(img.detach().float().contiguous(), gt_bboxes, gt_keypointss, *ign)
            l = _EngineStep.apply(self._anchor, self, losses, img)
        else:
            losses = eng.forward(img.float().contiguous(), gt_bboxes, gt_keypointss, *ign)
            l = _EngineStep.apply(self._anchor, self, losses)
        out = dict(loss_cls=l[0], loss_bbox=l[1], loss_obj=l[2], loss_kps=l[3])
        self._last = (out, l[4])          # lets train_step use the kernel's total and log record
        return out

    @staticmethod
    def _ignore_args(eng, gt_bboxes_ignore, n, device):
        """-> () with ignore_iof_thr off, else (padded boxes [N,Imax,4], counts [N]): a DeviceGT's tensors as they are (the
        engine binds them without a copy), a list of tensors padded on the device, None as zero counts."""
        if eng.ignore_iof_thr < 0:
            return ()
        return pad_ignore(gt_bboxes_ignore, n, device)

    def _parse_losses(self, losses):
        """base.py:184-217: total = sum of the entries whose key contains 'loss'; log_vars are
        world-averaged.  One batched D2H copy (and one 5-float all-reduce) instead of five."""
        log_vars = OrderedDict((k, v.mean()) for k, v in losses.items())
        loss = sum(v for k, v in log_vars.items() if 'loss' in k)
        vec = torch.stack([v.detach() for v in log_vars.values()] + [loss.detach()])
        dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
        host = getattr(self, '_log_host', None)
        if host is None or not vec.is_cuda:
            if dist_on:
                vec = vec / torch.distributed.get_world_size()
                torch.distributed.all_reduce(vec)
            vals = vec.cpu().tolist()
            out = OrderedDict(zip(list(log_vars) + ['loss'], vals))
            return loss, out
        # generic dict (not produced by forward_train just now): world-average on a side stream
        rec = _LogRecord(self, host[self._log_iter % host.shape[0]])
        self._log_iter += 1
        if dist_on:
            side = getattr(self, '_log_stream', None)
            if side is None:
                side = self._log_stream = torch.cuda.Stream(device=vec.device)
            side.wait_stream(torch.cuda.current_stream())
            vec.record_stream(side)
            with torch.cuda.stream(side):
                vec.div_(torch.distributed.get_world_size())
                torch.distributed.all_reduce(vec)
        self._log_copy(rec, vec)
        vec.record_stream(self._log_stream)
        out = OrderedDict((k, LazyScalar(rec, i)) for i, k in enumerate(list(log_vars) + ['loss']))
        return loss, out

    def _parse_engine_losses(self, total):
        """_parse_losses for the dict forward_train just returned: the finalize kernel already
        wrote ((cls + bbox) + obj) + kps next to the four losses, so `loss` is that scalar (one
        autograd edge into the fused step) and log_vars are five lazily copied floats.  World
        size 1: copied to the host right away on a side stream.  World > 1: they sit in the head
        of the gradient buffer and come back averaged with the gradient all-reduce that backward
        issues (base.py:210-215 all-reduces each of them separately)."""
        eng = self.engine
        rec = _LogRecord(self, self._log_host[self._log_iter % self._log_host.shape[0]])
        self._log_iter += 1
        if eng.world_size > 1 and torch.is_grad_enabled() and total.requires_grad:
            self._log_pending = rec
        elif eng.world_size > 1:
            self._log_fetch_now(rec)      # val_step / no_grad: every rank is here, no backward follows
        else:
            self._log_copy(rec, eng.plan.losses)
        keys = ['loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps', 'loss']
        return total, OrderedDict((k, LazyScalar(rec, i)) for i, k in enumerate(keys))

    def train_step(self, data, optimizer):
        """base.py:219-252."""
        losses = self(**data)
        last = getattr(self, '_last', None)
        self._last = None
        if last is not None and last[0] is losses and self.engine is not None:
            loss, log_vars = self._parse_engine_losses(last[1])
        else:
            loss, log_vars = self._parse_losses(losses)
        out = dict(loss=loss, log_vars=log_vars, num_samples=len(data['img_metas']))
        if last is not None and len(last) == 3 and last[0] is losses:
            # a validation step (model.eval()): the five scalars once more as this rank's device tensor, in log_vars' order --
            # what the runner sums per validation epoch without a host read
            out['log_tensor'] = last[2]
        return out

    val_step = train_step
