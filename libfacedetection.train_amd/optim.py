"""Fused optimizers over the engine's flat parameter buffer: SGD, Adam and AdamW with parameter groups and
gradient clipping, each update one HIP launch (two with clipping).

torch.optim.SGD / Adam / AdamW semantics.  `build_optimizer` reads an mmcv optimizer config, `paramwise_cfg` included
(mmcv 1.x DefaultOptimizerConstructor: custom_keys, bias_lr_mult, bias_decay_mult, norm_decay_mult, dwconv_decay_mult),
and forms one parameter group per distinct (lr, weight_decay).  What the device sees of the groups is a byte per element
of the flat buffer (its group) and a small table of the groups' hyper-parameters, rewritten only when a hook changes one,
so LR schedules never force a host sync.

The shipped configs (configs/yunet_n.py:1: SGD, lr 0.01, momentum 0.9, weight_decay 5e-4 on EVERY parameter, no
paramwise_cfg, no grad_clip) are one group without clipping and launch the plain yunet_sgd_step_ex kernel, as before.

Not supported, and refused with the reason: Adam's amsgrad / maximize / foreach / capturable / fused flags,
paramwise_cfg.dcn_offset_lr_mult (no DCN layers here) and clipping norms other than 1, 2 and inf.

Frozen parameters (requires_grad=False when the group map is built) and every element that no group covers carry the byte
L.OPT_FROZEN in the map: the grouped kernels leave their parameter and state bytes untouched.  One such byte sends the
update through the grouped launch; with none, the paths are the ones above.
"""
import warnings

import torch

from . import _lib as L
from . import kernels as K


class DeviceScalar:
    """A float that stays in device memory until somebody asks for it (LoggerHook does, when it fires)."""

    def __init__(self, tensor, index=0):
        self.tensor, self.index = tensor, index

    def __float__(self):
        return float(self.tensor[self.index])

    def __format__(self, spec):
        return format(float(self), spec)


class _FusedOptimizer:
    """What the fused optimizers share: the groups and their device image, the flat state buffers, clipping, and the
    own / torch state-dict formats.  Subclasses name their state buffers (STATE), the group keys that go into the device
    table (_row) and launch the update (_update)."""

    STATE = ()

    def __init__(self, model, defaults, groups=None):
        self.model = model
        self.defaults = dict(defaults)
        if groups is None:
            groups = [dict(params=list(model.parameters()))]
        if not 1 <= len(groups) <= L.OPT_MAX_GROUPS:
            raise ValueError(f'{type(self).__name__}: {len(groups)} parameter groups; the device group map is one byte per '
                             f'element (1..{L.OPT_MAX_GROUPS} groups)')
        self.param_groups = []
        for g in groups:
            g = dict(self.defaults, **g)
            g.setdefault('initial_lr', g['lr'])
            self.param_groups.append(g)
        self._state = {k: None for k in self.STATE}
        self._steps = 0
        self._pending = None       # torch-format per-parameter state waiting for the engine's flat layout
        self._lr_dev, self._lr_val = None, None
        self._map, self._table, self._table_val = None, None, None
        self._map_sig, self._covered = None, None
        self._norm_scratch, self._norm_out = None, None
        self.grad_scale = 1.0      # multiplies the gradient inside the kernels (loss-scale removal)
        self.grad_clip = None      # dict(max_norm=, norm_type=2): set by OptimizerHook; clipping runs on the device

    # ---- the engine's flat layout ------------------------------------------------------------------------------------
    def _offset(self, eng, p):
        """Parameters are views of eng.params.data: a parameter's offset is the distance of its storage from the base."""
        off = (p.data_ptr() - eng.params.data.data_ptr()) // 4
        if off < 0 or off + p.numel() > eng.params.data.numel():
            raise RuntimeError(f'{type(self).__name__}: a parameter is not a view of the engine\'s flat buffer')
        return off

    def _bind(self):
        eng = self.model.engine
        if eng is None:
            raise RuntimeError(f'{type(self).__name__}.step() before the first forward_train: no gradients yet')
        n = eng.params.data.numel()
        if self._pending is not None:
            self._layout_pending(eng)
        for k, buf in self._state.items():
            if buf is not None and buf.numel() == n and buf.device != eng.device:
                # a state buffer restored from a checkpoint (map_location='cpu') or left behind by
                # model.to(other device): move it, keep the step count -- do NOT restart the state
                self._state[k] = buf.to(eng.device, torch.float32).contiguous()
                self._lr_dev, self._lr_val = None, None
        if any(buf is None or buf.numel() != n for buf in self._state.values()):
            for k in self._state:
                self._state[k] = torch.zeros_like(eng.params.data)
            self._lr_dev, self._lr_val = None, None
            self._steps = 0
        if self._lr_dev is None or self._lr_dev.device != eng.device:
            self._lr_dev = torch.zeros(1, device=eng.device)
            self._lr_val = None
        return eng

    def _bind_groups(self, eng):
        """The device image of the groups: the byte map (built once per layout) and the table (uploaded when a value in
        it changed)."""
        n = eng.params.data.numel()
        sig = self._frozen_ids()
        if self._map is None or self._map.numel() != n or self._map.device != eng.device or sig != self._map_sig:
            self._map = self._host_map(eng).to(eng.device)
            self._map_sig = sig
            self._table = torch.zeros(len(self.param_groups), L.OPT_ROW, device=eng.device, dtype=torch.float64)
            self._table_val = None
        rows = [self._row(g) for g in self.param_groups]
        if rows != self._table_val:
            self._table.copy_(torch.tensor(rows, dtype=torch.float64))
            self._table_val = rows

    def _frozen_ids(self):
        """id() of the parameters that take no update, as a frozenset; the map is rebuilt when it changes (a stage frozen
        or thawed between two steps).  A bound YuNet says which parameters its last step gave no gradient
        (YuNet.frozen_parameters: the flags as forward_train read them, so gradient and update agree, and the ~90 flags --
        20 us -- are read once per step, not twice); any other model: requires_grad is read here."""
        named = getattr(self.model, 'frozen_parameters', None)
        named = named() if named is not None else None
        if named is not None:
            return frozenset(id(p) for _, p in named)
        return frozenset(id(p) for g in self.param_groups for p in g['params'] if not p.requires_grad)

    def _host_map(self, eng):
        """The byte map on the host: a trainable parameter's elements carry its group, everything else -- parameters with
        requires_grad=False and elements of the flat buffer that no group covers -- L.OPT_FROZEN."""
        host = torch.full((eng.params.data.numel(),), L.OPT_FROZEN, dtype=torch.uint8)
        frozen = self._frozen_ids()
        for gi, g in enumerate(self.param_groups):
            for p in g['params']:
                if id(p) not in frozen:
                    off = self._offset(eng, p)
                    host[off:off + p.numel()] = gi
        return host

    def _clip_coef(self, eng):
        """Launch the norm kernel when clipping is on; returns the device float the update multiplies the gradient by."""
        if self.grad_clip is None:
            return None
        if self._norm_out is None or self._norm_out.device != eng.device:
            self._norm_scratch = K.grad_norm_scratch(eng.device)
            self._norm_out = torch.zeros(2, device=eng.device)
        K.grad_norm(eng.params.grad, self.grad_clip['max_norm'], self.grad_clip.get('norm_type', 2),
                    float(self.grad_scale), self._norm_scratch, self._norm_out)
        return self._norm_out[1:2]

    @property
    def grad_norm(self):
        """The last clipped step's gradient norm (of the unscaled gradient), still on the device; None without clipping."""
        return None if self._norm_out is None or self.grad_clip is None else DeviceScalar(self._norm_out, 0)

    def set_grad_clip(self, grad_clip):
        if grad_clip is None:
            self.grad_clip = None
            return
        cfg = dict(grad_clip)
        unknown = set(cfg) - {'max_norm', 'norm_type', 'error_if_nonfinite', 'foreach'}
        if unknown or 'max_norm' not in cfg:
            raise ValueError(f'grad_clip: expected max_norm [, norm_type], got {sorted(cfg)}')
        if cfg.get('error_if_nonfinite'):
            raise NotImplementedError('grad_clip: error_if_nonfinite needs the norm on the host every iteration')
        K.norm_type_code(cfg.get('norm_type', 2))           # refuse other norms here, with the reason
        self.grad_clip = dict(max_norm=float(cfg['max_norm']), norm_type=cfg.get('norm_type', 2))

    def _grouped(self, eng=None):
        """Several groups, clipping, or an element without update (a frozen parameter, or one no group covers)."""
        if len(self.param_groups) > 1 or self.grad_clip is not None:
            return True
        if eng is None:
            return False
        if self._frozen_ids():
            return True
        if self._covered is None:
            self._covered = sum(p.numel() for p in self.param_groups[0]['params'])
        return self._covered != eng.params.data.numel()

    def zero_grad(self, set_to_none=False):
        """No launch: the fused backward overwrites the flat gradient.  The engine is told that the buffer holds no total
        to keep, so with gradient accumulation on (YuNet.set_grad_accumulation) the next backward overwrites as well."""
        eng = getattr(self.model, 'engine', None)
        if eng is not None:
            eng.mark_grad_zeroed()
        return None

    @torch.no_grad()
    def step(self, closure=None):
        eng = self._bind()
        if getattr(eng, '_os_main', None) is not None or getattr(eng, '_os_side', None) is not None:
            # opt-in one-shot all-reduce: a peer that never arrived left NaN in the gradient and a status word on the
            # host.  Find out BEFORE the update is applied (and before an after_train_iter CheckpointHook could save the
            # poisoned parameters as "the last checkpoint"): wait for this step's collectives, then read the words
            # (costs the launch overlap of one step, only on this path)
            torch.cuda.current_stream(eng.device).synchronize()
            eng._check_oneshot()
        self._update(eng)
        self._steps += 1

    # ---- state dicts ---------------------------------------------------------------------------------------------
    def _params_in_order(self, n_ckpt_groups):
        """The parameter torch numbers i in a checkpoint: torch counts through the groups; an mmcv paramwise checkpoint
        has one group per parameter in model.parameters() order, a plain one a single group in that order."""
        if n_ckpt_groups == len(self.param_groups) and n_ckpt_groups > 1:
            return [p for g in self.param_groups for p in g['params']]
        return list(self.model.parameters())

    def _layout_pending(self, eng):
        """torch.optim per-parameter state -> the engine's flat layout."""
        flats = {k: torch.zeros_like(eng.params.data) for k in self.STATE}
        for p, st in self._pending:
            off = self._offset(eng, p)
            for k in self.STATE:
                flats[k][off:off + p.numel()].copy_(st[k])
        self._state = flats
        self._pending = None
        self._lr_dev, self._lr_val = None, None

    def state_dict(self):
        if self._pending is not None and self.model.engine is not None:
            self._layout_pending(self.model.engine)
        sd = dict(param_groups=[{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups],
                  steps=self._steps)
        for k, buf in self._state.items():
            sd[k] = None if buf is None else buf.clone()
        return sd

    def load_state_dict(self, sd):
        """Own format (state_dict above) or torch's ({'state': {i: {...}}, 'param_groups': [...]}, as stored in
        weights/yunet_*.pth): per-parameter state is laid out into the flat buffers in the order torch numbers the
        parameters in."""
        groups = sd.get('param_groups') or [{}]
        if len(groups) == len(self.param_groups):
            for g, src in zip(self.param_groups, groups):
                g.update({k: v for k, v in src.items() if k != 'params'})
        elif len(groups) == 1:
            self.param_groups[0].update({k: v for k, v in groups[0].items() if k != 'params'})
        else:
            warnings.warn(f'checkpoint has {len(groups)} parameter groups, the optimizer {len(self.param_groups)}: '
                          'keeping the configured hyper-parameters')
        self._lr_dev, self._lr_val, self._table_val = None, None, None
        self._pending = None
        first = self.STATE[0]
        if sd.get(first) is not None:
            for k in self.STATE:
                self._state[k] = sd[k].detach().clone().float().reshape(-1)
            self._steps = int(sd.get('steps', 1))
        elif isinstance(sd.get('state'), dict) and sd['state']:
            params = self._params_in_order(len(groups))
            pending, steps = [], 1
            for i, p in enumerate(params):
                st = sd['state'].get(i)
                if st is None or any(st.get(k) is None or st[k].numel() != p.numel() for k in self.STATE):
                    warnings.warn(f'optimizer state does not match the model: {self._what} restarts from zero')
                    pending = None
                    break
                pending.append((p, {k: st[k].detach().clone().float().reshape(-1) for k in self.STATE}))
                if 'step' in st:
                    steps = int(st['step'])
            if pending is not None:
                # The flat layout is defined by the engine, which a model binds lazily at its first
                # forward -- EpochBasedRunner.resume() (train_detector with resume_from / auto_resume)
                # loads the optimizer BEFORE any forward.  Keep the per-parameter state and lay it out
                # in _bind(), once the engine exists.
                self._pending = pending
                self._state = {k: None for k in self.STATE}
                self._steps = steps
                if self.model.engine is not None:
                    self._layout_pending(self.model.engine)
        else:
            warnings.warn(f'checkpoint carries no {self._what}: it restarts from zero')
            self._state = {k: None for k in self.STATE}
            self._steps = 0


class FusedSGD(_FusedOptimizer):
    STATE = ('momentum_buffer',)
    _what = 'SGD momentum'

    def __init__(self, model, lr=0.01, momentum=0.9, weight_decay=0.0, dampening=0, nesterov=False, groups=None):
        if nesterov and (momentum <= 0 or dampening != 0):        # torch/optim/sgd.py
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        super().__init__(model, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=dampening,
                                     nesterov=nesterov), groups)

    @property
    def _buf(self):
        return self._state['momentum_buffer']

    @_buf.setter
    def _buf(self, v):
        self._state['momentum_buffer'] = v

    @staticmethod
    def _row(g):
        return [float(g['lr']), float(g['weight_decay']), float(g['momentum']), 0.0]

    def _update(self, eng):
        g = self.param_groups[0]
        first = self._steps == 0
        if not self._grouped(eng):
            # the default path: one group, no clipping -- the plain kernel, lr in its own device word
            if self._lr_val != g['lr']:
                self._lr_dev.fill_(float(g['lr']))
                self._lr_val = g['lr']
            K.sgd_step(eng.params.data, eng.params.grad, self._buf, self._lr_dev, g['momentum'],
                       g['weight_decay'], float(self.grad_scale), first=first,
                       dampening=g.get('dampening', 0.0), nesterov=g.get('nesterov', False))
            return
        nesterov = bool(g.get('nesterov', False))
        if nesterov and any(x['momentum'] <= 0 for x in self.param_groups):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        self._bind_groups(eng)
        coef = self._clip_coef(eng)
        K.sgd_step_grouped(eng.params.data, eng.params.grad, self._buf, self._map, self._table,
                           float(self.grad_scale), coef, first=first, dampening=g.get('dampening', 0.0),
                           nesterov=nesterov)


class FusedAdam(_FusedOptimizer):
    """torch.optim.Adam (decoupled=False: weight decay joins the gradient) and AdamW (decoupled=True: p *= 1 - lr * wd)."""

    STATE = ('exp_avg', 'exp_avg_sq')
    _what = 'Adam state'

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, groups=None,
                 **flags):
        on = sorted(k for k, v in flags.items() if v)
        if set(flags) - {'amsgrad', 'maximize', 'foreach', 'capturable', 'differentiable', 'fused'}:
            raise TypeError(f'unexpected optimizer argument(s) {sorted(flags)}')
        if on:
            raise NotImplementedError(f'{"AdamW" if decoupled else "Adam"}: {on} not implemented by the fused update '
                                      '(it is the plain single-tensor form of torch.optim.Adam)')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or eps < 0 or lr < 0 or weight_decay < 0:
            raise ValueError(f'invalid Adam hyper-parameters: lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}')
        self.decoupled = bool(decoupled)
        super().__init__(model, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), groups)

    @staticmethod
    def _row(g):
        return [float(g['lr']), float(g['weight_decay']), float(g['betas'][0]), float(g['betas'][1])]

    def _update(self, eng):
        self._bind_groups(eng)
        coef = self._clip_coef(eng)
        K.adam_step_grouped(eng.params.data, eng.params.grad, self._state['exp_avg'], self._state['exp_avg_sq'],
                            self._map, self._table, self._steps + 1, eps=self.param_groups[0]['eps'],
                            decoupled=self.decoupled, grad_scale=float(self.grad_scale), clip_coef=coef)


# ---- mmcv 1.x DefaultOptimizerConstructor ---------------------------------------------------------------------------

PARAMWISE_KEYS = ('custom_keys', 'bias_lr_mult', 'bias_decay_mult', 'norm_decay_mult', 'dwconv_decay_mult',
                  'dcn_offset_lr_mult', 'bypass_duplicate')
_NORMS = (torch.nn.modules.batchnorm._BatchNorm, torch.nn.modules.instancenorm._InstanceNorm, torch.nn.GroupNorm,
          torch.nn.LayerNorm)


def paramwise_options(model, base_lr, base_wd, paramwise_cfg):
    """[(dotted name, parameter, lr, weight_decay | None)] in model.parameters() order, by the rules of mmcv's
    DefaultOptimizerConstructor.add_params.  base_wd None: the optimizer config has no weight_decay."""
    cfg = dict(paramwise_cfg or {})
    unknown = set(cfg) - set(PARAMWISE_KEYS)
    if unknown:
        raise ValueError(f'paramwise_cfg: unknown option(s) {sorted(unknown)}; known are {PARAMWISE_KEYS}')
    if 'dcn_offset_lr_mult' in cfg:
        raise NotImplementedError('paramwise_cfg.dcn_offset_lr_mult: this model has no deformable convolutions')
    custom = cfg.get('custom_keys', {})
    if not isinstance(custom, dict):
        raise TypeError(f'If specified, custom_keys must be a dict, but got {type(custom)}')
    if base_wd is None:
        for key, v in custom.items():
            if 'decay_mult' in v:
                raise ValueError('base_wd should not be None')
        if any(k in cfg for k in ('bias_decay_mult', 'norm_decay_mult', 'dwconv_decay_mult')):
            raise ValueError('base_wd should not be None')
    keys = sorted(sorted(custom.keys()), key=len, reverse=True)
    bias_lr_mult = cfg.get('bias_lr_mult', 1.)
    bias_decay_mult = cfg.get('bias_decay_mult', 1.)
    norm_decay_mult = cfg.get('norm_decay_mult', 1.)
    dwconv_decay_mult = cfg.get('dwconv_decay_mult', 1.)
    out = []
    for prefix, module in model.named_modules():
        is_norm = isinstance(module, _NORMS)
        is_dwconv = isinstance(module, torch.nn.Conv2d) and module.in_channels == module.groups
        for name, p in module.named_parameters(recurse=False):
            full = f'{prefix}.{name}' if prefix else name
            lr, wd = base_lr, base_wd
            key = next((k for k in keys if k in full), None)
            if key is not None:
                lr = base_lr * custom[key].get('lr_mult', 1.)
                if base_wd is not None:
                    wd = base_wd * custom[key].get('decay_mult', 1.)
            else:
                if name == 'bias' and not is_norm:
                    lr = base_lr * bias_lr_mult
                if base_wd is not None:
                    if is_norm:
                        wd = base_wd * norm_decay_mult
                    elif is_dwconv:
                        wd = base_wd * dwconv_decay_mult
                    elif name == 'bias':
                        wd = base_wd * bias_decay_mult
            out.append((full, p, lr, wd))
    return out


def build_param_groups(model, base_lr, base_wd, paramwise_cfg, default_wd=0.0):
    """One group per distinct (lr, weight_decay), in order of first appearance; each carries its parameters and their
    dotted names."""
    groups = {}
    for full, p, lr, wd in paramwise_options(model, base_lr, base_wd, paramwise_cfg):
        wd = default_wd if wd is None else wd
        g = groups.setdefault((lr, wd), dict(lr=lr, weight_decay=wd, params=[], param_names=[]))
        g['params'].append(p)
        g['param_names'].append(full)
    return list(groups.values())


def build_optimizer(model, cfg):
    """optimizer = dict(type='SGD' | 'Adam' | 'AdamW', ..., paramwise_cfg=dict(...)) -> FusedSGD / FusedAdam
    (mmdet/apis/train.py:167 -> mmcv build_optimizer)."""
    cfg = dict(cfg)
    t = cfg.pop('type')
    paramwise = cfg.pop('paramwise_cfg', None)
    constructor = cfg.pop('constructor', 'DefaultOptimizerConstructor')
    if constructor != 'DefaultOptimizerConstructor':
        raise NotImplementedError(f'optimizer constructor {constructor!r}: only mmcv\'s DefaultOptimizerConstructor')
    if t not in ('SGD', 'Adam', 'AdamW'):
        raise NotImplementedError(f'optimizer type {t}: the fused optimizers are SGD, Adam and AdamW')
    target = model.module if hasattr(model, 'module') else model
    kw = dict(cfg)
    if t == 'AdamW':
        kw.setdefault('weight_decay', 1e-2)                 # torch.optim.AdamW's default
    if paramwise:
        default_lr = 0.01 if t == 'SGD' else 1e-3
        kw['groups'] = build_param_groups(target, cfg.get('lr', default_lr), cfg.get('weight_decay'), paramwise,
                                          default_wd=kw.get('weight_decay', 0.0))
    if t == 'SGD':
        return FusedSGD(target, **kw)
    return FusedAdam(target, decoupled=(t == 'AdamW'), **kw)
