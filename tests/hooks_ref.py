"""Test-side restatement of the custom hooks' semantics (mmdet/core/hook/ema.py and
yunet_sample_size_statistics_hook.py), written from their formulas -- not a copy of either implementation.

EMA:   every `interval` iterations (it + 1 divisible), for every floating-point entry,
           ema = ema * (1 - m) + m * value,   m = momentum_fun(it) or the constant;
       Exp:    m(x) = (1 - momentum) * exp(-(1 + x) / total_iter) + momentum
       Linear: m(x) = min(momentum ** interval, (1 + x) / (warm_up + x))
       at every epoch end and every epoch start: value <-> ema for every entry (integer ones included).
Sizes: per box (w, h) = (int(x2 - x1), int(y2 - y1)) of the fp32 differences, counted under the key "w,h" in
       first-seen order (iteration, image, box); an image without boxes counts as Noimg.
"""
import math

import torch


def momentum_fun(kind, momentum, interval=1, total_iter=2000, warm_up=100):
    if kind == 'ExpMomentumEMAHook':
        return lambda x: (1 - momentum) * math.exp(-(1 + x) / total_iter) + momentum
    if kind == 'LinearMomentumEMAHook':
        return lambda x: min(momentum ** interval, (1 + x) / (warm_up + x))
    raise ValueError(kind)


def hook_momentum_fun(cfg):
    """momentum_fun of a custom_hooks entry dict(type=..., momentum=..., interval=..., total_iter | warm_up)."""
    kw = {k: cfg[k] for k in ('interval', 'total_iter', 'warm_up') if k in cfg}
    return momentum_fun(cfg['type'], cfg.get('momentum', 0.0002), **kw)


def ema_name(key):
    return 'ema_' + key.replace('.', '_')


class EMAReplay:
    """EMA state over `entries` (key -> tensor, cloned), replayed with eager torch."""

    def __init__(self, entries, interval, mfun):
        self.ema = {k: v.detach().clone() for k, v in entries.items()}
        self.interval, self.mfun = interval, mfun

    def step(self, it, live):
        if (it + 1) % self.interval != 0:
            return
        m = self.mfun(it)
        for k, e in self.ema.items():
            if e.dtype.is_floating_point:
                e.mul_(1 - m).add_(live[k], alpha=m)

    def swap(self, live):
        """live (key -> tensor, modified in place) <-> ema."""
        for k, e in self.ema.items():
            t = live[k].clone()
            live[k].copy_(e)
            e.copy_(t)


def size_statistics(batches):
    """batches: [(iteration, [per-image fp32 tensor [g, 4]])] -> (data dict in first-seen order, total, noimg)."""
    data, total, noimg = {}, 0, 0
    for _, images in sorted(batches, key=lambda b: b[0]):
        for boxes in images:
            if boxes.shape[0] == 0:
                noimg += 1
                continue
            d = (boxes[:, 2:4] - boxes[:, 0:2]).cpu()
            for w, h in d.tolist():
                tag = f'{math.trunc(w)},{math.trunc(h)}'
                data[tag] = data.get(tag, 0) + 1
                total += 1
    return data, total, noimg


def padded_to_lists(padded, counts):
    """GTList.padded [N, Gmax, 4] + counts [N] -> the per-image [g, 4] tensors (on the CPU)."""
    p, c = padded.detach().cpu(), counts.detach().cpu()
    return [p[n, :int(c[n])] for n in range(p.shape[0])]
