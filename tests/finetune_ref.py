"""The yardstick of tests/test_finetune_gpu.py: oracle/yunet_oracle.py composed with a `training` flag per part, in fp32
(losses, assignment, gradients, BatchNorm buffers) and in fp64 (the gradient of sum(flat * dflat), against which both fp32
implementations are measured, as in tests/test_engine_gpu.py::test_forward_train_vs_oracle).  CPU only."""
import functools

import torch
import torch.nn.functional as F

import helpers as Hh
import yunet_oracle as O


def conv_stack(img, sd, arch, flag):
    """flag(BatchNorm name) -> bool.  backbone_forward / neck_forward / head_forward take one flag each; a backbone whose
    stages differ (frozen_stages) is the same composition of O.conv_dp_unit and O._bn_relu stage by stage."""
    st = arch['stage_channels']
    stage_flags = [flag(f'backbone.model{i}.conv2.bn') for i in range(len(st))]
    if len(set(stage_flags)) == 1:
        feats = O.backbone_forward(img, sd, arch, stage_flags[0])
    else:
        x = F.conv2d(img, sd['backbone.model0.conv1.weight'], sd['backbone.model0.conv1.bias'], stride=2, padding=1)
        x = O._bn_relu(x, sd, 'backbone.model0.bn1', stage_flags[0])
        x = O.conv_dp_unit(x, sd, 'backbone.model0.conv2', True, stage_flags[0])
        feats = []
        for i in range(len(st)):
            if i > 0:
                x = O.conv_dp_unit(x, sd, f'backbone.model{i}.conv1', True, stage_flags[i])
                x = O.conv_dp_unit(x, sd, f'backbone.model{i}.conv2', True, stage_flags[i])
            if i in arch['out_idx']:
                feats.append(x)
            if i in arch['downsample_idx']:
                x = F.max_pool2d(x, 2)
    feats = O.neck_forward(feats, sd, arch, flag('neck.lateral_convs.0.bn'))
    return O.head_forward(feats, sd, arch, flag('bbox_head.multi_level_share_convs.0.0.bn'))


def _leaves(sd, dtype):
    work = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    work = {k: v.clone() for k, v in work.items()}          # F.batch_norm updates the running buffers in place
    leaf = {k: work[k].clone().requires_grad_(True) for k in O.param_keys(work)}
    work.update(leaf)
    return work, leaf


def step_fp32(batch, sd, arch, flag):
    """-> (losses, gradients, aux, state after the step): one oracle training step with the flags."""
    work, leaf = _leaves(sd, torch.float32)
    maps = conv_stack(batch['img'], work, arch, flag)
    flat = O.flatten_preds(*maps)
    sizes = [tuple(c.shape[2:]) for c in maps[0]]
    losses, aux = O.loss_step(flat, batch['gt_bboxes'], batch['gt_labels'], batch['gt_keypointss'], sizes, arch)
    sum(losses.values()).backward()
    aux['flat'], aux['sizes'] = flat.detach(), sizes
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    after = {k: v.detach() for k, v in work.items()}
    return {k: float(v.detach()) for k, v in losses.items()}, grads, aux, after


def grads_fp64(batch, sd, arch, flag, dflat):
    work, leaf = _leaves(sd, torch.float64)
    flat = O.flatten_preds(*conv_stack(batch['img'].double(), work, arch, flag))
    (flat * dflat.double()).sum().backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}


def near_tie(aux, batch):
    return [i for i in range(aux['flat'].shape[0]) if Hh.image_near_tie(aux['flat'][i], batch['gt_bboxes'][i], aux['sizes'])]


@functools.lru_cache(None)
def warm_state(kind, seed):
    """Fresh weights whose BatchNorm buffers are those ONE train-mode step (batch 2, 64 x 64) leaves behind: running
    statistics that differ from the batch's, so a layer normalising with the wrong ones shows."""
    import yunet_amd.synthetic as S
    arch = O.yunet_arch(kind)
    sd = O.init_state(arch, seed=seed)
    _, _, _, after = step_fp32(S.make_batch(2, 64, 64, 900 + seed), sd, arch, lambda name: True)
    for k, v in after.items():
        if k.endswith(('running_mean', 'running_var', 'num_batches_tracked')):
            sd[k] = v.clone()
    return sd
