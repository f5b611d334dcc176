"""Child process of tests/test_deterministic_gpu.py: a few deterministic (or default) SGD steps from a golden fixture's
weights, every tensor of the reproducibility contract dumped to one .npz.

    deterministic_child.py KIND FIXTURE N SIZE STEPS OUT [--default]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def build(kind, fixture, deterministic=True, dev='cuda'):
    import helpers as Hh
    import yunet_amd
    g = Hh.load_golden(fixture)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w:')}, strict=True)
    if deterministic:
        m.set_deterministic(True)
    m.to(dev).train()
    return m


def step(m, opt, n, size, it, dev='cuda'):
    import yunet_amd.synthetic as S
    b = S.to_device(S.make_batch(n, size, size, S.batch_seed(0, it)), dev)
    out = m.train_step(b, opt)
    opt.zero_grad()
    out['loss'].backward()
    opt.step()
    return out


def contract(m, opt, losses):
    """The tensors the deterministic mode promises to reproduce, as numpy arrays."""
    torch.cuda.synchronize()
    fp = m.engine.params
    return dict(losses=np.stack(losses), grad=fp.grad.cpu().numpy(), params=fp.data.cpu().numpy(),
                momentum=opt._buf.cpu().numpy(), running_mean=fp.running_mean.cpu().numpy(),
                running_var=fp.running_var.cpu().numpy(), num_batches_tracked=fp.num_batches_tracked.cpu().numpy())


def main(argv):
    from yunet_amd.optim import FusedSGD
    kind, fixture, n, size, steps, out = argv[0], argv[1], int(argv[2]), int(argv[3]), int(argv[4]), argv[5]
    m = build(kind, fixture, deterministic='--default' not in argv)
    opt = FusedSGD(m, lr=0.01, momentum=0.9, weight_decay=5e-4)
    losses = []
    for it in range(steps):
        step(m, opt, n, size, it)
        losses.append(m.engine.plan.losses.cpu().numpy().copy())
    np.savez(out, **contract(m, opt, losses))


if __name__ == '__main__':
    main(sys.argv[1:])
