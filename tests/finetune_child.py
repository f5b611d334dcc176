"""Child process of tests/test_finetune_gpu.py: a few SGD steps at deterministic='fast' with the first backbone stages frozen,
from a golden fixture's weights; the tensors of the reproducibility contract (tests/deterministic_child.py) go to one .npz.

    finetune_child.py KIND FIXTURE N SIZE STEPS FROZEN_STAGES|bn OUT [LR]        (bn: every BatchNorm in eval(), every parameter trains)
"""
import sys

import numpy as np
import torch

import deterministic_child as DC


def main(argv):
    from yunet_amd.optim import FusedSGD
    kind, fixture, n, size, steps, what, out = argv[0], argv[1], int(argv[2]), int(argv[3]), int(argv[4]), argv[5], argv[6]
    m = DC.build(kind, fixture, deterministic=False)
    m.set_deterministic('fast')
    if what == 'bn':
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.eval()
    else:
        m.backbone.frozen_stages = int(what)
        m.train()                                    # (the override applies frozen_stages to the modules' flags)
    opt = FusedSGD(m, lr=float(argv[7]) if len(argv) > 7 else 0.01, momentum=0.9, weight_decay=5e-4)
    losses = []
    for it in range(steps):
        DC.step(m, opt, n, size, it)
        losses.append(m.engine.plan.losses.cpu().numpy().copy())
    plan = m.engine.plan
    assert plan.det and plan.frozen_bn and bool(plan.frozen_params) == (what != 'bn')
    frozen = sum(p.numel() for p in m.parameters() if not p.requires_grad)
    np.savez(out, frozen_elements=frozen, **DC.contract(m, opt, losses))


if __name__ == '__main__':
    main(sys.argv[1:])
