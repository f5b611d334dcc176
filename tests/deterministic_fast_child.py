"""Child process of tests/test_deterministic_fast_gpu.py: a few SGD steps at the fast deterministic level (or in the default
mode) from a golden fixture's weights, every tensor of the reproducibility contract dumped to one .npz; `grad1`: the flat
gradient after the first step.

    deterministic_fast_child.py KIND FIXTURE N SIZE STEPS OUT [--default]
"""
import sys

import numpy as np

import deterministic_child as DC


def main(argv):
    from yunet_amd.optim import FusedSGD
    kind, fixture, n, size, steps, out = argv[0], argv[1], int(argv[2]), int(argv[3]), int(argv[4]), argv[5]
    m = DC.build(kind, fixture, deterministic=False)
    if '--default' not in argv:
        m.set_deterministic('fast')          # (plans are built by the first step: keyed 'det-fast')
    opt = FusedSGD(m, lr=0.01, momentum=0.9, weight_decay=5e-4)
    losses, grad1 = [], None
    for it in range(steps):
        DC.step(m, opt, n, size, it)
        losses.append(m.engine.plan.losses.cpu().numpy().copy())
        if it == 0:
            grad1 = m.engine.params.grad.cpu().numpy().copy()
    key = next(reversed(m.engine.plans))
    np.savez(out, grad1=grad1, plan_key=np.array([str(v) for v in key]), **DC.contract(m, opt, losses))


if __name__ == '__main__':
    main(sys.argv[1:])
