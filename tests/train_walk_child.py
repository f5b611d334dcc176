"""Child process of tests/test_train_walk_gpu.py: one case of train_walk.CASES under the environment the parent set
(YUNET_KEEP_POOL_Z is read when a plan is built).

    python tests/train_walk_child.py CASE OUT.pt

Writes {worst: {node: worst error / bound}, grad: the flat gradient's bytes}."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]
import torch                            # noqa: E402
import test_train_walk_gpu as G         # noqa: E402

if __name__ == '__main__':
    worst, grad, _ = G.run_case(sys.argv[1])
    torch.save(dict(worst=worst, grad=grad), sys.argv[2])
