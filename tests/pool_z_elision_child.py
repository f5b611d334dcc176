"""Child process of tests/test_pool_z_elision_gpu.py: one full training step of YuNet_n (N = 4, 128 x 128) per mode, under
the YUNET_KEEP_POOL_Z the parent set -- the switch is read when a plan is built and the C options once per process.

    python tests/pool_z_elision_child.py OUT.pt

Writes {mode: {losses, log, grad, params, momentum, running_mean, running_var, num_batches_tracked, elided}}."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]
import torch                            # noqa: E402
import yunet_amd                        # noqa: E402
import yunet_amd.synthetic as S         # noqa: E402
import yunet_oracle as O                # noqa: E402
from yunet_amd.optim import FusedSGD    # noqa: E402

MODES = (('fp32', 'fp32', False), ('deterministic', 'fp32', True), ('bf16', 'bf16', False))


def step(precision, det):
    dev = torch.device('cuda', 0)
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'yunet_n.py'))
    model = yunet_amd.build_detector(cfg.model)
    sd = O.init_state(O.yunet_arch('n'), seed=3)
    model.load_state_dict(sd, strict=True)
    model.to(dev).train()
    model.set_precision(precision)
    model.set_deterministic(det)
    opt = FusedSGD(model, lr=1e-2, momentum=0.9, weight_decay=5e-4)
    b = S.make_batch(4, 128, 128, 4321)
    out = model.train_step(S.to_device(b, dev), opt)
    opt.zero_grad()
    out['loss'].backward()
    eng = model.engine
    grad = eng.params.grad.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    plan = eng.plan
    assert (plan.n, plan.h, plan.w) == (4, 128, 128)
    fp = eng.params
    mom = opt._state.get('momentum_buffer')
    res = dict(losses=plan.losses.detach().cpu().clone(),          # cls, bbox, obj, kps, total (the finalize kernel's record)
               log=[float(out['log_vars'][k]) for k in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps', 'loss')],
               grad=grad.cpu(), params=fp.data.detach().cpu().clone(), momentum=mom.detach().cpu().clone(),
               running_mean=fp.running_mean.cpu().clone(), running_var=fp.running_var.cpu().clone(),
               num_batches_tracked=fp.num_batches_tracked.cpu().clone(), elided=len(plan.elided_z))
    return res


if __name__ == '__main__':
    torch.save({name: step(p, d) for name, p, d in MODES}, sys.argv[1])
