"""The bound the optimizer tests share (test_optim_kernels_gpu.py, test_optim_surface_gpu.py)."""
import math

import torch


def ulp32(x):
    """Spacing of fp32 at |x|."""
    x = abs(float(x))
    return 2.0 ** -149 if x < 2.0 ** -126 else 2.0 ** (math.floor(math.log2(x)) - 23)


def check(what, dev, t32, ref64):
    """|dev - ref64| <= max(4 |t32 - ref64|, 1 ulp) with the figures printed first."""
    dev, t32, ref64 = (torch.as_tensor(v).double().cpu().reshape(-1) for v in (dev, t32, ref64))
    e_dev = float((dev - ref64).abs().max())
    e_t32 = float((t32 - ref64).abs().max())
    bound = max(4.0 * e_t32, ulp32(ref64.abs().max()))
    print(f'{what}: device {e_dev:.3e}  torch-fp32 {e_t32:.3e}  bound {bound:.3e}')
    assert torch.isfinite(dev).all()
    assert e_dev <= bound, (what, e_dev, e_t32, bound)
