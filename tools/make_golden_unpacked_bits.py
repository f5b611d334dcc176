#!/usr/bin/env python
"""The kernels built without packed fp32 arithmetic (csrc/Makefile: UNPACKED), one launch per instance and code path, and
SHA-256 of what they write.

    YUNET_HIP_LIB=<library of the commit before the change> python tools/make_golden_unpacked_bits.py [OUT.json]

writes tests/golden/unpacked_parent_bits.json (or OUT.json); tests/test_unpacked_bits_gpu.py runs the same cases on the library of the
tree and compares.  Unpacking changes which instruction does an operation, not the operation: every element goes through
the same IEEE fma / add / mul, so dx and the reduced weight-gradient row are the same bytes.  The producer's BN-backward
sums are added with fp64 atomics in launch order and are compared with a tolerance instead.

Inputs come from a seeded CPU generator through elementwise operations only (no host-side reduction, whose summation
order depends on the thread count): the BatchNorm sums handed to the kernel are chosen per channel, not measured.

dp_bwd16s (conv_bwd16.hip), fp32 and bf16 storage: N = 1 at 32 x 64 (one strip pair per image, whole strips) and N = 3 at
40 x 72 (ragged last strip, several bands), each with a full-size dy and with a pooled dy + window positions.
"""
import hashlib
import json
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'unpacked_parent_bits.json')
DEV = 'cuda'

# name -> (cin, cout, (N, H, W), pooled dy, storage type)
CASES = {}
for _dt in ('f32', 'bf16'):
    for _shape in ((1, 32, 64), (3, 40, 72)):
        for _pool in (False, True):
            CASES[f'bwd16s-{_dt}-{_shape[0]}x{_shape[1]}x{_shape[2]}-{"pooled" if _pool else "plain"}'] = (16, 16, _shape, _pool, _dt)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def chosen_sums(g, c, count, mean_scale, mean_shift, var_lo, var_hi):
    """fp64 [2c] forward sums of a BatchNorm with per-channel mean and variance drawn from g."""
    mean = (torch.randn(c, generator=g) * mean_scale + mean_shift).double()
    var = (torch.rand(c, generator=g) * (var_hi - var_lo) + var_lo).double()
    return torch.cat([count * mean, count * (var + mean * mean)]).contiguous()


def run_case(name):
    """-> {'dx': sha, 'wgrad': sha, 'bstats': [float.hex ...]} of one yunet_dp_bwd launch."""
    import yunet_amd.kernels as k
    cin, cout, (n, h, w), pooled, dt = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    cnt = n * h * w
    x = torch.randn(n, h, w, cin, generator=g) * 2 + 0.5
    w_pw = torch.randn(cout, cin, generator=g) * (2.0 / (cin + cout)) ** 0.5
    b_pw = torch.randn(cout, generator=g) * 0.1
    w_dw = torch.randn(cout, 9, generator=g) * 0.3
    b_dw = torch.randn(cout, generator=g) * 0.1
    gi, bi = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.2
    go, bo = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    in_sums = chosen_sums(g, cin, cnt, 0.1, 0.5, 3.2, 4.8)
    out_sums = chosen_sums(g, cout, cnt, 0.2, 0.0, 1.0, 2.0)
    out_bsums = (torch.randn(2 * cout, generator=g) * 0.01 * cnt).double()
    if pooled:
        dy = torch.randn(n, h // 2, w // 2, cout, generator=g)
        idx = torch.randint(0, 4, (n, h // 2, w // 2, cout), generator=g, dtype=torch.uint8).to(DEV)
    else:
        dy = torch.randn(n, h, w, cout, generator=g) * (torch.rand(n, h, w, cout, generator=g) > 0.5)      # ReLU-masked
        idx = None
    act = torch.bfloat16 if dt == 'bf16' else torch.float32
    xg = x.to(act).to(DEV)
    zg = torch.zeros(n, h, w, cout, dtype=act, device=DEV)          # not read: dp_bwd16s recomputes z from x
    in_bn = k.BN(in_sums.to(DEV), gi.to(DEV), bi.to(DEV), cnt, bstats=torch.zeros(2 * cin, dtype=torch.float64, device=DEV))
    out_bn = k.BN(out_sums.to(DEV), go.to(DEV), bo.to(DEV), cnt, bstats=out_bsums.to(DEV))
    dx = torch.full((n, h, w, cin), float('nan'), device=DEV)
    dx, dw1, db1, dw2, db2 = k.dp_bwd(xg, w_pw.to(DEV), b_pw.to(DEV), w_dw.to(DEV), b_dw.to(DEV), zg, dy.to(DEV), in_bn, out_bn,
                                      dx=dx, pool_idx=idx)
    torch.cuda.synchronize()
    wgrad = torch.cat([t.reshape(-1) for t in (dw1, db1, dw2, db2)])
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(wgrad).all()), name
    return {'dx': sha(dx), 'wgrad': sha(wgrad), 'bstats': [float(v).hex() for v in in_bn.bstats.cpu()]}


def main():
    sys.path.insert(0, ROOT)
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    out = {'cases': {name: run_case(name) for name in CASES}}
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote {path}: {len(CASES)} cases')


if __name__ == '__main__':
    main()
