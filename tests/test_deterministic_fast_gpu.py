"""-m gpu: the fast deterministic level (YUNET_DET_FAST in YunetBN.det_rows) -- the kernels of the
default mode in their order-fixed DET forms.  Every kernel through the C ABI, launched on the same inputs in its default
form (det_rows = 0, slots = 1) and in its fast form: the outputs that are not sums are the same bytes, the sums go to rows
1 .. grid and fold to the default form's sums within fp64 rounding, repeated launches give the same bytes, and everything
matches an fp64 evaluation at the tolerances of the default-mode tests of the same instances.  Then whole steps in fresh
processes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yunet_amd._lib as L
from yunet_amd.engine import DET_ROWS as R
import helpers as Hh
from test_deterministic_gpu import CONTRACT, five_times
from test_kernels_gpu import bn_ref, mk_unit, nchw, nhwc, rel_err, stats_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = R | L.DET_FAST
TOL_FWD, TOL_BWD = 2e-5, 5e-5           # tests/test_kernels_gpu.py: test_dp_fwd / test_fused_pooling, test_dp_bwd
# folded sums against the default form's: both add the same fp32 per-lane partials in another fp64 order; fp64 rounding over
# at most 2^22 addends stays below 1e-12 of sum |addend|, and the largest entry (a sum of squares) is its own sum |addend|
TOL_SUMS = 1e-10


def K():
    import yunet_amd.kernels as k
    return k


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.uint8 if t.dtype == torch.uint8 else (np.uint32 if t.dtype == torch.float32 else np.uint64))


def same_bytes(a, b):
    return np.array_equal(bits(a), bits(b))


def sums_err(got, want):
    return float((got.double().cpu() - want.double().cpu()).abs().max() / want.double().cpu().abs().max())


def bn_pair(k, c, row0, gamma, beta, count, bstats=None):
    """The same BatchNorm twice: default form (one [2c] block per kind) and fast form ([1 + R, 2c] blocks, R | YUNET_DET_FAST).
    row0: the forward sums readers take (None: zeros, this launch produces them); bstats: None (no backward block), 'zero'
    (this launch produces them) or the [2c] sums readers take."""
    gamma, beta = gamma.float().to(DEV), beta.float().to(DEV)

    def block(rows, v):
        t = torch.zeros(rows, 2 * c, dtype=torch.float64, device=DEV)
        if v is not None and not isinstance(v, str):
            t[0] = v.to(DEV)
        return t
    dflt = k.BN(block(1, row0).view(-1), gamma, beta, count, bstats=None if bstats is None else block(1, bstats).view(-1))
    fast = k.BN(block(1 + R, row0), gamma, beta, count, bstats=None if bstats is None else block(1 + R, bstats), det_rows=FAST)
    return dflt, fast


def check_rows(block, grid):
    """Before the fold: row 0 is zero (the fold writes it), workgroup 0 -- which always has work -- has written row 1, and no
    row beyond the grid is touched.  (A workgroup of a wave-streaming kernel whose waves got no strip adds zeros to its
    row.)  Returns the number of rows that hold something."""
    block = block.cpu()
    assert not bool(block[0].any()), 'row 0 is written by the fold only'
    used = torch.nonzero(block[1:].abs().sum(1) > 0).flatten()
    assert used.numel() >= 1 and int(used[0]) == 0 and int(used[-1]) < grid, (used.tolist()[-4:], grid)
    return int(used.numel())


# ------------------------------------------------------------------------------------------------------------ forward
def fwd_case(cin, cout, n, h, w, pool=False, seed=0):
    k = K()
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + h + w + n + seed)
    x = torch.randn(n, cin, h, w, generator=g) * 3 + 1.5
    w_pw, b_pw, w_dw, b_dw = mk_unit(cin, cout, g)
    gamma, beta = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.2
    go, bo = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    if pool:
        go[1], go[cout - 3], go[5] = -go[1], -0.7, 0.0          # falling BN: the minimum wins; constant: position 0
    a = F.relu(bn_ref(x.double(), gamma.double(), beta.double())[0])
    zr = F.conv2d(F.conv2d(a, w_pw.double(), b_pw.double()), w_dw.double(), b_dw.double(), padding=1, groups=cout)
    xg = nhwc(x).to(DEV)
    in_d, in_f = bn_pair(k, cin, stats_of(xg), gamma, beta, n * h * w)
    out_d, out_f = bn_pair(k, cout, None, go, bo, n * h * w)
    ws = (w_pw.to(DEV).view(cout, cin).contiguous(), b_pw.to(DEV), w_dw.to(DEV).view(cout, 9).contiguous(), b_dw.to(DEV))

    def launch(in_bn, out_bn, with_z=True):
        z = torch.full((n, h, w, cout), -777.0, device=DEV)
        d = k._dp_desc(xg, *ws, z, in_bn, out_bn)
        keep = [z]
        if pool:
            keep += [torch.full((n, h // 2, w // 2, cout), 555.0, device=DEV),
                     torch.full((n, h // 2, w // 2, cout), 99, device=DEV, dtype=torch.uint8)]
            d.pool_out, d.pool_idx = keep[1].data_ptr(), keep[2].data_ptr()
        if not with_z:
            d.z = None
        L.check(L.load().yunet_dp_fwd(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'yunet_dp_fwd')
        return keep
    ref = launch(in_d, out_d)
    torch.cuda.synchronize()

    def run(with_z=True):
        out_f.stats.zero_()
        outs = launch(in_f, out_f, with_z)
        rows = out_f.stats.clone()
        return (*outs, rows, k.bn_fold(out_f.stats).clone())
    res = five_times(run)                                                              # 4. repeat launches
    *outs, rows, folded = res
    for name, got, want in zip(('z', 'pool_out', 'pool_idx'), outs, ref):
        assert same_bytes(got, want), (name, n, h, w)                                  # 1. non-sum outputs
    # 2. row structure; the streaming forward kernels launch at most three workgroups per compute unit
    G = check_rows(rows, min(R, 3 * torch.cuda.get_device_properties(0).multi_processor_count))
    e = sums_err(folded, out_d.stats)
    print(f'[fwd {cin}->{cout} {(n, h, w)} pool={pool}] rows in use {G}, folded sums vs default {e:.3g}')
    assert e <= TOL_SUMS, (e, n, h, w)                                                 # 3. folded sums
    assert rel_err(nchw(outs[0].cpu()), zr) < TOL_FWD, (n, h, w)                       # 5. fp64 reference
    assert rel_err(folded, stats_of(nhwc(zr))) < TOL_FWD, (n, h, w)
    if pool:
        act = F.relu(bn_ref(zr, go.double(), bo.double())[0])
        ref_pool = F.max_pool2d(act, 2)
        got_pool = F.relu((nchw(outs[1].cpu()).double() - zr.mean(dim=(0, 2, 3), keepdim=True))
                          / torch.sqrt(zr.var(dim=(0, 2, 3), unbiased=False, keepdim=True) + 1e-5)
                          * go.double().view(1, -1, 1, 1) + bo.double().view(1, -1, 1, 1))
        assert rel_err(got_pool, ref_pool) < TOL_FWD, (n, h, w)
    return run, outs, rows, folded


@pytest.mark.parametrize('n,h,w', [(2, 16, 32), (48, 80, 80), (70, 20, 20), (6, 10, 10)])
def test_dp_fwd64s_fast(n, h, w):
    """dp_fwd64s_kernel<false, DET>: strips of 14 + 14 + 4 columns; several bands per wave; the 20 x 20 and 10 x 10 levels."""
    fwd_case(64, 64, n, h, w)


def test_dp_fwd64s_pooled_fast():
    """dp_fwd64s_kernel<true, DET>."""
    fwd_case(64, 64, 3, 40, 48, pool=True)


@pytest.mark.parametrize('cout,n,h,w', [(16, 2, 16, 32), (16, 44, 160, 160), (64, 2, 16, 32), (64, 48, 80, 80)])
def test_dp_fwd16s_fast(cout, n, h, w):
    """dp_fwd16s_kernel<16, false, DET> and <64, false, DET>."""
    fwd_case(16, cout, n, h, w)


def test_dp_fwd16s_pooled_fast_with_and_without_z():
    """dp_fwd16s_kernel<16, true, DET>, both bodies: with a null z the winners, positions and rows are the same bytes."""
    run, outs, rows, folded = fwd_case(16, 16, 2, 64, 96, pool=True)
    guard, pooled, idx, rows2, folded2 = run(with_z=False)
    torch.cuda.synchronize()
    assert bool((guard == -777.0).all()), 'the run with a null z wrote a full-size output'
    assert same_bytes(pooled, outs[1]) and same_bytes(idx, outs[2])
    assert same_bytes(rows2, rows) and same_bytes(folded2, folded)


# ----------------------------------------------------------------------------------------------------------- backward
def bwd_case(cin, cout, n, h, w, pooldy=False):
    k = K()
    g = torch.Generator().manual_seed(11 + cin * 100 + cout + n + h + w)
    x = (torch.randn(n, cin, h, w, generator=g) * 2 + 0.5).double()
    w_pw, b_pw, w_dw, b_dw = [t.double().requires_grad_(True) for t in mk_unit(cin, cout, g)]
    gi, bi = (torch.rand(cin, generator=g) + 0.5).double(), (torch.randn(cin, generator=g) * .2).double()
    go, bo = (torch.rand(cout, generator=g) + 0.5).double(), (torch.randn(cout, generator=g) * .2).double()
    b_in, xhat_in = bn_ref(x, gi, bi)
    b_in = b_in.detach().requires_grad_(True)
    z = F.conv2d(F.conv2d(F.relu(b_in), w_pw, b_pw), w_dw, b_dw, padding=1, groups=cout)
    zb, xhat_out = bn_ref(z, go, bo)
    xg = nhwc(x.float()).to(DEV)
    zg = nhwc(z.detach().float()).to(DEV)
    ws = (w_pw.detach().float().to(DEV).view(cout, cin).contiguous(), b_pw.detach().float().to(DEV),
          w_dw.detach().float().to(DEV).view(cout, 9).contiguous(), b_dw.detach().float().to(DEV))
    idx = None
    if pooldy:
        # the window positions a forward launch records; dy: the pooled gradient, which reaches the recorded position only
        fin, _ = bn_pair(k, cin, stats_of(xg), gi, bi, n * h * w)
        fout, _ = bn_pair(k, cout, None, go, bo, n * h * w)
        idx = k.dp_fwd(xg, *ws, fin, fout, pool=True)[2]
        dyp = torch.randn(n, cout, h // 2, w // 2, generator=g)
        pos = nchw(idx.cpu()).long()
        full = torch.zeros(n, cout, h // 2, w // 2, 4, dtype=torch.float64).scatter_(-1, pos.unsqueeze(-1), dyp.double().unsqueeze(-1))
        dy_ref = full.view(n, cout, h // 2, w // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, cout, h, w)
        dy_dev = nhwc(dyp).to(DEV)
    else:
        r = torch.randn(n, cout, h, w, generator=g).double()
        dy_ref = (r * (zb.detach() > 0)).float().double()          # the gradient at the BN output, ReLU mask applied, as stored
        dy_dev = nhwc(dy_ref.float()).to(DEV)
    (zb * dy_ref).sum().backward()
    out_sums = torch.cat([dy_ref.sum(dim=(0, 2, 3)), (dy_ref * xhat_out.detach()).sum(dim=(0, 2, 3))])
    in_d, in_f = bn_pair(k, cin, stats_of(xg), gi, bi, n * h * w, bstats='zero')
    out_d, out_f = bn_pair(k, cout, stats_of(zg), go, bo, n * h * w, bstats=out_sums)
    grid = k.dp_grid(n, h, w, cin, cout)
    part = torch.empty(grid, k.dp_row_width(cin, cout), device=DEV)

    def launch(in_bn, out_bn):
        part.fill_(float('nan'))          # every row is written by the launch
        dx = k.dp_bwd(xg, *ws, zg, dy_dev, in_bn, out_bn, partials=part, pool_idx=idx)[0]
        return dx, part.clone()
    ref = launch(in_d, out_d)
    torch.cuda.synchronize()

    def run():
        in_f.bstats.zero_()
        dx, rows_w = launch(in_f, out_f)
        rows = in_f.bstats.clone()
        return dx, rows_w, rows, k.bn_fold(in_f.bstats).clone()
    dx, rows_w, rows, folded = five_times(run)                                         # 4. repeat launches
    assert bool(torch.isfinite(rows_w).all())
    assert same_bytes(dx, ref[0]), ('dx', n, h, w)                                     # 1. non-sum outputs
    assert same_bytes(rows_w, ref[1]), ('wgrad_partials', n, h, w)
    check_rows(rows, grid)                                                             # 2. row structure
    e = sums_err(folded, in_d.bstats)
    print(f'[bwd {cin}->{cout} {(n, h, w)} pooldy={pooldy}] grid {grid}, folded sums vs default {e:.3g}')
    assert e <= TOL_SUMS, (e, n, h, w)                                                 # 3. folded sums
    tot = rows_w.double().sum(0).cpu()                                                 # 5. fp64 reference
    o1, o2, o3 = cout * cin, cout * cin + cout, cout * cin + cout + cout * 9
    assert rel_err(nchw(dx.cpu()), b_in.grad) < TOL_BWD, ('dx', n, h, w)
    assert rel_err(tot[:o1].view(cout, cin, 1, 1), w_pw.grad) < TOL_BWD and rel_err(tot[o1:o2], b_pw.grad) < TOL_BWD, (n, h, w)
    assert rel_err(tot[o2:o3].view(cout, 1, 3, 3), w_dw.grad) < TOL_BWD, (n, h, w)
    ref_b = torch.cat([b_in.grad.sum(dim=(0, 2, 3)), (b_in.grad * xhat_in).sum(dim=(0, 2, 3))])
    assert rel_err(folded, ref_b) < TOL_BWD, ('bstats', n, h, w)


@pytest.mark.parametrize('n,h,w,pooldy', [(2, 16, 32, False), (3, 40, 40, False), (16, 80, 80, False), (6, 10, 10, False),
                                           (70, 20, 20, False), (3, 40, 48, True)])
def test_dp_bwd64_fast(n, h, w, pooldy):
    """dp_bwd64_kernel<8 | 4, PACKED, POOLDY, DET>: 8 x 16 tiles with fewer tiles than workgroups, 8 x 8 tiles (NW = 4),
    800 tiles, the packed canvas with fewer and more tiles than workgroups, pooled dy."""
    bwd_case(64, 64, n, h, w, pooldy)


@pytest.mark.parametrize('n,h,w,pooldy', [(2, 32, 64, False), (48, 80, 80, False), (2, 64, 96, True)])
def test_dp_bwd16s_fast(n, h, w, pooldy):
    """dp_bwd16s_kernel<POOLDY, DET>."""
    bwd_case(16, 16, n, h, w, pooldy)


@pytest.mark.parametrize('n,h,w,pooldy', [(2, 16, 32, False), (16, 80, 80, True)])
def test_dp_bwd_split_32_64_fast(n, h, w, pooldy):
    """dp_bwd_kernel<32, 64, 8, 16, false, GEMM = 1, POOLDY, FULL, DET>: the split-bf16 backward of YuNet_s' 32 -> 64 unit."""
    bwd_case(32, 64, n, h, w, pooldy)


# --------------------------------------------------------------------------------------------------------- whole steps
_children = {}


def child(tmp_path_factory, tag, *args):
    """One fresh process per (tag, argument list), shared among the tests below, under its own time limit; a failing child
    ends the test."""
    if (tag, args) not in _children:
        out = str(tmp_path_factory.mktemp('fast') / 'out.npz')
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'deterministic_fast_child.py'), *map(str, args[:5]), out,
                            *args[5:]], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        _children[(tag, args)] = dict(np.load(out))
    return _children[(tag, args)]


FIXTURES = [('s', 'train5_s_160.npz', 160), ('n', 'conv_stack_n_160.npz', 320)]


@pytest.mark.parametrize('kind,fixture,size', FIXTURES)
def test_whole_step_fast_is_bitwise_reproducible_across_processes(tmp_path_factory, kind, fixture, size):
    """Three SGD steps of batch 4 from the trained fixture at the fast level, twice, each in a fresh process: every tensor of
    the contract is the same bytes."""
    a = child(tmp_path_factory, 'a', kind, fixture, 4, size, 3)
    b = child(tmp_path_factory, 'b', kind, fixture, 4, size, 3)
    assert list(a['plan_key'])[-1] == 'det-fast'
    assert np.isfinite(a['losses']).all() and float(np.abs(a['grad']).max()) > 0
    for k in CONTRACT + ('grad1',):
        assert np.array_equal(a[k], b[k]), k
    start = Hh.load_golden(fixture)['w:backbone.model0.bn1.num_batches_tracked']
    assert int(a['num_batches_tracked'][0]) == int(start) + 3


@pytest.mark.parametrize('kind,fixture,size', FIXTURES)
def test_first_step_fast_agrees_with_the_default_mode(tmp_path_factory, kind, fixture, size):
    """Losses and flat gradient of the first step against a default-mode child, within what tests/test_bench_gpu.py grants two
    default-mode runs: 1e-5 of scale."""
    a = child(tmp_path_factory, 'a', kind, fixture, 4, size, 3)
    d = child(tmp_path_factory, 'd', kind, fixture, 4, size, 1, '--default')
    assert list(d['plan_key'])[-1] == 'fp32'
    for name, got, want in (('losses', a['losses'][0], d['losses'][0]), ('grad', a['grad1'], d['grad1'])):
        scale = float(np.abs(want).max())
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f'[fast vs default {kind}] {name}: {err:.3g} of scale {scale:.3g}')
        assert err <= 1e-5 * scale + 1e-9, name


def test_train5_vs_reference_golden_fast():
    """tests/test_deterministic_gpu.py::test_train5_vs_reference_golden_deterministic at the fast level: same golden, same bars."""
    import yunet_amd.synthetic as S
    from test_engine_gpu import build, golden_state, rel
    from yunet_amd.optim import FusedSGD
    g = Hh.load_golden('train5_s_160.npz')
    m, cfg = build('s')
    m.load_state_dict(golden_state(g, 'w:'), strict=True)
    m.set_deterministic('fast')
    m.to(DEV)
    opt = FusedSGD(m, lr=float(g['lr']), momentum=float(g['momentum']), weight_decay=float(g['wd']))
    logs, npos = [], []
    for it in range(int(g['iters'])):
        kk = (1 - it / 1500) * (1 - 0.001)
        opt.param_groups[0]['lr'] = float(g['lr']) * (1 - kk)
        b = S.to_device(S.make_batch(int(g['n_img']), int(g['height']), int(g['width']), S.batch_seed(0, it)), DEV)
        out = m.train_step(b, opt)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()
        lv = out['log_vars']
        logs.append([float(lv['loss_cls']), float(lv['loss_bbox']), float(lv['loss_obj']), float(lv['loss_kps']), float(lv['loss'])])
        npos.append(int(m.engine.plan.norm[2].item()))
    plan = m.engine.plan
    assert plan.det and plan.det_rows == FAST and any(op.opcode == L.OP_BN_FOLD for op in plan.fwd_a)
    logs, ref = np.array(logs), g['logs']
    assert np.allclose(logs[0], ref[0], rtol=1e-4), (logs[0], ref[0])
    assert npos[0] == int(g['num_pos'][0])
    assert np.allclose(logs, ref, rtol=2e-2), (logs, ref)
    fin = golden_state(g, 'f:')
    for k in ('backbone.model0.conv1.weight', 'neck.lateral_convs.0.conv1.weight',
              'bbox_head.multi_level_bbox.0.conv1.weight', 'backbone.model3.conv2.bn.running_var'):
        got = m.state_dict()[k].cpu()
        assert rel(got, fin[k]) < 2e-2, (k, rel(got, fin[k]))
