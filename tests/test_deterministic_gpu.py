"""-m gpu: the deterministic mode of the fused training engine -- same inputs, same state, same build,
same device model give the same BYTES: whole steps in fresh processes, every kernel with order-fixed BatchNorm sums through
the C ABI, the fold kernel against its documented order, parity with the reference golden, the command line, resume."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deterministic_child as DC
import yunet_amd._lib as L
from yunet_amd.engine import DET_ROWS as R          # rows of a deterministic sum block
import helpers as Hh
from test_kernels_gpu import bn_ref, mk_unit, nchw, nhwc, rel_err, rel_err_ch, stats_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ('losses', 'grad', 'params', 'momentum', 'running_mean', 'running_var', 'num_batches_tracked')


def K():
    import yunet_amd.kernels as k
    return k


def child(tmp_path, tag, *args):
    out = str(tmp_path / f'{tag}.npz')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'deterministic_child.py'), *map(str, args), out],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.mark.parametrize('kind,fixture,size', [('s', 'train5_s_160.npz', 160), ('n', 'conv_stack_n_160.npz', 320)])
def test_whole_step_is_bitwise_reproducible_across_processes(tmp_path, kind, fixture, size):
    """Three SGD steps of batch 4 from the trained fixture, twice, each in a fresh process: losses, every parameter
    gradient, the updated parameters, the momentum buffers and the BN buffers are the same bytes."""
    a = child(tmp_path, 'a', kind, fixture, 4, size, 3)
    b = child(tmp_path, 'b', kind, fixture, 4, size, 3)
    assert np.isfinite(a['losses']).all() and float(np.abs(a['grad']).max()) > 0
    for k in CONTRACT:
        assert np.array_equal(a[k], b[k]), k
    start = Hh.load_golden(fixture)['w:backbone.model0.bn1.num_batches_tracked']      # (the n fixture is a trained checkpoint)
    assert int(a['num_batches_tracked'][0]) == int(start) + 3


# ------------------------------------------------------------------------------------------ kernels through the C ABI
def det_bn(k, c, stats_rows, gamma, beta, count, bstats=False):
    """A YunetBN whose blocks are [1 + R, 2c]: row 0 = `stats_rows` (the producer's sums), bstats zero when asked for."""
    st = torch.zeros(1 + R, 2 * c, dtype=torch.float64, device=DEV)
    if stats_rows is not None:
        st[0] = stats_rows.to(DEV)
    bst = torch.zeros(1 + R, 2 * c, dtype=torch.float64, device=DEV) if bstats else None
    return k.BN(st, gamma.float().to(DEV), beta.float().to(DEV), count, bstats=bst, det_rows=R)


def five_times(run):
    """`run()` -> tuple of device tensors; five launches on the same buffers must give identical bytes.  Returns the last."""
    outs = []
    for _ in range(5):
        res = run()
        torch.cuda.synchronize()
        outs.append([t.detach().cpu().numpy().copy() for t in res])
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert np.array_equal(x, y)
    return res


# Two shapes per family: fewer tiles than workgroups, and N H W at least twice the persistent grid's pixels per pass, so that
# every workgroup accumulates several tiles.  Forward: up to 1024 workgroups x (8 x 16 | 16 x 32 for the big-tile 16 -> 16
# unit) pixels; backward: 256 workgroups x the same tiles.
SMALL = (2, 16, 32)
FWD_WALK = {(16, 16): (44, 160, 160)}           # 2200 tiles of 16 x 32; every other unit: 2400 tiles of 8 x 16
BWD_WALK = {(16, 16): (48, 80, 80)}             # 720 tiles of 16 x 32; every other unit: 800 tiles of 8 x 16


def dp_shapes(cin, cout, backward):
    walk = BWD_WALK.get((cin, cout), (16, 80, 80)) if backward else FWD_WALK.get((cin, cout), (48, 80, 80))
    return [SMALL, walk] + [s[2:] for s in PACKED_SHAPES if s[:2] == (cin, cout)]


PACKED_SHAPES = [(64, 64, 6, 10, 10), (64, 64, 70, 20, 20), (64, 16, 70, 20, 20)]     # packed canvas: fewer / more tiles than workgroups


@pytest.mark.parametrize('cin,cout', [(16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64)])
def test_dp_fwd_det(cin, cout):
    """yunet_dp_fwd with out_bn.det_rows: z and the folded sums vs fp64 at test_dp_fwd's tolerances (2e-5, per channel
    8e-5), identical bytes over five launches (rows are re-zeroed like the step's memset does)."""
    k = K()
    g = torch.Generator().manual_seed(cin * 100 + cout + 1)
    for (n, h, w) in dp_shapes(cin, cout, False):
        x = torch.randn(n, cin, h, w, generator=g) * 3 + 1.5
        w_pw, b_pw, w_dw, b_dw = mk_unit(cin, cout, g)
        gamma, beta = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.2
        a = F.relu(bn_ref(x.double(), gamma.double(), beta.double())[0])
        zr = F.conv2d(F.conv2d(a, w_pw.double(), b_pw.double()), w_dw.double(), b_dw.double(), padding=1, groups=cout)
        xg = nhwc(x).to(DEV)
        in_bn = det_bn(k, cin, stats_of(xg), gamma, beta, n * h * w)
        out_bn = det_bn(k, cout, None, torch.ones(cout), torch.zeros(cout), n * h * w)
        args = (xg, w_pw.to(DEV).view(cout, cin).contiguous(), b_pw.to(DEV), w_dw.to(DEV).view(cout, 9).contiguous(), b_dw.to(DEV))

        def run():
            out_bn.stats.zero_()
            z = k.dp_fwd(*args, in_bn, out_bn)
            return z, k.bn_fold(out_bn.stats).clone(), out_bn.stats.clone()
        z, sums, _ = five_times(run)
        assert rel_err(nchw(z.cpu()), zr) < 2e-5, (n, h, w)
        assert rel_err(sums, stats_of(nhwc(zr))) < 2e-5, (n, h, w)


@pytest.mark.parametrize('cin,cout', [(16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64), (64, 16)])
def test_dp_bwd_det(cin, cout):
    """yunet_dp_bwd with in_bn.det_rows: dx, the weight gradients and the producer's folded BN-backward sums vs fp64
    autograd, identical bytes over five launches.  Tolerance: that of the default-mode test of the same kernel instance --
    test_dp_bwd's 5e-5, and test_dp_bwd_exact_fp32mma's 2e-5 for the 64 -> 64 and 32 -> 64 units, whose deterministic form is
    the exact-fp32 tile kernel that test drives."""
    k = K()
    tol = 2e-5 if (cin, cout) in ((64, 64), (32, 64)) else 5e-5
    out_bn_on = not (cin == 64 and cout == 16)
    g = torch.Generator().manual_seed(11 + cin * 100 + cout)
    for (n, h, w) in dp_shapes(cin, cout, True):
        x = (torch.randn(n, cin, h, w, generator=g) * 2 + 0.5).double()
        w_pw, b_pw, w_dw, b_dw = [t.double().requires_grad_(True) for t in mk_unit(cin, cout, g)]
        gi, bi = (torch.rand(cin, generator=g) + 0.5).double(), (torch.randn(cin, generator=g) * .2).double()
        go, bo = (torch.rand(cout, generator=g) + 0.5).double(), (torch.randn(cout, generator=g) * .2).double()
        r = torch.randn(n, cout, h, w, generator=g).double()
        b_in, xhat_in = bn_ref(x, gi, bi)
        b_in = b_in.detach().requires_grad_(True)
        z = F.conv2d(F.conv2d(F.relu(b_in), w_pw, b_pw), w_dw, b_dw, padding=1, groups=cout)
        if out_bn_on:
            zb, xhat_out = bn_ref(z, go, bo)
            zb.retain_grad()
            (F.relu(zb) * r).sum().backward()
            dy_ref = zb.grad
        else:
            (z * r).sum().backward()
            dy_ref = r
        xg = nhwc(x.float()).to(DEV)
        zg = nhwc(z.detach().float()).to(DEV)
        in_bn = det_bn(k, cin, stats_of(xg), gi, bi, n * h * w, bstats=True)
        out_bn = None
        if out_bn_on:
            out_bn = det_bn(k, cout, stats_of(zg), go, bo, n * h * w, bstats=True)
            out_bn.bstats[0] = torch.cat([dy_ref.sum(dim=(0, 2, 3)), (dy_ref * xhat_out.detach()).sum(dim=(0, 2, 3))]).to(DEV)
        args = (xg, w_pw.detach().float().to(DEV).view(cout, cin).contiguous(), b_pw.detach().float().to(DEV),
                w_dw.detach().float().to(DEV).view(cout, 9).contiguous(), b_dw.detach().float().to(DEV), zg,
                nhwc(dy_ref.float()).to(DEV))

        part = torch.empty(k.dp_grid(n, h, w, cin, cout), k.dp_row_width(cin, cout), device=DEV)

        def run():
            in_bn.bstats.zero_()
            part.fill_(float('nan'))          # every row is written by the launch (or zeroed by its launcher)
            dx, dw1, db1, dw2, db2 = k.dp_bwd(*args, in_bn, out_bn, partials=part)
            return dx, part.clone(), dw1, db1, dw2, db2, k.bn_fold(in_bn.bstats).clone(), in_bn.bstats.clone()
        dx, rows, dw1, db1, dw2, db2, bsum, _ = five_times(run)
        assert bool(torch.isfinite(rows).all())
        # the bounds of _dp_bwd_case (test_kernels_gpu.py), max-norm and per channel
        assert rel_err(nchw(dx.cpu()), b_in.grad) < tol, ('dx', n, h, w)
        assert rel_err_ch(nchw(dx.cpu()), b_in.grad) < 4 * tol, ('dx per channel', n, h, w)
        assert rel_err_ch(dw1.reshape(cout, cin), w_pw.grad.reshape(cout, cin), dim=0) < 4 * tol, ('dw1 per output channel', n, h, w)
        assert rel_err(dw1, w_pw.grad) < tol and rel_err(db1, b_pw.grad) < tol and rel_err(dw2, w_dw.grad) < tol, (n, h, w)
        if not out_bn_on:       # with BN the dw-bias gradient is identically zero (noise only)
            assert rel_err(db2, b_dw.grad) < tol, ('db2', n, h, w)
        else:
            assert float(db2.abs().max()) < 1e-3 * float(dy_ref.abs().sum())
        ref_b = torch.cat([b_in.grad.sum(dim=(0, 2, 3)), (b_in.grad * xhat_in).sum(dim=(0, 2, 3))])
        assert rel_err(bsum, ref_b) < tol, ('bstats', n, h, w)


@pytest.mark.parametrize('ci,c,n,h,w', [(16, 16, 2, 64, 96), (64, 64, 3, 40, 48), (32, 64, 16, 80, 80)])
def test_fused_pooling_det(ci, c, n, h, w):
    """The pooled forms (fused max_pool2d forward, pooled-dy backward) with deterministic sums: P -> pool -> Q as in
    test_fused_pooling, at its tolerances (2e-5 forward, 5e-5 backward), identical bytes over five launches."""
    k = K()
    g = torch.Generator().manual_seed(c + h + ci + 1)
    x = (torch.randn(n, ci, h, w, generator=g) * 1.5 + 0.3).double().requires_grad_(True)
    P = [t.double().requires_grad_(True) for t in mk_unit(ci, c, g)]
    Q = [t.double().requires_grad_(True) for t in mk_unit(c, c, g)]
    gp, bp = (torch.rand(c, generator=g) + 0.5).double(), (torch.randn(c, generator=g) * .3).double()
    gq, bq = (torch.rand(c, generator=g) + 0.5).double(), (torch.randn(c, generator=g) * .3).double()
    zp = F.conv2d(F.conv2d(x, P[0], P[1]), P[2], P[3], padding=1, groups=c)
    zbp, xhat_p = bn_ref(zp, gp, bp)
    zbp.retain_grad()

    def dev(t, *shape):
        t = t.detach().float().to(DEV)
        return t.view(*shape).contiguous() if shape else t
    xg = nhwc(x.detach().float()).to(DEV)
    pw = [dev(P[0], c, ci), dev(P[1]), dev(P[2], c, 9), dev(P[3])]
    qw = [dev(Q[0], c, c), dev(Q[1]), dev(Q[2], c, 9), dev(Q[3])]
    bn_p = det_bn(k, c, None, gp, bp, n * h * w, bstats=True)
    bn_q = det_bn(k, c, None, gq, bq, n * (h // 2) * (w // 2), bstats=True)
    # The fp64 graph pools through the window positions the KERNEL recorded: among 10^5 - 10^6 windows a few hold two
    # values closer than an fp32 rounding, fp32 and fp64 then pick different elements (test_fused_pooling allows 1e-4 of
    # the windows), and F.max_pool2d's own choice would send one window's whole gradient to another pixel of dx.
    # That the recorded positions ARE the maxima is asserted on its own, as in test_fused_pooling.
    idx = k.dp_fwd(xg, *pw, None, bn_p, pool=True)[2]
    torch.cuda.synchronize()
    act = F.relu(zbp)
    win = act.view(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    pooled = win.gather(-1, nchw(idx.cpu()).long().unsqueeze(-1)).squeeze(-1)
    ref_pool = F.max_pool2d(act.detach(), 2)
    agree = (pooled.detach() == ref_pool) | (ref_pool <= 1e-4)          # (dead windows carry no gradient)
    assert float(agree.double().mean()) > 0.9999
    assert rel_err(pooled.detach(), ref_pool) < 2e-5                     # a differing choice is a near-tie
    pooled.retain_grad()
    zq = F.conv2d(F.conv2d(pooled, Q[0], Q[1]), Q[2], Q[3], padding=1, groups=c)
    zbq, xhat_q = bn_ref(zq, gq, bq)
    zbq.retain_grad()
    r = torch.randn(zq.shape, generator=g).double()
    (F.relu(zbq) * r).sum().backward()
    dq = zbq.grad

    def run():
        bn_p.stats.zero_(), bn_q.stats.zero_(), bn_p.bstats.zero_(), bn_q.bstats.zero_()
        zpg, praw, idx = k.dp_fwd(xg, *pw, None, bn_p, pool=True)
        k.bn_fold(bn_p.stats)
        zqg = k.dp_fwd(praw, *qw, bn_p, bn_q)
        k.bn_fold(bn_q.stats)
        bn_q.bstats[0] = torch.cat([dq.sum(dim=(0, 2, 3)), (dq * xhat_q.detach()).sum(dim=(0, 2, 3))]).to(DEV)
        dpool, qdw1, _, qdw2, _ = k.dp_bwd(praw, *qw, zqg, nhwc(dq.float()).to(DEV), bn_p, bn_q)
        k.bn_fold(bn_p.bstats)
        dxp, pdw1, _, pdw2, _ = k.dp_bwd(xg, *pw, zpg, dpool, None, bn_p, pool_idx=idx)
        return zpg, zqg, dpool, qdw1, qdw2, dxp, pdw1, pdw2, bn_p.stats.clone(), bn_p.bstats.clone(), bn_q.stats.clone()
    zpg, zqg, dpool, qdw1, qdw2, dxp, pdw1, pdw2, pst, pbst, _ = five_times(run)
    assert rel_err(nchw(zpg.cpu()), zp.detach()) < 2e-5 and rel_err(pst[0], stats_of(nhwc(zp.detach()))) < 2e-5
    assert rel_err(nchw(zqg.cpu()), zq.detach()) < 5e-5
    tol = 5e-5
    assert rel_err(nchw(dpool.cpu()), pooled.grad * (pooled.detach() > 0)) < tol
    ref_b = torch.cat([zbp.grad.sum(dim=(0, 2, 3)), (zbp.grad * xhat_p.detach()).sum(dim=(0, 2, 3))])
    assert rel_err(pbst[0], ref_b) < tol
    for name, got, want in (('q.dw1', qdw1, Q[0].grad), ('q.dw2', qdw2, Q[2].grad), ('p.dx', nchw(dxp.cpu()), x.grad),
                            ('p.dw1', pdw1, P[0].grad), ('p.dw2', pdw2, P[2].grad)):
        assert rel_err(got, want) < tol, (name, float(rel_err(got, want)))


@pytest.mark.parametrize('n,h,w', [(2, 32, 64), (128, 160, 160)])
def test_stem_fwd_det(n, h, w):
    """yunet_stem_fwd_det vs fp64 at test_stem_fwd_bwd's 2e-5; (2, 32, 64): a handful of strip tasks for 3072 waves,
    (128, 160, 160): more tasks than waves at any band height, every wave adds several bands into its row."""
    k = K()
    g = torch.Generator().manual_seed(h)
    img = torch.rand(n, 3, h, w, generator=g) * 255
    wt, b = torch.randn(16, 3, 3, 3, generator=g) * 0.05, torch.randn(16, generator=g) * 0.1
    z = F.conv2d(img.double(), wt.double(), b.double(), stride=2, padding=1)
    block = torch.zeros(1 + R, 32, dtype=torch.float64, device=DEV)
    imgd, wd, bd = img.to(DEV), wt.to(DEV), b.to(DEV)

    def run():
        block.zero_()
        zg = k.stem_fwd_det(imgd, wd, bd, block)
        return zg, k.bn_fold(block).clone(), block.clone()
    zg, sums, _ = five_times(run)
    assert rel_err(nchw(zg.cpu()), z) < 2e-5
    assert rel_err(sums, stats_of(nhwc(z))) < 2e-5


@pytest.mark.parametrize('c,n,h,w', [(16, 3, 12, 20), (64, 3, 12, 20), (64, 8, 80, 160)])
def test_pool_and_upadd_bwd_det(c, n, h, w):
    """yunet_pool_bwd(_add) and yunet_upadd_bwd (both kernels) with det_rows, vs fp64 autograd at test_pool_fwd_bwd's /
    test_upadd_fwd_bwd's tolerances (dx 2e-5, sums 5e-5).  (3, 12, 20): a few workgroups; (8, 80, 160): 1600 chunks of 256 threads for the
    768-workgroup cap, every workgroup strides over two or three."""
    k = K()
    g = torch.Generator().manual_seed(c + n)
    za = (torch.randn(n, c, h, w, generator=g) * 2).double()
    zb_ = (torch.randn(n, c, h // 2, w // 2, generator=g) * 2).double()
    ga, ba = (torch.rand(c, generator=g) + 0.5).double(), torch.randn(c, generator=g).double() * .3
    gb, bb = (torch.rand(c, generator=g) + 0.5).double(), torch.randn(c, generator=g).double() * .3
    ya, xha = bn_ref(za, ga, ba)
    yb, xhb = bn_ref(zb_, gb, bb)
    ya, yb = ya.detach().requires_grad_(True), yb.detach().requires_grad_(True)
    # the tap feeds max_pool2d and the merge's identity branch
    out = F.relu(ya) + F.interpolate(F.relu(yb), scale_factor=2., mode='nearest')
    pooled = F.max_pool2d(F.relu(ya), 2)
    r, rp = torch.randn(out.shape, generator=g).double(), torch.randn(pooled.shape, generator=g).double()
    ((out * r).sum() + (pooled * rp).sum()).backward()
    zag, zbg = nhwc(za.float()).to(DEV), nhwc(zb_.float()).to(DEV)
    bna = det_bn(k, c, stats_of(zag), ga, ba, n * h * w, bstats=True)
    bnb = det_bn(k, c, stats_of(zbg), gb, bb, n * h * w // 4, bstats=True)
    rg, rpg = nhwc(r.float()).to(DEV), nhwc(rp.float()).to(DEV)

    def run():
        # the engine's order: merge backward (coarse kernel: the tap's share is left to the pool backward), pool backward
        bna.bstats.zero_(), bnb.bstats.zero_()
        _, dxb = k.upadd_bwd(zag, bna, zbg, bnb, rg, skip_a=True)
        dxa = k.pool_bwd(zag, bna, rpg, extra=rg)
        fused = (dxa.clone(), dxb.clone(), k.bn_fold(bna.bstats).clone(), k.bn_fold(bnb.bstats).clone())
        # and the general merge kernel (both shares) followed by an accumulating pool backward into the same rows
        bna.bstats.zero_(), bnb.bstats.zero_()
        dxa2, dxb2 = k.upadd_bwd(zag, bna, zbg, bnb, rg)
        k.pool_bwd(zag, bna, rpg, dx=dxa2, accumulate=True)
        return fused + (dxa2, dxb2, k.bn_fold(bna.bstats).clone(), k.bn_fold(bnb.bstats).clone())
    res = five_times(run)
    ref_a = torch.cat([ya.grad.sum(dim=(0, 2, 3)), (ya.grad * xha).sum(dim=(0, 2, 3))])
    ref_b = torch.cat([yb.grad.sum(dim=(0, 2, 3)), (yb.grad * xhb).sum(dim=(0, 2, 3))])
    for dxa, dxb, sa, sb in (res[:4], res[4:]):
        assert rel_err(nchw(dxa.cpu()), ya.grad) < 2e-5 and rel_err(nchw(dxb.cpu()), yb.grad) < 2e-5
        assert rel_err(sa, ref_a) < 5e-5 and rel_err(sb, ref_b) < 5e-5


def test_bf16_storage_refuses_deterministic_sums():
    k = K()
    c, n, h, w = 16, 2, 8, 8
    z = torch.randn(n, h, w, c, device=DEV).bfloat16()
    bn = det_bn(k, c, None, torch.ones(c), torch.zeros(c), n * h * w, bstats=True)
    import yunet_amd._lib as L
    with pytest.raises(L.YunetHipError):
        k.pool_bwd(z, bn, torch.zeros(n, h // 2, w // 2, c, device=DEV))


# ------------------------------------------------------------------------------------------------------------- fold
def fold_reference(rows):
    """The documented order of yunet_bn_fold, in torch fp64 on the host (every addition is one IEEE operation): slice s adds
    rows s, s + 16, ... in ascending order starting from 0.0, then the slice sums are added in ascending s from 0.0."""
    slices = []
    for s in range(16):
        v = torch.zeros(rows.shape[1], dtype=torch.float64)
        for r in range(s, rows.shape[0], 16):
            v = v + rows[r]
        slices.append(v)
    t = torch.zeros(rows.shape[1], dtype=torch.float64)
    for v in slices:
        t = t + v
    return t


@pytest.mark.parametrize('c', [16, 64])
@pytest.mark.parametrize('nrows', [1, 2, 255, 256, 257, 1024])
def test_bn_fold_is_the_documented_sum_bit_for_bit(nrows, c):
    g = torch.Generator().manual_seed(nrows * 100 + c)
    rows = (torch.randn(nrows, 2 * c, generator=g, dtype=torch.float64) * 1e6 *
            torch.exp(torch.randn(nrows, 2 * c, generator=g, dtype=torch.float64) * 3))
    block = torch.cat([torch.full((1, 2 * c), 7.0, dtype=torch.float64), rows]).to(DEV)
    got = K().bn_fold(block).cpu()
    torch.cuda.synchronize()
    want = fold_reference(rows)
    assert np.array_equal(got.numpy().view(np.uint64), want.numpy().view(np.uint64))
    assert torch.equal(block[1:].cpu(), rows)                                     # the rows are read only
    assert rel_err(got, rows.sum(0)) < 1e-12                                      # and it is the column sum


# ----------------------------------------------------------------------------------------------- parity, CLI, resume
def test_train5_vs_reference_golden_deterministic():
    """tests/test_engine_gpu.py::test_train5_vs_reference_golden with deterministic=True: same golden, same tolerances."""
    import yunet_amd.synthetic as S
    from test_engine_gpu import build, golden_state, rel
    from yunet_amd.optim import FusedSGD
    g = Hh.load_golden('train5_s_160.npz')
    m, cfg = build('s')
    m.load_state_dict(golden_state(g, 'w:'), strict=True)
    m.set_deterministic(True)
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
    assert m.engine.plan.det and any(op.opcode == L.OP_BN_FOLD for op in m.engine.plan.fwd_a)
    logs, ref = np.array(logs), g['logs']
    assert np.allclose(logs[0], ref[0], rtol=1e-4), (logs[0], ref[0])
    assert npos[0] == int(g['num_pos'][0])
    assert np.allclose(logs, ref, rtol=2e-2), (logs, ref)
    fin = golden_state(g, 'f:')
    for k in ('backbone.model0.conv1.weight', 'neck.lateral_convs.0.conv1.weight',
              'bbox_head.multi_level_bbox.0.conv1.weight', 'backbone.model3.conv2.bn.running_var'):
        got = m.state_dict()[k].cpu()
        assert rel(got, fin[k]) < 2e-2, (k, rel(got, fin[k]))


def test_cli_deterministic_runs_leave_identical_checkpoints(tmp_path):
    """tools/train.py configs/yunet_s.py --seed 7 --deterministic --max-iters 5 --no-validate on the synthetic source, twice:
    the last checkpoints (two iterations per epoch, one checkpoint per epoch: after iteration 4) hold the same bytes."""
    cks = []
    for tag in ('a', 'b'):
        wd = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), os.path.join(ROOT, 'configs', 'yunet_s.py'),
                            '--seed', '7', '--deterministic', '--max-iters', '5', '--no-validate', '--work-dir', str(wd),
                            '--cfg-options', 'data.samples_per_gpu=4', 'data.train.type=SyntheticWiderFace',
                            'data.train.img_scale=(160,160)', 'data.train.iters_per_epoch=2', 'checkpoint_config.interval=1'],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        cks.append(torch.load(str(wd / 'epoch_2.pth'), map_location='cpu', weights_only=False))
    a, b = cks
    assert a['meta']['iter'] == 4 and 'deterministic = True' in a['meta']['config']
    assert set(a['state_dict']) == set(b['state_dict'])
    for k, v in a['state_dict'].items():
        assert torch.equal(v, b['state_dict'][k]), k

    def tensors(o, path=''):
        if torch.is_tensor(o):
            yield path, o
        elif isinstance(o, dict):
            for k in sorted(o, key=str):
                yield from tensors(o[k], f'{path}/{k}')
        elif isinstance(o, (list, tuple)):
            for i, x in enumerate(o):
                yield from tensors(x, f'{path}/{i}')
    ta, tb = dict(tensors(a['optimizer'])), dict(tensors(b['optimizer']))
    assert ta and set(ta) == set(tb)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k


def test_resume_is_bitwise_in_deterministic_mode(tmp_path):
    """Five deterministic steps == three steps, checkpoint, load into a fresh model and optimizer, two more steps."""
    import yunet_amd.runner as Rn
    from yunet_amd.optim import FusedSGD

    def mk():
        m = DC.build('s', 'train5_s_160.npz')
        return m, FusedSGD(m, lr=0.01, momentum=0.9, weight_decay=5e-4)
    m, opt = mk()
    for it in range(5):
        DC.step(m, opt, 4, 160, it)
    want = DC.contract(m, opt, [m.engine.plan.losses.cpu().numpy()])
    m1, opt1 = mk()
    for it in range(3):
        DC.step(m1, opt1, 4, 160, it)
    path = str(tmp_path / 'ck.pth')
    Rn.save_checkpoint(m1, opt1, path, dict(epoch=1, iter=3))
    m2, opt2 = mk()
    assert Rn.load_checkpoint(m2, path, opt2)['iter'] == 3
    for it in range(3, 5):
        DC.step(m2, opt2, 4, 160, it)
    got = DC.contract(m2, opt2, [m2.engine.plan.losses.cpu().numpy()])
    for k in CONTRACT:
        assert np.array_equal(got[k], want[k]), k
