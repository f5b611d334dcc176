"""-m gpu: the wave-streaming kernels at the shapes where a first input row issued from the PROLOGUE can go wrong.

dp_fwd64s (plain, pooled and the grouped launch) and dp_fwd16s put every table load in flight, issue the first input row of
the wave's first task behind them and only then write the tables to LDS and meet at the barrier (csrc/conv_fwd64.hip); the
main loop takes that row from the registers.  What can break: a wave WITHOUT a task (it must fetch nothing and store
nothing), a first task on the image border (halo column outside the image, band 0 starting at row 0), a ragged last strip,
the even-row bands of the pooled instances, a grouped launch whose units differ in size -- and a row left over from an
earlier task, which shows when the same launch is repeated on the same buffers.

Every case is held against a CPU fp64 restatement at the bars of tests/test_kernels_gpu.py (2e-5 forward, 5e-5 backward,
1e-4 the stem's weight gradient) and runs twice: z, the pooled winners, their positions and dx must repeat bit for bit (the
BatchNorm sums are added with fp64 atomics in no fixed order and are held to the bar only).  The backward launches and the
stem go through the same shapes although their prologues still issue the first row after the barrier."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from route_cases import route as dp_route
from test_kernels_gpu import _dp_bwd_case, bn_ref, mk_unit, nchw, nhwc, rel_err, stats_of

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def K():
    import yunet_amd.kernels as k
    return k


def lib():
    import yunet_amd._lib as L
    return L


def make_unit(ci, co, n, h, w, seed, pool=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ci, h, w, generator=g) * 3 + 1.5
    W = mk_unit(ci, co, g)
    gi, bi = torch.rand(ci, generator=g) + 0.5, torch.randn(ci, generator=g) * 0.2
    go, bo = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.3
    if pool:
        go[1], go[co - 3], go[5] = -go[1], -0.7, 0.0        # the window minimum / the first element wins
    return x, W, gi, bi, go, bo


def fwd_ref(x, W, gi, bi):
    a = F.relu(bn_ref(x.double(), gi.double(), bi.double())[0])
    p = F.conv2d(a, W[0].double(), W[1].double())
    return F.conv2d(p, W[2].double(), W[3].double(), padding=1, groups=W[0].shape[0])


def dev_weights(W):
    co, ci = W[0].shape[:2]
    return [W[0].to(DEV).view(co, ci).contiguous(), W[1].to(DEV), W[2].to(DEV).view(co, 9).contiguous(), W[3].to(DEV)]


# (cin, cout, N, H, W, pool, expected instance)
FWD_CASES = {
    # 5 bands of 2 rows = 5 tasks for the 8 waves of two workgroups: three waves have no task
    'fewer-tasks-than-waves': (64, 64, 1, 10, 10, False, 'dp_fwd64s_kernel<false,false>'),
    # one 14-column strip: the halo columns -1 and 14 lie outside the image, band 0 starts at row 0
    'first-task-on-the-border': (64, 64, 2, 6, 14, False, 'dp_fwd64s_kernel<false,false>'),
    'ragged-last-strip-64': (64, 64, 3, 12, 20, False, 'dp_fwd64s_kernel<false,false>'),         # 14 + 6 columns
    'ragged-last-strip-16': (16, 16, 2, 32, 72, False, 'dp_fwd16s_kernel<16,false,'),            # 30 + 30 + 12 columns
    'pooled-16': (16, 16, 2, 32, 64, True, 'dp_fwd16s_kernel<16,true,'),
    'pooled-64': (64, 64, 2, 8, 16, True, 'dp_fwd64s_kernel<true,false>'),
}


def launch_fwd(k, xg, Wd, in_bn, go, bo, cnt, pool, z):
    st = torch.zeros(2 * Wd[0].shape[0], dtype=torch.float64, device=DEV)
    out = k.dp_fwd(xg, *Wd, in_bn, k.BN(st, go.to(DEV), bo.to(DEV), cnt), z=z, pool=pool)
    torch.cuda.synchronize()
    return (out if pool else (out,)), st


@pytest.mark.parametrize('cid', list(FWD_CASES))
def test_forward_first_row_from_the_prologue(cid):
    ci, co, n, h, w, pool, instance = FWD_CASES[cid]
    k, L = K(), lib()
    x, W, gi, bi, go, bo = make_unit(ci, co, n, h, w, seed=len(cid) * 1000 + h * w, pool=pool)
    zr = fwd_ref(x, W, gi, bi)
    xg, Wd, cnt = nhwc(x).to(DEV), dev_weights(W), n * h * w
    in_bn = k.BN(stats_of(xg).to(DEV), gi.to(DEV), bi.to(DEV), cnt)
    z = torch.full((n, h, w, co), float('nan'), device=DEV)
    d = k._dp_desc(xg, *Wd, z, in_bn, k.BN(torch.zeros(2 * co, dtype=torch.float64, device=DEV), go.to(DEV), bo.to(DEV), cnt))
    if pool:
        keep = (torch.empty(n, h // 2, w // 2, co, device=DEV), torch.empty(n, h // 2, w // 2, co, dtype=torch.uint8, device=DEV))
        d.pool_out, d.pool_idx = keep[0].data_ptr(), keep[1].data_ptr()
    assert (dp_route(L.load(), d, 0) or '').startswith(instance), dp_route(L.load(), d, 0)
    first, st = launch_fwd(k, xg, Wd, in_bn, go, bo, cnt, pool, z)
    first = [t.clone() for t in first]
    assert rel_err(nchw(first[0].cpu()), zr) < 2e-5
    assert rel_err(st, stats_of(nhwc(zr))) < 2e-5
    if pool:
        # the raw winners, transformed, are the pooled activations (tests/test_kernels_gpu.py: test_fused_pooling)
        zb = bn_ref(zr, go.double(), bo.double())[0]
        pooled = F.max_pool2d(F.relu(zb), 2)
        mean, var = zr.mean(dim=(0, 2, 3)).view(1, -1, 1, 1), zr.var(dim=(0, 2, 3), unbiased=False).view(1, -1, 1, 1)
        act = F.relu((nchw(first[1].cpu()).double() - mean) / torch.sqrt(var + 1e-5) * go.double().view(1, -1, 1, 1)
                     + bo.double().view(1, -1, 1, 1))
        assert rel_err(act, pooled) < 2e-5
        assert bool((first[2][..., 5] == 0).all())              # the constant channel: position 0 everywhere
    again, st2 = launch_fwd(k, xg, Wd, in_bn, go, bo, cnt, pool, z)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert rel_err(st2, stats_of(nhwc(zr))) < 2e-5


def test_grouped_forward_of_three_sizes():
    """yunet_dp_fwd_group: 8 x 8, 4 x 4 and 2 x 2 at N = 2 in one grid -- every unit's workgroups derive their first task from
    the unit's own grid, and most waves of the two small units have no task"""
    k, L = K(), lib()
    units, keep = [], []
    for j, s in enumerate((8, 4, 2)):
        n = 2
        x, W, gi, bi, go, bo = make_unit(64, 64, n, s, s, seed=40 + s)
        xg, Wd, cnt = nhwc(x).to(DEV), dev_weights(W), n * s * s
        z = torch.full((n, s, s, 64), float('nan'), device=DEV)
        st = torch.zeros(128, dtype=torch.float64, device=DEV)
        in_bn, out_bn = k.BN(stats_of(xg).to(DEV), gi.to(DEV), bi.to(DEV), cnt), k.BN(st, go.to(DEV), bo.to(DEV), cnt)
        units.append(k._dp_desc(xg, *Wd, z, in_bn, out_bn))
        keep.append((fwd_ref(x, W, gi, bi), xg, Wd, z, st, in_bn, out_bn))
    arr = (C.POINTER(L.YunetDP) * 3)(*[C.pointer(d) for d in units])
    assert L.load().yunet_dp_fwd_group_one_grid(arr, 3) == 1
    results = []
    for _ in range(2):
        for u in keep:
            u[4].zero_()
        L.check(L.load().yunet_dp_fwd_group(arr, 3, k._stream()), 'yunet_dp_fwd_group')
        torch.cuda.synchronize()
        results.append([u[3].clone() for u in keep])
        for (zr, _, _, z, st, _, _) in keep:
            assert rel_err(nchw(z.cpu()), zr) < 2e-5
            assert rel_err(st, stats_of(nhwc(zr))) < 2e-5
    for a, b in zip(*results):
        assert torch.equal(a, b)


# backward through yunet_dp_bwd at the same shapes: dp_bwd64 (64 -> 64) and dp_bwd16s (16 -> 16 on the big-tile map)
BWD_SHAPES = {(64, 64): [(1, 10, 10), (2, 6, 14), (3, 12, 20)], (16, 16): [(2, 32, 72)]}


@pytest.mark.parametrize('ci,co', list(BWD_SHAPES))
def test_backward_against_fp64(ci, co):
    _dp_bwd_case(ci, co, 'bn_bn', tol=5e-5, shapes=BWD_SHAPES[(ci, co)])


@pytest.mark.parametrize('ci,co', list(BWD_SHAPES))
def test_backward_repeats_bit_for_bit(ci, co):
    k = K()
    for (n, h, w) in BWD_SHAPES[(ci, co)]:
        x, W, gi, bi, go, bo = make_unit(ci, co, n, h, w, seed=7 * h + w)
        g = torch.Generator().manual_seed(h * w)
        zr = fwd_ref(x, W, gi, bi)
        dy = torch.randn(n, h, w, co, generator=g) * (torch.rand(n, h, w, co, generator=g) > 0.5)
        xg, zg, Wd, cnt = nhwc(x).to(DEV), nhwc(zr.float()).to(DEV), dev_weights(W), n * h * w
        dx = torch.full((n, h, w, ci), float('nan'), device=DEV)
        bst = torch.randn(2 * co, generator=g).double().to(DEV)      # (any sums: the two runs share them)
        got = []
        for _ in range(2):
            in_bn = k.BN(stats_of(xg).to(DEV), gi.to(DEV), bi.to(DEV), cnt, bstats=torch.zeros(2 * ci, dtype=torch.float64, device=DEV))
            out_bn = k.BN(stats_of(zg).to(DEV), go.to(DEV), bo.to(DEV), cnt, bstats=bst)
            k.dp_bwd(xg, *Wd, zg, dy.to(DEV), in_bn, out_bn, dx=dx)
            torch.cuda.synchronize()
            got.append(dx.clone())
        assert not bool(torch.isnan(got[0]).any())
        assert torch.equal(got[0], got[1]), (n, h, w)


def test_stem_on_a_16_by_64_image():
    """the stem's row ring on an image of 8 x 32 outputs: forward against fp64 and twice; the matrix-core weight gradient"""
    k = K()
    n, h, w = 2, 16, 64
    g = torch.Generator().manual_seed(1664)
    img = torch.rand(n, 3, h, w, generator=g) * 255
    wt = (torch.randn(16, 3, 3, 3, generator=g) * 0.05).double().requires_grad_(True)
    b = (torch.randn(16, generator=g) * 0.1).double().requires_grad_(True)
    gamma, beta = (torch.rand(16, generator=g) + 0.5).double(), torch.randn(16, generator=g).double() * 0.2
    z = F.conv2d(img.double(), wt, b, stride=2, padding=1)
    zb, xhat = bn_ref(z, gamma, beta)
    zb.retain_grad()
    (F.relu(zb) * torch.randn(z.shape, generator=g).double()).sum().backward()
    wd, bd = wt.detach().float().to(DEV).contiguous(), b.detach().float().to(DEV)
    zs = []
    for _ in range(2):
        stats = torch.zeros(32, dtype=torch.float64, device=DEV)
        zs.append(k.stem_fwd(img.to(DEV), wd, bd, stats))
        torch.cuda.synchronize()
        assert rel_err(nchw(zs[-1].cpu()), z.detach()) < 2e-5
        assert rel_err(stats, stats_of(nhwc(z.detach()))) < 2e-5
    assert torch.equal(zs[0], zs[1])
    dy = zb.grad
    bst = torch.cat([dy.sum(dim=(0, 2, 3)), (dy * xhat.detach()).sum(dim=(0, 2, 3))]).to(DEV)
    bn = k.BN(stats, gamma.float().to(DEV), beta.float().to(DEV), n * (h // 2) * (w // 2), bstats=bst)
    dw, db = k.stem_bwd(img.to(DEV), zs[0], nhwc(dy.float()).to(DEV), bn, wd, bd)
    torch.cuda.synchronize()
    assert rel_err(dw, wt.grad) < 1e-4
    assert float(db.abs().max()) < 1e-3 * float(dy.abs().sum())
