"""-m gpu: the bf16 build's conv kernels (BASELINE.json configs[2]) against the fp64 reference of their contract
(tests/bf16_ref.py), per element, at shapes whose tile / task count exceeds the persistent grid.

Every walk case first asserts the walk from the launcher's own geometry: tile kernels have more tiles than workgroups
(backward: yunet_dp_bwd_blocks is the grid; forward: at most 4 workgroups per compute unit), the wave-streaming kernels
more (strip, band) tasks than waves.  The wave-streaming 16-input forward (dp_fwd16s) picks its band height so that no
wave gets a second task at any batch the nets run, so it is checked at the step's own shapes without a walk.

Fused pooling tie rule (bf16_ref.py): the winner of a window is the first position (raster order) among the maxima of
sign(gamma) * stored z -- the rule of pool_fwd_bf16 / pool_bwd_bf16 on the stored tensor and of F.max_pool2d."""
import pytest
import torch

import bf16_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def K():
    import yunet_amd.kernels as k
    return k


@pytest.fixture
def options():
    import yunet_amd._lib as L
    saved = {}

    def set_(name, v):
        prev = L.set_option(name, v)
        saved.setdefault(name, prev)
    yield set_
    for name, v in saved.items():
        L.set_option(name, v)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ceil(a, b):
    return (a + b - 1) // b


def pack_on(n, h, w):
    return h <= 20 and w <= 20 and n >= 4


def canvas_tiles(n, h, w, th, tw):
    r = min(n, 16)
    return ceil(r * (w + 1), tw) * ceil(ceil(n, r) * (h + 1), th)


def fwd64s_tasks(n, h, w, waves, pool=False):
    """conv_fwd64.hip fwd64s_rows / fwd64s_geometry"""
    strips = ceil(w, 14)
    r = h
    while r > 8 and n * strips * ceil(h, r) < waves:
        r = (r + 1) // 2
    while r > 2 and n * strips * ceil(h, r) < waves // 4:
        r = (r + 1) // 2
    if pool and r % 2:
        r += 1
    return n * strips * ceil(h, r)


def assert_walk(cin, cout, n, h, w, pool=False, bwd16s_rows=0, fwd16s=True):
    """the forward and backward instances the bf16 build dispatches for this unit walk the persistent grid"""
    k = K()
    grid_b = k.dp_grid(n, h, w, cin, cout)
    packed = cin == 64 and cout in (64, 16) and pack_on(n, h, w)
    big = cin == 16 and cout == 16 and w >= 64 and h >= 32
    nw4 = cin == 64 and cout == 64 and not packed and w % 16 and w % 8 == 0
    th, tw = (16, 32) if big else (8, 8 if nw4 else 16)
    tiles_b = canvas_tiles(n, h, w, th, tw) if packed else n * ceil(w, tw) * ceil(h, th)
    if cin == 16 and cout == 16 and bwd16s_rows:           # dp_bwd16s: strips of 28 columns, forced band height
        tasks = n * ceil(w, 28) * ceil(h, bwd16s_rows)
        assert tasks > grid_b * 8, ('dp_bwd16s does not walk', tasks, grid_b * 8)
    else:
        assert tiles_b > grid_b, ('backward does not walk', tiles_b, grid_b)
    if cin == 64 and cout == 64:                           # dp_fwd64s, every occupancy the launcher may find
        for bpc in (1, 2, 3):
            t = fwd64s_tasks(n, h, w, cus() * bpc * 4, pool)
            assert t > cus() * bpc * 4, ('dp_fwd64s does not walk', bpc, t)
    elif not (cin == 16 and cout in (16, 64) and fwd16s):  # tile forward, <= 4 workgroups per CU
        ft = canvas_tiles(n, h, w, 8, 16) if packed else n * ceil(w, 32 if big else 16) * ceil(h, 16 if big else 8)
        assert ft > 4 * cus(), ('forward does not walk', ft, 4 * cus())
    print(f'[walk {cin}->{cout} {n}x{h}x{w}] backward {tiles_b} tiles on {grid_b} workgroups')


def make_unit(cin, cout, g):
    return (torch.randn(cout, cin, generator=g) * (2.0 / (cin + cout)) ** 0.5, torch.randn(cout, generator=g) * 0.1,
            torch.randn(cout, 9, generator=g) * 0.3, torch.randn(cout, generator=g) * 0.1)


def run_unit(cin, cout, shape, mode, seed, recompute=False):
    """forward + backward of one unit in the bf16 build against bwd_ref / fwd_ref"""
    k = K()
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    head = cin == 64 and cout == 16
    in_on, out_on = mode.startswith('bn'), mode.endswith('_bn') and not head
    x16 = (torch.randn(n, h, w, cin, generator=g) * 2 + 0.5).to(torch.bfloat16)
    x64 = x16.double()
    W = make_unit(cin, cout, g)
    Wd = [t.to(DEV).contiguous() for t in W]
    gi, bi = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * .2
    go, bo = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * .2
    sx = R.stats_of(x64)
    in_ref = R.BNRef(sx, gi, bi, n * h * w) if in_on else None
    in_bn = k.BN(sx.to(DEV), gi.to(DEV), bi.to(DEV), n * h * w,
                 bstats=torch.zeros(2 * cin, dtype=torch.float64, device=DEV)) if in_on else None
    ost = torch.zeros(2 * cout, dtype=torch.float64, device=DEV)
    out_bn = k.BN(ost, go.to(DEV), bo.to(DEV), n * h * w) if out_on else None
    xg = x16.to(DEV)
    z = k.dp_fwd(xg, *Wd, in_bn, out_bn, z=torch.empty(n, h, w, cout, device=DEV) if head else None)
    torch.cuda.synchronize()
    gemm = cin % 32 == 0
    fr = R.fwd_ref(x64, *W, in_bn=in_ref, bf16_gemm=gemm)
    zc = z.cpu()
    assert zc.dtype == (torch.float32 if head else torch.bfloat16)
    tag = f'{cin}->{cout} {n}x{h}x{w} {mode}'
    R.check_bf16(f'z {tag}', zc, fr['z'], fr['mag'], fr['terms'], fr['amb'], stored='fp32' if head else 'bf16')
    if out_on:
        amb_st = torch.cat([fr['amb'].sum((0, 1, 2)), (2 * fr['z'].abs() * fr['amb']).sum((0, 1, 2))])
        R.check_fp32(f'out stats {tag}', ost, R.stats_of(fr['z']), 2e-5, amb=amb_st)
    # backward
    dy = torch.randn(n, h, w, cout, generator=g).double()
    z64 = zc.double()
    dys = None
    if out_on:
        ob = R.BNRef(ost.cpu(), go, bo, n * h * w)
        zb = fr['z'] if recompute else z64
        bst = torch.cat([dy.sum((0, 1, 2)), (dy * ob.xhat(zb)).sum((0, 1, 2))])
        ob.bstats = bst
        out_bn = k.BN(ost, go.to(DEV), bo.to(DEV), n * h * w, bstats=bst.to(DEV))
    else:
        ob = None
        dys = torch.rand(cout, generator=g) + 0.5
    dx, dw1, db1, dw2, db2 = k.dp_bwd(xg, *Wd, z, dy.float().to(DEV), in_bn, out_bn,
                                      dy_scale=dys.to(DEV) if dys is not None else None)
    torch.cuda.synchronize()
    br = R.bwd_ref(x64, *W, z=z64, dy=dy, in_bn=in_ref, out_bn=ob, dy_scale=dys,
                   bf16_gemm=cin == 64 and cout == 64, recompute_z=recompute)
    return check_grads(tag, br, dx, dw1, db1, dw2, db2, in_bn, out_on, dy)


def check_grads(tag, br, dx, dw1, db1, dw2, db2, in_bn, out_on, dy, tol=5e-5):
    worst = [R.check_fp32(f'dx {tag}', dx, br['dx'], tol, ch_dim=-1),
             R.check_fp32(f'dw1 {tag}', dw1.reshape(br['dw1'].shape), br['dw1'], tol, amb=br['amb']['dw1'], ch_dim=0),
             R.check_fp32(f'db1 {tag}', db1, br['db1'], tol),
             R.check_fp32(f'dw2 {tag}', dw2.reshape(br['dw2'].shape), br['dw2'], tol, amb=br['amb']['dw2'])]
    if out_on:   # with BN behind the unit the depthwise-bias gradient is zero in exact arithmetic: noise only
        assert float(db2.abs().max()) < 1e-3 * float(dy.abs().sum())
    else:
        worst.append(R.check_fp32(f'db2 {tag}', db2, br['db2'], tol))
    if in_bn is not None:
        worst.append(R.check_fp32(f'in bstats {tag}', in_bn.bstats, br['in_bst'], tol))
    return max(worst)


WALK = [(64, 64, (40, 80, 80)),       # dp_fwd64s, dp_bwd64<8>
        (64, 64, (160, 40, 40)),      # dp_fwd64s, dp_bwd64<4> (8 x 8 tiles, 512 workgroups)
        (64, 64, (400, 20, 20)),      # dp_fwd64s on a small map, dp_bwd64<8, packed>
        (16, 64, (40, 80, 80)),       # dp_fwd16s<64> (no walk, see the module docstring), dp_bwd<16,64,..,FULL>
        (16, 32, (40, 80, 80)),       # dp_fwd<16,32>, dp_bwd<16,32,..,FULL>
        (32, 64, (40, 80, 80)),       # dp_fwd<32,64>, dp_bwd<32,64,..,GEMM=1,FULL>
        (64, 16, (40, 80, 80)),       # heads, fp32 z: dp_fwd<64,16>, dp_bwd<64,16>
        (64, 16, (330, 20, 20))]      # packed heads


@pytest.mark.parametrize('mode', ['bn_bn', 'id_bn', 'bn_nobn'])
@pytest.mark.parametrize('cin,cout,shape', WALK)
def test_bf16_unit_walk(cin, cout, shape, mode):
    assert_walk(cin, cout, *shape)
    run_unit(cin, cout, shape, mode, seed=cin * 1000 + cout + shape[1])


@pytest.mark.parametrize('mode', ['bn_bn', 'id_bn'])
def test_bf16_16x16_big_tile_walk(mode, options):
    """the 16 -> 16 tile kernels dp_fwd<16,16,16,32> and dp_bwd<16,16,16,32,FULL> (options fwd16s = bwd16s = 0)"""
    options('fwd16s', 0)
    options('bwd16s', 0)
    assert_walk(16, 16, 24, 160, 160, fwd16s=False)
    run_unit(16, 16, (24, 160, 160), mode, seed=5)


@pytest.mark.parametrize('shape,rows', [((5, 50, 70), 0), ((2, 160, 160), 0), ((24, 160, 160), 4)])
def test_bf16_dp_bwd16s(shape, rows, options):
    """dp_bwd16s of the bf16 build: z recomputed from the bf16 x (the stored z is not read) -- fp64 reference at the
    test_dp_bwd bars; (5, 50, 70): ragged strips and bands; rows = 4 forces short bands so that (24, 160, 160) gives
    every wave several tasks.  The fp32 build's dp_bwd16s on the same widened input agrees to 1e-6."""
    k = K()
    options('bwd16s', 1)
    if rows:
        options('bwd16s_rows', rows)
        assert_walk(16, 16, *shape, bwd16s_rows=rows)
    worst = run_unit(16, 16, shape, 'bn_bn', seed=11 + shape[0], recompute=True)
    print(f'[dp_bwd16s bf16 {shape}] worst error / bound {worst:.3g}')
    # the two builds on the same input
    n, h, w = shape
    g = torch.Generator().manual_seed(3)
    x16 = (torch.randn(n, h, w, 16, generator=g) * 2 + 0.5).to(torch.bfloat16).to(DEV)
    Wd = [t.to(DEV).contiguous() for t in make_unit(16, 16, g)]
    gi, bi = (torch.rand(16, generator=g) + 0.5).to(DEV), (torch.randn(16, generator=g) * .2).to(DEV)
    go, bo = (torch.rand(16, generator=g) + 0.5).to(DEV), (torch.randn(16, generator=g) * .2).to(DEV)
    dy = torch.randn(n, h, w, 16, generator=g).to(DEV)
    sx = R.stats_of(x16.double().cpu()).to(DEV)
    bst = torch.randn(32, generator=g).double().to(DEV)
    st = torch.cat([torch.full((16,), 0.3 * n * h * w), torch.full((16,), 2.0 * n * h * w)]).double().to(DEV)
    res = []
    for x in (x16, x16.float()):
        ib = k.BN(sx, gi, bi, n * h * w, bstats=torch.zeros(32, dtype=torch.float64, device=DEV))
        ob = k.BN(st, go, bo, n * h * w, bstats=bst)
        res.append([t.clone() for t in k.dp_bwd(x, *Wd, torch.empty_like(x), dy, ib, ob)] + [ib.bstats.clone()])
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert float((a.double() - b.double()).abs().max()) <= 1e-6 * float(b.abs().max() + 1e-30)


POOLED = [(16, 16, (24, 160, 160)),   # dp_fwd16s<16,true>; the tile backward (bwd16s = 0) walking, then dp_bwd16s<POOLDY>
          (64, 64, (40, 80, 80)),     # dp_fwd64s<POOL>, dp_bwd64<8,false,true>
          (64, 64, (160, 40, 40)),    # dp_fwd64s<POOL>, dp_bwd64<4,false,true>
          (32, 64, (40, 80, 80))]     # dp_fwd<32,64,8,16,false,POOL>, dp_bwd<32,64,..,GEMM=1,POOLDY,FULL>


@pytest.mark.parametrize('ci,c,shape', POOLED)
def test_bf16_fused_pooling(ci, c, shape, options):
    """bf16 twin of test_fused_pooling: unit P -> BN -> ReLU -> max_pool2d(2) -> unit Q, P's forward writing the window
    winners (bf16) and positions, P's backward expanding Q's pooled gradient.  Negative and zero gammas kept."""
    k = K()
    n, h, w = shape
    if ci == 16:
        options('bwd16s', 0)                 # the pooled tile backward dp_bwd<16,16,16,32,..,POOLDY,FULL>
    assert_walk(ci, c, n, h, w, pool=True)
    g = torch.Generator().manual_seed(c + h + ci)
    x16 = (torch.randn(n, h, w, ci, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    P, Q = make_unit(ci, c, g), make_unit(c, c, g)
    gp, bp = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * .3
    gp[1], gp[c - 3] = -gp[1], -0.7          # falling BN: the window minimum wins
    gp[5] = 0.0                              # constant channel: position 0
    gq, bq = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * .3
    Pd, Qd = [t.to(DEV).contiguous() for t in P], [t.to(DEV).contiguous() for t in Q]
    bn_p = k.BN(torch.zeros(2 * c, dtype=torch.float64, device=DEV), gp.to(DEV), bp.to(DEV), n * h * w,
                bstats=torch.zeros(2 * c, dtype=torch.float64, device=DEV))
    z, praw, idx = k.dp_fwd(x16.to(DEV), *Pd, None, bn_p, pool=True)
    torch.cuda.synchronize()
    tag = f'pool {ci}->{c} {n}x{h}x{w}'
    fr = R.fwd_ref(x16.double(), *P, bf16_gemm=ci % 32 == 0)
    R.check_bf16(f'z {tag}', z.cpu(), fr['z'], fr['mag'], fr['terms'], fr['amb'])
    zc, pc, ic = z.cpu(), praw.cpu(), idx.cpu()
    R.check_pool(tag, zc, pc, ic, gp)
    # relu(bn(winner)) == max_pool2d(relu(bn(stored z))) exactly (fp64, the same coefficients)
    bpr = R.BNRef(bn_p.stats.cpu(), gp, bp, n * h * w)
    assert torch.equal(bpr.act(pc.double()), R.windows(bpr.act(zc.double())).amax(-1))
    # the unfused bf16 pair on the stored z16 follows the same rule
    bn_u = k.BN(bn_p.stats.clone(), gp.to(DEV), bp.to(DEV), n * h * w,
                bstats=torch.zeros(2 * c, dtype=torch.float64, device=DEV))
    pu = k.pool_fwd(z, bn_u)
    dpo = torch.randn(pu.shape, generator=g).to(DEV)
    du = k.pool_bwd(z, bn_u, dpo)
    torch.cuda.synchronize()
    pa = bpr.act(pc.double())
    R.check_bf16(f'unfused pooled {tag}', pu.cpu(), pa, pa.abs() + bpr.beta.abs(), 4)
    live = bpr.act(pc.double()) > 0
    R.check_routing(f'unfused {tag}', du.cpu(), dpo.cpu().double() * live, ic)
    # Q from the pooled winners through P's BN + ReLU
    bn_q = k.BN(torch.zeros(2 * c, dtype=torch.float64, device=DEV), gq.to(DEV), bq.to(DEV), n * h * w // 4)
    zq = k.dp_fwd(praw, *Qd, bn_p, bn_q)
    torch.cuda.synchronize()
    qr = R.fwd_ref(pc.double(), *Q, in_bn=bpr, bf16_gemm=c % 32 == 0)
    R.check_bf16(f'q.z {tag}', zq.cpu(), qr['z'], qr['mag'], qr['terms'], qr['amb'])
    # backward: Q writes the masked pooled gradient + P's BN-backward sums, P expands it at idx
    dq = torch.randn(zq.shape, generator=g).double()
    qb = R.BNRef(bn_q.stats.cpu(), gq, bq, n * h * w // 4)
    qb.bstats = torch.cat([dq.sum((0, 1, 2)), (dq * qb.xhat(zq.cpu().double())).sum((0, 1, 2))])
    bn_q.bstats = qb.bstats.to(DEV)
    dpool, qdw1, qdb1, qdw2, qdb2 = k.dp_bwd(praw, *Qd, zq, dq.float().to(DEV), bn_p, bn_q)
    torch.cuda.synchronize()
    qref = R.bwd_ref(pc.double(), *Q, z=zq.cpu().double(), dy=dq, in_bn=bpr, out_bn=qb, bf16_gemm=c == 64)
    wq = check_grads(f'Q {tag}', qref, dpool, qdw1, qdb1, qdw2, qdb2, bn_p, True, dq)
    bpr.bstats = bn_p.bstats.cpu()
    dxp, pdw1, pdb1, pdw2, pdb2 = k.dp_bwd(x16.to(DEV), *Pd, z, dpool, None, bn_p, pool_idx=idx)
    torch.cuda.synchronize()
    pref = R.bwd_ref(x16.double(), *P, z=zc.double(), dy=dpool.cpu(), out_bn=bpr, bf16_gemm=ci == 64, pool_idx=ic)
    wp = check_grads(f'P {tag}', pref, dxp, pdw1, pdb1, pdw2, pdb2, None, True, dpool.cpu().double())
    if ci == 16:        # and the instance the step runs: dp_bwd16s<POOLDY>, z recomputed from x
        options('bwd16s', 1)
        r16 = k.dp_bwd(x16.to(DEV), *Pd, z, dpool, None, bn_p, pool_idx=idx)
        torch.cuda.synchronize()
        pref16 = R.bwd_ref(x16.double(), *P, z=None, dy=dpool.cpu(), out_bn=bpr, recompute_z=True, pool_idx=ic)
        wp = max(wp, check_grads(f'P dp_bwd16s {tag}', pref16, *r16, None, True, dpool.cpu().double()))
    print(f'[{tag}] worst error / bound Q {wq:.3g} P {wp:.3g}')


@pytest.mark.parametrize('n,h,w', [(4, 320, 320), (5, 66, 150)])
def test_bf16_stem(n, h, w):
    """stem (matrix cores) with bf16 storage: z within one bf16 ulp per element of the fp64 convolution, BN sums of the
    unrounded values; weight gradients -- the _bf16 entry reading the stored z and the step's yunet_stem_bwd_rz -- at
    the fp32 test's bar (1e-4)"""
    k = K()
    g = torch.Generator().manual_seed(h + w)
    img = torch.rand(n, 3, h, w, generator=g) * 255
    wt, b = torch.randn(16, 3, 3, 3, generator=g) * 0.05, torch.randn(16, generator=g) * 0.1
    st = torch.zeros(32, dtype=torch.float64, device=DEV)
    z16 = k.stem_fwd(img.to(DEV), wt.to(DEV), b.to(DEV), st, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    import torch.nn.functional as F
    zr = F.conv2d(img.double(), wt.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1)
    mag = F.conv2d(img.double(), wt.double().abs(), b.double().abs(), stride=2, padding=1).permute(0, 2, 3, 1)
    R.check_bf16(f'stem z {n}x{h}x{w}', z16.cpu(), zr, mag, 28)
    R.check_fp32(f'stem stats {n}x{h}x{w}', st, R.stats_of(zr), 2e-5)
    gam, bet = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g) * .2
    dy = torch.randn(zr.shape, generator=g).double()
    cnt = n * (h // 2) * (w // 2)
    for name, zz, rz in (('stored z', z16.cpu().double(), False), ('recomputed z', zr, True)):
        bnr = R.BNRef(st.cpu(), gam, bet, cnt)
        xh = bnr.xhat(zz)
        bst = torch.cat([dy.sum((0, 1, 2)), (dy * xh).sum((0, 1, 2))])
        mean, inv = bnr.mean_invstd()
        dz = gam.double() * inv * (dy - bst[:16] / cnt - xh * bst[16:] / cnt)
        wl = wt.double().clone().requires_grad_(True)
        (F.conv2d(img.double(), wl, None, stride=2, padding=1) * dz.permute(0, 3, 1, 2)).sum().backward()
        bn = k.BN(st, gam.to(DEV), bet.to(DEV), cnt, bstats=bst.to(DEV))
        if rz:
            dw, db = k.stem_bwd(img.to(DEV), z16.float(), dy.float().to(DEV), bn, wt.to(DEV), b.to(DEV))
        else:
            dw, db = k.stem_bwd(img.to(DEV), z16, dy.float().to(DEV), bn)
        torch.cuda.synchronize()
        R.check_fp32(f'stem dw {name} {n}x{h}x{w}', dw, wl.grad, 1e-4)
        assert float(db.abs().max()) < 1e-3 * float(dy.abs().sum())


def test_bf16_fwd_group():
    """yunet_dp_fwd_group_bf16: three independent plain 64 -> 64 units in one grid (the share convs of the pyramid
    levels) -- each against its fp64 reference, and bit-identical to its own launch"""
    import ctypes as C
    import yunet_amd._lib as L
    k = K()
    g = torch.Generator().manual_seed(8)
    units, keep, refs = [], [], []
    for (n, h, w) in [(40, 80, 80), (40, 40, 40), (40, 20, 20)]:
        x16 = (torch.randn(n, h, w, 64, generator=g) * 2 + 0.5).to(torch.bfloat16)
        W = make_unit(64, 64, g)
        Wd = [t.to(DEV).contiguous() for t in W]
        gi, bi = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * .2
        sx = R.stats_of(x16.double())
        ib = k.BN(sx.to(DEV), gi.to(DEV), bi.to(DEV), n * h * w)
        ob = k.BN(torch.zeros(128, dtype=torch.float64, device=DEV), torch.ones(64, device=DEV),
                  torch.zeros(64, device=DEV), n * h * w)
        xg = x16.to(DEV)
        z = torch.empty(n, h, w, 64, device=DEV, dtype=torch.bfloat16)
        d = k._dp_desc(xg, *Wd, z, ib, ob)
        units.append(d)
        keep.append((xg, Wd, ib, ob, z))
        refs.append((R.fwd_ref(x16.double(), *W, in_bn=R.BNRef(sx, gi, bi, n * h * w), bf16_gemm=True), xg, Wd, ib))
    arr = (C.POINTER(L.YunetDP) * 3)(*[C.pointer(d) for d in units])
    L.check(L.load().yunet_dp_fwd_group_bf16(arr, 3, k._stream()), 'yunet_dp_fwd_group_bf16')
    torch.cuda.synchronize()
    for (fr, xg, Wd, ib), (_, _, _, _, z) in zip(refs, keep):
        R.check_bf16(f'group z {tuple(z.shape)}', z.cpu(), fr['z'], fr['mag'], fr['terms'], fr['amb'])
        alone = k.dp_fwd(xg, *Wd, ib, None)
        torch.cuda.synchronize()
        assert torch.equal(alone.cpu().view(torch.int16), z.cpu().view(torch.int16))
