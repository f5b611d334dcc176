"""-m gpu: the descriptor fields of yunet_dp_fwd / yunet_dp_bwd that the dense, dx-overwriting kernel tests never set --
accumulate_dx, z_img_stride above dense (a pyramid level inside the heads' [N, P, 16] output), x_img_stride above dense,
dx == NULL -- per kernel instance, at the smallest shapes that select it.

Every case is checked twice:
  * the plain launch (dense tensors, dx overwritten) of the SAME instance against fp64 autograd through
    [BN + ReLU ->] conv1x1 -> dw3x3 [-> BN + ReLU], at the bars of tests/test_kernels_gpu.py (forward 2e-5, 8e-5 per
    channel; backward 5e-5, 4x per channel; 2e-5 under bwd_fp32mma = 1; bf16 storage: the checkers of tests/bf16_ref.py);
  * every other launch against that plain launch: strides change addresses only, so z, dx and the reduced weight and
    bias gradients are equal bit for bit, the BatchNorm sums (fp64 atomics in any order) to 1e-12; an accumulating launch
    gives base + dx_plain bit for bit (one fp32 add per element) with the same sums, whatever `base` holds.
Bit-equality held for every instance below; no case uses another bar.

Strided buffers come from tests/dp_layout.py: N * stride elements, strides that are no multiple of the dense size
(dense + 4 and dense + 1028 floats; 8 / 1032 elements where x is bf16, so that images stay 16-byte aligned), input gaps
(x, z, dy, the other levels' rows of dflat) NaN, output gaps (z, dx, the other levels' rows of flat) a sentinel that must
come back bit for bit.

The id of a case names the instance yunet_dp_bwd (csrc/dp_route.h: dp_bwd_route) sends it to; assert_route() proves the
route from what the host can see: yunet_dp_bwd_reads_z, yunet_dp_pool_fusion_ok and yunet_dp_bwd_blocks against the tile
count of the instance's tile, and yunet_dp_route, which names the instance.  assert_fwd_route() holds the option values and
the shape rules of dp_fwd_route that the forward ids assume, and asks yunet_dp_route for the name as well."""
import contextlib
import ctypes as C
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import bf16_ref as R
import dp_layout as D
from route_cases import route as dp_route
from test_bf16_kernels_gpu import check_grads as bf16_check_grads
from test_kernels_gpu import bn_ref, mk_unit, nchw, nhwc, rel_err, rel_err_ch, stats_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16 = torch.float32, torch.bfloat16
SENT = D.SENTINEL[F32]


def K():
    import yunet_amd.kernels as k
    return k


def lib():
    import yunet_amd._lib as L
    return L


@contextlib.contextmanager
def options(opts):
    L = lib()
    prev = {name: L.set_option(name, v) for name, v in (opts or {}).items()}
    try:
        yield
    finally:
        for name, v in prev.items():
            L.set_option(name, v)


def ceil(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ cases
# id -> (cin, cout, (N, H, W), keywords).  kind: the instance the DEFAULT dispatch reaches (with accumulate_dx where
# `acc_route` says that only an accumulating launch gets there); mode: input / output BatchNorm (heads: no output BN, a
# random dy_scale); opts: dispatcher options the case runs under; tol: the max-norm bar against fp64.
def _c(cin, cout, shape, kind, **kw):
    return dict(cin=cin, cout=cout, shape=shape, kind=kind, **kw)


BWD = {
    # dp_bwd_kernel<ci, co, 8, 16>: ragged (12 x 20) and whole-tile FULL (8 x 16) instances
    'tile-16x16-ragged': _c(16, 16, (2, 12, 20), 'tile'),
    'tile-16x32-ragged': _c(16, 32, (2, 12, 20), 'tile'),
    'tile-16x32-FULL': _c(16, 32, (2, 8, 16), 'tile'),
    'tile-16x64-ragged': _c(16, 64, (2, 12, 20), 'tile'),
    'tile-16x64-ragged-id_bn': _c(16, 64, (2, 12, 20), 'tile', mode='id_bn'),
    'tile-16x64-FULL': _c(16, 64, (2, 8, 16), 'tile'),
    'tile-32x32-ragged': _c(32, 32, (2, 12, 20), 'tile'),
    'tile-32x32-FULL': _c(32, 32, (2, 8, 16), 'tile'),
    'tile-32x64-split-ragged': _c(32, 64, (2, 12, 20), 'tile'),
    'tile-32x64-split-FULL': _c(32, 64, (2, 8, 16), 'tile'),
    'tile-32x64-fp32-ragged': _c(32, 64, (2, 12, 20), 'tile', opts={'bwd32_split': 0}),
    'tile-32x64-fp32-FULL': _c(32, 64, (2, 8, 16), 'tile', opts={'bwd32_split': 0}),
    # dp_bwd_kernel<16, 16, 16, 32>: a big-tile 16 -> 16 unit leaves the wave-streaming kernel when it accumulates
    'big16-FULL': _c(16, 16, (1, 32, 64), 'big16', acc_route=True),
    'big16-ragged': _c(16, 16, (1, 40, 72), 'big16', acc_route=True),
    'big16-pooled': _c(16, 16, (1, 32, 64), 'big16', acc_route=True, pooled=True),
    # dp_bwd64 (conv_bwd64.hip)
    'bwd64-8w': _c(64, 64, (3, 16, 32), 'bwd64-8w'),
    'bwd64-8w-ragged': _c(64, 64, (2, 12, 20), 'bwd64-8w'),
    'bwd64-8w-ragged-id_bn': _c(64, 64, (2, 12, 20), 'bwd64-8w', mode='id_bn'),
    'bwd64-4w': _c(64, 64, (2, 16, 24), 'bwd64-4w'),
    'bwd64-packed-5x10': _c(64, 64, (5, 10, 10), 'bwd64-packed'),
    'bwd64-packed-19x10': _c(64, 64, (19, 10, 10), 'bwd64-packed'),
    'bwd64-packed-4x20': _c(64, 64, (4, 20, 20), 'bwd64-packed'),
    'bwd64-pooled': _c(64, 64, (1, 2, 2), 'bwd64-8w', pooled=True),      # the smallest shape yunet_dp_pool_fusion_ok takes
    'bwd64-fp32mma-tile': _c(64, 64, (2, 12, 20), 'tile', opts={'bwd_fp32mma': 1}, tol=2e-5),
    'bwd64-fp32mma-packed': _c(64, 64, (5, 10, 10), 'tile-packed', opts={'bwd_fp32mma': 1}, tol=2e-5),
    # dp_bwd_kernel<64, 16, 8, 16>: the fused heads (no output BN, dy_scale), unpacked and on the packed canvas
    'head-unpacked': _c(64, 16, (2, 12, 20), 'tile', mode='bn_nobn'),
    'head-packed-5x10': _c(64, 16, (5, 10, 10), 'tile-packed', mode='bn_nobn'),
    'head-packed-19x10': _c(64, 16, (19, 10, 10), 'tile-packed', mode='bn_nobn'),
    'head-packed-4x20': _c(64, 16, (4, 20, 20), 'tile-packed', mode='bn_nobn'),
    # dp_bwd16s (conv_bwd16.hip): refuses accumulation by design
    'bwd16s-FULL': _c(16, 16, (1, 32, 64), 'bwd16s'),
    'bwd16s-ragged': _c(16, 16, (3, 40, 72), 'bwd16s'),
    'bwd16s-ragged-id_bn': _c(16, 16, (3, 40, 72), 'bwd16s', mode='id_bn'),     # (dp_bwd_streams16 ignores in_transform)
    # walks: more tiles than workgroups -- the next tile's prefetch is in flight while `dx +=` reads the old dx
    'walk-tile-16x64': _c(16, 64, (9, 64, 64), 'tile', walk=True),
    'walk-bwd64-8w': _c(64, 64, (9, 64, 64), 'bwd64-8w', walk=True),
    'walk-bwd64-4w': _c(64, 64, (10, 64, 56), 'bwd64-4w', walk=True),
    'walk-bwd64-packed': _c(64, 64, (70, 20, 20), 'bwd64-packed', walk=True),
    # bf16 activation storage
    'bf16-head-unpacked': _c(64, 16, (2, 12, 20), 'tile', mode='bn_nobn', bf16=True),
    'bf16-head-packed-5x10': _c(64, 16, (5, 10, 10), 'tile-packed', mode='bn_nobn', bf16=True),
    'bf16-head-packed-19x10': _c(64, 16, (19, 10, 10), 'tile-packed', mode='bn_nobn', bf16=True),
    'bf16-head-packed-4x20': _c(64, 16, (4, 20, 20), 'tile-packed', mode='bn_nobn', bf16=True),
    'bf16-bwd64-8w': _c(64, 64, (3, 16, 32), 'bwd64-8w', bf16=True),
    'bf16-bwd64-packed': _c(64, 64, (5, 10, 10), 'bwd64-packed', bf16=True),
    'bf16-tile-16x64': _c(16, 64, (2, 12, 20), 'tile', bf16=True),
}
HEADS = [i for i, c in BWD.items() if c['cout'] == 16 and c['cin'] == 64]
WALKS = [i for i, c in BWD.items() if c.get('walk')]
NOT_WALKS = [i for i in BWD if i not in WALKS]
ACCUMULATING = [i for i, c in BWD.items() if c['kind'] != 'bwd16s']
NO_DX = ['tile-16x64-ragged', 'tile-32x64-split-FULL', 'big16-ragged', 'bwd64-8w', 'bwd64-4w', 'bwd64-packed-5x10',
         'bwd64-fp32mma-tile', 'head-unpacked', 'head-packed-5x10', 'bf16-bwd64-8w']


def note(family, name, err, bar):
    """print an error against fp64 next to its bar (pytest -s shows the lines) and hand it back for the assertion"""
    print(f'[descriptor fp64] {family:14s} {name:10s} {err:.3g} (bar {bar:.3g})')
    return err


class Case(types.SimpleNamespace):
    pass


def off_the_relu_threshold(x32, gi, bi, bf16, margin=1e-4):
    """dx = mask * da is discontinuous at bn(x) = 0: an element whose fp64 bn(x) lies within fp32 rounding of zero may take
    the other branch in the kernel's fp32 arithmetic, an error of the size of da itself that says nothing about the kernel.
    So the inputs keep |bn(x)| >= `margin`: elements nearer than that move 0.05 up.  bn(x) is O(1) here and the kernels
    round it to about 1e-7, so the margin is 1000x that rounding and moves about one element in 10^4; a kernel whose mask
    is wrong by more than rounding still flips elements beyond the margin, and everything but the mask is compared on
    every element as before, so the margin hides no kernel error.  (With in_transform = IDENTITY there is no mask and the
    helper is not called.)"""
    for _ in range(8):
        near = bn_ref(x32.double(), gi.double(), bi.double())[0].abs() < margin
        if not bool(near.any()):
            return x32
        x32 = torch.where(near, x32 + 0.05, x32)
        x32 = x32.to(BF16).float() if bf16 else x32
    raise AssertionError('could not move the input off the ReLU threshold')


@functools.lru_cache(maxsize=None)
def case(cid, table='bwd'):
    """The inputs of one case on the device and its fp64 reference, built once and never modified."""
    spec = (BWD if table == 'bwd' else FWD)[cid]
    cin, cout, (n, h, w) = spec['cin'], spec['cout'], spec['shape']
    mode, bf16, pooled = spec.get('mode', 'bn_bn'), spec.get('bf16', False), spec.get('pooled', False)
    in_on, out_on = mode.startswith('bn'), mode.endswith('_bn')
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + n + h + w)
    c = Case(id=cid, spec=spec, cin=cin, cout=cout, n=n, h=h, w=w, in_on=in_on, out_on=out_on, bf16=bf16,
             kind=spec['kind'], opts=spec.get('opts'), tol=spec.get('tol', 5e-5), cnt=n * h * w,
             family=('bf16 ' if bf16 else '') + spec['kind'])
    x32 = torch.randn(n, cin, h, w, generator=g) * 2 + 0.5
    x32 = x32.to(BF16).float() if bf16 else x32
    unit = mk_unit(cin, cout, g)
    gi, bi = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * .2
    if in_on:
        x32 = off_the_relu_threshold(x32, gi, bi, bf16)
    go, bo = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * .2
    r = torch.randn(n, cout, h, w, generator=g).double()
    scale = torch.rand(cout, generator=g) + 0.5
    idx = None
    if pooled:      # the unit feeds max_pool2d only: the gradient reaches one recorded position per 2 x 2 window
        idx = torch.randint(0, 4, (n, h // 2, w // 2, cout), generator=g, dtype=torch.uint8)
        r = r * nchw(R.expand_pooled(torch.ones(n, h // 2, w // 2, cout), idx))
    c.base = (torch.randn(n, h, w, cin, generator=g) * 100).to(DEV)
    c.W = [unit[0].view(cout, cin).contiguous().to(DEV), unit[1].to(DEV), unit[2].view(cout, 9).contiguous().to(DEV),
           unit[3].to(DEV)]
    c.gi, c.bi, c.go, c.bo = gi.to(DEV), bi.to(DEV), go.to(DEV), bo.to(DEV)
    c.x = nhwc(x32).to(BF16 if bf16 else F32).to(DEV)
    c.sx = stats_of(nhwc(x32)).to(DEV)
    c.idx = idx.to(DEV) if pooled else None
    c.dy_scale = None if out_on else scale.to(DEV)
    if bf16:
        return _bf16_reference(c, nhwc(x32).double(), [unit[0].view(cout, cin), unit[1], unit[2].view(cout, 9), unit[3]],
                               gi, bi, go, bo, nhwc(r), scale)
    # ---- fp64 autograd, as tests/test_kernels_gpu.py:_dp_bwd_case
    x = x32.double()
    w_pw, b_pw, w_dw, b_dw = [t.double().requires_grad_(True) for t in unit]
    if in_on:
        b_in, xhat_in = bn_ref(x, gi.double(), bi.double())
        b_in = b_in.detach().requires_grad_(True)
        a = F.relu(b_in)
    else:
        b_in = x.clone().requires_grad_(True)
        a = b_in
    z = F.conv2d(F.conv2d(a, w_pw, b_pw), w_dw, b_dw, padding=1, groups=cout)
    if out_on:
        zb, xhat_out = bn_ref(z, go.double(), bo.double())
        zb.retain_grad()
        (F.relu(zb) * r).sum().backward()
        dy = zb.grad                                    # grad wrt the BN output, ReLU mask applied
        c.bst = torch.cat([dy.sum(dim=(0, 2, 3)), (dy * xhat_out.detach()).sum(dim=(0, 2, 3))]).to(DEV).contiguous()
    else:
        (z * r * scale.double().view(1, -1, 1, 1)).sum().backward()
        dy = r
        c.bst = None
    dyn = nhwc(dy)
    c.zref = nhwc(z.detach())
    c.z = c.zref.float().to(DEV)
    c.sz = stats_of(c.z)
    c.dy_sum = float(dy.abs().sum())
    if pooled:      # what the pool's consumer wrote: the gradient of every window's recorded element
        c.dy = torch.gather(R.windows(dyn), -1, idx.long().unsqueeze(-1)).squeeze(-1).float().contiguous().to(DEV)
    else:
        c.dy = dyn.float().contiguous().to(DEV)
    c.ref = dict(dx=nhwc(b_in.grad), dw1=w_pw.grad.reshape(cout, cin), db1=b_pw.grad, dw2=w_dw.grad.reshape(cout, 9),
                 db2=b_dw.grad)
    if in_on:
        c.ref['bst'] = torch.cat([b_in.grad.sum(dim=(0, 2, 3)), (b_in.grad * xhat_in).sum(dim=(0, 2, 3))])
    return c


def _bf16_reference(c, x64, W, gi, bi, go, bo, dy, scale):
    """bf16 storage: the contract of tests/bf16_ref.py (the stored z is the reference forward rounded to bf16)"""
    gemm = c.cin % 32 == 0
    in_ref = R.BNRef(c.sx.cpu(), gi, bi, c.cnt) if c.in_on else None
    c.fr = R.fwd_ref(x64, *W, in_bn=in_ref, bf16_gemm=gemm)
    head = not c.out_on
    z16 = c.fr['z'].float() if head else c.fr['z'].to(BF16)
    c.z = z16.to(DEV)
    c.sz = R.stats_of(c.fr['z']).to(DEV)
    ob = None
    c.bst = None
    if c.out_on:
        ob = R.BNRef(c.sz.cpu(), go, bo, c.cnt)
        ob.bstats = torch.cat([dy.sum((0, 1, 2)), (dy * ob.xhat(z16.double())).sum((0, 1, 2))])
        c.bst = ob.bstats.to(DEV)
    c.dy = dy.float().contiguous().to(DEV)
    c.dy_sum = float(dy.abs().sum())
    c.br = R.bwd_ref(x64, *W, z=z16.double(), dy=dy.float().double(), in_bn=in_ref, out_bn=ob,
                     dy_scale=None if c.out_on else scale, bf16_gemm=c.cin == 64 and c.cout == 64)
    return c


def check_fp64(c, r):
    """the plain launch's gradients against the case's fp64 reference, at the project's bars"""
    if c.bf16:
        w = bf16_check_grads(c.id, c.br, r['dx'], r['dw1'], r['db1'], r['dw2'], r['db2'],
                             types.SimpleNamespace(bstats=r['bst']) if c.in_on else None, c.out_on,
                             torch.tensor(c.dy_sum).view(1), tol=c.tol)
        note(c.family, 'err/bound', w, 1.0)
        return
    ref, tol = c.ref, c.tol
    assert note(c.family, 'dx', rel_err(r['dx'], ref['dx']), tol) < tol
    assert note(c.family, 'dx/ch', rel_err_ch(r['dx'], ref['dx'], dim=3), 4 * tol) < 4 * tol
    assert note(c.family, 'dw1', rel_err(r['dw1'], ref['dw1']), tol) < tol
    assert note(c.family, 'dw1/ch', rel_err_ch(r['dw1'].reshape(c.cout, c.cin), ref['dw1'], dim=0), 4 * tol) < 4 * tol
    assert note(c.family, 'db1', rel_err(r['db1'], ref['db1']), tol) < tol
    assert note(c.family, 'dw2', rel_err(r['dw2'], ref['dw2']), tol) < tol
    if c.out_on:        # with BN behind the unit the depthwise-bias gradient is identically zero (noise only)
        assert float(r['db2'].abs().max()) < 1e-3 * c.dy_sum
    else:
        assert note(c.family, 'db2', rel_err(r['db2'], ref['db2']), tol) < tol
    if c.in_on:
        assert note(c.family, 'in bstats', rel_err(r['bst'], ref['bst']), tol) < tol


# ------------------------------------------------------------------------------------------------ launches
def gap(c, which):
    """extra elements per image: two strides that are no multiple of the dense size, images 16-byte aligned"""
    return {'small': 8 if c.bf16 else 4, 'large': 1032 if c.bf16 else 1028}[which]


def flat_levels(c, later):
    """(P, first row) of a three-level [N, P, 16] head output in which the case's level comes first or second"""
    rows = c.h * c.w
    return (rows + 60 + 15, 0) if not later else (100 + rows + 25, 100)


def bn_pair(c, bst0=None):
    k = K()
    in_bn = out_bn = None
    if c.in_on:
        b = torch.zeros(2 * c.cin, dtype=torch.float64, device=DEV) if bst0 is None else bst0.clone()
        in_bn = k.BN(c.sx, c.gi, c.bi, c.cnt, bstats=b)
    if c.out_on:
        out_bn = k.BN(c.sz, c.go, c.bo, c.cnt, bstats=c.bst)
    return in_bn, out_bn


def run_bwd(c, xs=0, zs=0, level=None, acc=False, need_dx=True, opts=None, bst0=None):
    """One yunet_dp_bwd launch through flat buffers: xs / zs extra elements per image of x, dx / z, dy; level = (P, base):
    z and dy are a level's rows of a [N, P, 16] buffer.  Gaps are NaN (inputs) or the sentinel (dx, checked here).
    -> dense dx, the reduced gradients, the producer's BN-backward sums."""
    k = K()
    n, h, w, cin, cout = c.n, c.h, c.w, c.cin, c.cout
    xd, zd = h * w * cin, h * w * cout
    xstride = xd + xs
    zstride, zoff = (level[0] * 16, level[1] * 16) if level else (zd + zs, 0)
    x = D.scatter(c.x, xstride)
    z = D.scatter(c.z, zstride, zoff)[zoff:]
    dy = c.dy if c.idx is not None else D.scatter(c.dy, zstride, zoff)[zoff:]        # (a pooled dy is dense)
    dx = None
    if need_dx:
        dx = D.scatter(c.base, xstride, pattern=SENT) if acc else D.filled(n * xstride, F32, DEV, SENT)
    in_bn, out_bn = bn_pair(c, bst0)
    with options({**(c.opts or {}), **(opts or {})}):
        got = k.dp_bwd(x, *c.W, z, dy, in_bn, out_bn, dy_scale=c.dy_scale, dx=dx, accumulate_dx=acc, z_img_stride=zstride,
                       need_dx=need_dx, pool_idx=c.idx, x_img_stride=xstride, shape=(n, h, w))
    torch.cuda.synchronize()
    out = dict(dw1=got[1].reshape(cout, cin), db1=got[2], dw2=got[3].reshape(cout, 9), db2=got[4])
    out['bst'] = in_bn.bstats if c.in_on else None
    if need_dx:
        assert got[0] is dx
        assert D.gaps_hold(dx, n, xstride, xd), (c.id, 'dx: written between the images')
        out['dx'] = D.gather(dx, (n, h, w, cin), xstride)
    else:
        assert got[0] is None
    return out


@functools.lru_cache(maxsize=None)
def plain(cid):
    """the dense, non-accumulating launch of the case's instance (big16: the tile kernel, which a plain launch reaches
    only with the wave-streaming kernel switched off)"""
    c = case(cid)
    return run_bwd(c, opts={'bwd16s': 0} if c.kind == 'big16' else None)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(D.bits(a.contiguous()), D.bits(b.contiguous()))


def assert_same(c, r, acc=False, need_dx=True):
    """a launch against the plain launch of the same instance on the same values"""
    p = plain(c.id)
    if need_dx:
        want = c.base + p['dx'] if acc else p['dx']             # one fp32 add per element, as the kernels read
        assert same_bits(r['dx'], want), (c.id, 'dx', float((r['dx'] - want).abs().max()))
    for name in ('dw1', 'db1', 'dw2', 'db2'):
        assert same_bits(r[name], p[name]), (c.id, name, float((r[name] - p[name]).abs().max()))
    if c.in_on and need_dx:
        assert rel_err(r['bst'], p['bst']) < 1e-12, (c.id, 'in_bn.bstats', rel_err(r['bst'], p['bst']))


def descriptor(c, acc=False, need_dx=True):
    """the YunetDP of a dense backward launch, for the host-side queries"""
    k = K()
    in_bn, out_bn = bn_pair(c)
    d = k._dp_desc(c.x, *c.W, c.z, in_bn, out_bn)
    if c.z.dtype != c.x.dtype:
        d.z_dtype = d.x_dtype
    d.dy, d.dx, d.accumulate_dx = c.dy.data_ptr(), (c.base.data_ptr() if need_dx else None), int(acc)
    d.pool_idx = c.idx.data_ptr() if c.idx is not None else None
    return d, (in_bn, out_bn)


def bwd_tiles(c):
    """tiles of the instance the id names (bwd_grid.h, common.h: make_pack)"""
    n, h, w = c.n, c.h, c.w
    th, tw = {'big16': (16, 32), 'bwd16s': (16, 32), 'bwd64-4w': (8, 8)}.get(c.kind, (8, 16))
    if c.kind.endswith('packed'):
        r = min(n, 16)
        return ceil(r * (w + 1), tw) * ceil(ceil(n, r) * (h + 1), th)
    return n * ceil(w, tw) * ceil(h, th)


def tf(v):
    return 'true' if v else 'false'


def bwd_instance(c, streams):
    """the kernel instance the id of a backward case claims, spelled as the kernel's own name (non-deterministic form);
    a whole-tile map runs the FULL instance where one exists (the exact-fp32 32 -> 64 unit without pooled dy has none)"""
    cin, cout, pooled = c.cin, c.cout, c.idx is not None
    packed = c.kind.endswith('packed')
    if streams:
        return f'dp_bwd16s_kernel<{tf(pooled)},false>'
    if c.kind.startswith('bwd64'):
        return f"dp_bwd64_kernel<{4 if c.kind == 'bwd64-4w' else 8},{tf(packed)},{tf(pooled)},false>"
    th, tw = (16, 32) if c.kind in ('big16', 'bwd16s') else (8, 16)
    opts = c.opts or {}
    split = (cin, cout) == (32, 64) and opts.get('bwd32_split', 1) and not opts.get('bwd_fp32mma', 0)
    full = c.h % th == 0 and c.w % tw == 0 and not packed and (
        th == 16 or split or (pooled and cin == 32) or (not pooled and (cin, cout) in ((16, 32), (16, 64), (32, 32))))
    return f'dp_bwd_kernel<{cin},{cout},{th},{tw},{tf(packed)},{int(bool(split))},{tf(pooled)},{tf(full)},false>'


def assert_route(c):
    """what the host can see of the dispatch: the query that separates the wave-streaming kernel, the fusion query, the
    packed-canvas rule, the whole-tile rule and the grid of the instance's tile; yunet_dp_route names the instance"""
    k, L = K(), lib()
    n, h, w, cin, cout = c.n, c.h, c.w, c.cin, c.cout
    packed = h <= 20 and w <= 20 and n >= 4 and cin == 64
    big = cin == 16 and cout == 16 and w >= 64 and h >= 32
    with options(c.opts):
        for acc, need_dx in ((False, True), (True, True), (False, False)):
            d, keep = descriptor(c, acc, need_dx)
            streams = c.kind in ('bwd16s', 'big16') and not acc and need_dx
            assert L.load().yunet_dp_bwd_reads_z(C.byref(d)) == (0 if streams else 1), (c.id, acc, need_dx)
            d.wgrad_partials, d.wgrad_blocks = c.dy.data_ptr(), k.dp_grid(n, h, w, cin, cout)     # (any buffer: host only)
            assert dp_route(L.load(), d, 1) == bwd_instance(c, streams), (c.id, acc, need_dx)
        if c.kind == 'big16':           # ... and with the option off the plain launch stays on the tile kernel
            with options({'bwd16s': 0}):
                d, keep = descriptor(c)
                assert L.load().yunet_dp_bwd_reads_z(C.byref(d)) == 1
        assert L.load().yunet_dp_pool_fusion_ok(n, h, w, cin, cout) == \
            int(h % 2 == 0 and w % 2 == 0 and (big or (cin == 64 and cout == 64 and not packed) or (cin, cout) == (32, 64)))
        if c.idx is not None:
            assert L.load().yunet_dp_pool_fusion_ok(n, h, w, cin, cout) == 1
        assert packed == c.kind.endswith('packed') and big == (c.kind in ('big16', 'bwd16s')), c.id
        if 'FULL' in c.id:
            assert (h % 16 == 0 and w % 32 == 0) if big else (h % 8 == 0 and w % 16 == 0)
        if 'ragged' in c.id:
            assert not ((h % 16 == 0 and w % 32 == 0) if big else (h % 8 == 0 and w % 16 == 0))
        if c.kind == 'bwd64-4w':
            assert w % 16 != 0 and w % 8 == 0
        if c.kind == 'bwd64-8w':
            assert not (w % 16 != 0 and w % 8 == 0)
        tiles, grid = bwd_tiles(c), k.dp_grid(n, h, w, cin, cout)
        if c.spec.get('walk'):
            assert tiles > grid, (c.id, 'walk shape does not walk', tiles, grid)
            assert grid == (512 if c.kind == 'bwd64-4w' else 256)
        else:
            assert tiles == grid, (c.id, 'grid is not the tile count of the instance', tiles, grid)


# ------------------------------------------------------------------------------------------------ backward tests
@pytest.mark.parametrize('cid', list(BWD))
def test_bwd_route_and_plain_launch_vs_fp64(cid):
    c = case(cid)
    assert_route(c)
    check_fp64(c, plain(cid))


@pytest.mark.parametrize('which', ['small', 'large'])
@pytest.mark.parametrize('cid', NOT_WALKS)
def test_bwd_strided_x_dx(cid, which):
    """x_img_stride above dense: x gaps NaN, dx gaps the sentinel"""
    c = case(cid)
    acc = c.spec.get('acc_route', False)
    assert_same(c, run_bwd(c, xs=gap(c, which), acc=acc), acc=acc)


@pytest.mark.parametrize('which', ['small', 'large'])
@pytest.mark.parametrize('cid', NOT_WALKS)
def test_bwd_strided_z_dy(cid, which):
    """z_img_stride above dense: z and dy gaps NaN (a pooled dy is dense by contract: only z is strided there)"""
    c = case(cid)
    acc = c.spec.get('acc_route', False)
    assert_same(c, run_bwd(c, zs=gap(c, which), acc=acc), acc=acc)


@pytest.mark.parametrize('later', [False, True], ids=['first-level', 'later-level'])
@pytest.mark.parametrize('cid', HEADS)
def test_head_bwd_reads_its_level_of_dflat(cid, later):
    """the fused heads' backward: dy is a level's rows of dflat [N, P, 16] (z_img_stride = P * 16, base offset, the other
    levels' rows NaN), scaled by a random dy_scale; dense and strided x"""
    c = case(cid)
    assert c.dy_scale is not None and not c.out_on and c.in_on
    lv = flat_levels(c, later)
    assert_same(c, run_bwd(c, level=lv))
    assert_same(c, run_bwd(c, level=lv, xs=gap(c, 'small')))
    assert_same(c, run_bwd(c, level=lv, xs=gap(c, 'large'), acc=True), acc=True)


@pytest.mark.parametrize('cid', ACCUMULATING)
def test_bwd_accumulate_dx(cid):
    """accumulate_dx = 1: dx = base + dx_plain bit for bit (base = randn * 100), the producer's BN-backward sums those of
    the plain launch (the old dx is not summed), weight gradients unchanged -- dense and with every tensor strided"""
    c = case(cid)
    assert_route(c)
    assert_same(c, run_bwd(c, acc=True), acc=True)
    if cid not in HEADS:
        assert_same(c, run_bwd(c, acc=True, xs=gap(c, 'small'), zs=gap(c, 'large')), acc=True)


@pytest.mark.parametrize('cid', NO_DX)
def test_bwd_without_dx(cid):
    """dx == NULL: the weight gradients of the launch with a dx, bit for bit; in_bn.bstats is left untouched (the kernels
    add the producer's sums only where they write dx: include/yunet_hip.h)"""
    c = case(cid)
    bst0 = torch.arange(1, 2 * c.cin + 1, dtype=torch.float64, device=DEV) * 0.37
    opts = {'bwd16s': 0} if c.kind == 'big16' else None
    for strides in (dict(), dict(xs=gap(c, 'small'), zs=gap(c, 'small'))):
        r = run_bwd(c, need_dx=False, bst0=bst0, opts=opts, **strides)
        assert_same(c, r, need_dx=False)
        if c.in_on:
            assert torch.equal(r['bst'], bst0), (cid, strides, 'in_bn.bstats changed without a dx')


def test_bwd_dy_scale_is_ignored_behind_an_output_bn():
    """out_has_bn = 1: the kernels fold the unit's own BN backward into dz and never read dy_scale -- a NaN vector changes
    neither dx nor any weight or bias gradient (a scaled dz reaches db2 and dw2 first) nor the producer's sums"""
    for cid in ('tile-16x64-ragged', 'bwd64-8w'):
        c = case(cid)
        k = K()
        in_bn, out_bn = bn_pair(c)
        poison = torch.full((c.cout,), float('nan'), device=DEV)
        got = k.dp_bwd(c.x, *c.W, c.z, c.dy, in_bn, out_bn, dy_scale=poison)
        torch.cuda.synchronize()
        assert c.in_on and c.out_on
        assert_same(c, dict(dx=got[0], dw1=got[1].reshape(c.cout, c.cin), db1=got[2], dw2=got[3].reshape(c.cout, 9),
                            db2=got[4], bst=in_bn.bstats))


# ------------------------------------------------------------------------------------------------ forward
FWD = {
    # dp_fwd_kernel<ci, co, 8, 16>
    'tile-16x32': _c(16, 32, (2, 12, 20), 'fwd tile'),
    'tile-32x32': _c(32, 32, (2, 12, 20), 'fwd tile'),
    'tile-32x64': _c(32, 64, (2, 12, 20), 'fwd tile', mode='id_bn'),
    'tile-32x64-pool': _c(32, 64, (2, 12, 20), 'fwd tile', pool=True),
    'tile-64x64': _c(64, 64, (2, 12, 20), 'fwd tile', opts={'fwd64s': 0}),
    'tile-64x16': _c(64, 16, (2, 12, 20), 'fwd tile', mode='bn_nobn'),
    # dp_fwd16s (conv_fwd16.hip)
    'fwd16s-16x16-a': _c(16, 16, (1, 32, 64), 'fwd16s'),
    'fwd16s-16x16-b': _c(16, 16, (2, 16, 32), 'fwd16s'),
    'fwd16s-16x64-a': _c(16, 64, (1, 32, 64), 'fwd16s'),
    'fwd16s-16x64-b': _c(16, 64, (2, 16, 32), 'fwd16s', mode='id_bn'),
    # dp_fwd64s (conv_fwd64.hip), the packed levels too under the default fwd64s = 2
    'fwd64s': _c(64, 64, (3, 16, 32), 'fwd64s'),
    'fwd64s-ragged': _c(64, 64, (2, 12, 20), 'fwd64s'),
    'fwd64s-ragged-id_bn': _c(64, 64, (2, 12, 20), 'fwd64s', mode='id_bn'),
    'fwd64s-level-5x10': _c(64, 64, (5, 10, 10), 'fwd64s'),
    'fwd64s-level-4x20': _c(64, 64, (4, 20, 20), 'fwd64s'),
    # packed canvas: dp_fwd_kernel<64, 64 | 16, 8, 16, PACKED>
    'packed-64x64-5x10': _c(64, 64, (5, 10, 10), 'fwd packed', opts={'fwd64s': 1}),
    'packed-64x64-19x10': _c(64, 64, (19, 10, 10), 'fwd packed', opts={'fwd64s': 1}),
    'packed-64x64-4x20': _c(64, 64, (4, 20, 20), 'fwd packed', opts={'fwd64s': 1}),
    'packed-64x16-5x10': _c(64, 16, (5, 10, 10), 'fwd packed', mode='bn_nobn'),
    'packed-64x16-19x10': _c(64, 16, (19, 10, 10), 'fwd packed', mode='bn_nobn'),
    'packed-64x16-4x20': _c(64, 16, (4, 20, 20), 'fwd packed', mode='bn_nobn'),
    # bf16 x, fp32 z: the heads
    'bf16-head-unpacked': _c(64, 16, (2, 12, 20), 'fwd tile', mode='bn_nobn', bf16=True),
    'bf16-head-packed-5x10': _c(64, 16, (5, 10, 10), 'fwd packed', mode='bn_nobn', bf16=True),
    'bf16-head-packed-19x10': _c(64, 16, (19, 10, 10), 'fwd packed', mode='bn_nobn', bf16=True),
    'bf16-head-packed-4x20': _c(64, 16, (4, 20, 20), 'fwd packed', mode='bn_nobn', bf16=True),
}
FWD_HEADS = [i for i, c in FWD.items() if c['cout'] == 16]


def option(name):
    """the current value of a dispatcher option (set_option hands back the previous one)"""
    L = lib()
    v = L.set_option(name, 0)
    L.set_option(name, v)
    return v


def assert_fwd_route(c):
    """The ids rely on dp_fwd_route (csrc/dp_route.h), non-deterministic BN sums, no prof, in this order: `fwd16s` (option
    fwd16s != 0: every 16 -> 16 / 16 -> 64 unit, the pooled 16 -> 64 excepted), the fused-pool branch (32 -> 64: the tile
    kernel), the packed-canvas line (dp_use_pack: N >= 4, H, W <= 20, cin = 64 -- except the 64 -> 64 unit with
    activation-typed z under fwd64s >= 2), the fwd64s line (64 -> 64, fwd64s != 0), the tile instances.
    Hold the option values and the shape rules the kinds assume, so that a changed default shows up here."""
    n, h, w, cin, cout = c.n, c.h, c.w, c.cin, c.cout
    with options(c.opts):
        fwd16s, fwd64s = option('fwd16s'), option('fwd64s')
        assert fwd64s == (c.opts or {}).get('fwd64s', 2), (c.id, 'the default of option fwd64s is no longer 2')
        use_pack = n >= 4 and h <= 20 and w <= 20 and cin == 64
        want = ('fwd16s' if cin == 16 and cout in (16, 64) and fwd16s and not c.spec.get('pool') else
                'fwd packed' if use_pack and not (cout == 64 and fwd64s >= 2) else
                'fwd64s' if cin == 64 and cout == 64 and fwd64s and not c.spec.get('pool') else 'fwd tile')
        assert c.kind == want, (c.id, c.kind, want, fwd16s, fwd64s)
        # ... and yunet_dp_route names that instance (the descriptor of a dense launch; host only)
        k, pool = K(), bool(c.spec.get('pool'))
        in_bn = k.BN(c.sx, c.gi, c.bi, c.cnt) if c.in_on else None
        out_bn = k.BN(torch.zeros(2 * cout, dtype=torch.float64, device=DEV), c.go, c.bo, c.cnt) if c.out_on else None
        z = torch.empty(n, h, w, cout, device=DEV, dtype=c.x.dtype if c.out_on else F32)
        d = k._dp_desc(c.x, *c.W, z, in_bn, out_bn)
        if pool:
            d.pool_out = d.pool_idx = z.data_ptr()
        name = {'fwd16s': f'dp_fwd16s_kernel<{cout},{tf(pool)},false>', 'fwd64s': f'dp_fwd64s_kernel<{tf(pool)},false>',
                'fwd packed': f'dp_fwd_kernel<{cin},{cout},8,16,true,false,false>',
                'fwd tile': f'dp_fwd_kernel<{cin},{cout},8,16,false,{tf(pool)},false>'}[c.kind]
        assert dp_route(lib().load(), d, 0) == name, (c.id, name)


def run_fwd(c, xs=0, zs=0, level=None):
    """One yunet_dp_fwd launch through flat buffers (run_bwd's layout); the z gaps are the sentinel, checked here.
    -> dense z, the output BN sums, (pooled, idx) of a fused-pool unit."""
    k = K()
    n, h, w, cin, cout = c.n, c.h, c.w, c.cin, c.cout
    xd, zd = h * w * cin, h * w * cout
    xstride = xd + xs
    zstride, zoff = (level[0] * 16, level[1] * 16) if level else (zd + zs, 0)
    x = D.scatter(c.x, xstride)
    zdt = F32 if not c.out_on else c.x.dtype                # the heads write fp32
    zbuf = D.filled(n * zstride, zdt, DEV, D.SENTINEL[zdt])
    in_bn = k.BN(c.sx, c.gi, c.bi, c.cnt) if c.in_on else None
    st = torch.zeros(2 * cout, dtype=torch.float64, device=DEV)
    out_bn = k.BN(st, c.go, c.bo, c.cnt) if c.out_on else None
    pool = c.spec.get('pool', False)
    with options(c.opts):
        got = k.dp_fwd(x, *c.W, in_bn, out_bn, z=zbuf[zoff:], z_img_stride=zstride, pool=pool, x_img_stride=xstride,
                       shape=(n, h, w))
    torch.cuda.synchronize()
    assert D.gaps_hold(zbuf, n, zstride, zd, zoff), (c.id, 'z: written outside the level / between the images')
    out = dict(z=D.gather(zbuf, (n, h, w, cout), zstride, zoff), stats=st if c.out_on else None)
    if pool:
        out['pooled'], out['idx'] = got[1], got[2]
    return out


@functools.lru_cache(maxsize=None)
def plain_fwd(cid):
    return run_fwd(case(cid, 'fwd'))


def assert_same_fwd(c, r):
    p = plain_fwd(c.id)
    assert same_bits(r['z'], p['z']), (c.id, 'z')
    if c.out_on:
        assert rel_err(r['stats'], p['stats']) < 1e-12, (c.id, 'out_bn.stats')
    if 'pooled' in p:
        assert same_bits(r['pooled'], p['pooled']) and torch.equal(r['idx'], p['idx'])


def check_fwd_fp64(c, r):
    if c.bf16:
        w = R.check_bf16(c.id, r['z'], c.fr['z'], c.fr['mag'], c.fr['terms'], c.fr['amb'], stored='fp32')
        note('bf16 ' + c.kind, 'err/bound', w, 1.0)
        return
    assert note(c.kind, 'z', rel_err(r['z'], c.zref), 2e-5) < 2e-5
    assert note(c.kind, 'z/ch', rel_err_ch(r['z'], c.zref, dim=3), 8e-5) < 8e-5
    if c.out_on:
        assert note(c.kind, 'out stats', rel_err(r['stats'], stats_of(c.zref)), 2e-5) < 2e-5
    if 'pooled' in r:       # the winners are the stored values at idx, bit for bit, and idx follows the first-maximum rule
        R.check_pool(c.id, r['z'].cpu(), r['pooled'].cpu(), r['idx'].cpu(), c.go.cpu())


@pytest.mark.parametrize('cid', list(FWD))
def test_fwd_strided(cid):
    """the plain launch against fp64; strided x, strided z and both against the plain launch, gaps intact"""
    c = case(cid, 'fwd')
    assert_fwd_route(c)
    check_fwd_fp64(c, plain_fwd(cid))
    for which in ('small', 'large'):
        assert_same_fwd(c, run_fwd(c, xs=gap(c, which)))
        assert_same_fwd(c, run_fwd(c, zs=gap(c, which)))
    assert_same_fwd(c, run_fwd(c, xs=gap(c, 'large'), zs=gap(c, 'small')))


@pytest.mark.parametrize('later', [False, True], ids=['first-level', 'later-level'])
@pytest.mark.parametrize('cid', FWD_HEADS)
def test_head_fwd_writes_its_level_of_flat(cid, later):
    """the fused heads' forward: fp32 z straight into a level's rows of flat [N, P, 16] (from fp32 and from bf16 x); the
    other levels' rows keep the sentinel"""
    c = case(cid, 'fwd')
    lv = flat_levels(c, later)
    r = run_fwd(c, level=lv)
    assert r['z'].dtype == F32
    assert_same_fwd(c, r)
    assert_same_fwd(c, run_fwd(c, level=lv, xs=gap(c, 'small')))


def test_an_ablation_mask_leaves_the_group():
    """needs no launch: a 64 -> 64 unit whose prof is an ablation mask (< 64) routes to dp_fwd64s on its own, as without
    the mask; yunet_dp_fwd_group puts into one grid only units with that route AND a NULL prof, so a group with this unit
    goes out one by one: yunet_dp_fwd_group_one_grid, the predicate the entry branches on, says so (tests/test_dp_route.py
    holds it against the recorded entry over every triple)"""
    k, c = K(), case('fwd64s', 'fwd')
    st = torch.zeros(128, dtype=torch.float64, device=DEV)
    d = k._dp_desc(c.x, *c.W, torch.empty(c.n, c.h, c.w, 64, device=DEV), k.BN(c.sx, c.gi, c.bi, c.cnt),
                   k.BN(st, c.go, c.bo, c.cnt))
    L = lib()
    plain = dp_route(L.load(), d, 0)
    q = L.load().yunet_dp_fwd_group_one_grid
    pair = (C.POINTER(L.YunetDP) * 2)(C.pointer(d), C.pointer(d))
    assert q(pair, 2) == 1
    d.prof = 1
    assert plain == dp_route(L.load(), d, 0) == 'dp_fwd64s_kernel<false,false>'
    assert q(pair, 2) == 0


def test_fwd_group_of_three_strided_units():
    """yunet_dp_fwd_group over three independent 64 -> 64 units, every one with strided x and z: each equals its own dense
    launch bit for bit, sums to 1e-12, gaps intact"""
    k, L = K(), lib()
    ids = ['fwd64s', 'fwd64s-ragged', 'fwd64s-level-5x10']
    units, keep = [], []
    for j, cid in enumerate(ids):
        c = case(cid, 'fwd')
        xs, zs = gap(c, 'small' if j % 2 else 'large'), gap(c, 'large' if j % 2 else 'small')
        xd = zd = c.h * c.w * 64
        x = D.scatter(c.x, xd + xs)
        zbuf = D.filled(c.n * (zd + zs), F32, DEV, SENT)
        st = torch.zeros(128, dtype=torch.float64, device=DEV)
        in_bn, out_bn = k.BN(c.sx, c.gi, c.bi, c.cnt), k.BN(st, c.go, c.bo, c.cnt)
        units.append(k._dp_desc(x, *c.W, zbuf, in_bn, out_bn, xd + xs, zd + zs, (c.n, c.h, c.w)))
        keep.append((c, x, zbuf, st, in_bn, out_bn, zd + zs))
    arr = (C.POINTER(L.YunetDP) * 3)(*[C.pointer(d) for d in units])
    L.check(L.load().yunet_dp_fwd_group(arr, 3, k._stream()), 'yunet_dp_fwd_group')
    torch.cuda.synchronize()
    for c, x, zbuf, st, _, _, zstride in keep:
        assert D.gaps_hold(zbuf, c.n, zstride, c.h * c.w * 64)
        r = dict(z=D.gather(zbuf, (c.n, c.h, c.w, 64), zstride), stats=st)
        assert_same_fwd(c, r)
        check_fwd_fp64(c, r)
