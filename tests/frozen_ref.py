"""fp64 references of the backward kernels under FROZEN BatchNorm (fine-tuning: engine.py Plan._reader_bn, DESIGN.md
section 12).  Host-only helper module (no GPU, no pytest fixtures); tests/test_frozen_ref.py checks it on the CPU,
tests/test_frozen_bn_kernels_gpu.py applies it to the kernels.

The regime.  A frozen layer normalises with constants: y = (t - m) / sqrt(v + eps) gamma + beta, m and v the running
statistics.  On the device its forward sums are synthesised from them (yunet_bn_batch mode 2: [m count | (v + m^2) count],
pinned by test_bn_batch_mode2_synthesised_sums -- block() below is that expression), and the READER of its backward sums
(the producer's backward) takes a zero block, so that dz = gamma invstd dy: no batch term is subtracted, and the
depthwise-bias gradient db2 (the stem's db) -- identically zero behind a training-mode BatchNorm -- is a real gradient.
The consumers still add [sum dy | sum dy xhat] to the layer's own block, with xhat from m and v.

Statistics per case (seeded): m = batch mean + delta sigma, delta ~ N(0, 0.5^2); v = batch var exp(N(0, 0.5^2)); both
rounded to fp32, as a checkpoint holds them.  Five channels of every frozen layer are fixed:
    NEG    gamma < 0
    ZERO   gamma = 0, beta = 0.3 > 0: the activation is the constant beta, nothing reaches the unit in front of it
    DEAD   beta so negative that the ReLU mask is off everywhere: every gradient through it is exactly 0
    ALIVE  beta so positive that the mask is on everywhere
    FAR    |m| ~ 50 sqrt(v): the data of the channel is shifted to a mean of 50 standard deviations first
DEAD and ALIVE take the smallest such beta (0.5 beyond the channel's extreme), so that no channel's activations dwarf the
others in a max-norm."""
import types

import torch
import torch.nn.functional as F

import bf16_ref as R
from test_kernels_gpu import bn_ref, mk_unit, nchw, nhwc, stats_of

EPS = 1e-5
NEG, ZERO, DEAD, ALIVE, FAR = 0, 1, 2, 3, 4
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def _b(v):
    return v.view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------ frozen BatchNorm
def fbn(t, m, v, gamma, beta, eps=EPS):
    """frozen BatchNorm of an NCHW tensor, in t's precision -> (output, xhat)"""
    xhat = (t - _b(m.to(t.dtype))) / torch.sqrt(_b(v.to(t.dtype)) + eps)
    return xhat * _b(gamma.to(t.dtype)) + _b(beta.to(t.dtype)), xhat


def frozen_stats(t, g):
    """(m, v) of a frozen layer whose input is the NCHW tensor t: near the batch's, not equal to them; fp32 values in fp64"""
    t = t.double()
    c = t.shape[1]
    mean, var = t.mean(dim=(0, 2, 3)), t.var(dim=(0, 2, 3), unbiased=False)
    m = mean + 0.5 * torch.randn(c, generator=g, dtype=F64) * var.sqrt()
    v = var * torch.exp(0.5 * torch.randn(c, generator=g, dtype=F64))
    return m.float().double(), v.float().double()


def block(m, v, count):
    """the fp64 sums a kernel reads for a frozen layer: what yunet_bn_batch mode 2 writes"""
    return torch.cat([m * count, (v + m * m) * count]).contiguous()


def far_shift(t, ch=FAR):
    """what to add to channel `ch` of the NCHW tensor t so that its mean is 50 of its standard deviations"""
    x = t[:, ch].double()
    return float(50.0 * x.std(unbiased=False) - x.mean())


def specialise(gamma, beta, xhat):
    """set the fixed channels of a frozen layer (fp32 gamma, beta, in place) from the layer's fp64 xhat"""
    gamma[NEG] = -gamma[NEG]
    gamma[ZERO], beta[ZERO] = 0.0, 0.3
    beta[DEAD] = -float((gamma[DEAD].double() * xhat[:, DEAD]).max()) - 0.5
    beta[ALIVE] = -float((gamma[ALIVE].double() * xhat[:, ALIVE]).min()) + 0.5
    return gamma, beta


def off_threshold(x32, bn, bf16=False, margin=1e-4):
    """Keep |bn(x)| >= margin (tests/test_dp_descriptor_gpu.py: off_the_relu_threshold gives the reasons), `bn` any
    BatchNorm of the fp64 tensor -- a frozen one does not move with x.  Elements nearer than that move 0.05 up (bf16
    storage: at least to the next bf16 value).  -> (x, elements moved); at most one element in 1000 may move."""
    moved = 0
    for _ in range(8):
        near = bn(x32.double()).abs() < margin
        if not bool(near.any()):
            assert moved * 1000 <= x32.numel(), ('the threshold margin moved too many elements', moved, x32.numel())
            return x32, moved
        moved += int(near.sum())
        step = torch.full_like(x32, 0.05)
        if bf16:
            step = torch.maximum(step, R.ulp_bf16(x32).float())
        x32 = torch.where(near, x32 + step, x32)
        x32 = x32.to(BF16).float() if bf16 else x32
    raise AssertionError('could not move the input off the ReLU threshold')


def sums(d, xhat):
    """[sum d | sum d xhat] over an NCHW gradient: what a layer's consumers add to its block"""
    return torch.cat([d.sum(dim=(0, 2, 3)), (d * xhat).sum(dim=(0, 2, 3))])


# ------------------------------------------------------------------------------------------------ ConvDPUnit
def _bn_side(mode, p, t):
    """(output, xhat) of one side's BatchNorm on the NCHW tensor t: None, 'train' (batch statistics, inside autograd) or
    'frozen' (constants)"""
    if mode == 'frozen':
        return fbn(t, p.m, p.v, p.gamma, p.beta)
    return bn_ref(t, p.gamma.to(t.dtype), p.beta.to(t.dtype))


def unit_grads(u, dtype=F64, in_mode=None, out_mode=None, dy_mask=None):
    """Autograd through [BN + ReLU ->] conv1x1 -> dw3x3 [-> BN + ReLU] in `dtype`, with u.in_mode / u.out_mode unless given.
    dy_mask: the output ReLU as a fixed 0 / 1 mask (the fp32 run takes the fp64 run's, as a kernel takes a masked dy).
    -> dict(dx, dw1, db1, dw2, db2 [, in_sums]) in the kernels' layouts (NHWC, [cout, cin], [cout, 9]) and z, dy, mask, bst
    (the output layer's own backward sums) as NCHW / vectors."""
    in_mode = u.in_mode if in_mode is None else in_mode
    out_mode = u.out_mode if out_mode is None else out_mode
    cin, cout = u.cin, u.cout
    x = u.x32.to(dtype)
    w_pw, b_pw, w_dw, b_dw = [t.to(dtype).clone().requires_grad_(True) for t in u.unit]
    xhat_in = None
    if in_mode != 'none':
        y_in, xhat_in = _bn_side(in_mode, u.inp, x)
        b_in = y_in.detach().requires_grad_(True)
        a = F.relu(b_in)
    else:
        b_in = x.clone().requires_grad_(True)
        a = b_in
    z = F.conv2d(F.conv2d(a, w_pw, b_pw), w_dw, b_dw, padding=1, groups=cout)
    out = types.SimpleNamespace(z=z.detach(), mask=None, bst=None)
    r = u.r.to(dtype)
    if out_mode != 'none':
        zb, xhat_out = _bn_side(out_mode, u.out, z)
        zb.retain_grad()
        if dy_mask is None:
            (F.relu(zb) * r).sum().backward()
            out.mask = (zb.detach() > 0).to(F64)
        else:
            (zb * (r * dy_mask.to(dtype))).sum().backward()
        out.dy = zb.grad                                      # grad wrt the BN output, ReLU mask applied
        out.bst = sums(out.dy, xhat_out.detach())
    else:
        (z * r * _b(u.scale.to(dtype))).sum().backward()
        out.dy = r
    out.g = dict(dx=nhwc(b_in.grad), dw1=w_pw.grad.reshape(cout, cin), db1=b_pw.grad, dw2=w_dw.grad.reshape(cout, 9),
                 db2=b_dw.grad)
    if xhat_in is not None:
        out.g['in_sums'] = sums(b_in.grad, xhat_in.detach())
    return out


def _side(c, g):
    p = types.SimpleNamespace(gamma=torch.rand(c, generator=g) + 0.5, beta=torch.randn(c, generator=g) * .2, m=None, v=None)
    return p


def unit_case(cin, cout, shape, in_mode='frozen', out_mode='frozen', bf16=False, pooled=False, seed=0):
    """Inputs (CPU tensors) and the fp64 reference of one ConvDPUnit backward launch.  in_mode / out_mode: 'none',
    'train' (batch statistics with the batch-consistent backward sums, as every other kernel test) or 'frozen'.
    bf16: activation storage as in tests/bf16_ref.py (x and z rounded; the reference is bf16_ref.bwd_ref's contract, into
    which the frozen statistics go as sums).  pooled: the unit feeds max_pool2d only (dy is the pooled gradient).
    Fields: x32 (NCHW), unit, inp / out (gamma, beta, m, v, stats = the forward block, bst = the sums its reader takes),
    z (NHWC, what the kernel reads), dy (NHWC or pooled), idx, scale, ref (dict), moved, count."""
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    u = types.SimpleNamespace(cin=cin, cout=cout, n=n, h=h, w=w, count=n * h * w, in_mode=in_mode, out_mode=out_mode,
                              bf16=bf16, moved=0, idx=None)
    x32 = torch.randn(n, cin, h, w, generator=g) * 2 + 0.5
    unit = list(mk_unit(cin, cout, g))
    u.inp, u.out = _side(cin, g), _side(cout, g)
    r = torch.randn(n, cout, h, w, generator=g).double()
    u.scale = torch.rand(cout, generator=g) + 0.5
    if pooled:      # the gradient reaches one recorded position per 2 x 2 window
        u.idx = torch.randint(0, 4, (n, h // 2, w // 2, cout), generator=g, dtype=torch.uint8)
        r = r * nchw(R.expand_pooled(torch.ones(n, h // 2, w // 2, cout), u.idx))
    u.r = r
    # ---- the input side
    if in_mode == 'frozen':
        x32[:, FAR] += far_shift(x32)
    x32 = x32.to(BF16).float() if bf16 else x32
    if in_mode == 'frozen':
        u.inp.m, u.inp.v = frozen_stats(x32, g)
        specialise(u.inp.gamma, u.inp.beta, fbn(x32.double(), u.inp.m, u.inp.v, u.inp.gamma, u.inp.beta)[1])
    if in_mode != 'none':
        x32, u.moved = off_threshold(x32, lambda t: _bn_side(in_mode, u.inp, t)[0], bf16)
        u.inp.stats = block(u.inp.m, u.inp.v, u.count) if in_mode == 'frozen' else stats_of(nhwc(x32))
    u.x32, u.unit = x32, unit
    if bf16:
        return _bf16_unit(u, g)
    # ---- the output side: its statistics come from the unit's own z
    if out_mode == 'frozen':
        z = unit_grads(u, out_mode='none').z
        unit[3][FAR] += far_shift(z)
        z = unit_grads(u, out_mode='none').z
        u.out.m, u.out.v = frozen_stats(z, g)
        specialise(u.out.gamma, u.out.beta, fbn(z, u.out.m, u.out.v, u.out.gamma, u.out.beta)[1])
    ref = unit_grads(u)
    u.ref, u.mask = ref.g, ref.mask
    u.z = nhwc(ref.z)
    if out_mode == 'frozen':
        u.out.stats, u.out.bst = block(u.out.m, u.out.v, u.count), torch.zeros(2 * cout, dtype=F64)
    elif out_mode == 'train':
        u.out.stats, u.out.bst = stats_of(u.z.float()), ref.bst
    dyn = nhwc(ref.dy)
    u.dy_abs_sum = float(dyn.abs().sum())
    u.dy = torch.gather(R.windows(dyn), -1, u.idx.long().unsqueeze(-1)).squeeze(-1) if pooled else dyn
    return u


def _bf16_unit(u, g):
    """bf16 storage: the stored z is the contract's forward rounded to bf16 (heads: fp32), dy = r under the frozen mask of
    the STORED z, the reference bf16_ref.bwd_ref with the frozen blocks as the layers' sums and zero backward sums"""
    assert u.in_mode in ('none', 'frozen') and u.out_mode in ('none', 'frozen') and u.idx is None
    cin, cout = u.cin, u.cout
    W = [u.unit[0].view(cout, cin), u.unit[1], u.unit[2].view(cout, 9), u.unit[3]]
    x64 = nhwc(u.x32).double()
    in_ref = R.BNRef(u.inp.stats, u.inp.gamma, u.inp.beta, u.count) if u.in_mode == 'frozen' else None
    gemm_fwd, gemm_bwd = cin % 32 == 0, cin == 64 and cout == 64
    fr = R.fwd_ref(x64, *W, in_bn=in_ref, bf16_gemm=gemm_fwd)
    dy = nhwc(u.r)
    out_ref = None
    if u.out_mode == 'frozen':
        u.unit[3][FAR] += far_shift(nchw(fr['z']))
        fr = R.fwd_ref(x64, *W, in_bn=in_ref, bf16_gemm=gemm_fwd)
        z16 = fr['z'].to(BF16)
        zs = nchw(z16.double())
        u.out.m, u.out.v = frozen_stats(zs, g)
        specialise(u.out.gamma, u.out.beta, fbn(zs, u.out.m, u.out.v, u.out.gamma, u.out.beta)[1])
        u.mask = (fbn(zs, u.out.m, u.out.v, u.out.gamma, u.out.beta)[0] > 0).to(F64)
        dy = dy * nhwc(u.mask)
        u.out.stats, u.out.bst = block(u.out.m, u.out.v, u.count), torch.zeros(2 * cout, dtype=F64)
        out_ref = R.BNRef(u.out.stats, u.out.gamma, u.out.beta, u.count, bstats=u.out.bst)
        u.z = z16
    else:
        u.z = fr['z'].float()
    u.dy = dy.float().double()
    u.dy_abs_sum = float(u.dy.abs().sum())
    u.br = R.bwd_ref(x64, *W, z=u.z.double(), dy=u.dy, in_bn=in_ref, out_bn=out_ref,
                     dy_scale=None if out_ref is not None else u.scale, bf16_gemm=gemm_bwd)
    u.ref = {k: u.br[k] for k in ('dx', 'dw1', 'db1', 'dw2', 'db2')}
    if in_ref is not None:
        u.ref['in_sums'] = u.br['in_bst']
    return u


# ------------------------------------------------------------------------------------------------ stem
def stem_grads(s, dtype=F64, dy_mask=None):
    """autograd through conv3x3(stride 2) -> frozen BN -> ReLU in `dtype` -> (dw [16, 3, 3, 3], db [16], z, dy, mask)"""
    wt, b = s.wt.to(dtype).clone().requires_grad_(True), s.b.to(dtype).clone().requires_grad_(True)
    z = F.conv2d(s.img.to(dtype), wt, b, stride=2, padding=1)
    if s.bn.m is None:
        return None, None, z.detach(), None, None
    zb, _ = fbn(z, s.bn.m, s.bn.v, s.bn.gamma, s.bn.beta)
    zb.retain_grad()
    if dy_mask is None:
        (F.relu(zb) * s.r.to(dtype)).sum().backward()
    else:
        (zb * (s.r * dy_mask).to(dtype)).sum().backward()
    return wt.grad, b.grad, z.detach(), zb.grad, (zb.detach() > 0).to(F64)


def stem_case(n, h, w):
    """The stem behind a frozen bn1: images in [0, 255].  Fields: img, wt, b, bn (gamma, beta, m, v, stats, bst), z (NHWC),
    dy (NHWC), dw, db (fp64), and err32 = the max-norm errors (dw, db) of torch's fp32 CPU autograd of the same
    composition against them."""
    g = torch.Generator().manual_seed(h)
    s = types.SimpleNamespace(n=n, h=h, w=w, count=n * (h // 2) * (w // 2))
    s.img = torch.rand(n, 3, h, w, generator=g) * 255
    s.wt, s.b = torch.randn(16, 3, 3, 3, generator=g) * 0.05, torch.randn(16, generator=g) * 0.1
    s.bn = _side(16, g)
    s.b[FAR] += far_shift(stem_grads(s)[2])
    z = stem_grads(s)[2]
    s.r = torch.randn(z.shape, generator=g).double()
    s.bn.m, s.bn.v = frozen_stats(z, g)
    specialise(s.bn.gamma, s.bn.beta, fbn(z, s.bn.m, s.bn.v, s.bn.gamma, s.bn.beta)[1])
    s.bn.stats, s.bn.bst = block(s.bn.m, s.bn.v, s.count), torch.zeros(32, dtype=F64)
    s.dw, s.db, z, dy, s.mask = stem_grads(s)
    s.z, s.dy = nhwc(z), nhwc(dy)
    dw32, db32, _, _, _ = stem_grads(s, F32, dy_mask=s.mask)
    s.err32 = (float((dw32.double() - s.dw).abs().max()), float((db32.double() - s.db).abs().max()))
    return s


# ------------------------------------------------------------------------------------------------ element-wise
def _frozen_layer(z32, g):
    """a frozen layer over the raw NCHW tensor z32 (FAR channel shifted, kept off the ReLU threshold) -> (z32, layer)"""
    c = z32.shape[1]
    p = _side(c, g)
    z32[:, FAR] += far_shift(z32)
    p.m, p.v = frozen_stats(z32, g)
    specialise(p.gamma, p.beta, fbn(z32.double(), p.m, p.v, p.gamma, p.beta)[1])
    z32, p.moved = off_threshold(z32, lambda t: fbn(t, p.m, p.v, p.gamma, p.beta)[0])
    p.stats = block(p.m, p.v, z32.numel() // c)
    return z32, p


def ew_case(c, shape=(3, 12, 20)):
    """max_pool2d(2) over a frozen BN + ReLU (alone, and with a second full-size consumer: pool_bwd's `extra`) and the
    upsample-add of two frozen BN + ReLU branches.  Fields: za, zb (NHWC fp32), a, b (the layers), r_p, r_e (the pooled /
    full-size output gradients, NHWC), and fp64 references: pool = (dx, sums), pool_extra = (dx, sums),
    upadd = (dxa, sums a, dxb, sums b).  gap: the smallest distance between a live window's maximum and its runner-up,
    exact ties aside (ZERO's four-way ties, which position 0 wins as in F.max_pool2d)."""
    n, h, w = shape
    g = torch.Generator().manual_seed(300 + c)
    e = types.SimpleNamespace(c=c, n=n, h=h, w=w)
    za, e.a = _frozen_layer(torch.randn(n, c, h, w, generator=g) * 2, g)
    zb, e.b = _frozen_layer(torch.randn(n, c, h // 2, w // 2, generator=g) * 2, g)
    r_p = torch.randn(n, c, h // 2, w // 2, generator=g).double()
    r_e = torch.randn(n, c, h, w, generator=g).double()
    e.za, e.zb, e.r_p, e.r_e = nhwc(za), nhwc(zb), nhwc(r_p), nhwc(r_e)

    def layer(z32, p):
        y, xhat = fbn(z32.double(), p.m, p.v, p.gamma, p.beta)
        return y.detach().requires_grad_(True), xhat
    ya, xha = layer(za, e.a)
    (F.max_pool2d(F.relu(ya), 2) * r_p).sum().backward()
    e.pool = (nhwc(ya.grad), sums(ya.grad, xha))
    top = R.windows(nhwc(F.relu(ya.detach()))).sort(dim=-1, descending=True).values
    gap = (top[..., 0] - top[..., 1])[(top[..., 0] > 0) & (top[..., 0] != top[..., 1])]
    e.gap = float(gap.min())
    ya, xha = layer(za, e.a)
    ((F.max_pool2d(F.relu(ya), 2) * r_p).sum() + (F.relu(ya) * r_e).sum()).backward()
    e.pool_extra = (nhwc(ya.grad), sums(ya.grad, xha))
    ya, xha = layer(za, e.a)
    yb, xhb = layer(zb, e.b)
    ((F.relu(ya) + F.interpolate(F.relu(yb), scale_factor=2., mode='nearest')) * r_e).sum().backward()
    e.upadd = (nhwc(ya.grad), sums(ya.grad, xha), nhwc(yb.grad), sums(yb.grad, xhb))
    return e


# ------------------------------------------------------------------------------------------------ cases and bars
# The per-channel bars (4x the max-norm bar) rest on a premise, stated where tests/test_kernels_gpu.py introduces them: a
# channel's own maximum is a few times below the tensor's.  The rows here keep max / channel max below 4 for dx and below
# 120 for dw1 -- except the four-pixel row (1, 2, 2), where a pooled dy leaves ONE live pixel per output channel and the
# input ReLU two of four per input channel: with the row's first seed a channel of dx has its only live element 496x
# below the tensor's maximum, and an error of 8e-7 of that maximum reads as 3.8e-4 "per channel".  That row takes the
# first seed (in steps of SEED_STEP) at which the fp64 reference meets the premise as the other rows do: dx within 16,
# dw1 within 64 (conditioning(), asserted by tests/test_frozen_ref.py).
SEED_STEP = 1000003
SEED_BUMP = {(64, 64, (1, 2, 2)): 5}


def conditioning(t, dim):
    """max |t| over the tensor / over its weakest channel that is not identically zero"""
    ch = t.abs().amax(dim=[d for d in range(t.dim()) if d != dim])
    return float(t.abs().max() / ch[ch > 0].min())


def unit_case_of(spec, regime='ff'):
    """a row of tests/test_dp_descriptor_gpu.py: BWD under a regime: two letters, input then output layer, f(rozen) or
    t(raining); a side the row's mode has no BatchNorm on stays without one"""
    mode = spec.get('mode', 'bn_bn')
    name = {'f': 'frozen', 't': 'train'}
    cin, cout, (n, h, w) = spec['cin'], spec['cout'], spec['shape']
    return unit_case(cin, cout, (n, h, w), in_mode=name[regime[0]] if mode.startswith('bn') else 'none',
                     out_mode=name[regime[1]] if mode.endswith('_bn') else 'none', bf16=spec.get('bf16', False),
                     pooled=spec.get('pooled', False), seed=1000 * cin + 10 * cout + n + h + w + 7 * (regime != 'ff') +
                     SEED_STEP * SEED_BUMP.get((cin, cout, (n, h, w)), 0))


def rel_el(a, b):
    """worst relative error per element over the elements of the reference that are not zero"""
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    keep = b != 0
    return float(((a - b).abs()[keep] / b.abs()[keep]).max()) if bool(keep.any()) else 0.0


# The per-channel bar of db2 is relative to the channel's own sum.  In one case that sum cancels: channel 28 of
# tile-16x64-ragged under 'ff' has db2 = 3.21e-3 with sum |dz| = 703 (the tensor's largest db2: 111).  torch's fp32 CPU
# autograd is off by 2.02e-6 there -- 3e-9 of sum |dz|, 6.31e-4 of the channel's value, three times the 4 x 5e-5 bar -- so
# that one bar is 10x the reference's own error (the project's 10x rule); every other case keeps 4 tol, where the fp32
# reference's worst is 6.1e-5 (bwd64-8w).
DB2_CH_BAR = {('tile-16x64-ragged', 'ff'): 10 * 6.31e-4}


def check_unit(u, got, tol, note, family, db2_ch_bar=None):
    """The gradients `got` of one launch (dx NHWC, dw1, db1, dw2, db2, bst = what the launch added to the input layer's
    zeroed block) against u.ref at the project's bars: max-norm tol, 4 tol per channel; db2 behind a frozen output layer
    like every other gradient (per channel: per element; db2_ch_bar: a case's entry of DB2_CH_BAR).
    bf16 storage: the per-element checkers of tests/bf16_ref.py."""
    db2_ch_bar = db2_ch_bar or 4 * tol
    from test_kernels_gpu import rel_err, rel_err_ch
    ref, cin, cout = u.ref, u.cin, u.cout
    dw1, dw2 = got['dw1'].reshape(cout, cin), got['dw2'].reshape(cout, 9)
    if u.bf16:
        amb = u.br['amb']
        worst = [R.check_fp32('dx ' + family, got['dx'], ref['dx'], tol, ch_dim=-1),
                 R.check_fp32('dw1 ' + family, dw1, ref['dw1'], tol, amb=amb['dw1'], ch_dim=0),
                 R.check_fp32('db1 ' + family, got['db1'], ref['db1'], tol),
                 R.check_fp32('dw2 ' + family, dw2, ref['dw2'], tol, amb=amb['dw2']),
                 R.check_fp32('db2 ' + family, got['db2'].reshape(cout, 1), ref['db2'].reshape(cout, 1), tol, ch_dim=0)]
        if 'in_sums' in ref:
            worst.append(R.check_fp32('in sums ' + family, got['bst'], ref['in_sums'], tol))
        note(family, 'err/bound', max(worst), 1.0)
        note(family, 'db2', rel_err(got['db2'], ref['db2']), tol)
        return
    assert note(family, 'dx', rel_err(got['dx'], ref['dx']), tol) < tol
    assert note(family, 'dx/ch', rel_err_ch(got['dx'], ref['dx'], dim=3), 4 * tol) < 4 * tol
    assert note(family, 'dw1', rel_err(dw1, ref['dw1']), tol) < tol
    assert note(family, 'dw1/ch', rel_err_ch(dw1, ref['dw1'], dim=0), 4 * tol) < 4 * tol
    assert note(family, 'db1', rel_err(got['db1'], ref['db1']), tol) < tol
    assert note(family, 'dw2', rel_err(dw2, ref['dw2']), tol) < tol
    if u.out_mode == 'train':       # the depthwise-bias gradient is identically zero (noise only)
        assert float(got['db2'].abs().max()) < 1e-3 * u.dy_abs_sum
    else:
        assert note(family, 'db2', rel_err(got['db2'], ref['db2']), tol) < tol
    if u.out_mode == 'frozen':
        assert note(family, 'db2/ch', rel_el(got['db2'], ref['db2']), db2_ch_bar) < db2_ch_bar
    if 'in_sums' in ref:
        assert note(family, 'in sums', rel_err(got['bst'], ref['in_sums']), tol) < tol


def check_dead(u, got):
    """every gradient through a DEAD channel of a frozen layer is exactly 0.0 (dy and the activation are, and the zero
    block leaves no constant term in dz)"""
    dw1, dw2 = got['dw1'].reshape(u.cout, u.cin), got['dw2'].reshape(u.cout, 9)
    zero = lambda t: not bool(t.double().abs().max() > 0)
    if u.out_mode == 'frozen':
        assert zero(dw2[DEAD]) and zero(got['db2'][DEAD]) and zero(got['db1'][DEAD]) and zero(dw1[DEAD]), 'dead output channel'
    if u.in_mode == 'frozen':
        c = u.cin
        assert zero(got['dx'][..., DEAD]) and zero(dw1[:, DEAD]), 'dead input channel'
        bst = got['bst'] if 'bst' in got else got['in_sums']
        assert zero(bst[DEAD]) and zero(bst[c + DEAD]), 'dead input channel: sums'
