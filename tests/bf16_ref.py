"""fp64 reference of the bf16 build's arithmetic contract (BASELINE.json configs[2], "bf16 fwd / fp32 grads") and
per-element checkers.  Host-only helper module (no GPU, no pytest fixtures); tests/test_bf16_ref.py shows on the CPU that
every checker rejects the defects a kernel could have, tests/test_bf16_kernels_gpu.py applies them to the kernels.

The contract, one row per kernel family, as the sources implement it (common.h: act_t, -DYUNET_ACT_BF16):

  * 16-input-channel forward units (conv_fwd16.hip dp_fwd16s, conv_fwd.hip dp_fwd<16,...>): fp32 arithmetic; z is
    stored as the round-to-nearest-even (RNE) bf16 of the fp32 result; the BN sums are taken over the unrounded values.
  * 32 / 64-input-channel forward units (dp_fwd<32|64,...>, packed canvases, conv_fwd64.hip dp_fwd64s): one bf16 matrix
    product of a = bf16(relu(bn(x))) (a computed in fp32, then rounded) with bf16(W1), fp32 accumulation; depthwise and
    biases fp32; z stored as RNE bf16, BN sums unrounded.  (The fp32 build splits both operands three ways instead.)
  * Heads (64 -> 16, no BatchNorm behind them): the 64-input rule above, z written as fp32.
  * dp_bwd64 (64 -> 64 backward, conv_bwd64.hip, BWD64_LEAN: every bf16 build): p = bf16(a) bf16(W1) as one product;
    dW1 = bf16(a)^T dp and da = dp bf16(W1), dp fp32-accurate (split hi + lo); everything else fp32.
  * The other backward tile kernels (dp_bwd<...>, including the split-bf16 GEMM = 1 32 -> 64 instance and the packed
    64 -> 16 heads): fp32-accurate arithmetic on the widened stored bf16 x and z (the BN backward's xhat comes from the
    STORED z).
  * dp_bwd16s (conv_bwd16.hip): recomputes z from the bf16 x in fp32 and does not read the stored z.
  * Stem (conv_stem.hip, matrix cores): z stored as RNE bf16 of the fp32 result, BN sums unrounded.  The training step's
    stem weight gradient is yunet_stem_bwd_rz (z recomputed from the image; reads no activation); the _bf16 stem_bwd
    entry reads the stored z.
  * Fused max-pooling (dp_fwd<...,POOL>, dp_fwd16s<16,true>, dp_fwd64s with pool_out): the winner of a 2 x 2 window is
    the FIRST window position (raster order 2 dy + dx) among the maxima of sign(gamma) * (stored z); its stored value
    is written bit for bit.  That is also what pool_fwd / pool_bwd on the stored tensor and F.max_pool2d do.

The checkers bound every element by its own error scale instead of one max-norm: `mag` is the same pipeline run on
|W|, |b|, |a|, `terms` the number of fp32 accumulations behind an element.  Operands that the contract rounds to bf16
can be ambiguous: an fp64 `a` within 2^-20 relative of a bf16 rounding midpoint may round to the other neighbour in
the kernel's fp32 arithmetic.  Such an operand contributes one bf16 ulp of `a`, propagated through |W1| and |W2|."""
import torch
import torch.nn.functional as F

AMBIG_REL = 2.0 ** -20
EPS32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ bf16 arithmetic
def rne_bf16(t):
    """fp64 -> the nearest bf16 value (ties to even), held in fp64; a direct rounding, not via fp32."""
    t = t.double()
    m, e = torch.frexp(t)                                   # t = m 2^e, 0.5 <= |m| < 1
    return torch.ldexp(torch.round(torch.ldexp(m, torch.full_like(e, 8))), e - 8)


def ulp_bf16(t):
    """spacing of bf16 values at |t| (0 at t == 0)"""
    t = t.double()
    _, e = torch.frexp(t)
    return torch.where(t == 0, torch.zeros_like(t), torch.ldexp(torch.ones_like(t), e - 8))


def ambiguous(t, rel=AMBIG_REL):
    """elements whose bf16 rounding can flip under a relative perturbation of `rel` (near a rounding midpoint)"""
    t = t.double()
    return rne_bf16(t * (1 + rel)) != rne_bf16(t * (1 - rel))


# ------------------------------------------------------------------------------------------------ reference pipeline
class BNRef:
    """a BatchNorm as a kernel sees it: fp64 sums [sum | sum of squares] over `count` values, gamma, beta, and for the
    backward the sums of dy and dy * xhat (bstats)."""

    def __init__(self, stats, gamma, beta, count, bstats=None, eps=1e-5):
        self.stats, self.gamma, self.beta = stats.double().cpu(), gamma.double().cpu(), beta.double().cpu()
        self.bstats = None if bstats is None else bstats.double().cpu()
        self.count, self.eps = int(count), float(eps)

    def mean_invstd(self):
        c = self.gamma.numel()
        mean = self.stats[:c] / self.count
        var = (self.stats[c:] / self.count - mean * mean).clamp_min(0.0)
        return mean, 1.0 / torch.sqrt(var + self.eps)

    def xhat(self, z):
        mean, inv = self.mean_invstd()
        return (z - mean) * inv

    def act(self, z):
        return F.relu(self.xhat(z) * self.gamma + self.beta)


class RunningBNRef(BNRef):
    """a BatchNorm in eval mode, applied directly as nn.BatchNorm2d.eval() does: (z - running_mean) /
    sqrt(running_var + eps) gamma + beta.  No sums: a kernel that derives its coefficients from synthesised sums is
    checked against this, not against its own recovery."""

    def __init__(self, running_mean, running_var, gamma, beta, eps=1e-5):
        self.rm, self.rv = running_mean.double().cpu(), running_var.double().cpu()
        self.gamma, self.beta = gamma.double().cpu(), beta.double().cpu()
        self.stats = self.bstats = None
        self.eps = float(eps)

    def mean_invstd(self):
        return self.rm, 1.0 / torch.sqrt(self.rv + self.eps)


def stats_of(z):
    z = z.double().reshape(-1, z.shape[-1])
    return torch.cat([z.sum(0), (z * z).sum(0)])


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def depthwise(p, w2, b2=None):
    """3 x 3 depthwise convolution, padding 1, NHWC -> NHWC; w2 [C, 9]"""
    c = p.shape[-1]
    return _nhwc(F.conv2d(_nchw(p), w2.reshape(c, 1, 3, 3), b2, padding=1, groups=c))


def _f64(*ts):
    return [None if t is None else t.detach().double().cpu() for t in ts]


def fwd_ref(x, w1, b1, w2, b2, in_bn=None, bf16_gemm=False):
    """z of one ConvDPUnit under the contract.  x NHWC (the widened stored activations), w1 [cout, cin], w2 [cout, 9].
    bf16_gemm: the 32 / 64-input rule (a and W1 rounded to bf16 before the one product).
    -> dict(z, mag, amb, terms): amb = the ambiguous-operand term per element (zeros without bf16_gemm)."""
    x, w1, b1, w2, b2 = _f64(x, w1, b1, w2, b2)
    a = in_bn.act(x) if in_bn is not None else x
    if bf16_gemm:
        aq, w1q = rne_bf16(a), rne_bf16(w1)
        da = torch.where(ambiguous(a), ulp_bf16(a), torch.zeros_like(a))
    else:
        aq, w1q, da = a, w1, torch.zeros_like(a)
    p = aq @ w1q.t() + b1
    z = depthwise(p, w2, b2)
    mag = depthwise(aq.abs() @ w1q.abs().t() + b1.abs(), w2.abs(), b2.abs())
    amb = depthwise(da @ w1q.abs().t(), w2.abs())
    return dict(z=z, mag=mag, amb=amb, terms=x.shape[-1] + 12)


def expand_pooled(dpool, idx):
    """the pooled gradient [N, H/2, W/2, C] at the recorded window positions (uint8 2 dy + dx) of a full-size map"""
    dpool, idx = dpool.double().cpu(), idx.long().cpu()
    n, ho, wo, c = dpool.shape
    full = torch.zeros(n, ho, wo, c, 4, dtype=torch.float64)
    full.scatter_(4, idx.unsqueeze(-1), dpool.unsqueeze(-1))
    return full.view(n, ho, wo, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2 * ho, 2 * wo, c)


def bwd_ref(x, w1, b1, w2, b2, z, dy, in_bn=None, out_bn=None, dy_scale=None, bf16_gemm=False, recompute_z=False,
            pool_idx=None):
    """Gradients of one ConvDPUnit under the contract, in fp64.
    z: the stored forward output the kernel reads (ignored with recompute_z: dp_bwd16s).  dy: gradient wrt the unit's BN
    output (ReLU mask applied; out_bn.bstats = its sums) or, without out_bn, wrt z scaled per channel by dy_scale.
    pool_idx: dy is the pooled gradient, routed to the recorded window positions.
    bf16_gemm: dp_bwd64's rule (p, dW1, da from bf16(a) and bf16(W1)).
    -> dict(dx, dw1, db1, dw2, db2, in_bst), da = dx before the input ReLU's mask, and amb = {dw1, dw2}: the
    ambiguous-operand terms."""
    x, w1, b1, w2, b2, z, dy, dy_scale = _f64(x, w1, b1, w2, b2, z, dy, dy_scale)
    if pool_idx is not None:
        dy = expand_pooled(dy, pool_idx)
    a0 = in_bn.act(x) if in_bn is not None else x
    if recompute_z:
        z = fwd_ref(x, w1, b1, w2, b2, in_bn)['z']
    if out_bn is not None:
        mean, inv = out_bn.mean_invstd()
        c = out_bn.gamma.numel()
        xh = (z - mean) * inv
        dz = out_bn.gamma * inv * (dy - out_bn.bstats[:c] / out_bn.count - xh * out_bn.bstats[c:] / out_bn.count)
    else:
        dz = dy * (dy_scale if dy_scale is not None else 1.0)
    a = a0.clone().requires_grad_(True)
    W1, B1, W2, B2 = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    if bf16_gemm:     # straight-through: the product sees the rounded operands, the gradients reach the fp32 ones
        aq = a + (rne_bf16(a0) - a0)
        w1q = W1 + (rne_bf16(w1) - w1)
    else:
        aq, w1q = a, W1
    p = aq @ w1q.t() + B1
    zz = depthwise(p, W2, B2)
    (zz * dz).sum().backward()
    da = a.grad
    in_bst = None
    if in_bn is not None:
        xh_in = in_bn.xhat(x)
        mask = (xh_in * in_bn.gamma + in_bn.beta) > 0
        dx = da * mask
        in_bst = torch.cat([dx.sum((0, 1, 2)), (dx * xh_in).sum((0, 1, 2))])
    else:
        dx = da
    amb = dict(dw1=torch.zeros_like(w1), dw2=torch.zeros_like(w2))
    if bf16_gemm:
        d_a = torch.where(ambiguous(a0), ulp_bf16(a0), torch.zeros_like(a0))
        pd = depthwise(dz.abs(), w2.abs().flip(-1))           # |dp| <= depthwise^T(|W2|) |dz|
        amb['dw1'] = pd.abs().reshape(-1, pd.shape[-1]).t() @ d_a.reshape(-1, d_a.shape[-1])
        dp_amb = d_a @ rne_bf16(w1).abs().t()
        amb['dw2'] = depthwise_wgrad(dp_amb, dz.abs())
    return dict(dx=dx, da=da, dw1=W1.grad, db1=B1.grad, dw2=W2.grad, db2=B2.grad, in_bst=in_bst, amb=amb)


def depthwise_wgrad(p, dz):
    """sum over pixels of p[shifted by the tap] * dz, per channel and tap -> [C, 9]"""
    n, h, w, c = p.shape
    pp = F.pad(_nchw(p), (1, 1, 1, 1))
    out = torch.empty(c, 9, dtype=torch.float64)
    dzc = _nchw(dz)
    for t in range(9):
        ky, kx = divmod(t, 3)
        out[:, t] = (pp[:, :, ky:ky + h, kx:kx + w] * dzc).sum((0, 2, 3))
    return out


# ------------------------------------------------------------------------------------------------ checkers
def _report(name, ratio, got, ref, bound):
    flat = int(torch.argmax(ratio.reshape(-1)))
    worst = float(ratio.reshape(-1)[flat])
    where = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape)) if ratio.dim() else ()
    msg = (f'[{name}] worst error / bound {worst:.3g} at {where}: got {float(got.reshape(-1)[flat]):.9g}, '
           f'ref {float(ref.reshape(-1)[flat]):.9g}, bound {float(bound.reshape(-1)[flat]):.3g}')
    print(msg)
    return worst, msg


def check_bf16(name, got, ref, mag, terms, amb=None, stored='bf16'):
    """bf16-stored outputs: |got - ref| <= ulp_bf16(ref) + terms 2^-24 mag (+ amb) per element.  stored='fp32' (the heads'
    z): one fp32 rounding instead of one bf16 ulp.  Raises AssertionError; returns the worst error / bound."""
    got, ref, mag = got.double().cpu(), ref.double().cpu(), mag.double().cpu()
    unit = ulp_bf16(ref) if stored == 'bf16' else EPS32 * ref.abs()
    bound = unit + terms * EPS32 * mag + 1e-300
    if amb is not None:
        bound = bound + amb.double().cpu()
    ratio = (got - ref).abs() / bound
    worst, msg = _report(name, ratio, got, ref, bound)
    assert worst <= 1.0, msg
    return worst


def check_fp32(name, got, ref, tol, amb=None, ch_dim=None):
    """fp32 outputs (gradients, BN sums): test_dp_bwd's bars against the contract's fp64 reference, per element --
    |got - ref| <= tol max|ref| (+ amb), and with ch_dim <= 4 tol max over the element's channel (+ amb)."""
    got, ref = got.double().cpu().reshape(ref.shape), ref.double().cpu()
    err = (got - ref).abs()
    extra = amb.double().cpu().reshape(ref.shape) if amb is not None else torch.zeros_like(ref)
    bound = tol * ref.abs().max() + extra + 1e-300
    ratio = err / bound
    worst, msg = _report(name, ratio, got, ref, bound)
    assert worst <= 1.0, msg
    if ch_dim is not None:
        dims = [d for d in range(ref.dim()) if d != ch_dim % ref.dim()]
        chmax = ref.abs().amax(dim=dims, keepdim=True)
        bch = 4 * tol * chmax + extra + 1e-300
        r2 = err / bch
        w2, msg2 = _report(name + ' per channel', r2, got, ref, bch)
        assert w2 <= 1.0, msg2
        worst = max(worst, w2)
    return worst


def windows(z):
    """NHWC [N, H, W, C] -> [N, H/2, W/2, C, 4], window position 2 dy + dx last"""
    n, h, w, c = z.shape
    return z.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)


def pool_rule_idx(z_stored, gamma):
    """the contract's window positions: first maximum of sign(gamma) * stored z"""
    key = windows(z_stored.double().cpu()) * torch.sign(gamma.double().cpu()).view(1, 1, 1, -1, 1)
    return torch.argmax(key, dim=-1)           # (first maximal index, torch.argmax's documented tie rule)


def check_pool(name, z_stored, winners, idx, gamma):
    """fused pooling: idx is the contract's position in every window, and the winner is the stored value there, bit
    for bit (z_stored / winners: the raw stored tensors, e.g. bf16)."""
    want = pool_rule_idx(z_stored, gamma)
    got_idx = idx.long().cpu()
    bad = got_idx != want
    print(f'[{name}] window positions off the rule: {int(bad.sum())} of {bad.numel()}')
    assert not bool(bad.any()), (name, 'first bad window', [int(i) for i in bad.nonzero()[0]])
    at = torch.gather(windows(z_stored.cpu()), -1, got_idx.unsqueeze(-1)).squeeze(-1)
    diff = at.view(torch.int16) != winners.cpu().view(torch.int16) if at.dtype == torch.bfloat16 else at != winners.cpu()
    print(f'[{name}] winners not bitwise the stored value: {int(diff.sum())}')
    assert not bool(diff.any()), (name, 'winner is not the stored value at idx')


def check_routing(name, dense, dpool, idx):
    """a pooled gradient routed to a full-size map: all of a window's gradient on the element idx names, zero elsewhere"""
    want = expand_pooled(dpool, idx)
    bad = dense.double().cpu() != want
    print(f'[{name}] elements off the routing: {int(bad.sum())}')
    assert not bool(bad.any()), (name, 'first bad element', [int(i) for i in bad.nonzero()[0]])
