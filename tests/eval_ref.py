"""fp64 reference of the eval-mode forward (Plan.fwd_eval: BatchNorm on the running statistics) and per-element
checkers, one function per op the eval list runs.  Host-only helper module (no GPU, no pytest fixtures);
tests/test_eval_ref.py shows on the CPU that the checkers reject the defects an eval path could have,
tests/test_eval_forward_gpu.py applies them to every layer of one forward_eval.

BatchNorm is applied as nn.BatchNorm2d.eval() does (bf16_ref.RunningBNRef), never through the synthesised sums of
bn_batch_kernel mode 2, so the reference shares no bug with that mode.  Each layer's reference takes the kernel's own
stored input, widened to fp64 (teacher forcing): errors do not compound and a failing layer is named.

Bars, per element (bf16_ref.check_bf16):
  * fp32 build: one fp32 rounding of the result plus terms 2^-24 mag, `mag` the same pipeline on |W|, |b|, |a|.
  * bf16 build: one bf16 ulp plus terms 2^-24 mag plus the ambiguous-operand term (bf16_ref's contract).
  * The input transform (common.h bnrelu / bn_coef) adds a term of its own, bn_err(): it forms
    fma(x - mean, gamma * invstd, beta) in fp32 with mean, invstd and scale rounded to fp32, and the invstd comes from
    a variance recovered as (v + m^2) count / count - mean^2 in fp64.  With running statistics far from the data
    (|mean| of 50 over a variance of 1e-8) that error scales with |x - mean| |scale|, not with |a|, so bars built on
    |a| alone would be too tight where the ReLU clips and too loose nowhere."""
import torch
import torch.nn.functional as F

import bf16_ref as R
from bf16_ref import EPS32, RunningBNRef, check_bf16, check_pool, ulp_bf16, rne_bf16, ambiguous  # noqa: F401

HEAD_PARTS = (('cls', 1), ('bbox', 4), ('obj', 1), ('kps', 10))    # flat channel order, yunet_head.py:456-477
STEM_TERMS = 28                                                      # 27 products + the bias


# ------------------------------------------------------------------------------------------------ parameters
def running_bn(sd, name, eps=1e-5):
    return RunningBNRef(sd[name + '.running_mean'], sd[name + '.running_var'], sd[name + '.weight'],
                        sd[name + '.bias'], eps)


def unit_weights(sd, prefix):
    """(w1 [cout, cin], b1, w2 [cout, 9], b2) of a ConvDPUnit, fp64"""
    w1 = sd[prefix + '.conv1.weight']
    w2 = sd[prefix + '.conv2.weight']
    return (w1.reshape(w1.shape[0], -1).double(), sd[prefix + '.conv1.bias'].double(),
            w2.reshape(w2.shape[0], 9).double(), sd[prefix + '.conv2.bias'].double())


def head_weights(sd, level):
    """the four 64 -> c heads of a level as the one 64 -> 16 unit the engine runs (cls | bbox | obj | kps)"""
    parts = [unit_weights(sd, f'bbox_head.multi_level_{name}.{level}') for name, _ in HEAD_PARTS]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(4))


# ------------------------------------------------------------------------------------------------ input transform
def bn_err(bn, x):
    """bound of |kernel a - fp64 a| for a = relu(bn(x)) under running statistics (see the module docstring):
    mean rounded to fp32 (|m| |s|), the subtraction, invstd and scale = gamma invstd rounded to fp32 (3 |x - m| |s|),
    the fma rounding (|a|), and the variance recovered from the sums (a few fp64 ulps of v + m^2, relative to
    v + eps and halved by the square root)."""
    x = x.double()
    mean, inv = bn.mean_invstd()
    s = (bn.gamma * inv).abs()
    d = (x - mean).abs()
    pre = ((x - mean) * inv * bn.gamma + bn.beta).abs()
    rel_var = 4 * 2.0 ** -53 * (bn.rv + mean * mean) / (bn.rv + bn.eps) / 2 if hasattr(bn, 'rv') else 0.0
    return EPS32 * (mean.abs() * s + 4 * d * s + pre) + rel_var * d * s


def _transform_amb(a, da, w1q, w2, bf16_gemm):
    """the input-transform error da of a, propagated through |W1| and |W2|; with the bf16 product, an `a` whose
    rounding can flip inside [a - da, a + da] also contributes one bf16 ulp"""
    if bf16_gemm:
        flip = rne_bf16(a + da) != rne_bf16(a - da)
        da = da + torch.where(flip, ulp_bf16(a.abs() + da), torch.zeros_like(a))
    return R.depthwise(da @ w1q.abs().t(), w2.abs())


# ------------------------------------------------------------------------------------------------ one function per op
def stem_ref(img, w, b):
    """3 x 3 stride-2 convolution of the image, NHWC -> dict(z, mag, terms)"""
    img, w, b = img.double().cpu(), w.double().cpu(), b.double().cpu()
    z = F.conv2d(img, w, b, stride=2, padding=1).permute(0, 2, 3, 1)
    mag = F.conv2d(img.abs(), w.abs(), b.abs(), stride=2, padding=1).permute(0, 2, 3, 1)
    return dict(z=z, mag=mag, terms=STEM_TERMS, amb=None)


def unit_ref(x, w1, b1, w2, b2, in_bn=None, bf16_gemm=False):
    """one ConvDPUnit with input transform none (in_bn None) or BN (running statistics) + ReLU -> dict(z, mag, amb,
    terms) for check_bf16.  x: the kernel's stored input widened to fp64."""
    r = R.fwd_ref(x, w1, b1, w2, b2, in_bn=in_bn, bf16_gemm=bf16_gemm)
    if in_bn is not None:
        x64 = x.detach().double().cpu()
        a = in_bn.act(x64)
        w1q = rne_bf16(w1.double().cpu()) if bf16_gemm else w1.double().cpu()
        r['amb'] = r['amb'] + _transform_amb(a, bn_err(in_bn, x64), w1q, w2.double().cpu(), bf16_gemm)
    return r


def pool_rule(z_stored, winners, idx, gamma, name='pool'):
    """fused max-pool winners: bf16_ref's tie rule with sign(gamma) of the running-statistics BN"""
    check_pool(name, z_stored, winners, idx, gamma)


def plain_pool_ref(z, bn):
    """pool_fwd on a pyramid tap: max_pool2d(relu(bn(z))) -> dict(z, mag, terms)"""
    z = z.double().cpu()
    a = bn.act(z)
    return dict(z=R.windows(a).amax(-1), mag=R.windows(bn_err(bn, z) / EPS32).amax(-1), terms=1, amb=None)


def _up2(t):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def upadd_ref(a, b, bn_a, bn_b):
    """TFPN merge: relu(bn_a(a)) + nearest-x2(relu(bn_b(b))) -> dict(z, mag, terms); the fp32 add is one more rounding
    of |z| <= mag"""
    a, b = a.double().cpu(), b.double().cpu()
    z = bn_a.act(a) + _up2(bn_b.act(b))
    mag = (bn_err(bn_a, a) + _up2(bn_err(bn_b, b))) / EPS32 + z.abs()
    return dict(z=z, mag=mag, terms=1, amb=None)


def heads_ref(x, sd, level, in_bn, bf16_gemm=False):
    """the 64 -> 16 head unit of a level (written as fp32 into flat) -> dict(z [N, h, w, 16], mag, amb, terms)"""
    return unit_ref(x, *head_weights(sd, level), in_bn=in_bn, bf16_gemm=bf16_gemm)


def flat_level(flat, sizes, level):
    """the [N, h, w, 16] view of one pyramid level of flat [N, P, 16]"""
    base = sum(h * w for h, w in sizes[:level])
    h, w = sizes[level]
    return flat[:, base:base + h * w].reshape(flat.shape[0], h, w, 16)


def check(name, got, r, stored):
    """per-element bar of a reference dict; stored: 'fp32' or 'bf16' (the storage of `got`)"""
    return check_bf16(name, got, r['z'], r['mag'], r['terms'], r.get('amb'), stored=stored)


# ------------------------------------------------------------------------------------------------ mode 2 sums
def synthesised_sums(rm, rv, count, slots=8):
    """what bn_batch_kernel mode 2 writes: slot 0 = [m count | (v + m^2) count], the other replicas zero"""
    m, v = rm.double(), rv.double()
    out = torch.zeros(slots, 2 * m.numel(), dtype=torch.float64)
    out[0] = torch.cat([m * count, (v + m * m) * count])
    return out


def recover(block, count, eps=1e-5):
    """mean and biased variance as common.h bn_coef recovers them from a [slots, 2C] block (bn_sum's pairwise order
    over the first eight replicas), and invstd in fp64"""
    c = block.shape[1] // 2
    v = torch.zeros(8, 2 * c, dtype=torch.float64)
    v[:min(8, block.shape[0])] = block[:8].double()
    s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))
    for k in range(8, block.shape[0]):
        s = s + block[k].double()
    inv = 1.0 / count
    mean = s[:c] * inv
    var = (s[c:] * inv - mean * mean).clamp_min(0.0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


class SumsBN(RunningBNRef):
    """a BatchNorm applied the way the kernels do in eval mode: coefficients recovered from a block of sums.  Used to
    emulate kernels (with and without defects) on the CPU; the reference never goes through it."""

    def __init__(self, block, count, gamma, beta, eps=1e-5):
        mean, var, _ = recover(block, count, eps)
        super().__init__(mean, var, gamma, beta, eps)


# ------------------------------------------------------------------------------------------------ end to end
def check_flat(name, got, ref, tol):
    """flat [N, P, 16] against the full fp64 network: |got - ref| <= tol max|ref over that output channel| per
    element (the cls logits are large next to the box / landmark channels: one global scale would hide those)"""
    got, ref = got.double().cpu(), ref.double().cpu()
    chmax = ref.abs().amax(dim=(0, 1), keepdim=True)
    bound = tol * chmax + 1e-300
    ratio = (got - ref).abs() / bound
    worst, msg = R._report(name, ratio, got, ref, bound.expand_as(ref))
    assert worst <= 1.0, msg
    return worst
