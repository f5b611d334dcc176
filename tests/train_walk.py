"""One training step (Plan.fwd_a, fwd_b, bwd) walked op by op against fp64, each op from its own stored inputs.
Host-only helper module (no GPU, no pytest fixtures), in the style of eval_ref.py and bf16_ref.py:
tests/test_train_walk.py shows on the CPU that walk() rejects the wiring defects it exists to catch,
tests/test_train_walk_gpu.py turns a live Plan into a Record and walks it.

The record.  After one forward_train + backward every activation, every fp32 gradient, every BatchNorm sum block and
every unit's weight-gradient partials are still on the device (Plan._new_t / _grad_of / Plan.bn: nothing is reused within
a step).  A Record holds them as CPU tensors under names, plus the graph as a list of nodes:

    stem                 image -> z, the sums of its BatchNorm, the weight gradient from the image
    unit                 a ConvDPUnit: x, z (stored | recomputed by the backward | elided), fused pool_out / pool_idx,
                         where its dy comes from (a tensor's gradient | rows of dflat x dy_scale), the accumulate flag,
                         its partials and the four gradients as they stand in the flat gradient (heads: z = rows of flat)
    pool                 max_pool2d as a kernel of its own (a pyramid tap), with the merge's share (`extra`) or without
    upadd                the TFPN merge, general (writes both gradients) or coarse-only (skip_a)
    fold, bn_run, bn_grad   the deterministic fold of a sum block; the BatchNorm table ops (running statistics; d(gamma), d(beta))

Teacher forcing: the reference of a node starts from the bytes that node read, so nothing builds up over the layers and
every node is held to the bar its kernel meets alone (all from tests/test_kernels_gpu.py unless named):

    what                              fp32 build                                   bf16 build
    forward z, forward sums           2e-5 of the tensor, 8e-5 per output          bf16_ref.check_bf16 per element (sums: that
                                      channel (test_dp_fwd, test_stem_fwd_bwd)      bound summed, over the UNROUNDED values)
    unit backward: dx, dw, db         5e-5, 4x per channel (bf16_ref.check_fp32,    bwd_ref(bf16_gemm) + its amb terms
                                      test_dp_bwd)
    BatchNorm backward sums           5e-5 (test_dp_bwd, test_pool_fwd_bwd)         the same (gradients are fp32)
    pool / merge output, dx           2e-5 (test_pool_fwd_bwd, test_upadd_fwd_bwd)  output: eval_ref's bound; dx: 2e-5
    stem weight gradient              1e-4 (test_stem_fwd_bwd)                      the same
    db2 / stem db behind a training   |db| < 1e-3 sum |dy| (identically zero;      the same
    BatchNorm                         test_dp_bwd)
    reduction of the partials         1e-5 (test_reduce_partials)                   the same
    d(gamma), d(beta)                 the fp32 of the block's replica sum in bn_sum's order, bit for bit
                                      (test_bn_batch_mode1_param_grad)
    running statistics                one fp32 ulp of the fp64 restatement of test_bn_batch_mode0_running_update
                                      (that test pins the compiled fmas bit for bit; the restatement has the fp32 one only)
    fold                              row 0 = the sum of the rows in yunet_bn_fold's documented order, bit for bit

A tensor's stored gradient is the SUM over its consumers (a unit, a plain pool, the merge's identity branch, the merge's
upsampled branch), each computed in fp64 from that consumer's own stored inputs; the bar of a sum is the sum of its
parts' bars.  This checks the accumulate flags and the extra / skip_a hand-over without a special case.  The BatchNorm
backward sums of a layer are taken over the STORED masked gradient and xhat of the STORED z, so they need no exemption.

ReLU decisions made by rounding: an element whose fp64 BatchNorm output is within MARGIN = 1e-4 of zero
(frozen_ref.off_threshold's margin) is ambiguous; the gradient it passes on may be the unmasked value or 0, so that
value's magnitude joins the element's bound.  At most one element in 1000 of a tensor may be ambiguous (off_threshold's
cap): asserted per tensor, counted in the printed line.

No bound here is derived from a HIP result.  Where a bar above cannot hold on in-place data, check_measured() evaluates the
same op on the same stored inputs in torch fp32 on the CPU, measures that against the fp64 reference and allows 4 x its
error (the kernel's summation order differs from torch's and must not be asked to beat it), never less than the bar.
profiles/train_walk.json holds the measurements of the GPU cases.  One check needed it: db1 of backbone.model0.conv2 in
the YuNet_n fp32 cases -- behind a training BatchNorm sum(dz) = 0, so the pointwise bias gradient is what the depthwise
convolution's zero padding leaves at the border of a 64 x 160 map; torch fp32 is off by 1.7e-5 .. 3.4e-5 of the tensor
there, the kernel by 5.5e-5 .. 6.4e-5, against the bar of 5e-5.  tests/test_train_walk_gpu.py lets no other check use a
measured bound."""
import contextlib
import io
import re
import types

import torch
import torch.nn.functional as F

import bf16_ref as R
import eval_ref as E

MARGIN = 1e-4
AMB_CAP = 1000
TOL_FWD, TOL_BWD, TOL_EW, TOL_SUMS, TOL_STEM, TOL_REDUCE = 2e-5, 5e-5, 2e-5, 5e-5, 1e-4, 1e-5
F64 = torch.float64
NS = types.SimpleNamespace


# ------------------------------------------------------------------------------------------------ the record
class Record:
    """Named tensors and the graph of one training step.  build: 'fp32' | 'bf16' (activation storage)."""

    def __init__(self, build, img, momentum=0.1):
        self.build, self.img, self.momentum = build, img, momentum
        self.tensors, self.bn, self.nodes = {}, {}, []
        self.frozen = {}              # state_dict key -> its range of the flat gradient (must be exactly zero)
        self.flat = self.dflat = None

    def tensor(self, name, buf, shape, bn=None, grad=None):
        """an activation: buf NHWC (None: elided), shape (n, h, w, c), bn = the layer its consumers apply, grad fp32 | None"""
        n, h, w, c = shape
        self.tensors[name] = NS(name=name, buf=buf, n=n, h=h, w=w, c=c, bn=bn, grad=grad)
        return self.tensors[name]

    def layer(self, name, **kw):
        """a BatchNorm layer: c, stats / bstats [rows, 2c] fp64, slots (rows the readers add up), gamma, beta, frozen,
        rm0 rv0 nbt0 (before the step) rm1 rv1 nbt1 (after), dgamma dbeta (the flat gradient's | None), counts (the
        counts the op records carried, or None)"""
        self.bn[name] = NS(name=name, counts=None, **kw)
        return self.bn[name]

    def node(self, kind, name, **kw):
        self.nodes.append(NS(kind=kind, name=name, **kw))
        return self.nodes[-1]


def slot_sum(block, slots):
    """what a reader takes from a [rows, 2c] block: common.h bn_sum's order over the first `slots` replicas"""
    v = torch.zeros(8, block.shape[1], dtype=F64)
    v[:min(8, slots)] = block[:min(8, slots)].double()
    s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))
    for k in range(8, slots):
        s = s + block[k].double()
    return s


def fold_rows(block):
    """yunet_bn_fold's documented order over rows 1..: slice s adds rows 1 + s, 1 + s + 16, ... ascending from 0.0, then
    the sixteen slice sums are added in ascending s from 0.0"""
    rows = block[1:].double()
    pad = (-rows.shape[0]) % 16
    rows = torch.cat([rows, torch.zeros(pad, rows.shape[1], dtype=F64)]).view(-1, 16, rows.shape[1])
    acc = torch.zeros(16, rows.shape[2], dtype=F64)
    for k in range(rows.shape[0]):
        acc = acc + rows[k]
    out = torch.zeros(rows.shape[2], dtype=F64)
    for s in range(16):
        out = out + acc[s]
    return out


class WalkError(AssertionError):
    def __init__(self, failed):
        self.failed = failed          # [(node name, message)]
        self.nodes = [n for n, _ in failed]
        super().__init__('train walk failed at: ' + '; '.join(f'{n}: {m}' for n, m in failed[:6]))


# ------------------------------------------------------------------------------------------------ torch evaluation of one node
# The same ops in plain torch in a given dtype, from stored inputs: torch fp32 on the CPU is how tests/test_train_walk.py
# builds its record, and the yardstick a measured bound would come from.
def bn_coef(stats, count, gamma, beta, dtype, eps=1e-5):
    """(mean, invstd, gamma, beta) as a kernel derives them: fp64 from the sums, then the arithmetic's type"""
    c = gamma.numel()
    s = stats.double()
    mean = s[:c] / count
    var = (s[c:] / count - mean * mean).clamp_min(0.0)
    return NS(mean=mean.to(dtype), inv=(1.0 / torch.sqrt(var + eps)).to(dtype), gamma=gamma.to(dtype), beta=beta.to(dtype),
              count=count)


def running_coef(rm, rv, gamma, beta, dtype, eps=1e-5, count=1):
    return NS(mean=rm.double().to(dtype), inv=(1.0 / torch.sqrt(rv.double() + eps)).to(dtype), gamma=gamma.to(dtype),
              beta=beta.to(dtype), count=count)


def t_act(x, bn):
    xh = (x - bn.mean) * bn.inv
    y = xh * bn.gamma + bn.beta
    return F.relu(y), xh, y > 0


def t_unit_fwd(x, w, in_bn, dtype):
    x = x.to(dtype)
    a = t_act(x, in_bn)[0] if in_bn is not None else x
    w1, b1, w2, b2 = [t.to(dtype) for t in w]
    return R.depthwise(a @ w1.t() + b1, w2, b2)


def t_sums(d, xh):
    d, xh = d.double(), xh.double()
    return torch.cat([d.sum((0, 1, 2)), (d * xh).sum((0, 1, 2))])


def t_unit_bwd(x, w, z, dy, in_bn, out_bn, bst, dy_scale, dtype, per_image=True, bf16_operand=False):
    """-> dx (masked), partial rows [N, width] (one per image; W_pw | b_pw | W_dw | b_dw), the sums added to the input layer.
    dy: full size.  out_bn with bst [2c] = the sums its reader takes.  bf16_operand: the defect of a backward GEMM operand
    (a) rounded to bf16."""
    x, dy = x.to(dtype), dy.to(dtype)
    w1, b1, w2, b2 = [t.to(dtype) for t in w]
    if in_bn is not None:
        a, xh_in, mask = t_act(x, in_bn)
    else:
        a, xh_in, mask = x, None, None
    if z is None:
        z = R.depthwise(a @ w1.t() + b1, w2, b2)
    if out_bn is not None:
        c = w1.shape[0]
        xh = (z.to(dtype) - out_bn.mean) * out_bn.inv
        s = (bst.double() / out_bn.count).to(dtype)
        dz = out_bn.gamma * out_bn.inv * (dy - s[:c] - xh * s[c:])
    else:
        dz = dy * (dy_scale.to(dtype) if dy_scale is not None else 1.0)
    if bf16_operand:
        a = a.to(torch.bfloat16).to(dtype)
    rows, das = [], []
    for i in range(x.shape[0]) if per_image else [slice(None)]:
        sl = slice(i, i + 1) if per_image else i
        ai = a[sl].clone().requires_grad_(True)
        P = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
        (R.depthwise(ai @ P[0].t() + P[1], P[2], P[3]) * dz[sl]).sum().backward()
        rows.append(torch.cat([p.grad.reshape(-1) for p in P]))
        das.append(ai.grad)
    da = torch.cat(das)
    dx = da * mask if mask is not None else da
    return dx, torch.stack(rows), (t_sums(dx, xh_in) if xh_in is not None else None)


def t_pool_bwd(z, bn, dout, dtype):
    y = ((z.to(dtype) - bn.mean) * bn.inv * bn.gamma + bn.beta).requires_grad_(True)
    out = F.max_pool2d(F.relu(y).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    (out * dout.to(dtype)).sum().backward()
    return y.grad


def up2(t):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def down2(t):
    n, h, w, c = t.shape
    return t.reshape(n, h // 2, 2, w // 2, 2, c).sum((2, 4))


def t_stem_bwd(img, w, b, dy, bn, bst, dtype, frozen=False, per_image=True):
    """-> partial rows [N, 16 * 27 + 16] of the stem's weight and bias gradient (z recomputed from the image)"""
    img, dy = img.to(dtype), dy.to(dtype)
    rows = []
    z = F.conv2d(img, w.to(dtype).view(16, 3, 3, 3), b.to(dtype), stride=2, padding=1).permute(0, 2, 3, 1)
    xh = (z - bn.mean) * bn.inv
    s = (bst.double() / bn.count).to(dtype)
    dz = bn.gamma * bn.inv * (dy - s[:16] - xh * s[16:])
    for i in range(img.shape[0]) if per_image else [slice(None)]:
        sl = slice(i, i + 1) if per_image else i
        W, B = w.to(dtype).view(16, 3, 3, 3).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)
        (F.conv2d(img[sl], W, B, stride=2, padding=1).permute(0, 2, 3, 1) * dz[sl]).sum().backward()
        rows.append(torch.cat([W.grad.reshape(-1), B.grad]))
    return torch.stack(rows)


def running_update(stats, count, rm, rv, momentum):
    """nn.BatchNorm2d's update from the fp64 sums, as yunet_bn_batch mode 0 orders it (fp32 blend of the fp64 mean and
    unbiased variance rounded to fp32); the compiled kernel's two fmas are not restated -> within one fp32 ulp of it"""
    c = rm.numel()
    s = stats.double()
    mean = s[:c] / count
    var = (s[c:] / count - mean * mean).clamp_min(0.0)
    unb = var * (count / (count - 1.0)) if count > 1 else var
    mom = torch.tensor(momentum, dtype=torch.float32)
    one_m = torch.tensor(1.0, dtype=torch.float32) - mom
    rv1 = (mom.double() * unb.float().double() + (one_m * rv.float()).double()).float()        # fma(mom, unbiased, (1 - mom) v)
    return mom * mean.float() + one_m * rm.float(), rv1


# ------------------------------------------------------------------------------------------------ the walk
class _Walk:
    def __init__(self, rec):
        self.rec, self.bf = rec, rec.build == 'bf16'
        self.stored = rec.build
        self.worst, self.failed, self.amb, self.measured = {}, [], {}, []
        self.contrib = {}             # tensor name -> [(kind, ref dx fp64, tol, |unmasked| fp64)]
        self.count = {}               # BatchNorm layer -> elements per channel, from its producer's geometry
        self.walked = []              # (node name, kernel ops it stands for)

    # ---- plumbing
    def ratio(self, fn, *a, **kw):
        """run a bf16_ref / eval_ref checker quietly -> (worst error / bound, its message when above 1)"""
        out = io.StringIO()
        try:
            with contextlib.redirect_stdout(out):
                return float(fn(*a, **kw) or 0.0), None
        except AssertionError as e:
            m = re.search(r'worst error / bound ([0-9.eE+\-infa]+)', str(e))
            w = float(m.group(1)) if m else float('inf')
            return (w if w > 1.0 else float('inf')), str(e).splitlines()[0][:240]

    def check(self, node, fn, *a, **kw):
        """a failure is filed under the node and the walk goes on"""
        w, msg = self.ratio(fn, *a, **kw)
        if msg is not None:
            self.failed.append((node, msg))
        self.worst[node] = max(self.worst.get(node, 0.0), w)
        return w

    def check_measured(self, node, what, eval32, got, ref, tol, **kw):
        """check_fp32 at the project bar; where that bar does not hold on in-place data (a cancelling sum: a bias gradient
        behind a BatchNorm, the stem's weight gradient on a real image), 4 x the error of torch fp32 on the CPU on the same
        stored inputs against the same fp64 reference -- never less than the bar.  The measurement is filed in `measured`."""
        w, msg = self.ratio(R.check_fp32, f'{node} {what}', got, ref, tol, **kw)
        if msg is not None:
            w32, _ = self.ratio(R.check_fp32, f'{node} {what} torch fp32', eval32()[what].reshape(ref.shape), ref, tol, **kw)
            allowed = max(1.0, 4.0 * w32)
            self.measured.append(dict(node=node, check=what, bar=tol, torch_fp32_error=w32 * tol, bound=allowed * tol,
                                      kernel_error=w * tol))
            w = w / allowed
            if w > 1.0:
                self.failed.append((node, msg + f' (torch fp32: {w32:.3g} of the bar)'))
        self.worst[node] = max(self.worst.get(node, 0.0), w)
        return w

    def coef32(self, layer):
        b = self.rec.bn[layer]
        if b.frozen:
            return running_coef(b.rm0, b.rv0, b.gamma, b.beta, torch.float32, count=self.count[layer])
        return bn_coef(slot_sum(b.stats, b.slots), self.count[layer], b.gamma, b.beta, torch.float32)

    def exact(self, node, what, ok):
        self.worst.setdefault(node, 0.0)
        if not ok:
            self.worst[node] = float('inf')
            self.failed.append((node, what))

    def bnref(self, name, bstats=None):
        b = self.rec.bn[name]
        if b.frozen:
            ref = R.RunningBNRef(b.rm0, b.rv0, b.gamma, b.beta)
            ref.count, ref.bstats = self.count[name], None if bstats is None else bstats.double()
            return ref
        return R.BNRef(slot_sum(b.stats, b.slots), b.gamma, b.beta, self.count[name], bstats=bstats)

    def add(self, tname, kind, dx, tol, da):
        self.contrib.setdefault(tname, []).append((kind, dx.double(), tol, da.double().abs()))

    # ---- forward pieces
    def sums(self, node, layer, z_stored, r):
        """forward sums of `layer` against the sums of the stored z (fp32 build) | of the fp64 z (bf16; an elided z)"""
        b = self.rec.bn[layer]
        c = b.c
        if b.frozen:       # yunet_bn_batch mode 2 (frozen_ref.block): replica 0 exactly, the others zero
            import frozen_ref as FZ
            want = torch.zeros_like(b.stats)
            want[0] = FZ.block(b.rm0.double(), b.rv0.double(), self.count[layer])
            self.exact(node, f'{layer}: frozen sums are not the running statistics', torch.equal(b.stats[:max(b.slots, 1)],
                                                                                                  want[:max(b.slots, 1)]))
            return
        got = slot_sum(b.stats, b.slots)
        if self.bf:        # over the UNROUNDED values: check_bf16's bound without the storage ulp, summed per channel
            z = r['z']
            el = r['terms'] * R.EPS32 * r['mag'] + (r['amb'] if r.get('amb') is not None else 0.0)
            amb = torch.cat([el.sum((0, 1, 2)), (2 * z.abs() * el + el * el).sum((0, 1, 2))])
            self.check(node, R.check_fp32, f'{node} sums', got, R.stats_of(z), 0.0, amb=amb)
            return
        ref = R.stats_of(z_stored if z_stored is not None else r['z'])
        self.check(node, R.check_fp32, f'{node} sums', got, ref, TOL_FWD)
        self.check(node, R.check_fp32, f'{node} sums of squares', got[c:], ref[c:], TOL_FWD, ch_dim=0)

    def z_check(self, node, got, r, stored):
        if self.bf:
            self.check(node, E.check, node, got, r, stored)
        else:
            self.check(node, R.check_fp32, node, got, r['z'], TOL_FWD, ch_dim=-1)

    def elided_pool(self, node, r, winners, idx, gamma):
        """winners of an elided z against the fp64 z at the forward bar; a position may differ only where the window's two
        candidates' transformed values lie within that bar of each other"""
        z = r['z']
        if self.bf:
            bar = R.ulp_bf16(z) + r['terms'] * R.EPS32 * r['mag'] + (r['amb'] if r.get('amb') is not None else 0.0)
        else:
            bar = torch.full_like(z, TOL_FWD * float(z.abs().max()))
        key = R.windows(z) * torch.sign(gamma.double()).view(1, 1, 1, -1, 1)
        want, got = key.argmax(-1, keepdim=True), idx.long().unsqueeze(-1)
        gap = (key.gather(-1, want) - key.gather(-1, got)).squeeze(-1)
        bad = (got != want).squeeze(-1) & (gap > R.windows(bar).gather(-1, want).squeeze(-1))
        self.exact(node, f'{int(bad.sum())} window positions off the rule beyond the forward bar', not bool(bad.any()))
        at = {k: R.windows(v).gather(-1, got).squeeze(-1) for k, v in r.items() if torch.is_tensor(v)}
        at['terms'] = r['terms']
        self.z_check(node, winners, at, self.stored)

    # ---- nodes
    def stem(self, nd):
        rec = self.rec
        zt = rec.tensors[nd.z]
        self.count[nd.out_bn] = zt.n * zt.h * zt.w
        r = E.stem_ref(rec.img, nd.w[0].view(16, 3, 3, 3), nd.w[1])
        self.z_check(nd.name, zt.buf, r, self.stored)
        self.sums(nd.name, nd.out_bn, zt.buf, r)
        ops = 1
        if nd.bwd:
            ops += 1
            b = rec.bn[nd.out_bn]
            bst = torch.zeros(2 * b.c, dtype=F64) if b.frozen else slot_sum(b.bstats, b.slots)
            bn = self.bnref(nd.out_bn)
            mean, inv = bn.mean_invstd()
            coef = NS(mean=mean, inv=inv, gamma=bn.gamma, beta=bn.beta, count=self.count[nd.out_bn])
            row = t_stem_bwd(rec.img, nd.w[0], nd.w[1], zt.grad, coef, bst, F64, per_image=False)[0]
            if nd.g is not None:
                ev = {}

                def eval32():
                    if not ev:
                        r32 = t_stem_bwd(rec.img, nd.w[0], nd.w[1], zt.grad, self.coef32(nd.out_bn), bst, torch.float32,
                                         per_image=False)[0]
                        ev.update(dw=r32[:432], db=r32[432:])
                    return ev
                self.check_measured(nd.name, 'dw', eval32, nd.g[0], row[:432], TOL_STEM)
                if b.frozen:
                    self.check_measured(nd.name, 'db', eval32, nd.g[1], row[432:], TOL_STEM)
                else:
                    self.exact(nd.name, 'stem db is not noise', float(nd.g[1].abs().max()) < 1e-3 * float(zt.grad.abs().sum()))
                self.reduce(nd)
        self.walked.append((nd.name, ops))

    def reduce(self, nd):
        if nd.partials is None:
            return
        name = f'reduce {nd.name}'
        got = torch.cat([g.reshape(-1) for g in nd.g])
        self.check(name, R.check_fp32, name, got, nd.partials[:nd.rows].double().sum(0), TOL_REDUCE)

    def unit(self, nd):
        rec = self.rec
        x = rec.tensors[nd.x]
        cout, cin = nd.w[0].shape
        if nd.out_bn:
            self.count[nd.out_bn] = x.n * x.h * x.w
        in_bn = self.bnref(x.bn) if x.bn else None
        gemm = self.bf and cin % 32 == 0
        r = E.unit_ref(x.buf, *nd.w, in_bn=in_bn, bf16_gemm=gemm) if self.bf else \
            R.fwd_ref(x.buf, *nd.w, in_bn=in_bn)
        zt = rec.tensors[nd.z] if nd.z else None
        z_stored = zt.buf if zt is not None else nd.flat_rows
        if z_stored is not None:
            self.z_check(nd.name, z_stored, r, self.stored if zt is not None else 'fp32')
        else:
            self.exact(nd.name, 'z neither stored nor elided', nd.zmode == 'elided')
        if nd.out_bn:
            self.sums(nd.name, nd.out_bn, z_stored, r)
        if nd.pool_out:
            pt, gamma = rec.tensors[nd.pool_out], rec.bn[nd.out_bn].gamma
            if z_stored is not None:
                self.check(nd.name, R.check_pool, nd.name, z_stored, pt.buf, nd.pool_idx, gamma)
            else:
                self.elided_pool(nd.name, r, pt.buf, nd.pool_idx, gamma)
        ops = 1
        if nd.bwd:
            ops += 1
            self.unit_bwd(nd, x, in_bn, zt, cin, cout)
        self.walked.append((nd.name, ops))

    def unit_bwd(self, nd, x, in_bn, zt, cin, cout):
        rec = self.rec
        out_bn = None
        if nd.out_bn:
            b = rec.bn[nd.out_bn]
            out_bn = self.bnref(nd.out_bn, bstats=torch.zeros(2 * b.c, dtype=F64) if b.frozen else slot_sum(b.bstats, b.slots))
        pool_idx = None
        if nd.dy[0] == 'grad':
            dy = rec.tensors[nd.dy[1]].grad
            pool_idx = nd.pool_idx if nd.dy[1] == nd.pool_out else None
        else:
            dy = nd.dy[1]
        stored = zt is not None and zt.buf is not None and nd.zmode == 'stored'
        z = zt.buf if stored else (nd.flat_rows if zt is None else None)
        ref = R.bwd_ref(x.buf, *nd.w, z=z if z is not None else torch.zeros(1), dy=dy, in_bn=in_bn, out_bn=out_bn,
                        dy_scale=nd.dy_scale, bf16_gemm=self.bf and cin == 64 and cout == 64, recompute_z=z is None,
                        pool_idx=pool_idx)
        self.add(nd.x, 'unit', ref['dx'], TOL_BWD, ref['da'])
        if nd.g is None:
            return
        amb, nm = ref['amb'], nd.name
        full = R.expand_pooled(dy, pool_idx) if pool_idx is not None else dy.double()
        ev = {}

        def eval32():
            if not ev:
                rows = t_unit_bwd(x.buf.float(), nd.w, None if z is None else z.float(), full.float(),
                                  self.coef32(x.bn) if x.bn else None, self.coef32(nd.out_bn) if out_bn is not None else None,
                                  None if out_bn is None else out_bn.bstats, nd.dy_scale, torch.float32, per_image=False)[1]
                ev.update(zip(('dw1', 'db1', 'dw2', 'db2'), torch.split(rows[0], [cout * cin, cout, cout * 9, cout])))
            return ev
        self.check_measured(nm, 'dw1', eval32, nd.g[0].reshape(cout, cin), ref['dw1'], TOL_BWD, amb=amb['dw1'], ch_dim=0)
        self.check_measured(nm, 'db1', eval32, nd.g[1], ref['db1'], TOL_BWD)
        self.check_measured(nm, 'dw2', eval32, nd.g[2].reshape(cout, 9), ref['dw2'], TOL_BWD, amb=amb['dw2'])
        if out_bn is not None and not rec.bn[nd.out_bn].frozen:
            self.exact(nm, 'db2 behind a training BatchNorm is not noise',
                       float(nd.g[3].abs().max()) < 1e-3 * float(full.abs().sum()))
        else:
            self.check_measured(nm, 'db2', eval32, nd.g[3], ref['db2'], TOL_BWD)
        self.reduce(nd)

    def pool(self, nd):
        rec = self.rec
        x, out = rec.tensors[nd.x], rec.tensors[nd.out]
        bn = self.bnref(x.bn)
        r = E.plain_pool_ref(x.buf, bn)
        name = nd.name
        if self.bf:
            self.check(name, E.check, name, out.buf, r, 'bf16')
        else:
            self.check(name, R.check_fp32, name, out.buf, r['z'], TOL_EW)
        ops = 1
        if nd.bwd:
            ops += 1
            mean, inv = bn.mean_invstd()
            coef = NS(mean=mean, inv=inv, gamma=bn.gamma, beta=bn.beta)
            dx = t_pool_bwd(x.buf.double(), coef, out.grad.double(), F64)
            # unmasked: the whole window's gradient at every element, read only where the element is ambiguous
            self.add(nd.x, 'pool', dx, TOL_EW, up2(out.grad.double()))
        self.walked.append((name, ops))

    def upadd(self, nd):
        rec = self.rec
        a, b, out = rec.tensors[nd.a], rec.tensors[nd.b], rec.tensors[nd.out]
        bna, bnb = self.bnref(a.bn), self.bnref(b.bn)
        name = nd.name
        if self.bf:
            self.check(name, E.check, name, out.buf, E.upadd_ref(a.buf, b.buf, bna, bnb), 'bf16')
        else:
            self.check(name, R.check_fp32, name, out.buf, bna.act(a.buf.double()) + up2(bnb.act(b.buf.double())), TOL_EW)
        ops = 1
        if nd.bwd:
            ops += 1
            g = out.grad.double()
            ya = bna.xhat(a.buf.double()) * bna.gamma + bna.beta
            yb = bnb.xhat(b.buf.double()) * bnb.gamma + bnb.beta
            self.add(nd.a, 'merge identity', g * (ya > 0), TOL_EW, g)
            gb = down2(g)
            self.add(nd.b, 'merge upsampled', gb * (yb > 0), TOL_EW, gb)
        self.walked.append((name, ops))

    def fold(self, nd):
        b = self.rec.bn[nd.layer]
        block = b.bstats if nd.backward else b.stats
        self.exact(nd.name, 'row 0 is not the fixed-order sum of the rows', torch.equal(block[0], fold_rows(block)))
        self.walked.append((nd.name, 0))

    def bn_run(self, nd):
        rec = self.rec
        for name, b in rec.bn.items():
            tag = f'{nd.name} {name}'
            if name not in nd.layers:
                same = torch.equal(b.rm0, b.rm1) and torch.equal(b.rv0, b.rv1) and int(b.nbt0) == int(b.nbt1)
                self.exact(nd.name, f'{name}: a layer outside the table moved', same)
                continue
            rm, rv = running_update(slot_sum(b.stats, b.slots), self.count[name], b.rm0, b.rv0, rec.momentum)
            ulp = lambda t: torch.ldexp(torch.ones_like(t), torch.frexp(t)[1] - 24).double() + 1e-300
            self.check(nd.name, R.check_fp32, tag + ' mean', b.rm1, rm.double(), 0.0, amb=ulp(rm))
            self.check(nd.name, R.check_fp32, tag + ' var', b.rv1, rv.double(), 0.0, amb=ulp(rv))
            self.exact(nd.name, f'{name}: num_batches_tracked', int(b.nbt1) == int(b.nbt0) + 1)
        self.walked.append((nd.name, getattr(nd, 'ops', 1)))

    def bn_fill(self, nd):
        """the frozen layers' sums from their running statistics: each block is checked with its producer (sums())"""
        self.exact(nd.name, 'a training layer in the fill table', all(self.rec.bn[n].frozen for n in nd.layers))
        self.walked.append((nd.name, 1))

    def reduce_batch(self, nd):
        """one launch over a table of jobs: every job's result is checked with its unit (reduce())"""
        self.worst.setdefault(nd.name, 0.0)
        self.walked.append((nd.name, 1))

    def bn_grad(self, nd):
        for name in nd.layers:
            b = self.rec.bn[name]
            s = slot_sum(b.bstats, b.slots).float()
            self.exact(nd.name, f'{name}: d(beta) is not the fp32 of its block sum', torch.equal(b.dbeta, s[:b.c]))
            self.exact(nd.name, f'{name}: d(gamma) is not the fp32 of its block sum', torch.equal(b.dgamma, s[b.c:]))
        self.walked.append((nd.name, 1))

    # ---- per tensor, per layer
    def tensor_grads(self):
        rec = self.rec
        for name, t in rec.tensors.items():
            node = f'grad {name}'
            parts = self.contrib.get(name, [])
            if t.grad is None:
                if parts:
                    self.exact(node, 'consumers ran a backward but the tensor has no gradient', False)
                continue
            if not parts:
                self.exact(node, 'a stored gradient without a consumer', False)
                continue
            ref = sum(p[1] for p in parts)
            amb = torch.zeros_like(ref)
            n_amb = 0
            if t.bn is not None:
                bn = self.bnref(t.bn)
                y = bn.xhat(t.buf.double()) * bn.gamma + bn.beta
                near = y.abs() < MARGIN
                n_amb = int(near.sum())
                amb = torch.where(near, sum(p[3] for p in parts), amb)
            self.amb[name] = (n_amb, ref.numel())
            self.exact(node, f'{n_amb} of {ref.numel()} elements within {MARGIN} of the ReLU threshold: above one in {AMB_CAP}',
                       n_amb * AMB_CAP <= ref.numel())
            scale = float(ref.abs().max())
            tol = sum(p[2] * float(p[1].abs().max()) for p in parts) / scale if scale > 0 else TOL_BWD
            self.check(node, R.check_fp32, node, t.grad, ref, tol, amb=amb, ch_dim=-1 if any(p[0] == 'unit' for p in parts) else None)

    def layer_sums(self):
        rec = self.rec
        for name, b in rec.bn.items():
            node = f'bstats {name}'
            carriers = [t for t in rec.tensors.values() if t.bn == name and t.grad is not None]
            got = slot_sum(b.bstats, b.slots)
            if not carriers:
                self.exact(node, 'backward sums without a gradient', not bool(got.any()))
                continue
            bn = self.bnref(name)
            ref = sum(t_sums(t.grad, bn.xhat(t.buf.double())) for t in carriers)
            self.check(node, R.check_fp32, node, got, ref, TOL_SUMS)
            if b.counts is not None:
                self.exact(node, f'the op records carry counts {sorted(b.counts)}, the producer has {self.count[name]}',
                           set(b.counts) == {self.count[name]})

    def run(self):
        rec = self.rec
        for nd in rec.nodes:
            getattr(self, nd.kind)(nd)
        self.tensor_grads()
        self.layer_sums()
        for key, g in rec.frozen.items():
            self.exact(f'frozen {key}', 'the frozen range of the flat gradient is not zero', not bool(g.any()))
        return self


def walk(rec, tag='', quiet=False, raise_on_fail=True):
    """Check every node of the record -> {node name: worst error / bound}.  Prints one line per node (and, for a
    tensor's gradient, its count of ambiguous elements); raises WalkError naming the failing nodes."""
    w = _Walk(rec).run()
    if not quiet:
        print(f'[train walk {tag}] worst error / bound per node:')
        for k, v in w.worst.items():
            amb = w.amb.get(k[5:]) if k.startswith('grad ') else None
            print(f'    {k:64s} {v:9.3g}' + (f'   ambiguous {amb[0]} of {amb[1]}' if amb else ''))
    rec.walked, rec.amb, rec.measured = w.walked, w.amb, w.measured
    for m in w.measured:
        if not quiet:
            print(f"    measured bound: {m['node']} {m['check']}: torch fp32 {m['torch_fp32_error']:.3g}, bound {m['bound']:.3g}, "
                  f"kernel {m['kernel_error']:.3g} (bar {m['bar']:.3g})")
    if w.failed and raise_on_fail:
        raise WalkError(w.failed)
    rec.failed = w.failed
    return w.worst


# ------------------------------------------------------------------------------------------------ the GPU cases
# One geometry reaches, for both shipped nets and both builds, exactly the kernel instances yunet_dp_route names at the
# benchmark shape (the big-tile and wave-streaming classes at the first units, fused pooling, packed canvases at the
# 16 x 40 / 8 x 20 / 4 x 10 levels, dp_bwd64 on 8 x 8 and on 8 x 16 tiles): tests/test_train_walk.py asserts the equality
# of the two sets for every case, so a routing change that empties a case fails there.  Persistent-grid walking (thousands
# of tiles per launch) is no wiring matter and stays with test_kernels_gpu.py's BIG_SHAPES.
GEOMETRY = (4, 128, 320)
BENCH = {'n': (256, 320, 320), 's': (512, 320, 320)}
_CASE = dict(kind='n', precision='fp32', deterministic=False, finetune=False, keep_pool_z=False)
CASES = {
    'n_fp32': dict(_CASE, seed=3),
    's_fp32': dict(_CASE, kind='s', seed=3),
    'n_bf16': dict(_CASE, precision='bf16', seed=3),
    'n_det': dict(_CASE, deterministic=True, seed=3),
    'n_det_fast': dict(_CASE, deterministic='fast', seed=3),
    'n_finetune': dict(_CASE, finetune=True, seed=3),
    'n_keep_pool_z': dict(_CASE, keep_pool_z=True, seed=3),
}


def finetune_signature(layout, stages=2):
    """(frozen BatchNorm layers, frozen parameter keys) of backbone norm_eval=True with frozen_stages=`stages`"""
    bn = tuple(n for n in layout.bn_names if n.startswith('backbone.'))
    pre = tuple(f'backbone.model{i}.' for i in range(stages + 1))
    return bn, tuple(k for k in layout.entries if k.startswith(pre))


def plan_routes(plan):
    """the kernel instance names of every ConvDPUnit launch of the plan's training lists"""
    import route_cases
    import yunet_amd._lib as L
    lib = L.load()
    return {route_cases.route(lib, op.dp, int(op.opcode == L.OP_DP_BWD)) for arr in (plan.c_fwd_a, plan.c_bwd) for op in arr
            if op.opcode in (L.OP_DP_FWD, L.OP_DP_BWD)}
