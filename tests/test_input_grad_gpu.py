"""-m gpu: the gradient with respect to the input image.

1, 2, 7 pin the kernel (`yunet_stem_bwd_dx[_bf16]`): against fp64 autograd at the bar of the plain units' dx (5e-5,
tests/test_kernels_gpu.py), tap by tap with one-hot gradients, and at its refusals.  3 pins the stand-alone stem
(`functional.stem`), 4 - 6 the fused engine: `img.grad` of YuNet.forward_train against an fp64 evaluation of
d sum(flat * dflat) / d img over the oracle's conv stack -- helpers.fp64_conv_grads with the image as the leaf -- by the rule
of tests/test_engine_gpu.py::test_forward_train_vs_oracle: the HIP error within 10 x the fp32 oracle's own error (floored at
1e-5 of the tensor) plus 1 % of the tensor.  Shapes are the smallest that reach every path: 64 x 64 images, batch 2."""
import ctypes as C
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import finetune_ref as FR
import yunet_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5


def K():
    import yunet_amd.kernels as k
    return k


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def bytes_of(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()


def rne_bf16(t):
    return t.float().bfloat16().to(t.dtype)


# ================================================================================================ 1. kernel against fp64
# (N, H, W): one tile, a partial second tile in x, two tiles in y with several images, and one whose 16 x 32 z-pixel tiles split both dimensions in three with partial last
# tiles (36 = 16 + 16 + 4 rows, 69 = 32 + 32 + 5 columns) and whose width 138 = 4 m + 2 takes the 8-byte store path
SHAPES = [(2, 32, 32), (1, 32, 96), (3, 64, 32), (1, 72, 138)]


def stem_case(n, h, w, seed):
    gen = torch.Generator().manual_seed(seed)
    img = torch.rand(n, 3, h, w, generator=gen) * 255.0
    wt = torch.randn(16, 3, 3, 3, generator=gen) * 0.05
    b = torch.randn(16, generator=gen) * 0.1
    gamma = (0.5 + torch.rand(16, generator=gen)) * torch.where(torch.rand(16, generator=gen) < 0.25, -1.0, 1.0)
    beta = torch.randn(16, generator=gen) * 0.1
    up = torch.randn(n, 16, h // 2, w // 2, generator=gen)
    dy = up * (torch.rand(up.shape, generator=gen) < 0.6)                 # a random ReLU mask applied
    rm = torch.randn(16, generator=gen) * 2.0
    rv = 1.0 + 4.0 * torch.rand(16, generator=gen)
    return img, wt, b, gamma, beta, dy, rm, rv


def dz_formula(z, dy, mean, invstd, gamma, count, frozen):
    """dz = scale (dy - (sum dy + xhat sum(dy xhat)) / count), NCHW fp64; frozen: scale dy."""
    v = lambda t: t.view(1, -1, 1, 1)
    scale = gamma * invstd
    if frozen:
        return v(scale) * dy
    xhat = (z - v(mean)) * v(invstd)
    s1, s2 = dy.sum(dim=(0, 2, 3)), (dy * xhat).sum(dim=(0, 2, 3))
    return v(scale) * (dy - (v(s1) + xhat * v(s2)) / count)


def reference(img, wt, b, gamma, beta, dy, rm, rv, frozen, z_round=False):
    """fp64: conv2d(stride 2, pad 1) -> BatchNorm -> sum(y * dy) -> autograd to the image.  z_round: the backward sees z
    rounded to bf16 (the statistics stay those of the unrounded z, as the forward kernel takes them): the same formula
    written out, which the unrounded case checks against autograd."""
    x = img.double().clone().requires_grad_(True)
    w64, g64, dy64 = wt.double(), gamma.double(), dy.double()
    z = F.conv2d(x, w64, b.double(), stride=2, padding=1)
    if frozen:
        y = F.batch_norm(z, rm.double(), rv.double(), g64, beta.double(), training=False, eps=EPS)
    else:
        y = F.batch_norm(z, None, None, g64, beta.double(), training=True, eps=EPS)
    (y * dy64).sum().backward()
    zd = z.detach()
    count = zd.numel() // 16
    mean = rm.double() if frozen else zd.mean(dim=(0, 2, 3))
    var = rv.double() if frozen else zd.var(dim=(0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    by_formula = lambda zz: F.conv_transpose2d(dz_formula(zz, dy64, mean, invstd, g64, count, frozen), w64, stride=2,
                                               padding=1, output_padding=1)
    assert rel_err(by_formula(zd), x.grad) < 1e-12
    return by_formula(rne_bf16(zd)) if z_round else x.grad


def run_kernel(img, wt, b, gamma, beta, dy, rm, rv, frozen, dtype):
    """The inputs as functional._StemFn builds them: z and its sums from the forward kernel of the storage build, the
    backward sums from the same dy in torch (zero for a frozen layer)."""
    import yunet_amd.functional as Fn
    k = K()
    d = lambda t: t.to(DEV).contiguous()
    stats = torch.zeros(32, device=DEV, dtype=torch.float64)
    z = k.stem_fwd(d(img), d(wt), d(b), stats, dtype=dtype)
    count = z.numel() // 16
    if frozen:
        stats = Fn._sums_from_moments(d(rm), d(rv), count)
    dyh = d(nhwc(dy))
    mean, invstd, _ = Fn._bn_coef(stats, count, d(gamma), d(beta), EPS)
    xhat = (z.float() - mean) * invstd
    sums = torch.cat([dyh.double().reshape(-1, 16).sum(0), (dyh * xhat).double().reshape(-1, 16).sum(0)]).contiguous()
    bn = k.BN(stats, d(gamma), d(beta), count, EPS, bstats=torch.zeros_like(sums) if frozen else sums)
    out = k.stem_bwd_dx(d(img), z, dyh, bn, d(wt), d(b))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('frozen', [False, True], ids=['train', 'frozen'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_vs_fp64(shape, frozen):
    """fp32 storage (z is read as stored; this build has no second way of obtaining it).  Bar: 5e-5."""
    case = stem_case(*shape, seed=100 + shape[1] + shape[2])
    got = run_kernel(*case, frozen, torch.float32)
    ref = reference(*case, frozen)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = rel_err(got, ref)
    print(f'stem_bwd_dx {shape} frozen={frozen}: rel err {err:.2e}')
    assert err < 5e-5, err


@pytest.mark.parametrize('frozen', [False, True], ids=['train', 'frozen'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_vs_fp64_bf16_storage(shape, frozen):
    """The bf16 build: the same check with z rounded to bf16 in the reference as well, same bar."""
    case = stem_case(*shape, seed=200 + shape[1] + shape[2])
    got = run_kernel(*case, frozen, torch.bfloat16)
    ref = reference(*case, frozen, z_round=True)
    err = rel_err(got, ref)
    print(f'stem_bwd_dx_bf16 {shape} frozen={frozen}: rel err {err:.2e}')
    assert err < 5e-5, err


# ================================================================================================== 2. tap pattern, exact
@pytest.mark.parametrize('k', [0, 7, 15])
def test_tap_pattern_exact(k):
    """Frozen BatchNorm, dy one-hot (1.0) at channel k of a 16 x 16 map's four corners, one edge and one interior pixel:
    dimg is exactly zero outside rows 2 i - 1 .. 2 i + 1, columns 2 j - 1 .. 2 j + 1 (clipped) and inside equals
    fp32(scale_k W[k, c, ky, kx]) with ky = y + 1 - 2 i, kx = x + 1 - 2 j, to 1 ulp."""
    import yunet_amd.functional as Fn
    kk = K()
    img, wt, b, gamma, beta, _, rm, rv = stem_case(1, 32, 32, seed=300 + k)
    d = lambda t: t.to(DEV).contiguous()
    count = 16 * 16
    stats = Fn._sums_from_moments(d(rm), d(rv), count)
    bn = kk.BN(stats, d(gamma), d(beta), count, EPS, bstats=torch.zeros_like(stats))
    z = torch.randn(1, 16, 16, 16, device=DEV)
    # the scale as the kernels' coefficient chain forms it: fp64 sums -> invstd rounded to fp32 -> gamma * invstd in fp32
    s = stats.cpu()
    mean = s[:16] / count
    var = (s[16:] / count - mean * mean).clamp(min=0)
    scale = gamma * (1.0 / torch.sqrt(var + float(torch.tensor(EPS, dtype=torch.float32)))).float()
    for i, j in [(0, 0), (0, 15), (15, 0), (15, 15), (0, 6), (9, 5)]:
        dy = torch.zeros(1, 16, 16, 16, device=DEV)
        dy[0, i, j, k] = 1.0
        got = kk.stem_bwd_dx(d(img), z, dy, bn, d(wt), d(b)).cpu()
        want = torch.zeros(1, 3, 32, 32)
        inside = torch.zeros(32, 32, dtype=torch.bool)
        for ky in range(3):
            for kx in range(3):
                y, x = 2 * i + ky - 1, 2 * j + kx - 1
                if 0 <= y < 32 and 0 <= x < 32:
                    want[0, :, y, x] = (scale[k].double() * wt[k, :, ky, kx].double()).float()
                    inside[y, x] = True
        assert int(inside.sum()) == (3 - (i == 0)) * (3 - (j == 0))      # (rows / columns past 31 do not exist: 2 * 15 + 1)
        assert not bool(got[0][:, ~inside].any()), (i, j, 'non-zero outside the footprint')
        ulp = torch.maximum(torch.nextafter(want.abs(), torch.tensor(float('inf'))) - want.abs(),
                            want.abs() - torch.nextafter(want.abs(), torch.tensor(0.0)))
        assert bool(((got - want).abs() <= ulp)[0][:, inside].all()), (i, j, float((got - want).abs().max()))
        assert bool((got[0][:, inside] != 0).all())


# =============================================================================================== 3. stand-alone modules
@pytest.mark.parametrize('bn_eval', [False, True], ids=['train', 'bn_eval'])
def test_standalone_stem(bn_eval):
    """functional.stem with an image that asks for a gradient (raised before this option existed): x.grad against fp64
    autograd of Conv2d + BatchNorm2d + ReLU with the same state; parameter gradients and running buffers byte-equal to the
    same call with x detached."""
    import yunet_amd.functional as Fn
    from yunet_amd.yunet_layer import Conv_head
    torch.manual_seed(41)
    m = Conv_head(3, 16, 16)
    with torch.no_grad():
        m.bn1.weight.copy_(0.5 + torch.rand(16))
        m.bn1.bias.copy_(torch.randn(16) * 0.1)
        m.bn1.running_mean.copy_(torch.randn(16))
        m.bn1.running_var.copy_(1.0 + torch.rand(16))
    state = {k: v.clone() for k, v in m.state_dict().items()}
    x0 = torch.rand(2, 3, 64, 64) * 255.0
    up = torch.randn(2, 16, 32, 32)
    # fp64 yardstick
    ref = nn.Sequential(nn.Conv2d(3, 16, 3, stride=2, padding=1), nn.BatchNorm2d(16), nn.ReLU()).double()
    ref[0].load_state_dict({'weight': state['conv1.weight'].double(), 'bias': state['conv1.bias'].double()})
    ref[1].load_state_dict({k[len('bn1.'):]: (v.double() if v.is_floating_point() else v) for k, v in state.items()
                            if k.startswith('bn1.')})
    ref.train()
    if bn_eval:
        ref[1].eval()
    x64 = x0.double().requires_grad_(True)
    (ref(x64) * up.double()).sum().backward()

    def run(with_grad):
        m.load_state_dict(state)
        m.to(DEV).train()
        if bn_eval:
            m.bn1.eval()
        for p in m.parameters():
            p.grad = None
        x = x0.to(DEV).requires_grad_(with_grad)
        y = Fn.stem(m, x)
        (y * up.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        rec = {n: bytes_of(p.grad) for n, p in m.named_parameters() if n.startswith(('conv1', 'bn1'))}
        rec.update({n: bytes_of(v) for n, v in m.state_dict().items() if n.startswith('bn1.') and ('running' in n or 'tracked' in n)})
        return x.grad, rec

    g, rec = run(True)
    none, rec0 = run(False)
    assert none is None and g is not None and g.dtype == torch.float32 and g.shape == x0.shape
    err = rel_err(g, x64.grad)
    print(f'functional.stem bn_eval={bn_eval}: x.grad rel err {err:.2e}')
    assert err < 5e-5, err
    assert rec.keys() == rec0.keys() and len(rec) == 7
    for n in rec:
        assert torch.equal(rec[n], rec0[n]), n


def test_standalone_stem_keeps_dtype_and_layout():
    import yunet_amd.functional as Fn
    from yunet_amd.yunet_layer import Conv_head
    torch.manual_seed(42)
    m = Conv_head(3, 16, 16).to(DEV).train()
    x = (torch.rand(2, 3, 32, 32, device=DEV) * 255.0).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    Fn.stem(m, x).sum().backward()
    assert x.grad.dtype == x.dtype and x.grad.is_contiguous(memory_format=torch.channels_last)
    x2 = x.detach().contiguous().requires_grad_(True)
    Fn.stem(m, x2).sum().backward()
    assert rel_err(x.grad, x2.grad) < 1e-6


# ======================================================================================================= 4 - 6. the engine
def build(kind, sd, setup=None, **backbone):
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    cfg.model.backbone.update(backbone)
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).train()
    if setup is not None:
        setup(m)
    return m


def oracle_img_grad(img, sd, arch, dflat, dtype, flag=None, bf16_z=False):
    """d sum(flat * dflat) / d img over the oracle's conv stack: helpers.fp64_conv_grads with the image as the leaf (flag:
    finetune_ref.conv_stack's per-layer training flags).  bf16_z: the bf16 oracle -- every raw conv output that feeds a
    BatchNorm (the tensors the bf16 build stores) is rounded to bf16 on its way in, with a straight-through gradient."""
    work = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    work = {k: v.clone() for k, v in work.items()}
    x = img.to(dtype).clone().requires_grad_(True)
    plain = O._bn_relu
    if bf16_z:
        O._bn_relu = lambda t, *a, **kw: plain(t + (rne_bf16(t) - t).detach(), *a, **kw)
    try:
        maps = O.conv_stack_forward(x, work, arch, True) if flag is None else FR.conv_stack(x, work, arch, flag)
    finally:
        O._bn_relu = plain
    (O.flatten_preds(*maps) * dflat.to(dtype)).sum().backward()
    return x.grad


def step(m, batch, img=None):
    """One forward_train + backward of the four losses' sum; img: the image tensor to use (a leaf that asks for a
    gradient) instead of the batch's own."""
    import yunet_amd.synthetic as S
    bd = S.to_device(batch, DEV)
    if img is not None:
        bd['img'] = img
    losses = m.forward_train(**bd)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return losses


def record(m, losses):
    rec = {'loss:' + k: bytes_of(v) for k, v in losses.items()}
    rec.update({'grad:' + n: bytes_of(p.grad) for n, p in m.named_parameters() if p.grad is not None})
    rec.update({'buf:' + k: bytes_of(v) for k, v in m.state_dict().items()
                if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))})
    return rec


def check_rule(name, got, img, sd, arch, dflat, flag=None, bf16=False):
    g64 = oracle_img_grad(img, sd, arch, dflat, torch.float64, flag)
    g32 = oracle_img_grad(img, sd, arch, dflat, torch.float32, flag, bf16_z=bf16)
    scale = float(g64.abs().max())
    err_oracle = float((g32.double() - g64).abs().max())
    err_hip = float((got.cpu().double() - g64).abs().max())
    tol = 10 * max(err_oracle, 1e-5 * scale) + 1e-2 * scale
    print(f'[{name}] img.grad: max |g64| {scale:.3e}  oracle err {err_oracle:.3e}  hip err {err_hip:.3e}  bound {tol:.3e}')
    assert scale > 0 and err_hip <= tol, (name, err_hip, err_oracle, scale)


@pytest.mark.parametrize('kind', ['n', 's'])
def test_engine_img_grad_vs_fp64(kind):
    """img.grad was None before this option existed.  The pair runs under deterministic='fast', so the step with the image
    gradient has to leave the bytes of the step without it: losses, every parameter gradient, every BatchNorm buffer."""
    import yunet_amd.synthetic as S
    arch = O.yunet_arch(kind)
    sd = O.init_state(arch, seed=31)
    b = S.make_batch(2, 64, 64, 4321)
    m = build(kind, sd)
    m.set_deterministic('fast')
    plain = record(m, step(m, b))
    assert not m.engine.plan.input_grad
    m.load_state_dict(sd, strict=True)
    img = b['img'].to(DEV).requires_grad_(True)
    losses = step(m, b, img)
    plan = m.engine.plan
    assert plan.input_grad and img.grad is not None and img.grad.shape == img.shape and img.grad.dtype == torch.float32
    with_grad = record(m, losses)
    assert plain.keys() == with_grad.keys() and len(plain) > 50
    for k in plain:
        assert torch.equal(plain[k], with_grad[k]), k
    check_rule(f'yunet_{kind}', img.grad, b['img'], sd, arch, plan.dflat.cpu())
    # the detached step afterwards runs on the plain plan again, and both stay cached
    step(m, b)
    assert not m.engine.plan.input_grad and len(m.engine.plans) == 2


def freeze_everything(m):
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.eval()
    for p in m.parameters():
        p.requires_grad = False


def test_engine_frozen_network():
    """Every BatchNorm in eval(), frozen_stages = all stages and the remaining parameters without gradient: the documented
    way to the image gradient of the inference-mode network.  The backward still runs down to the stem."""
    import yunet_amd.synthetic as S
    import yunet_amd._lib as L
    arch = O.yunet_arch('n')
    sd = FR.warm_state('n', 1)
    m = build('n', sd, freeze_everything, frozen_stages=len(arch['stage_channels']) - 1)
    b = S.make_batch(2, 64, 64, 4322)
    before = {k: bytes_of(v) for k, v in m.state_dict().items()}
    img = b['img'].to(DEV).requires_grad_(True)
    step(m, b, img)
    plan = m.engine.plan
    codes = [op.opcode for op in plan.bwd]
    assert plan.input_grad and codes.count(L.OP_STEM_BWD_DX) == 1 and L.OP_STEM_BWD not in codes and plan.reduce_jobs == []
    check_rule('frozen', img.grad, b['img'], sd, arch, plan.dflat.cpu(), flag=lambda name: False)
    assert all(p.grad is None for p in m.parameters())
    after = {k: bytes_of(v) for k, v in m.state_dict().items()}
    assert all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize('level', ['fast', True])
def test_engine_modes_deterministic_accumulate_and_hold(level):
    """Both deterministic levels: two evaluations from one state give byte-equal img.grad; a second backward after a new
    forward adds into img.grad (autograd's own accumulation: the torch sum of the two); a gradient the caller holds keeps
    its bytes while later steps run (each backward writes a fresh tensor)."""
    import yunet_amd.synthetic as S
    arch = O.yunet_arch('n')
    sd = O.init_state(arch, seed=32)
    b1, b2 = S.make_batch(2, 64, 64, 4323), S.make_batch(2, 64, 64, 4324)
    m = build('n', sd)
    m.set_deterministic(level)

    def grad_of(batch):
        m.load_state_dict(sd, strict=True)
        img = batch['img'].to(DEV).requires_grad_(True)
        step(m, batch, img)
        return img.grad

    g1 = grad_of(b1)
    held = bytes_of(g1)
    g2 = grad_of(b2)
    assert g1.data_ptr() != g2.data_ptr()
    assert torch.equal(bytes_of(g1), held), 'a later step overwrote a gradient the caller holds'
    assert torch.equal(bytes_of(grad_of(b1)), held), 'two evaluations from one state differ'
    assert not torch.equal(bytes_of(g2), held)
    # accumulation into one leaf: step on b1's targets, then on b2's, both with the same image tensor
    m.load_state_dict(sd, strict=True)
    img = b1['img'].to(DEV).requires_grad_(True)
    step(m, b1, img)
    first = img.grad.clone()
    m.load_state_dict(sd, strict=True)
    step(m, b2, img)
    m.load_state_dict(sd, strict=True)
    alone = b1['img'].to(DEV).requires_grad_(True)
    step(m, b2, alone)
    assert torch.equal(bytes_of(first), held)
    assert torch.equal(bytes_of(img.grad), bytes_of(first + alone.grad))


def test_engine_bf16_storage():
    import yunet_amd.synthetic as S
    arch = O.yunet_arch('n')
    sd = O.init_state(arch, seed=33)
    b = S.make_batch(2, 64, 64, 4325)
    m = build('n', sd)
    m.set_precision('bf16')
    img = b['img'].to(DEV).requires_grad_(True)
    step(m, b, img)
    plan = m.engine.plan
    assert plan.input_grad and plan.act_dtype == torch.bfloat16
    check_rule('bf16', img.grad, b['img'], sd, arch, plan.dflat.cpu(), bf16=True)


def test_engine_multiscale_canvas():
    """A square_range batch as the device pipeline collates it: image n in the top-left S_n x S_n corner of the
    [N, 3, Smax, Smax] canvas, zero to the right and below (S = 64 and 32).  The gradient is checked on the whole canvas."""
    import yunet_amd.synthetic as S
    arch = O.yunet_arch('n')
    sd = O.init_state(arch, seed=34)
    big, small = S.make_batch(1, 64, 64, 4326), S.make_batch(1, 32, 32, 4327)
    canvas = torch.zeros(2, 3, 64, 64)
    canvas[0] = big['img'][0]
    canvas[1, :, :32, :32] = small['img'][0]
    b = S.attach_padding(dict(img=canvas, img_metas=big['img_metas'] + small['img_metas'],
                              gt_bboxes=list(big['gt_bboxes']) + list(small['gt_bboxes']),
                              gt_labels=list(big['gt_labels']) + list(small['gt_labels']),
                              gt_keypointss=list(big['gt_keypointss']) + list(small['gt_keypointss'])))
    m = build('n', sd)
    img = canvas.to(DEV).requires_grad_(True)
    step(m, b, img)
    assert bool(img.grad[1, :, 32:, :].any()) or bool(img.grad[1, :, :, 32:].any())      # the border has a gradient too
    check_rule('canvas', img.grad, canvas, sd, arch, m.engine.plan.dflat.cpu())


def test_engine_eval_and_no_grad_are_unchanged():
    """model.eval() keeps returning graph-free validation losses whatever the image asks for; under no_grad a training
    step stays on the plain plan."""
    import yunet_amd.synthetic as S
    arch = O.yunet_arch('n')
    sd = O.init_state(arch, seed=35)
    b = S.make_batch(2, 64, 64, 4328)
    m = build('n', sd)
    bd = S.to_device(b, DEV)
    bd['img'] = bd['img'].requires_grad_(True)
    with torch.no_grad():
        m.forward_train(**bd)
    assert not m.engine.plan.input_grad
    m.eval()
    losses = m.forward_train(**bd)
    assert all(not v.requires_grad for v in losses.values()) and not m.engine.plan.input_grad and bd['img'].grad is None


# ================================================================================================ 7. entry-point refusals
@pytest.mark.parametrize('suffix', ['', '_bf16'])
def test_entry_point_refusals(suffix):
    """Odd H, C = 8 and a null dy: YUNET_EINVAL, and the output buffer keeps its bytes."""
    import yunet_amd._lib as L
    k = K()
    lib = L.load()
    fn = getattr(lib, 'yunet_stem_bwd_dx' + suffix)
    n, h, w = 1, 32, 32
    z = torch.randn(n, h // 2, w // 2, 16, device=DEV).to(torch.bfloat16 if suffix else torch.float32)
    dy = torch.randn(n, h // 2, w // 2, 16, device=DEV)
    wt = torch.randn(16, 3, 3, 3, device=DEV)
    stats = torch.cat([torch.zeros(16), torch.ones(16)]).double().to(DEV) * (n * h * w // 4)
    bn = k.BN(stats, torch.ones(16, device=DEV), torch.zeros(16, device=DEV), n * h * w // 4, EPS, bstats=torch.zeros_like(stats))
    out = torch.full((n, 3, h, w), 7.25, device=DEV)
    want = bytes_of(out)
    p = lambda t: C.c_void_p(t.data_ptr())
    bnc = bn.c()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert fn(p(z), p(dy), C.byref(bnc), p(wt), p(out), n, h - 1, w, 16, stream) == L.EINVAL
    assert fn(p(z), p(dy), C.byref(bnc), p(wt), p(out), n, h, w, 8, stream) == L.EINVAL
    assert fn(p(z), None, C.byref(bnc), p(wt), p(out), n, h, w, 16, stream) == L.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(bytes_of(out), want)
    assert fn(p(z), p(dy), C.byref(bnc), p(wt), p(out), n, h, w, 16, stream) == 0          # and the accepted call writes all of it
    torch.cuda.synchronize()
    assert not bool((out == 7.25).any())
