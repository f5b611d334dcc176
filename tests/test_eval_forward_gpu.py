"""-m gpu: the eval-mode forward (Plan.fwd_eval) per layer against the fp64 reference of tests/eval_ref.py, at the
geometries tools/test_widerface.py runs, in both builds.

One forward_eval leaves every intermediate tensor readable: Plan allocates one buffer per tensor and fwd_eval writes
each exactly once (no buffer is reused or overwritten later in the list), so after the call Plan.tensors (unit name ->
(input, output)), the fused-pool winners and positions, the pool / TFPN-merge outputs (named by the ops' pointers) and
plan.flat are the stored values every layer read or wrote.  Each layer's reference starts from the kernel's own stored
input (teacher forcing), so a failure names the layer.  flat is also compared end to end with the full fp64 network,
per output channel."""
import os

import pytest
import torch
import torch.nn.functional as F

import detect_oracle as D
import eval_ref as E
import yunet_oracle as O
from test_bf16_kernels_gpu import canvas_tiles, cus, fwd64s_tasks, pack_on

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PRECISIONS = ('fp32', 'bf16')
# end-to-end bars, per element, relative to the output channel's largest |value| over the batch: fp32 -- ten times
# tighter than the old global bar (2e-4 max|ref| over all channels); bf16 -- one bf16 ulp (2^-8 relative) for each of
# the <= 16 stored activations between the image and a head output
FLAT_TOL = {'fp32': 2e-5, 'bf16': 16 * 2.0 ** -8}


# ------------------------------------------------------------------------------------------------ inputs and models
def padded_images(n, h, w, seed):
    """smooth structured content (D.structured_images' two octaves) in the top-left, and a zero band on the right and
    at the bottom: an original-size image padded to a multiple of 32 (tools/test_widerface.py --mode 2)"""
    g = torch.Generator().manual_seed(500 + seed)
    hi, wi = h - max(8, (h // 10) // 2 * 2), w - max(8, (w // 7) // 2 * 2)
    lo, mid = torch.rand(n, 3, 10, 10, generator=g), torch.rand(n, 3, 40, 40, generator=g)
    body = F.interpolate(lo, size=(hi, wi), mode='bilinear', align_corners=False) * 0.7 + \
        F.interpolate(mid, size=(hi, wi), mode='bilinear', align_corners=False) * 0.3
    img = torch.zeros(n, 3, h, w)
    img[:, :, :hi, :wi] = body * 255
    return img.contiguous()


def _load(kind):
    return torch.load(os.path.join(GOLDEN, f'yunet_{kind}_synth_trained.pth'), map_location='cpu',
                      weights_only=False)['state_dict']


def adversarial(sd):
    """running statistics where the eval path can go wrong: var 1e-8 under |mean| 50 (mode 2's cancellation),
    var 1e4, and gamma < 0 / gamma = 0 (the fused-pool winner rule) -- in some channels of every BatchNorm"""
    sd = {k: v.clone() for k, v in sd.items()}
    for k in [k for k in sd if k.endswith('.running_mean')]:
        p = k[:-len('.running_mean')]
        rm, rv, gam = sd[k], sd[p + '.running_var'], sd[p + '.weight']
        rm[0], rv[0] = 50.0, 1e-8
        rm[1], rv[1] = -50.0, 1e-8
        gam[1] = gam[1].abs() * 1e-3            # (z + 50) x 316 (invstd at var 1e-8): scaled down, still large
        rv[2] = 1e4
        gam[3], gam[4] = -gam[3].abs(), 0.0
    return sd


_STATES = {}


def state(name):
    """state dicts, each built once per module: the trained fixtures, a second state (detect_oracle.make_state), and
    the adversarial running statistics on the trained YuNet_n"""
    if name not in _STATES:
        if name in ('n', 's'):
            _STATES[name] = ('n' if name == 'n' else 's', _load(name))
        elif name == 'n2':
            _STATES[name] = ('n', D.make_state('n', 11, 160, calib_iters=10)[1])
        else:
            _STATES[name] = ('n', adversarial(_load('n')))
    return _STATES[name]


def build(kind, sd, precision):
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(f'configs/yunet_{kind}.py')
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).eval()
    m.set_precision(precision)
    return m


_FLAT_REF = {}


def flat_ref(sname, img):
    """the full fp64 network (BatchNorm on the running statistics), once per state and input"""
    key = (sname, tuple(img.shape), float(img.sum()))
    if key not in _FLAT_REF:
        kind, sd = state(sname)
        sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
        _FLAT_REF[key] = D.eval_flat(img.double(), sd64, O.yunet_arch(kind))[0]
    return _FLAT_REF[key]


# ------------------------------------------------------------------------------------------------ per-layer walk
def check_layers(plan, img, sd, prec, tag):
    """every op of one forward_eval against its fp64 reference (teacher-forced) -> {layer: worst error / bound}"""
    import yunet_amd._lib as L
    stored, bf16 = ('bf16', True) if prec == 'bf16' else ('fp32', False)
    T = plan.tensors
    by_ptr = {}
    for x, z in T.values():
        by_ptr[x.buf.data_ptr()], by_ptr[z.buf.data_ptr()] = x, z
    name_of = {id(z): nm for nm, (_, z) in T.items()}
    made = {}             # buffer -> the op that wrote it, for tensors no unit wrote
    for op in plan.fwd_eval:
        if op.opcode == L.OP_POOL_FWD:
            made[op.p[1]] = ('pool', by_ptr[op.p[0]])
        elif op.opcode == L.OP_UPADD_FWD:
            made[op.p[2]] = ('upadd', by_ptr[op.p[0]], by_ptr[op.p[1]])
    for x, z in T.values():
        if z.pooled_into is not None:
            made[z.pooled_into[0].buf.data_ptr()] = ('fused', z, z.pooled_into[1])
    assert not any(op.opcode == L.OP_DP_FWD and op.dp.out_has_bn for op in plan.fwd_eval), 'eval accumulates sums'
    worst = {}

    def rec(name, w):
        worst[name] = max(worst.get(name, 0.0), w)

    def bn(name):
        return E.running_bn(sd, name)

    x0 = T['backbone.model0.conv2'][0]
    rec('stem', E.check(f'stem {tag}', x0.buf.cpu(), E.stem_ref(img, sd['backbone.model0.conv1.weight'],
                                                                  sd['backbone.model0.conv1.bias']), stored))
    for nm, (x, z) in T.items():
        src = made.get(x.buf.data_ptr())
        if src is not None and src[0] == 'pool':
            rec(f'pool {name_of[id(src[1])]}', E.check(f'pool {name_of[id(src[1])]} {tag}', x.buf.cpu(),
                                                       E.plain_pool_ref(src[1].buf.cpu(), bn(src[1].bn)), stored))
        elif src is not None and src[0] == 'upadd':
            a, b = src[1], src[2]
            rec(f'upadd -> {nm}', E.check(f'upadd -> {nm} {tag}', x.buf.cpu(),
                                          E.upadd_ref(a.buf.cpu(), b.buf.cpu(), bn(a.bn), bn(b.bn)), stored))
        elif src is not None:
            E.pool_rule(src[1].buf.cpu(), x.buf.cpu(), src[2].cpu(), sd[src[1].bn + '.weight'],
                        f'fused pool {name_of[id(src[1])]} {tag}')
            rec(f'fused pool {name_of[id(src[1])]}', 0.0)
        r = E.unit_ref(x.buf.cpu(), *E.unit_weights(sd, nm), in_bn=bn(x.bn) if x.bn else None,
                       bf16_gemm=bf16 and x.c % 32 == 0)
        rec(nm, E.check(f'{nm} {tag}', z.buf.cpu(), r, stored))
    flat = plan.flat.cpu()
    bases = [sum(a * b for a, b in plan.sizes[:lvl]) for lvl in range(len(plan.sizes))]
    f0, f1 = plan.flat.data_ptr(), plan.flat.data_ptr() + 4 * plan.flat.numel()
    heads = {(op.dp.z - f0) // 64: by_ptr[op.dp.x] for op in plan.fwd_eval
             if op.opcode == L.OP_DP_FWD and f0 <= op.dp.z < f1}
    assert sorted(heads) == bases, (sorted(heads), bases)
    for lvl in range(len(plan.sizes)):
        x = heads[bases[lvl]]          # the head unit's input: the level's last share conv (or lateral conv) output
        r = E.heads_ref(x.buf.cpu(), sd, lvl, bn(x.bn), bf16_gemm=bf16)
        rec(f'head.{lvl}', E.check(f'head.{lvl} {tag}', E.flat_level(flat, plan.sizes, lvl), r, 'fp32'))
    return worst


def report(tag, worst):
    print(f'[eval {tag}] worst error / bound per layer:')
    for k, v in worst.items():
        print(f'    {k:48s} {v:.3g}')


def assert_geometry(plan, n, h, w, prec):
    """the geometry a case claims: level sizes and P, the packed canvas at 20 x 20 / 10 x 10 for batch >= 4, the
    dp_fwd64s task count of the 64 -> 64 units per level"""
    sizes = [(h // s, w // s) for s in (8, 16, 32)]
    assert plan.sizes == sizes and plan.P == sum(a * b for a, b in sizes), (plan.sizes, sizes)
    assert plan.flat.shape == (n, plan.P, 16)
    for (a, b) in sizes:
        packed = pack_on(n, a, b)
        tasks = fwd64s_tasks(n, a, b, cus() * 4)
        info = f'canvas tiles {canvas_tiles(n, a, b, 8, 16)}' if packed else f'fwd64s tasks {tasks} on {cus() * 4} waves'
        print(f'[geometry {n}x{h}x{w} {prec}] level {a}x{b}: {"packed" if packed else "per image"}, {info}')
    return sizes


def eval_case(sname, n, h, w, prec, seed, img=None, check_flat=True):
    kind, sd0 = state(sname)
    m = build(kind, sd0, prec)
    eng = m._ensure_engine(torch.device(DEV))
    img = padded_images(n, h, w, seed) if img is None else img
    rm0, rv0 = eng.params.running_mean.clone(), eng.params.running_var.clone()
    flat = eng.forward_eval(img.to(DEV).contiguous())
    torch.cuda.synchronize()
    plan = eng.plan
    assert_geometry(plan, n, h, w, prec)
    assert torch.equal(rm0, eng.params.running_mean) and torch.equal(rv0, eng.params.running_var)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    tag = f'{sname} {n}x{h}x{w} {prec}'
    worst = check_layers(plan, img, sd, prec, tag)
    if check_flat:
        worst['flat vs fp64 network'] = E.check_flat(f'flat {tag}', flat.cpu(), flat_ref(sname, img), FLAT_TOL[prec])
    report(tag, worst)
    return m, flat.cpu(), img


# ------------------------------------------------------------------------------------------------ cases
CASES = [('n', 1, 640, 640), ('n', 1, 1120, 1664), ('n', 1, 704, 1024), ('n', 1, 1376, 1024), ('n', 1, 160, 1024),
         ('n', 4, 320, 320), ('s', 1, 640, 640), ('s', 1, 704, 1024), ('n2', 1, 704, 1024), ('adv', 1, 704, 1024),
         ('adv', 4, 320, 320)]


@pytest.mark.parametrize('prec', PRECISIONS)
@pytest.mark.parametrize('sname,n,h,w', CASES)
def test_eval_forward_per_layer(sname, n, h, w, prec):
    """each layer of forward_eval within its per-element fp64 bar; flat within the end-to-end bar per channel (the
    adversarial state is checked per layer only: its var = 1e-8 channels amplify by 3e2 by construction)"""
    if (h, w) == (1120, 1664):
        assert (h // 32, w // 32) == (35, 52)                       # odd stride-32 rows
    if (h, w) == (1376, 1024):
        assert (h // 32) % 2 == 1 and (h // 16) % 2 == 0
    if n == 4:
        assert pack_on(4, 20, 20) and pack_on(4, 10, 10)            # the packed canvas at both small levels
    eval_case(sname, n, h, w, prec, seed=h + w + n, check_flat=sname != 'adv')


@pytest.mark.parametrize('prec', PRECISIONS)
def test_eval_after_train_step(prec):
    """one training step (train_step + backward: the engine's forward, backward and mode-0 update), then forward_eval
    at the same (N, H, W): both on one plan and one stats block; op 0 must re-read the updated running statistics and
    leave no training sums in any replica; eval leaves the running statistics unchanged"""
    import yunet_amd.synthetic as S
    kind, sd0 = state('n2')
    m = build(kind, sd0, prec)
    m.train()
    rm0 = m._ensure_engine(torch.device(DEV)).params.running_mean.clone()
    b = S.make_batch(4, 320, 320, 77, max_gt=64, structured=True)
    assert max(len(g) for g in b['gt_bboxes']) <= 64
    out = m.train_step(S.to_device(b, DEV), None)
    out['loss'].backward()
    torch.cuda.synchronize()
    eng = m.engine
    plan_train = eng.plan
    rm1 = eng.params.running_mean.clone()
    assert not torch.equal(rm1, rm0), 'the training step did not update the running statistics'
    m.eval()
    img = b['img'].contiguous()
    flat = eng.forward_eval(img.to(DEV))
    torch.cuda.synchronize()
    assert eng.plan is plan_train, 'train and eval at one (N, H, W) must share the plan'
    assert torch.equal(rm1, eng.params.running_mean), 'eval changed running_mean'
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}       # the statistics after the step
    tag = f'train->eval 4x320x320 {prec}'
    worst = check_layers(eng.plan, img, sd, prec, tag)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    ref = D.eval_flat(img.double(), sd64, O.yunet_arch(kind))[0]
    worst['flat vs fp64 network'] = E.check_flat(f'flat {tag}', flat.cpu(), ref, FLAT_TOL[prec])
    report(tag, worst)


@pytest.mark.parametrize('prec', PRECISIONS)
def test_eval_batch_independence(prec):
    """an image's eval output at batch 4 (packed canvas) and alone at batch 1 (per-image tiles) meet one fp64 bar"""
    img = padded_images(4, 320, 320, 5)
    _, flat4, _ = eval_case('n', 4, 320, 320, prec, seed=5, img=img)
    _, flat1, _ = eval_case('n', 1, 320, 320, prec, seed=5, img=img[1:2].contiguous())
    ref1 = flat_ref('n', img[1:2].contiguous())
    E.check_flat(f'image 1 at batch 4 {prec}', flat4[1:2], ref1, FLAT_TOL[prec])
    E.check_flat(f'image 1 at batch 1 {prec}', flat1, ref1, FLAT_TOL[prec])


def test_eval_plan_eviction():
    """mode 2 walks hundreds of shapes and get_plan keeps MAX_PLANS: after MAX_PLANS more shapes the first one's
    plan is evicted and rebuilt, and its output meets the same bars"""
    import yunet_amd.engine as EN
    kind, sd0 = state('n')
    m = build(kind, sd0, 'fp32')
    eng = m._ensure_engine(torch.device(DEV))
    shapes = [(96, 96 + 32 * k) for k in range(EN.MAX_PLANS + 1)]
    imgs = {s: padded_images(1, *s, seed=s[1]) for s in shapes}
    first = eng.forward_eval(imgs[shapes[0]].to(DEV)).cpu().clone()
    plan0 = eng.plan
    for s in shapes[1:]:
        eng.forward_eval(imgs[s].to(DEV))
    torch.cuda.synchronize()
    assert len(eng.plans) == EN.MAX_PLANS and all(p is not plan0 for p in eng.plans.values()), 'first plan not evicted'
    del plan0
    again = eng.forward_eval(imgs[shapes[0]].to(DEV))
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    worst = check_layers(eng.plan, imgs[shapes[0]], sd, 'fp32', 'rebuilt 1x96x96 fp32')
    worst['flat'] = E.check_flat('rebuilt flat', again.cpu(), flat_ref('n', imgs[shapes[0]]), FLAT_TOL['fp32'])
    E.check_flat('first flat', first, flat_ref('n', imgs[shapes[0]]), FLAT_TOL['fp32'])
    report('rebuilt plan 1x96x96 fp32', worst)
