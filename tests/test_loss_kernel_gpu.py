"""-m gpu: the fused loss step (loss_kernel, loss_norm_kernel, loss_finalize_kernel of csrc/loss_step.hip) per element
against the fp64 reference of tests/loss_ref.py, on regime batches that reach both sides of every branch the kernel
takes.  Each case prints its branch census and the worst error / bar ratio, and asserts the census it relies on.

Not forced: CIoU's clamp(-1, 1).  With alpha = 0 (IoU <= 0.5) rho^2 / c^2 < 1 keeps cious above -1, and alpha > 0 needs
IoU > 0.5, which keeps it there too in practice."""
import ctypes as C

import pytest
import torch

import crafted as Cr
import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ALL_BOXES = ('generic', 'tie', 'touch', 'disjoint', 'nested')


def _dev(case):
    return {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in case.items()}


def run_loss(case, cfg, blocks=None, norm=None, defer=False, num_total=None):
    """yunet_loss + yunet_loss_finalize_ex through the C ABI -> (losses [5], dflat, partials, dy_norm) on the host."""
    import yunet_amd._lib as L
    import yunet_amd.kernels as k
    d = _dev(case)
    N, P, _ = d['flat'].shape
    Gmax = d['gt_boxes'].shape[1]
    lib = L.load()
    if norm is None:
        norm = k.loss_norm(d['img_stats'])
    blocks = blocks or int(lib.yunet_loss_blocks(N, P))
    part = torch.empty(blocks, 4, device=DEV)
    dflat = torch.full_like(d['flat'], float('nan'))
    losses = torch.empty(5, device=DEV)
    lv = k.make_levels(d['sizes'], d['strides'])
    kc = R.kernel_cfg(cfg, defer)
    L.check(lib.yunet_loss(k._p(d['flat']), k._p(d['gt_inds']), k._p(d['max_overlaps']), k._p(d['gt_boxes']),
                           k._p(d['gt_kps']), C.byref(lv), C.byref(kc), k._p(norm), N, P, Gmax, k._p(dflat),
                           k._p(part), blocks, k._stream()), 'yunet_loss')
    nt = dyn = None
    if defer:
        nt = torch.tensor([float(num_total)], device=DEV)
        dyn = torch.full((16,), float('nan'), device=DEV)
    L.check(lib.yunet_loss_finalize_ex(k._p(part), blocks, k._p(losses), None, k._p(nt), k._p(dyn), k._stream()),
            'yunet_loss_finalize_ex')
    torch.cuda.synchronize()
    return losses.cpu(), dflat.cpu(), part.cpu(), None if dyn is None else dyn.cpu()


# the loss bars: the terms' own bars summed plus the reduction.  Their relative size is set by how a 1-ulp move of the
# fp32 inputs moves the losses (box coordinates of a few hundred pixels against boxes of a few pixels), ~2-4e-5 on these
# batches -- the old global bar was 1e-4
MAX_LOSS_BAR = 5e-5


def grade(name, case, cfg, got_losses, got_dflat, need=None, max_loss_bar=MAX_LOSS_BAR, **kw):
    c = R.census(case, cfg)
    rep = R.check(got_losses[:4], got_dflat, case, cfg, **kw)
    print(f'\n[{name}] census {c}\n[{name}] {rep}')
    for key, lo in (need or {}).items():
        assert c[key] >= lo, f'census: {key} = {c[key]} < {lo}'
    assert rep.ok, rep
    # the escape routes stay small: elements graded against either branch (ambiguous) or against the fp32 restatement
    # too (a tie / clamp decision that differs between fp32 and fp64)
    assert rep.n_amb + rep.n_unres <= 0.01 * rep.n_pos + 5, rep
    assert rep.loss_rel_bar <= max_loss_bar, rep
    return c, rep


def regime_need(box_loss, vis='fractional'):
    need = dict(pos=200, overlap_pos=50, overlap_zero=10, overlap_neg=10, edge_tie=10, sl1_quad=50, sl1_lin=50,
                sl1_zero=50, level_0=10, level_1=10, level_2=3)
    if box_loss == 'EIoULoss':
        need.update(eiou_quad=10, eiou_lin=10)
    if box_loss == 'CIoULoss':
        need.update(ciou_alpha_on=10, ciou_alpha_off=10)
    if box_loss == 'IoULoss':
        need.update(iou_eps_clamp=5)
    if vis == 'fractional':
        need.update({f'vis_{v / 5:.1f}': 5 for v in range(6)})
    return need


@pytest.mark.parametrize('box,mode', R.BOX_LOSSES)
def test_box_losses_per_element(box, mode):
    case = R.make_case(4, 320, 320, 11, boxes=ALL_BOXES)
    cfg = R.make_cfg(box, mode, box_eps=1e-16 if mode == 'square' else 1e-6)
    losses, dflat, _, _ = run_loss(case, cfg)
    c, _ = grade(f'{box}/{mode}', case, cfg, losses, dflat, regime_need(box))
    assert c['iou_max'] >= 0.999


def test_eiou_converging_model():
    """EIoU's quadratic branch: IoU 0.9 .. 0.9999 on most positives (a converging model)."""
    case = R.make_case(4, 320, 320, 12, boxes=('generic',))
    cfg = R.make_cfg('EIoULoss')
    losses, dflat, _, _ = run_loss(case, cfg)
    # at IoU 0.9999 the quadratic branch's 0.5 x^2 / sp, x = 1 - IoU ~ 1e-4, moves by ~1e-2 of itself under a 1-ulp
    # move of a box coordinate: the box loss's own bar follows that conditioning
    grade('eiou converging', case, cfg, losses, dflat, dict(eiou_quad=500, eiou_lin=50), max_loss_bar=1e-3)


def test_all_invisible_landmarks_give_exact_zero():
    case = R.make_case(3, 160, 160, 13, boxes=ALL_BOXES, vis='invisible')
    cfg = R.make_cfg('EIoULoss')
    losses, dflat, _, _ = run_loss(case, cfg)
    grade('invisible', case, cfg, losses, dflat, {'pos': 50, 'vis_0.0': 50})
    assert float(losses[3]) == 0.0
    assert bool((dflat[..., 6:] == 0).all())


@pytest.mark.parametrize('h,w,n', [(480, 320, 3), (100, 100, 5), (320, 480, 2)])
def test_rectangular_and_odd_inputs(h, w, n):
    """Positives on the first and last prior of every level (make_case(edges=True))."""
    case = R.make_case(n, h, w, 14 + h + w, boxes=ALL_BOXES)
    cfg = R.make_cfg('EIoULoss')
    losses, dflat, _, _ = run_loss(case, cfg)
    grade(f'{h}x{w}', case, cfg, losses, dflat, dict(level_0=2 * n, level_1=2 * n, level_2=2 * n))
    # negatives: every channel but obj is exactly 0
    neg = case['gt_inds'] == 0
    assert bool((dflat[neg][:, [0, 1, 2, 3, 4] + list(range(6, 16))] == 0).all())


@pytest.mark.parametrize('n,size', [(256, 320), (64, 640)])
def test_bench_geometry_walks_the_grid_stride_loop(n, size):
    case = R.make_case(n, size, size, 15 + n, boxes=ALL_BOXES, frac=0.02, edges=False)
    N, P, _ = case['flat'].shape
    assert N * P > R.MAX_LOSS_BLOCKS * R.LOSS_THREADS, 'the batch does not walk the grid-stride loop'
    cfg = R.make_cfg('EIoULoss')
    losses, dflat, _, _ = run_loss(case, cfg)
    grade(f'bench {n}x{size}', case, cfg, losses, dflat, dict(pos=500), draws=2)


def test_block_counts_agree_and_repeat_bitwise():
    """Direct launches with 1 .. 2048 blocks: the grid-stride walk and the finalize reduction's unrolled-by-8 loop and
    its tail; the same block count twice gives the same bits."""
    case = R.make_case(8, 320, 320, 16, boxes=ALL_BOXES, frac=0.05)
    cfg = R.make_cfg('EIoULoss')
    ref = R.ref_of(case, cfg)
    first = None
    for blocks in (1, 3, 64, 449, 2048):
        l1, d1, p1, _ = run_loss(case, cfg, blocks=blocks)
        l2, d2, p2, _ = run_loss(case, cfg, blocks=blocks)
        assert torch.equal(l1, l2) and torch.equal(d1, d2) and torch.equal(p1, p2), blocks
        grade(f'blocks={blocks}', case, cfg, l1, d1, blocks=blocks, ref=ref, draws=2)
        if first is None:
            first = d1
        assert torch.equal(d1, first), 'dflat depends on the block count'


@pytest.mark.parametrize('num_total', [0.0, 0.25, 37.25])
def test_deferred_normaliser(num_total):
    """defer_num_total = 1 (engine.py's training path) + finalize_ex: the head backward's dy_norm times the deferred
    gradient rounds like the undeferred gradient, bit for bit."""
    import yunet_amd.kernels as k
    case = R.make_case(4, 320, 320, 17, boxes=ALL_BOXES)
    cfg = R.make_cfg('EIoULoss')
    norm = k.loss_norm(case['img_stats'].to(DEV))
    norm[0] = num_total
    l0, d0, _, _ = run_loss(case, cfg, norm=norm)
    l1, d1, _, dyn = run_loss(case, cfg, norm=norm, defer=True, num_total=num_total)
    inv = torch.tensor(1.0) / torch.tensor(max(num_total, 1.0))
    assert torch.equal(dyn[:6], inv.expand(6)) and torch.equal(dyn[6:], torch.ones(10))
    assert torch.equal(d1[..., :6] * dyn[:6], d0[..., :6])
    assert torch.equal(d1[..., 6:], d0[..., 6:])
    assert torch.equal(l1[3], l0[3])
    grade(f'deferred {num_total}', case, cfg, l1, d1[..., :] * dyn, num_total=num_total)
    grade(f'undeferred {num_total}', case, cfg, l0, d0, num_total=num_total, draws=2)


@pytest.mark.parametrize('n', [1, 255, 257, 600])
def test_loss_norm_against_fp64(n):
    import yunet_amd.kernels as k
    g = torch.Generator().manual_seed(n)
    st = torch.stack([torch.randint(0, 200, (n,), generator=g).float(),
                      (torch.randint(0, 1000, (n,), generator=g).double() / 5.0 + torch.rand(n, generator=g,
                                                                                             dtype=torch.float64)).float()], 1)
    for inv_world in (1.0, 0.25):
        norm = k.loss_norm(st.to(DEV), inv_world).cpu()
        cnt = float(st[:, 0].double().sum())
        assert float(norm[2]) == cnt and float(norm[0]) == cnt * inv_world       # integer counts: exact
        w64 = float(st[:, 1].double().sum())
        bar = (-(-n // 256) + 9) * R.U32 * float(st[:, 1].double().abs().sum())
        assert abs(float(norm[1]) - w64) <= bar, (float(norm[1]), w64, bar)


def test_assign_then_loss_end_to_end():
    """k.assign -> k.loss on GTs with fractional visibility: the assignment's weight sum against fp64, the losses and
    dflat against loss_ref on the kernel's own assignment."""
    import yunet_amd.kernels as k
    import yunet_amd.synthetic as S
    h = w = 320
    b = S.make_batch(8, h, w, 18, with_img=False)
    g = torch.Generator().manual_seed(18)
    gkl = []
    for kp in b['gt_keypointss']:
        kp = kp.clone()
        nv = torch.randint(0, 6, (kp.shape[0],), generator=g)
        kp[:, :, 2] = (torch.argsort(torch.rand(kp.shape[0], 5, generator=g), 1) < nv[:, None]).float()
        gkl.append(kp)
    flat = Cr.crafted_preds(b['gt_bboxes'], gkl, h, w, 19)
    gb, gk, cnt = Cr.pad_gt(b['gt_bboxes'], gkl)
    sizes = Cr.featmap_sizes(h, w)
    gi, ovl, st, _ = k.assign(flat.to(DEV), gb.to(DEV), gk.to(DEV), cnt.to(DEV).int(), sizes, [8, 16, 32])
    torch.cuda.synchronize()
    gi, ovl, st = gi.cpu(), ovl.cpu(), st.cpu()
    case = dict(flat=flat, gt_inds=gi, max_overlaps=ovl, gt_boxes=gb, gt_kps=gk, img_stats=st, sizes=sizes,
                strides=[8, 16, 32])
    for n in range(8):
        pos = gi[n] > 0
        w64 = float(gk[n][(gi[n][pos] - 1).long()][:, :, 2].double().mean(1).sum())
        assert int(st[n, 0]) == int(pos.sum())
        assert abs(float(st[n, 1]) - w64) <= 64 * R.U32 * max(w64, 1.0), (n, float(st[n, 1]), w64)
    cfg = R.make_cfg('EIoULoss')
    losses, dflat, _, _ = run_loss(case, cfg)
    grade('assign->loss', case, cfg, losses, dflat, {f'vis_{v / 5:.1f}': 1 for v in range(6)})
