"""-m gpu: ignore regions through every layer -- yunet_aug_ignore against the fixture the unmodified
reference made (tests/golden/ignore_cases.npz), yunet_ignore_mark against the fp64 rule of tests/ignore_ref.py, the
flagged instances of the loss kernel per element at the bars of tests/test_loss_kernel_gpu.py, the engine against the
oracle's step with the objectness mask applied here, and RetinaFaceSource end to end."""
import os

import numpy as np
import pytest
import torch

import helpers as Hh
import ignore_ref as G
import loss_ref as R
import loss_terms_ref as LT
import yunet_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LOSS_BAR = 5e-5                 # tests/test_loss_kernel_gpu.py
ALL_BOXES = ('generic', 'tie', 'touch', 'disjoint', 'nested')
PIPELINE = [
    dict(type='LoadImageFromFile', to_float32=True),
    dict(type='LoadAnnotations', with_bbox=True, with_keypoints=True),
    dict(type='RandomSquareCrop', crop_choice=G.CROP_CHOICE),
    dict(type='Resize', img_scale=(64, 64), keep_ratio=False),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='Normalize', mean=[0., 0., 0.], std=[1., 1., 1.], to_rgb=False),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_bboxes_ignore', 'gt_keypointss']),
]


def _dev(case):
    return {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in case.items()}


# ------------------------------------------------------------------------------------------------------ pipeline
def pipeline_of(size):
    p = [dict(t) for t in PIPELINE]
    if not isinstance(size, int):
        p[3] = dict(type='Resize', img_scale=tuple(size), multiscale_mode='square_range', keep_ratio=False)
    return p


_pipe_runs = {}


def run_pipe(name, rows):
    """The set `name` through the device pipeline with `rows` padded ignore rows (None: the option off), once."""
    if (name, rows) not in _pipe_runs:
        from yunet_amd.pipelines import DevicePipeline, SourceBatch
        iteration, items, outs = G.load_set(name)
        seed, _, size = G.SETS[name]
        pipe = DevicePipeline(pipeline_of(size), seed=seed, gmax=64, ignore_rows=rows)
        ign = [it['ign'] for it in items] if rows is not None else None
        sb = SourceBatch.from_lists([it['img'] for it in items], [it['boxes'] for it in items], [it['kps'] for it in items],
                                    DEV, gt_bboxes_ignore=ign)
        out = pipe(sb, iteration)
        torch.cuda.synchronize()
        assert pipe.check() == []
        _pipe_runs[(name, rows)] = (pipe, out, items, outs)
    return _pipe_runs[(name, rows)]


@pytest.mark.parametrize('name', list(G.SETS))
def test_aug_ignore_is_bit_equal_to_the_reference_fixture(name):
    pipe, out, items, outs = run_pipe(name, G.ROWS)
    params = pipe.params.cpu().numpy()
    for i, it in enumerate(items):
        S = it['S'] if name != 's64' else 0
        assert params[i, [0, 1, 2, 3, 7]].tolist() == [it['left'], it['top'], it['cw'], int(it['flip']), S], i
    ign = out['gt_bboxes_ignore']
    assert tuple(ign.padded.shape) == (4, G.ROWS, 4) and ign.padded.dtype == torch.float32 and ign.counts.dtype == torch.int32
    ob, oc = G.padded(outs)
    assert np.array_equal(ign.counts.cpu().numpy(), oc)
    assert np.array_equal(ign.padded.cpu().numpy(), ob)
    assert len(ign) == 4 and ign[0].data_ptr() == ign.padded.data_ptr()
    # 17 kept boxes into 16 rows: the first 16, in order; into 32 rows: all of them
    assert len(outs[2]) == 17 and int(oc[2]) == 16 and np.array_equal(ob[2], outs[2][:16])
    _, wide, _, _ = run_pipe(name, 32)
    w = wide['gt_bboxes_ignore']
    assert w.counts.cpu().tolist() == [len(o) for o in outs]
    assert np.array_equal(w.padded.cpu().numpy()[2, :17], outs[2]) and not w.padded.cpu().numpy()[2, 17:].any()
    # the GT rows are the reference's too: the shared helper did not move them
    z = np.load(G.GOLD)
    for i in range(4):
        g = z[f'{name}/gt_{i}']
        assert int(out['gt_bboxes'].counts[i]) == len(g)
        assert np.array_equal(out['gt_bboxes'].padded[i, :len(g)].cpu().numpy(), g)


@pytest.mark.parametrize('name', list(G.SETS))
def test_every_other_output_keeps_its_bytes(name):
    pipe_on, on, _, _ = run_pipe(name, G.ROWS)
    pipe_off, off, _, _ = run_pipe(name, None)
    assert 'gt_bboxes_ignore' not in off and set(on) - set(off) == {'gt_bboxes_ignore'}
    assert torch.equal(pipe_on.params, pipe_off.params)
    for key in ('gt_bboxes', 'gt_keypointss'):
        assert torch.equal(on[key].padded, off[key].padded) and torch.equal(on[key].counts, off[key].counts)
    assert on['img'].shape == off['img'].shape and torch.equal(on['img'], off['img'])
    assert on['img_metas'] == off['img_metas']


def test_source_without_ignore_tables_and_failed_decide_give_zero_counts():
    """A batch made without gt_bboxes_ignore stands for no ignore box; an image without GT has no window (cw == 0)."""
    from yunet_amd.pipelines import DevicePipeline, SourceBatch
    _, items, _ = G.load_set('s64')
    pipe = DevicePipeline(pipeline_of(64), seed=1, gmax=64, ignore_rows=16)
    imgs, boxes, kps = [it['img'] for it in items], [it['boxes'] for it in items], [it['kps'] for it in items]
    out = pipe(SourceBatch.from_lists(imgs, boxes, kps, DEV), 0)
    assert out['gt_bboxes_ignore'].counts.cpu().tolist() == [0, 0, 0, 0] and not bool(out['gt_bboxes_ignore'].padded.any())
    boxes[1], kps[1] = boxes[1][:0], kps[1][:0]
    ign = [np.array([[0, 0, 90, 90]], np.float32)] * 4
    out = pipe(SourceBatch.from_lists(imgs, boxes, kps, DEV, gt_bboxes_ignore=ign), 0)
    torch.cuda.synchronize()
    assert int(pipe.params[1, 2]) == 0 and int(out['gt_bboxes_ignore'].counts[1]) == 0
    assert not bool(out['gt_bboxes_ignore'].padded[1].any())


# --------------------------------------------------------------------------------------------------- mark kernel
SIZES, STRIDES, P = [(8, 8), (4, 4), (2, 2)], [8, 16, 32], 84


def run_mark(gt_inds, boxes, cnt, thr):
    import yunet_amd.kernels as k
    gi = gt_inds.to(DEV).clone()
    nm = torch.full((gi.shape[0],), -7, dtype=torch.int32, device=DEV)
    out = k.ignore_mark(gi, boxes.to(DEV), cnt.to(DEV), SIZES, STRIDES, thr, n_marked=nm)
    torch.cuda.synchronize()
    assert out is gi
    return gi.cpu(), nm.cpu()


def integer_case():
    gi = torch.zeros(3, P, dtype=torch.int32)
    gi[0, 9], gi[2, 20], gi[2, 69] = 2, 1, 5                      # positives under the boxes below
    boxes = torch.full((3, 16, 4), float('nan'))
    # image 0: half of cell (1, 1) at stride 8 (prior 9, a positive) and a quarter of cell (2, 1) (prior 10);
    #          [16, 32, 24, 36] is half of prior 34 = cell (4, 2) at stride 8 and 1/8 of a stride-16 cell
    boxes[0, 0] = torch.tensor([8.0, 8.0, 12.0, 16.0])
    boxes[0, 1] = torch.tensor([16.0, 8.0, 20.0, 12.0])
    boxes[0, 2] = torch.tensor([16.0, 32.0, 24.0, 36.0])
    # image 1: count 0, every row garbage (a box over the whole image, NaN rows): nothing may be read
    boxes[1, 0] = torch.tensor([-1e30, -1e30, 1e30, 1e30])
    # image 2: a large region over positives and background of all three levels; rows >= 1 are garbage
    boxes[2, 0] = torch.tensor([0.0, 0.0, 40.0, 48.0])
    boxes[2, 1] = torch.tensor([-1e30, -1e30, 1e30, 1e30])
    return gi, boxes, torch.tensor([3, 0, 1], dtype=torch.int32)


@pytest.mark.parametrize('thr', [0.25, 0.5, 0.0])
def test_mark_kernel_on_exact_thresholds(thr):
    gi, boxes, cnt = integer_case()
    want, iof = G.mark_ref(gi, torch.nan_to_num(boxes, nan=0.0), cnt, SIZES, STRIDES, thr)
    assert int((iof == thr).sum()) >= 2 if thr else True             # priors exactly ON the threshold exist (not marked)
    got, nm = run_mark(gi, boxes, cnt, thr)
    assert torch.equal(got, want)
    assert torch.equal(got[1], gi[1]) and int((got[1] != 0).sum()) == 0          # count 0: untouched, garbage not read
    assert int(got[0, 9]) == 2 and int(got[2, 20]) == 1 and int(got[2, 69]) == 5  # positives keep their assignment
    assert float(iof[2, 20]) > thr and float(iof[2, 69]) > thr and float(iof[0, 9]) == 0.5
    assert nm.tolist() == [int((got[n] == -1).sum()) for n in range(3)] and nm[2] > 0
    if thr == 0.0:
        assert torch.equal(got == -1, (iof > 0) & (gi == 0))         # any overlap marks
        assert int(got[0, 10]) == -1 and int(got[0, 34]) == -1
    if thr == 0.25:
        assert int(got[0, 10]) == 0 and int(got[0, 34]) == -1          # 0.25 is not > 0.25; 0.5 is
    if thr == 0.5:
        assert int((got[0] == -1).sum()) == 0                          # 0.5 is not > 0.5


def random_case(seed=3):
    g = torch.Generator().manual_seed(seed)
    gi = torch.zeros(3, P, dtype=torch.int32)
    gi[torch.rand(3, P, generator=g) < 0.1] = 1
    x1, y1 = torch.rand(3, 16, generator=g) * 56 - 4, torch.rand(3, 16, generator=g) * 56 - 4
    boxes = torch.stack([x1, y1, x1 + 2 + torch.rand(3, 16, generator=g) * 30, y1 + 2 + torch.rand(3, 16, generator=g) * 30], 2)
    return gi, boxes.float().contiguous(), torch.tensor([16, 5, 1], dtype=torch.int32)


@pytest.mark.parametrize('thr', [0.25, 0.5])
def test_mark_kernel_on_random_float_boxes(thr):
    """fp32 against fp64: priors within 1e-6 of the threshold in fp64 are left out; the seed keeps them under 1 % of P
    (the restatement alone decides that, on the CPU)."""
    gi, boxes, cnt = random_case()
    want, iof = G.mark_ref(gi, boxes, cnt, SIZES, STRIDES, thr)
    near = (iof - thr).abs() < 1e-6
    assert int(near.sum()) <= 0.01 * P
    assert int((want == -1).sum()) >= 20 and int(((iof > 0) & (iof <= thr)).sum()) >= 20
    got, nm = run_mark(gi, boxes, cnt, thr)
    assert torch.equal(got[~near], want[~near])
    assert torch.equal((got > 0), (gi > 0)) and nm.tolist() == [int((got[n] == -1).sum()) for n in range(3)]


def test_standalone_assigner_returns_the_marks():
    """SimOTAAssigner.assign(..., gt_bboxes_ignore=): -1 entries, which PseudoSampler counts neither as positive nor negative."""
    from yunet_amd.sim_ota_assigner import PseudoSampler, SimOTAAssigner
    g = torch.Generator().manual_seed(7)
    pri = O.grid_priors(SIZES, STRIDES)
    priors = torch.cat([pri[:, :2] + pri[:, 2:] * 0.5, pri[:, 2:]], 1).to(DEV)
    dec = torch.cat([pri[:, :2] - 4, pri[:, :2] + pri[:, 2:] + 4], 1).to(DEV)
    scores = torch.rand(P, 1, generator=g).to(DEV)
    gt = torch.tensor([[10.0, 12.0, 30.0, 40.0]], device=DEV)
    ign = torch.tensor([[32.0, 0.0, 64.0, 64.0]], device=DEV)
    labels = torch.zeros(1, dtype=torch.int64, device=DEV)
    off = SimOTAAssigner().assign(scores, priors, dec, gt, labels, gt_bboxes_ignore=ign)
    on = SimOTAAssigner(ignore_iof_thr=0.5).assign(scores, priors, dec, gt, labels, gt_bboxes_ignore=ign)
    want, _ = G.mark_ref(off.gt_inds.int().cpu()[None], ign.cpu()[None], torch.tensor([1], dtype=torch.int32), SIZES, STRIDES, 0.5)
    assert int((off.gt_inds < 0).sum()) == 0 and torch.equal(on.gt_inds.cpu(), want[0].long())
    assert torch.equal(on.gt_inds > 0, off.gt_inds > 0) and int((on.gt_inds == -1).sum()) > 10
    s = PseudoSampler().sample(on, dec, gt)
    assert s.pos_inds.numel() + s.neg_inds.numel() + int((on.gt_inds == -1).sum()) == P


# ----------------------------------------------------------------------------------------------------------- loss
_loss = {}


def loss_case(key):
    """The regime batches, built and referenced once: (case, marked, gt_inds with the marks)."""
    if key not in _loss:
        case = R.make_case(3, 160, 160, 13, boxes=ALL_BOXES) if key == 'square' else R.make_case(2, 320, 480, 21, boxes=ALL_BOXES)
        marked, gi = G.mark_some(case, seed=4)
        _loss[key] = (case, marked, gi)
    return _loss[key]


def run_loss(case, cfg_k, gt_inds=None, ignore=False, grad=True):
    """kernels.loss -> (losses [4], dflat | None, partials) on the host; dflat starts as NaN."""
    import yunet_amd._lib as L
    import yunet_amd.kernels as k
    d = _dev(case)
    gi = d['gt_inds'] if gt_inds is None else gt_inds.to(DEV).contiguous()
    N, Pn, _ = d['flat'].shape
    part = torch.full((int(L.load().yunet_loss_blocks(N, Pn)), 4), float('nan'), device=DEV)
    losses, dflat, _ = k.loss(d['flat'], gi, d['max_overlaps'], d['gt_boxes'], d['gt_kps'], d['img_stats'], d['sizes'],
                              d['strides'], cfg_k, grad=grad, partials=part, ignore=ignore)
    torch.cuda.synchronize()
    return losses.cpu(), None if dflat is None else dflat.cpu(), part.cpu()


@pytest.mark.parametrize('key', ['square', 'rect'])
def test_flagged_loss_per_element_and_everything_else_byte_equal(key):
    case, marked, gi = loss_case(key)
    share = float(marked.sum()) / float((case['gt_inds'] == 0).sum())
    assert 0.28 < share < 0.39
    cfg = R.make_cfg('EIoULoss')
    kc = R.kernel_cfg(cfg)
    l0, d0, p0 = run_loss(case, kc)                                   # unflagged, nothing marked
    l1, d1, p1 = run_loss(case, kc, gt_inds=gi, ignore=True)
    # loss_obj and the obj channel per element, at the loss kernel's own bars: the masked case IS a plain case
    mc = G.masked_case(case, marked)
    rep = R.check(l1, d1, mc, cfg)
    print(f'\n[{key}] marked {int(marked.sum())} of {int((case["gt_inds"] == 0).sum())} background priors: {rep}')
    assert rep.ok, rep
    assert rep.n_amb + rep.n_unres <= 0.01 * rep.n_pos + 5 and rep.loss_rel_bar <= MAX_LOSS_BAR, rep
    ref = G.masked_loss_ref(case, cfg, marked)
    assert float(ref['losses'][2]) < 0.8 * float(ref['ref']['losses'][2])          # the mask is not a rounding matter
    # the other three losses and every other channel: the bytes of the unflagged run
    assert torch.equal(l1[[0, 1, 3]], l0[[0, 1, 3]]) and not torch.equal(l1[2], l0[2])
    others = [c for c in range(16) if c != 5]
    assert torch.equal(d1[..., others], d0[..., others])
    assert torch.equal(d1[..., 5][~marked], d0[..., 5][~marked])
    assert torch.equal(p1[:, [0, 1, 3]], p0[:, [0, 1, 3]])
    assert bool((d1[marked] == 0).all()) and bool((d0[..., 5][marked] != 0).any())     # marked rows: all 16 channels 0
    # the flag with nothing marked: every byte of the unflagged run
    l2, d2, p2 = run_loss(case, kc, ignore=True)
    assert torch.equal(l2, l0) and torch.equal(d2, d0) and torch.equal(p2, p0)
    # the value-only instance: the partial rows of the gradient instance
    l3, d3, p3 = run_loss(case, kc, gt_inds=gi, ignore=True, grad=False)
    assert d3 is None and torch.equal(p3, p1) and torch.equal(l3, l1)
    # without the flag a negative entry is background, as it always was
    l4, d4, _ = run_loss(case, kc, gt_inds=gi)
    assert torch.equal(l4, l0) and torch.equal(d4, d0)


def test_flagged_varifocal_objectness():
    case = LT.make_case(*LT.GOLDEN_CASE)
    cfg = LT.make_cfg(**LT.GOLDEN_CONFIGS['vfl_a0.75_g2.0_iw1'])
    kc, kt = LT.kernel_cfg(cfg)
    kc.terms = kt
    marked, gi = G.mark_some(case, seed=5)
    l0, d0, p0 = run_loss(case, kc)
    l1, d1, p1 = run_loss(case, kc, gt_inds=gi, ignore=True)
    rep = LT.check(l1, d1, G.masked_case(case, marked), cfg)
    print(f'\n[varifocal obj] {rep}')
    assert rep.ok, rep
    assert torch.equal(l1[[0, 1, 3]], l0[[0, 1, 3]]) and float(l1[2]) < float(l0[2])
    assert bool((d1[marked] == 0).all()) and bool((d0[..., 5][marked] != 0).any())
    assert torch.equal(d1[~marked], d0[~marked])
    l2, d2, p2 = run_loss(case, kc, ignore=True)
    assert torch.equal(l2, l0) and torch.equal(d2, d0) and torch.equal(p2, p0)
    _, _, p3 = run_loss(case, kc, gt_inds=gi, ignore=True, grad=False)
    assert torch.equal(p3, p1)


# --------------------------------------------------------------------------------------------------------- engine
SEED, THR = 4101, 0.5
IGN = [torch.tensor([[0.0, 0.0, 32.0, 32.0], [36.0, 4.0, 64.0, 44.0]]), torch.zeros(0, 4)]


def build(thr=None, kind='n'):
    import yunet_amd
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    if thr is not None:
        cfg.model.train_cfg.assigner['ignore_iof_thr'] = thr
    m = yunet_amd.build_detector(cfg.model)
    m.load_state_dict(O.init_state(O.yunet_arch(kind), seed=SEED), strict=True)
    return m.to(DEV).train()


def oracle_masked_step(b, training=True):
    """The oracle's step on batch b with the marked priors outside loss_obj -> (losses, grads, aux, marked)."""
    arch = O.yunet_arch('n')
    sd = O.init_state(arch, seed=SEED)
    leaf = {k: sd[k].detach().clone().requires_grad_(True) for k in O.param_keys(sd)}
    work = dict(sd)
    work.update(leaf)
    maps = O.conv_stack_forward(b['img'], work, arch, training=training)
    flat = O.flatten_preds(*maps)
    sizes = [tuple(c.shape[2:]) for c in maps[0]]
    losses, aux = O.loss_step(flat, b['gt_bboxes'], b['gt_labels'], b['gt_keypointss'], sizes, arch)
    gi = aux['gt_inds']
    ib = torch.zeros(2, 16, 4)
    ib[0, :2] = IGN[0]
    want, iof = G.mark_ref(gi.int(), ib, torch.tensor([2, 0], dtype=torch.int32), sizes, arch['strides'], THR)
    marked = want == -1
    terms = torch.nn.functional.binary_cross_entropy_with_logits(flat[..., 5], (gi > 0).float(), reduction='none')
    losses = dict(losses)
    losses['loss_obj'] = arch['loss_obj_weight'] * (terms * (~marked).float()).sum() / max(float(aux['num_pos']), 1.0)
    grads = None
    if training:
        sum(losses.values()).backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    aux.update(flat=flat.detach(), sizes=sizes, iof=iof)
    return {k: float(v.detach()) for k, v in losses.items()}, grads, aux, marked


def batch():
    import yunet_amd.synthetic as S
    return S.make_batch(2, 64, 64, SEED)


def test_engine_step_against_the_oracle_with_the_mask():
    """YuNet_n, 64 x 64, bs 2, two ignore boxes on image 0: losses, assignment with marks, every parameter gradient."""
    import yunet_amd.synthetic as S
    b = batch()
    lv, grads, aux, marked = oracle_masked_step(b)
    for i in range(2):      # the seed keeps SimOTA clear of ties, so the assignment has to be the oracle's
        assert not Hh.image_near_tie(aux['flat'][i], b['gt_bboxes'][i], aux['sizes'])
    assert int(marked.sum()) >= 30 and int(((aux['gt_inds'][0] > 0) & (aux['iof'][0] > THR)).sum()) >= 1
    assert int(((aux['iof'] - THR).abs() < 1e-6).sum()) == int((aux['iof'] == THR).sum())      # exact or clear of it
    m = build(THR)
    db = S.to_device(b, DEV)
    losses = m.forward_train(**db, gt_bboxes_ignore=[t.to(DEV) for t in IGN])
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    plan = m.engine.plan
    assert plan.imax == 16 and any('ignore' in k for k in m.engine.plans)
    want_gi = aux['gt_inds'].int().clone()
    want_gi[marked] = -1
    assert torch.equal(plan.gt_inds.cpu(), want_gi)
    for k in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps'):
        assert abs(float(losses[k]) - lv[k]) <= 1e-4 * abs(lv[k]) + 1e-6, (k, float(losses[k]), lv[k])
    dflat = plan.dflat.cpu()
    assert bool((dflat[marked] == 0).all())
    sd = O.init_state(O.yunet_arch('n'), seed=SEED)
    g64 = Hh.fp64_conv_grads(b, sd, O.yunet_arch('n'), dflat)
    scale = max(float(v.abs().max()) for v in g64.values())
    for k, v in grads.items():
        got = dict(m.named_parameters())[k].grad.cpu().double()
        err_hip = float((got - g64[k]).abs().max())
        err_ref = float((v.double() - g64[k]).abs().max())
        tol = 10 * max(err_ref, 1e-5 * scale) + 1e-2 * float(g64[k].abs().max())
        assert err_hip <= tol, (k, err_hip, err_ref, float(g64[k].abs().max()), scale)
    # a DeviceGT is bound without a copy; a list was padded on the device; None is zero counts
    from yunet_amd.pipelines import DeviceGT
    pb = torch.zeros(2, 16, 4, device=DEV)
    pb[0, :2] = IGN[0].to(DEV)
    dg = DeviceGT(list(pb))
    dg.padded, dg.counts = pb, torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    l2 = m.forward_train(**db, gt_bboxes_ignore=dg)
    torch.cuda.synchronize()
    assert m.engine.plan is plan and plan.c_fwd_a[plan.mark_idx].p[0] == pb.data_ptr()
    assert all(torch.equal(l2[k], losses[k]) for k in losses)
    l3 = m.forward_train(**db, gt_bboxes_ignore=None)
    torch.cuda.synchronize()
    assert int((m.engine.plan.gt_inds < 0).sum()) == 0 and float(l3['loss_obj']) > float(losses['loss_obj'])


def test_threshold_off_gives_the_bytes_of_a_run_without_ignore_boxes():
    import yunet_amd.synthetic as S
    db = S.to_device(batch(), DEV)
    out = []
    for ign in (None, [t.to(DEV) for t in IGN]):
        m = build(-1)
        losses = m.forward_train(**db, gt_bboxes_ignore=ign)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        assert not any('ignore' in k for k in m.engine.plans)
        out.append((torch.stack([losses[k].detach() for k in sorted(losses)]).cpu(), m.engine.params.grad.cpu().clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    # and equal to a model that never heard of the option, next to one with the threshold on
    m = build(None)
    losses = m.forward_train(**db)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert torch.equal(torch.stack([losses[k].detach() for k in sorted(losses)]).cpu(), out[0][0])
    assert torch.equal(m.engine.params.grad.cpu(), out[0][1])


def test_one_validation_step():
    """model.eval(): the value-only flagged instance behind the eval-mode conv stack, against the oracle in eval mode."""
    import yunet_amd.synthetic as S
    b = batch()
    lv, _, aux, marked = oracle_masked_step(b, training=False)
    for i in range(2):
        assert not Hh.image_near_tie(aux['flat'][i], b['gt_bboxes'][i], aux['sizes'])
    m = build(THR)
    m.eval()
    grad_before = m._ensure_engine(torch.device(DEV, torch.cuda.current_device())).params.grad.clone()
    with torch.no_grad():
        losses = m.forward_train(**S.to_device(b, DEV), gt_bboxes_ignore=[t.to(DEV) for t in IGN])
    torch.cuda.synchronize()
    plan = m.engine.plan
    want_gi = aux['gt_inds'].int().clone()
    want_gi[marked] = -1
    assert torch.equal(plan.gt_inds.cpu(), want_gi) and int(marked.sum()) >= 30
    for k in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps'):
        assert abs(float(losses[k]) - lv[k]) <= 1e-4 * abs(lv[k]) + 1e-6, (k, float(losses[k]), lv[k])
    assert torch.equal(m.engine.params.grad, grad_before)


@pytest.mark.parametrize('level', [True, 'fast'])
def test_deterministic_levels_repeat_bytes(level):
    import yunet_amd.synthetic as S
    db = S.to_device(batch(), DEV)
    ign = [t.to(DEV) for t in IGN]
    runs = []
    for _ in range(2):
        m = build(THR)
        m.set_deterministic(level)
        losses = m.forward_train(**db, gt_bboxes_ignore=ign)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        assert int((m.engine.plan.gt_inds < 0).sum()) >= 30
        runs.append((torch.stack([losses[k].detach() for k in sorted(losses)]).cpu(), m.engine.params.grad.cpu().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_standalone_head_loss_uses_the_marks():
    """YuNet_Head.loss(..., gt_bboxes_ignore=) outside the engine: the engine's losses and its assignment with marks."""
    import yunet_amd.synthetic as S
    b = batch()
    lv, _, aux, marked = oracle_masked_step(b)
    m = build(THR)
    fl = aux['flat'].to(DEV).requires_grad_(True)
    cls, box, obj, kps = [], [], [], []
    off = 0
    for (fh, fw) in aux['sizes']:
        mm = fl[:, off:off + fh * fw].reshape(2, fh, fw, 16).permute(0, 3, 1, 2)
        cls.append(mm[:, 0:1]); box.append(mm[:, 1:5]); obj.append(mm[:, 5:6]); kps.append(mm[:, 6:16])
        off += fh * fw
    db = S.to_device(b, DEV)
    losses = m.bbox_head.loss(cls, box, obj, kps, db['gt_bboxes'], db['gt_labels'], db['gt_keypointss'], [dict(), dict()],
                              gt_bboxes_ignore=[t.to(DEV) for t in IGN])
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    want_gi = aux['gt_inds'].int().clone()
    want_gi[marked] = -1
    assert torch.equal(m.bbox_head.last_gt_inds.cpu(), want_gi)
    for k in ('loss_cls', 'loss_bbox', 'loss_obj', 'loss_kps'):
        assert abs(float(losses[k]) - lv[k]) <= 1e-4 * abs(lv[k]) + 1e-6, (k, float(losses[k]), lv[k])
    assert bool((fl.grad.cpu()[marked] == 0).all())


# ------------------------------------------------------------------------------------------- source, end to end
def write_dataset(root, w=96, h=80):
    """Three PNGs with 0, 2 and 20 ignore boxes: image 1 has one flagged row and one face below min_size = 8."""
    from PIL import Image
    rng = np.random.default_rng(9)
    lines = []
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / f'im{i}.png')
        lines.append(f'# im{i}.png {w} {h}')
        for g in range(2):
            x, y = 10 + 40 * g, 12 + 20 * g
            kp = ' '.join(f'{x + 3 + 2 * j} {y + 4 + j} 1' for j in range(5))
            lines.append(f'{x} {y} {x + 24} {y + 28} {kp}')
        if i == 1:
            lines.append('60 8 80 30 1')                                                   # labelv2's ignore flag
            lines.append('40 60 46 67 ' + ' '.join(f'{41 + j} {62 + j} 1' for j in range(5)))  # 6 x 7 px: below min_size
        if i == 2:
            for g in range(20):
                x, y = 2 + 9 * (g % 10), 3 + 40 * (g // 10)
                lines.append(f'{x} {y} {x + 7} {y + 9} 1')
    (root / 'labelv2.txt').write_text('\n'.join(lines) + '\n')
    return str(root / 'labelv2.txt'), str(root)


def test_source_end_to_end_both_caches(tmp_path):
    from yunet_amd.datasets import RetinaFaceDataset, RetinaFaceSource, ignore_counts
    ann, prefix = write_dataset(tmp_path)
    ds = RetinaFaceDataset(ann, img_prefix=prefix, pipeline=PIPELINE, min_size=8)
    assert ignore_counts(ds) == [0, 2, 20]
    kw = dict(samples_per_gpu=3, workers=0)
    plain = RetinaFaceSource(ds, PIPELINE, cache=None, ignore_capacity='dataset', **kw)
    cached = RetinaFaceSource(ds, PIPELINE, cache='device', ignore_capacity='dataset', **kw)
    off = RetinaFaceSource(ds, PIPELINE, cache='device', **kw)
    assert plain.ignore_rows == 32 and off.ignore_rows is None
    kept = 0
    for it in range(3):
        a, b, c = plain.batch(it, DEV), cached.batch(it, DEV), off.batch(it, DEV)
        torch.cuda.synchronize()
        assert 'gt_bboxes_ignore' not in c and torch.equal(a['img'], c['img'])
        for key in ('gt_bboxes', 'gt_keypointss', 'gt_bboxes_ignore'):
            assert torch.equal(a[key].padded, b[key].padded) and torch.equal(a[key].counts, b[key].counts), (it, key)
        assert torch.equal(a['img'], b['img']) and torch.equal(a['gt_bboxes'].padded, c['gt_bboxes'].padded)
        ign, params = a['gt_bboxes_ignore'], plain.pipe.params.cpu().numpy()
        assert tuple(ign.padded.shape) == (3, 32, 4)
        for k, i in enumerate(plain._indices(it)):
            left, top, cw, flip = (int(v) for v in params[k, :4])
            rows, _ = G.transform(ds.get_ann_info(i)['bboxes_ignore'], left, top, cw, 64, bool(flip))
            assert int(ign.counts[k]) == len(rows)
            assert np.array_equal(ign.padded[k, :len(rows)].cpu().numpy(), rows) and not bool(ign.padded[k, len(rows):].any())
            kept += len(rows)
    assert kept > 0
