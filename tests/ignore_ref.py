"""TEST INFRASTRUCTURE ONLY -- fp64 / numpy restatements for the ignore-region feature.  Nothing in
the product imports this.

  mark_ref           the rule of yunet_ignore_mark in float64: the candidate box of prior (x, y, s) is its cell
                     [x, y, x+s, y+s]; iof = iw * ih / (s * s); a background prior (gt_inds == 0) whose largest iof over
                     its image's ignore boxes is > thr (strict) gets gt_inds = -1; positives stay.
  masked_loss_ref    the loss step with marked priors outside loss_obj, built on tests/loss_ref.py by import: the obj
                     terms of the marked priors leave the sum, their dflat row is 0, everything else is loss_ref's.
  masked_case        the same thing as an ordinary loss_ref case, so that loss_ref.check grades a flagged kernel run at
                     its own bars: a marked prior becomes background with the objectness logit -1e4, whose BCE (and
                     Varifocal) term and gradient are exactly 0 in float32 and float64.  test_ignore.py holds the two
                     equal.
  the pipeline part  what RandomSquareCrop -> Resize -> RandomFlip do to gt_bboxes_ignore, on oracle/pipeline_oracle.py's
                     own GT arithmetic, and the inputs of tests/golden/ignore_cases.npz (tools/make_golden_ignore.py
                     runs the unmodified reference on them)."""
import os

import numpy as np
import torch

import loss_ref as R
import pipeline_oracle as P
import yunet_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ignore_cases.npz')
OFF_LOGIT = -1.0e4            # softplus(-1e4) = 0 and sigmoid(-1e4) = 0 exactly, in fp32 and fp64


# ------------------------------------------------------------------------------------------------------- mark rule
def iof_ref(ign_boxes, ign_count, sizes, strides):
    """-> [N,P] float64: the largest share of each prior's cell covered by one of its image's first ign_count boxes
    (0 where the image has none).  Rows >= count are not read."""
    pri = O.grid_priors(sizes, strides, torch.float64)           # x, y, s, s (offset 0)
    x, y, s = pri[:, 0], pri[:, 1], pri[:, 2]
    N = ign_boxes.shape[0]
    out = torch.zeros(N, pri.shape[0], dtype=torch.float64)
    for n in range(N):
        b = ign_boxes[n, :max(0, min(int(ign_count[n]), ign_boxes.shape[1]))].double()
        if b.shape[0] == 0:
            continue
        iw = (torch.minimum(b[:, None, 2], (x + s)[None]) - torch.maximum(b[:, None, 0], x[None])).clamp_min(0)
        ih = (torch.minimum(b[:, None, 3], (y + s)[None]) - torch.maximum(b[:, None, 1], y[None])).clamp_min(0)
        out[n] = (iw * ih / (s * s)[None]).max(0).values
    return out


def mark_ref(gt_inds, ign_boxes, ign_count, sizes, strides, thr):
    """-> (gt_inds with the marks, iof [N,P] float64).  thr is the fp32 value the kernel receives."""
    iof = iof_ref(ign_boxes, ign_count, sizes, strides)
    out = gt_inds.clone()
    out[(gt_inds == 0) & (iof > float(np.float32(thr)))] = -1
    return out, iof


# ------------------------------------------------------------------------------------------------------ masked loss
def masked_loss_ref(case, cfg, marked, **kw):
    """loss_ref with the priors of `marked` ([N,P] bool, background priors) outside loss_obj -> dict(losses, dflat)."""
    assert not bool((marked & (case['gt_inds'] > 0)).any())
    r = R.ref_of(case, cfg, **kw)
    keep = (~marked).to(torch.float64)
    losses = r['losses'].clone()
    losses[2] = cfg['w_obj'] * (r['terms']['obj'] * keep).sum() / r['num_total']
    dflat = r['dflat'].clone()
    dflat[..., 5] = dflat[..., 5] * keep
    assert bool((dflat[marked] == 0).all())           # a background prior has no other channel
    return dict(losses=losses, dflat=dflat, ref=r)


def masked_case(case, marked):
    """The loss_ref case whose plain losses / dflat are the masked ones of `case` (module docstring)."""
    out = dict(case)
    flat = case['flat'].clone()
    flat[..., 5] = torch.where(marked, torch.tensor(OFF_LOGIT), flat[..., 5])
    gi = case['gt_inds'].clone()
    gi[marked] = 0
    out['flat'], out['gt_inds'] = flat.contiguous(), gi
    return out


def mark_some(case, share=1.0 / 3.0, seed=0):
    """About `share` of the background priors of a loss_ref case -> (marked [N,P] bool, gt_inds with -1 there)."""
    g = torch.Generator().manual_seed(seed)
    marked = (torch.rand(case['gt_inds'].shape, generator=g) < share) & (case['gt_inds'] == 0)
    gi = case['gt_inds'].clone()
    gi[marked] = -1
    return marked, gi


# --------------------------------------------------------------------------------------------------------- pipeline
CROP_CHOICE = [0.5, 0.7, 0.9, 1.1, 1.3, 1.5]
ROWS = 16                     # padded ignore rows per image of the fixture's runs
SHAPES = [(40, 56, 2), (90, 70, 3), (64, 64, 1), (57, 83, 4)]          # (h, w, faces) per source
#        set    seed base-iteration Resize
SETS = {'s64': (71, 0, 64), 'r32_96': (73, 0, (32, 96))}
KIND = ('crafted', 'none', 'many', 'random')                            # what image i's ignore boxes are


def sources(seed):
    """-> (uint8 images, GT boxes, GT keypoints) of SHAPES from the seed (pipeline_oracle.synth_image)."""
    rng = np.random.default_rng(seed)
    return zip(*[P.synth_image(rng, h, w, g) for h, w, g in SHAPES])


def decide(h, w, boxes, seed, iteration, image, size):
    """The draws of one image -> (left, top, cw, S, flip, draws): pipeline_oracle's crop decision, the square_range draw
    when `size` is (lo, hi) (tests/multiscale_ref.py), one uniform for the flip."""
    st = P.Stream(seed, iteration, image)
    left, top, cw = P.decide_crop(h, w, boxes, CROP_CHOICE, st)
    S = size if isinstance(size, int) else st.randint(size[0], size[1] + 1) // 32 * 32
    flip = st.uniform() < 0.5
    return left, top, cw, S, bool(flip), st.ctr


def craft(kind, h, w, left, top, cw, rng):
    """Ignore boxes of one image, placed against its crop window (the window is accepted on gt_bboxes alone, so they do
    not move it).  float32 [I,4]."""
    if kind == 'none':
        return np.zeros((0, 4), np.float32)
    if kind == 'crafted':
        m = cw // 2
        rows = [[left - 4, top + 4, left + 4, top + 12],                  # centre ON the left edge: dropped (strict >)
                [left - 6, top - 5, left + 10, top + 9],                  # kept, clipped on two sides (left and top)
                [left + m - 3, top + m - 4, left + m + 5, top + m + 6],   # kept, inside
                [left + cw + 3, top, left + cw + 9, top + 8],             # outside: dropped
                [left + 8, top + cw - 3, left + 14, top + cw + 3],        # centre ON the bottom edge: dropped
                [left + cw - 7, top + cw - 9, left + cw + 5, top + cw + 3]]   # kept, clipped right and bottom
        return np.array(rows, np.float32)
    if kind == 'many':
        # 17 boxes with the centre inside the window (one more than ROWS), three outside, interleaved
        rows = []
        for k in range(17):
            cx, cy = left + (k % 5 + 0.5) * cw / 5.0, top + (k // 5 + 0.5) * cw / 4.0
            rows.append([cx - 1.25 - 0.25 * k, cy - 2.0, cx + 1.25 + 0.25 * k, cy + 1.5])
            if k in (2, 9, 13):
                rows.append([left - 30.0 - k, top - 30.0, left - 20.0 - k, top - 22.0])
        return np.array(rows, np.float32)
    x1, y1 = rng.uniform(-8, w - 4, 6), rng.uniform(-8, h - 4, 6)
    return np.stack([x1, y1, x1 + rng.uniform(3, 30, 6), y1 + rng.uniform(3, 30, 6)], 1).astype(np.float32)


def transform(ign, left, top, cw, S, flip):
    """gt_bboxes_ignore through crop -> resize -> flip, on pipeline_oracle's GT arithmetic -> (rows [K,4] float32, mask)."""
    kps = np.zeros((len(ign), 5, 3), np.float32)
    b, k, mask = P.crop_gt(ign, kps, left, top, cw)
    b, k = P.resize_gt(b, k, cw, S)
    if flip:
        b, k = P.flip_gt(b, k, S)
    return b.astype(np.float32), mask


def build_set(name, iteration):
    """The inputs of set `name` at `iteration` -> list of per-image dicts (img, boxes, kps, ign, window, S, flip, draws)."""
    seed, _, size = SETS[name]
    rng = np.random.default_rng(seed + 1000)
    out = []
    for i, (im, b, k) in enumerate(zip(*sources(seed))):
        h, w = im.shape[:2]
        left, top, cw, S, flip, draws = decide(h, w, b, seed, iteration, i, size)
        out.append(dict(img=im, boxes=b, kps=k, ign=craft(KIND[i], h, w, left, top, cw, rng), left=left, top=top, cw=cw, S=S,
                        flip=flip, draws=draws))
    return out


def hard_cases(items, outs):
    """What a set holds: items of build_set, outs = the transformed kept rows per image."""
    seen = dict(edge_centre_dropped=False, clipped_two_sides=False, flipped=False, unflipped=False, empty=False, overflow=False)
    for it, o in zip(items, outs):
        ign, left, top, cw = it['ign'], it['left'], it['top'], it['cw']
        if len(ign) == 0:
            seen['empty'] = True
            continue
        c = (ign[:, :2] + ign[:, 2:]) / 2
        _, mask = transform(ign, left, top, cw, it['S'], it['flip'])
        on_edge = (c[:, 0] == left) | (c[:, 0] == left + cw) | (c[:, 1] == top) | (c[:, 1] == top + cw)
        seen['edge_centre_dropped'] |= bool((on_edge & ~mask).any())
        two = ((ign[:, 0] < left).astype(int) + (ign[:, 1] < top) + (ign[:, 2] > left + cw) + (ign[:, 3] > top + cw)) >= 2
        seen['clipped_two_sides'] |= bool((two & mask).any())
        seen['flipped' if it['flip'] else 'unflipped'] |= bool(mask.any())
        seen['overflow'] |= int(mask.sum()) > ROWS
    return seen


def load_set(name):
    """tests/golden/ignore_cases.npz, set `name` -> (iteration, items of build_set at it, reference outputs per image)."""
    z = np.load(GOLD)
    iteration = int(z[f'{name}/iteration'])
    items = build_set(name, iteration)
    outs = []
    for i, it in enumerate(items):
        assert np.array_equal(z[f'{name}/ign_src_{i}'], it['ign']) and np.array_equal(z[f'{name}/boxes_{i}'], it['boxes'])
        assert np.array_equal(z[f'{name}/meta_{i}'], [it['left'], it['top'], it['cw'], int(it['flip']), it['S'], it['draws']])
        outs.append(z[f'{name}/ign_{i}'])
    return iteration, items, outs


def padded(outs, rows=ROWS):
    """The kernel's layout: the first `rows` kept rows per image, zeros behind -> ([N,rows,4] float32, [N] int32)."""
    ob = np.zeros((len(outs), rows, 4), np.float32)
    oc = np.zeros(len(outs), np.int32)
    for i, o in enumerate(outs):
        oc[i] = min(len(o), rows)
        ob[i, :oc[i]] = o[:oc[i]]
    return ob, oc
