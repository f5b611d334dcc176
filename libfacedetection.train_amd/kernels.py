"""Tensor-level wrappers of the C ABI (one call = one kernel launch on torch's current stream).

PyTorch is only the container here: tensors are allocated with torch, their `data_ptr()`s
are handed to libyunet_hip.so.  Layout conventions: activations NHWC fp32 contiguous,
parameters in the reference's OIHW shapes (made contiguous 2-D views on the fly).
"""
import ctypes as C

import torch

from . import _lib as L


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _act(t):
    """(storage flag, entry-point suffix) of an activation tensor: fp32 or bf16 (BASELINE configs[2])."""
    if t.dtype == torch.bfloat16:
        return L.BF16, '_bf16'
    assert t.dtype == torch.float32, 'activations are fp32 or bf16'
    return L.F32, ''


def _chk_act(*ts):
    for t in ts:
        if t is not None:
            assert t.is_cuda and t.dtype in (torch.float32, torch.bfloat16) and t.is_contiguous(), \
                'expected a contiguous fp32 / bf16 CUDA tensor'


def _chk_f32(*ts):
    for t in ts:
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), \
                'expected a contiguous fp32 CUDA tensor'


class BN:
    """Python-side YunetBN: keeps the tensors alive while the descriptor is in use."""

    def __init__(self, stats, gamma, beta, count, eps=1e-5, bstats=None, slots=1, det_rows=0):
        # slots > 1: stats / bstats are [slots, 2C] replica blocks (YunetBN::slots); the sums are their column sums
        # det_rows = R > 0 (deterministic sums, YunetBN::det_rows): [1 + R, 2C] blocks, row 0 = the sums after bn_fold
        # (det_rows may carry L.DET_FAST above the row count: the fast deterministic level, same blocks)
        rows = 1 + (det_rows & (L.DET_FAST - 1)) if det_rows else slots
        assert not det_rows or slots == 1
        assert stats.dtype == torch.float64 and stats.numel() == rows * 2 * gamma.numel()
        assert bstats is None or bstats.numel() == rows * 2 * gamma.numel()
        self.stats, self.gamma, self.beta, self.bstats = stats, gamma, beta, bstats
        self.count, self.eps, self.slots, self.det_rows = int(count), float(eps), int(slots), int(det_rows)

    def c(self):
        return L.YunetBN(self.stats.data_ptr(), self.bstats.data_ptr() if self.bstats is not None
                         else None, self.gamma.data_ptr(), self.beta.data_ptr(), self.count,
                         self.eps, self.slots, self.det_rows)


_NULL_BN = L.YunetBN(None, None, None, None, 1, 1e-5)


def conv_blocks():
    return L.load().yunet_conv_blocks()


def dp_grid(n, h, w, cin=64, cout=64):
    """rows of the weight-gradient partial buffer (= persistent grid) of yunet_dp_bwd"""
    return L.load().yunet_dp_bwd_blocks(n, h, w, cin, cout)


def stem_grid(n, h, w):
    return L.load().yunet_stem_bwd_blocks(n, h, w)


def dp_row_width(cin, cout):
    return cout * cin + cout + cout * 9 + cout


def stem_fwd(img, w, b, stats, dtype=torch.float32):
    """img [N,3,H,W] NCHW -> raw z [N,H/2,W/2,16] NHWC (fp32 or bf16 storage); accumulates stats (fp64 [32])."""
    _chk_f32(img, w, b)
    n, _, h, ww = img.shape
    z = torch.empty(n, h // 2, ww // 2, 16, device=img.device, dtype=dtype)
    fn = getattr(L.load(), 'yunet_stem_fwd' + _act(z)[1])
    L.check(fn(_p(img), _p(w), _p(b), _p(z), _p(stats), n, h, ww, 16, _stream()), 'yunet_stem_fwd')
    return z


def stem_fwd_det(img, w, b, block):
    """stem_fwd (fp32 storage) with order-fixed BN sums: block fp64 [1 + R, 32], workgroup g adds to row 1 + g."""
    _chk_f32(img, w, b)
    n, _, h, ww = img.shape
    assert block.dtype == torch.float64 and block.dim() == 2 and block.shape[1] == 32 and block.is_contiguous()
    z = torch.empty(n, h // 2, ww // 2, 16, device=img.device, dtype=torch.float32)
    L.check(L.load().yunet_stem_fwd_det(_p(img), _p(w), _p(b), _p(z), _p(block), block.shape[0] - 1, n, h, ww, 16, _stream()),
            'yunet_stem_fwd_det')
    return z


def bn_fold(block):
    """block fp64 [1 + R, 2C]: row 0 = rows 1 .. R added in the fixed order of yunet_bn_fold."""
    assert block.dtype == torch.float64 and block.dim() == 2 and block.shape[1] % 2 == 0 and block.is_contiguous()
    L.check(L.load().yunet_bn_fold(_p(block), block.shape[0] - 1, block.shape[1] // 2, _stream()), 'yunet_bn_fold')
    return block[0]


def stem_bwd(img, z, dy, bn, w=None, b=None):
    """-> (dw [16,3,3,3], db [16]) given dy = grad wrt bn1 output (ReLU-masked).  With the stem's parameters (w, b) and
    fp32 storage, z is recomputed from the image instead of read (yunet_stem_bwd_rz: what a training step runs)."""
    n, _, h, wd = img.shape
    blocks = stem_grid(n, h, wd)
    width = 16 * 27 + 16
    part = torch.empty(blocks, width, device=img.device, dtype=torch.float32)
    bnc = bn.c()
    if w is not None and b is not None and _act(z)[1] == '':
        L.check(L.load().yunet_stem_bwd_rz(_p(img), _p(w), _p(b), _p(dy), C.byref(bnc), _p(part), blocks, n, h, wd, 16,
                                           _stream()), 'yunet_stem_bwd_rz')
    else:
        fn = getattr(L.load(), 'yunet_stem_bwd' + _act(z)[1])
        L.check(fn(_p(img), _p(z), _p(dy), C.byref(bnc), _p(part), blocks, n, h, wd, 16, _stream()), 'yunet_stem_bwd')
    out = torch.empty(width, device=img.device, dtype=torch.float32)
    reduce_partials(part, out)
    return out[:432].view(16, 3, 3, 3), out[432:]


def stem_bwd_dx(img, z, dy, bn, w, b=None):
    """-> dimg [N,3,H,W] fp32 NCHW: the gradient w.r.t. the image given dy = grad wrt bn1 output (ReLU-masked), the stem's raw
    output z as stored (fp32 | bf16) and its weights w [16,3,3,3] (yunet_stem_bwd_dx[_bf16]).  Same arguments as stem_bwd:
    `img` gives the shape, and the bias does not enter this gradient."""
    _chk_act(z)
    _chk_f32(dy, w)
    n, _, h, wd = img.shape
    assert tuple(z.shape) == (n, h // 2, wd // 2, 16) and dy.shape == z.shape and w.numel() == 432
    dimg = torch.empty(n, 3, h, wd, device=z.device, dtype=torch.float32)
    bnc = bn.c()
    fn = getattr(L.load(), 'yunet_stem_bwd_dx' + _act(z)[1])
    L.check(fn(_p(z), _p(dy), C.byref(bnc), _p(w), _p(dimg), n, h, wd, 16, _stream()), 'yunet_stem_bwd_dx')
    return dimg


def reduce_partials(part, out, accumulate=False):
    L.check(L.load().yunet_reduce_partials(_p(part), part.shape[0], part.shape[1], _p(out),
                                           int(accumulate), _stream()), 'yunet_reduce_partials')


def reduce_job_table(jobs, device):
    """Device table of YunetReduceJob records for yunet_reduce_partials_batch.
    jobs: (partials ptr, out ptr, rows, width, accumulate).  Returns (table, total_chunks)."""
    import numpy as np
    tab = np.zeros((len(jobs), 4), dtype=np.int64)          # 32-byte records
    chunk = 0
    for r, (pp, op, rows, width, acc) in enumerate(jobs):
        tab[r, 0], tab[r, 1] = pp, op
        tab[r, 2] = (int(width) << 32) | int(rows)          # int32 blocks | int32 width
        tab[r, 3] = (chunk << 32) | int(acc)                # int32 accumulate | int32 chunk0
        chunk += (width + 63) // 64
    return torch.from_numpy(tab).to(device), chunk


def reduce_partials_batch(parts, outs, accumulate=None):
    """out_k[j] (+)= sum_b parts_k[b, j] for every pair, one launch."""
    acc = accumulate or [False] * len(parts)
    jobs = [(p.data_ptr(), o.data_ptr(), p.shape[0], p.shape[1], int(a))
            for p, o, a in zip(parts, outs, acc)]
    tab, chunks = reduce_job_table(jobs, parts[0].device)
    L.check(L.load().yunet_reduce_partials_batch(_p(tab), len(jobs), chunks, _stream()),
            'yunet_reduce_partials_batch')
    return tab      # keep alive until the launch has run


def _chk_strided(t, n, stride, dense, what):
    """a flat buffer that holds n images of `dense` elements, `stride` elements apart, from its first element on"""
    assert stride >= dense and t.numel() >= (n - 1) * stride + dense, \
        f'{what}: {n} images of {dense} elements at stride {stride} do not fit {t.numel()} elements'
    assert t.data_ptr() % 16 == 0 and (stride * t.element_size()) % 16 == 0, \
        f'{what}: every image must start on a 16-byte boundary (the kernels use 128-bit accesses)'


def _dp_desc(x, w_pw, b_pw, w_dw, b_dw, z, in_bn, out_bn, x_img_stride=None,
             z_img_stride=None, shape=None):
    """shape = (N, H, W): x and z are FLAT buffers (any tensor whose first element is image 0's first element), image i
    at element i * x_img_stride / i * z_img_stride; None: N, H, W come from the dense 4-D x."""
    cout, cin = w_pw.shape[0], w_pw.shape[1]
    if shape is None:
        n, h, w, xc = x.shape
        assert xc == cin
    else:
        n, h, w = shape
    d = L.YunetDP()
    d.N, d.H, d.W, d.cin, d.cout = n, h, w, cin, cout
    d.in_transform = L.T_BNRELU if in_bn is not None else L.T_IDENTITY
    d.out_has_bn = 1 if out_bn is not None else 0
    d.x_img_stride = x_img_stride if x_img_stride is not None else h * w * cin
    d.z_img_stride = z_img_stride if z_img_stride is not None else h * w * cout
    if shape is not None or x_img_stride is not None:
        _chk_strided(x, n, d.x_img_stride, h * w * cin, 'x')
    if z is not None and (shape is not None or z_img_stride is not None):
        _chk_strided(z, n, d.z_img_stride, h * w * cout, 'z')
    d.x = x.data_ptr()
    d.in_bn = in_bn.c() if in_bn is not None else _NULL_BN
    d.out_bn = out_bn.c() if out_bn is not None else _NULL_BN
    d.w_pw, d.b_pw, d.w_dw, d.b_dw = (w_pw.data_ptr(), b_pw.data_ptr(), w_dw.data_ptr(),
                                     b_dw.data_ptr())
    d.z = z.data_ptr()
    d.x_dtype = _act(x)[0]
    d.z_dtype = _act(z)[0]
    return d


def dp_fwd(x, w_pw, b_pw, w_dw, b_dw, in_bn=None, out_bn=None, z=None, z_img_stride=None, pool=False,
           x_img_stride=None, shape=None):
    """ConvDPUnit forward.  x [N,H,W,Cin] raw producer output (in_bn given) or activations, fp32 or
    bf16 storage.  Returns raw z [N,H,W,Cout] in x's storage type (pass z to choose: the fused heads
    write fp32); accumulates out_bn.stats when out_bn is given.
    pool=True (fused max_pool2d of the BN+ReLU output): returns (z, pooled, idx) -- pooled [N,H/2,W/2,Cout]
    holds the RAW z of every window's winner (feed it to the consumer with in_bn = this unit's BN),
    idx the uint8 window positions 2*dy + dx.
    shape = (N, H, W): x and z are flat buffers with x_img_stride / z_img_stride elements between images (YunetDP's
    fields; default: dense); z defaults to a fresh flat buffer of N * z_img_stride elements.  pooled and idx stay dense."""
    _chk_f32(w_pw, b_pw, w_dw, b_dw)
    _chk_act(x, z)
    n, h, w = x.shape[:3] if shape is None else shape
    cout = w_pw.shape[0]
    if z is None:
        z = torch.empty(n, h, w, cout, device=x.device, dtype=x.dtype) if shape is None else \
            torch.empty(n * (z_img_stride or h * w * cout), device=x.device, dtype=x.dtype)
    d = _dp_desc(x, w_pw, b_pw, w_dw, b_dw, z, in_bn, out_bn, x_img_stride, z_img_stride, shape)
    if pool:
        pooled = torch.empty(n, h // 2, w // 2, cout, device=x.device, dtype=x.dtype)
        idx = torch.empty(n, h // 2, w // 2, cout, device=x.device, dtype=torch.uint8)
        d.pool_out, d.pool_idx = pooled.data_ptr(), idx.data_ptr()
    L.check(getattr(L.load(), 'yunet_dp_fwd' + _act(x)[1])(C.byref(d), _stream()), 'yunet_dp_fwd')
    return (z, pooled, idx) if pool else z


def dp_bwd(x, w_pw, b_pw, w_dw, b_dw, z, dy, in_bn=None, out_bn=None, dy_scale=None,
           dx=None, accumulate_dx=False, z_img_stride=None, need_dx=True, pool_idx=None, partials=None,
           x_img_stride=None, shape=None):
    """ConvDPUnit backward.  x, z: saved activations (fp32 or bf16); dy, dx fp32.
    Returns (dx, d_w_pw, d_b_pw, d_w_dw, d_b_dw).
    pool_idx (the idx of dp_fwd(..., pool=True)): dy is the POOLED gradient [N,H/2,W/2,cout] -- the dx
    the pool's consumer wrote -- and reaches the recorded window positions while the tile is staged.
    partials: a [dp_grid(...), dp_row_width(...)] fp32 buffer for the per-workgroup weight-gradient rows (default: a fresh one).
    need_dx=False: YunetDP.dx = NULL (no input gradient, and in_bn.bstats is left alone).
    shape = (N, H, W): x, z, dy and dx are flat buffers -- x and dx with x_img_stride elements between images, z and dy
    with z_img_stride (a pooled dy stays dense); dx defaults to a fresh flat buffer of N * x_img_stride elements."""
    _chk_f32(w_pw, b_pw, w_dw, b_dw, dy)
    _chk_act(x)
    n, h, w = x.shape[:3] if shape is None else shape
    cout, cin = w_pw.shape[0], w_pw.shape[1]
    if dx is None and need_dx:
        dx = torch.empty(x.shape, device=x.device, dtype=torch.float32) if shape is None else \
            torch.empty(n * (x_img_stride or h * w * cin), device=x.device, dtype=torch.float32)
    d = _dp_desc(x, w_pw, b_pw, w_dw, b_dw, z, in_bn, out_bn, x_img_stride, z_img_stride, shape)
    strided = shape is not None or x_img_stride is not None or z_img_stride is not None
    if dx is not None:
        _chk_f32(dx)
        if strided:
            _chk_strided(dx, n, d.x_img_stride, h * w * cin, 'dx')
    if strided and pool_idx is None:
        _chk_strided(dy, n, d.z_img_stride, h * w * cout, 'dy')
    d.dy = dy.data_ptr()
    d.dy_scale = dy_scale.data_ptr() if dy_scale is not None else None
    d.dx = dx.data_ptr() if dx is not None else None
    d.accumulate_dx = int(accumulate_dx)
    if pool_idx is not None:
        assert pool_idx.dtype == torch.uint8 and tuple(pool_idx.shape) == (n, h // 2, w // 2, cout)
        assert tuple(dy.shape) == (n, h // 2, w // 2, cout)
        d.pool_idx = pool_idx.data_ptr()
    blocks = dp_grid(n, h, w, cin, cout)
    width = dp_row_width(cin, cout)
    part = torch.empty(blocks, width, device=x.device, dtype=torch.float32) if partials is None else partials
    assert tuple(part.shape) == (blocks, width) and part.dtype == torch.float32 and part.is_contiguous()
    d.wgrad_partials, d.wgrad_blocks = part.data_ptr(), blocks
    if z.dtype != x.dtype:
        d.z_dtype = d.x_dtype          # heads: z (the fp32 flat) is never read in backward
    L.check(getattr(L.load(), 'yunet_dp_bwd' + _act(x)[1])(C.byref(d), _stream()), 'yunet_dp_bwd')
    out = torch.empty(width, device=x.device, dtype=torch.float32)
    reduce_partials(part, out)
    o1, o2, o3 = cout * cin, cout * cin + cout, cout * cin + cout + cout * 9
    return (dx, out[:o1].view(cout, cin, 1, 1), out[o1:o2], out[o2:o3].view(cout, 1, 3, 3),
            out[o3:])


def pool_fwd(z, bn):
    n, h, w, c = z.shape
    out = torch.empty(n, h // 2, w // 2, c, device=z.device, dtype=z.dtype)
    bnc = bn.c()
    L.check(getattr(L.load(), 'yunet_pool_fwd' + _act(z)[1])(_p(z), C.byref(bnc), _p(out), n, h, w, c, _stream()),
            'yunet_pool_fwd')
    return out


def pool_bwd(z, bn, dy_out, dx=None, accumulate=False, extra=None):
    """max_pool2d backward through relu(bn(z)); `extra`: a full-size gradient of the same activation added under the
    same mask (yunet_pool_bwd_add: the TFPN merge's share of a pyramid tap)."""
    n, h, w, c = z.shape
    if dx is None:
        dx = torch.empty(z.shape, device=z.device, dtype=torch.float32)
    bnc = bn.c()
    L.check(getattr(L.load(), 'yunet_pool_bwd_add' + _act(z)[1])(
        _p(z), C.byref(bnc), _p(dy_out), _p(extra) if extra is not None else None, _p(dx), int(accumulate),
        n, h, w, c, _stream()), 'yunet_pool_bwd_add')
    return dx


def upadd_fwd(za, bna, zb, bnb):
    n, h, w, c = za.shape
    out = torch.empty_like(za)
    a, b = bna.c(), bnb.c()
    L.check(getattr(L.load(), 'yunet_upadd_fwd' + _act(za)[1])(_p(za), C.byref(a), _p(zb), C.byref(b), _p(out), n, h,
                                                               w, c, _stream()), 'yunet_upadd_fwd')
    return out


def upadd_bwd(za, bna, zb, bnb, dout, dxa=None, acc_a=False, dxb=None, acc_b=False, skip_a=False):
    """skip_a: the fine tensor's share is left to pool_bwd(extra=dout) -- returns (None, dxb)."""
    n, h, w, c = za.shape
    if not skip_a:
        dxa = torch.empty(za.shape, device=za.device, dtype=torch.float32) if dxa is None else dxa
    dxb = torch.empty(zb.shape, device=zb.device, dtype=torch.float32) if dxb is None else dxb
    a, b = bna.c(), bnb.c()
    L.check(getattr(L.load(), 'yunet_upadd_bwd' + _act(za)[1])(_p(za), C.byref(a), _p(zb), C.byref(b), _p(dout),
                                                               None if skip_a else _p(dxa), int(acc_a), _p(dxb),
                                                               int(acc_b), n, h, w, c, _stream()), 'yunet_upadd_bwd')
    return (None if skip_a else dxa), dxb


def add(a, b, out=None):
    """out = a + b (yunet_add): the merge of the two tower head outputs (YuNet_Head(stacked_convs > 0))."""
    _chk_f32(a, b)
    out = torch.empty_like(a) if out is None else out
    L.check(L.load().yunet_add(_p(a), _p(b), _p(out), a.numel(), _stream()), 'yunet_add')
    return out


def bn_update_running(stats, running_mean, running_var, count, momentum=0.1):
    L.check(L.load().yunet_bn_update_running(_p(stats), _p(running_mean), _p(running_var),
                                             running_mean.numel(), int(count), float(momentum),
                                             _stream()), 'yunet_bn_update_running')


def bn_param_grad(bstats, dgamma, dbeta, accumulate=False):
    L.check(L.load().yunet_bn_param_grad(_p(bstats), _p(dgamma), _p(dbeta), dgamma.numel(),
                                         int(accumulate), _stream()), 'yunet_bn_param_grad')


def make_levels(sizes, strides):
    lv = L.YunetLevels()
    lv.num_levels = len(sizes)
    for i, ((h, w), s) in enumerate(zip(sizes, strides)):
        lv.h[i], lv.w[i], lv.stride[i] = int(h), int(w), int(s)
    return lv


SOFT_NMS_METHODS = {'naive': L.SOFTNMS_NAIVE, 'linear': L.SOFTNMS_LINEAR, 'gaussian': L.SOFTNMS_GAUSSIAN}


def make_soft_nms(iou_thr=0.3, sigma=0.5, min_score=1e-3, method='linear'):
    """-> YunetSoftNms (mmcv.ops.soft_nms's values and defaults; method by name)."""
    if method not in SOFT_NMS_METHODS:
        raise ValueError(f'soft_nms method {method!r}: one of {sorted(SOFT_NMS_METHODS)}')
    return L.YunetSoftNms(SOFT_NMS_METHODS[method], float(iou_thr), float(sigma), float(min_score))


def detect(flat, sizes, strides, score_thr=0.02, iou_thr=0.45, max_out=None, with_kps=True, soft=None):
    """flat [N,P,16] raw head outputs -> (dets [N,max_out,5], kps [N,max_out,10] or None, count [N]).
    Rows at or beyond count[i] are unspecified.  soft = dict(iou_thr, sigma, min_score, method) (any subset; defaults of
    make_soft_nms) runs Soft-NMS in place of the greedy sweep (yunet_detect_soft; iou_thr is then the dict's)."""
    _chk_f32(flat)
    cfg = None if soft is None else make_soft_nms(**soft)
    n, p = flat.shape[0], flat.shape[1]
    max_out = p if max_out is None or max_out < 0 else int(max_out)
    dev = flat.device
    dets = torch.empty(n, max_out, 5, device=dev, dtype=torch.float32)
    kps = torch.empty(n, max_out, 10, device=dev, dtype=torch.float32) if with_kps else None
    count = torch.empty(n, device=dev, dtype=torch.int32)
    scratch = torch.empty(int(L.load().yunet_detect_scratch_bytes(n, p)), device=dev, dtype=torch.uint8)
    lv = make_levels(sizes, strides)
    if cfg is None:
        L.check(L.load().yunet_detect(_p(flat), C.byref(lv), n, p, float(score_thr), float(iou_thr), max_out,
                                      _p(dets), _p(kps) if with_kps else None, _p(count), _p(scratch), _stream()),
                'yunet_detect')
    else:
        L.check(L.load().yunet_detect_soft(_p(flat), C.byref(lv), n, p, float(score_thr), C.byref(cfg), max_out,
                                           _p(dets), _p(kps) if with_kps else None, _p(count), _p(scratch), _stream()),
                'yunet_detect_soft')
    return dets, kps, count


def rescale_dets(dets, kps, count, scale_factor):
    """get_bboxes(rescale=True) of a batch, in place (yunet_rescale_dets): dets [N,M,5] rows below count[n] divided by
    scale_factor[n] ([N,4] fp32 on the device), kps [N,M,10] (or None) by its first two entries."""
    _chk_f32(dets, kps, scale_factor)
    n, m = dets.shape[0], dets.shape[1]
    assert kps is None or kps.shape[:2] == (n, m), 'kps: [N, M, 10] or None'
    assert scale_factor.shape == (n, 4) and count.dtype == torch.int32 and count.numel() == n
    L.check(L.load().yunet_rescale_dets(_p(dets), _p(kps) if kps is not None else None, _p(count), _p(scale_factor), n, m, _stream()),
            'yunet_rescale_dets')


def nms(boxes, scores, iou_thr=0.45, score_thr=float('-inf'), max_out=None, counts=None):
    """Greedy single-class NMS of explicit candidates: boxes [N,K,4], scores [N,K] (fp32 CUDA),
    optional counts [N] int32 -> (dets [N,max_out,5], keep [N,max_out] int32, count [N])."""
    _chk_f32(boxes, scores)
    n, k = scores.shape
    max_out = k if max_out is None or max_out < 0 else int(max_out)
    dev = boxes.device
    dets = torch.empty(n, max_out, 5, device=dev, dtype=torch.float32)
    keep = torch.empty(n, max_out, device=dev, dtype=torch.int32)
    count = torch.empty(n, device=dev, dtype=torch.int32)
    scratch = torch.empty(int(L.load().yunet_detect_scratch_bytes(n, k)), device=dev, dtype=torch.uint8)
    L.check(L.load().yunet_nms(_p(boxes), _p(scores), _p(counts), n, k, float(score_thr), float(iou_thr),
                               max_out, _p(dets), _p(keep), _p(count), _p(scratch), _stream()), 'yunet_nms')
    return dets, keep, count


def soft_nms(boxes, scores, iou_thr=0.3, sigma=0.5, min_score=1e-3, method='linear', score_thr=float('-inf'),
             max_out=None, counts=None):
    """Single-class Soft-NMS (mmcv.ops.soft_nms, offset 0) of explicit candidates: the arguments and results of nms();
    dets[..., 4] holds the decayed scores, non-increasing.  Exact score ties go to the lower index."""
    _chk_f32(boxes, scores)
    cfg = make_soft_nms(iou_thr, sigma, min_score, method)
    n, k = scores.shape
    max_out = k if max_out is None or max_out < 0 else int(max_out)
    dev = boxes.device
    dets = torch.empty(n, max_out, 5, device=dev, dtype=torch.float32)
    keep = torch.empty(n, max_out, device=dev, dtype=torch.int32)
    count = torch.empty(n, device=dev, dtype=torch.int32)
    scratch = torch.empty(int(L.load().yunet_detect_scratch_bytes(n, k)), device=dev, dtype=torch.uint8)
    L.check(L.load().yunet_soft_nms(_p(boxes), _p(scores), _p(counts), n, k, float(score_thr), C.byref(cfg),
                                    max_out, _p(dets), _p(keep), _p(count), _p(scratch), _stream()), 'yunet_soft_nms')
    return dets, keep, count


# csrc/score.hip: threads of a scoring workgroup (= rows of a prediction tile) and ground truths staged in LDS at a time
SCORE_BLOCK, SCORE_GT_CHUNK = L.SCORE_BLOCK, L.SCORE_GT_CHUNK


def _chk_table(t, dtype, rows, what):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.shape[0] == rows, f'{what}: {dtype} [{rows}, ...] on the GPU'


def _chk_offsets(off, n_img, total, what):
    assert off.is_cuda and off.dtype == torch.int64 and off.shape == (n_img + 1,), f'{what}: int64 [I + 1] on the GPU'
    assert 0 <= total < 2 ** 31, f'{what}: at most 2^31 - 1 rows'


def score_wider_match(pred, pred_off, gt, gt_off, iou_thresh=0.5):
    """The matching stage of the WIDER scorer (yunet_score_wider_match): pred [P,5] fp64 xywh+score, gt [G,4] fp64 xywh,
    int64 offsets [I+1] -> (best int32 [P] relative to the image's first box, hit uint8 [P], first int32 [G]: the first
    row of the image that hit the box, INT_MAX when none).  Rows of images without boxes are unspecified."""
    n_img, P, G = pred_off.numel() - 1, pred.shape[0], gt.shape[0]
    _chk_table(pred.view(-1, 5), torch.float64, P, 'pred')
    _chk_table(gt.view(-1, 4), torch.float64, G, 'gt')
    _chk_offsets(pred_off, n_img, P, 'pred_off')
    _chk_offsets(gt_off, n_img, G, 'gt_off')
    dev = pred.device
    best = torch.empty(P, device=dev, dtype=torch.int32)
    hit = torch.empty(P, device=dev, dtype=torch.uint8)
    first = torch.empty(G, device=dev, dtype=torch.int32)
    L.check(L.load().yunet_score_wider_match(_p(pred), _p(pred_off), _p(gt), _p(gt_off), n_img, P, G, float(iou_thresh),
                                             _p(best), _p(hit), _p(first), _stream()), 'yunet_score_wider_match')
    return best, hit, first


def score_wider(pred, pred_off, gt, gt_off, gt_bits, thr, iou_thresh=0.5):
    """yunet_score_wider: the packed prediction / ground-truth set of the WIDER protocol (as score_wider_match, plus
    gt_bits uint8 [G] and the fp64 threshold table thr [T]) -> (counts int64 [3, T, 2], minmax fp64 [2]), on the device."""
    n_img, P, G, T = pred_off.numel() - 1, pred.shape[0], gt.shape[0], thr.numel()
    _chk_table(pred.view(-1, 5), torch.float64, P, 'pred')
    _chk_table(gt.view(-1, 4), torch.float64, G, 'gt')
    _chk_table(gt_bits, torch.uint8, G, 'gt_bits')
    _chk_table(thr, torch.float64, T, 'thr')
    _chk_offsets(pred_off, n_img, P, 'pred_off')
    _chk_offsets(gt_off, n_img, G, 'gt_off')
    assert 1 <= T <= L.SCORE_MAX_THRESH
    dev = pred.device
    best = torch.empty(P, device=dev, dtype=torch.int32)
    hit = torch.empty(P, device=dev, dtype=torch.uint8)
    first = torch.empty(G, device=dev, dtype=torch.int32)
    keys = torch.empty(2, device=dev, dtype=torch.int64)
    counts = torch.empty(3, T, 2, device=dev, dtype=torch.int64)          # (written as uint64; every count is < 2^63)
    minmax = torch.empty(2, device=dev, dtype=torch.float64)
    L.check(L.load().yunet_score_wider(_p(pred), _p(pred_off), _p(gt), _p(gt_off), _p(gt_bits), n_img, P, G,
                                       float(iou_thresh), _p(thr), T, _p(best), _p(hit), _p(first), _p(keys), _p(counts),
                                       _p(minmax), _stream()), 'yunet_score_wider')
    return counts, minmax


def score_map_tpfp(dets, det_off, gts, gt_off, kept, order, iou_thr):
    """yunet_score_map_tpfp: dets [D,5] fp32 xyxy+score, per image its kept then its ignored boxes in gts [G,4] fp32,
    kept int32 [I], order int32 [D] (per image: the row visited k-th) -> (tp, fp) fp32 [D] in row order.  iou_thr is
    compared as fp32."""
    n_img, D, G = det_off.numel() - 1, dets.shape[0], gts.shape[0]
    _chk_table(dets.view(-1, 5), torch.float32, D, 'dets')
    _chk_table(gts.view(-1, 4), torch.float32, G, 'gts')
    _chk_table(kept, torch.int32, n_img, 'kept')
    _chk_table(order, torch.int32, D, 'order')
    _chk_offsets(det_off, n_img, D, 'det_off')
    _chk_offsets(gt_off, n_img, G, 'gt_off')
    dev = dets.device
    code = torch.empty(D, device=dev, dtype=torch.int32)
    first = torch.empty(G, device=dev, dtype=torch.int32)
    tp = torch.empty(D, device=dev, dtype=torch.float32)
    fp = torch.empty(D, device=dev, dtype=torch.float32)
    L.check(L.load().yunet_score_map_tpfp(_p(dets), _p(det_off), _p(gts), _p(gt_off), _p(kept), _p(order), n_img, D, G,
                                          float(iou_thr), _p(code), _p(first), _p(tp), _p(fp), _stream()),
            'yunet_score_map_tpfp')
    return tp, fp


# csrc/score.hip, ranking: rows of an image ranked in LDS at once, elements of a radix-sort / scan tile, and the first
# D the curve refuses
RANK_SEG_CAP, RANK_RADIX_TILE, RANK_CURVE_MAX = L.RANK_SEG_CAP, L.RANK_RADIX_TILE, L.RANK_CURVE_MAX


def _rank_scratch(D, dev):
    return torch.empty(int(L.load().yunet_score_rank_scratch_bytes(D)), device=dev, dtype=torch.uint8)


def score_rank_images(dets, det_off):
    """yunet_score_rank_images: dets [D,5] fp32, det_off int64 [I+1] -> order int32 [D] as score_map_tpfp takes it (per
    image: the row visited k-th; descending score, ties by ascending row = np.argsort(-s, kind='stable'))."""
    n_img, D = det_off.numel() - 1, dets.shape[0]
    _chk_table(dets.view(-1, 5), torch.float32, D, 'dets')
    _chk_offsets(det_off, n_img, D, 'det_off')
    order = torch.empty(D, device=dets.device, dtype=torch.int32)
    L.check(L.load().yunet_score_rank_images(_p(dets), _p(det_off), n_img, D, _p(order), _stream()),
            'yunet_score_rank_images')
    return order


def score_rank_global(dets):
    """yunet_score_rank_global: dets [D,5] fp32 -> rank int32 [D], the stable descending order of all scores (ties in row
    order = np.argsort(-s, kind='stable'))."""
    D = dets.shape[0]
    _chk_table(dets.view(-1, 5), torch.float32, D, 'dets')
    assert D < 2 ** 31, 'dets: at most 2^31 - 1 rows'
    rank = torch.empty(D, device=dets.device, dtype=torch.int32)
    scratch = _rank_scratch(D, dets.device)
    L.check(L.load().yunet_score_rank_global(_p(dets), D, _p(rank), _p(scratch), _stream()), 'yunet_score_rank_global')
    return rank


def score_map_curve(tp, fp, rank):
    """yunet_score_map_curve: tp, fp fp32 [D] in row order and rank int32 [D] -> fp32 [4, D] in ranked order: cumulative
    tp, cumulative fp, precision = ctp / max(ctp + cfp, eps) and its reverse running maximum.  D < RANK_CURVE_MAX."""
    D = rank.shape[0]
    _chk_table(tp, torch.float32, D, 'tp')
    _chk_table(fp, torch.float32, D, 'fp')
    _chk_table(rank, torch.int32, D, 'rank')
    assert D < RANK_CURVE_MAX, f'the curve takes fewer than {RANK_CURVE_MAX} rows (exact fp32 counts)'
    out = torch.empty(4, D, device=rank.device, dtype=torch.float32)
    scratch = _rank_scratch(D, rank.device)
    L.check(L.load().yunet_score_map_curve(_p(tp), _p(fp), _p(rank), D, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]),
                                           _p(scratch), _stream()), 'yunet_score_map_curve')
    return out


def box_loss_code(box_loss, mode=None):
    """YUNET_BOX_* of a loss class name of mmdet/models/losses/iou_loss.py (+ IoULoss's `mode`)."""
    if box_loss == 'IoULoss':
        try:
            return {'linear': L.BOX_IOU_LINEAR, 'square': L.BOX_IOU_SQUARE, 'log': L.BOX_IOU_LOG}[mode or 'log']
        except KeyError:
            raise ValueError(f"IoULoss mode {mode!r}: 'linear', 'square' or 'log'") from None
    table = {'EIoULoss': L.BOX_EIOU, 'DIoULoss': L.BOX_DIOU, 'GIoULoss': L.BOX_GIOU, 'CIoULoss': L.BOX_CIOU,
             'BoundedIoULoss': L.BOX_BOUNDED}
    if box_loss not in table:
        raise NotImplementedError(f'loss_bbox type {box_loss!r}: the fused loss kernel implements IoULoss, GIoULoss, '
                                  f'DIoULoss, CIoULoss, EIoULoss and BoundedIoULoss')
    return table[box_loss]


CLS_LOSSES = {'CrossEntropyLoss': L.CLS_BCE, 'VarifocalLoss': L.CLS_VARIFOCAL}
KPS_LOSSES = {'SmoothL1Loss': L.KPS_SMOOTH_L1, 'L1Loss': L.KPS_L1, 'MSELoss': L.KPS_MSE, 'BalancedL1Loss': L.KPS_BALANCED_L1}


def _term(name, spec, table):
    """(type name, parameters) of one loss term: a type name or a dict(type=..., **parameters); None = the default."""
    if spec is None:
        return next(iter(table)), {}
    spec = dict(type=spec) if isinstance(spec, str) else dict(spec)
    kind = spec.pop('type')
    if kind not in table:
        raise NotImplementedError(f'{name} type {kind!r}: the fused loss kernel implements ' + ', '.join(table))
    if not spec.pop('use_sigmoid', True):
        raise NotImplementedError(f'{name}: use_sigmoid=False (the head predicts one sigmoid score per prior)')
    return kind, spec


def _varifocal(name, par):
    alpha, gamma = float(par.get('alpha', 0.75)), float(par.get('gamma', 2.0))
    if not alpha >= 0.0:
        raise ValueError(f'{name}: VarifocalLoss alpha={alpha} must be >= 0')
    if not gamma >= 1.0:
        raise ValueError(f'{name}: VarifocalLoss gamma={gamma} must be >= 1 (the derivative of |sigmoid(x) - t|^gamma '
                         'is unbounded at sigmoid(x) = t below 1)')
    return alpha, gamma, int(bool(par.get('iou_weighted', True)))


def make_loss_terms(loss_cls=None, loss_obj=None, loss_kps=None):
    """YunetLossTerms of the three terms that have a choice beside loss_bbox.  Each is None (the default: CrossEntropyLoss /
    CrossEntropyLoss / SmoothL1Loss), a type name, or dict(type=..., alpha=, gamma=, iou_weighted=) with the reference
    constructors' defaults.  BalancedL1Loss / SmoothL1Loss take their beta from make_loss_cfg's kps_beta."""
    t = L.YunetLossTerms()
    for name, spec in (('loss_cls', loss_cls), ('loss_obj', loss_obj)):
        kind, par = _term(name, spec, CLS_LOSSES)
        setattr(t, name[5:] + '_loss', CLS_LOSSES[kind])
        if kind == 'VarifocalLoss':
            a, g, w = _varifocal(name, par)
            setattr(t, name[5:] + '_alpha', a)
            setattr(t, name[5:] + '_gamma', g)
            setattr(t, name[5:] + '_iou_weighted', w)
    kind, par = _term('loss_kps', loss_kps, KPS_LOSSES)
    t.kps_loss = KPS_LOSSES[kind]
    if kind == 'BalancedL1Loss':
        t.kps_alpha, t.kps_gamma = float(par.get('alpha', 0.5)), float(par.get('gamma', 1.5))
        if not t.kps_alpha > 0.0 or not t.kps_gamma > 0.0:
            raise ValueError(f'loss_kps: BalancedL1Loss alpha={t.kps_alpha}, gamma={t.kps_gamma} must be > 0')
    return t


def make_loss_cfg(box_loss='EIoULoss', w_cls=1.0, w_box=5.0, w_obj=1.0, w_kps=0.1,
                  box_eps=1e-6, smooth_point=0.1, kps_beta=1.0 / 9.0, box_mode=None, terms=None):
    """-> YunetLossCfg.  BoundedIoULoss: box_eps = its eps, smooth_point = its beta.  `terms` (a YunetLossTerms of
    make_loss_terms) rides on the returned object as `.terms` for `loss()` / the engine; None = the default terms."""
    c = L.YunetLossCfg()
    c.box_loss = box_loss_code(box_loss, box_mode)
    c.w_cls, c.w_box, c.w_obj, c.w_kps = w_cls, w_box, w_obj, w_kps
    c.box_eps, c.smooth_point, c.kps_beta = box_eps, smooth_point, kps_beta
    if c.box_loss == L.BOX_BOUNDED and not c.smooth_point > 0.0:
        raise ValueError(f'loss_bbox: BoundedIoULoss beta={smooth_point} must be > 0')
    if terms is not None and terms.kps_loss in (L.KPS_SMOOTH_L1, L.KPS_BALANCED_L1) and not c.kps_beta > 0.0:
        raise ValueError(f'loss_kps: beta={kps_beta} must be > 0')
    c.terms = terms
    return c


def assign(flat, gt_boxes, gt_kps, gt_count, sizes, strides, center_radius=2.5, gt_labels=None,
           want_labels=False, pre_scores=None, pre_boxes=None, candidate_topk=10, iou_weight=3.0, cls_weight=1.0):
    """flat [N,P,16]; gt_boxes [N,Gmax,4]; gt_kps [N,Gmax,5,3]; gt_count [N] int32.
    -> gt_inds [N,P] int32, max_overlaps [N,P], img_stats [N,2], labels or None.
    candidate_topk / iou_weight / cls_weight: SimOTAAssigner's constructor arguments (1 <= candidate_topk <= 16)."""
    _chk_f32(flat, gt_boxes, gt_kps, pre_scores, pre_boxes)
    n, p = (flat.shape[0], flat.shape[1]) if flat is not None else pre_scores.shape
    gmax = gt_boxes.shape[1]
    dev = gt_boxes.device
    gt_inds = torch.empty(n, p, device=dev, dtype=torch.int32)
    ovl = torch.empty(n, p, device=dev, dtype=torch.float32)
    labels = torch.empty(n, p, device=dev, dtype=torch.int32) if want_labels else None
    img_stats = torch.empty(n, 2, device=dev, dtype=torch.float32)
    scratch = torch.empty(n, p, 12, device=dev, dtype=torch.float32)
    lv = make_levels(sizes, strides)
    cfg = L.YunetAssignCfg(float(center_radius), int(candidate_topk), float(iou_weight), float(cls_weight))
    L.check(L.load().yunet_assign_cfg(_p(flat), _p(pre_scores), _p(pre_boxes), _p(gt_boxes),
                                      _p(gt_kps), _p(gt_labels), _p(gt_count), C.byref(lv), n, p,
                                      gmax, C.byref(cfg), _p(gt_inds), _p(labels), _p(ovl),
                                      _p(img_stats), _p(scratch), _stream()), 'yunet_assign')
    return gt_inds, ovl, img_stats, labels


def loss_norm(img_stats, inv_world=1.0):
    norm = torch.empty(4, device=img_stats.device, dtype=torch.float32)
    L.check(L.load().yunet_loss_norm(_p(img_stats), img_stats.shape[0], float(inv_world), _p(norm),
                                     _stream()), 'yunet_loss_norm')
    return norm


def ignore_capacity_rows(capacity):
    """Rows per image of the padded ignore boxes: the smallest power of two >= max(capacity, 16), at most 1024."""
    rows = L.IGNORE_MIN_ROWS
    while rows < min(int(capacity), L.IGNORE_MAX_BOXES):
        rows *= 2
    return rows


def ignore_mark(gt_inds, ign_boxes, ign_count, sizes, strides, thr, n_marked=None):
    """gt_inds [N,P] int32, IN PLACE: background priors (0) whose cell [x, y, x+s, y+s] is covered by an ignore box to a
    share > thr (strict, thr >= 0) become -1; positives stay.  ign_boxes [N,Imax,4] fp32 xyxy, ign_count [N] int32 (rows
    beyond an image's count are not read); n_marked: an [N] int32 tensor to receive the marks per image.  -> gt_inds."""
    _chk_f32(ign_boxes)
    n, p = gt_inds.shape
    if (gt_inds.dtype != torch.int32 or not gt_inds.is_contiguous() or ign_boxes.dim() != 3 or ign_boxes.shape[0] != n or
            ign_boxes.shape[2] != 4 or not ign_boxes.is_contiguous() or ign_count.dtype != torch.int32 or
            ign_count.numel() != n or not ign_count.is_contiguous()):
        raise ValueError('ignore_mark: gt_inds [N,P] int32, ign_boxes [N,Imax,4] fp32, ign_count [N] int32, all contiguous')
    if n_marked is not None and (n_marked.dtype != torch.int32 or n_marked.numel() != n or not n_marked.is_contiguous()):
        raise ValueError('ignore_mark: n_marked must be a contiguous int32 [N] tensor')
    if not float(thr) >= 0.0:
        raise ValueError(f'ignore_mark: thr={thr} must be >= 0 (a negative ignore_iof_thr means off: launch nothing)')
    lv = make_levels(sizes, strides)
    L.check(L.load().yunet_ignore_mark(_p(ign_boxes), _p(ign_count), C.byref(lv), n, p, ign_boxes.shape[1], float(thr),
                                       _p(gt_inds), _p(n_marked), _stream()), 'yunet_ignore_mark')
    return gt_inds


def loss(flat, gt_inds, ovl, gt_boxes, gt_kps, img_stats, sizes, strides, cfg, inv_world=1.0,
         norm=None, grad=True, partials=None, ignore=False):
    """-> (losses [4] = cls,bbox,obj,kps ; dflat [N,P,16] ; norm [3]).
    grad=False: losses alone -- the kernel's value-only instance runs, no dflat is allocated and None stands in its place.
    partials: a [yunet_loss_blocks(N, P), 4] fp32 tensor to receive the per-block rows (default: a temporary).
    ignore=True: the kernel instances that keep priors with gt_inds < 0 (ignore_mark) out of loss_obj."""
    n, p, _ = flat.shape
    gmax = gt_boxes.shape[1]
    dev = flat.device
    lib = L.load()
    if norm is None:
        norm = loss_norm(img_stats, inv_world)
    blocks = lib.yunet_loss_blocks(n, p)
    part = partials if partials is not None else torch.empty(blocks, 4, device=dev, dtype=torch.float32)
    if tuple(part.shape) != (blocks, 4) or part.dtype != torch.float32 or not part.is_contiguous() or part.device != dev:
        raise ValueError(f'partials must be a contiguous fp32 [{blocks}, 4] tensor on {dev}')
    dflat = torch.empty_like(flat) if grad else None
    lv = make_levels(sizes, strides)
    terms = getattr(cfg, 'terms', None)               # None: the default terms, which yunet_loss_terms hands to yunet_loss
    if ignore:
        L.check(lib.yunet_loss_terms_ex(_p(flat), _p(gt_inds), _p(ovl), _p(gt_boxes), _p(gt_kps), C.byref(lv),
                                        C.byref(cfg), None if terms is None else C.byref(terms), L.LOSS_IGNORE, _p(norm), n, p,
                                        gmax, _p(dflat), _p(part), blocks, _stream()), 'yunet_loss_terms_ex')
    else:
        L.check(lib.yunet_loss_terms(_p(flat), _p(gt_inds), _p(ovl), _p(gt_boxes), _p(gt_kps), C.byref(lv),
                                     C.byref(cfg), None if terms is None else C.byref(terms), _p(norm), n, p, gmax, _p(dflat),
                                     _p(part), blocks, _stream()), 'yunet_loss_terms')
    losses = torch.empty(5, device=dev, dtype=torch.float32)      # cls, bbox, obj, kps, total
    L.check(lib.yunet_loss_finalize(_p(part), blocks, _p(losses), None, _stream()), 'yunet_loss_finalize')
    return losses[:4], dflat, norm


def sgd_step(params, grads, buf, lr_dev, momentum, weight_decay, grad_scale=1.0, first=False, dampening=0.0,
             nesterov=False):
    """torch.optim.SGD's update over one flat buffer (yunet_sgd_step_ex)."""
    L.check(L.load().yunet_sgd_step_ex(_p(params), _p(grads), _p(buf), params.numel(), _p(lr_dev),
                                       float(momentum), float(dampening), int(bool(nesterov)), float(weight_decay),
                                       float(grad_scale), int(first), _stream()), 'yunet_sgd_step_ex')


NORM_TYPES = {2: L.NORM_L2, 1: L.NORM_L1, float('inf'): L.NORM_INF}


def norm_type_code(norm_type):
    """clip_grad_norm_'s norm_type -> YUNET_NORM_*; anything but 1, 2 and inf is refused here, on the host."""
    try:
        key = float(norm_type)
    except (TypeError, ValueError):
        key = None
    if key not in NORM_TYPES:
        raise ValueError(f'grad_clip: norm_type {norm_type!r} is not implemented on the device (only 1, 2 and inf are: '
                         'one pass of sums or maxima over the flat gradient)')
    return NORM_TYPES[key]


def grad_norm_scratch(device):
    """The zeroed scratch yunet_grad_norm needs once; its launches keep it ready for the next one."""
    return torch.zeros(L.NORM_SCRATCH_BYTES // 8, device=device, dtype=torch.float64)


def grad_norm(grads, max_norm, norm_type=2, grad_scale=1.0, scratch=None, out=None):
    """out[0] = ||grads * grad_scale||_p, out[1] = min(1, max_norm / (out[0] + 1e-6)) in one launch, no host sync
    (yunet_grad_norm).  `grads`: any contiguous run of fp32 elements (4-byte aligned is enough)."""
    _chk_f32(grads)
    code = norm_type_code(norm_type)
    if scratch is None:
        scratch = grad_norm_scratch(grads.device)
    if out is None:
        out = torch.empty(2, device=grads.device, dtype=torch.float32)
    assert scratch.is_cuda and scratch.numel() * scratch.element_size() >= L.NORM_SCRATCH_BYTES
    _chk_f32(out)
    L.check(L.load().yunet_grad_norm(_p(grads), grads.numel(), float(grad_scale), code, float(max_norm), _p(scratch),
                                     _p(out), _stream()), 'yunet_grad_norm')
    return out


def _chk_groups(params, group_of, table):
    assert group_of.is_cuda and group_of.dtype == torch.uint8 and group_of.is_contiguous() and \
        group_of.numel() == params.numel(), 'group map: one uint8 per parameter element'
    assert table.is_cuda and table.dtype == torch.float64 and table.is_contiguous() and table.dim() == 2 and \
        table.shape[1] == L.OPT_ROW and 1 <= table.shape[0] <= L.OPT_MAX_GROUPS, 'group table: [groups, 4] float64'


def sgd_step_grouped(params, grads, buf, group_of, table, grad_scale=1.0, clip_coef=None, first=False, dampening=0.0,
                     nesterov=False):
    """torch.optim.SGD over parameter groups: table rows {lr, weight_decay, momentum, -}, group_of[i] the row of element
    i; the gradient is multiplied by grad_scale * clip_coef[0] (a device float, None = 1)  (yunet_sgd_step_grouped)."""
    _chk_f32(params, grads, buf, clip_coef)
    _chk_groups(params, group_of, table)
    L.check(L.load().yunet_sgd_step_grouped(_p(params), _p(grads), _p(buf), params.numel(), _p(group_of), _p(table),
                                            table.shape[0], float(dampening), int(bool(nesterov)), float(grad_scale),
                                            _p(clip_coef), int(first), _stream()), 'yunet_sgd_step_grouped')


def adam_step_grouped(params, grads, exp_avg, exp_avg_sq, group_of, table, step, eps=1e-8, decoupled=False,
                      grad_scale=1.0, clip_coef=None):
    """torch.optim.Adam (decoupled=False) / AdamW (True) over parameter groups: table rows {lr, weight_decay, beta1,
    beta2}; `step` counts this update from 1  (yunet_adam_step_grouped)."""
    _chk_f32(params, grads, exp_avg, exp_avg_sq, clip_coef)
    _chk_groups(params, group_of, table)
    L.check(L.load().yunet_adam_step_grouped(_p(params), _p(grads), _p(exp_avg), _p(exp_avg_sq), params.numel(),
                                             _p(group_of), _p(table), table.shape[0], float(eps), int(bool(decoupled)),
                                             int(step), float(grad_scale), _p(clip_coef), _stream()),
            'yunet_adam_step_grouped')


ACCUM_MODES = {'save': L.ACCUM_SAVE, 'add': L.ACCUM_ADD}


def grad_accum(acc, grads, mode):
    """mode 'save': acc <- grads; 'add': grads <- acc + grads (one fp32 add per element), one launch on the current stream
    (yunet_grad_accum).  Contiguous fp32 runs of the same length, 4-byte aligned is enough; length 0 launches nothing."""
    if mode not in ACCUM_MODES:
        raise ValueError(f"grad_accum: mode {mode!r} is not 'save' or 'add'")
    _chk_f32(acc, grads)
    if acc.numel() != grads.numel():
        raise ValueError('grad_accum: acc and grads differ in size')
    L.check(L.load().yunet_grad_accum(_p(acc), _p(grads), grads.numel(), ACCUM_MODES[mode], _stream()), 'yunet_grad_accum')


def ema_coefficients(momentum):
    """(keep, m) of the EMA hooks: 1 - momentum in double, as the reference's python does, then both as fp32 -- what
    torch's  ema.mul_(1 - momentum).add_(src, alpha=momentum)  hands its fp32 kernels."""
    momentum = float(momentum)
    return C.c_float(1.0 - momentum).value, C.c_float(momentum).value


def ema_update(pairs, momentum):
    """ema <- ema * (1 - momentum) + momentum * src over up to three (src, ema) pairs of fp32 CUDA tensors (contiguous
    views of any offset), ONE launch on the current stream (yunet_ema_update)."""
    if not 1 <= len(pairs) <= L.EMA_MAX_SEGMENTS:
        raise ValueError(f'ema_update: 1..{L.EMA_MAX_SEGMENTS} segments, got {len(pairs)}')
    for s, e in pairs:
        _chk_f32(s, e)
        if s.numel() != e.numel():
            raise ValueError('ema_update: src and ema differ in size')
    k = len(pairs)
    src = (C.c_void_p * k)(*[s.data_ptr() for s, _ in pairs])
    ema = (C.c_void_p * k)(*[e.data_ptr() for _, e in pairs])
    n = (C.c_longlong * k)(*[s.numel() for s, _ in pairs])
    keep, m = ema_coefficients(momentum)
    L.check(L.load().yunet_ema_update(src, ema, n, k, keep, m, _stream()), 'yunet_ema_update')


def box_size_hist(boxes, counts, iteration, bin_count, bin_first, totals, spill):
    """One batch of GT boxes into the persistent (w, h) grid of YuNetSampleSizeStatisticsHook (yunet_box_size_hist):
    boxes [N, Gmax, 4] fp32 and counts [N] int32 on the device; bin_count / bin_first [(H + 1), (W + 1)] int64,
    totals [4] int64, spill [cap, 2] int64.  One launch on the current stream, no host sync."""
    _chk_f32(boxes)
    assert boxes.dim() == 3 and boxes.shape[2] == 4, 'boxes: [N, Gmax, 4]'
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == boxes.shape[0]
    for t in (bin_count, bin_first, totals, spill):
        assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous(), 'expected a contiguous int64 CUDA tensor'
    assert bin_count.shape == bin_first.shape and bin_count.dim() == 2 and totals.numel() == 4
    h1, w1 = bin_count.shape
    L.check(L.load().yunet_box_size_hist(_p(boxes), _p(counts), boxes.shape[0], boxes.shape[1], int(iteration), w1 - 1,
                                         h1 - 1, _p(bin_count), _p(bin_first), _p(totals), _p(spill),
                                         spill.shape[0], _stream()), 'yunet_box_size_hist')
