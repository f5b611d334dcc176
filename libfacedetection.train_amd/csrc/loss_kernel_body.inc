// loss_kernel_body.inc -- the body of the loss step's kernel, included once per instance by loss_step.hip:
//   loss_kernel        EXT = false: the default selection (sigmoid BCE | IoU family | sigmoid BCE | smooth-L1), nothing else;
//   loss_terms_kernel  EXT = true: adds the terms of YunetLossTerms `tm` and YUNET_BOX_BOUNDED, each chosen by a launch-uniform code.
// Text inclusion, not an inlined function: the default instance keeps its pointer arguments' __restrict__ as kernel arguments
// and compiles to the code it had before the second instance existed (profiles/loss_terms_codegen.txt).
// In scope: the kernel's arguments, `constexpr bool EXT`, `constexpr bool GRAD`, `constexpr bool IGN`, `tm`
// (YunetLossTerms) and `bal_b` (BalancedL1Loss's b).
// IGN = true (the *_ign instances, YUNET_LOSS_IGNORE): a prior with gt_inds < 0 adds nothing to the loss_obj partial and
// its dflat row is all zero; every other prior runs the same operations in the same order, so a launch with nothing
// marked writes the bytes of the IGN = false instance (profiles/ignore_codegen.txt: those compile to what they did).
// GRAD = false (loss_value_kernel, loss_terms_value_kernel: the validation step, dflat == NULL): the four float4 stores are
// not compiled, `o` and the derivative halves of the dual numbers are dead and leave the code.  The value half of every
// dual operation is the same sequence of single-rounded fp32 operations in both forms (-ffp-contract=off), so `acc` and
// the partial rows equal the gradient-writing instance's bit for bit.
    // cfg.defer_num_total: norm[0] (the all-reduced positives, possibly still in flight on another stream) is NOT
    // read: the cls / bbox / obj terms and their gradients leave this kernel un-normalised (x 1.0 is exact) and
    // loss_finalize_kernel applies 1 / max(num_total, 1) to the losses and hands it to the head backward as dy_scale
    const float num_total = cfg.defer_num_total ? 1.0f : fmaxf(norm[0], 1.0f);
    const float inv_total = 1.0f / num_total;
    const float kps_den = norm[1] + 1.1920928955078125e-07f;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const long long total = (long long)N * P;
    for (long long e = (long long)blockIdx.x * LOSS_THREADS + threadIdx.x; e < total;
         e += (long long)gridDim.x * LOSS_THREADS) {
        const int n = (int)(e / P), p = (int)(e - (long long)n * P);
        const float4* src = reinterpret_cast<const float4*>(flat + e * 16);
        float4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
        float o[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.0f;
        const int gi = gt_inds[e];
        const float t_obj = gi > 0 ? 1.0f : 0.0f;
        const float xo = q1.y;
        if (IGN && gi < 0) {
            // a prior yunet_ignore_mark put inside an ignore region: outside loss_obj, its whole dflat row stays 0
        } else if (EXT && tm.obj_loss == YUNET_CLS_VARIFOCAL) {
            float gv;
            acc[2] += varifocal(xo, t_obj, tm.obj_alpha, tm.obj_gamma, tm.obj_iou_weighted, &gv);
            o[5] = cfg.w_obj * gv * inv_total;
        } else {
            acc[2] += bce_logits(xo, t_obj);
            o[5] = cfg.w_obj * (sigmoidf_ref(xo) - t_obj) * inv_total;
        }
        if (gi > 0) {
            const int g = gi - 1;
            float px, py, s;
            prior_of(L, p, px, py, s);
            // cls: BCE with IoU soft target, positives only
            const float t = max_overlaps[e];
            if (EXT && tm.cls_loss == YUNET_CLS_VARIFOCAL) {
                float gv;
                acc[0] += varifocal(q0.x, t, tm.cls_alpha, tm.cls_gamma, tm.cls_iou_weighted, &gv);
                o[0] = cfg.w_cls * gv * inv_total;
            } else {
                acc[0] += bce_logits(q0.x, t);
                o[0] = cfg.w_cls * (sigmoidf_ref(q0.x) - t) * inv_total;
            }
            // box: decode as duals w.r.t. (dx, dy, dw, dh)
            D4 ddx = mk(q0.y), ddy = mk(q0.z), ddw = mk(q0.w), ddh = mk(q1.x);
            ddx.d[0] = 1.f; ddy.d[1] = 1.f; ddw.d[2] = 1.f; ddh.d[3] = 1.f;
            const D4 cx = dadd(dscale(ddx, s), px), cy = dadd(dscale(ddy, s), py);
            D4 ew = mk(expf(ddw.v)), eh = mk(expf(ddh.v));
            ew.d[2] = ew.v; eh.d[3] = eh.v;
            const D4 bw = dscale(ew, s), bh = dscale(eh, s);
            const D4 hx = dscale(bw, 0.5f), hy = dscale(bh, 0.5f);   // w/2 is exact
            const D4 x1 = cx - hx, y1 = cy - hy, x2 = cx + hx, y2 = cy + hy;
            const float* tb = gt_boxes + ((size_t)n * Gmax + g) * 4;
            D4 lb;
            if (EXT && cfg.box_loss == YUNET_BOX_BOUNDED)
                lb = bounded_iou(x1, y1, x2, y2, tb[0], tb[1], tb[2], tb[3], cfg.smooth_point, cfg.box_eps);
            else switch (cfg.box_loss) {      // uniform over the launch
                case YUNET_BOX_EIOU: lb = eiou(x1, y1, x2, y2, tb[0], tb[1], tb[2], tb[3], cfg.smooth_point, cfg.box_eps); break;
                case YUNET_BOX_DIOU: lb = diou(x1, y1, x2, y2, tb[0], tb[1], tb[2], tb[3], cfg.box_eps); break;
                case YUNET_BOX_GIOU: lb = giou(x1, y1, x2, y2, tb[0], tb[1], tb[2], tb[3], cfg.box_eps); break;
                case YUNET_BOX_CIOU: lb = ciou(x1, y1, x2, y2, tb[0], tb[1], tb[2], tb[3], cfg.box_eps); break;
                default: lb = iou_family(x1, y1, x2, y2, tb[0], tb[1], tb[2], tb[3], cfg.box_loss - YUNET_BOX_IOU_LINEAR, cfg.box_eps);
            }
            acc[1] += lb.v;
            // (d * w) * 1/num_total, in this order: with the deferred normaliser the last factor is applied by the head
            // backward (dy_scale) and the product must round the same way
            const float kb = cfg.w_box;
            o[1] = lb.d[0] * kb * inv_total; o[2] = lb.d[1] * kb * inv_total;
            o[3] = lb.d[2] * kb * inv_total; o[4] = lb.d[3] * kb * inv_total;
            // kps: smooth-L1 on (kps - prior_xy)/stride, weight = mean visibility
            const float* kp = gt_kps + ((size_t)n * Gmax + g) * 15;
            const float w = ((((kp[2] + kp[5]) + kp[8]) + kp[11]) + kp[14]) / 5.0f;
            const float pr[10] = {q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
            const float kk = cfg.w_kps / kps_den;
            float lk = 0.0f;
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                const float tgt = (kp[(j >> 1) * 3 + (j & 1)] - ((j & 1) ? py : px)) / s;
                const float d = pr[j] - tgt;
                const float ad = fabsf(d);
                if (EXT && tm.kps_loss != YUNET_KPS_SMOOTH_L1) {
                    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                    float lv, gv;
                    if (tm.kps_loss == YUNET_KPS_L1) {                       // l1_loss, smooth_l1_loss.py:36-52
                        lv = ad;
                        gv = sgn;
                    } else if (tm.kps_loss == YUNET_KPS_MSE) {               // F.mse_loss, mse_loss.py:9-12
                        lv = d * d;
                        gv = 2.0f * d;
                    } else {                                                 // balanced_l1_loss, balanced_l1_loss.py:13-53
                        const float al = tm.kps_alpha, ga = tm.kps_gamma, be = cfg.kps_beta, bd = bal_b * ad;
                        if (ad < be) {
                            const float lg = log1pf(bd / be);
                            lv = al / bal_b * (bd + 1.0f) * lg - al * ad;
                            // d/d|d|: alpha log(b |d| / beta + 1) + alpha (b |d| + 1) / (b |d| + beta) - alpha, the last two merged
                            gv = (al * lg + al * (1.0f - be) / (bd + be)) * sgn;
                        } else {
                            lv = (ga * ad + ga / bal_b) - al * be;
                            gv = ga * sgn;
                        }
                    }
                    lk += lv * w;
                    o[6 + j] = gv * w * kk;
                    continue;
                }
                const bool quad = ad < cfg.kps_beta;
                lk += (quad ? 0.5f * ad * ad / cfg.kps_beta : ad - 0.5f * cfg.kps_beta) * w;
                const float gsl = quad ? d / cfg.kps_beta : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
                o[6 + j] = gsl * w * kk;
            }
            acc[3] += lk;
        }
        if (GRAD) {
            float4* dst = reinterpret_cast<float4*>(dflat + e * 16);
            dst[0] = make_float4(o[0], o[1], o[2], o[3]);
            dst[1] = make_float4(o[4], o[5], o[6], o[7]);
            dst[2] = make_float4(o[8], o[9], o[10], o[11]);
            dst[3] = make_float4(o[12], o[13], o[14], o[15]);
        }
    }
    // deterministic block reduction -> one partial row per block
    __shared__ float s_p[LOSS_THREADS / 64][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float v = acc[k];
#pragma unroll
        for (int o2 = 32; o2 >= 1; o2 >>= 1) v += __shfl_xor(v, o2, 64);
        if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        float v = 0.0f;
        for (int w = 0; w < LOSS_THREADS / 64; ++w) v += s_p[w][threadIdx.x];
        // loss_i = weight * sum / normaliser
        const float wgt = threadIdx.x == 0 ? cfg.w_cls : threadIdx.x == 1 ? cfg.w_box
                          : threadIdx.x == 2 ? cfg.w_obj : cfg.w_kps;
        const float den = threadIdx.x == 3 ? kps_den : num_total;
        partials[blockIdx.x * 4 + threadIdx.x] = wgt * v / den;
    }
