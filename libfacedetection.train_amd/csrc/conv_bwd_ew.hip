// conv_bwd_ew.hip -- the backward kernels outside the ConvDPUnits (NHWC fp32 gradients): stem weight gradient,
// max_pool2d and upsample-add backward.  Gradient conventions as in conv_bwd.hip.
#include "common.h"
#include "bwd_grid.h"

namespace {

// ----------------------------------------------------------------------------- stem wgrad
__global__ __launch_bounds__(256) void stem_bwd_kernel(const float* __restrict__ img,
                                                       const act_t* __restrict__ z,
                                                       const float* __restrict__ dy, YunetBN bn,
                                                       float* __restrict__ partials, int N, int H,
                                                       int W) {
    constexpr int PH = 2 * SB_TH + 1;
    constexpr int PW4 = (2 * SB_TW + 8) / 4;            // aligned float4 per patch row
    constexpr int PWS = PW4 * 4 + 1;                    // odd LDS row stride
    constexpr int NLD = (3 * PH * PW4 + 255) / 256;
    constexpr int DZS = 20;
    constexpr int PATCH_F = ((3 * PH * PWS + 3) / 4) * 4;
    constexpr int DZT_F = SB_TH * SB_TW * DZS;
    constexpr int ALL_F = (PATCH_F + DZT_F) > 256 * 33 ? (PATCH_F + DZT_F) : 256 * 33;
    __shared__ __attribute__((aligned(16))) float s_all[ALL_F];
    float* s_patch = s_all;
    float* s_dzt = s_all + PATCH_F;
    __shared__ float s_k[4][16];
    const int tid = threadIdx.x;
    const int Ho = H / 2, Wo = W / 2;
    if (tid < 16) {
        const BNFold f = bn_fold(bn_bwd_coef(bn, 16, tid));     // dz = A dy + B z + D (common.h)
        s_k[0][tid] = f.a; s_k[1][tid] = f.b; s_k[2][tid] = f.dh; s_k[3][tid] = f.dl;
    }
    __syncthreads();
    const int lc4 = tid & 3;  // channel quad in the dz load phase
    float fa[4], fb[4], fdh[4], fdl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        fa[i] = s_k[0][lc4 * 4 + i]; fb[i] = s_k[1][lc4 * 4 + i];
        fdh[i] = s_k[2][lc4 * 4 + i]; fdl[i] = s_k[3][lc4 * 4 + i];
    }
    // role: 4 output-channel quads x 4 tap groups of 7; 16 pixel slices of 16 pixels
    const int role = tid & 15, slice = tid >> 4;
    const int cog = role & 3, tg = role >> 2;
    int toff[7];
    bool tok[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int t = tg * 7 + k;
        tok[k] = t < 27;
        const int tt = tok[k] ? t : 0;
        const int ci = tt / 9, ky = (tt % 9) / 3, kx = tt % 3;
        toff[k] = ci * PH * PWS + ky * PWS + kx + 3;   // patch col 0 = image col 2*x0 - 4
    }
    float4 acc[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = make_float4(0, 0, 0, 0);
    float4 accb = make_float4(0, 0, 0, 0);

    const int tiles_x = (Wo + SB_TW - 1) / SB_TW, tiles_y = (Ho + SB_TH - 1) / SB_TH;
    const int ntiles = N * tiles_x * tiles_y;
    for (int t = first_tile(); t < ntiles; t += gridDim.x) {
        const int n = t / (tiles_x * tiles_y);
        const int r = t - n * tiles_x * tiles_y;
        const int y0 = (r / tiles_x) * SB_TH, x0 = (r % tiles_x) * SB_TW;
        __syncthreads();
        {
            float4 ld[NLD];
#pragma unroll
            for (int k = 0; k < NLD; ++k) {
                const int i = tid + 256 * k;
                const int rowi = i / PW4, c4 = i - rowi * PW4;
                const int ci = rowi / PH, py = rowi - ci * PH;
                const int iy = 2 * y0 - 1 + py, ix = 2 * x0 - 4 + 4 * c4;
                ld[k] = make_float4(0, 0, 0, 0);
                if (rowi < 3 * PH && iy >= 0 && iy < H && ix >= 0 && ix + 3 < W)
                    ld[k] = *reinterpret_cast<const float4*>(img + (((size_t)n * 3 + ci) * H + iy) * W + ix);
                else if (rowi < 3 * PH && iy >= 0 && iy < H) {
                    const float* src = img + (((size_t)n * 3 + ci) * H + iy) * W;
                    if (ix + 0 >= 0 && ix + 0 < W) ld[k].x = src[ix + 0];
                    if (ix + 1 >= 0 && ix + 1 < W) ld[k].y = src[ix + 1];
                    if (ix + 2 >= 0 && ix + 2 < W) ld[k].z = src[ix + 2];
                    if (ix + 3 >= 0 && ix + 3 < W) ld[k].w = src[ix + 3];
                }
            }
#pragma unroll
            for (int k = 0; k < NLD; ++k) {
                const int i = tid + 256 * k;
                const int rowi = i / PW4, c4 = i - rowi * PW4;
                if (rowi < 3 * PH) {
                    float* dst = s_patch + rowi * PWS + 4 * c4;
                    dst[0] = ld[k].x; dst[1] = ld[k].y; dst[2] = ld[k].z; dst[3] = ld[k].w;
                }
            }
        }
        for (int q = tid; q < SB_TH * SB_TW * 4; q += 256) {
            const int pix = q >> 2;
            const int oy = y0 + pix / SB_TW, ox = x0 + pix % SB_TW;
            float4 v = make_float4(0, 0, 0, 0);
            if (oy < Ho && ox < Wo) {
                const size_t off = (((size_t)n * Ho + oy) * Wo + ox) * 16 + lc4 * 4;
                const float4 g4 = *reinterpret_cast<const float4*>(dy + off);
                const float4 z4 = act_ld4(z + off);
                v.x = bn_dz_folded(g4.x, z4.x, fa[0], fb[0], fdh[0], fdl[0]);
                v.y = bn_dz_folded(g4.y, z4.y, fa[1], fb[1], fdh[1], fdl[1]);
                v.z = bn_dz_folded(g4.z, z4.z, fa[2], fb[2], fdh[2], fdl[2]);
                v.w = bn_dz_folded(g4.w, z4.w, fa[3], fb[3], fdh[3], fdl[3]);
            }
            *reinterpret_cast<float4*>(s_dzt + pix * DZS + lc4 * 4) = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < 16; ++j) {
            const int pix = slice * 16 + j;
            const int ty = pix / SB_TW, tx = pix % SB_TW;
            const float4 dz = *reinterpret_cast<const float4*>(s_dzt + pix * DZS + cog * 4);
            const float* pb = s_patch + 2 * ty * PWS + 2 * tx;
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const float v = tok[k] ? pb[toff[k]] : 0.0f;
                acc[k].x = fmaf(v, dz.x, acc[k].x); acc[k].y = fmaf(v, dz.y, acc[k].y);
                acc[k].z = fmaf(v, dz.z, acc[k].z); acc[k].w = fmaf(v, dz.w, acc[k].w);
            }
            if (tg == 0) { accb.x += dz.x; accb.y += dz.y; accb.z += dz.z; accb.w += dz.w; }
        }
    }
    // reduce over the 16 pixel slices
    __syncthreads();
    float* red = s_all;  // [256][33], aliases the patch / dz tiles (all reads are done)
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        red[tid * 33 + k * 4 + 0] = acc[k].x; red[tid * 33 + k * 4 + 1] = acc[k].y;
        red[tid * 33 + k * 4 + 2] = acc[k].z; red[tid * 33 + k * 4 + 3] = acc[k].w;
    }
    red[tid * 33 + 28] = accb.x; red[tid * 33 + 29] = accb.y;
    red[tid * 33 + 30] = accb.z; red[tid * 33 + 31] = accb.w;
    __syncthreads();
    float* row = partials + (size_t)blockIdx.x * (16 * 27 + 16);
    for (int o = tid; o < 16 * 27 + 16; o += 256) {
        float v = 0.0f;
        if (o < 16 * 27) {
            const int co = o / 27, tt = o - co * 27;
            const int tgi = tt / 7, k = tt - tgi * 7;
            const int rl = tgi * 4 + (co >> 2);
            for (int s = 0; s < 16; ++s) v += red[(s * 16 + rl) * 33 + k * 4 + (co & 3)];
        } else {
            const int co = o - 16 * 27;
            const int rl = (co >> 2);  // tg == 0
            for (int s = 0; s < 16; ++s) v += red[(s * 16 + rl) * 33 + 28 + (co & 3)];
        }
        row[o] = v;
    }
}

// ------------------------------------------------------------------- pool / upsample-add
// `extra` (may be null): a second, FULL-SIZE gradient of the same activation y = relu(bn(z)) -- the share the
// upsample-add of the neck sends to a pyramid tap (dsum, identity branch).  Both shares pass the same ReLU mask and
// feed the same BatchNorm-backward sums, so dx = mask (extra + route(dy_out)) is written once here instead of
// upadd_bwd writing mask extra and this kernel re-reading z and read-modify-writing dx (engine.py: _upadd / _pool).
// (DET: the deterministic form of the sums' flush, common.h: bn_det_add; fp32 storage only)
template <bool DET = false>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const act_t* __restrict__ z, YunetBN bn,
                                                       const float* __restrict__ dyo,
                                                       const float* __restrict__ extra,
                                                       float* __restrict__ dx, int accumulate, int N,
                                                       int H, int W, int C) {
    const int C4 = C / 4, Ho = H / 2, Wo = W / 2;
    const long long total = (long long)N * Ho * Wo * C4;
    const int c4 = threadIdx.x % C4;
    __shared__ float s_tab[5 * 64];
    bn_table_fill(s_tab, bn, C, threadIdx.x);
    __syncthreads();
    BNCoef k[4];
    bn_table_get(s_tab, C, c4 * 4, k);
    double bst[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bst[i] = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total;
         e += (long long)gridDim.x * 256) {
        long long pix = e / C4;
        const int ox = (int)(pix % Wo);
        pix /= Wo;
        const int oy = (int)(pix % Ho), n = (int)(pix / Ho);
        const float4 g4 = *reinterpret_cast<const float4*>(dyo + e * 4);
        const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
        float zv[4][4], yv[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 v = act_ld4(z + (((size_t)n * H + 2 * oy + (j >> 1)) * W + 2 * ox + (j & 1)) * C + c4 * 4);
            zv[j][0] = v.x; zv[j][1] = v.y; zv[j][2] = v.z; zv[j][3] = v.w;
#pragma unroll
            for (int i = 0; i < 4; ++i) yv[j][i] = bnrelu(zv[j][i], k[i].mean, k[i].scale, k[i].beta);
        }
        float o[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int am = 0;
            float m = yv[0][i];
#pragma unroll
            for (int j = 1; j < 4; ++j)
                if (yv[j][i] > m) { m = yv[j][i]; am = j; }
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j][i] = (j == am && m > 0.0f) ? gv[i] : 0.0f;
            if (m > 0.0f) {
                bst[i] += (double)gv[i];
                bst[4 + i] += (double)(gv[i] * (bn_center(zv[am][i], k[i].mean, k[i].mean_lo) * k[i].invstd));
            }
        }
        if (extra) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 e4 = *reinterpret_cast<const float4*>(
                    extra + (((size_t)n * H + 2 * oy + (j >> 1)) * W + 2 * ox + (j & 1)) * C + c4 * 4);
                const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (yv[j][i] > 0.0f) {
                        o[j][i] += ev[i];
                        bst[i] += (double)ev[i];
                        bst[4 + i] += (double)(ev[i] * (bn_center(zv[j][i], k[i].mean, k[i].mean_lo) * k[i].invstd));
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float4* dst = reinterpret_cast<float4*>(
                dx + (((size_t)n * H + 2 * oy + (j >> 1)) * W + 2 * ox + (j & 1)) * C + c4 * 4);
            float4 v = make_float4(o[j][0], o[j][1], o[j][2], o[j][3]);
            if (accumulate) {
                const float4 p = *dst;
                v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
            }
            *dst = v;
        }
    }
    __shared__ double red[256 * 8];
#pragma unroll
    for (int i = 0; i < 8; ++i) red[threadIdx.x * 8 + i] = bst[i];
    __syncthreads();
    if ((int)threadIdx.x < 2 * C && bn.bstats) {
        const int which = threadIdx.x / C, c = threadIdx.x % C;
        const int q = c >> 2, kk = (c & 3) + 4 * which;
        double v = 0.0;
        for (int p = 0; p < 256 / C4; ++p) v += red[(p * C4 + q) * 8 + kk];
        if constexpr (DET) bn_det_add(bn.bstats, C, which * C + c, v);
        else atomic_add_f64(bn_slot(bn.bstats, bn.slots, C) + which * C + c, v);
    }
}

template <bool DET = false>
__global__ __launch_bounds__(256) void upadd_bwd_kernel(const act_t* __restrict__ za, YunetBN bna,
                                                        const act_t* __restrict__ zb, YunetBN bnb,
                                                        const float* __restrict__ dout,
                                                        float* __restrict__ dxa, int acc_a,
                                                        float* __restrict__ dxb, int acc_b, int N,
                                                        int H, int W, int C) {
    // one thread = one float4 of one COARSE pixel (covers the 2x2 fine pixels)
    const int C4 = C / 4, Hb = H / 2, Wb = W / 2;
    const long long total = (long long)N * Hb * Wb * C4;
    const int c4 = threadIdx.x % C4;
    __shared__ float s_ta[5 * 64], s_tb[5 * 64];
    if (dxa) bn_table_fill(s_ta, bna, C, threadIdx.x);          // (the fine tensor's BatchNorm is not needed without its share)
    bn_table_fill(s_tb, bnb, C, threadIdx.x);
    __syncthreads();
    BNCoef ka[4], kb[4];
    bn_table_get(dxa ? s_ta : s_tb, C, c4 * 4, ka);
    bn_table_get(s_tb, C, c4 * 4, kb);
    double bsa[8], bsb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bsa[i] = bsb[i] = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total;
         e += (long long)gridDim.x * 256) {
        long long pix = e / C4;
        const int bx = (int)(pix % Wb);
        pix /= Wb;
        const int by = (int)(pix % Hb), n = (int)(pix / Hb);
        float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t off = (((size_t)n * H + 2 * by + (j >> 1)) * W + 2 * bx + (j & 1)) * C + c4 * 4;
            const float4 g4 = *reinterpret_cast<const float4*>(dout + off);
            if (!dxa) {          // the fine tensor's share is applied by pool_bwd_kernel (extra): za is not read
                sum[0] += g4.x; sum[1] += g4.y; sum[2] += g4.z; sum[3] += g4.w;
                continue;
            }
            const float4 z4 = act_ld4(za + off);
            const float gv[4] = {g4.x, g4.y, g4.z, g4.w}, zv[4] = {z4.x, z4.y, z4.z, z4.w};
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sum[i] += gv[i];
                const bool on = bnrelu(zv[i], ka[i].mean, ka[i].scale, ka[i].beta) > 0.0f;
                o[i] = on ? gv[i] : 0.0f;
                if (on) {
                    bsa[i] += (double)gv[i];
                    bsa[4 + i] += (double)(gv[i] * (bn_center(zv[i], ka[i].mean, ka[i].mean_lo) * ka[i].invstd));
                }
            }
            float4* dst = reinterpret_cast<float4*>(dxa + off);
            float4 v = make_float4(o[0], o[1], o[2], o[3]);
            if (acc_a) {
                const float4 p = *dst;
                v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
            }
            *dst = v;
        }
        const size_t offb = (((size_t)n * Hb + by) * Wb + bx) * C + c4 * 4;
        const float4 zb4 = act_ld4(zb + offb);
        const float zbv[4] = {zb4.x, zb4.y, zb4.z, zb4.w};
        float ob[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool on = bnrelu(zbv[i], kb[i].mean, kb[i].scale, kb[i].beta) > 0.0f;
            ob[i] = on ? sum[i] : 0.0f;
            if (on) {
                bsb[i] += (double)sum[i];
                bsb[4 + i] += (double)(sum[i] * (bn_center(zbv[i], kb[i].mean, kb[i].mean_lo) * kb[i].invstd));
            }
        }
        float4* dstb = reinterpret_cast<float4*>(dxb + offb);
        float4 v = make_float4(ob[0], ob[1], ob[2], ob[3]);
        if (acc_b) {
            const float4 p = *dstb;
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        *dstb = v;
    }
    __shared__ double red[256 * 8];
#define UPADD_FLUSH(SRC, DST, SLOTS)                                                  \
    __syncthreads();                                                                 \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) red[threadIdx.x * 8 + i] = SRC[i]; \
    __syncthreads();                                                                 \
    if ((int)threadIdx.x < 2 * C && DST) {                                           \
        const int which = threadIdx.x / C, c = threadIdx.x % C;                      \
        const int q = c >> 2, kk = (c & 3) + 4 * which;                              \
        double v = 0.0;                                                              \
        for (int p = 0; p < 256 / C4; ++p) v += red[(p * C4 + q) * 8 + kk];          \
        if constexpr (DET) bn_det_add(DST, C, which * C + c, v);                     \
        else atomic_add_f64(bn_slot(DST, SLOTS, C) + which * C + c, v);              \
    }
    UPADD_FLUSH(bsa, (dxa ? bna.bstats : nullptr), bna.slots)
    UPADD_FLUSH(bsb, bnb.bstats, bnb.slots)
#undef UPADD_FLUSH
}

// The coarse gradient alone (dxa == NULL: the fine tensor's share of a pyramid tap is applied by pool_bwd_kernel,
// DESIGN 3): dxb = mask_b (sum of the 2 x 2 fine gradients) + the coarse BatchNorm's backward sums.  Round 5: the
// general kernel above compiled `if (on) sum += ...` of its 16 channel lanes into exec-mask branches around fp64 adds
// and separated a thread's four fine loads by them (3.3 TB/s); here the four loads + the coarse z are issued together
// and the mask is a select (adding the +0.0 of a masked-out element leaves every sum unchanged: same values, same
// order of additions as the general kernel).
template <bool DET = false>
__global__ __launch_bounds__(256) void upadd_bwd_coarse_kernel(const act_t* __restrict__ zb, YunetBN bnb,
                                                               const float* __restrict__ dout, float* __restrict__ dxb,
                                                               int acc_b, int N, int H, int W, int C) {
    const int C4 = C / 4, Hb = H / 2, Wb = W / 2;
    const long long total = (long long)N * Hb * Wb * C4;
    const int c4 = threadIdx.x % C4;
    __shared__ float s_tb[5 * 64];
    bn_table_fill(s_tb, bnb, C, threadIdx.x);
    __syncthreads();
    BNCoef kb[4];
    bn_table_get(s_tb, C, c4 * 4, kb);
    double bsb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bsb[i] = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        long long pix = e / C4;
        const int bx = (int)(pix % Wb);
        pix /= Wb;
        const int by = (int)(pix % Hb), n = (int)(pix / Hb);
        const size_t off0 = (((size_t)n * H + 2 * by) * W + 2 * bx) * C + c4 * 4;
        const size_t offb = (((size_t)n * Hb + by) * Wb + bx) * C + c4 * 4;
        const float4 g0 = *reinterpret_cast<const float4*>(dout + off0);
        const float4 g1 = *reinterpret_cast<const float4*>(dout + off0 + C);
        const float4 g2 = *reinterpret_cast<const float4*>(dout + off0 + (size_t)W * C);
        const float4 g3 = *reinterpret_cast<const float4*>(dout + off0 + (size_t)W * C + C);
        const float4 zb4 = act_ld4(zb + offb);
        float4 old = make_float4(0.f, 0.f, 0.f, 0.f);
        if (acc_b) old = *reinterpret_cast<const float4*>(dxb + offb);
        const float sum[4] = {((0.f + g0.x) + g1.x) + g2.x + g3.x, ((0.f + g0.y) + g1.y) + g2.y + g3.y,
                              ((0.f + g0.z) + g1.z) + g2.z + g3.z, ((0.f + g0.w) + g1.w) + g2.w + g3.w};
        const float zbv[4] = {zb4.x, zb4.y, zb4.z, zb4.w};
        float ob[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool on = bnrelu(zbv[i], kb[i].mean, kb[i].scale, kb[i].beta) > 0.0f;
            ob[i] = on ? sum[i] : 0.0f;
            const float xh = on ? bn_center(zbv[i], kb[i].mean, kb[i].mean_lo) * kb[i].invstd : 0.0f;
            bsb[i] += (double)ob[i];
            bsb[4 + i] += (double)(ob[i] * xh);
        }
        float4 v = make_float4(ob[0], ob[1], ob[2], ob[3]);
        if (acc_b) { v.x += old.x; v.y += old.y; v.z += old.z; v.w += old.w; }
        *reinterpret_cast<float4*>(dxb + offb) = v;
    }
    __shared__ double red[256 * 8];
#pragma unroll
    for (int i = 0; i < 8; ++i) red[threadIdx.x * 8 + i] = bsb[i];
    __syncthreads();
    if ((int)threadIdx.x < 2 * C && bnb.bstats) {
        const int which = threadIdx.x / C, c = threadIdx.x % C;
        const int q = c >> 2, kk = (c & 3) + 4 * which;
        double v = 0.0;
        for (int p = 0; p < 256 / C4; ++p) v += red[(p * C4 + q) * 8 + kk];
        if constexpr (DET) bn_det_add(bnb.bstats, C, which * C + c, v);
        else atomic_add_f64(bn_slot(bnb.bstats, bnb.slots, C) + which * C + c, v);
    }
}

}  // namespace

extern "C" int ACT_SUFFIX(yunet_stem_bwd)(const float* img, const float* z, const float* dy, const YunetBN* bn,
                                          float* wgrad_partials, int wgrad_blocks, int N, int H, int W, int cmid,
                                          void* stream) {
    if (cmid != 16 || (H & 1) || (W & 1) || wgrad_blocks != yunet_stem_bwd_blocks(N, H, W))
        return YUNET_EINVAL;
    const int tiles = N * ((W / 2 + SB_TW - 1) / SB_TW) * ((H / 2 + SB_TH - 1) / SB_TH);
    int grid = tiles < CONV_BLOCKS ? tiles : CONV_BLOCKS;
    if (grid > wgrad_blocks) grid = wgrad_blocks;
    hipLaunchKernelGGL(stem_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, img,
                       reinterpret_cast<const act_t*>(z), dy, *bn, wgrad_partials, N, H, W);
    return hip_status();
}

extern "C" int ACT_SUFFIX(yunet_pool_bwd_add)(const float* z, const YunetBN* bn, const float* dy_out, const float* extra,
                                              float* dx, int accumulate, int N, int H, int W, int C, void* stream) {
    if ((H & 1) || (W & 1) || (C & 3) || (256 % (C / 4)) || C > 64) return YUNET_EINVAL;
    const long long total = (long long)N * (H / 2) * (W / 2) * (C / 4);
    if (YUNET_DET_ROWS(bn->det_rows) && bn->bstats) {          // deterministic sums (include/yunet_hip.h): fp32 storage only
#ifndef YUNET_ACT_BF16
        if (!bn_det_fits(*bn, ew_grid(total))) return YUNET_EINVAL;
        hipLaunchKernelGGL(pool_bwd_kernel<true>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const act_t*>(z), *bn, dy_out, extra, dx, accumulate, N, H, W, C);
        return hip_status();
#else
        return YUNET_EINVAL;
#endif
    }
    hipLaunchKernelGGL(pool_bwd_kernel<false>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const act_t*>(z), *bn, dy_out, extra, dx, accumulate, N, H, W, C);
    return hip_status();
}

extern "C" int ACT_SUFFIX(yunet_pool_bwd)(const float* z, const YunetBN* bn, const float* dy_out, float* dx,
                                          int accumulate, int N, int H, int W, int C, void* stream) {
    return ACT_SUFFIX(yunet_pool_bwd_add)(z, bn, dy_out, nullptr, dx, accumulate, N, H, W, C, stream);
}

extern "C" int ACT_SUFFIX(yunet_upadd_bwd)(const float* za, const YunetBN* bna, const float* zb,
                                           const YunetBN* bnb, const float* dout, float* dxa, int accumulate_a,
                                           float* dxb, int accumulate_b, int N, int H, int W, int C,
                                           void* stream) {
    if ((H & 1) || (W & 1) || (C & 3) || (256 % (C / 4)) || C > 64) return YUNET_EINVAL;
    const long long total = (long long)N * (H / 2) * (W / 2) * (C / 4);
    if ((YUNET_DET_ROWS(bnb->det_rows) && bnb->bstats) || (dxa && YUNET_DET_ROWS(bna->det_rows) && bna->bstats)) {      // deterministic sums: both blocks or neither
#ifndef YUNET_ACT_BF16
        if (!bnb->bstats || !bn_det_fits(*bnb, ew_grid(total)) || (dxa && (!bna->bstats || !bn_det_fits(*bna, ew_grid(total)))))
            return YUNET_EINVAL;
        if (!dxa)
            hipLaunchKernelGGL(upadd_bwd_coarse_kernel<true>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream,
                               reinterpret_cast<const act_t*>(zb), *bnb, dout, dxb, accumulate_b, N, H, W, C);
        else
            hipLaunchKernelGGL(upadd_bwd_kernel<true>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream,
                               reinterpret_cast<const act_t*>(za), *bna, reinterpret_cast<const act_t*>(zb), *bnb, dout, dxa,
                               accumulate_a, dxb, accumulate_b, N, H, W, C);
        return hip_status();
#else
        return YUNET_EINVAL;
#endif
    }
    if (!dxa && yunet_options().upadd_coarse) {        // the coarse gradient alone: dedicated kernel (round 5)
        hipLaunchKernelGGL(upadd_bwd_coarse_kernel<false>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const act_t*>(zb), *bnb, dout, dxb, accumulate_b, N, H, W, C);
        return hip_status();
    }
    hipLaunchKernelGGL(upadd_bwd_kernel<false>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const act_t*>(za), *bna, reinterpret_cast<const act_t*>(zb), *bnb, dout, dxa,
                       accumulate_a, dxb, accumulate_b, N, H, W, C);
    return hip_status();
}
