// conv_bwd.hip -- backward of the ConvDPUnits on gfx950 (NHWC fp32): the generic tile kernel dp_bwd_kernel and the
// yunet_dp_bwd dispatcher.  The other families live next to it: conv_bwd64.hip (64 -> 64 units), conv_bwd16.hip (16 -> 16,
// z recomputed), conv_bwd_ew.hip (stem / pool / upsample-add), conv_bwd_host.hip (grid-size queries, reductions: compiled
// once); dp_bwd_parts.h and bwd_grid.h hold what they share.
//
// The reference gets these from autograd over F.conv2d / batch_norm / relu / max_pool2d /
// interpolate.  Gradient tensors exchanged between kernels are
// "grad w.r.t. the BatchNorm OUTPUT with the ReLU mask applied" (dy); the kernel that
// produces dy also accumulates the two BN-backward sums (sum dy, sum dy*xhat) in fp64, and
// the producer's backward turns dy into dz = k1*(dy - c1 - xhat*c2) while loading.
//
// dp_bwd per 8x16 tile (512 threads): dz halo -> LDS; a = T(x) -> LDS; p = a*W1^T+b1 (MFMA,
// recomputed, never stored in HBM); depthwise backward on the VALU (dp, dW2, db2, db1);
// dW1 += a^T * dp (MFMA, K = pixels, accumulators persistent across tiles);
// da = dp * W1 (MFMA); dx = da * relu-mask, BN-backward sums of the producer.
#include "common.h"
#include "dp_route.h"
#include "dp_bwd_parts.h"

#include <type_traits>

namespace {

#define BWD_THREADS 512
#define BWD_WAVES 8

// GEMM = 0: the three pointwise GEMMs on the exact-fp32 matrix instruction (v_mfma_f32_16x16x4_f32).
// GEMM = 1: split-bf16 -- every fp32 operand x is split on the fly into hi = bf16(x) and
//   lo = bf16(x - hi) (x = hi + lo to 2^-17 relative) and each product runs as the three bf16
//   MFMAs hi*hi + lo*hi + hi*lo with fp32 accumulation (v_mfma_f32_16x16x32_bf16: 16x the fp32
//   matrix rate, so 3/16 of the matrix time).  The dropped lo*lo term is <= 2^-18 relative: the
//   products carry ~1e-5 relative error instead of 6e-8.  Used for GRADIENTS only (backward of
//   the 64 -> 64 units); the forward pass stays on the exact instruction.
template <int CIN, int COUT, int TH, int TW, int GEMM = 0>
struct BwdGeom {
    static constexpr int HW_ = TW + 2, HH_ = TH + 2, HP = HH_ * HW_;
    static constexpr int IP = TH * TW, IMT = IP / 16;
    static constexpr int LSO = COUT + 4, LSI = CIN + 4, WS = CIN + 4, WST = COUT + 4;
    static constexpr int C4I = CIN / 4, C4O = COUT / 4;
    static constexpr int NTO = COUT / 16, NTI = CIN / 16;
    static constexpr int KSI = CIN / 4, KSO = COUT / 4;
    static constexpr int PG = BWD_THREADS / C4O;   // pixel groups of the VALU phase
    static constexpr int PPT = IP / PG;            // pixels (rows) per thread
    // dW1 (K = pixels): a wave owns MB x NB 16x16 tiles whose rows / columns are interleaved
    // (ci = MB*m + j, co = NB*n + i), so ONE MB-float and ONE NB-float LDS read feed MB*NB
    // MFMAs; the NGRP wave groups cover [CIN x COUT], the remaining waves split K
    static constexpr int MB = (NTI >= 2 && (NTI * NTO < 16 || GEMM == 1)) ? 2 : 1, NB = NTO >= 2 ? 2 : 1;
    static constexpr int NGRP = (NTI / MB) * (NTO / NB);
    static constexpr int KSPLIT = BWD_WAVES / NGRP;
    static constexpr int KSTEPS = (IP / 4) / KSPLIT;  // k-steps of 4 pixels per wave
    static constexpr int KPX = IP / KSPLIT;           // pixels of K per wave (dW1)
    static constexpr int NDZ = (HP * C4O + BWD_THREADS - 1) / BWD_THREADS;  // (dy,z) float4 pairs / thread
    static constexpr int NX = (IP * C4I) / BWD_THREADS;                       // x float4 / thread
    // LDS carve (floats)
    static constexpr int OFF_DZ = 0;
    static constexpr int OFF_A = OFF_DZ + HP * LSO;
    static constexpr int OFF_PB = OFF_A + IP * LSI;
    static constexpr int WORK_F = OFF_PB + IP * LSO;
    // GEMM = 1: W1 and W1^T as bf16 hi / lo planes, rows padded to WSB / WSTB elements
    static constexpr int WSB = CIN + 8, WSTB = COUT + 8;
    static constexpr int W1_F = GEMM ? (2 * COUT * WSB) / 2 + COUT : COUT * WS;     // (+ bias row)
    static constexpr int W1T_F = GEMM ? (2 * CIN * WSTB) / 2 : CIN * WST;
    static constexpr int PAR_F = W1_F + 9 * COUT + 7 * COUT + 5 * CIN + W1T_F + 4 * CIN + IP / 4;   // w1 | w2 | out-bn | in-bn | w1^T | fp64 sums | validity bytes
    static_assert(GEMM == 0 || (CIN % 32 == 0 && COUT % 32 == 0 && (IP / KSPLIT) % 32 == 0), "bf16 MFMA: K in blocks of 32");
    static constexpr size_t RED1 = ((size_t)BWD_WAVES / NGRP * COUT * CIN + (size_t)BWD_THREADS * 24) * 4;   // flush area: dW1 K-slice planes + dW2/db records
    static constexpr size_t WORK = (size_t)WORK_F * 4;
    static constexpr size_t WORKB = WORK > RED1 ? WORK : RED1;
    static constexpr size_t SMEM = WORKB + (size_t)PAR_F * 4;
    static constexpr int MPW = IMT / BWD_WAVES;     // 16-pixel M tiles per wave
    // the register-bound variants re-derive thread-invariant indices per tile (see opaque())
    static constexpr bool LAUNDER = COUT >= 64 || CIN * COUT >= 2048 || TH * TW > 128;
    static_assert(IP % 16 == 0 && IMT % BWD_WAVES == 0, "whole M tiles per wave");
    static_assert(PG % TW == 0 && IP % PG == 0, "VALU mapping");
    static_assert(BWD_THREADS % C4I == 0 && BWD_THREADS % C4O == 0, "load mapping");
    static_assert((IP * C4I) % BWD_THREADS == 0, "x load mapping");
    static_assert((IP / 4) % KSPLIT == 0, "k split");
    static_assert(BWD_WAVES % NGRP == 0 && NGRP <= BWD_WAVES, "dW1 wave groups");
};


// FULL: the map is an exact multiple of the tile (H % TH == 0, W % TW == 0: the 160 x 160 and 80 x 80 levels), so
// every interior tile pixel is a real pixel and the per-element validity tests -- hundreds of integer
// instructions per tile -- compile away.  The launch picks the instance.
// DET (YunetBN::det_rows of the producer's BatchNorm, include/yunet_hip.h): the producer's BN-backward sums take a fixed
// order -- per tile every wave leaves its partial in a row of its own (in the dz tile, dead by then), thread c adds the
// eight rows in wave order into s_bst, and the workgroup's sums go to its own row of the block (common.h: bn_det_add).
// fp32 storage only.
template <int CIN, int COUT, int TH, int TW, bool PACKED, int GEMM = 0, bool POOLDY = false, bool FULL = false, bool DET = false>
__global__ __launch_bounds__(BWD_THREADS) void dp_bwd_kernel(const YunetDP d, const PackGeom pk) {
    using G = BwdGeom<CIN, COUT, TH, TW, GEMM>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* sm = reinterpret_cast<float*>(smem_raw);
    float* s_dz = sm + G::OFF_DZ;
    float* s_a = sm + G::OFF_A;
    float* s_pb = sm + G::OFF_PB;
    // the parameter/coefficient block sits after the (possibly larger) reduction work area
    float* s_w1 = reinterpret_cast<float*>(smem_raw + G::WORKB);   // [COUT][WS]  (GEMM 1: bf16 planes hi | lo [COUT][WSB], then b1[COUT])
    float* s_w2 = s_w1 + G::W1_F;                                  // [9][COUT]
    float* s_co = s_w2 + 9 * COUT;                                 // folded BN backward of the unit's own BN: A|B|Dh|Dl (+3 spare rows)
    float* s_ci = s_co + 7 * COUT;                                 // mean|scale|beta|invstd|mean_lo
    float* s_w1t = s_ci + 5 * CIN;                                 // [CIN][WST] (B operand of the da GEMM; GEMM 1: planes hi | lo [CIN][WSTB])
    double* s_bst = reinterpret_cast<double*>(s_w1t + G::W1T_F);   // [2][CIN] producer's BN-backward sums
    // GEMM 1 views of the weight block
    __bf16* s_w1h = reinterpret_cast<__bf16*>(s_w1);
    __bf16* s_w1l = s_w1h + COUT * G::WSB;
    float* s_b1 = reinterpret_cast<float*>(s_w1l + COUT * G::WSB);
    __bf16* s_w1th = reinterpret_cast<__bf16*>(s_w1t);
    __bf16* s_w1tl = s_w1th + CIN * G::WSTB;
    unsigned char* s_in = reinterpret_cast<unsigned char*>(s_bst + 2 * CIN);   // [IP] packed mode: pixel is real

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int H = d.H, W = d.W;
    const bool bn_in = d.in_transform == YUNET_T_BNRELU;
    const bool bn_out = d.out_has_bn != 0;
    // The input transform is applied branch-free where MFMA operands are read: with the identity
    // coefficients (mean 0, scale 1, beta 0) and a floor of -inf it returns its argument exactly,
    // so one straight-line GEMM body serves both kinds of unit and can be software-pipelined.
    const float relu_floor = bn_in ? 0.0f : -__builtin_inff();
    // debug ablation mask (tools/kbench.py --ablate): prof < 4096 is a bit mask, not a pointer
    const unsigned abl = (unsigned long long)d.prof < 4096ull ? (unsigned)(unsigned long long)d.prof : 0u;

    // per-image tiling, or (PACKED) one tile grid over the packed canvas of all images (common.h)
    const int tiles_x = ((PACKED ? pk.CW : W) + TW - 1) / TW, tiles_y = ((PACKED ? pk.CH : H) + TH - 1) / TH;
    const int tiles_img = tiles_x * tiles_y;
    const int ntiles = PACKED ? tiles_img : d.N * tiles_img;
    // inside(ip, Y, X): is interior tile pixel ip = (Y, X) a real pixel?  Packed tiles look it up in
    // a per-tile byte map written during the stage (one canvas -> image mapping per pixel and tile
    // instead of one per use).
    static_assert(!(FULL && PACKED), "FULL: unpacked maps only");
    auto inside = [&](int ip, int y, int x) {
        if constexpr (FULL) return true;
        else if constexpr (PACKED) return s_in[ip] != 0;
        else return y < H && x < W;
    };

    // ---- prefetch registers: raw dy / z_out (haloed) and x (interior) of the NEXT tile ------------
    // Loaded through per-image buffer descriptors: one 32-bit byte offset per slot, and a slot
    // outside the image (zero padding of the halo, ragged last tiles) simply gets an offset past
    // the end -- the hardware range check returns 0, so there are no branches and no 64-bit
    // address arithmetic.  okmask keeps one validity bit per halo slot for the stage.
    float4 pdy[G::NDZ];
    act_raw4 pz[G::NDZ], px[G::NX];          // saved activations: storage type of this build (fp32 | bf16)
    unsigned okmask = 0;
    // POOLDY (YunetDP.pool_idx): the unit's output feeds max_pool2d and nothing else.  A halo slot then
    // loads the gradient of ITS pooled element and that element's argmax bytes (4 channels = one dword);
    // the stage keeps the gradient where the slot is the window maximum.  posmask: window position
    // 2*(y&1) + (x&1) of every slot, two bits each.
    static_assert(!(POOLDY && PACKED), "pooled dy: unpacked levels only");
    static_assert(!POOLDY || G::NDZ <= 16, "posmask holds 16 slots");
    unsigned pid[POOLDY ? G::NDZ : 1];
    unsigned posmask = 0;
    const int Wq = W >> 1;
    const unsigned pooledbytes = (unsigned)((H >> 1) * Wq * COUT) * 4u;
    // dy / dx are fp32 in every build; z and x are activations
    const unsigned dybytes = (unsigned)(H * W * COUT) * 4u, zbytes = (unsigned)(H * W * COUT) * ACT_B;
    const unsigned xbytes = (unsigned)(H * W * CIN) * ACT_B, dxbytes = (unsigned)(H * W * CIN) * 4u;
    constexpr int PSTEP = BWD_THREADS / G::C4O;            // halo pixels between a thread's slots
    // issue(t, part): part -1 = everything at once; parts 0..3 = x | first | second | last third of the
    // (dy, z) slots.  A CU keeps far fewer bytes in flight than the 124 KB of a tile: issued in one go
    // the waves sit in the issue for the time the transfer takes (measured 5.8 k cycles per tile with
    // the per-phase counters); in four pieces between the phases the transfer runs under the compute.
    auto issue = [&](int t, auto part_c) {
        constexpr int PART = decltype(part_c)::value;
        const int tid = G::LAUNDER ? opaque((int)threadIdx.x) : (int)threadIdx.x;
        const int och4 = tid % G::C4O, ich4 = tid % G::C4I;
        const int n = PACKED ? 0 : t / tiles_img, rr = t - n * tiles_img;
        const int y0 = (rr / tiles_x) * TH, x0 = (rr % tiles_x) * TW;      // canvas coordinates if PACKED
        // packed: descriptors over the whole tensors, the image index is part of the offset
        const unsigned dyrange = PACKED ? (unsigned)d.N * (unsigned)d.z_img_stride * 4u : dybytes;
        const unsigned zrange = PACKED ? (unsigned)d.N * (unsigned)d.z_img_stride * ACT_B : zbytes;
        const unsigned xrange = PACKED ? (unsigned)d.N * (unsigned)d.x_img_stride * ACT_B : xbytes;
        const size_t zbase = PACKED ? (size_t)0 : (size_t)n * d.z_img_stride;
        const size_t xbase = PACKED ? (size_t)0 : (size_t)n * d.x_img_stride;
        const auto r_dy = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(d.dy) + (POOLDY ? (size_t)n * (pooledbytes / 4u) : zbase), 0, POOLDY ? pooledbytes : dyrange, 0x00020000);
        const auto r_id = __builtin_amdgcn_make_buffer_rsrc(
            d.pool_idx + (POOLDY ? (size_t)n * (pooledbytes / 4u) : (size_t)0), 0,
            POOLDY ? pooledbytes / 4u : 0u, 0x00020000);
        const auto r_z = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<act_t*>(const_cast<float*>(d.z)) + zbase, 0, zrange, 0x00020000);
        const auto r_x = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<act_t*>(const_cast<float*>(d.x)) + xbase, 0, xrange, 0x00020000);
        if (PART <= 0) { okmask = 0; posmask = 0; }
#pragma unroll
        for (int i = 0; i < G::NDZ; ++i) {
            if (PART >= 0 && PART != 1 + (3 * i) / G::NDZ) continue;
            const int hp = tid / G::C4O + PSTEP * i;
            const int hy = hp / G::HW_, hx = hp - hy * G::HW_;
            const int y = y0 - 1 + hy, x = x0 - 1 + hx;
            bool ok;
            unsigned eo;                              // element offset of the slot
            if constexpr (PACKED) {
                int pn, py, px;
                ok = hp < G::HP && pk_locate(pk, y, x, pn, py, px);
                eo = (unsigned)(pn * d.z_img_stride + (py * W + px) * COUT + och4 * 4);
            } else {
                ok = hp < G::HP && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
                eo = (unsigned)((y * W + x) * COUT + och4 * 4);
            }
            okmask |= ok ? (1u << i) : 0u;
            if constexpr (POOLDY) {
                const unsigned eq = (unsigned)(((y >> 1) * Wq + (x >> 1)) * COUT + och4 * 4);   // pooled element
                posmask |= (unsigned)(((y & 1) << 1) | (x & 1)) << (2 * i);
                const u32x4 vdy = __builtin_amdgcn_raw_buffer_load_b128(r_dy, ok ? eq * 4u : pooledbytes, 0, 0);
                pdy[i] = *reinterpret_cast<const float4*>(&vdy);
                pid[i] = __builtin_amdgcn_raw_buffer_load_b32(r_id, ok ? eq : pooledbytes, 0, 0);
            } else {
                const u32x4 vdy = __builtin_amdgcn_raw_buffer_load_b128(r_dy, ok ? eo * 4u : dyrange, 0, 0);
                pdy[i] = *reinterpret_cast<const float4*>(&vdy);
            }
            pz[i] = act_raw4{};
            if (bn_out) pz[i] = act_bufld4(r_z, ok ? eo * ACT_B : zrange);
            // packed: finish one slot's address arithmetic before the next one starts (otherwise
            // all 16 canvas -> image mappings are computed up front and spill)
            if constexpr (PACKED) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < G::NX; ++i) {
            if (PART > 0) continue;
            const int ip = (tid + BWD_THREADS * i) / G::C4I;
            const int y = y0 + ip / TW, x = x0 + ip % TW;
            unsigned off;
            if constexpr (PACKED) {
                int pn, py, px;
                off = pk_locate(pk, y, x, pn, py, px)
                          ? (unsigned)(pn * d.x_img_stride + (py * W + px) * CIN + ich4 * 4) * ACT_B : xrange;
            } else {
                off = (FULL || (y < H && x < W)) ? (unsigned)((y * W + x) * CIN + ich4 * 4) * ACT_B : xbytes;
            }
            px[i] = act_bufld4(r_x, off);
            if constexpr (PACKED) __builtin_amdgcn_sched_barrier(0);
        }
    };

    // the first tile's global loads go out BEFORE the weights / coefficients are staged: the HBM
    // latency of a cold start runs under the prologue
    using All = std::integral_constant<int, -1>;
    int t = first_tile();
    if (t < ntiles) issue(t, All{});

    if constexpr (GEMM == 1) {
        // W1 -> bf16 hi / lo planes in both orientations, 8 weights per thread and pass, every global
        // load of a pass in flight at once, 16-byte LDS stores
        // (32 -> 64: 256 groups for 512 threads -- the upper half repeats the lower half's groups, same values to the same
        // addresses, instead of a divergent branch)
        static_assert(COUT * CIN <= 8 * BWD_THREADS && (8 * BWD_THREADS) % (COUT * CIN) == 0, "8-weight groups per thread");
        const int t8 = tid % (COUT * CIN / 8);
        {
            const int co = t8 / (CIN / 8), c0 = (t8 % (CIN / 8)) * 8;
            const float4 a = *reinterpret_cast<const float4*>(d.w_pw + co * CIN + c0);
            const float4 b = *reinterpret_cast<const float4*>(d.w_pw + co * CIN + c0 + 4);
            const float w8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            const Split8 sp = split8(w8);
            *reinterpret_cast<u32x4*>(s_w1h + co * G::WSB + c0) = sp.hi;
            *reinterpret_cast<u32x4*>(s_w1l + co * G::WSB + c0) = sp.lo;
            if (c0 == 0) s_b1[co] = d.b_pw[co];
        }
        {
            const int ci = t8 / (COUT / 8), o0 = (t8 % (COUT / 8)) * 8;
            float w8[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) w8[j] = d.w_pw[(o0 + j) * CIN + ci];
            const Split8 sp = split8(w8);
            *reinterpret_cast<u32x4*>(s_w1th + ci * G::WSTB + o0) = sp.hi;
            *reinterpret_cast<u32x4*>(s_w1tl + ci * G::WSTB + o0) = sp.lo;
        }
    } else {
        staged_table<COUT * CIN, BWD_THREADS>(d.w_pw, tid, [&](int i, float w) {       // (common.h: every load in flight first)
            s_w1[(i / CIN) * G::WS + (i % CIN)] = w;
            if (i % CIN == 0) s_w1[(i / CIN) * G::WS + CIN] = d.b_pw[i / CIN];   // bias rides in the row padding
            s_w1t[(i % CIN) * G::WST + (i / CIN)] = w;
        });
    }
    staged_table<COUT * 9, BWD_THREADS>(d.w_dw, tid, [&](int i, float w) { s_w2[(i % 9) * COUT + i / 9] = w; });
    for (int c = tid; c < COUT; c += BWD_THREADS) {
        // dz = k1 * (dy - c1 - xhat * c2) folded into dz = A dy + B z + D (see bn_fold in common.h)
        if (bn_out) {
            const BNFold f = bn_fold(bn_bwd_coef(d.out_bn, COUT, c));
            s_co[c] = f.a; s_co[COUT + c] = f.b; s_co[2 * COUT + c] = f.dh; s_co[3 * COUT + c] = f.dl;
        } else {
            s_co[c] = d.dy_scale ? d.dy_scale[c] : 1.0f;
            s_co[COUT + c] = 0.f; s_co[2 * COUT + c] = 0.f; s_co[3 * COUT + c] = 0.f;
        }
    }
    for (int c = tid; c < CIN; c += BWD_THREADS) {
        if (bn_in) {
            const BNCoef k = bn_coef(d.in_bn, CIN, c);
            s_ci[c] = k.mean; s_ci[CIN + c] = k.scale; s_ci[2 * CIN + c] = k.beta;
            s_ci[3 * CIN + c] = k.invstd; s_ci[4 * CIN + c] = k.mean_lo;
        } else {
            s_ci[c] = 0.f; s_ci[CIN + c] = 1.f; s_ci[2 * CIN + c] = 0.f; s_ci[3 * CIN + c] = 1.f;
            s_ci[4 * CIN + c] = 0.f;
        }
    }
    __syncthreads();

    // ---- per-thread constants ---------------------------------------------------------------
    // VALU phase: channel quad cq, pixel column vtx, rows vr0..vr0+PPT-1
    const int cq = tid % G::C4O, pg = tid / G::C4O;
    const int vtx = pg % TW, vr0 = (pg / TW) * G::PPT;
    // persistent accumulators (flushed once per workgroup)
    float4 gw2[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) gw2[t] = make_float4(0, 0, 0, 0);
    float4 gb2 = make_float4(0, 0, 0, 0), gb1 = make_float4(0, 0, 0, 0);
    // per-lane partials of the producer's BN-backward sums, D layout: channel nt*16 + l15.
    // fp64: sum(dy) cancels heavily and feeds c1 = mean(dy) of EVERY dz of the producer --
    // fp32 partials here showed up as 0.3 % errors in depthwise weight gradients upstream.
    // (kept in LDS, one fp64 atomic per lane / channel block / tile: as registers they cost 16
    // VGPRs for the whole kernel and pushed the 64-channel variant into scratch)
    for (int i = tid; i < 2 * CIN; i += BWD_THREADS) s_bst[i] = 0.0;
    f32x4 gw1[G::MB * G::NB];   // dW1: this wave's interleaved 16x16 tiles
#pragma unroll
    for (int i = 0; i < G::MB * G::NB; ++i) gw1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int w1_grp = wid % G::NGRP, w1_kslice = wid / G::NGRP;
    const int w1_ci0 = (w1_grp / (G::NTO / G::NB)) * 16 * G::MB;   // first ci / co of the wave's block
    const int w1_co0 = (w1_grp % (G::NTO / G::NB)) * 16 * G::NB;

    // next tile's loads in four pieces (measured: -8 % on 16->16 at 160x160, -6 % on 16->64, +2 % on the
    // 64->16 heads, which keep the single issue)
    constexpr bool SPREAD = GEMM == 1 || COUT >= 32 || CIN == 16;
    const bool pf_on = !(abl & 32);
    for (; t < ntiles; t += gridDim.x) {
        const int n = PACKED ? 0 : t / tiles_img, rr = t - n * tiles_img;
        const int y0 = (rr / tiles_x) * TH, x0 = (rr % tiles_x) * TW;      // canvas coordinates if PACKED

        // ---- stage: dz (BN backward of this unit's own BN) and a = T(x) -> LDS ------------------
        {
            const int tid = G::LAUNDER ? opaque((int)threadIdx.x) : (int)threadIdx.x;
            const int och4 = tid % G::C4O, ich4 = tid % G::C4I;
            const float4 o_a = *reinterpret_cast<float4*>(s_co + och4 * 4);
            const float4 o_b = *reinterpret_cast<float4*>(s_co + COUT + och4 * 4);
            const float4 o_dh = *reinterpret_cast<float4*>(s_co + 2 * COUT + och4 * 4);
            const float4 o_dl = *reinterpret_cast<float4*>(s_co + 3 * COUT + och4 * 4);
            const int hp0 = tid / G::C4O;
#pragma unroll
            for (int i = 0; i < G::NDZ; ++i) {
                const int hp = hp0 + PSTEP * i;
                if ((i + 1) * PSTEP <= G::HP || hp < G::HP) {
                    float4 dy = pdy[i];
                    const float4 z = act_unpack(pz[i]);
                    if constexpr (POOLDY) {
                        // max_pool2d backward: the pooled gradient reaches the window maximum only
                        const unsigned id = pid[i], pos = (posmask >> (2 * i)) & 3u;
                        dy.x = (id & 0xffu) == pos ? dy.x : 0.0f;
                        dy.y = ((id >> 8) & 0xffu) == pos ? dy.y : 0.0f;
                        dy.z = ((id >> 16) & 0xffu) == pos ? dy.z : 0.0f;
                        dy.w = (id >> 24) == pos ? dy.w : 0.0f;
                    }
                    // zero padding of dz: a slot outside the image loaded dy = z = 0, which the BN backward
                    // would turn into D
                    const bool ok = (okmask >> i) & 1u;
                    float4 v;
                    v.x = ok ? fmaf(o_a.x, dy.x, fmaf(o_b.x, z.x, o_dh.x)) + o_dl.x : 0.0f;
                    v.y = ok ? fmaf(o_a.y, dy.y, fmaf(o_b.y, z.y, o_dh.y)) + o_dl.y : 0.0f;
                    v.z = ok ? fmaf(o_a.z, dy.z, fmaf(o_b.z, z.z, o_dh.z)) + o_dl.z : 0.0f;
                    v.w = ok ? fmaf(o_a.w, dy.w, fmaf(o_b.w, z.w, o_dh.w)) + o_dl.w : 0.0f;
                    *reinterpret_cast<float4*>(s_dz + hp * G::LSO + och4 * 4) = v;
                }
            }
            if constexpr (PACKED) {
                for (int ip = tid; ip < G::IP; ip += BWD_THREADS) {
                    int pn, py, px;
                    s_in[ip] = pk_locate(pk, y0 + ip / TW, x0 + ip % TW, pn, py, px) ? 1 : 0;
                }
            }
            // the interior input tile goes to LDS RAW; the input transform (BN+ReLU of the
            // producer) is applied where MFMA operands are read, so the raw values stay available
            // for the ReLU mask and the BN-backward sums of the producer
#pragma unroll
            for (int i = 0; i < G::NX; ++i) {
                const int ip = (tid + BWD_THREADS * i) / G::C4I;
                *reinterpret_cast<float4*>(s_a + ip * G::LSI + ich4 * 4) = act_unpack(px[i]);
            }
        }
        __syncthreads();
        const bool more = t + (int)gridDim.x < ntiles && pf_on;
        if (SPREAD && more) issue(t + gridDim.x, std::integral_constant<int, 0>{});

        // ---- p = a * W1^T + b1 on the interior pixels (one M tile per wave) ---------------------
        if constexpr (GEMM == 1) {
            if (!(abl & 1)) {
#pragma unroll 1
                for (int mi = 0; mi < G::MPW; ++mi) {
                    const int mt = wid * G::MPW + mi;
                    f32x4 acc[G::NTO];
#pragma unroll
                    for (int nt = 0; nt < G::NTO; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    // lane group g supplies input channels 32*kb + 8g .. +7 of pixel row l15 (A) and
                    // of weight row nt*16 + l15 (B): the same k order on both sides
                    const float* arow = s_a + (mt * 16 + l15) * G::LSI + 8 * g;
                    const float* crow = s_ci + 8 * g;
                    const __bf16* bh = s_w1h + l15 * G::WSB + 8 * g;
                    const __bf16* bl = s_w1l + l15 * G::WSB + 8 * g;
#pragma unroll
                    for (int kb = 0; kb < CIN / 32; ++kb) {
                        float a8[8];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const float4 xv = *reinterpret_cast<const float4*>(arow + 32 * kb + 4 * h);
                            const float4 mv = *reinterpret_cast<const float4*>(crow + 32 * kb + 4 * h);
                            const float4 sv = *reinterpret_cast<const float4*>(crow + CIN + 32 * kb + 4 * h);
                            const float4 tv = *reinterpret_cast<const float4*>(crow + 2 * CIN + 32 * kb + 4 * h);
                            a8[4 * h + 0] = tin(xv.x, mv.x, sv.x, tv.x, relu_floor);
                            a8[4 * h + 1] = tin(xv.y, mv.y, sv.y, tv.y, relu_floor);
                            a8[4 * h + 2] = tin(xv.z, mv.z, sv.z, tv.z, relu_floor);
                            a8[4 * h + 3] = tin(xv.w, mv.w, sv.w, tv.w, relu_floor);
                        }
                        const Split8 as = split8(a8);
#pragma unroll
                        for (int nt = 0; nt < G::NTO; ++nt) {
                            const u32x4 vh = *reinterpret_cast<const u32x4*>(bh + nt * 16 * G::WSB + 32 * kb);
                            const u32x4 vl = *reinterpret_cast<const u32x4*>(bl + nt * 16 * G::WSB + 32 * kb);
                            acc[nt] = mfma3(as, vh, vl, acc[nt]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ip = mt * 16 + 4 * g + r;
                        const bool in = inside(ip, y0 + ip / TW, x0 + ip % TW);
#pragma unroll
                        for (int nt = 0; nt < G::NTO; ++nt)
                            s_pb[ip * G::LSO + nt * 16 + l15] = in ? acc[nt][r] + s_b1[nt * 16 + l15] : 0.0f;
                    }
                }
            }
        } else if (!(abl & 1)) {
            // 16-channel inputs: one k block per pixel tile -- the wave's pixel tiles are unrolled so that their
            // read -> transform -> 4 dependent MFMAs -> write chains overlap (rolled, each tile pays the whole latency)
#pragma unroll (CIN == 16 ? G::MPW : 1)
            for (int mi = 0; mi < G::MPW; ++mi) {
                const int mt = wid * G::MPW + mi;
                f32x4 acc[G::NTO];
#pragma unroll
                for (int nt = 0; nt < G::NTO; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
                // k-permuted operands: within each block of 16 input channels lane group g supplies
                // channels 4g..4g+3 -- one 16-byte LDS read feeds four MFMA k-steps (A and B use
                // the same permutation, so the sum over k is unchanged)
                const float* arow = s_a + (mt * 16 + l15) * G::LSI + 4 * g;
                const float* brow = s_w1 + l15 * G::WS + 4 * g;
                const float* crow = s_ci + 4 * g;
                // rolled loop, operands of block q+1 loaded while block q is on the matrix cores
                // (a rolled loop bounds the live operand set to two blocks -- a fully unrolled one
                // lets the scheduler hoist every read and spill)
                constexpr int NQ = CIN / 16, UNR = (NQ > 2 && G::NTO >= 4) ? 1 : NQ;
                float4 a_c = *reinterpret_cast<const float4*>(arow);
                float4 m_c = *reinterpret_cast<const float4*>(crow);
                float4 s_c = *reinterpret_cast<const float4*>(crow + CIN);
                float4 t_c = *reinterpret_cast<const float4*>(crow + 2 * CIN);
                float4 b_c[G::NTO];
#pragma unroll
                for (int nt = 0; nt < G::NTO; ++nt)
                    b_c[nt] = *reinterpret_cast<const float4*>(brow + nt * 16 * G::WS);
#pragma unroll UNR
                for (int q = 0; q < NQ; ++q) {
                    const int qn = UNR == 1 ? 16 * ((q + 1) % NQ) : (q + 1 < NQ ? 16 * (q + 1) : 0);
                    const float4 a_n = *reinterpret_cast<const float4*>(arow + qn);
                    const float4 m_n = *reinterpret_cast<const float4*>(crow + qn);
                    const float4 s_n = *reinterpret_cast<const float4*>(crow + CIN + qn);
                    const float4 t_n = *reinterpret_cast<const float4*>(crow + 2 * CIN + qn);
                    float4 b_n[G::NTO];
#pragma unroll
                    for (int nt = 0; nt < G::NTO; ++nt)
                        b_n[nt] = *reinterpret_cast<const float4*>(brow + nt * 16 * G::WS + qn);
                    const float ax = tin(a_c.x, m_c.x, s_c.x, t_c.x, relu_floor);
                    const float ay = tin(a_c.y, m_c.y, s_c.y, t_c.y, relu_floor);
                    const float az = tin(a_c.z, m_c.z, s_c.z, t_c.z, relu_floor);
                    const float aw = tin(a_c.w, m_c.w, s_c.w, t_c.w, relu_floor);
#pragma unroll
                    for (int nt = 0; nt < G::NTO; ++nt) acc[nt] = mfma16(ax, b_c[nt].x, acc[nt]);
#pragma unroll
                    for (int nt = 0; nt < G::NTO; ++nt) acc[nt] = mfma16(ay, b_c[nt].y, acc[nt]);
#pragma unroll
                    for (int nt = 0; nt < G::NTO; ++nt) acc[nt] = mfma16(az, b_c[nt].z, acc[nt]);
#pragma unroll
                    for (int nt = 0; nt < G::NTO; ++nt) acc[nt] = mfma16(aw, b_c[nt].w, acc[nt]);
                    a_c = a_n; m_c = m_n; s_c = s_n; t_c = t_n;
#pragma unroll
                    for (int nt = 0; nt < G::NTO; ++nt) b_c[nt] = b_n[nt];
                }
                float bias_pw[G::NTO];
#pragma unroll
                for (int nt = 0; nt < G::NTO; ++nt) bias_pw[nt] = s_w1[(nt * 16 + (G::LAUNDER ? opaque(l15) : l15)) * G::WS + CIN];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ip = mt * 16 + 4 * g + r;
                    const bool in = inside(ip, y0 + ip / TW, x0 + ip % TW);
#pragma unroll
                    for (int nt = 0; nt < G::NTO; ++nt)
                        s_pb[ip * G::LSO + nt * 16 + l15] = in ? acc[nt][r] + bias_pw[nt] : 0.0f;
                }
            }
        }
        __syncthreads();
        if (SPREAD && more) issue(t + gridDim.x, std::integral_constant<int, 1>{});

        // ---- depthwise backward on the VALU; dp overwrites p in place ----------------------------
        // A thread owns a channel quad and a column of PPT rows.  The dz column triple is walked
        // once with a sliding window: each dz value is read from LDS one time and feeds every
        // output row it touches (3x fewer LDS reads than tap-by-tap when PPT = 4).
        if (!(abl & 2)) {
            // thread coordinates re-derived from an opaque copy of tid: all LDS addresses of this phase
            // become ONE per-tile base register + compile-time offsets (hoisted out of the tile loop
            // they are ~30 separate address registers, which the allocator then spills)
            const int tv = G::LAUNDER ? opaque((int)threadIdx.x) : (int)threadIdx.x;
            const int cq = tv % G::C4O, pg = tv / G::C4O;
            const int vtx = pg % TW, vr0 = (pg / TW) * G::PPT;
            const float* zb = s_dz + (vr0 * G::HW_ + vtx) * G::LSO + cq * 4;
            float* pb = s_pb + (vr0 * TW + vtx) * G::LSO + cq * 4;
            const float* wb = s_w2 + cq * 4;
            float4 pv[G::PPT], dp[G::PPT];
#pragma unroll
            for (int r = 0; r < G::PPT; ++r) {
                pv[r] = *reinterpret_cast<const float4*>(pb + r * TW * G::LSO);
                dp[r] = make_float4(0, 0, 0, 0);
            }
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                float4 wk[3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    wk[a] = *reinterpret_cast<const float4*>(wb + (8 - (3 * a + b)) * COUT);
#pragma unroll
                for (int j = 0; j < G::PPT + 2; ++j) {
                    const float4 z4 = *reinterpret_cast<const float4*>(zb + (j * G::HW_ + b) * G::LSO);
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const int r = j - a;
                        if (r < 0 || r >= G::PPT) continue;
                        const int k = 8 - (3 * a + b);
                        dp[r].x = fmaf(z4.x, wk[a].x, dp[r].x); dp[r].y = fmaf(z4.y, wk[a].y, dp[r].y);
                        dp[r].z = fmaf(z4.z, wk[a].z, dp[r].z); dp[r].w = fmaf(z4.w, wk[a].w, dp[r].w);
                        gw2[k].x = fmaf(pv[r].x, z4.x, gw2[k].x); gw2[k].y = fmaf(pv[r].y, z4.y, gw2[k].y);
                        gw2[k].z = fmaf(pv[r].z, z4.z, gw2[k].z); gw2[k].w = fmaf(pv[r].w, z4.w, gw2[k].w);
                        if (a == 1 && b == 1) {
                            gb2.x += z4.x; gb2.y += z4.y; gb2.z += z4.z; gb2.w += z4.w;
                        }
                    }
                }
                // one column at a time: without this the scheduler hoists all 3*(PPT+2) reads
                if (G::PPT > 1) __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int r = 0; r < G::PPT; ++r) {
                const bool in = inside((vr0 + r) * TW + vtx, y0 + vr0 + r, x0 + vtx);
                if (!in) dp[r] = make_float4(0, 0, 0, 0);
                gb1.x += dp[r].x; gb1.y += dp[r].y; gb1.z += dp[r].z; gb1.w += dp[r].w;
                *reinterpret_cast<float4*>(pb + r * TW * G::LSO) = dp[r];
            }
        }
        __syncthreads();
        // prefetch the next tile's global data; issued here (not right after the stage) so that the
        // p GEMM and the VALU phase run without ~64 prefetch registers live -- the two GEMMs, the
        // mask phase and the store that follow are several microseconds, enough for HBM
        if (SPREAD) { if (more) issue(t + gridDim.x, std::integral_constant<int, 2>{}); }
        else if (more) issue(t + gridDim.x, All{});

        // ---- dW1 += a^T * dp (K = pixels) and da = dp * W1 on the matrix cores -------------------
        if constexpr (GEMM == 1) {
            if (!(abl & 4)) {
                static_assert(GEMM == 0 || (G::MB == 2 && G::NB == 2), "bf16 dW1: 2x2 interleaved tiles");
                // K = pixels.  Within a block of 32 pixels lane group g supplies rows 8g .. 8g+7 of BOTH
                // operands (8-byte reads of 2 interleaved channels, rows 8 apart between lane groups:
                // conflict-free for ds_read_b64 with the 68-float row stride)
                const float* ap = s_a + (w1_kslice * G::KPX + 8 * g) * G::LSI + w1_ci0 + 2 * l15;
                const float* bp = s_pb + (w1_kslice * G::KPX + 8 * g) * G::LSO + w1_co0 + 2 * l15;
                float am[2], as_[2], ab[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int ca = w1_ci0 + 2 * (G::LAUNDER ? opaque(l15) : l15) + j;
                    am[j] = s_ci[ca]; as_[j] = s_ci[CIN + ca]; ab[j] = s_ci[2 * CIN + ca];
                }
#pragma unroll 1
                for (int kb = 0; kb < G::KPX / 32; ++kb) {
                    // dp first (split once, used by both ci tiles), then one ci tile at a time: at most
                    // 16 raw floats + 24 packed operand registers are live
                    Split8 sd0, sd1;
                    {
                        float d0[8], d1[8];
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            const float2 dv = *reinterpret_cast<const float2*>(bp + (32 * kb + t) * G::LSO);
                            d0[t] = dv.x; d1[t] = dv.y;
                        }
                        sd0 = split8(d0);
                        sd1 = split8(d1);
                    }
                    float2 av[8];
#pragma unroll
                    for (int t = 0; t < 8; ++t) av[t] = *reinterpret_cast<const float2*>(ap + (32 * kb + t) * G::LSI);
                    {
                        float a0[8];
#pragma unroll
                        for (int t = 0; t < 8; ++t) a0[t] = tin(av[t].x, am[0], as_[0], ab[0], relu_floor);
                        const Split8 sa0 = split8(a0);
                        gw1[0] = mfma3(sa0, sd0.hi, sd0.lo, gw1[0]);
                        gw1[1] = mfma3(sa0, sd1.hi, sd1.lo, gw1[1]);
                    }
                    {
                        float a1[8];
#pragma unroll
                        for (int t = 0; t < 8; ++t) a1[t] = tin(av[t].y, am[1], as_[1], ab[1], relu_floor);
                        const Split8 sa1 = split8(a1);
                        gw1[2] = mfma3(sa1, sd0.hi, sd0.lo, gw1[2]);
                        gw1[3] = mfma3(sa1, sd1.hi, sd1.lo, gw1[3]);
                    }
                }
            }
        } else
        if (!(abl & 4)) {
            const float* ap = s_a + (w1_kslice * G::KSTEPS * 4 + g) * G::LSI + w1_ci0 + G::MB * l15;
            const float* bp = s_pb + (w1_kslice * G::KSTEPS * 4 + g) * G::LSO + w1_co0 + G::NB * l15;
            float am[G::MB], as_[G::MB], ab[G::MB];
#pragma unroll
            for (int j = 0; j < G::MB; ++j) {
                const int ca = w1_ci0 + G::MB * (G::LAUNDER ? opaque(l15) : l15) + j;
                am[j] = s_ci[ca]; as_[j] = s_ci[CIN + ca]; ab[j] = s_ci[2 * CIN + ca];
            }
            // a single 16 x 16 tile per wave (16 -> 16 units) would be one chain of KSTEPS dependent MFMAs: four
            // partial accumulators, summed once per tile
            constexpr int NPART = (G::MB * G::NB == 1) ? 4 : 1;
            f32x4 part[NPART];
            if constexpr (NPART > 1) {
#pragma unroll
                for (int q = 0; q < NPART; ++q) part[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll 8
            for (int s = 0; s < G::KSTEPS; ++s) {
                float av[G::MB], bv[G::NB];
                if (G::MB == 2) {
                    const float2 t2 = *reinterpret_cast<const float2*>(ap + 4 * s * G::LSI);
                    av[0] = t2.x; av[G::MB - 1] = t2.y;
                } else {
                    av[0] = ap[4 * s * G::LSI];
                }
                if (G::NB == 2) {
                    const float2 t2 = *reinterpret_cast<const float2*>(bp + 4 * s * G::LSO);
                    bv[0] = t2.x; bv[G::NB - 1] = t2.y;
                } else {
                    bv[0] = bp[4 * s * G::LSO];
                }
#pragma unroll
                for (int j = 0; j < G::MB; ++j) {
                    const float a = tin(av[j], am[j], as_[j], ab[j], relu_floor);
                    if constexpr (NPART > 1) {
                        part[s % NPART] = mfma16(a, bv[0], part[s % NPART]);
                    } else {
#pragma unroll
                        for (int i = 0; i < G::NB; ++i)
                            gw1[j * G::NB + i] = mfma16(a, bv[i], gw1[j * G::NB + i]);
                    }
                }
            }
            if constexpr (NPART > 1) {
                static_assert(NPART == 1 || G::KSTEPS % 4 == 0, "partial accumulators: whole rounds of four k-steps");
#pragma unroll
                for (int r = 0; r < 4; ++r) gw1[0][r] += (part[0][r] + part[1][r]) + (part[2][r] + part[3][r]);
            }
        }
        if (SPREAD && more) issue(t + gridDim.x, std::integral_constant<int, 3>{});
        f32x4 da[G::MPW][G::NTI];
#pragma unroll
        for (int mi = 0; mi < G::MPW; ++mi)
#pragma unroll
            for (int nt = 0; nt < G::NTI; ++nt) da[mi][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (GEMM == 1) {
            if (!(abl & 8)) {
#pragma unroll
                for (int mi = 0; mi < G::MPW; ++mi) {
                    // k = output channels: lane group g supplies channels 32*kb + 8g .. +7
                    const float* prow = s_pb + ((wid * G::MPW + mi) * 16 + l15) * G::LSO + 8 * g;
                    const __bf16* wh = s_w1th + l15 * G::WSTB + 8 * g;
                    const __bf16* wl = s_w1tl + l15 * G::WSTB + 8 * g;
#pragma unroll
                    for (int kb = 0; kb < COUT / 32; ++kb) {
                        float p8[8];
                        const float4 v0 = *reinterpret_cast<const float4*>(prow + 32 * kb);
                        const float4 v1 = *reinterpret_cast<const float4*>(prow + 32 * kb + 4);
                        p8[0] = v0.x; p8[1] = v0.y; p8[2] = v0.z; p8[3] = v0.w;
                        p8[4] = v1.x; p8[5] = v1.y; p8[6] = v1.z; p8[7] = v1.w;
                        const Split8 ps = split8(p8);
#pragma unroll
                        for (int nt = 0; nt < G::NTI; ++nt) {
                            const u32x4 vh = *reinterpret_cast<const u32x4*>(wh + nt * 16 * G::WSTB + 32 * kb);
                            const u32x4 vl = *reinterpret_cast<const u32x4*>(wl + nt * 16 * G::WSTB + 32 * kb);
                            da[mi][nt] = mfma3(ps, vh, vl, da[mi][nt]);
                        }
                    }
                }
            }
        } else if (!(abl & 8)) {
#pragma unroll
            for (int mi = 0; mi < G::MPW; ++mi) {
                const float* prow = s_pb + ((wid * G::MPW + mi) * 16 + l15) * G::LSO + 4 * g;
                const float* wrow = s_w1t + l15 * G::WST + 4 * g;
                constexpr int NQ = COUT / 16, UNR = (NQ > 2 && G::NTI >= 4) ? 1 : NQ;   // k = output channels, permuted as above
                float4 a_c = *reinterpret_cast<const float4*>(prow);
                float4 b_c[G::NTI];
#pragma unroll
                for (int nt = 0; nt < G::NTI; ++nt)
                    b_c[nt] = *reinterpret_cast<const float4*>(wrow + nt * 16 * G::WST);
#pragma unroll UNR
                for (int q = 0; q < NQ; ++q) {
                    const int qn = UNR == 1 ? 16 * ((q + 1) % NQ) : (q + 1 < NQ ? 16 * (q + 1) : 0);
                    const float4 a_n = *reinterpret_cast<const float4*>(prow + qn);
                    float4 b_n[G::NTI];
#pragma unroll
                    for (int nt = 0; nt < G::NTI; ++nt)
                        b_n[nt] = *reinterpret_cast<const float4*>(wrow + nt * 16 * G::WST + qn);
#pragma unroll
                    for (int nt = 0; nt < G::NTI; ++nt) da[mi][nt] = mfma16(a_c.x, b_c[nt].x, da[mi][nt]);
#pragma unroll
                    for (int nt = 0; nt < G::NTI; ++nt) da[mi][nt] = mfma16(a_c.y, b_c[nt].y, da[mi][nt]);
#pragma unroll
                    for (int nt = 0; nt < G::NTI; ++nt) da[mi][nt] = mfma16(a_c.z, b_c[nt].z, da[mi][nt]);
#pragma unroll
                    for (int nt = 0; nt < G::NTI; ++nt) da[mi][nt] = mfma16(a_c.w, b_c[nt].w, da[mi][nt]);
                    a_c = a_n;
#pragma unroll
                    for (int nt = 0; nt < G::NTI; ++nt) b_c[nt] = b_n[nt];
                }
            }
        }
        __syncthreads();  // every wave is done reading s_a for dW1
        if (bn_in) {
#pragma unroll
            for (int nt = 0; nt < G::NTI; ++nt) {
                const int c = nt * 16 + (G::LAUNDER ? opaque(l15) : l15);   // (keeps the 5*NTI coefficients out of loop-invariant registers)
                const float cm = s_ci[c], cs = s_ci[CIN + c], cb = s_ci[2 * CIN + c], ci = s_ci[3 * CIN + c];
                const float cl = s_ci[4 * CIN + c];
                // Sums of this wave's 16 * MPW pixels in fp32 (a handful of terms: rounding 1e-7 of the
                // partial), folded over the four lane groups with two cross-lane adds; only then fp64 and
                // ONE LDS atomic per channel and wave (the long, heavily cancelling accumulation over the
                // whole tensor stays in fp64).  64 lanes x 2 fp64 atomics on 16 addresses per channel block
                // used to serialise in the LDS.
                float t0 = 0.0f, t1 = 0.0f;
#pragma unroll
                for (int mi = 0; mi < G::MPW; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ip = (wid * G::MPW + mi) * 16 + 4 * g + r;
                        float* ap = s_a + ip * G::LSI + c;
                        const float xr = *ap;
                        const bool in = inside(ip, y0 + ip / TW, x0 + ip % TW);
                        const float v = (in && fmaf(xr - cm, cs, cb) > 0.0f) ? da[mi][nt][r] : 0.0f;   // ReLU mask
                        t0 += v;
                        t1 = fmaf(v, bn_center(xr, cm, cl) * ci, t1);
                        *ap = v;
                    }
                t0 += __shfl_xor(t0, 16, 64); t1 += __shfl_xor(t1, 16, 64);
                t0 += __shfl_xor(t0, 32, 64); t1 += __shfl_xor(t1, 32, 64);
                if constexpr (DET) {
                    // s_dz was last read by the depthwise phase (two barriers back) and is rewritten by the next tile's stage
                    // (after the barrier that ends this tile): [BWD_WAVES][2 CIN] doubles of it carry the waves' partials
                    static_assert((size_t)BWD_WAVES * 2 * CIN * 8 <= (size_t)G::HP * G::LSO * 4, "wave rows fit in the dz tile");
                    double* wrow = reinterpret_cast<double*>(s_dz) + wid * 2 * CIN;
                    if (g == 0) { wrow[c] = (double)t0; wrow[CIN + c] = (double)t1; }
                } else if (g == 0) {
                    __hip_atomic_fetch_add(s_bst + c, (double)t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(s_bst + CIN + c, (double)t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        } else {
#pragma unroll
            for (int nt = 0; nt < G::NTI; ++nt)
#pragma unroll
                for (int mi = 0; mi < G::MPW; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        s_a[((wid * G::MPW + mi) * 16 + 4 * g + r) * G::LSI + nt * 16 + l15] = da[mi][nt][r];
        }
        __syncthreads();
        if constexpr (DET) {
            if (bn_in && tid < 2 * CIN) {
                const double* wrow = reinterpret_cast<const double*>(s_dz) + tid;
                double v = s_bst[tid];
#pragma unroll
                for (int wv = 0; wv < BWD_WAVES; ++wv) v += wrow[wv * 2 * CIN];
                s_bst[tid] = v;
            }
        }

        // ---- dx store (coalesced) + BN-backward sums of the producer ------------------------------
        if (d.dx && !(abl & 16)) {
            const int tid = G::LAUNDER ? opaque((int)threadIdx.x) : (int)threadIdx.x;
            const int ich4 = tid % G::C4I;
            const unsigned xrange = PACKED ? (unsigned)d.N * (unsigned)d.x_img_stride * 4u : dxbytes;
            const auto r_dx = __builtin_amdgcn_make_buffer_rsrc(
                d.dx + (PACKED ? (size_t)0 : (size_t)n * d.x_img_stride), 0, xrange, 0x00020000);
            unsigned off[G::NX];
#pragma unroll
            for (int i = 0; i < G::NX; ++i) {
                const int ip = (tid + BWD_THREADS * i) / G::C4I;
                const int y = y0 + ip / TW, x = x0 + ip % TW;
                if constexpr (PACKED) {
                    int pn, py, px;
                    off[i] = pk_locate(pk, y, x, pn, py, px)
                                 ? (unsigned)(pn * d.x_img_stride + (py * W + px) * CIN + ich4 * 4) * 4u : xrange;
                } else {
                    off[i] = (FULL || (y < H && x < W)) ? (unsigned)((y * W + x) * CIN + ich4 * 4) * 4u : dxbytes;
                }
            }
            // two separate paths: the plain store must not wait on the vector-memory counter (the next
            // tile's prefetch is in flight and the counter is in-order), only dx += reads memory
            if (d.accumulate_dx) {
                u32x4 old[G::NX];
#pragma unroll
                for (int i = 0; i < G::NX; ++i) old[i] = __builtin_amdgcn_raw_buffer_load_b128(r_dx, off[i], 0, 0);
#pragma unroll
                for (int i = 0; i < G::NX; ++i) {
                    const int ip = (tid + BWD_THREADS * i) / G::C4I;
                    float4 v = *reinterpret_cast<const float4*>(s_a + ip * G::LSI + ich4 * 4);
                    const float4 o = *reinterpret_cast<const float4*>(&old[i]);
                    v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                    __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(&v), r_dx, off[i], 0, PACKED ? 0 : DX_AUX);
                }
            } else {
#pragma unroll
                for (int i = 0; i < G::NX; ++i) {
                    const int ip = (tid + BWD_THREADS * i) / G::C4I;
                    const float4 v = *reinterpret_cast<const float4*>(s_a + ip * G::LSI + ich4 * 4);
                    __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(&v), r_dx, off[i], 0, PACKED ? 0 : DX_AUX);
                }
            }
        }
        __syncthreads();
    }

    // ============ flush per-workgroup partial sums ==============================================
    using Row = DpWgradRow<CIN, COUT>;
    float* row = d.wgrad_partials + (size_t)blockIdx.x * Row::WIDTH;
    // Every wave parks its dW1 tiles in the LDS plane of its K slice and every thread its
    // dW2 | db1 | db2 accumulators in a record (two passes of 6 / 5 float4: 11 at once do not fit next to
    // the planes with 512 threads); the sums over K slices / pixel groups are taken in a fixed order
    // while the row is written.  Three barriers in all.
    float* s_gw1 = sm;                                   // [KSPLIT][COUT][CIN]
    float* red = sm + G::KSPLIT * COUT * CIN;            // [BWD_THREADS][24]
    {
        float* pl = s_gw1 + w1_kslice * COUT * CIN;
#pragma unroll
        for (int j = 0; j < G::MB; ++j)
#pragma unroll
            for (int i = 0; i < G::NB; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pl[(w1_co0 + G::NB * l15 + i) * CIN + w1_ci0 + G::MB * (4 * g + r) + j] = gw1[j * G::NB + i][r];
    }
    float4* my = reinterpret_cast<float4*>(red + tid * 24);
#pragma unroll
    for (int k = 0; k < 6; ++k) my[k] = gw2[k];
    __syncthreads();
    for (int i = tid; i < COUT * CIN; i += BWD_THREADS) {
        float v = 0.0f;
#pragma unroll
        for (int ks = 0; ks < G::KSPLIT; ++ks) v += s_gw1[ks * COUT * CIN + i];
        row[i] = v;
    }
    // record slot k of pass ps: dW2 tap 6*ps + k, then db1, db2
    auto reduce_pass = [&](int ps, int nslot) {
        for (int o = tid; o < COUT * nslot; o += BWD_THREADS) {
            const int c = o / nslot, k = o - c * nslot;
            const int q = c >> 2, e = c & 3;
            float v = 0.0f;
            for (int p = 0; p < G::PG; ++p) v += red[(p * G::C4O + q) * 24 + k * 4 + e];
            const int slot = ps * 6 + k;
            if (slot < 9) row[Row::W2 + c * 9 + slot] = v;
            else if (slot == 9) row[Row::B1 + c] = v;
            else row[Row::B2 + c] = v;
        }
    };
    reduce_pass(0, 6);
    __syncthreads();
    my[0] = gw2[6]; my[1] = gw2[7]; my[2] = gw2[8]; my[3] = gb1; my[4] = gb2;
    __syncthreads();
    reduce_pass(1, 5);
    // (c) BN-backward sums of the producer: one global fp64 atomic per channel
    if constexpr (DET) {
        if (bn_in && d.dx && d.in_bn.bstats && tid < 2 * CIN) bn_det_add(d.in_bn.bstats, CIN, tid, s_bst[tid]);
    } else
    if (bn_in && d.dx && d.in_bn.bstats && tid < 2 * CIN) atomic_add_f64(bn_slot(d.in_bn.bstats, d.in_bn.slots, CIN) + tid, s_bst[tid]);
}
template <int CIN, int COUT, int TH, int TW, bool PACKED = false, int GEMM = 0, bool POOLDY = false, bool FULL = false, bool DET = false>
int launch_dp_bwd(const YunetDP* d, hipStream_t stream) {
    using G = BwdGeom<CIN, COUT, TH, TW, GEMM>;
    if constexpr (FULL) {
        if (d->H % TH != 0 || d->W % TW != 0) return YUNET_EINVAL;
    }
    static PerDevice attr_set;      // per device (common.h)
    PackGeom pk;
    const int grid = dp_bwd_launch_setup<TH, TW, PACKED>(
        d, attr_set, reinterpret_cast<const void*>(dp_bwd_kernel<CIN, COUT, TH, TW, PACKED, GEMM, POOLDY, FULL, DET>), G::SMEM, pk);
    if (grid < 0) return grid;
    static_assert(!DET || YUNET_ACT_DTYPE == YUNET_F32, "deterministic sums: fp32 storage only");
    if (DET && !bn_det_fits(d->in_bn, grid)) return YUNET_EINVAL;
    if (grid < d->wgrad_blocks) {
        // yunet_dp_bwd_blocks() sized the partial buffer for another kernel's grid (the 64 -> 64 units on 8 x 8
        // tiles, while this launch is their exact-fp32 A/B variant on 8 x 16 tiles): the reduction sums every row,
        // so the rows no workgroup of this grid writes are zeroed
        const size_t width = DpWgradRow<CIN, COUT>::WIDTH;
        if (hipMemsetAsync(d->wgrad_partials + (size_t)grid * width, 0, (size_t)(d->wgrad_blocks - grid) * width * 4,
                           stream) != hipSuccess)
            return hip_status();
    }
    hipLaunchKernelGGL((dp_bwd_kernel<CIN, COUT, TH, TW, PACKED, GEMM, POOLDY, FULL, DET>), dim3(grid), dim3(BWD_THREADS), G::SMEM,
                       stream, *d, pk);
    return hip_status();
}

}  // namespace

// map a route (dp_route.h) to its instance; the DET forms exist with fp32 storage only
#ifndef YUNET_ACT_BF16
#define DP_BWD_LAUNCH(ci, co, th_, tw_, pk, g, pl, fl) \
    (r.det ? launch_dp_bwd<ci, co, th_, tw_, pk, g, pl, fl, true>(d, s) : launch_dp_bwd<ci, co, th_, tw_, pk, g, pl, fl>(d, s))
#else
#define DP_BWD_LAUNCH(ci, co, th_, tw_, pk, g, pl, fl) launch_dp_bwd<ci, co, th_, tw_, pk, g, pl, fl>(d, s)
#endif
#define DP_FULL_0(...)
#define DP_FULL_1(...) if (r.full) return DP_BWD_LAUNCH(__VA_ARGS__, true);
extern "C" int ACT_SUFFIX(yunet_dp_bwd)(const YunetDP* d, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    DpRoute r;
    if (const int rc = dp_bwd_route(d, YUNET_ACT_DTYPE, &r)) return rc;
    if (r.family == DP_BWD16S) return ACT_SUFFIX(launch_dp_bwd16s)(d, r, s);
    if (r.family == DP_BWD64) return ACT_SUFFIX(launch_dp_bwd64)(d, r, s);
#define X(ci, co, th_, tw_, pk, g, pl, ft)                   \
    if (DP_BWD_IS(r, ci, co, th_, pk, g, pl)) {              \
        DP_FULL_##ft(ci, co, th_, tw_, pk, g, pl)            \
        return DP_BWD_LAUNCH(ci, co, th_, tw_, pk, g, pl, false); \
    }
    DP_BWD_TILE_INSTANCES(X)
#undef X
    return YUNET_EINVAL;
}
#undef DP_FULL_0
#undef DP_FULL_1
#undef DP_BWD_LAUNCH
