// conv_bwd64.hip -- backward of the 64 -> 64 ConvDPUnit (split-bf16 matrix path).  conv_bwd.hip's dispatcher reaches it through
// launch_dp_bwd64 (common.h).
#include "common.h"
#include "dp_bwd_parts.h"
#include "dp_route.h"

#include <type_traits>

namespace {

// ================================================================================================
// dp_bwd64: the 64 -> 64 ConvDPUnit backward (split-bf16 matrix path), round 3.
//
// Same arithmetic as dp_bwd_kernel<64,64,8,16,PACKED,1,POOLDY> (conv_bwd.hip), re-laid for the two units the round-2
// profile showed busy (VALU 44 %, LDS 38 %, matrix cores 9 %, seven barriers per tile):
//   * every operand is split into bf16 hi / lo ONCE, where it is produced (a = T(x) in the stage, dp at the end
//     of the depthwise phase) and lives in LDS as two XOR-swizzled bf16 planes [pixel][channel]; the three GEMMs
//     read ready-made matrix operands (the old kernel re-split `a` in two GEMMs and `dp` in two);
//   * the p and da GEMMs are split over OUTPUT channels: a wave owns one 16-channel tile and 4 of the 8 pixel
//     tiles, and keeps its W1 / W1^T fragments (hi + lo, 32 registers) for the whole launch -- no weight planes in
//     LDS (37 KB), no weight reads per tile (the old kernel re-read all of W1 from LDS for 16 pixels);
//   * dW1 (K = pixels) takes its operands from the same row-major planes with the gfx950 transposing LDS read
//     (ds_read_b64_tr_b16: a 16-lane group reads a [4 pixels][16 channels] block and each lane receives one
//     channel's 4 pixels) -- no second, transposed copy and no in-register transposition;
//   * the ReLU mask + the producer's BN-backward sums run on the da accumulators in registers (a lane's channel
//     is fixed for the launch: fp64 partials per lane, reduced once at the end -- no LDS atomics);
//   * five barriers per tile.
// LDS: dz halo 45 KB | raw x 32 KB | p / dx staging 32 KB | a planes 32 KB | small tables; the dp planes alias the
// dz halo (dead after the depthwise phase).
namespace bwd64 {
// Round 6: the two fp32 tiles the matrix-layout phases touch with 4-byte accesses (p / dx writes, x reads of the mask) are
// XOR-swizzled: a wave's 32-lane group there is 16 channels x 2 pixel groups 4 pixels apart = 256 words = the SAME banks
// (every such access paid a 2-way conflict); element (pixel, channel) now lives at channel ^ 16 * ((pixel >> 2) & 1).  The
// row-wise 16-byte accesses of the stage / depthwise / store phases see a wave-uniform flip (a wave's four pixels share
// pixel bit 2), so nothing else changes.
__device__ __forceinline__ int tile_swz(int pixel) { return ((pixel >> 2) & 1) << 4; }
// cache-policy bits of the x loads of the unpacked instances: x is read exactly once (tile interior only), non-temporal
// keeps it out of the L2 the dy / z halo re-reads live in (step -0.04 ms, profiles/r06_bench_ab_ntx.log)
constexpr int X_AUX = 2;
constexpr int C = 64, C4 = 16;
constexpr int PLANE_PX = 128;      // (pixels of the largest tile: plane_off() only needs the row pitch)
// NW = waves per workgroup: 8 -> 8 x 16 pixel tiles, one workgroup (149 KB of LDS) per CU;
//                           4 -> 8 x 8 pixel tiles, TWO independent workgroups (80 KB each) per CU, whose phases
//                                interleave on the SIMDs instead of marching in lockstep through five barriers
template <int NW>
struct Geo {
    static constexpr int NT = NW * 64;
    static constexpr int TH = 8, TW = 2 * NW, HW_ = TW + 2, HH_ = TH + 2, HP = HH_ * HW_, IP = TH * TW;
    static constexpr int PSTEP = NT / C4;                              // halo pixels per pass of the workgroup
    // (dy, z) float4 pairs per thread.  NW = 8: 180 halo pixels = 5 full passes + a partial one;
    // NW = 4: 100 = 6 full passes + 4 pixels, which are loaded as ONE float per thread (REM)
    static constexpr int NDZ = NW == 8 ? (HP + PSTEP - 1) / PSTEP : HP / PSTEP;
    static constexpr bool REM = NW == 4;
    static constexpr int REM_HP0 = NDZ * PSTEP;                        // first halo pixel of the remainder
    static constexpr int NX = (IP * C4) / NT;                          // x float4 per thread
    static constexpr int PLANE = IP * C * 2;                           // one bf16 plane
    static constexpr int XP = C;                                       // floats per pixel of the fp32 tiles s_x / s_p
    static constexpr int OFF_DZ = 0;                                   // float [HP][64]; later dp planes hi | lo
    static constexpr int OFF_X = OFF_DZ + HP * C * 4;                  // float [IP][XP] raw x
    static constexpr int OFF_P = OFF_X + IP * XP * 4;                  // float [IP][XP] p, later the masked dx
    static constexpr int OFF_A = OFF_P + IP * XP * 4;                  // bf16 planes hi | lo of a = T(x)
    static constexpr int WORKB = OFF_A + 2 * PLANE;
    static constexpr int PAR_F = 9 * C + 7 * C + 5 * C + C;            // w2 | out-bn | in-bn | b1 (floats)
    static constexpr int MH = NW / 4;                                  // pixel halves (p / da GEMM: 4 pixel tiles per wave)
    static constexpr int SMEM = WORKB + PAR_F * 4 + MH * 2 * C * 8 + IP;   // + fp64 sums per pixel half + validity bytes
    static constexpr int KSPLIT = NW / 4;                              // dW1: pixels 64 ks .. 64 ks + 63 per wave quad
    static_assert(2 * PLANE <= HP * C * 4, "dp planes alias the dz halo");
    static_assert((size_t)KSPLIT * C * C * 4 + (size_t)NT * 24 * 4 <= (size_t)WORKB, "flush area");
    static_assert(!REM || (HP - REM_HP0) * C == NT, "remainder: one float per thread");
    static_assert(IP % 64 == 0 && NX * NT == IP * C4, "tile mapping");
};
using Row = DpWgradRow<C, C>;        // the workgroup's row of wgrad_partials
// byte offset of channels 8*chunk .. 8*chunk+7 of pixel `pix` inside a plane (16-byte chunks, XOR-swizzled so
// that both the row-wise 16-byte operand reads and the transposing reads are bank-conflict free)
__device__ __forceinline__ int plane_off(int pix, int chunk) { return pix * (C * 2) + ((chunk ^ (pix & 7)) << 4); }
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
// [4 pixels][16 channels] block, transposed: this lane's channel, 4 consecutive pixels (see tools/ubench/tr_probe.hip)
__device__ __forceinline__ u32x2 tr_read(const unsigned char* p) {
    const bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        reinterpret_cast<__attribute__((address_space(3))) bf16x4*>(
            (__attribute__((address_space(3))) unsigned char*)p));
    return __builtin_bit_cast(u32x2, v);
}
// bf16 activation storage (YUNET_ACT_BF16): the forward of this mode multiplied
// bf16(a) with bf16(W1) (conv_fwd64.hip), so the backward that is consistent with it recomputes p as that ONE product,
// takes dW1 = bf16(a)^T dp as two (dp = hi + lo) and da = dp bf16(W1) as two: 5 matrix products per tile instead of 9,
// and the low plane of `a` is neither written nor read
// (round 5; against the earlier variant, which split the fp32 a and W1 as the fp32 build does:
// same-box A/B of the bf16 step 4.00 -> 3.89 ms, profiles/r05_bf16_lean_ab.log)
#ifdef YUNET_ACT_BF16
constexpr bool BWD64_LEAN = true;
#else
constexpr bool BWD64_LEAN = false;
#endif
__device__ __forceinline__ f32x4 mfma1r(const u32x4 a, const u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma3r(const u32x4 ah, const u32x4 al, const u32x4 bh, const u32x4 bl, f32x4 c) {
    const bf16x8 xh = __builtin_bit_cast(bf16x8, ah), xl = __builtin_bit_cast(bf16x8, al);
    const bf16x8 yh = __builtin_bit_cast(bf16x8, bh), yl = __builtin_bit_cast(bf16x8, bl);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, yh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, yl, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, yh, c, 0, 0, 0);
    return c;
}
}  // namespace bwd64

// DET (YUNET_DET_FAST in the producer's YunetBN::det_rows): the workgroup's sums -- already added up in a fixed order -- go to
// its own row of the [1 + R][2C] block (common.h: bn_det_add) instead of one fp64 atomic per channel; nothing else differs.
template <int NW, bool PACKED, bool POOLDY, bool DET = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))     // 256 registers per lane: 8 waves per CU
void dp_bwd64_kernel(const YunetDP d, const PackGeom pk) {
    using namespace bwd64;
    using G = Geo<NW>;
    constexpr int NT = G::NT, TH = G::TH, TW = G::TW, HW_ = G::HW_, HP = G::HP, IP = G::IP, NDZ = G::NDZ, NX = G::NX;
    constexpr int PSTEP = G::PSTEP, PLANE = G::PLANE, OFF_DZ = G::OFF_DZ, OFF_X = G::OFF_X, OFF_P = G::OFF_P;
    constexpr int OFF_A = G::OFF_A, WORKB = G::WORKB, KSPLIT = G::KSPLIT, MH = G::MH, XP = G::XP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* s_dz = reinterpret_cast<float*>(smem_raw + OFF_DZ);
    float* s_x = reinterpret_cast<float*>(smem_raw + OFF_X);
    float* s_p = reinterpret_cast<float*>(smem_raw + OFF_P);
    unsigned char* s_a = smem_raw + OFF_A;                 // planes of a: hi at 0, lo at PLANE
    unsigned char* s_d = smem_raw + OFF_DZ;                // planes of dp (alias the dz halo)
    float* s_w2 = reinterpret_cast<float*>(smem_raw + WORKB);      // [9][64]
    float* s_co = s_w2 + 9 * C;                            // folded BN backward of the unit's own BN: A|B|Dh|Dl (+3 spare rows)
    float* s_ci = s_co + 7 * C;                            // mean|scale|beta|invstd|mean_lo
    float* s_b1 = s_ci + 5 * C;                            // [64] pointwise bias
    double* s_bst = reinterpret_cast<double*>(s_b1 + C);   // [MH pixel halves][2][64]
    unsigned char* s_in = reinterpret_cast<unsigned char*>(s_bst + MH * 2 * C);  // [IP] packed mode: pixel is real

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: everything derived from it lives in SGPRs
    const int l15 = lane & 15, g = lane >> 4;
    const int H = d.H, W = d.W;
    const bool bn_in = d.in_transform == YUNET_T_BNRELU;
    const bool bn_out = d.out_has_bn != 0;
    const float relu_floor = bn_in ? 0.0f : -__builtin_inff();
    // debug ablation mask (tools/kbench.py --ablate): prof < 4096 is a bit mask, not a pointer
    const unsigned abl = (unsigned long long)d.prof < 4096ull ? (unsigned)(unsigned long long)d.prof : 0u;
    const int tiles_x = ((PACKED ? pk.CW : W) + TW - 1) / TW, tiles_y = ((PACKED ? pk.CH : H) + TH - 1) / TH;
    const int tiles_img = tiles_x * tiles_y;
    const int ntiles = PACKED ? tiles_img : d.N * tiles_img;
    auto inside = [&](int ip, int y, int x) {
        if constexpr (PACKED) return s_in[ip] != 0;
        else return y < H && x < W;
    };

    // ---- prefetch registers (next tile): raw dy / z_out over the halo, x over the interior -- as in dp_bwd_kernel
    float4 pdy[NDZ];
    act_raw4 pz[NDZ], px[NX];
    unsigned okmask = 0;
    static_assert(!(POOLDY && PACKED), "pooled dy: unpacked levels only");
    unsigned pid[POOLDY ? NDZ : 1];
    float rem_dy = 0.0f, rem_z = 0.0f;        // NW = 4: the last 4 halo pixels, one float per thread
    unsigned rem_id = 0;
    const int Wq = W >> 1;
    const unsigned pooledbytes = (unsigned)((H >> 1) * Wq * C) * 4u;
    const unsigned dybytes = (unsigned)(H * W * C) * 4u, zbytes = (unsigned)(H * W * C) * ACT_B;
    const unsigned xbytes = (unsigned)(H * W * C) * ACT_B, dxbytes = (unsigned)(H * W * C) * 4u;
    // packed canvas (20 x 20 / 10 x 10 levels): descriptors over the whole tensors, the image index is part of the offset
    auto issue_packed = [&](int t, auto part_c) {
        constexpr int PART = decltype(part_c)::value;
        const int tid = opaque((int)threadIdx.x);
        const int och4 = tid % C4;
        const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
        const unsigned dyrange = (unsigned)d.N * (unsigned)d.z_img_stride * 4u;
        const unsigned zrange = (unsigned)d.N * (unsigned)d.z_img_stride * ACT_B;
        const unsigned xrange = (unsigned)d.N * (unsigned)d.x_img_stride * ACT_B;
        const auto r_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.dy), 0, dyrange, 0x00020000);
        const auto r_z = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<act_t*>(const_cast<float*>(d.z)), 0, zrange, 0x00020000);
        const auto r_x = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<act_t*>(const_cast<float*>(d.x)), 0, xrange, 0x00020000);
        if (PART <= 0) okmask = 0;
#pragma unroll
        for (int i = 0; i < NDZ; ++i) {
            if (PART >= 0 && PART != 1 + (3 * i) / NDZ) continue;
            const int hp = tid / C4 + PSTEP * i;
            const int hy = hp / HW_, hx = hp - hy * HW_;
            int pn, py, pxx;
            const bool ok = hp < HP && pk_locate(pk, y0 - 1 + hy, x0 - 1 + hx, pn, py, pxx);
            const unsigned eo = (unsigned)(pn * d.z_img_stride + (py * W + pxx) * C + och4 * 4);
            okmask |= ok ? (1u << i) : 0u;
            const u32x4 vdy = __builtin_amdgcn_raw_buffer_load_b128(r_dy, ok ? eo * 4u : dyrange, 0, 0);
            pdy[i] = *reinterpret_cast<const float4*>(&vdy);
            pz[i] = act_raw4{};
            if (bn_out) pz[i] = act_bufld4(r_z, ok ? eo * ACT_B : zrange);
            // finish one slot's address arithmetic before the next one starts (as in dp_bwd_kernel)
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (G::REM) {
            if (PART < 0 || PART == 3) {
                const int hp = G::REM_HP0 + tid / C, ch = tid % C;
                const int hy = hp / HW_, hx = hp - hy * HW_;
                int pn, py, pxx;
                const bool ok = pk_locate(pk, y0 - 1 + hy, x0 - 1 + hx, pn, py, pxx);
                const unsigned eo = (unsigned)(pn * d.z_img_stride + (py * W + pxx) * C + ch);
                okmask |= ok ? (1u << NDZ) : 0u;
                rem_dy = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r_dy, ok ? eo * 4u : dyrange, 0, 0));
                rem_z = 0.0f;
                if (bn_out) rem_z = act_bufld1(r_z, ok ? eo * ACT_B : zrange);
            }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            if (PART > 0) continue;
            const int ip = tid / C4 + PSTEP * i;
            int pn, py, pxx;
            const unsigned off = pk_locate(pk, y0 + ip / TW, x0 + ip % TW, pn, py, pxx)
                                     ? (unsigned)(pn * d.x_img_stride + (py * W + pxx) * C + och4 * 4) * ACT_B : xrange;
            px[i] = act_bufld4(r_x, off);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // ---- round 5 (unpacked maps): the same loads with a shift-only thread -> halo-slot mapping ------------------
    // The old mapping (halo pixel hp = tid / 16 + 32 i, row hp / 18) cost a division by the halo width, ~15 vector and
    // ~15 scalar instructions per load -- 16 loads per thread and tile, a quarter of the tile's VALU work, and every one
    // of the four issue pieces decomposed the tile index again.  Here the halo [TH + 2][TW + 2] is split into its TW-wide
    // main part -- pixel slot ps = tid / 16 of pass i < 5 is halo row 2 i + (ps >> log2 TW), column ps & (TW - 1) -- and
    // the two extra columns TW, TW + 1 (pass 5: row ps >> 1, column TW + (ps & 1); with NW = 4 their rows 8, 9 are the
    // one-float-per-thread remainder): a thread's element offset is ONE tile-invariant value `tm` plus a scalar per
    // (tile, pass), the interior loads use the same `tm`, and a uniform branch drops every per-element validity test
    // when the whole halo lies inside the image (48 % of the 80 x 80 tiles, 36 % at 40 x 40).
    constexpr int XSH = NW == 8 ? 4 : 3;                    // log2(TW)
    constexpr int NEXTRA = NW == 8 ? 20 : 16;               // halo pixels of the extra pass (NW = 8: 20 of 32 slots)
    static_assert(PACKED || (NDZ == 6 && NX == 4 && PSTEP == 2 * TW && (1 << XSH) == TW), "issue_unpacked pass geometry");
    auto issue_unpacked = [&](int t, auto part_c) {
        constexpr int PART = decltype(part_c)::value;
        const int tid = opaque((int)threadIdx.x);
        const int och4 = tid & 15, ps = tid >> 4;
        const int r = ps >> XSH, hxm = ps & (TW - 1);
        const int n = t / tiles_img, rr = t - n * tiles_img;
        const int ty = rr / tiles_x;
        const int y0 = ty * TH, x0 = (rr - ty * tiles_x) * TW;
        const size_t zbase = (size_t)n * d.z_img_stride, xbase = (size_t)n * d.x_img_stride;
        const auto r_dy = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(d.dy) + (POOLDY ? (size_t)n * (pooledbytes / 4u) : zbase), 0, POOLDY ? pooledbytes : dybytes, 0x00020000);
        const auto r_id = __builtin_amdgcn_make_buffer_rsrc(
            d.pool_idx + (POOLDY ? (size_t)n * (pooledbytes / 4u) : (size_t)0), 0, POOLDY ? pooledbytes / 4u : 0u, 0x00020000);
        const auto r_z = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<act_t*>(const_cast<float*>(d.z)) + zbase, 0, zbytes, 0x00020000);
        const auto r_x = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<act_t*>(const_cast<float*>(d.x)) + xbase, 0, xbytes, 0x00020000);
        const bool inner = y0 > 0 && x0 > 0 && y0 + TH < H && x0 + TW < W;      // uniform: the halo is inside the image
        if (PART <= 0) okmask = 0;
        const int tm = (r * W + hxm) * C + och4 * 4;              // elements from slot (row 0, column 0) of a pass
        const int hbase = ((y0 - 1) * W + (x0 - 1)) * C;          // halo origin (negative on the top / left border: masked)
        // pooled dy: halo slot (hy, hx) reads the pooled element ((y0 - 1 + hy) >> 1, (x0 - 1 + hx) >> 1); y0, x0 even
        const int tq = (r * Wq + ((hxm - 1) >> 1)) * C + och4 * 4;
        const int qbase = (((y0 >> 1) - 1) * Wq + (x0 >> 1)) * C;
        auto ld = [&](int i, bool ok, unsigned eo, unsigned eq) {
            if constexpr (POOLDY) {
                const u32x4 vdy = __builtin_amdgcn_raw_buffer_load_b128(r_dy, ok ? eq * 4u : pooledbytes, 0, 0);
                pdy[i] = *reinterpret_cast<const float4*>(&vdy);
                pid[i] = __builtin_amdgcn_raw_buffer_load_b32(r_id, ok ? eq : pooledbytes, 0, 0);
            } else {
                const u32x4 vdy = __builtin_amdgcn_raw_buffer_load_b128(r_dy, ok ? eo * 4u : dybytes, 0, 0);
                pdy[i] = *reinterpret_cast<const float4*>(&vdy);
            }
            pz[i] = act_raw4{};
            if (bn_out) pz[i] = act_bufld4(r_z, ok ? eo * ACT_B : zbytes);
        };
        auto body = [&](auto inner_c) {
            constexpr bool INNER = decltype(inner_c)::value;
            const bool xok_m = INNER || (unsigned)(x0 - 1 + hxm) < (unsigned)W;
#pragma unroll
            for (int i = 0; i < NDZ; ++i) {
                if (PART >= 0 && PART != 1 + (3 * i) / NDZ) continue;
                if (i < 5) {
                    const bool ok = INNER || (xok_m && (unsigned)(y0 - 1 + 2 * i + r) < (unsigned)H);
                    okmask |= ok ? (1u << i) : 0u;
                    ld(i, ok, (unsigned)(hbase + i * 2 * W * C + tm), (unsigned)(qbase + i * Wq * C + tq));
                } else {
                    const int hy = ps >> 1, hx = TW + (ps & 1);
                    const bool ok = ps < NEXTRA && (INNER || ((unsigned)(y0 - 1 + hy) < (unsigned)H &&
                                                              (unsigned)(x0 - 1 + hx) < (unsigned)W));
                    okmask |= ok ? (1u << i) : 0u;
                    ld(i, ok, (unsigned)(hbase + (hy * W + hx) * C + och4 * 4),
                       (unsigned)(qbase + ((((hy - 1) >> 1) + 1) * Wq + ((hx - 1) >> 1)) * C + och4 * 4));
                }
            }
            if constexpr (G::REM) {
                if (PART < 0 || PART == 3) {
                    const int j = tid >> 6, ch = tid & 63;
                    const int hy = TH + (j >> 1), hx = TW + (j & 1);
                    const bool ok = INNER || ((unsigned)(y0 - 1 + hy) < (unsigned)H && (unsigned)(x0 - 1 + hx) < (unsigned)W);
                    const unsigned eo = (unsigned)(hbase + (hy * W + hx) * C + ch);
                    okmask |= ok ? (1u << NDZ) : 0u;
                    if constexpr (POOLDY) {
                        const unsigned eq = (unsigned)(qbase + ((((hy - 1) >> 1) + 1) * Wq + ((hx - 1) >> 1)) * C + ch);
                        rem_dy = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r_dy, ok ? eq * 4u : pooledbytes, 0, 0));
                        rem_id = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(r_id, ok ? eq : pooledbytes, 0, 0) & 0xffu;
                    } else {
                        rem_dy = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r_dy, ok ? eo * 4u : dybytes, 0, 0));
                    }
                    rem_z = 0.0f;
                    if (bn_out) rem_z = act_bufld1(r_z, ok ? eo * ACT_B : zbytes);
                }
            }
        };
        if (PART != 0) {
            if (inner) body(std::true_type{});
            else body(std::false_type{});
        }
        if (PART <= 0) {
            // raw x over the tile: pass i covers tile rows 2 i, 2 i + 1 -- the same `tm`
            const bool tfull = y0 + TH <= H && x0 + TW <= W;
            const int xb = (y0 * W + x0) * C;
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const bool ok = tfull || (y0 + 2 * i + r < H && x0 + hxm < W);
                px[i] = act_bufld4<X_AUX>(r_x, ok ? (unsigned)(xb + i * 2 * W * C + tm) * ACT_B : xbytes);
            }
        }
    };
    // round 6: every piece one issue point LATER than in rounds 2-5 (x after the depthwise phase ... the last third of dy / z
    // between the da GEMM and the mask): the requests spend less time queued in a memory system that is already
    // oversubscribed by 256 CUs prefetching a whole tile each -- issuing EARLIER (inside the stage, into the registers it
    // frees: built, +23 %) or all at once (+3 %) is worse, later is neutral at 80 x 80 and -1 .. -3 % on the smaller maps
    // (profiles/r06_bwd64_pf5.log)
    auto issue = [&](int t, auto part_c) {
        if constexpr (PACKED) issue_packed(t, part_c);
        else issue_unpacked(t, part_c);
    };
    using All = std::integral_constant<int, -1>;
    int t = first_tile();

    // ---- this wave's weight fragments, straight from global memory into registers ------------------------------
    // p = a * W1^T and da = dp * W1: wave `wid` owns output-channel tile nt = wid & 3 of both GEMMs and the pixel
    // tiles 4 * (wid >> 2) .. + 3.  B operand of v_mfma_f32_16x16x32_bf16: lane (l15, g) supplies column l15,
    // k = 32 kb + 8 g .. + 7.
    // The weight loads (L2 hits after the first workgroups) are issued BEFORE the first tile's 16 loads per thread
    // and consumed after: vector-memory returns are counted in order, so weights queued behind a cold-start tile
    // would wait for all of HBM's latency before the first split could run.
    const int nt = wid & 3, mh = wid >> 2;
    u32x4 w1h[2], w1l[2], wth[2], wtl[2];
    {
        const int co = nt * 16 + l15;             // p GEMM: column = output channel, k = input channel
        const int ci = nt * 16 + l15;             // da GEMM: column = input channel, k = output channel
        float4 ra[2], rb[2];
        float rt[2][8];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            ra[kb] = *reinterpret_cast<const float4*>(d.w_pw + co * C + 32 * kb + 8 * g);
            rb[kb] = *reinterpret_cast<const float4*>(d.w_pw + co * C + 32 * kb + 8 * g + 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) rt[kb][j] = d.w_pw[(32 * kb + 8 * g + j) * C + ci];
        }
        if (t < ntiles) issue(t, All{});
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const float w8[8] = {ra[kb].x, ra[kb].y, ra[kb].z, ra[kb].w, rb[kb].x, rb[kb].y, rb[kb].z, rb[kb].w};
            const Split8 sp = split8(w8);
            w1h[kb] = sp.hi; w1l[kb] = sp.lo;
            const Split8 st = split8(rt[kb]);
            wth[kb] = st.hi; wtl[kb] = st.lo;
        }
    }
    for (int c = tid; c < C; c += NT) s_b1[c] = d.b_pw[c];
    staged_table<C * 9, NT>(d.w_dw, tid, [&](int i, float w) { s_w2[(i % 9) * C + i / 9] = w; });
    for (int c = tid; c < C; c += NT) {
        // the sums of both BatchNorms in flight together (as bn_bwd_coef() then bn_coef() they were five rounds of eight
        // loads, each waited out before the next was issued)
        BNBwdRaw oraw;
        BNCoefRaw iraw;
        if (bn_out) oraw = bn_bwd_coef_issue(d.out_bn, C, c);
        if (bn_in) iraw = bn_coef_issue(d.in_bn, C, c);
        // dz = k1 * (dy - c1 - xhat * c2) folded into dz = A dy + B z + D (bn_fold in common.h): two FMAs and an
        // add per element instead of nine operations
        if (bn_out) {
            const BNFold f = bn_fold(bn_bwd_coef_finish(d.out_bn, C, c, oraw));
            s_co[c] = f.a; s_co[C + c] = f.b; s_co[2 * C + c] = f.dh; s_co[3 * C + c] = f.dl;
        } else {
            s_co[c] = d.dy_scale ? d.dy_scale[c] : 1.0f;
            s_co[C + c] = 0.f; s_co[2 * C + c] = 0.f; s_co[3 * C + c] = 0.f;
        }
        if (bn_in) {
            const BNCoef k = bn_coef_finish(d.in_bn, C, c, iraw);
            s_ci[c] = k.mean; s_ci[C + c] = k.scale; s_ci[2 * C + c] = k.beta;
            s_ci[3 * C + c] = k.invstd; s_ci[4 * C + c] = k.mean_lo;
        } else {
            s_ci[c] = 0.f; s_ci[C + c] = 1.f; s_ci[2 * C + c] = 0.f; s_ci[3 * C + c] = 1.f; s_ci[4 * C + c] = 0.f;
        }
    }
    __syncthreads();

    // ---- persistent accumulators ----------------------------------------------------------------------------------
    float4 gw2[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) gw2[k] = make_float4(0, 0, 0, 0);
    float4 gb2 = make_float4(0, 0, 0, 0), gb1 = make_float4(0, 0, 0, 0);
    // dW1 (K = pixels): wave quad ks = wid >> 2 takes pixels 64 ks .. 64 ks + 63; wave (wid & 3) of a quad owns the
    // 2 x 2 block of 16 x 16 tiles  ci tiles 2 * (grp >> 1) + {0, 1}  x  co tiles 2 * (grp & 1) + {0, 1}
    f32x4 gw1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) gw1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int w1_ct = 2 * ((wid & 3) >> 1), w1_ot = 2 * (wid & 1), w1_ks = wid >> 2;
    // producer's BN-backward sums: fp64, one private LDS slot per (pixel half, channel) -- wave (mh, nt) owns
    // channels nt * 16 .. + 15 of half mh, so plain read-modify-write (as registers they cost 4 VGPRs)
    for (int i = tid; i < MH * 2 * C; i += NT) s_bst[i] = 0.0;

    const bool pf_on = !(abl & 32);
    for (; t < ntiles; t += gridDim.x) {
        const int n = PACKED ? 0 : t / tiles_img, rr = t - n * tiles_img;
        const int y0 = (rr / tiles_x) * TH, x0 = (rr % tiles_x) * TW;
        // every pixel of the tile is a real pixel (all tiles of an 80 x 80 map, and of a 40 x 40 one with 8 x 8
        // tiles): the per-element validity tests -- hundreds of integer instructions per tile -- are skipped
        const bool tile_full = !PACKED && y0 + TH <= H && x0 + TW <= W;

        // ---- stage: dz = BN backward of this unit's own BN -> LDS; x raw -> LDS; a = T(x) split -> planes ---------
        {
            const int tid = opaque((int)threadIdx.x);
            const int och4 = tid % C4;
            const float4 o_a = *reinterpret_cast<float4*>(s_co + och4 * 4);
            const float4 o_b = *reinterpret_cast<float4*>(s_co + C + och4 * 4);
            const float4 o_dh = *reinterpret_cast<float4*>(s_co + 2 * C + och4 * 4);
            const float4 o_dl = *reinterpret_cast<float4*>(s_co + 3 * C + och4 * 4);
            const int hp0 = tid / C4;
            if constexpr (!PACKED) {
                // the slots of issue_unpacked: pass i < 5 -> halo row 2 i + r, column hxm; pass 5 -> the two extra columns
                const int ps = tid >> 4, r = ps >> XSH, hxm = ps & (TW - 1);
                const bool inner = y0 > 0 && x0 > 0 && y0 + TH < H && x0 + TW < W;
                float* const lm = s_dz + (r * HW_ + hxm) * C + och4 * 4;
                auto fold = [&](auto inner_c) {
                    constexpr bool INNER = decltype(inner_c)::value;
#pragma unroll
                    for (int i = 0; i < NDZ; ++i) {
                        const int hy = ps >> 1, hx = TW + (ps & 1);         // (pass 5)
                        if (i < 5 || ps < NEXTRA) {
                            float4 dy = pdy[i];
                            const float4 z = act_unpack(pz[i]);
                            if constexpr (POOLDY) {
                                // window position of the slot: y0, x0 are even, so the parities are the slot's own
                                const unsigned pos = i < 5 ? (unsigned)(((r ^ 1) << 1) | ((hxm + 1) & 1))
                                                           : (unsigned)((((hy + 1) & 1) << 1) | ((ps & 1) ^ 1));
                                const unsigned id = pid[i];
                                dy.x = (id & 0xffu) == pos ? dy.x : 0.0f;
                                dy.y = ((id >> 8) & 0xffu) == pos ? dy.y : 0.0f;
                                dy.z = ((id >> 16) & 0xffu) == pos ? dy.z : 0.0f;
                                dy.w = (id >> 24) == pos ? dy.w : 0.0f;
                            }
                            // zero padding of dz: a slot outside the image loaded dy = z = 0, which the BN backward
                            // would turn into D
                            const bool ok = INNER || ((okmask >> i) & 1u);
                            float4 v;
                            v.x = ok ? fmaf(o_a.x, dy.x, fmaf(o_b.x, z.x, o_dh.x)) + o_dl.x : 0.0f;
                            v.y = ok ? fmaf(o_a.y, dy.y, fmaf(o_b.y, z.y, o_dh.y)) + o_dl.y : 0.0f;
                            v.z = ok ? fmaf(o_a.z, dy.z, fmaf(o_b.z, z.z, o_dh.z)) + o_dl.z : 0.0f;
                            v.w = ok ? fmaf(o_a.w, dy.w, fmaf(o_b.w, z.w, o_dh.w)) + o_dl.w : 0.0f;
                            float* dst = i < 5 ? lm + i * 2 * HW_ * C : s_dz + (hy * HW_ + hx) * C + och4 * 4;
                            *reinterpret_cast<float4*>(dst) = v;
                        }
                    }
                    if constexpr (G::REM) {
                        const int j = tid >> 6, ch = tid & 63;
                        const int hp = (TH + (j >> 1)) * HW_ + TW + (j & 1);
                        float dyv = rem_dy;
                        if constexpr (POOLDY) dyv = rem_id == (unsigned)((((j >> 1) ^ 1) << 1) | ((j & 1) ^ 1)) ? dyv : 0.0f;
                        const bool ok = INNER || ((okmask >> NDZ) & 1u);
                        s_dz[hp * C + ch] = ok ? fmaf(s_co[ch], dyv, fmaf(s_co[C + ch], rem_z, s_co[2 * C + ch])) + s_co[3 * C + ch] : 0.0f;
                    }
                };
                if (inner) fold(std::true_type{});
                else fold(std::false_type{});
            } else {
#pragma unroll
            for (int i = 0; i < NDZ; ++i) {
                const int hp = hp0 + PSTEP * i;
                if ((i + 1) * PSTEP <= HP || hp < HP) {
                    const float4 dy = pdy[i];
                    const float4 z = act_unpack(pz[i]);
                    // zero padding of dz: a slot outside the image loaded dy = z = 0, which the BN backward
                    // would turn into D
                    const bool ok = (okmask >> i) & 1u;
                    float4 v;
                    v.x = ok ? fmaf(o_a.x, dy.x, fmaf(o_b.x, z.x, o_dh.x)) + o_dl.x : 0.0f;
                    v.y = ok ? fmaf(o_a.y, dy.y, fmaf(o_b.y, z.y, o_dh.y)) + o_dl.y : 0.0f;
                    v.z = ok ? fmaf(o_a.z, dy.z, fmaf(o_b.z, z.z, o_dh.z)) + o_dl.z : 0.0f;
                    v.w = ok ? fmaf(o_a.w, dy.w, fmaf(o_b.w, z.w, o_dh.w)) + o_dl.w : 0.0f;
                    *reinterpret_cast<float4*>(s_dz + hp * C + och4 * 4) = v;
                }
            }
            if constexpr (G::REM) {
                const int hp = G::REM_HP0 + tid / C, ch = tid % C;
                const bool ok = (okmask >> NDZ) & 1u;
                s_dz[hp * C + ch] = ok ? fmaf(s_co[ch], rem_dy, fmaf(s_co[C + ch], rem_z, s_co[2 * C + ch])) + s_co[3 * C + ch] : 0.0f;
            }
            }
            if constexpr (PACKED) {
                for (int ip = tid; ip < IP; ip += NT) {
                    int pn, py, pxx;
                    s_in[ip] = pk_locate(pk, y0 + ip / TW, x0 + ip % TW, pn, py, pxx) ? 1 : 0;
                }
            }
            const float4 i_mean = *reinterpret_cast<float4*>(s_ci + och4 * 4);
            const float4 i_scale = *reinterpret_cast<float4*>(s_ci + C + och4 * 4);
            const float4 i_beta = *reinterpret_cast<float4*>(s_ci + 2 * C + och4 * 4);
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const int ip = hp0 + PSTEP * i;
                const float4 xv = act_unpack(px[i]);
                *reinterpret_cast<float4*>(s_x + ip * XP + ((och4 * 4) ^ tile_swz(hp0))) = xv;
                unsigned h0, l0, h1, l1;
                split2(tin(xv.x, i_mean.x, i_scale.x, i_beta.x, relu_floor),
                       tin(xv.y, i_mean.y, i_scale.y, i_beta.y, relu_floor), h0, l0);
                split2(tin(xv.z, i_mean.z, i_scale.z, i_beta.z, relu_floor),
                       tin(xv.w, i_mean.w, i_scale.w, i_beta.w, relu_floor), h1, l1);
                unsigned char* ap = s_a + plane_off(ip, och4 >> 1) + (och4 & 1) * 8;
                *reinterpret_cast<u32x2*>(ap) = u32x2{h0, h1};
                if (!BWD64_LEAN) *reinterpret_cast<u32x2*>(ap + PLANE) = u32x2{l0, l1};
            }
        }
        __syncthreads();
        const bool more = t + (int)gridDim.x < ntiles && pf_on;

        // ---- p = a * W1^T + b1: this wave's 16 output channels on 4 pixel tiles -------------------------------------
        if (!(abl & 1)) {
            const int l15o = opaque(l15), go = opaque(g);
            const unsigned char* abase = s_a + (mh * 64 + l15o) * (C * 2);
            const int sw = l15o & 7;
            const float bias1 = s_b1[nt * 16 + l15o];
            f32x4 acc[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) acc[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {           // four independent accumulator chains per k block
                u32x4 ah[4], al[4];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    const unsigned char* ap = abase + mi * 16 * (C * 2) + (((4 * kb + go) ^ sw) << 4);
                    ah[mi] = *reinterpret_cast<const u32x4*>(ap);
                    if (!BWD64_LEAN) al[mi] = *reinterpret_cast<const u32x4*>(ap + PLANE);
                }
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    acc[mi] = BWD64_LEAN ? mfma1r(ah[mi], w1h[kb], acc[mi]) : mfma3r(ah[mi], al[mi], w1h[kb], w1l[kb], acc[mi]);
                __builtin_amdgcn_sched_barrier(0);
            }
            float* pw = s_p + (mh * 64 + 4 * go) * XP + ((nt * 16 + l15o) ^ tile_swz(4 * go));
            if (tile_full) {
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pw[(mi * 16 + r) * XP] = acc[mi][r] + bias1;
            } else {
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ip = (mh * 4 + mi) * 16 + 4 * go + r;
                        const bool in = inside(ip, y0 + ip / TW, x0 + ip % TW);
                        pw[(mi * 16 + r) * XP] = in ? acc[mi][r] + bias1 : 0.0f;
                    }
            }
        }
        __syncthreads();

        // ---- depthwise backward on the VALU (sliding window over a 4-row column); dp stays in registers -------------
        float4 dp[4];
        int d_pix0;
        {
            const int tv = opaque((int)threadIdx.x);
            const int cq = tv % C4, pg = tv / C4;
            const int vtx = pg % TW, vr0 = (pg / TW) * 4;
            d_pix0 = vr0 * TW + vtx;
            const float* zb = s_dz + (vr0 * HW_ + vtx) * C + cq * 4;
            const float* pb = s_p + (vr0 * TW + vtx) * XP + ((cq * 4) ^ tile_swz(vtx));
            const float* wb = s_w2 + cq * 4;
            float4 pv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pv[r] = *reinterpret_cast<const float4*>(pb + r * TW * XP);
                dp[r] = make_float4(0, 0, 0, 0);
            }
            if (!(abl & 2)) {
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    float4 wk[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                        wk[a] = *reinterpret_cast<const float4*>(wb + (8 - (3 * a + b)) * C);
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        const float4 z4 = *reinterpret_cast<const float4*>(zb + (j * HW_ + b) * C);
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            const int r = j - a;
                            if (r < 0 || r >= 4) continue;
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
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (!tile_full) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool in = inside((vr0 + r) * TW + vtx, y0 + vr0 + r, x0 + vtx);
                    if (!in) dp[r] = make_float4(0, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                gb1.x += dp[r].x; gb1.y += dp[r].y; gb1.z += dp[r].z; gb1.w += dp[r].w;
            }
        }
        // next tile's loads go out in four pieces from here on (the p GEMM and the depthwise phase above run with no
        // load in flight: a CU cannot keep a whole tile's 124 KB in flight, and the in-order vector-memory queue would
        // hold any scratch access behind them)
        if (more) issue(t + gridDim.x, std::integral_constant<int, 0>{});
        __syncthreads();      // every dz read is done: the dp planes may overwrite the halo
        {
            const int cq = opaque((int)threadIdx.x) % C4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pix = d_pix0 + r * TW;
                unsigned h0, l0, h1, l1;
                split2(dp[r].x, dp[r].y, h0, l0);
                split2(dp[r].z, dp[r].w, h1, l1);
                unsigned char* q = s_d + plane_off(pix, cq >> 1) + (cq & 1) * 8;
                *reinterpret_cast<u32x2*>(q) = u32x2{h0, h1};
                *reinterpret_cast<u32x2*>(q + PLANE) = u32x2{l0, l1};
            }
        }
        __syncthreads();
        if (more) issue(t + gridDim.x, std::integral_constant<int, 1>{});

        // ---- dW1 += a^T * dp (K = pixels): operands through the transposing LDS read --------------------------------
        // k index of lane group G, element e (0..7): pixel 32 kb + 4 * (4 (G >> 1) + 2 (e >> 2) + (G & 1)) + (e & 3) --
        // the two 4-pixel blocks a 32-lane half reads in one instruction then differ in pixel bit 2, which the
        // plane swizzle turns into different banks (any k order is valid as long as A and B agree)
        if (!(abl & 4)) {
            const int lo_ = opaque(lane);
            const int i16 = lo_ & 15, G = lo_ >> 4;
            const int prow = 4 * (4 * (G >> 1) + (G & 1)) + (i16 >> 2);          // + 8 for the second read
            const int sub = i16 & 3;                                              // 4-channel quad inside the 16-channel tile
#pragma unroll
            for (int kbi = 0; kbi < 2; ++kbi) {
                const int p0 = 64 * w1_ks + 32 * kbi + prow;
                u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
                for (int tI = 0; tI < 2; ++tI) {
                    const int chA = 2 * (w1_ct + tI) + (sub >> 1), chB = 2 * (w1_ot + tI) + (sub >> 1);
                    const unsigned char* a0 = s_a + plane_off(p0, chA) + (sub & 1) * 8;
                    const unsigned char* a1 = s_a + plane_off(p0 + 8, chA) + (sub & 1) * 8;
                    const unsigned char* b0 = s_d + plane_off(p0, chB) + (sub & 1) * 8;
                    const unsigned char* b1 = s_d + plane_off(p0 + 8, chB) + (sub & 1) * 8;
                    const u32x2 ah0 = tr_read(a0), ah1 = tr_read(a1);
                    u32x2 al0 = u32x2{0, 0}, al1 = u32x2{0, 0};
                    if (!BWD64_LEAN) { al0 = tr_read(a0 + PLANE); al1 = tr_read(a1 + PLANE); }
                    const u32x2 bh0 = tr_read(b0), bh1 = tr_read(b1), bl0 = tr_read(b0 + PLANE), bl1 = tr_read(b1 + PLANE);
                    ah[tI] = u32x4{ah0.x, ah0.y, ah1.x, ah1.y}; al[tI] = u32x4{al0.x, al0.y, al1.x, al1.y};
                    bh[tI] = u32x4{bh0.x, bh0.y, bh1.x, bh1.y}; bl[tI] = u32x4{bl0.x, bl0.y, bl1.x, bl1.y};
                }
                if (BWD64_LEAN) {      // a = its bf16 plane: a^T (dp_lo) then a^T (dp_hi)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        gw1[q] = mfma1r(ah[q >> 1], bh[q & 1], mfma1r(ah[q >> 1], bl[q & 1], gw1[q]));
                } else {
                gw1[0] = mfma3r(ah[0], al[0], bh[0], bl[0], gw1[0]);
                gw1[1] = mfma3r(ah[0], al[0], bh[1], bl[1], gw1[1]);
                gw1[2] = mfma3r(ah[1], al[1], bh[0], bl[0], gw1[2]);
                gw1[3] = mfma3r(ah[1], al[1], bh[1], bl[1], gw1[3]);
                }
            }
        }
        if (more) issue(t + gridDim.x, std::integral_constant<int, 2>{});

        // ---- da = dp * W1 (this wave's 16 input channels, 4 pixel tiles) + ReLU mask + BN-backward sums ----------------
        // Everything a step needs is requested before the step that consumes it (operands of both k blocks, then the
        // raw x of the mask): with two waves per SIMD a read -> wait -> use chain per pixel tile is pure LDS latency.
        {
            const int l15o = opaque(l15), go = opaque(g);
            const unsigned char* dbase = s_d + (mh * 64 + l15o) * (C * 2);
            const int sw = l15o & 7;
            const int c = nt * 16 + l15o;
            f32x4 da[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) da[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!(abl & 8)) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {       // four independent accumulator chains per k block
                    u32x4 ph[4], pl[4];
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) {
                        const unsigned char* q = dbase + mi * 16 * (C * 2) + (((4 * kb + go) ^ sw) << 4);
                        ph[mi] = *reinterpret_cast<const u32x4*>(q);
                        pl[mi] = *reinterpret_cast<const u32x4*>(q + PLANE);
                    }
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
                        da[mi] = BWD64_LEAN ? mfma1r(ph[mi], wth[kb], mfma1r(pl[mi], wth[kb], da[mi]))
                                            : mfma3r(ph[mi], pl[mi], wth[kb], wtl[kb], da[mi]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (more) issue(t + gridDim.x, std::integral_constant<int, 3>{});
            if (bn_in) {
                const float m_mean = s_ci[c], m_scale = s_ci[C + c], m_beta = s_ci[2 * C + c], m_inv = s_ci[3 * C + c];
                const float m_lo = s_ci[4 * C + c];
                const float* xrd = s_x + (mh * 64 + 4 * go) * XP + (c ^ tile_swz(4 * go));
                float* pw = s_p + (mh * 64 + 4 * go) * XP + (c ^ tile_swz(4 * go));
                float xr[4][4];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) xr[mi][r] = xrd[(mi * 16 + r) * XP];
                if (!tile_full) {
                    // a pixel outside the image carries dp = 0, hence da = 0: only the mask of the BN sums is at
                    // stake, and da = 0 contributes nothing to them either -- but keep x finite and masked
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ip = (mh * 4 + mi) * 16 + 4 * go + r;
                            if (!inside(ip, y0 + ip / TW, x0 + ip % TW)) da[mi][r] = 0.0f;
                        }
                }
                float t0 = 0.0f, t1 = 0.0f;
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = fmaf(xr[mi][r] - m_mean, m_scale, m_beta) > 0.0f ? da[mi][r] : 0.0f;   // ReLU mask
                        t0 += v;
                        t1 = fmaf(v, bn_center(xr[mi][r], m_mean, m_lo) * m_inv, t1);
                        pw[(mi * 16 + r) * XP] = v;
                    }
                // 64 pixels per lane in fp32 (a handful of terms), folded over the four lane groups; then fp64 for the
                // long, heavily cancelling accumulation over the whole tensor
                t0 += __shfl_xor(t0, 16, 64); t1 += __shfl_xor(t1, 16, 64);
                t0 += __shfl_xor(t0, 32, 64); t1 += __shfl_xor(t1, 32, 64);
                if (go == 0) {
                    double* bs = s_bst + (mh * 2) * C + c;
                    bs[0] += (double)t0;
                    bs[C] += (double)t1;
                }
            } else {
                float* pw = s_p + (mh * 64 + 4 * go) * XP + (c ^ tile_swz(4 * go));
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pw[(mi * 16 + r) * XP] = da[mi][r];
            }
        }
        __syncthreads();

        // ---- dx store (coalesced rows of s_p) --------------------------------------------------------------------------
        if (d.dx && !(abl & 16)) {
            const int tid = opaque((int)threadIdx.x);
            const int ich4 = tid % C4;
            const unsigned xrange = PACKED ? (unsigned)d.N * (unsigned)d.x_img_stride * 4u : dxbytes;
            const auto r_dx = __builtin_amdgcn_make_buffer_rsrc(
                d.dx + (PACKED ? (size_t)0 : (size_t)n * d.x_img_stride), 0, xrange, 0x00020000);
            unsigned off[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const int ip = tid / C4 + PSTEP * i;
                const int y = y0 + ip / TW, x = x0 + ip % TW;
                if constexpr (PACKED) {
                    int pn, py, pxx;
                    off[i] = pk_locate(pk, y, x, pn, py, pxx)
                                 ? (unsigned)(pn * d.x_img_stride + (py * W + pxx) * C + ich4 * 4) * 4u : xrange;
                } else {
                    off[i] = (y < H && x < W) ? (unsigned)((y * W + x) * C + ich4 * 4) * 4u : dxbytes;
                }
            }
            if (d.accumulate_dx) {
                u32x4 old[NX];
#pragma unroll
                for (int i = 0; i < NX; ++i) old[i] = __builtin_amdgcn_raw_buffer_load_b128(r_dx, off[i], 0, 0);
#pragma unroll
                for (int i = 0; i < NX; ++i) {
                    const int ip = tid / C4 + PSTEP * i;
                    float4 v = *reinterpret_cast<const float4*>(s_p + ip * XP + ((ich4 * 4) ^ tile_swz(ip)));
                    const float4 o = *reinterpret_cast<const float4*>(&old[i]);
                    v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                    __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(&v), r_dx, off[i], 0, DX_AUX);
                }
            } else {
#pragma unroll
                for (int i = 0; i < NX; ++i) {
                    const int ip = tid / C4 + PSTEP * i;
                    const float4 v = *reinterpret_cast<const float4*>(s_p + ip * XP + ((ich4 * 4) ^ tile_swz(ip)));
                    // (non-temporal on the big maps, default policy on the packed 20 x 20 / 10 x 10 levels: common.h)
                    if constexpr (PACKED) __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(&v), r_dx, off[i], 0, 0);
                    else __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(&v), r_dx, off[i], 0, DX_AUX);
                }
            }
        }
        // no barrier here: the next stage writes the halo / x / a planes (all read before the barrier above) and
        // s_p is next written by the p GEMM, one barrier later
    }

    // ============ flush per-workgroup partial sums ================================================================
    __syncthreads();                                     // the last tile's dx rows have been read
    float* row = d.wgrad_partials + (size_t)blockIdx.x * Row::WIDTH;
    float* sm = reinterpret_cast<float*>(smem_raw);
    float* s_gw1 = sm;                                   // [KSPLIT][COUT][CIN]
    float* red = sm + KSPLIT * C * C;                    // [NT][24]
    {
        float* pl = s_gw1 + w1_ks * C * C;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)      // D layout: column = co (B operand tile), row = ci (A operand tile)
                    pl[((w1_ot + i) * 16 + l15) * C + (w1_ct + j) * 16 + 4 * g + r] = gw1[j * 2 + i][r];
    }
    float4* my = reinterpret_cast<float4*>(red + tid * 24);
#pragma unroll
    for (int k = 0; k < 6; ++k) my[k] = gw2[k];
    __syncthreads();
    for (int i = tid; i < C * C; i += NT) {
        float v = s_gw1[i];
        if constexpr (KSPLIT == 2) v += s_gw1[C * C + i];
        row[i] = v;
    }
    constexpr int PG = NT / C4;
    auto reduce_pass = [&](int ps, int nslot) {
        for (int o = tid; o < C * nslot; o += NT) {
            const int c = o / nslot, k = o - c * nslot;
            const int q = c >> 2, e = c & 3;
            float v = 0.0f;
            for (int p = 0; p < PG; ++p) v += red[(p * C4 + q) * 24 + k * 4 + e];
            const int slot = ps * 6 + k;
            if (slot < 9) row[Row::W2 + c * 9 + slot] = v;
            else if (slot == 9) row[Row::B1 + c] = v;
            else row[Row::B2 + c] = v;
        }
    };
    reduce_pass(0, 6);
    if (bn_in && d.dx && d.in_bn.bstats && tid < 2 * C) {
        double v = s_bst[tid];
        if constexpr (MH == 2) v += s_bst[2 * C + tid];
        if constexpr (DET) bn_det_add(d.in_bn.bstats, C, tid, v);
        else atomic_add_f64(bn_slot(d.in_bn.bstats, d.in_bn.slots, C) + tid, v);
    }
    __syncthreads();
    my[0] = gw2[6]; my[1] = gw2[7]; my[2] = gw2[8]; my[3] = gb1; my[4] = gb2;
    __syncthreads();
    reduce_pass(1, 5);
}

template <int NW, bool PACKED, bool POOLDY, bool DET = false>
int launch_dp_bwd64(const YunetDP* d, hipStream_t stream) {
    using G = bwd64::Geo<NW>;
    static PerDevice attr_set;      // per device (common.h)
    PackGeom pk;
    const int grid = dp_bwd_launch_setup<G::TH, G::TW, PACKED>(
        d, attr_set, reinterpret_cast<const void*>(dp_bwd64_kernel<NW, PACKED, POOLDY, DET>), G::SMEM, pk);
    if (grid < 0) return grid;
    if (DET && !bn_det_fits(d->in_bn, grid)) return YUNET_EINVAL;
    hipLaunchKernelGGL((dp_bwd64_kernel<NW, PACKED, POOLDY, DET>), dim3(grid), dim3(G::NT), G::SMEM, stream, *d, pk);
    return hip_status();
}
// the six instances the dispatcher reaches, in the form DET
template <bool DET>
int launch_dp_bwd64_form(const YunetDP* d, const DpRoute& r, hipStream_t stream) {
    if (r.pool) return r.nw == 4 ? launch_dp_bwd64<4, false, true, DET>(d, stream) : launch_dp_bwd64<8, false, true, DET>(d, stream);
    if (r.packed) return r.nw == 4 ? launch_dp_bwd64<4, true, false, DET>(d, stream) : launch_dp_bwd64<8, true, false, DET>(d, stream);
    return r.nw == 4 ? launch_dp_bwd64<4, false, false, DET>(d, stream) : launch_dp_bwd64<8, false, false, DET>(d, stream);
}

}  // namespace

// conv_bwd.hip's dispatcher: r.nw = bwd64_nw(N, H, W) (bwd_grid.h: the choice also fixes the rows of wgrad_partials);
// pooled dy (YunetDP.pool_idx: unpacked levels only, yunet_dp_pool_fusion_ok), else the packed canvas on the small levels
int ACT_SUFFIX(launch_dp_bwd64)(const YunetDP* d, const DpRoute& r, hipStream_t stream) {
#ifndef YUNET_ACT_BF16
    // a launch that produces the producer's BN-backward sums into order-fixed rows (dp_route.h: dp_bwd_det)
    if (r.det) return launch_dp_bwd64_form<true>(d, r, stream);
#endif
    return r.det ? YUNET_EINVAL : launch_dp_bwd64_form<false>(d, r, stream);
}
