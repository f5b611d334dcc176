// dp_bwd_parts.h -- what the backward tile kernels share (conv_bwd.hip: dp_bwd_kernel, conv_bwd64.hip: dp_bwd64_kernel,
// conv_bwd16.hip: dp_bwd16s_kernel).
#pragma once
#include "common.h"

// Opaque copy of a thread-invariant value: stops the compiler from hoisting everything derived
// from it (per-slot offsets, halo coordinates) out of the persistent tile loop, where those
// values would occupy dozens of VGPRs for the whole kernel.
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ float tin(float x, float mean, float scale, float beta, float floor_) {
    return fmaxf(fmaf(x - mean, scale, beta), floor_);
}

// ---- split-bf16 helpers (GEMM = 1) --------------------------------------------------------------
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// (x0, x1) -> packed bf16 pairs hi = rne(x), lo = rne(x - hi); element 0 in the low half
__device__ __forceinline__ void split2(float x0, float x1, unsigned& hi, unsigned& lo) {
    const f32x2 v = {x0, x1};
    const unsigned hb = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    const f32x2 r = {x0 - __uint_as_float(hb << 16), x1 - __uint_as_float(hb & 0xffff0000u)};
    hi = hb;
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
}
struct Split8 {
    u32x4 hi, lo;     // 8 bf16 each: the 8 k-slots one lane feeds to v_mfma_f32_16x16x32_bf16
};
__device__ __forceinline__ Split8 split8(const float (&x)[8]) {
    unsigned h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split2(x[2 * i], x[2 * i + 1], h[i], l[i]);
    Split8 o;
    o.hi = u32x4{h[0], h[1], h[2], h[3]};
    o.lo = u32x4{l[0], l[1], l[2], l[3]};
    return o;
}
// D += A*B with A = ah + al, B = bh + bl (lo*lo dropped); small terms first
__device__ __forceinline__ f32x4 mfma3(const Split8& a, const u32x4 bh, const u32x4 bl, f32x4 c) {
    const bf16x8 ah = __builtin_bit_cast(bf16x8, a.hi), al = __builtin_bit_cast(bf16x8, a.lo);
    const bf16x8 vh = __builtin_bit_cast(bf16x8, bh), vl = __builtin_bit_cast(bf16x8, bl);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, vh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, vl, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, vh, c, 0, 0, 0);
    return c;
}

// one activation element through a buffer descriptor, widened to fp32
template <typename R>
__device__ __forceinline__ float act_bufld1(R rsrc, unsigned byte_off) {
#ifdef YUNET_ACT_BF16
    return __uint_as_float(((unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rsrc, byte_off, 0, 0)) << 16);
#else
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, byte_off, 0, 0));
#endif
}

// One row of YunetDP::wgrad_partials, written by one workgroup (kernels.py: dp_row_width is the same layout):
// dW1 [COUT][CIN] | db1 [COUT] | dW2 [COUT][9] | db2 [COUT]
template <int CIN, int COUT>
struct DpWgradRow {
    static constexpr int W1 = 0, B1 = COUT * CIN, W2 = B1 + COUT, B2 = W2 + COUT * 9, WIDTH = B2 + COUT;
};

// Launch set-up both tile kernels share: dynamic-LDS attribute (once per device: `attr_set` belongs to the kernel instance),
// pack geometry, tile count, persistent grid clamped to the rows of wgrad_partials.  Returns the grid, or a YUNET_E* code (< 0).
template <int TH, int TW, bool PACKED>
inline int dp_bwd_launch_setup(const YunetDP* d, PerDevice& attr_set, const void* kernel, size_t smem, PackGeom& pk) {
    if (per_device(attr_set, [&] {
            return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) == hipSuccess ? 1 : -1;
        }) < 0)
        return YUNET_EINVAL;
    pk = dp_pack_geom(d->N, d->H, d->W);
    pk.on = PACKED ? 1 : 0;
    if (!dp_pack_fits(pk, d->x_img_stride, d->z_img_stride)) return YUNET_EINVAL;
    const int tiles = PACKED ? ((pk.CW + TW - 1) / TW) * ((pk.CH + TH - 1) / TH)
                             : d->N * ((d->W + TW - 1) / TW) * ((d->H + TH - 1) / TH);
    int grid = tiles < CONV_BLOCKS ? tiles : CONV_BLOCKS;
    if (grid > d->wgrad_blocks) grid = d->wgrad_blocks;
    return grid < 1 ? YUNET_EINVAL : grid;
}
