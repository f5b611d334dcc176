// hooks.hip -- the per-iteration device work of the custom training hooks (runner.py / hooks.py):
//   ema_update_kernel    : ExpMomentumEMAHook / LinearMomentumEMAHook, every EMA segment in one launch
//                          (yunet_ema_update)
//   box_size_hist_kernel : YuNetSampleSizeStatisticsHook, the GT box-size histogram of one batch
//                          (yunet_box_size_hist)
// Both are short non-persistent launches on the caller's stream; neither synchronises the host.
//
// Rounding of the EMA update: torch's ROCm  ema.mul_(keep)  rounds ema * keep to fp32 (the python scalar is cast to
// float), and  add_(src, alpha=m)  evaluates  self + alpha * other, which the ROCm build contracts into one fused
// multiply-add:  fma(m, src, fl(ema * keep)).  The explicit __fmul_rn / __fmaf_rn below pin that form whatever the
// -ffp-contract setting; tests/test_custom_hooks_gpu.py checks it bit for bit against torch on the GPU.
#include "common.h"

namespace {

constexpr int kHookThreads = 256;
constexpr long long kEmaMaxBlocks = 1024;

// One segment as the launch sees it: `head` scalar elements until ema is 16-byte aligned, `vec` float4 units, then the
// scalar tail.  A segment whose src does not share ema's alignment runs scalar throughout (head = n, vec = 0).
struct EmaSeg {
    const float* src;
    float* ema;
    long long n, head, vec;
};
struct EmaArgs {
    EmaSeg s[YUNET_EMA_MAX_SEGMENTS];
    long long start[YUNET_EMA_MAX_SEGMENTS + 1];     // first work unit of each segment; start[nseg] = total
    int nseg;
    float keep, m;
};

__device__ __forceinline__ float ema_step(float e, float s, float keep, float m) {
    return __fmaf_rn(m, s, __fmul_rn(e, keep));
}

__global__ __launch_bounds__(kHookThreads) void ema_update_kernel(EmaArgs a) {
    const long long total = a.start[a.nseg];
    const long long stride = (long long)gridDim.x * kHookThreads;
    for (long long u = (long long)blockIdx.x * kHookThreads + threadIdx.x; u < total; u += stride) {
        int k = 0;
        while (k + 1 < a.nseg && u >= a.start[k + 1]) ++k;
        const EmaSeg& s = a.s[k];
        long long r = u - a.start[k];
        if (r >= s.head && r < s.head + s.vec) {
            const long long e0 = s.head + 4 * (r - s.head);
            const f32x4 x = *reinterpret_cast<const f32x4*>(s.src + e0);
            f32x4 e = *reinterpret_cast<const f32x4*>(s.ema + e0);
            e.x = ema_step(e.x, x.x, a.keep, a.m);
            e.y = ema_step(e.y, x.y, a.keep, a.m);
            e.z = ema_step(e.z, x.z, a.keep, a.m);
            e.w = ema_step(e.w, x.w, a.keep, a.m);
            *reinterpret_cast<f32x4*>(s.ema + e0) = e;
        } else {
            const long long i = r < s.head ? r : s.head + 4 * s.vec + (r - s.head - s.vec);
            s.ema[i] = ema_step(s.ema[i], s.src[i], a.keep, a.m);
        }
    }
}

// One thread per padded GT row (n, g).  Integer atomics only; the wave's box and empty-image counts are added with
// one atomic per wave.
__global__ __launch_bounds__(kHookThreads) void box_size_hist_kernel(
    const float* __restrict__ boxes, const int32_t* __restrict__ counts, int N, int Gmax, unsigned long long it_key,
    int W, int H, unsigned long long* __restrict__ bin_count, unsigned long long* __restrict__ bin_first,
    unsigned long long* __restrict__ totals, unsigned long long* __restrict__ spill, int spill_cap) {
    const long long idx = (long long)blockIdx.x * kHookThreads + threadIdx.x;
    const bool row = idx < (long long)N * Gmax;
    bool box = false, noimg = false;
    if (row) {
        const int n = (int)(idx / Gmax), g = (int)(idx - (long long)n * Gmax);
        const int c = counts[n];
        if (g == 0) {
            noimg = c == 0;
            if (c < 0 || c > Gmax) atomicOr(&totals[YUNET_HIST_STATUS], (unsigned long long)YUNET_HIST_BAD_COUNT);
        }
        box = g < (c < 0 ? 0 : (c > Gmax ? Gmax : c));
        if (box) {
            const float* b = boxes + 4 * idx;
            const float w = __fsub_rn(b[2], b[0]), h = __fsub_rn(b[3], b[1]);
            const float wt = truncf(w), ht = truncf(h);          // python int() of the fp32 difference
            const unsigned long long key = it_key | (unsigned long long)idx;
            if (wt >= 0.f && wt <= (float)W && ht >= 0.f && ht <= (float)H) {
                const long long bin = (long long)ht * (W + 1) + (long long)wt;
                atomicAdd(&bin_count[bin], 1ull);
                atomicMin(&bin_first[bin], key);
            } else {
                const unsigned long long slot = atomicAdd(&totals[YUNET_HIST_SPILLED], 1ull);
                if (slot < (unsigned long long)spill_cap) {
                    spill[2 * slot] = key;
                    spill[2 * slot + 1] = (unsigned long long)__float_as_uint(w) |
                                          ((unsigned long long)__float_as_uint(h) << 32);
                    atomicOr(&totals[YUNET_HIST_STATUS], (unsigned long long)YUNET_HIST_SPILL);
                } else {
                    atomicOr(&totals[YUNET_HIST_STATUS], (unsigned long long)YUNET_HIST_OVERFLOW);
                }
            }
        }
    }
    const unsigned long long nb = __popcll(__ballot(box)), ne = __popcll(__ballot(noimg));
    if ((threadIdx.x & 63) == 0) {
        if (nb) atomicAdd(&totals[YUNET_HIST_TOTAL], nb);
        if (ne) atomicAdd(&totals[YUNET_HIST_NOIMG], ne);
    }
}

}  // namespace

extern "C" int yunet_ema_update(const float* const* src, float* const* ema, const long long* n, int nseg, float keep,
                                float m, void* stream) {
    if (!src || !ema || !n || nseg < 1 || nseg > YUNET_EMA_MAX_SEGMENTS) return YUNET_EINVAL;
    EmaArgs a{};
    a.nseg = nseg;
    a.keep = keep;
    a.m = m;
    long long total = 0;
    for (int k = 0; k < nseg; ++k) {
        const long long nk = n[k];
        if (nk < 0) return YUNET_EINVAL;
        if (nk > 0 && (!src[k] || !ema[k])) return YUNET_EINVAL;
        if (nk > 0 && (((uintptr_t)src[k] | (uintptr_t)ema[k]) & 3)) return YUNET_EINVAL;
        EmaSeg& s = a.s[k];
        s.src = src[k];
        s.ema = ema[k];
        s.n = nk;
        const long long to16 = (long long)(((16 - ((uintptr_t)ema[k] & 15)) & 15) >> 2);
        const long long head = to16 < nk ? to16 : nk;
        if ((((uintptr_t)(src[k] + head)) & 15) == 0) {
            s.head = head;
            s.vec = (nk - head) >> 2;
        } else {
            s.head = nk;
            s.vec = 0;
        }
        a.start[k] = total;
        total += nk - 3 * s.vec;                   // scalar elements + float4 units
    }
    a.start[nseg] = total;
    if (total == 0) return 0;
    long long blocks = (total + kHookThreads - 1) / kHookThreads;
    if (blocks > kEmaMaxBlocks) blocks = kEmaMaxBlocks;
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)blocks), dim3(kHookThreads), 0, (hipStream_t)stream, a);
    return hip_status();
}

extern "C" int yunet_box_size_hist(const float* boxes, const int32_t* counts, int N, int Gmax, long long iteration,
                                   int W, int H, long long* bin_count, long long* bin_first, long long* totals,
                                   long long* spill, int spill_cap, void* stream) {
    if (!boxes || !counts || !bin_count || !bin_first || !totals) return YUNET_EINVAL;
    if (N < 0 || Gmax < 1 || (long long)N * Gmax >= (1ll << 31)) return YUNET_EINVAL;
    if (W < 0 || H < 0 || W > 65535 || H > 65535) return YUNET_EINVAL;
    if (iteration < 0 || iteration >= (1ll << 31)) return YUNET_EINVAL;
    if (spill_cap < 0 || (!spill && spill_cap > 0)) return YUNET_EINVAL;
    if (N == 0) return 0;
    const long long rows = (long long)N * Gmax;
    const unsigned blocks = (unsigned)((rows + kHookThreads - 1) / kHookThreads);
    hipLaunchKernelGGL(box_size_hist_kernel, dim3(blocks), dim3(kHookThreads), 0, (hipStream_t)stream, boxes, counts,
                       N, Gmax, (unsigned long long)iteration << 32, W, H, (unsigned long long*)bin_count,
                       (unsigned long long*)bin_first, (unsigned long long*)totals, (unsigned long long*)spill,
                       spill_cap);
    return hip_status();
}
