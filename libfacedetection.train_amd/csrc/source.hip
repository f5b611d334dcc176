// source.hip -- the decoded-source store of the device train pipeline (pipelines.SourceStore):
//   aug_gather_kernel      : a batch's SourceBatch metadata (src_off, src_hw, gt_off, packed boxes / keypoints) from
//                            the store's per-image tables and a device index vector, in one launch.
//   aug_window_plan_kernel : per image the source rectangle aug_pixels_kernel can read under the params that
//                            aug_decide_kernel wrote, and its offset in a compact window buffer.
//   yunet_upload_windows   : host code, one hipMemcpy2DAsync per non-empty rectangle from a pinned host store.
// Integer work only (no float arithmetic), so the -ffp-contract setting is irrelevant here.
#include "common.h"

namespace {

constexpr int kSrcThreads = 256;
constexpr int kGatherMaxN = 8192;     // (N + 1) int32 prefix offsets in LDS: 32 KiB

// Inclusive scan of one value per thread over the 256-thread block; `wsum` holds 4 wave totals.
template <typename T>
__device__ __forceinline__ T block_inclusive_scan(T v, T* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    for (int k = 0; k < wave; ++k) v += wsum[k];
    __syncthreads();
    return v;
}

// Every workgroup scans the N picked GT counts itself (N <= 8192: at most 32 tiles), so the launch needs no
// inter-workgroup hand-off; workgroup 0 writes the per-image tables, and the workgroups stride over the images to
// copy their boxes / keypoints.  An index outside [0, M) picks an empty image (0 x 0, no GT); rows at or beyond
// g_cap are not written.
__global__ __launch_bounds__(kSrcThreads) void aug_gather_kernel(
    const int32_t* __restrict__ idx, int N, int M, const long long* __restrict__ store_off,
    const int32_t* __restrict__ store_hw, const int32_t* __restrict__ store_goff, const int32_t* __restrict__ store_gcnt,
    const float* __restrict__ store_boxes, const float* __restrict__ store_kps, int g_cap,
    long long* __restrict__ src_off, int32_t* __restrict__ src_hw, int32_t* __restrict__ gt_off,
    float* __restrict__ boxes, float* __restrict__ kps) {
    extern __shared__ int32_t s_off[];          // [N + 1]
    __shared__ int32_t wsum[kSrcThreads / 64];
    __shared__ int32_t s_tot;
    const int tid = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < N; base += kSrcThreads) {
        const int n = base + tid;
        int c = 0;
        if (n < N) {
            const int i = idx[n];
            c = (i >= 0 && i < M) ? store_gcnt[i] : 0;
        }
        const int incl = block_inclusive_scan(c, wsum);
        if (n < N) s_off[n + 1] = carry + incl;
        if (tid == kSrcThreads - 1) s_tot = carry + incl;
        __syncthreads();
        carry = s_tot;
        __syncthreads();
    }
    if (tid == 0) s_off[0] = 0;
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int n = tid; n < N; n += kSrcThreads) {
            const int i = idx[n];
            const bool ok = i >= 0 && i < M;
            src_off[n] = ok ? store_off[i] : 0;
            src_hw[2 * n] = ok ? store_hw[2 * i] : 0;
            src_hw[2 * n + 1] = ok ? store_hw[2 * i + 1] : 0;
            gt_off[n] = s_off[n];
        }
        if (tid == 0) gt_off[N] = s_off[N];
    }
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        const int i = idx[n];
        if (i < 0 || i >= M) continue;
        const int d0 = s_off[n], g = s_off[n + 1] - d0;
        const int rows = (d0 + g <= g_cap) ? g : (g_cap > d0 ? g_cap - d0 : 0);
        const float* sb = store_boxes + (size_t)store_goff[i] * 4;
        const float* sk = store_kps + (size_t)store_goff[i] * 15;
        float* db = boxes + (size_t)d0 * 4;
        float* dk = kps + (size_t)d0 * 15;
        for (int e = tid; e < rows * 4; e += kSrcThreads) db[e] = sb[e];
        for (int e = tid; e < rows * 15; e += kSrcThreads) dk[e] = sk[e];
    }
}

// rect[n] = (row0, col0, rows, cols): rows [max(top, 0), min(top + cw, h)) x cols [max(left, 0), min(left + cw, w)),
// the taps aug_pixels_kernel can read (lin_coef clamps both taps to [0, cw - 1] inside the window); (0, 0, 0, 0)
// when cw == 0 or the window misses the image.  win_off[n] = exclusive scan of rows * cols * 3, win_off[N] the total.
__global__ __launch_bounds__(kSrcThreads) void aug_window_plan_kernel(
    const int32_t* __restrict__ params, const int32_t* __restrict__ src_hw, int N, int32_t* __restrict__ rect,
    long long* __restrict__ win_off) {
    __shared__ long long wsum[kSrcThreads / 64];
    __shared__ long long s_tot;
    const int tid = threadIdx.x;
    long long carry = 0;
    for (int base = 0; base < N; base += kSrcThreads) {
        const int n = base + tid;
        int y0 = 0, x0 = 0, rows = 0, cols = 0;
        if (n < N) {
            const int32_t* p = params + 8 * n;
            const int left = p[0], top = p[1], cw = p[2];
            const int h = src_hw[2 * n], w = src_hw[2 * n + 1];
            if (cw > 0) {
                const int a = top > 0 ? top : 0, b = top + cw < h ? top + cw : h;
                const int c = left > 0 ? left : 0, d = left + cw < w ? left + cw : w;
                if (b > a && d > c) { y0 = a; x0 = c; rows = b - a; cols = d - c; }
            }
            rect[4 * n + 0] = y0; rect[4 * n + 1] = x0; rect[4 * n + 2] = rows; rect[4 * n + 3] = cols;
        }
        const long long bytes = (long long)rows * cols * 3;
        const long long incl = block_inclusive_scan(bytes, wsum);
        if (n < N) win_off[n] = carry + incl - bytes;
        if (tid == kSrcThreads - 1) s_tot = carry + incl;
        __syncthreads();
        carry = s_tot;
        __syncthreads();
    }
    if (tid == 0) win_off[N] = carry;
}

}  // namespace

extern "C" int yunet_aug_gather(const int32_t* idx, int N, int M, const long long* store_off,
                                const int32_t* store_hw, const int32_t* store_goff, const int32_t* store_gcnt,
                                const float* store_boxes, const float* store_kps, int g_cap, long long* src_off,
                                int32_t* src_hw, int32_t* gt_off, float* boxes, float* kps, void* stream) {
    if (N < 1 || N > kGatherMaxN || M < 1 || g_cap < 0) return YUNET_EINVAL;
    const int grid = N < 256 ? N : 256;
    hipLaunchKernelGGL(aug_gather_kernel, dim3(grid), dim3(kSrcThreads), (N + 1) * sizeof(int32_t),
                       (hipStream_t)stream, idx, N, M, store_off, store_hw, store_goff, store_gcnt, store_boxes,
                       store_kps, g_cap, src_off, src_hw, gt_off, boxes, kps);
    return hip_status();
}

extern "C" int yunet_aug_window_plan(const int32_t* params, const int32_t* src_hw, int N, int32_t* rect,
                                     long long* win_off, void* stream) {
    if (N < 1) return YUNET_EINVAL;
    hipLaunchKernelGGL(aug_window_plan_kernel, dim3(1), dim3(kSrcThreads), 0, (hipStream_t)stream, params, src_hw,
                       N, rect, win_off);
    return hip_status();
}

extern "C" int yunet_upload_windows(const uint8_t* host_src, const long long* src_off, const int32_t* src_hw,
                                    const int32_t* rect, const long long* win_off, int N, uint8_t* win,
                                    long long win_bytes, void* stream) {
    if (!host_src || !src_off || !src_hw || !rect || !win_off || !win || N < 1) return YUNET_EINVAL;
    if (win_off[N] > win_bytes) return YUNET_EINVAL;
    for (int n = 0; n < N; ++n) {              // validate the whole plan before the first copy is queued
        const int32_t* r = rect + 4 * n;
        const int h = src_hw[2 * n], w = src_hw[2 * n + 1];
        const long long bytes = (long long)r[2] * r[3] * 3;
        if (r[0] < 0 || r[1] < 0 || r[2] < 0 || r[3] < 0 || r[0] + r[2] > h || r[1] + r[3] > w ||
            win_off[n] < 0 || win_off[n] + bytes > win_off[n + 1] || src_off[n] < 0)
            return YUNET_EINVAL;
    }
    for (int n = 0; n < N; ++n) {
        const int32_t* r = rect + 4 * n;
        if (r[2] == 0 || r[3] == 0) continue;
        const size_t w3 = (size_t)src_hw[2 * n + 1] * 3, cols3 = (size_t)r[3] * 3;
        const uint8_t* s = host_src + src_off[n] + (size_t)r[0] * w3 + (size_t)r[1] * 3;
        const hipError_t e = hipMemcpy2DAsync(win + win_off[n], cols3, s, w3, cols3, (size_t)r[2],
                                              hipMemcpyHostToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return -(int)e;
    }
    return 0;
}
