// source.hip -- the decoded-source store of the device train pipeline (pipelines.SourceStore):
//   aug_gather_kernel      : a batch's SourceBatch metadata (src_off, src_hw, gt_off, packed boxes / keypoints) from
//                            the store's per-image tables and a device index vector, in one launch.
//   aug_window_plan_kernel : per image the source rectangle aug_pixels_kernel can read under the params that
//                            aug_decide_kernel wrote, and its offset in a compact window buffer.
//   yunet_upload_windows   : host code, one hipMemcpy2DAsync per non-empty rectangle from a pinned host store.
//   fetch_windows_kernel   : the same window buffer read by the GPU itself from the pinned, device-mapped host store,
//                            with the plan taken from device memory (yunet_fetch_windows).
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


// ---- fetch_windows_kernel -------------------------------------------------------------------------------------------
// Workgroup k copies chunk k of the plan: chunk (n, p) is bytes [p * kFetchChunk, (p + 1) * kFetchChunk) of image n's
// packed window, a band of its rows (the first and last row of the band possibly in part).  The host cannot count
// the chunks without reading the plan back, so the grid is an upper bound (N + win_bytes / kFetchChunk: the valid
// windows are disjoint inside win_bytes) and every workgroup counts them itself: one pass over the N images'
// plan rows (in L2) validates each image and scans the chunk counts; workgroups past the last chunk return.
//
// Image n is VALID when its rectangle lies inside src_hw[n], its source span inside [0, store_bytes), and its
// destination [win_off[n], win_off[n] + bytes) inside [0, win_bytes), inside [win_off[n], win_off[n+1]] and at or
// after every earlier win_off (a running maximum: valid destinations are disjoint whatever the others hold).  An
// invalid image gets no chunk, so nothing of it is read or written; workgroup 0 ORs its YUNET_FETCH_BAD_* bits into
// *status.
//
// The copy: the chunk's rows give (row, block) slots, kFetchSlotsRow per row at most (the aligned 16-byte source blocks
// a row piece can touch).  A round hands each thread kFetchLoads slots lane-contiguously (one wave instruction reads
// 1 KiB of a row) and issues all their loads before the first wait; each loaded block is shifted in registers
// (v_alignbyte) onto the dword grid of its destination and stored.  Every block of a row piece is loaded once.
constexpr int kFetchLoads = 16;                        // 16-byte loads per thread per round: 64 KiB per workgroup
constexpr long long kFetchChunk = 48 << 10;            // window bytes per workgroup (rows of <= 12 KiB: one round)

__device__ __forceinline__ long long block_inclusive_max(long long v, long long* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(v, d, 64);
        if (lane >= d && u > v) v = u;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    for (int k = 0; k < wave; ++k) v = wsum[k] > v ? wsum[k] : v;
    __syncthreads();
    return v;
}

// The 16 bytes at src + A, A a store offset whose device address is 16-byte aligned.  EDGE: the block crosses the
// first or last byte of the store [0, store_bytes) and is read byte by byte inside it (clamped addresses: the 16
// loads issue at once).
template <bool EDGE>
__device__ __forceinline__ uint4 fetch_block(const uint8_t* __restrict__ src, long long A, long long store_bytes) {
    if (!EDGE) return *reinterpret_cast<const uint4*>(src + A);
    uint32_t b[16], d[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const long long o = A + j;
        b[j] = src[o < 0 ? 0 : (o < store_bytes ? o : store_bytes - 1)];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (A + j >= 0 && A + j < store_bytes) d[j >> 2] |= b[j] << (8 * (j & 3));
    return make_uint4(d[0], d[1], d[2], d[3]);
}

// Block bytes j in [jlo, jhi) go to win + D + j: whole destination dwords as dword stores, the rest as byte stores.
__device__ __forceinline__ void store_block(uint4 v, uint8_t* __restrict__ win, long long D, int jlo, int jhi) {
    const int e = (int)((reinterpret_cast<uintptr_t>(win) + D) & 3);
    uint8_t* F = win + D - e;
    const uint32_t s[6] = {0u, v.x, v.y, v.z, v.w, 0u};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t d = e == 0 ? s[k + 1] : __builtin_amdgcn_alignbyte(s[k + 1], s[k], 4 - e);
        const int j0 = 4 * k - e;                       // block byte of the dword's first byte
        if (j0 >= jlo && j0 + 4 <= jhi) {
            *reinterpret_cast<uint32_t*>(F + 4 * k) = d;
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (j0 + m >= jlo && j0 + m < jhi) F[4 * k + m] = (uint8_t)(d >> (8 * m));
        }
    }
}

// The row pieces of one chunk: window bytes [lo, hi) of a rectangle with rows of rb bytes, row r at store offset
// srect + r * w3 and window offset drect + r * rb.  Slot t = (row piece i, block q): the piece's store offsets
// [p0, p1), its q-th block A (device address 16-byte aligned: `mis` = src's address mod 16), the window offset D of
// A's first byte, and the bytes [jlo, jhi) of A that belong to the piece (jhi = 0: no block).
struct FetchChunk {
    long long lo, hi, rb, w3, srect, drect, rfirst;
    int per_row, slots, mis;
    __device__ __forceinline__ void slot(int t, long long& A, long long& D, int& jlo, int& jhi) const {
        const int i = (int)((unsigned)t / (unsigned)per_row), q = t - i * per_row;
        const long long r = rfirst + i, r_lo = r * rb;
        const long long x0 = (lo > r_lo ? lo : r_lo) - r_lo, x1 = (hi < r_lo + rb ? hi : r_lo + rb) - r_lo;
        const long long row = srect + r * w3, p0 = row + x0, p1 = row + x1;
        A = ((p0 + mis) & ~15ll) - mis + 16ll * q;
        D = drect + r_lo + (A - row);
        jlo = p0 > A ? (int)(p0 - A) : 0;
        jhi = t < slots && A < p1 ? (p1 - A < 16 ? (int)(p1 - A) : 16) : 0;
    }
};

// Rounds of U slots per thread, lane-contiguous (one wave instruction reads 1 KiB of a row); each round issues all its
// loads before the first wait.
template <int U, bool EDGE>
__device__ __forceinline__ void fetch_chunk(const FetchChunk& c, const uint8_t* __restrict__ src, long long store_bytes,
                                            uint8_t* __restrict__ win) {
    for (int t0 = 0; t0 < c.slots; t0 += kSrcThreads * U) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            long long A, D;
            int jlo, jhi;
            c.slot(t0 + u * kSrcThreads + threadIdx.x, A, D, jlo, jhi);
            v[u] = jhi > 0 ? fetch_block<EDGE>(src, A, store_bytes) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            long long A, D;
            int jlo, jhi, t = t0 + u * kSrcThreads + threadIdx.x;
            asm volatile("" : "+v"(t));                 // recompute the slot: cheaper than U slots' offsets in VGPRs
            c.slot(t, A, D, jlo, jhi);
            if (jhi > 0) store_block(v[u], win, D, jlo, jhi);
        }
    }
}

__global__ __launch_bounds__(kSrcThreads) void fetch_windows_kernel(
    const uint8_t* __restrict__ src, long long store_bytes, const long long* __restrict__ src_off,
    const int32_t* __restrict__ src_hw, const int32_t* __restrict__ rect, const long long* __restrict__ win_off, int N,
    uint8_t* __restrict__ win, long long win_bytes, int32_t* __restrict__ status) {
    __shared__ long long wsum[kSrcThreads / 64];
    __shared__ long long s_cnt, s_max, s_piece;
    __shared__ int s_n, s_bad;
    const int tid = threadIdx.x;
    const long long k = blockIdx.x;
    if (tid == 0) { s_n = -1; s_bad = 0; }
    long long cnt = 0, pmax = 0;                        // chunks of the images before the tile; max win_off before it
    for (int base = 0; base < N; base += kSrcThreads) {
        const int n = base + tid;
        int r0 = 0, c0 = 0, rows = 0, cols = 0, h = 0, w = 0;
        long long so = 0, a = 0, b = 0, prev = 0;
        if (n < N) {
            r0 = rect[4 * n]; c0 = rect[4 * n + 1]; rows = rect[4 * n + 2]; cols = rect[4 * n + 3];
            h = src_hw[2 * n]; w = src_hw[2 * n + 1];
            so = src_off[n]; a = win_off[n]; b = win_off[n + 1];
            prev = n > 0 ? win_off[n - 1] : 0;
        }
        const long long incl = block_inclusive_max(prev, wsum);
        const long long before = incl > pmax ? incl : pmax;           // max(0, win_off[0 .. n-1])
        int bad = 0;
        long long bytes = 0;
        if (n < N) {
            if (r0 < 0 || c0 < 0 || rows < 0 || cols < 0 || (long long)r0 + rows > h || (long long)c0 + cols > w)
                bad |= YUNET_FETCH_BAD_RECT;
            else if ((long long)rows * cols > (1ll << 60))
                bad |= YUNET_FETCH_BAD_DST;                            // can be no buffer's
            else
                bytes = (long long)rows * cols * 3;
            if (bytes > 0) {                                           // pixels from the image start to the span end
                const long long end = ((long long)r0 + rows - 1) * w + c0 + cols;
                if (so < 0 || so > store_bytes || end > (store_bytes - so) / 3) bad |= YUNET_FETCH_BAD_SRC;
            }
            if (a < before || b < a || bytes > b - a || a > win_bytes || bytes > win_bytes - a)
                bad |= YUNET_FETCH_BAD_DST;
        }
        const long long chunks = bad ? 0 : (bytes + kFetchChunk - 1) / kFetchChunk;
        const long long cincl = block_inclusive_scan(chunks, wsum);
        const long long first = cnt + cincl - chunks;
        if (k >= first && k < first + chunks) { s_n = n; s_piece = k - first; }
        if (bad && blockIdx.x == 0) atomicOr(&s_bad, bad);
        if (tid == kSrcThreads - 1) { s_cnt = cnt + cincl; s_max = before > a ? before : a; }
        __syncthreads();
        cnt = s_cnt; pmax = s_max;
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid == 0 && s_bad) atomicOr(status, s_bad);
    const int n = s_n;
    if (n < 0) return;                                  // past the last chunk

    FetchChunk c;
    const long long rows = rect[4 * n + 2];
    c.rb = 3ll * rect[4 * n + 3];
    c.w3 = 3ll * src_hw[2 * n + 1];
    c.lo = s_piece * kFetchChunk;
    c.hi = c.lo + kFetchChunk < rows * c.rb ? c.lo + kFetchChunk : rows * c.rb;
    c.rfirst = c.lo / c.rb;
    c.srect = src_off[n] + rect[4 * n] * c.w3 + 3ll * rect[4 * n + 1];
    c.drect = win_off[n];
    c.per_row = (int)(((c.rb < c.hi - c.lo ? c.rb : c.hi - c.lo) + 30) / 16);    // blocks a row piece can touch
    c.slots = (int)((c.hi - 1) / c.rb - c.rfirst + 1) * c.per_row;
    c.mis = (int)(reinterpret_cast<uintptr_t>(src) & 15);
    // the chunk's first and last byte in the store: blocks past either end of the store take the byte-wise path
    const long long p_first = c.srect + c.rfirst * c.w3 + (c.lo - c.rfirst * c.rb);
    const long long r_last = (c.hi - 1) / c.rb, p_last = c.srect + r_last * c.w3 + (c.hi - r_last * c.rb);
    if (((p_first + c.mis) & ~15ll) - c.mis < 0 || ((p_last + c.mis + 15) & ~15ll) - c.mis > store_bytes)
        fetch_chunk<1, true>(c, src, store_bytes, win);
    else
        fetch_chunk<kFetchLoads, false>(c, src, store_bytes, win);
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


// The whole of [p, p + bytes) pinned host memory with a device mapping -> its device address, else nullptr (a failed
// query leaves no error behind for the next hip_status()).
static const uint8_t* pinned_device_range(const uint8_t* p, long long bytes) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (at.type != hipMemoryTypeHost) return nullptr;
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, const_cast<uint8_t*>(p), 0) != hipSuccess || !dev) {
        (void)hipGetLastError();
        return nullptr;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    const uintptr_t d = reinterpret_cast<uintptr_t>(dev), b = reinterpret_cast<uintptr_t>(base);
    if (d < b || (unsigned long long)bytes > size - (d - b)) return nullptr;
    return static_cast<const uint8_t*>(dev);
}

extern "C" int yunet_fetch_windows(const uint8_t* host_src, long long store_bytes, const long long* src_off,
                                   const int32_t* src_hw, const int32_t* rect, const long long* win_off, int N,
                                   uint8_t* win, long long win_bytes, int32_t* status, void* stream) {
    if (!host_src || !src_off || !src_hw || !rect || !win_off || !win || !status || store_bytes < 1 ||
        win_bytes < 1 || N < 1 || N > kGatherMaxN)
        return YUNET_EINVAL;
    const long long grid = N + (win_bytes + kFetchChunk - 1) / kFetchChunk;
    if (grid > 0x7fffffff) return YUNET_EINVAL;
    const uint8_t* src = pinned_device_range(host_src, store_bytes);
    if (!src) return YUNET_EINVAL;                       // pageable memory: the device must never touch it
    hipLaunchKernelGGL(fetch_windows_kernel, dim3((unsigned)grid), dim3(kSrcThreads), 0, (hipStream_t)stream, src,
                       store_bytes, src_off, src_hw, rect, win_off, N, win, win_bytes, status);
    return hip_status();
}
