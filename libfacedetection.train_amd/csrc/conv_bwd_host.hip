// conv_bwd_host.hip -- the parts of the backward that do not depend on the activation storage type (compiled once):
// the grid-size queries, the BatchNorm parameter gradient and the reduction of the per-workgroup partial rows.
#include <cstdio>
#include <cstring>

#include "common.h"
#include "dp_route.h"

namespace {

__global__ void bn_param_grad_kernel(const double* __restrict__ bstats, float* __restrict__ dgamma,
                                     float* __restrict__ dbeta, int C, int accumulate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float db = (float)bstats[c], dg = (float)bstats[C + c];
    dbeta[c] = accumulate ? dbeta[c] + db : db;
    dgamma[c] = accumulate ? dgamma[c] + dg : dg;
}

// One row slice of a column: rows sl, sl + 16, ... added IN THAT ORDER.  Sixteen (then four) loads are issued before the
// first addition: written as `v += p[...]` in a plain loop the compiler waits out every load before the next one is issued
// (s_waitcnt vmcnt(0) per iteration), and a 768-row job -- 48 rows per slice, each an L2 / HBM round trip -- took 40 us
// at the END of the backward, where nothing overlaps it.  Same additions in the same order: bit-identical sums.
__device__ __forceinline__ float column_slice_sum(const float* __restrict__ p, int blocks, int width, int sl) {
    float v = 0.0f;
    int b = sl;
    for (; b + 16 * 15 < blocks; b += 16 * 16) {
        float x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = p[(size_t)(b + 16 * u) * width];
#pragma unroll
        for (int u = 0; u < 16; ++u) v += x[u];
    }
    for (; b + 16 * 3 < blocks; b += 16 * 4) {
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = p[(size_t)(b + 16 * u) * width];
#pragma unroll
        for (int u = 0; u < 4; ++u) v += x[u];
    }
    for (; b < blocks; b += 16) v += p[(size_t)b * width];
    return v;
}

// out[j] (+)= sum_b partials[b][j]: 64 columns x 16 row-slices per workgroup (coalesced 256-byte
// row segments, 16 x 16 loads in flight per column), combined in a fixed order -> deterministic.
__global__ __launch_bounds__(1024) void reduce_partials_kernel(const float* __restrict__ partials,
                                                               int blocks, int width,
                                                               float* __restrict__ out,
                                                               int accumulate) {
    __shared__ float s[16][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    float v = 0.0f;
    if (col < width) v = column_slice_sum(partials + col, blocks, width, sl);
    s[sl][lane] = v;
    __syncthreads();
    if (sl == 0 && col < width) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += s[k][lane];
        out[col] = accumulate ? out[col] + t : t;
    }
}

// table-driven variant: workgroup -> (job, 64-column chunk); same arithmetic and order as above
__global__ __launch_bounds__(1024) void reduce_partials_batch_kernel(const YunetReduceJob* __restrict__ jobs,
                                                                     int njobs) {
    __shared__ float s[16][64];
    // the last job whose first chunk is <= this workgroup (chunk0 ascends): bisection -- 6 dependent scalar loads
    // instead of up to njobs
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].chunk0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const YunetReduceJob job = jobs[lo];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int col = ((int)blockIdx.x - job.chunk0) * 64 + lane;
    float v = 0.0f;
    if (col < job.width) v = column_slice_sum(job.partials + col, job.blocks, job.width, sl);
    s[sl][lane] = v;
    __syncthreads();
    if (sl == 0 && col < job.width) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += s[k][lane];
        job.out[col] = job.accumulate ? job.out[col] + t : t;
    }
}

// Deterministic mode (YunetBN::det_rows): block[0][j] = sum of rows 1 .. rows of a [1 + rows][width] fp64 block.  16 columns
// x 16 row slices per workgroup (128-byte row segments); slice s adds rows 1 + s, 1 + s + 16, ... in ascending order, thread
// (s = 0, column) adds the sixteen slice sums in ascending s: the order include/yunet_hip.h documents, whatever the grid.
__global__ __launch_bounds__(256) void bn_fold_kernel(double* __restrict__ block, int rows, int width) {
    __shared__ double s[16][16];
    const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int col = blockIdx.x * 16 + cl;
    double v = 0.0;
    if (col < width) {
        const double* p = block + (size_t)width + col;
        int r = sl;
        for (; r + 16 * 7 < rows; r += 16 * 8) {          // eight loads in flight, added in row order
            double x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = p[(size_t)(r + 16 * u) * width];
#pragma unroll
            for (int u = 0; u < 8; ++u) v += x[u];
        }
        for (; r < rows; r += 16) v += p[(size_t)r * width];
    }
    s[sl][cl] = v;
    __syncthreads();
    if (sl == 0 && col < width) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += s[k][cl];
        block[col] = t;
    }
}

}  // namespace

extern "C" int yunet_bn_fold(double* block, int rows, int C, void* stream) {
    if (!block || rows < 1 || C < 1 || C > 4096) return YUNET_EINVAL;
    hipLaunchKernelGGL(bn_fold_kernel, dim3((2 * C + 15) / 16), dim3(256), 0, (hipStream_t)stream, block, rows, 2 * C);
    return hip_status();
}

extern "C" int yunet_dp_bwd_blocks(int N, int H, int W, int cin, int cout) {
    const bool two_per_cu = cin == 64 && cout == 64 && bwd64_nw(N, H, W) == 4;      // dp_bwd64 on 8 x 8 tiles
    const int th = dp_bwd_big_tile(H, W, cin, cout) ? 16 : 8, tw = two_per_cu ? 8 : th * 2;
    const PackGeom pk = dp_pack_geom(N, H, W);       // small maps: one tile grid over the packed canvas
    const long long tiles = dp_use_pack_bwd(N, H, W, cin, cout)
                                ? (long long)((pk.CW + tw - 1) / tw) * ((pk.CH + th - 1) / th)
                                  : (long long)N * ((W + tw - 1) / tw) * ((H + th - 1) / th);
    const int cap = two_per_cu ? 2 * DP_BWD_MAX_BLOCKS : DP_BWD_MAX_BLOCKS;
    return (int)(tiles < cap ? tiles : cap);
}
extern "C" int yunet_dp_pool_fusion_ok(int N, int H, int W, int cin, int cout) {
    if ((H & 1) || (W & 1)) return 0;
    if (cin == 16 && cout == 16) return dp_bwd_big_tile(H, W, cin, cout) ? 1 : 0;
    if (cin == 64 && cout == 64) return dp_use_pack_bwd(N, H, W, cin, cout) ? 0 : 1;
    if (cin == 32 && cout == 64) return 1;       // YuNet_s: the unit in front of its 80x80 -> 40x40 pool
    return 0;
}
extern "C" int yunet_dp_bwd_reads_z(const YunetDP* d) {
    return d && dp_bwd_streams16(d) ? 0 : 1;
}
extern "C" int yunet_dp_fwd_group_one_grid(const YunetDP* const* units, int n) {
    if (!units || n < 1 || !units[0] || (units[0]->x_dtype != YUNET_F32 && units[0]->x_dtype != YUNET_BF16)) return 0;
    return dp_fwd_one_grid(units, n, units[0]->x_dtype) ? 1 : 0;
}
// the route of a descriptor (dp_route.h) as the kernel's own name with every template argument
extern "C" int yunet_dp_route(const YunetDP* d, int backward, char* name, int cap) {
    DpRoute r;
    if (!d || !name || (d->x_dtype != YUNET_F32 && d->x_dtype != YUNET_BF16)) return YUNET_EINVAL;      // (x_dtype names the build)
    if (backward ? dp_bwd_route(d, d->x_dtype, &r) : dp_fwd_route(d, d->x_dtype, &r)) return YUNET_EINVAL;
    const char *pk = r.packed ? "true" : "false", *pl = r.pool ? "true" : "false", *fl = r.full ? "true" : "false",
               *dt = r.det ? "true" : "false";
    char buf[96];
    int len = -1;
    switch (r.family) {
    case DP_FWD16S: len = snprintf(buf, sizeof buf, "dp_fwd16s_kernel<%d,%s,%s>", r.cout, pl, dt); break;
    case DP_FWD64S: len = snprintf(buf, sizeof buf, "dp_fwd64s_kernel<%s,%s>", pl, dt); break;
    case DP_BWD16S: len = snprintf(buf, sizeof buf, "dp_bwd16s_kernel<%s,%s>", pl, dt); break;
    case DP_BWD64: len = snprintf(buf, sizeof buf, "dp_bwd64_kernel<%d,%s,%s,%s>", r.nw, pk, pl, dt); break;
    case DP_TILE:
        len = backward ? snprintf(buf, sizeof buf, "dp_bwd_kernel<%d,%d,%d,%d,%s,%d,%s,%s,%s>", r.cin, r.cout, r.th, r.tw, pk, r.gemm, pl, fl, dt)
                       : snprintf(buf, sizeof buf, "dp_fwd_kernel<%d,%d,%d,%d,%s,%s,%s>", r.cin, r.cout, r.th, r.tw, pk, pl, dt);
        break;
    }
    if (len < 0 || len >= (int)sizeof buf || len >= cap) return YUNET_EINVAL;
    memcpy(name, buf, (size_t)len + 1);
    return 0;
}
extern "C" int yunet_stem_bwd_blocks(int N, int H, int W) {
    const long long tiles = (long long)N * ((W / 2 + SB_TW - 1) / SB_TW) * ((H / 2 + SB_TH - 1) / SB_TH);
    return (int)(tiles < STEM_BWD_MAX_BLOCKS ? tiles : STEM_BWD_MAX_BLOCKS);
}

// the same weight gradient on the matrix cores with z RECOMPUTED from the image (w [16,3,3,3], b [16]: the stem's
// parameters) instead of read: 112 instead of 176 bytes per output pixel (conv_stem.hip)
extern "C" int yunet_stem_bwd_rz(const float* img, const float* w, const float* b, const float* dy, const YunetBN* bn,
                                 float* wgrad_partials, int wgrad_blocks, int N, int H, int W, int cmid, void* stream) {
    if (cmid != 16 || (H & 1) || (W & 1) || !w || !b || !bn->bstats || wgrad_blocks != yunet_stem_bwd_blocks(N, H, W)) return YUNET_EINVAL;
    return launch_stem_bwd_mma(img, w, b, dy, bn, wgrad_partials, wgrad_blocks, N, H, W, (hipStream_t)stream);
}

extern "C" int yunet_bn_param_grad(const double* bstats, float* dgamma, float* dbeta, int C,
                                   int accumulate, void* stream) {
    hipLaunchKernelGGL(bn_param_grad_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       bstats, dgamma, dbeta, C, accumulate);
    return hip_status();
}

extern "C" int yunet_reduce_partials(const float* partials, int blocks, int width, float* out,
                                     int accumulate, void* stream) {
    if (blocks < 1 || width < 1) return YUNET_EINVAL;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((width + 63) / 64), dim3(1024), 0,
                       (hipStream_t)stream, partials, blocks, width, out, accumulate);
    return hip_status();
}

extern "C" int yunet_reduce_partials_batch(const YunetReduceJob* jobs, int njobs, int total_chunks,
                                           void* stream) {
    if (!jobs || njobs < 1 || total_chunks < njobs) return YUNET_EINVAL;
    hipLaunchKernelGGL(reduce_partials_batch_kernel, dim3(total_chunks), dim3(1024), 0,
                       (hipStream_t)stream, jobs, njobs);
    return hip_status();
}
