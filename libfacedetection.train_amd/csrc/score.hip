// score.hip -- scoring a detection set on the device: the integer stages of
//   * the WIDER-Face protocol (mmdet/core/evaluation/widerface.py:152-239: norm_score, image_eval, img_pr_info), and
//   * EvalHook's mAP (mmdet/core/evaluation/mean_ap.py:168-267: tpfp_default, one class, no area ranges),
// as evaluation.py restates them.  Every result is an integer (a row index, a flag, a count), so the device path is
// exact: the floating-point values that decide them (fp64 / fp32 IoU, the normalised score) are formed with the
// reference's operations in the reference's order, one rounding each (-ffp-contract=off), and compared, never summed.
//
// WIDER, four launches:
//   score_init_kernel   : first[g] = INT_MAX, the min / max keys = the reference's starting values (2.0, -1.0)
//   score_minmax_kernel : min / max of the score column (block reduce, then one 64-bit atomicMin / atomicMax per
//                         workgroup on order-preserving integer keys of the doubles)
//   wider_match_kernel  : one workgroup per image; a thread owns a prediction row, the image's ground truths pass
//                         through LDS YUNET_SCORE_GT_CHUNK at a time (any count); first-index arg-max of the IoU,
//                         hit = IoU >= threshold, atomicMin(first[best], row) = the first row that hit a ground truth
//   wider_count_kernel  : a workgroup walks several images.  Per image: the last row that passes each score threshold
//                         (binary search of the row's smallest passing threshold, atomicMax of the row index in LDS,
//                         running maximum over the thresholds), then tiles of 256 rows: one block scan of six 10-bit
//                         fields (first_s and proposal_s of the three subsets) and a lookup of the thresholds whose
//                         last row lies in the tile.  The [3, T, 2] counters accumulate in LDS and are flushed once.
// mAP, two launches: map_match_kernel (fp32 IoU against kept + ignored boxes, a thread owns a visiting position,
// atomicMin(first[g], position)) and map_tpfp_kernel (tp where the position is the ground truth's first).
//
// Every offset read from a device table is checked against the totals the host passes before it addresses anything.
#include <limits.h>

#include "common.h"

namespace {

constexpr int NT = YUNET_SCORE_BLOCK;
constexpr int CH = YUNET_SCORE_GT_CHUNK;
constexpr int TMAX = YUNET_SCORE_MAX_THRESH;
static_assert(NT == 256 && TMAX == 4 * NT, "the running maximum gives every thread four thresholds");

// order-preserving map of a (non-NaN) double onto an unsigned integer, and back
__device__ __forceinline__ unsigned long long dkey(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dunkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// image i of a packed table: rows [lo, lo + n) when the offsets are sane, else an empty image
__device__ __forceinline__ bool span(const long long* __restrict__ off, int i, long long total, long long& lo,
                                     long long& n) {
    lo = off[i];
    const long long hi = off[i + 1];
    n = hi - lo;
    return lo >= 0 && hi >= lo && hi <= total;
}

// inclusive scan over the workgroup; buf [2][NT]; the result of every thread is left in buf[0 .. NT) (eight steps)
template <class T, class Op>
__device__ __forceinline__ T block_scan(T v, T* buf, Op op) {
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    int src = 0;
#pragma unroll
    for (int d = 1; d < NT; d <<= 1) {
        T x = buf[src * NT + tid];
        if (tid >= d) x = op(buf[src * NT + tid - d], x);
        buf[(src ^ 1) * NT + tid] = x;
        src ^= 1;
        __syncthreads();
    }
    return buf[tid];
}

__global__ __launch_bounds__(NT) void score_init_kernel(int32_t* __restrict__ first, long long G,
                                                        unsigned long long* __restrict__ keys) {
    for (long long g = (long long)blockIdx.x * NT + threadIdx.x; g < G; g += (long long)gridDim.x * NT)
        first[g] = INT_MAX;
    if (keys && blockIdx.x == 0 && threadIdx.x == 0) {
        keys[0] = dkey(2.0);            // norm_score: min_score = 2.0, max_score = -1.0 before the first image
        keys[1] = dkey(-1.0);
    }
}

__global__ __launch_bounds__(NT) void score_minmax_kernel(const double* __restrict__ pred, long long P,
                                                          unsigned long long* __restrict__ keys) {
    __shared__ double s_lo[NT], s_hi[NT];
    double lo = 2.0, hi = -1.0;
    for (long long r = (long long)blockIdx.x * NT + threadIdx.x; r < P; r += (long long)gridDim.x * NT) {
        const double s = pred[r * 5 + 4];
        lo = s < lo ? s : lo;
        hi = s > hi ? s : hi;
    }
    s_lo[threadIdx.x] = lo;
    s_hi[threadIdx.x] = hi;
    __syncthreads();
    for (int d = NT / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            const double a = s_lo[threadIdx.x + d], b = s_hi[threadIdx.x + d];
            if (a < s_lo[threadIdx.x]) s_lo[threadIdx.x] = a;
            if (b > s_hi[threadIdx.x]) s_hi[threadIdx.x] = b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMin(&keys[0], dkey(s_lo[0]));
        atomicMax(&keys[1], dkey(s_hi[0]));
    }
}

// pairwise_iou_xywh + argmax(axis=1) + the >= test of image_eval
__global__ __launch_bounds__(NT) void wider_match_kernel(const double* __restrict__ pred,
                                                         const long long* __restrict__ poff,
                                                         const double* __restrict__ gt,
                                                         const long long* __restrict__ goff, int I, long long P,
                                                         long long Gtot, double thresh, int32_t* __restrict__ best_out,
                                                         uint8_t* __restrict__ hit_out, int32_t* __restrict__ first) {
    __shared__ double sg[CH][5];                    // x1, y1, x2, y2, area of a chunk of ground truths
    const int tid = threadIdx.x;
    for (int i = blockIdx.x; i < I; i += gridDim.x) {
        long long p0, n, g0, G;
        const bool ok = span(poff, i, P, p0, n) & span(goff, i, Gtot, g0, G);
        if (!ok || n == 0 || G == 0) continue;      // (uniform over the workgroup)
        for (long long base = 0; base < n; base += NT) {
            const long long r = base + tid;
            const bool active = r < n;
            double px = 0, py = 0, px2 = 0, py2 = 0, pa = 0;
            if (active) {
                const double* p = pred + (p0 + r) * 5;
                px = p[0];
                py = p[1];
                px2 = px + p[2];
                py2 = py + p[3];
                pa = (px2 - px + 1) * (py2 - py + 1);
            }
            double bestv = -INFINITY;
            int best = 0;
            for (long long c0 = 0; c0 < G; c0 += CH) {
                const int cnt = (int)(G - c0 < CH ? G - c0 : CH);
                __syncthreads();
                for (int j = tid; j < cnt; j += NT) {
                    const double* g = gt + (g0 + c0 + j) * 4;
                    const double x = g[0], y = g[1], x2 = x + g[2], y2 = y + g[3];
                    sg[j][0] = x;
                    sg[j][1] = y;
                    sg[j][2] = x2;
                    sg[j][3] = y2;
                    sg[j][4] = (x2 - x + 1) * (y2 - y + 1);
                }
                __syncthreads();
                if (active) {
                    for (int j = 0; j < cnt; ++j) {
                        const double gx = sg[j][0], gy = sg[j][1], gx2 = sg[j][2], gy2 = sg[j][3], ga = sg[j][4];
                        const double w = (gx2 < px2 ? gx2 : px2) - (gx > px ? gx : px) + 1;
                        const double h = (gy2 < py2 ? gy2 : py2) - (gy > py ? gy : py) + 1;
                        double o = 0.0;
                        if (!(w <= 0 || h <= 0)) {
                            const double inter = w * h;
                            o = inter / (ga + pa - inter);
                        }
                        if (o > bestv) {            // strict: the first index of the maximum, as numpy's argmax
                            bestv = o;
                            best = (int)(c0 + j);
                        }
                    }
                }
            }
            if (active) {
                const bool hit = bestv >= thresh;
                best_out[p0 + r] = best;
                hit_out[p0 + r] = hit ? 1 : 0;
                if (hit) atomicMin(&first[g0 + best], (int)r);
            }
        }
    }
}

__global__ __launch_bounds__(NT) void wider_count_kernel(
    const double* __restrict__ pred, const long long* __restrict__ poff, const long long* __restrict__ goff,
    const uint8_t* __restrict__ gt_bits, int I, long long P, long long Gtot, const double* __restrict__ thr, int T,
    const unsigned long long* __restrict__ keys, const int32_t* __restrict__ best, const uint8_t* __restrict__ hit,
    const int32_t* __restrict__ first, unsigned long long* __restrict__ counts, double* __restrict__ minmax) {
    __shared__ double s_thr[TMAX];
    __shared__ int s_last[TMAX];
    __shared__ unsigned s_acc[3 * TMAX * 2];
    __shared__ unsigned long long s_scan[2 * NT];
    __shared__ int s_part[2 * NT];
    const int tid = threadIdx.x;
    const double lo = dunkey(keys[0]), hi = dunkey(keys[1]);
    const double diff = hi - lo;
    if (blockIdx.x == 0 && tid == 0) {
        minmax[0] = lo;
        minmax[1] = hi;
    }
    for (int t = tid; t < T; t += NT) s_thr[t] = thr[t];
    for (int k = tid; k < 3 * T * 2; k += NT) s_acc[k] = 0;
    __syncthreads();
    for (int i = blockIdx.x; i < I; i += gridDim.x) {
        long long p0, n, g0, G;
        const bool ok = span(poff, i, P, p0, n) & span(goff, i, Gtot, g0, G);
        if (!ok || n == 0 || G == 0) continue;      // images without predictions or ground truths count nothing
        for (int t = tid; t < T; t += NT) s_last[t] = -1;
        __syncthreads();
        // the smallest threshold index a row passes (thr[] is non-increasing, so "passes" is monotone in t)
        for (long long r = tid; r < n; r += NT) {
            const double s = (pred[(p0 + r) * 5 + 4] - lo) / diff;
            if (s >= s_thr[T - 1]) {                // NaN (one distinct score: 0 / 0) passes nothing
                int a = 0, b = T - 1;
                while (a < b) {
                    const int mid = (a + b) >> 1;
                    if (s >= s_thr[mid]) b = mid; else a = mid + 1;
                }
                atomicMax(&s_last[a], (int)r);
            }
        }
        __syncthreads();
        // last[t] = the largest row index whose smallest passing threshold is <= t
        int run[4], m = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = tid * 4 + k;
            const int v = t < T ? s_last[t] : -1;
            m = v > m ? v : m;
            run[k] = m;
        }
        block_scan(m, s_part, [](int a, int b) { return a > b ? a : b; });
        const int before = tid > 0 ? s_part[tid - 1] : -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = tid * 4 + k;
            if (t < T) s_last[t] = run[k] > before ? run[k] : before;
        }
        __syncthreads();
        unsigned carry[6] = {0, 0, 0, 0, 0, 0};     // first_s (0..2) and proposal_s (3..5) summed over earlier tiles
        for (long long base = 0; base < n; base += NT) {
            const long long r = base + tid;
            unsigned long long word = 0;
            if (r < n) {
                const int b = best[p0 + r];
                const bool h = hit[p0 + r] != 0 && b >= 0 && b < G;
                unsigned bits = 0;
                bool fh = false;
                if (h) {
                    bits = gt_bits[g0 + b];
                    fh = first[g0 + b] == (int)r;
                }
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const bool in = (bits >> s) & 1;
                    const unsigned long long f = h && in && fh, pr = !(h && !in);
                    word |= (f << (10 * s)) | (pr << (30 + 10 * s));
                }
            }
            block_scan(word, s_scan, [](unsigned long long a, unsigned long long b) { return a + b; });
            for (int t = tid; t < T; t += NT) {
                const long long L = s_last[t];
                if (L >= base && L < base + NT) {
                    const unsigned long long w = s_scan[L - base];
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        s_acc[(s * T + t) * 2 + 0] += carry[3 + s] + (unsigned)((w >> (30 + 10 * s)) & 1023);
                        s_acc[(s * T + t) * 2 + 1] += carry[s] + (unsigned)((w >> (10 * s)) & 1023);
                    }
                }
            }
            const unsigned long long tot = s_scan[NT - 1];
#pragma unroll
            for (int s = 0; s < 6; ++s) carry[s] += (unsigned)((tot >> (10 * s)) & 1023);
            __syncthreads();
        }
    }
    __syncthreads();
    for (int k = tid; k < 3 * T * 2; k += NT)
        if (s_acc[k]) atomicAdd(&counts[k], (unsigned long long)s_acc[k]);
}

// bbox_overlaps_np + max / argmax over kept and ignored boxes + the >= test of tpfp_default, by visiting position
__global__ __launch_bounds__(NT) void map_match_kernel(const float* __restrict__ det,
                                                       const long long* __restrict__ doff,
                                                       const float* __restrict__ gt,
                                                       const long long* __restrict__ goff,
                                                       const int32_t* __restrict__ kept,
                                                       const int32_t* __restrict__ order, int I, long long D,
                                                       long long Gtot, float thresh, int32_t* __restrict__ code,
                                                       int32_t* __restrict__ first) {
    __shared__ float sg[CH][5];
    const int tid = threadIdx.x;
    for (int i = blockIdx.x; i < I; i += gridDim.x) {
        long long d0, n, g0, G;
        const bool ok = span(doff, i, D, d0, n) & span(goff, i, Gtot, g0, G);
        if (!ok || n == 0 || G == 0) continue;
        const int nk = kept[i];
        for (long long base = 0; base < n; base += NT) {
            const long long k = base + tid;
            long long row = -1;
            if (k < n) {
                row = order[d0 + k];
                if (row < 0 || row >= n) row = -1;
            }
            const bool active = row >= 0;
            float x1 = 0, y1 = 0, x2 = 0, y2 = 0, a1 = 0;
            if (active) {
                const float* p = det + (d0 + row) * 5;
                x1 = p[0];
                y1 = p[1];
                x2 = p[2];
                y2 = p[3];
                a1 = (x2 - x1) * (y2 - y1);
            }
            float bestv = -INFINITY;
            int best = 0;
            for (long long c0 = 0; c0 < G; c0 += CH) {
                const int cnt = (int)(G - c0 < CH ? G - c0 : CH);
                __syncthreads();
                for (int j = tid; j < cnt; j += NT) {
                    const float* g = gt + (g0 + c0 + j) * 4;
                    const float a = g[0], b = g[1], c = g[2], d = g[3];
                    sg[j][0] = a;
                    sg[j][1] = b;
                    sg[j][2] = c;
                    sg[j][3] = d;
                    sg[j][4] = (c - a) * (d - b);
                }
                __syncthreads();
                if (active) {
                    for (int j = 0; j < cnt; ++j) {
                        const float xs = x1 > sg[j][0] ? x1 : sg[j][0], ys = y1 > sg[j][1] ? y1 : sg[j][1];
                        const float xe = x2 < sg[j][2] ? x2 : sg[j][2], ye = y2 < sg[j][3] ? y2 : sg[j][3];
                        const float dw = xe - xs, dh = ye - ys;
                        const float overlap = (dw > 0.0f ? dw : 0.0f) * (dh > 0.0f ? dh : 0.0f);
                        float uni = a1 + sg[j][4] - overlap;
                        uni = uni > 1e-6f ? uni : 1e-6f;
                        const float o = overlap / uni;
                        if (o > bestv) {
                            bestv = o;
                            best = (int)(c0 + j);
                        }
                    }
                }
            }
            if (k < n) {
                int c = -3;                                     // a position whose row index is out of range
                if (active) {
                    if (!(bestv >= thresh)) c = -1;             // below the threshold: fp
                    else if (best >= nk) c = -2;                // best box is an ignored one: neither
                    else {
                        c = best;
                        atomicMin(&first[g0 + best], (int)k);
                    }
                }
                code[d0 + k] = c;
            }
        }
    }
}

__global__ __launch_bounds__(NT) void map_tpfp_kernel(const long long* __restrict__ doff,
                                                      const long long* __restrict__ goff,
                                                      const int32_t* __restrict__ order, int I, long long D,
                                                      long long Gtot, const int32_t* __restrict__ code,
                                                      const int32_t* __restrict__ first, float* __restrict__ tp,
                                                      float* __restrict__ fp) {
    for (int i = blockIdx.x; i < I; i += gridDim.x) {
        long long d0, n, g0, G;
        const bool ok = span(doff, i, D, d0, n) & span(goff, i, Gtot, g0, G);
        if (!ok) continue;
        for (long long k = threadIdx.x; k < n; k += NT) {
            const long long row = order[d0 + k];
            if (row < 0 || row >= n) continue;
            float t = 0.0f, f = 0.0f;
            if (G == 0) {
                f = 1.0f;                                       // no box at all, kept or ignored: every row is fp
            } else {
                const int c = code[d0 + k];
                if (c >= 0 && c < G) {
                    if (first[g0 + c] == (int)k) t = 1.0f; else f = 1.0f;
                } else if (c == -1) {
                    f = 1.0f;
                }
            }
            tp[d0 + row] = t;
            fp[d0 + row] = f;
        }
    }
}

int grid_for(long long work) {
    long long b = (work + NT - 1) / NT;
    return (int)(b < 1 ? 1 : b > 1024 ? 1024 : b);
}

}  // namespace

extern "C" int yunet_score_wider_match(const double* pred, const long long* pred_off, const double* gt,
                                       const long long* gt_off, int I, long long P, long long G, double iou_thresh,
                                       int32_t* best, uint8_t* hit, int32_t* first, void* stream) {
    if (I < 0 || P < 0 || G < 0 || P > INT_MAX || G > INT_MAX) return YUNET_EINVAL;
    if (I == 0) return 0;
    if (!pred_off || !gt_off || (P > 0 && (!pred || !best || !hit)) || (G > 0 && (!gt || !first))) return YUNET_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (G > 0) hipLaunchKernelGGL(score_init_kernel, dim3(grid_for(G)), dim3(NT), 0, s, first, G, nullptr);
    if (P > 0 && G > 0)
        hipLaunchKernelGGL(wider_match_kernel, dim3(I < 8192 ? I : 8192), dim3(NT), 0, s, pred, pred_off, gt, gt_off, I,
                           P, G, iou_thresh, best, hit, first);
    return hip_status();
}

extern "C" int yunet_score_wider(const double* pred, const long long* pred_off, const double* gt,
                                 const long long* gt_off, const uint8_t* gt_bits, int I, long long P, long long G,
                                 double iou_thresh, const double* thr, int n_thr, int32_t* best, uint8_t* hit,
                                 int32_t* first, unsigned long long* keys, unsigned long long* counts, double* minmax,
                                 void* stream) {
    if (I < 0 || P < 0 || G < 0 || P > INT_MAX || G > INT_MAX || n_thr < 1 || n_thr > TMAX) return YUNET_EINVAL;
    if (!pred_off || !gt_off || !thr || !keys || !counts || !minmax) return YUNET_EINVAL;
    if ((P > 0 && (!pred || !best || !hit)) || (G > 0 && (!gt || !gt_bits || !first))) return YUNET_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(unsigned long long) * 3 * n_thr * 2, s) != hipSuccess) return hip_status();
    hipLaunchKernelGGL(score_init_kernel, dim3(grid_for(G)), dim3(NT), 0, s, first, G, keys);
    if (P > 0) hipLaunchKernelGGL(score_minmax_kernel, dim3(grid_for(P) < 256 ? grid_for(P) : 256), dim3(NT), 0, s, pred, P, keys);
    if (I > 0 && P > 0 && G > 0)
        hipLaunchKernelGGL(wider_match_kernel, dim3(I < 8192 ? I : 8192), dim3(NT), 0, s, pred, pred_off, gt, gt_off, I,
                           P, G, iou_thresh, best, hit, first);
    // always launched: it also writes minmax; images are spread over at most 256 workgroups, each flushing once
    hipLaunchKernelGGL(wider_count_kernel, dim3(I < 1 ? 1 : I < 256 ? I : 256), dim3(NT), 0, s, pred, pred_off, gt_off,
                       gt_bits, I, P, G, thr, n_thr, keys, best, hit, first, counts, minmax);
    return hip_status();
}

extern "C" int yunet_score_map_tpfp(const float* dets, const long long* det_off, const float* gts,
                                    const long long* gt_off, const int32_t* kept, const int32_t* order, int I,
                                    long long D, long long G, float iou_thr, int32_t* code, int32_t* first, float* tp,
                                    float* fp, void* stream) {
    if (I < 0 || D < 0 || G < 0 || D > INT_MAX || G > INT_MAX) return YUNET_EINVAL;
    if (I == 0 || D == 0) return 0;
    if (!det_off || !gt_off || !kept || !dets || !order || !code || !tp || !fp || (G > 0 && (!gts || !first)))
        return YUNET_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(tp, 0, sizeof(float) * D, s) != hipSuccess) return hip_status();
    if (hipMemsetAsync(fp, 0, sizeof(float) * D, s) != hipSuccess) return hip_status();
    const int grid = I < 8192 ? I : 8192;
    if (G > 0) {
        hipLaunchKernelGGL(score_init_kernel, dim3(grid_for(G)), dim3(NT), 0, s, first, G, nullptr);
        hipLaunchKernelGGL(map_match_kernel, dim3(grid), dim3(NT), 0, s, dets, det_off, gts, gt_off, kept, order, I, D, G,
                           iou_thr, code, first);
    }
    hipLaunchKernelGGL(map_tpfp_kernel, dim3(grid), dim3(NT), 0, s, det_off, gt_off, order, I, D, G, code, first, tp, fp);
    return hip_status();
}
