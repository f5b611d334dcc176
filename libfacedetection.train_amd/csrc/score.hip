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
// mAP, the ranking and the curve (eval_map_single_class(rank='device')).  Scores are compared through rank_key: an
// order-preserving 32-bit integer of the fp32 score, inverted, so that ascending keys are descending scores; ties keep
// the row order (np.argsort(-s, kind='stable')).
//   rank_images_kernel    : the `order` table map_match_kernel visits, one workgroup per image.  A row's position is
//                           the number of rows of its image that come before it, counted against the image's keys in
//                           LDS: all of them at once up to YUNET_RANK_SEG_CAP rows, in chunks of that size beyond.
//   radix_*_kernel        : the ranking of the whole set, a least-significant-digit radix sort of (key, index) pairs in
//                           four 8-bit passes.  Per pass: the digit histogram of every tile of YUNET_RANK_RADIX_TILE
//                           elements, one exclusive scan of the [digit][tile] table (one workgroup, a thread owns a
//                           digit), and the scatter: a tile is walked in rows of 256 elements in order; within a row
//                           the elements of a wave that share a digit find each other with eight ballots, the waves'
//                           counts pass through LDS, and thread d keeps digit d's next free slot.  Every step is a
//                           count, so the result is the same on every run.
//   curve_*_kernel        : tp / fp gathered in ranked order, summed as integers (tile sums, one scan of them, the
//                           scan inside the tiles), converted to fp32; precision = ctp / max(ctp + cfp, eps), one
//                           rounding per operation; the tiles' maxima, their suffix maximum, and the reverse running
//                           maximum of the precision (the envelope).  No atomics on any result.
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

// ---------------------------------------------------------------------------------- mAP: ranking and curve
constexpr int SEG = YUNET_RANK_SEG_CAP;
constexpr int RT = YUNET_RANK_RADIX_TILE;
constexpr int ROWS = RT / NT;                      // rows of 256 elements in a tile = elements a thread owns in a scan
static_assert(SEG % NT == 0 && RT % NT == 0 && NT == 256, "a thread per digit, whole rows per tile");

// ascending key = descending score (finite scores; -0.0 would rank after +0.0, a NaN by its bit pattern)
__device__ __forceinline__ uint32_t rank_key(float s) {
    const uint32_t b = (uint32_t)__float_as_int(s);
    return (b >> 31) ? b : (~b & 0x7fffffffu);
}

// rows of the chunk skey[0 .. cnt) (rows c0 .. c0 + cnt of the image) that come before row r with key `mine`
__device__ __forceinline__ int rows_before(const uint32_t* skey, int cnt, long long c0, uint32_t mine, long long r) {
    int pos = 0;
    for (int j = 0; j < cnt; ++j) {
        const uint32_t k = skey[j];
        pos += (k < mine) | ((k == mine) & (c0 + j < r));
    }
    return pos;
}

__global__ __launch_bounds__(NT) void rank_images_kernel(const float* __restrict__ det,
                                                         const long long* __restrict__ doff, int I, long long D,
                                                         int32_t* __restrict__ order) {
    __shared__ uint32_t skey[SEG];
    const int tid = threadIdx.x;
    for (int i = blockIdx.x; i < I; i += gridDim.x) {
        long long d0, n;
        if (!span(doff, i, D, d0, n) || n == 0) continue;          // (uniform over the workgroup)
        if (n <= SEG) {                                             // the whole image in LDS
            __syncthreads();
            for (int j = tid; j < n; j += NT) skey[j] = rank_key(det[(d0 + j) * 5 + 4]);
            __syncthreads();
            for (int r = tid; r < n; r += NT) order[d0 + rows_before(skey, (int)n, 0, skey[r], r)] = r;
        } else {                                                    // a thread owns a row, the image passes in chunks
            for (long long base = 0; base < n; base += NT) {
                const long long r = base + tid;
                const bool active = r < n;
                const uint32_t mine = active ? rank_key(det[(d0 + r) * 5 + 4]) : 0u;
                long long pos = 0;
                for (long long c0 = 0; c0 < n; c0 += SEG) {
                    const int cnt = (int)(n - c0 < SEG ? n - c0 : SEG);
                    __syncthreads();
                    for (int j = tid; j < cnt; j += NT) skey[j] = rank_key(det[(d0 + c0 + j) * 5 + 4]);
                    __syncthreads();
                    if (active) pos += rows_before(skey, cnt, c0, mine, r);
                }
                if (active && pos < n) order[d0 + pos] = (int32_t)r;
            }
        }
    }
}

// key and index of element e on the way into a pass: the first pass reads the score column itself
template <bool FIRST>
__device__ __forceinline__ uint32_t radix_key(const float* __restrict__ det, const uint32_t* __restrict__ kin,
                                              long long e) {
    return FIRST ? rank_key(det[e * 5 + 4]) : kin[e];
}

template <bool FIRST>
__global__ __launch_bounds__(NT) void radix_hist_kernel(const float* __restrict__ det,
                                                        const uint32_t* __restrict__ kin, long long D, int shift,
                                                        int nblk, uint32_t* __restrict__ hist) {
    __shared__ unsigned h[NT];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * RT;
    for (int m = 0; m < ROWS; ++m) {
        const long long e = base + m * NT + tid;
        if (e < D) atomicAdd(&h[(radix_key<FIRST>(det, kin, e) >> shift) & 255u], 1u);      // integer counts: exact
    }
    __syncthreads();
    hist[(long long)tid * nblk + blockIdx.x] = h[tid];
}

// hist [256][nblk] -> its exclusive scan in (digit, tile) order, in place.  One workgroup; thread d owns digit d's row.
__global__ __launch_bounds__(NT) void radix_scan_kernel(uint32_t* __restrict__ hist, int nblk) {
    __shared__ unsigned buf[2 * NT];
    const int tid = threadIdx.x;
    uint32_t* row = hist + (long long)tid * nblk;
    unsigned sum = 0;
    for (int b = 0; b < nblk; ++b) sum += row[b];
    unsigned run = block_scan(sum, buf, [](unsigned a, unsigned b) { return a + b; }) - sum;
    for (int b = 0; b < nblk; ++b) {
        const unsigned v = row[b];
        row[b] = run;
        run += v;
    }
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(NT) void radix_scatter_kernel(const float* __restrict__ det,
                                                           const uint32_t* __restrict__ kin,
                                                           const int32_t* __restrict__ iin, long long D, int shift,
                                                           int nblk, const uint32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ kout, int32_t* __restrict__ iout) {
    __shared__ unsigned run[NT];                    // digit d's next free slot of the output
    __shared__ unsigned wcnt[NT / 64][NT];          // this row: elements of wave w with digit d
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    run[tid] = hist[(long long)tid * nblk + blockIdx.x];
#pragma unroll
    for (int v = 0; v < NT / 64; ++v) wcnt[v][tid] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * RT;
    for (int m = 0; m < ROWS; ++m) {
        const long long e = base + m * NT + tid;
        const bool active = e < D;
        uint32_t k = 0;
        int32_t ix = 0;
        if (active) {
            k = radix_key<FIRST>(det, kin, e);
            ix = FIRST ? (int32_t)e : iin[e];
        }
        const unsigned d = (k >> shift) & 255u;
        unsigned long long same = __ballot(active);                 // the wave's active lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const unsigned below = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
        if (active) wcnt[w][d] = (unsigned)__popcll(same);           // (every lane of the group writes the same count)
        __syncthreads();
        if (active) {
            unsigned long long off = (unsigned long long)run[d] + below;
            for (int v = 0; v < w; ++v) off += wcnt[v][d];
            if (off < (unsigned long long)D) {
                iout[off] = ix;
                if (!LAST) kout[off] = k;
            }
        }
        __syncthreads();
        unsigned add = 0;
#pragma unroll
        for (int v = 0; v < NT / 64; ++v) {
            add += wcnt[v][tid];
            wcnt[v][tid] = 0;
        }
        run[tid] += add;
        __syncthreads();
    }
}

// (tp, fp) flags of ranked position e as one word: tp in the low half, fp in the high half (each sum is < 2^24)
__device__ __forceinline__ unsigned long long curve_flags(const float* __restrict__ tp, const float* __restrict__ fp,
                                                          const int32_t* __restrict__ rank, long long e, long long D) {
    if (e >= D) return 0ull;
    const long long row = rank[e];
    if (row < 0 || row >= D) return 0ull;
    return (tp[row] != 0.0f ? 1ull : 0ull) | (fp[row] != 0.0f ? 1ull << 32 : 0ull);
}

__global__ __launch_bounds__(NT) void curve_sum_kernel(const float* __restrict__ tp, const float* __restrict__ fp,
                                                       const int32_t* __restrict__ rank, long long D,
                                                       unsigned long long* __restrict__ tsum) {
    __shared__ unsigned long long buf[2 * NT];
    const long long first = (long long)blockIdx.x * RT + (long long)threadIdx.x * ROWS;
    unsigned long long s = 0;
#pragma unroll
    for (int m = 0; m < ROWS; ++m) s += curve_flags(tp, fp, rank, first + m, D);
    block_scan(s, buf, [](unsigned long long a, unsigned long long b) { return a + b; });
    if (threadIdx.x == 0) tsum[blockIdx.x] = buf[NT - 1];
}

// v [n] -> its exclusive scan (forward) or its exclusive suffix scan (reverse), in place; one workgroup, a thread owns
// a contiguous piece
template <class T, bool REVERSE, class Op>
__device__ __forceinline__ void table_scan(T* __restrict__ v, int n, T identity, T* buf, Op op) {
    const int per = (n + NT - 1) / NT;
    const int piece = REVERSE ? NT - 1 - (int)threadIdx.x : (int)threadIdx.x;      // scanned in thread order
    const int lo = piece * per < n ? piece * per : n, hi = lo + per < n ? lo + per : n;
    T sum = identity;
    for (int j = lo; j < hi; ++j) sum = op(sum, v[j]);
    block_scan(sum, buf, op);
    T run = threadIdx.x > 0 ? buf[threadIdx.x - 1] : identity;
    if (REVERSE) {
        for (int j = hi - 1; j >= lo; --j) {
            const T x = v[j];
            v[j] = run;
            run = op(run, x);
        }
    } else {
        for (int j = lo; j < hi; ++j) {
            const T x = v[j];
            v[j] = run;
            run = op(run, x);
        }
    }
}

__global__ __launch_bounds__(NT) void curve_scan_kernel(unsigned long long* __restrict__ tsum, int nblk) {
    __shared__ unsigned long long buf[2 * NT];
    table_scan<unsigned long long, false>(tsum, nblk, 0ull, buf,
                                          [](unsigned long long a, unsigned long long b) { return a + b; });
}

__global__ __launch_bounds__(NT) void curve_sufmax_kernel(float* __restrict__ tmax, int nblk) {
    __shared__ float buf[2 * NT];
    table_scan<float, true>(tmax, nblk, 0.0f, buf, [](float a, float b) { return a > b ? a : b; });
}

__global__ __launch_bounds__(NT) void curve_prec_kernel(const float* __restrict__ tp, const float* __restrict__ fp,
                                                        const int32_t* __restrict__ rank, long long D,
                                                        const unsigned long long* __restrict__ tsum, float eps,
                                                        float* __restrict__ ctp, float* __restrict__ cfp,
                                                        float* __restrict__ prec, float* __restrict__ tmax) {
    __shared__ unsigned long long buf[2 * NT];
    __shared__ float fbuf[2 * NT];
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * RT + (long long)tid * ROWS;
    unsigned long long inc[ROWS], s = 0;
#pragma unroll
    for (int m = 0; m < ROWS; ++m) {
        s += curve_flags(tp, fp, rank, first + m, D);
        inc[m] = s;
    }
    block_scan(s, buf, [](unsigned long long a, unsigned long long b) { return a + b; });
    const unsigned long long before = tsum[blockIdx.x] + (tid > 0 ? buf[tid - 1] : 0ull);
    float best = 0.0f;                                              // (a precision is never negative)
#pragma unroll
    for (int m = 0; m < ROWS; ++m) {
        if (first + m < D) {
            const unsigned long long c = before + inc[m];
            const float t = (float)(unsigned)(c & 0xffffffffull), f = (float)(unsigned)(c >> 32);     // exact: < 2^24
            const float den = t + f;
            const float p = t / (den > eps ? den : eps);
            ctp[first + m] = t;
            cfp[first + m] = f;
            prec[first + m] = p;
            best = p > best ? p : best;
        }
    }
    block_scan(best, fbuf, [](float a, float b) { return a > b ? a : b; });
    if (tid == 0) tmax[blockIdx.x] = fbuf[NT - 1];
}

// env[e] = max(prec[e ..]): thread t owns piece NT - 1 - t of the tile, so that the scan in thread order runs backwards
__global__ __launch_bounds__(NT) void curve_env_kernel(const float* __restrict__ prec, long long D,
                                                       const float* __restrict__ tmax, float* __restrict__ env) {
    __shared__ float fbuf[2 * NT];
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * RT + (long long)(NT - 1 - tid) * ROWS;
    float p[ROWS], best = 0.0f;
#pragma unroll
    for (int m = 0; m < ROWS; ++m) {
        p[m] = first + m < D ? prec[first + m] : 0.0f;
        best = p[m] > best ? p[m] : best;
    }
    block_scan(best, fbuf, [](float a, float b) { return a > b ? a : b; });
    float run = tmax[blockIdx.x];                                   // (after curve_sufmax_kernel: the later tiles)
    if (tid > 0) run = fbuf[tid - 1] > run ? fbuf[tid - 1] : run;
#pragma unroll
    for (int m = ROWS - 1; m >= 0; --m) {
        run = p[m] > run ? p[m] : run;
        if (first + m < D) env[first + m] = run;
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

// ---- the ranking and the curve of the mAP protocol
static long long rank_tiles(long long D) { return (D + RT - 1) / RT; }

extern "C" size_t yunet_score_rank_scratch_bytes(long long D) {
    if (D < 0 || D > INT_MAX) return 0;
    return (size_t)(4 * (3 * D + 256 * rank_tiles(D)) + 8);
}

extern "C" int yunet_score_rank_images(const float* dets, const long long* det_off, int I, long long D, int32_t* order,
                                       void* stream) {
    if (I < 0 || D < 0 || D > INT_MAX) return YUNET_EINVAL;
    if (I == 0 || D == 0) return 0;
    if (!dets || !det_off || !order) return YUNET_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(order, 0xff, sizeof(int32_t) * D, s) != hipSuccess) return hip_status();      // -1: no row
    hipLaunchKernelGGL(rank_images_kernel, dim3(I < 8192 ? I : 8192), dim3(NT), 0, s, dets, det_off, I, D, order);
    return hip_status();
}

extern "C" int yunet_score_rank_global(const float* dets, long long D, int32_t* rank, void* scratch, void* stream) {
    if (D < 0 || D > INT_MAX) return YUNET_EINVAL;
    if (D == 0) return 0;
    if (!dets || !rank || !scratch || ((uintptr_t)scratch & 7)) return YUNET_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (int)rank_tiles(D);
    uint32_t* ka = (uint32_t*)scratch;
    uint32_t* kb = ka + D;
    int32_t* ia = (int32_t*)(kb + D);
    uint32_t* hist = (uint32_t*)(ia + D);
    const dim3 g(nblk), b(NT);
    // (key, index): scores -> (ka, ia) -> (kb, rank) -> (ka, ia) -> rank
    hipLaunchKernelGGL(radix_hist_kernel<true>, g, b, 0, s, dets, nullptr, D, 0, nblk, hist);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(1), b, 0, s, hist, nblk);
    hipLaunchKernelGGL((radix_scatter_kernel<true, false>), g, b, 0, s, dets, nullptr, nullptr, D, 0, nblk, hist, ka, ia);
    hipLaunchKernelGGL(radix_hist_kernel<false>, g, b, 0, s, dets, ka, D, 8, nblk, hist);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(1), b, 0, s, hist, nblk);
    hipLaunchKernelGGL((radix_scatter_kernel<false, false>), g, b, 0, s, dets, ka, ia, D, 8, nblk, hist, kb, rank);
    hipLaunchKernelGGL(radix_hist_kernel<false>, g, b, 0, s, dets, kb, D, 16, nblk, hist);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(1), b, 0, s, hist, nblk);
    hipLaunchKernelGGL((radix_scatter_kernel<false, false>), g, b, 0, s, dets, kb, rank, D, 16, nblk, hist, ka, ia);
    hipLaunchKernelGGL(radix_hist_kernel<false>, g, b, 0, s, dets, ka, D, 24, nblk, hist);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(1), b, 0, s, hist, nblk);
    hipLaunchKernelGGL((radix_scatter_kernel<false, true>), g, b, 0, s, dets, ka, ia, D, 24, nblk, hist, nullptr, rank);
    return hip_status();
}

extern "C" int yunet_score_map_curve(const float* tp, const float* fp, const int32_t* rank, long long D, float* ctp,
                                     float* cfp, float* prec, float* env, void* scratch, void* stream) {
    if (D < 0 || D >= YUNET_RANK_CURVE_MAX) return YUNET_EINVAL;    // fp32 holds every count below 2^24 exactly
    if (D == 0) return 0;
    if (!tp || !fp || !rank || !ctp || !cfp || !prec || !env || !scratch || ((uintptr_t)scratch & 7)) return YUNET_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (int)rank_tiles(D);
    unsigned long long* tsum = (unsigned long long*)scratch;
    float* tmax = (float*)(tsum + nblk);
    const dim3 g(nblk), b(NT);
    hipLaunchKernelGGL(curve_sum_kernel, g, b, 0, s, tp, fp, rank, D, tsum);
    hipLaunchKernelGGL(curve_scan_kernel, dim3(1), b, 0, s, tsum, nblk);
    hipLaunchKernelGGL(curve_prec_kernel, g, b, 0, s, tp, fp, rank, D, tsum, 1.1920928955078125e-07f, ctp, cfp, prec, tmax);
    hipLaunchKernelGGL(curve_sufmax_kernel, dim3(1), b, 0, s, tmax, nblk);
    hipLaunchKernelGGL(curve_env_kernel, g, b, 0, s, prec, D, tmax, env);
    return hip_status();
}
