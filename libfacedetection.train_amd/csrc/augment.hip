// augment.hip -- the reference TRAIN input pipeline on the device:
//   RandomSquareCrop -> Resize(keep_ratio=False) -> RandomFlip (+ 5-landmark swap) -> collate
// (mmdet/datasets/pipelines/transforms.py:975-1169, 242-299, 425-546; configs/yunet_n.py:36-56).
//
// Two kernels per batch:
//   aug_decide_kernel : one wavefront per image.  Draws the crop scale / window with the
//       reference's retry logic from a counter-based generator (the same 32-bit integer
//       function as oracle/pipeline_oracle.py), tests all box centres per attempt with a wave
//       ballot, then transforms the kept boxes / keypoints (clip, shift, scale, clip, flip) and
//       compacts them order-preserving into the padded [N, Gmax, .] layout the loss step stages.
//   aug_pixels_kernel : one thread per output pixel: flip -> bilinear taps in the (virtual) padded
//       crop -> source uint8 gather, written planar NCHW fp32 (what stem_fwd reads).
//
// Multi-scale training (Resize(multiscale_mode='square_range'), transforms.py:128-149): MS = true makes one more
// bounded draw per image, between the crop draws and the flip draw, and uses S_n = edge / 32 * 32 in place of
// cfg.out_size; CANVAS = true writes image n into the top-left S_n x S_n corner of an out_hw x out_hw canvas whose
// remaining pixels are 0 (DefaultFormatBundle's padding_value through mmcv's collate).
//
// CutOut (transforms.py:2143-2214) is a third launch on the finished batch tensor: aug_cutout_kernel, one workgroup per
// (image, hole).  RandomAffine (transforms.py:2787-3001, with the landmarks) runs in front of it as two launches on the
// finished batch: aug_affine_decide_kernel (draws, matrix, GT) and aug_affine_pixels_kernel (the warp into a second tensor).
//
// Built with -ffp-contract=off: every float operation is the single rounded operation numpy
// performs, so boxes / keypoints are bit-identical to the reference and pixels to the oracle.
#include <cfloat>
#include <cmath>
#include <type_traits>

#include "common.h"

namespace {

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t stream_key(uint32_t seed, uint32_t iteration, uint32_t image) {
    const uint32_t k = mix32(seed ^ (iteration * 0x27D4EB2Fu));
    return mix32(k ^ (image * 0x9E3779B9u));
}
__device__ __forceinline__ uint32_t rand_u32(uint32_t key, uint32_t ctr) {
    return mix32(key ^ (ctr * 0x85EBCA6Bu + 0xC2B2AE35u));
}
__device__ __forceinline__ int bounded(uint32_t u, int n) {   // floor(u / 2^32 * n)
    return (int)(((unsigned long long)u * (unsigned long long)(uint32_t)n) >> 32);
}

__device__ __forceinline__ bool centre_inside(const float* b, int p0, int p1, int p2, int p3) {
    const float cx = (b[0] + b[2]) / 2.0f, cy = (b[1] + b[3]) / 2.0f;    // transforms.py:1081
    return cx > (float)p0 && cy > (float)p1 && cx < (float)p2 && cy < (float)p3;
}

// What RandomSquareCrop (clip to the patch, subtract its origin: transforms.py:1104-1107), Resize._resize_bboxes (scale,
// clip to the output) and RandomFlip.bbox_flip do to one kept row of a key of bbox_fields: the one code path of the GT
// boxes (aug_decide_kernel) and of the ignore boxes (aug_ignore_kernel).
__device__ __forceinline__ void crop_resize_flip_box(const float* b, int p0, int p1, int p2, int p3, float sf, float fS,
                                                     bool flip, float* o) {
    float x1 = fmaxf(b[0], (float)p0) - (float)p0, y1 = fmaxf(b[1], (float)p1) - (float)p1;
    float x2 = fminf(b[2], (float)p2) - (float)p0, y2 = fminf(b[3], (float)p3) - (float)p1;
    x1 = fminf(fmaxf(x1 * sf, 0.0f), fS); y1 = fminf(fmaxf(y1 * sf, 0.0f), fS);
    x2 = fminf(fmaxf(x2 * sf, 0.0f), fS); y2 = fminf(fmaxf(y2 * sf, 0.0f), fS);
    if (flip) { const float t = x1; x1 = fS - x2; x2 = fS - t; }
    o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
}
// the Resize factor of a window of edge cw scaled to S (mmcv.imresize: w_scale = S / w)
__device__ __forceinline__ float resize_factor(int S, int cw) { return (float)((double)S / (double)cw); }

#define AUG_P_LEFT 0
#define AUG_P_TOP 1
#define AUG_P_CW 2
#define AUG_P_FLIP 3
#define AUG_P_KEPT 4
#define AUG_P_DRAWS 5
#define AUG_P_STATUS 6
#define AUG_P_SIZE 7      // MS: S_n of the image; 0 from the fixed-size decide

// MS = false: S = cfg.out_size, scale_lo / scale_hi unused.  MS = true: S = S_n drawn from [scale_lo, scale_hi].
// PAD = false: image n's GT rows are [gt_off[n], gt_off[n + 1]).  PAD = true (the merged GT of mosaic_decide_kernel):
// rows [n * in_gmax, n * in_gmax + gt_off[n]), gt_off holding the counts.
template <bool MS, bool PAD = false>
__global__ __launch_bounds__(64) void aug_decide_kernel(
    const int32_t* __restrict__ src_hw, const float* __restrict__ boxes, const float* __restrict__ kps,
    const int32_t* __restrict__ gt_off, const YunetAugCfg cfg, int scale_lo, int scale_hi, uint32_t iteration,
    int32_t* __restrict__ params, float* __restrict__ out_boxes, float* __restrict__ out_kps,
    int32_t* __restrict__ out_count, int in_gmax) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int h = src_hw[2 * n], w = src_hw[2 * n + 1];
    const int g0 = PAD ? n * in_gmax : gt_off[n];
    const int G = PAD ? (gt_off[n] < 0 ? 0 : gt_off[n] > in_gmax ? in_gmax : gt_off[n]) : gt_off[n + 1] - g0;
    const float* bx = boxes + (size_t)g0 * 4;
    const float* kp = kps + (size_t)g0 * 15;
    const uint32_t key = stream_key(cfg.seed, iteration, (uint32_t)n);
    uint32_t ctr = 0;
    const int gmax = cfg.gmax;
    float* ob = out_boxes + (size_t)n * gmax * 4;
    float* ok = out_kps + (size_t)n * gmax * 15;

    // ---- RandomSquareCrop: scale / window search (transforms.py:1032-1090) --------------------
    int left = 0, top = 0, cw = 0;
    bool found = false;
    const int short_side = w < h ? w : h;
    for (int retry = 0; retry < cfg.max_retries && !found && G > 0; ++retry) {
        const double scale = cfg.crop_choice[bounded(rand_u32(key, ctr++), cfg.n_choice)];
        cw = (int)(scale * (double)short_side);
        for (int attempt = 0; attempt < cfg.max_attempts && !found; ++attempt) {
            if (w == cw) left = 0;
            else if (w > cw) left = bounded(rand_u32(key, ctr++), w - cw);
            else left = (w - cw) + bounded(rand_u32(key, ctr++), cw - w);
            if (h == cw) top = 0;
            else if (h > cw) top = bounded(rand_u32(key, ctr++), h - cw);
            else top = (h - cw) + bounded(rand_u32(key, ctr++), cw - h);
            bool any = false;
            for (int g = lane; g < G; g += 64)
                any |= centre_inside(bx + 4 * g, left, top, left + cw, top + cw);
            found = __any(any);
        }
    }
    // ---- Resize._random_scale, square_range: randint(lo, hi + 1) // 32 * 32 (transforms.py:143-149); drawn for a
    // failed image too, so that its S_n is defined
    int S = cfg.out_size;
    if (MS) S = (scale_lo + bounded(rand_u32(key, ctr++), scale_hi + 1 - scale_lo)) / 32 * 32;
    // ---- RandomFlip: one uniform against flip_ratio (transforms.py:514-521) -------------------
    const bool flip = found && ((double)rand_u32(key, ctr++) * (1.0 / 4294967296.0) < cfg.flip_ratio);

    // ---- kept boxes / keypoints: clip to the window, shift, scale, clip, flip; compact ---------
    int kept = 0;
    if (found) {
        const int p0 = left, p1 = top, p2 = left + cw, p3 = top + cw;
        const float sf = resize_factor(S, cw);
        const float fS = (float)S;
        for (int base = 0; base < G; base += 64) {
            const int g = base + lane;
            const bool keep = g < G && centre_inside(bx + 4 * g, p0, p1, p2, p3);
            const unsigned long long m = __ballot(keep);
            const int idx = kept + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && idx < gmax) {
                crop_resize_flip_box(bx + 4 * g, p0, p1, p2, p3, sf, fS, flip, ob + 4 * idx);
                const float* k = kp + 15 * g;
                float* q = ok + 15 * idx;
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const int js = flip ? (j == 0 ? 1 : j == 1 ? 0 : j == 3 ? 4 : j == 4 ? 3 : 2) : j;
                    float x = fmaxf(fminf(k[3 * js + 0], (float)p2), (float)p0) - (float)p0;
                    float y = fmaxf(fminf(k[3 * js + 1], (float)p3), (float)p1) - (float)p1;
                    x = fminf(fmaxf(x * sf, 0.0f), fS);
                    y = fminf(fmaxf(y * sf, 0.0f), fS);
                    if (flip) x = fS - x;
                    q[3 * j + 0] = x; q[3 * j + 1] = y; q[3 * j + 2] = k[3 * js + 2];
                }
            }
            kept += __popcll(m);
        }
    }
    const int count = kept < gmax ? kept : gmax;
    for (int i = count * 4 + lane; i < gmax * 4; i += 64) ob[i] = 0.0f;     // deterministic padding
    for (int i = count * 15 + lane; i < gmax * 15; i += 64) ok[i] = 0.0f;
    if (lane == 0) {
        int32_t* p = params + 8 * n;
        p[AUG_P_LEFT] = left; p[AUG_P_TOP] = top; p[AUG_P_CW] = found ? cw : 0;
        p[AUG_P_FLIP] = flip ? 1 : 0; p[AUG_P_KEPT] = kept; p[AUG_P_DRAWS] = (int32_t)ctr;
        p[AUG_P_STATUS] = found ? (kept > gmax ? 2 : 0) : 1; p[AUG_P_SIZE] = MS ? S : 0;
        out_count[n] = count;
    }
}

// ---- ignore boxes (gt_bboxes_ignore in bbox_fields): one wavefront per image, after aug_decide_kernel on its stream ------
// Reads the window, flip and S_n the decide left in params and takes the image's ragged ignore rows through the steps the
// GT boxes took: rows whose centre is strictly inside the patch are kept (transforms.py:1102-1103), in order, the first
// `imax` of them written; rows >= the count are zero.  An image whose decide failed (cw == 0) gets count 0.  Draws nothing.
__global__ __launch_bounds__(64) void aug_ignore_kernel(const int32_t* __restrict__ params, const float* __restrict__ ign_boxes,
                                                        const int32_t* __restrict__ ign_off, int out_size, int imax,
                                                        float* __restrict__ out_ign, int32_t* __restrict__ out_icount) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int32_t* p = params + 8 * n;
    const int left = p[AUG_P_LEFT], top = p[AUG_P_TOP], cw = p[AUG_P_CW];
    const bool flip = p[AUG_P_FLIP] != 0;
    const int S = p[AUG_P_SIZE] > 0 ? p[AUG_P_SIZE] : out_size;
    const int i0 = ign_off[n];
    const int I = cw > 0 ? max(ign_off[n + 1] - i0, 0) : 0;
    const float* bx = ign_boxes + (size_t)i0 * 4;
    float* ob = out_ign + (size_t)n * imax * 4;
    int kept = 0;
    if (I > 0) {
        const int p0 = left, p1 = top, p2 = left + cw, p3 = top + cw;
        const float sf = resize_factor(S, cw);
        const float fS = (float)S;
        for (int base = 0; base < I; base += 64) {
            const int g = base + lane;
            const bool keep = g < I && centre_inside(bx + 4 * g, p0, p1, p2, p3);
            const unsigned long long m = __ballot(keep);
            const int idx = kept + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && idx < imax) crop_resize_flip_box(bx + 4 * g, p0, p1, p2, p3, sf, fS, flip, ob + 4 * idx);
            kept += __popcll(m);
        }
    }
    const int count = kept < imax ? kept : imax;
    for (int i = count * 4 + lane; i < imax * 4; i += 64) ob[i] = 0.0f;
    if (lane == 0) out_icount[n] = count;
}

// OpenCV INTER_LINEAR coefficient of one destination coordinate (float32 bilinear, half-pixel
// centres, edge clamp) -- restated in oracle/pipeline_oracle.py:linear_coeffs
__device__ __forceinline__ void lin_coef(int d, int dst, int src, int& s0, int& s1, float& w0, float& w1) {
    const double scale = 1.0 / ((double)dst / (double)src);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= src - 1) { f = 0.0f; s = src - 1; }
    s0 = s;
    s1 = s + 1 < src ? s + 1 : src - 1;
    w0 = 1.0f - f;
    w1 = f;
}

// lin_coef with the coordinate scale 1 / (dst / src) handed in (mosaic_decide_kernel forms it once per sub-image with
// the same double operations): the same s0 / s1 / w0 / w1.
__device__ __forceinline__ void lin_coef_s(int d, double scale, int src, int& s0, int& s1, float& w0, float& w1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= src - 1) { f = 0.0f; s = src - 1; }
    s0 = s;
    s1 = s + 1 < src ? s + 1 : src - 1;
    w0 = 1.0f - f;
    w1 = f;
}

// ---- Mosaic(use_kps=True) (transforms.py:2218-2519; include/yunet_hip.h YUNET_MOSAIC_*) --------------------------------
__device__ __forceinline__ uint32_t mosaic_key(uint32_t seed, uint32_t iteration, uint32_t image) {
    return mix32(stream_key(seed, iteration, image) ^ YUNET_MOSAIC_SALT);
}

// One wavefront per image: the draws, the four sub-images' geometry (all wave-uniform integer / double arithmetic, as
// the Python code has it) and the merged GT, compacted order-preserving like aug_decide_kernel's.
__global__ __launch_bounds__(64) void mosaic_decide_kernel(
    const int32_t* __restrict__ idx, int M, const int32_t* __restrict__ store_hw, const int32_t* __restrict__ store_goff,
    const int32_t* __restrict__ store_gcnt, const float* __restrict__ store_boxes, const float* __restrict__ store_kps,
    const YunetMosaicCfg cfg, uint32_t iteration, int32_t* __restrict__ geom, int32_t* __restrict__ out_hw,
    float* __restrict__ out_boxes, float* __restrict__ out_kps, int32_t* __restrict__ out_count) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const uint32_t key = mosaic_key(cfg.seed, iteration, (uint32_t)n);
    uint32_t ctr = 0;
    const int S = cfg.img_scale, gmax = cfg.gmax;
    int32_t* gm = geom + (size_t)n * YUNET_MOSAIC_WORDS;
    float* ob = out_boxes + (size_t)n * gmax * 4;
    float* ok = out_kps + (size_t)n * gmax * 15;
    for (int i = lane; i < YUNET_MOSAIC_WORDS; i += 64) gm[i] = 0;
    __syncthreads();      // one wavefront: orders the zero fill before the words written below

    int qi[4];
    qi[0] = idx[n];
#pragma unroll
    for (int k = 1; k < 4; ++k) qi[k] = bounded(rand_u32(key, ctr++), M);                       // get_indexes
    const bool applied = !((double)rand_u32(key, ctr++) * (1.0 / 4294967296.0) > cfg.prob);     // transforms.py:2304
    int cx = 0, cy = 0;
    if (applied) {      // random.uniform(a, b) = a + (b - a) * random()
        const double span = cfg.center_hi - cfg.center_lo;
        cx = (int)((cfg.center_lo + span * ((double)rand_u32(key, ctr++) * (1.0 / 4294967296.0))) * (double)S);
        cy = (int)((cfg.center_lo + span * ((double)rand_u32(key, ctr++) * (1.0 / 4294967296.0))) * (double)S);
    }
    const float lim = (float)(2 * S);
    int kept = 0, status = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!applied && q > 0) break;
        const int i = qi[q];
        const bool ok_i = i >= 0 && i < M;
        const int h = ok_i ? store_hw[2 * i] : 0, w = ok_i ? store_hw[2 * i + 1] : 0;
        const int G = ok_i ? store_gcnt[i] : 0;
        const size_t g0 = ok_i ? (size_t)store_goff[i] : 0;
        float r = 1.0f, padw = 0.0f, padh = 0.0f;
        if (applied) {
            int rw = 0, rh = 0, x1 = 0, y1 = 0, x2 = 0, y2 = 0, c1 = 0, c2 = 0;
            double sx = 0.0, sy = 0.0, ratio = 1.0;
            if (h > 0 && w > 0) {
                const double rh_ = (double)S / (double)h, rw_ = (double)S / (double)w;
                ratio = rh_ < rw_ ? rh_ : rw_;                                                // min(S / h, S / w)
                rw = (int)((double)w * ratio);
                rh = (int)((double)h * ratio);
            }
            if (rw > 0 && rh > 0) {       // _mosaic_combine, transforms.py:2442-2501
                if (q == 0) {
                    x1 = cx - rw > 0 ? cx - rw : 0; y1 = cy - rh > 0 ? cy - rh : 0; x2 = cx; y2 = cy;
                    c1 = rw - (x2 - x1); c2 = rh - (y2 - y1);
                } else if (q == 1) {
                    x1 = cx; y1 = cy - rh > 0 ? cy - rh : 0; x2 = cx + rw < 2 * S ? cx + rw : 2 * S; y2 = cy;
                    c1 = 0; c2 = rh - (y2 - y1);
                } else if (q == 2) {
                    x1 = cx - rw > 0 ? cx - rw : 0; y1 = cy; x2 = cx; y2 = cy + rh < 2 * S ? cy + rh : 2 * S;
                    c1 = rw - (x2 - x1); c2 = 0;
                } else {
                    x1 = cx; y1 = cy; x2 = cx + rw < 2 * S ? cx + rw : 2 * S; y2 = cy + rh < 2 * S ? cy + rh : 2 * S;
                    c1 = 0; c2 = 0;
                }
                sx = 1.0 / ((double)rw / (double)w);
                sy = 1.0 / ((double)rh / (double)h);
            } else {
                status |= 4;
            }
            r = (float)ratio; padw = (float)(x1 - c1); padh = (float)(y1 - c2);
            if (lane == 0) {
                int32_t* gq = gm + YUNET_MOSAIC_QUAD + q * YUNET_MOSAIC_QWORDS;
                gq[YUNET_MOSAIC_Q_IDX] = ok_i ? i : 0; gq[YUNET_MOSAIC_Q_H] = h; gq[YUNET_MOSAIC_Q_W] = w;
                gq[YUNET_MOSAIC_Q_RW] = rw; gq[YUNET_MOSAIC_Q_RH] = rh;
                gq[YUNET_MOSAIC_Q_PX1] = x1; gq[YUNET_MOSAIC_Q_PY1] = y1; gq[YUNET_MOSAIC_Q_PX2] = x2;
                gq[YUNET_MOSAIC_Q_PY2] = y2; gq[YUNET_MOSAIC_Q_CX1] = c1; gq[YUNET_MOSAIC_Q_CY1] = c2;
                *reinterpret_cast<double*>(gq + YUNET_MOSAIC_Q_SX) = sx;
                *reinterpret_cast<double*>(gq + YUNET_MOSAIC_Q_SY) = sy;
            }
        } else if (lane == 0) {
            int32_t* gq = gm + YUNET_MOSAIC_QUAD;
            gq[YUNET_MOSAIC_Q_IDX] = ok_i ? i : 0; gq[YUNET_MOSAIC_Q_H] = h; gq[YUNET_MOSAIC_Q_W] = w;
        }
        if (q == 0 && lane == 0) {
            out_hw[2 * n] = applied ? 2 * S : h;
            out_hw[2 * n + 1] = applied ? 2 * S : w;
        }
        const float* bx = store_boxes + g0 * 4;
        const float* kp = store_kps + g0 * 15;
        for (int base = 0; base < G; base += 64) {
            const int g = base + lane;
            float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            bool keep = g < G;
            if (keep) {
#pragma unroll
                for (int e = 0; e < 4; ++e) b[e] = bx[4 * g + e];
                if (applied) {
                    b[0] = r * b[0] + padw; b[2] = r * b[2] + padw;       // transforms.py:2388-2391, fp32
                    b[1] = r * b[1] + padh; b[3] = r * b[3] + padh;
                    if (cfg.bbox_clip_border) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) b[e] = fminf(fmaxf(b[e], 0.0f), lim);
                    }
                    if (!cfg.skip_filter)
                        keep = (b[2] - b[0] > cfg.min_bbox_size) && (b[3] - b[1] > cfg.min_bbox_size);
                    keep = keep && b[0] < lim && b[2] > 0.0f && b[1] < lim && b[3] > 0.0f;     // find_inside_bboxes
                }
            }
            const unsigned long long m = __ballot(keep);
            const int at = kept + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && at < gmax) {
                float* o = ob + 4 * at;
                o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
                const float* k = kp + 15 * g;
                float* t = ok + 15 * at;
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    float x = k[3 * j], y = k[3 * j + 1];
                    if (applied) {
                        x = r * x + padw; y = r * y + padh;
                        if (cfg.bbox_clip_border) { x = fminf(fmaxf(x, 0.0f), lim); y = fminf(fmaxf(y, 0.0f), lim); }
                    }
                    t[3 * j] = x; t[3 * j + 1] = y; t[3 * j + 2] = k[3 * j + 2];
                }
            }
            kept += __popcll(m);
        }
    }
    const int count = kept < gmax ? kept : gmax;
    for (int i = count * 4 + lane; i < gmax * 4; i += 64) ob[i] = 0.0f;
    for (int i = count * 15 + lane; i < gmax * 15; i += 64) ok[i] = 0.0f;
    if (lane == 0) {
        gm[YUNET_MOSAIC_APPLIED] = applied ? 1 : 0; gm[YUNET_MOSAIC_CX] = cx; gm[YUNET_MOSAIC_CY] = cy;
        gm[YUNET_MOSAIC_DRAWS] = (int32_t)ctr; gm[YUNET_MOSAIC_KEPT] = kept;
        gm[YUNET_MOSAIC_STATUS] = status | (kept > gmax ? 2 : 0);
        out_count[n] = count;
    }
}

// One pixel (X, Y) of the mosaic canvas of the image whose table is g: quadrant by the centre, pad_val outside the
// paste rectangle, else the pixel of the resized sub-image -- cv2's float bilinear of the uint8 source, horizontal pass
// then vertical pass, each product and sum rounded to fp32 (the file is built without contraction).  lin_coef_s clamps
// both taps to the source, so whatever the table holds nothing outside sub-image idx is read.
__device__ __forceinline__ void mosaic_tap(const int32_t* __restrict__ g, const uint8_t* __restrict__ store,
                                           const long long* __restrict__ store_off, int cx, int cy, int X, int Y,
                                           float mpad, float* __restrict__ o) {
    const int q = (X >= cx ? 1 : 0) + (Y >= cy ? 2 : 0);
    const int32_t* gq = g + YUNET_MOSAIC_QUAD + q * YUNET_MOSAIC_QWORDS;
    const int4 A = *reinterpret_cast<const int4*>(gq);          // idx, h, w, rw
    const int4 B = *reinterpret_cast<const int4*>(gq + 4);      // rh, px1, py1, px2
    const int4 D = *reinterpret_cast<const int4*>(gq + 8);      // py2, cx1, cy1, -
    if (X < B.y || X >= B.w || Y < B.z || Y >= D.x || A.y < 1 || A.z < 1) {
        o[0] = mpad; o[1] = mpad; o[2] = mpad;
        return;
    }
    const double2 sc = *reinterpret_cast<const double2*>(gq + YUNET_MOSAIC_Q_SX);
    int sx0, sx1, sy0, sy1;
    float a0, a1, b0, b1;
    lin_coef_s(X - B.y + D.y, sc.x, A.z, sx0, sx1, a0, a1);
    lin_coef_s(Y - B.z + D.z, sc.y, A.y, sy0, sy1, b0, b1);
    const uint8_t* im = store + store_off[A.x];
    const uint8_t* r0 = im + (size_t)sy0 * A.z * 3;
    const uint8_t* r1 = im + (size_t)sy1 * A.z * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t0 = (float)r0[3 * sx0 + c] * a0 + (float)r0[3 * sx1 + c] * a1;
        const float t1 = (float)r1[3 * sx0 + c] * a0 + (float)r1[3 * sx1 + c] * a1;
        o[c] = t0 * b0 + t1 * b1;
    }
}

// Test entry: every canvas pixel through mosaic_tap, written HWC fp32 as the reference holds its canvas.
__global__ __launch_bounds__(256) void mosaic_canvas_kernel(const uint8_t* __restrict__ store,
                                                            const long long* __restrict__ store_off,
                                                            const int32_t* __restrict__ geom, int S, float mpad,
                                                            float* __restrict__ canvas) {
    const int n = blockIdx.y, E = 2 * S;
    const int32_t* g = geom + (size_t)n * YUNET_MOSAIC_WORDS;
    const int applied = g[YUNET_MOSAIC_APPLIED], cx = g[YUNET_MOSAIC_CX], cy = g[YUNET_MOSAIC_CY];
    float* o = canvas + (size_t)n * E * E * 3;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < E * E; i += gridDim.x * 256) {
        float v[3] = {mpad, mpad, mpad};
        if (applied) mosaic_tap(g, store, store_off, cx, cy, i % E, i / E, mpad, v);
        o[3 * (size_t)i] = v[0]; o[3 * (size_t)i + 1] = v[1]; o[3 * (size_t)i + 2] = v[2];
    }
}

// ---- PhotoMetricDistortion (transforms.py:1211-1312; include/yunet_hip.h YUNET_PHOTO_*) ------------------------
__device__ __forceinline__ uint32_t photo_key(uint32_t seed, uint32_t iteration, uint32_t image) {
    return mix32(stream_key(seed, iteration, image) ^ YUNET_PHOTO_SALT);
}
// numpy.random.uniform(a, b) = a + (b - a) * random_sample() in double; the image op rounds it to fp32 once
__device__ __forceinline__ float photo_uniform(uint32_t u, double a, double b) {
    return (float)(a + (b - a) * ((double)u * (1.0 / 4294967296.0)));
}

__global__ __launch_bounds__(64) void aug_photometric_kernel(const YunetPhotoCfg cfg, uint32_t seed, uint32_t iteration,
                                                             int N, float* __restrict__ pp) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const uint32_t key = photo_key(seed, iteration, (uint32_t)n);
    uint32_t ctr = 0;
    float t[YUNET_PHOTO_WORDS];
#pragma unroll
    for (int k = 0; k < YUNET_PHOTO_WORDS; ++k) t[k] = 0.0f;
    if (rand_u32(key, ctr++) >> 31) {                     // randint(2): brightness
        t[YUNET_PHOTO_BRIGHT] = 1.0f;
        t[YUNET_PHOTO_DELTA] = photo_uniform(rand_u32(key, ctr++), -cfg.brightness_delta, cfg.brightness_delta);
    }
    const uint32_t mode = rand_u32(key, ctr++) >> 31;
    t[YUNET_PHOTO_MODE] = (float)mode;
    if (mode == 1 && (rand_u32(key, ctr++) >> 31)) {      // contrast first
        t[YUNET_PHOTO_CONTRAST] = 1.0f;
        t[YUNET_PHOTO_ALPHA] = photo_uniform(rand_u32(key, ctr++), cfg.contrast_lower, cfg.contrast_upper);
    }
    if (rand_u32(key, ctr++) >> 31) {                     // saturation
        t[YUNET_PHOTO_SAT] = 1.0f;
        t[YUNET_PHOTO_SAT_F] = photo_uniform(rand_u32(key, ctr++), cfg.saturation_lower, cfg.saturation_upper);
    }
    if (rand_u32(key, ctr++) >> 31) {                     // hue
        t[YUNET_PHOTO_HUE] = 1.0f;
        t[YUNET_PHOTO_HUE_D] = photo_uniform(rand_u32(key, ctr++), -cfg.hue_delta, cfg.hue_delta);
    }
    if (mode == 0 && (rand_u32(key, ctr++) >> 31)) {      // contrast last
        t[YUNET_PHOTO_CONTRAST] = 1.0f;
        t[YUNET_PHOTO_ALPHA] = photo_uniform(rand_u32(key, ctr++), cfg.contrast_lower, cfg.contrast_upper);
    }
    int p0 = 0, p1 = 1, p2 = 2;
    if (rand_u32(key, ctr++) >> 31) {                     // swap: permutation(3), legacy Fisher-Yates
        t[YUNET_PHOTO_SWAP] = 1.0f;
        const int j2 = bounded(rand_u32(key, ctr++), 3);  // i = 2
        if (j2 == 0) { const int x = p2; p2 = p0; p0 = x; }
        else if (j2 == 1) { const int x = p2; p2 = p1; p1 = x; }
        const int j1 = bounded(rand_u32(key, ctr++), 2);  // i = 1
        if (j1 == 0) { const int x = p1; p1 = p0; p0 = x; }
    }
    t[YUNET_PHOTO_PERM + 0] = (float)p0;
    t[YUNET_PHOTO_PERM + 1] = (float)p1;
    t[YUNET_PHOTO_PERM + 2] = (float)p2;
    t[YUNET_PHOTO_DRAWS] = (float)ctr;
    float* o = pp + (size_t)n * YUNET_PHOTO_WORDS;
#pragma unroll
    for (int k = 0; k < YUNET_PHOTO_WORDS; ++k) o[k] = t[k];
}

// The table of one image, read once per thread (uniform across the workgroup: scalar loads).
struct Photo {
    bool bright, contrast, sat, hue, swap;
    int mode, p0, p1, p2;
    float delta, alpha, sat_f, hue_d;
};
__device__ __forceinline__ Photo load_photo(const float* __restrict__ t) {
    Photo q;
    q.bright = t[YUNET_PHOTO_BRIGHT] != 0.0f; q.delta = t[YUNET_PHOTO_DELTA];
    q.mode = t[YUNET_PHOTO_MODE] != 0.0f ? 1 : 0;
    q.contrast = t[YUNET_PHOTO_CONTRAST] != 0.0f; q.alpha = t[YUNET_PHOTO_ALPHA];
    q.sat = t[YUNET_PHOTO_SAT] != 0.0f; q.sat_f = t[YUNET_PHOTO_SAT_F];
    q.hue = t[YUNET_PHOTO_HUE] != 0.0f; q.hue_d = t[YUNET_PHOTO_HUE_D];
    q.swap = t[YUNET_PHOTO_SWAP] != 0.0f;
    q.p0 = (int)t[YUNET_PHOTO_PERM + 0]; q.p1 = (int)t[YUNET_PHOTO_PERM + 1]; q.p2 = (int)t[YUNET_PHOTO_PERM + 2];
    return q;
}

// One BGR pixel through PhotoMetricDistortion.__call__, fp32 in the reference's order.  BGR <-> HSV is cv2.cvtColor's
// scalar float path (RGB2HSV_f / HSV2RGB_f, hrange 360) restated; the sector table of HSV -> BGR is written with
// selects so that nothing is indexed at run time (no scratch).
__device__ __forceinline__ void photo_pixel(const Photo& q, float& b, float& g, float& r) {
    if (q.bright) { b += q.delta; g += q.delta; r += q.delta; }
    if (q.mode == 1 && q.contrast) { b *= q.alpha; g *= q.alpha; r *= q.alpha; }
    // BGR -> HSV
    float v = r, vmin = r;
    if (v < g) v = g;
    if (v < b) v = b;
    if (vmin > g) vmin = g;
    if (vmin > b) vmin = b;
    float diff = v - vmin;
    float s = diff / (fabsf(v) + FLT_EPSILON);
    diff = (float)(60.0 / (double)(diff + FLT_EPSILON));
    float h;
    if (v == r) h = (g - b) * diff;
    else if (v == g) h = (b - r) * diff + 120.0f;
    else h = (r - g) * diff + 240.0f;
    if (h < 0.0f) h += 360.0f;
    // saturation, hue (strict comparisons, > 360 first)
    if (q.sat) s *= q.sat_f;
    if (q.hue) {
        h += q.hue_d;
        if (h > 360.0f) h -= 360.0f;
        if (h < 0.0f) h += 360.0f;
    }
    // HSV -> BGR
    if (s == 0.0f) {
        b = g = r = v;
    } else {
        h *= 6.0f / 360.0f;
        // cv2 wraps with unbounded loops; h is within [-6, 12] for any table yunet_aug_photometric writes
        // (hue_delta <= 360), so 64 trips never cut a wrap short there and a corrupt table cannot hang the kernel
        if (h < 0.0f) {
            for (int k = 0; k < 64 && h < 0.0f; ++k) h += 6.0f;
        } else if (h >= 6.0f) {
            for (int k = 0; k < 64 && h >= 6.0f; ++k) h -= 6.0f;
        }
        const float fl = floorf(h);
        int sector = (int)fl;
        h -= fl;
        if ((unsigned)sector >= 6u) { sector = 0; h = 0.0f; }
        const float t0 = v, t1 = v * (1.0f - s), t2 = v * (1.0f - s * h), t3 = v * (1.0f - s * (1.0f - h));
        // sector table {1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0} for (b, g, r)
        b = sector <= 1 ? t1 : sector == 2 ? t3 : sector == 5 ? t2 : t0;
        g = sector == 0 ? t3 : sector <= 2 ? t0 : sector == 3 ? t2 : t1;
        r = (sector == 0 || sector == 5) ? t0 : sector == 1 ? t2 : sector == 4 ? t3 : t1;
    }
    if (q.mode == 0 && q.contrast) { b *= q.alpha; g *= q.alpha; r *= q.alpha; }
    if (q.swap) {
        const float c[3] = {b, g, r};
        const float x0 = q.p0 == 0 ? c[0] : q.p0 == 1 ? c[1] : c[2];
        const float x1 = q.p1 == 0 ? c[0] : q.p1 == 1 ? c[1] : c[2];
        const float x2 = q.p2 == 0 ? c[0] : q.p2 == 1 ? c[1] : c[2];
        b = x0; g = x1; r = x2;
    }
}

// WIN = false: image n is src + src_off[n], row pitch w (the resident / whole-upload layout).
// WIN = true : image n is the rectangle rect[n] = (row0, col0, rows, cols) of the source, stored compactly at
//   src + src_off[n] with row pitch cols (yunet_aug_window_plan; the host-store upload).  The float operations are
//   those of WIN = false, so the output is bit-identical; the extra rectangle test only ever fails when the plan
//   does not belong to these params, and then it reads pad instead of leaving the window buffer.
// CANVAS = false: S is the output edge of every image.  CANVAS = true: S is the canvas edge (out_hw) and image n's
//   edge is params[n][AUG_P_SIZE]; canvas pixels at or beyond it are 0 -- also under PH = POST, which distorts the
//   image, not the collate padding -- and the pixels inside take the float operations of CANVAS = false at S = S_n.
// PH = YUNET_PHOTO_NONE: no distortion (yunet_aug_pixels / _window); PRE: each in-image tap pixel is distorted after
//   its load (pad taps stay pad); POST: the output pixel is distorted after the vertical pass.  `pp` = the table of
//   yunet_aug_photometric (unused for NONE).
// MOSAIC = false: the code as it stands.  MOSAIC = true (WIN = false, PH = NONE / POST): `src` is the whole store,
//   src_hw the out_hw of mosaic_decide_kernel and geom its table.  An image whose mosaic was made reads the four taps
//   of the crop's bilinear through mosaic_tap (the canvas is never materialised; `mpad` fills it outside the paste
//   rectangles, `pad` lies outside the canvas); a skipped image is image store_off[its index] through the plain code.
template <bool WIN, int PH, bool CANVAS = false, bool MOSAIC = false>
__global__ __launch_bounds__(256) void aug_pixels_kernel(
    const uint8_t* __restrict__ src, const long long* __restrict__ src_off, const int32_t* __restrict__ src_hw,
    const int32_t* __restrict__ rect, const int32_t* __restrict__ params, const float* __restrict__ pp, int C,
    float pad, float* __restrict__ out, const int32_t* __restrict__ geom, const long long* __restrict__ store_off,
    float mpad) {
    const int n = blockIdx.y;
    const int32_t* p = params + 8 * n;
    const int left = p[AUG_P_LEFT], top = p[AUG_P_TOP], cw = p[AUG_P_CW], flip = p[AUG_P_FLIP];
    const int h = src_hw[2 * n], w = src_hw[2 * n + 1];
    const int ry = WIN ? rect[4 * n + 0] : 0, rx = WIN ? rect[4 * n + 1] : 0;
    const int rh = WIN ? rect[4 * n + 2] : h, rw = WIN ? rect[4 * n + 3] : w;
    const int32_t* gm = MOSAIC ? geom + (size_t)n * YUNET_MOSAIC_WORDS : nullptr;
    const bool mosaic = MOSAIC && gm[YUNET_MOSAIC_APPLIED] != 0;
    const int mcx = MOSAIC ? gm[YUNET_MOSAIC_CX] : 0, mcy = MOSAIC ? gm[YUNET_MOSAIC_CY] : 0;
    const uint8_t* im = MOSAIC ? src + (mosaic ? 0 : store_off[gm[YUNET_MOSAIC_QUAD + YUNET_MOSAIC_Q_IDX]]) : src + src_off[n];
    const int S = CANVAS ? p[AUG_P_SIZE] : C;
    float* o = out + (size_t)n * 3 * C * C;
    Photo q;
    if (PH != YUNET_PHOTO_NONE) q = load_photo(pp + (size_t)n * YUNET_PHOTO_WORDS);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < C * C; i += gridDim.x * 256) {
        const int dy = i / C, dx = i - dy * C;
        if (CANVAS && (dy >= S || dx >= S)) {
            o[i] = 0.0f;
            o[(size_t)C * C + i] = 0.0f;
            o[(size_t)2 * C * C + i] = 0.0f;
            continue;
        }
        float v[3] = {pad, pad, pad};
        if (cw > 0) {
            const int dxs = flip ? S - 1 - dx : dx;
            int sx0, sx1, sy0, sy1;
            float a0, a1, b0, b1;
            lin_coef(dxs, S, cw, sx0, sx1, a0, a1);
            lin_coef(dy, S, cw, sy0, sy1, b0, b1);
            const int X0 = left + sx0, X1 = left + sx1, Y0 = top + sy0, Y1 = top + sy1;
            bool x0in = X0 >= 0 && X0 < w, x1in = X1 >= 0 && X1 < w;
            bool y0in = Y0 >= 0 && Y0 < h, y1in = Y1 >= 0 && Y1 < h;
            if (WIN) {
                x0in = x0in && X0 >= rx && X0 < rx + rw; x1in = x1in && X1 >= rx && X1 < rx + rw;
                y0in = y0in && Y0 >= ry && Y0 < ry + rh; y1in = y1in && Y1 >= ry && Y1 < ry + rh;
            }
            const uint8_t* r0 = im + ((size_t)(Y0 - ry) * rw) * 3 - (size_t)rx * 3;
            const uint8_t* r1 = im + ((size_t)(Y1 - ry) * rw) * 3 - (size_t)rx * 3;
            if (MOSAIC && mosaic) {
                float t00[3] = {pad, pad, pad}, t01[3] = {pad, pad, pad}, t10[3] = {pad, pad, pad},
                      t11[3] = {pad, pad, pad};
                if (y0in && x0in) mosaic_tap(gm, src, store_off, mcx, mcy, X0, Y0, mpad, t00);
                if (y0in && x1in) mosaic_tap(gm, src, store_off, mcx, mcy, X1, Y0, mpad, t01);
                if (y1in && x0in) mosaic_tap(gm, src, store_off, mcx, mcy, X0, Y1, mpad, t10);
                if (y1in && x1in) mosaic_tap(gm, src, store_off, mcx, mcy, X1, Y1, mpad, t11);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float t0 = t00[c] * a0 + t01[c] * a1;    // horizontal pass
                    const float t1 = t10[c] * a0 + t11[c] * a1;
                    v[c] = t0 * b0 + t1 * b1;                      // vertical pass
                }
            } else if (PH == YUNET_PHOTO_PRE) {
                float t00[3], t01[3], t10[3], t11[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    t00[c] = (y0in && x0in) ? (float)r0[3 * X0 + c] : pad;
                    t01[c] = (y0in && x1in) ? (float)r0[3 * X1 + c] : pad;
                    t10[c] = (y1in && x0in) ? (float)r1[3 * X0 + c] : pad;
                    t11[c] = (y1in && x1in) ? (float)r1[3 * X1 + c] : pad;
                }
                if (y0in && x0in) photo_pixel(q, t00[0], t00[1], t00[2]);
                if (y0in && x1in) photo_pixel(q, t01[0], t01[1], t01[2]);
                if (y1in && x0in) photo_pixel(q, t10[0], t10[1], t10[2]);
                if (y1in && x1in) photo_pixel(q, t11[0], t11[1], t11[2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float t0 = t00[c] * a0 + t01[c] * a1;    // horizontal pass
                    const float t1 = t10[c] * a0 + t11[c] * a1;
                    v[c] = t0 * b0 + t1 * b1;                      // vertical pass
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v00 = (y0in && x0in) ? (float)r0[3 * X0 + c] : pad;
                    const float v01 = (y0in && x1in) ? (float)r0[3 * X1 + c] : pad;
                    const float v10 = (y1in && x0in) ? (float)r1[3 * X0 + c] : pad;
                    const float v11 = (y1in && x1in) ? (float)r1[3 * X1 + c] : pad;
                    const float t0 = v00 * a0 + v01 * a1;          // horizontal pass
                    const float t1 = v10 * a0 + v11 * a1;
                    v[c] = t0 * b0 + t1 * b1;                      // vertical pass
                }
            }
        }
        if (PH == YUNET_PHOTO_POST) photo_pixel(q, v[0], v[1], v[2]);
        o[i] = v[0];
        o[(size_t)C * C + i] = v[1];
        o[(size_t)2 * C * C + i] = v[2];
    }
}

// ---- CutOut (transforms.py:2143-2214; include/yunet_hip.h YUNET_CUTOUT_*) ----------------------------------------------
__device__ __forceinline__ uint32_t cutout_key(uint32_t seed, uint32_t iteration, uint32_t image) {
    return mix32(stream_key(seed, iteration, image) ^ YUNET_CUTOUT_SALT);
}
// int(candidate) / int(ratio * edge) of a non-negative finite double; 2^30 stands for anything larger (x2 / y2 are
// clipped to the edge, at most YUNET_AUG_MAX_EDGE, so the result is the same and x1 + extent stays within int32)
__device__ __forceinline__ int cutout_extent(double v) {
    return (int)(v > 1073741824.0 ? 1073741824.0 : v);
}

// One workgroup per (image, hole slot) on the finished batch tensor [N, 3, E, E].  The draws are random-access in the
// counter: workgroup (n, j) reads draw 0 (the hole count) and the three draws of its own hole, writes its slot of the
// table (slot 0's workgroup the two header words too) and, when j < n_holes, stores fill[c] over
// img[n, c, y1:y2, x1:x2].  PARAMS: the image's edge is params[n][AUG_P_SIZE] (the multi-scale canvas), clamped to E;
// else E.  Holes of one image may overlap: they store the same values, so no order between workgroups is needed.
template <bool PARAMS>
__global__ __launch_bounds__(256) void aug_cutout_kernel(const YunetCutoutCfg cfg, uint32_t iteration, int E,
                                                         const int32_t* __restrict__ params, float* __restrict__ img,
                                                         int32_t* __restrict__ holes) {
    const int n = blockIdx.x / YUNET_CUTOUT_MAX_HOLES, j = blockIdx.x % YUNET_CUTOUT_MAX_HOLES;
    int S = PARAMS ? params[8 * n + AUG_P_SIZE] : E;
    if (S > E) S = E;
    const uint32_t key = cutout_key(cfg.seed, iteration, (uint32_t)n);
    // an image without an edge (S < 1: not a table of this pipeline) gets no hole; the count draw is made all the same
    const int drawn = cfg.n_lo + bounded(rand_u32(key, 0u), cfg.n_hi + 1 - cfg.n_lo);
    const int nh = S < 1 ? 0 : drawn;
    int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    if (j < nh) {
        x1 = bounded(rand_u32(key, 1u + 3u * j), S);
        y1 = bounded(rand_u32(key, 2u + 3u * j), S);
        const int idx = bounded(rand_u32(key, 3u + 3u * j), cfg.n_cand);
        const double cw_ = cfg.cand[idx][0], ch_ = cfg.cand[idx][1];
        const int cw = cutout_extent(cfg.with_ratio ? cw_ * (double)S : cw_);      // int(ratio_w * w), Python's double
        const int ch = cutout_extent(cfg.with_ratio ? ch_ * (double)S : ch_);
        x2 = x1 + cw < S ? x1 + cw : S;                                            // np.clip(x1 + cutout_w, 0, w)
        y2 = y1 + ch < S ? y1 + ch : S;
    }
    if (threadIdx.x == 0) {
        int32_t* t = holes + (size_t)n * YUNET_CUTOUT_WORDS;
        if (j == 0) { t[0] = nh; t[1] = 1 + 3 * nh; }
        int32_t* s = t + 2 + 4 * j;
        s[0] = x1; s[1] = y1; s[2] = x2; s[3] = y2;
    }
    const int hw = x2 - x1, hh = y2 - y1;
    if (hw <= 0 || hh <= 0) return;
    const size_t plane = (size_t)E * E;
    float* o = img + (size_t)n * 3 * plane + (size_t)y1 * E + x1;
    const float f0 = cfg.fill[0], f1 = cfg.fill[1], f2 = cfg.fill[2];
    for (int i = threadIdx.x; i < hw * hh; i += 256) {       // consecutive lanes: consecutive pixels of a row segment
        const int y = i / hw, x = i - y * hw;
        float* q = o + (size_t)y * E + x;
        q[0] = f0;
        q[plane] = f1;
        q[2 * plane] = f2;
    }
}

// ---- RandomAffine (transforms.py:2787-3001; include/yunet_hip.h YUNET_AFFINE_*) ----------------------------------------
__device__ __forceinline__ uint32_t affine_key(uint32_t seed, uint32_t iteration, uint32_t image) {
    return mix32(stream_key(seed, iteration, image) ^ YUNET_AFFINE_SALT);
}
// random.uniform(a, b) = a + (b - a) * random_sample(), Python's doubles
__device__ __forceinline__ double affine_uniform(uint32_t u, double a, double b) {
    return a + (b - a) * ((double)u * (1.0 / 4294967296.0));
}
// c = a @ b of two float32 3 x 3 matrices: every entry a0*b0 + a1*b1 + a2*b2, summed from the left
__device__ __forceinline__ void affine_matmul(const float* a, const float* b, float* c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
__device__ __forceinline__ float affine_clip(float v, float hi, bool clip) {
    return clip ? fminf(fmaxf(v, 0.0f), hi) : v;
}

// One 64-lane workgroup per image: the six draws, M and its inverse (every lane computes them, lane 0 stores the table
// row), then the rows of the image in steps of 64 -- each lane transforms one row, a ballot gives the surviving rows
// their places in order.  in_* and out_* are different buffers.  PARAMS as in aug_cutout_kernel.
template <bool PARAMS>
__global__ __launch_bounds__(64) void aug_affine_decide_kernel(
    const YunetAffineCfg cfg, uint32_t iteration, int E, const int32_t* __restrict__ params,
    const float* __restrict__ in_boxes, const float* __restrict__ in_kps, const int32_t* __restrict__ in_count,
    float* __restrict__ out_boxes, float* __restrict__ out_kps, int32_t* __restrict__ out_count,
    double* __restrict__ table) {
    const int n = blockIdx.x, lane = threadIdx.x;
    int S = PARAMS ? params[8 * n + AUG_P_SIZE] : E;
    S = S > E ? E : S < 0 ? 0 : S;
    const int gmax = cfg.gmax;
    const int G = in_count[n] < 0 ? 0 : in_count[n] > gmax ? gmax : in_count[n];
    const uint32_t key = affine_key(cfg.seed, iteration, (uint32_t)n);
    double d[6];
    d[0] = affine_uniform(rand_u32(key, 0u), -cfg.max_rotate_degree, cfg.max_rotate_degree);
    d[1] = affine_uniform(rand_u32(key, 1u), cfg.scale_lo, cfg.scale_hi);
    d[2] = affine_uniform(rand_u32(key, 2u), -cfg.max_shear_degree, cfg.max_shear_degree);
    d[3] = affine_uniform(rand_u32(key, 3u), -cfg.max_shear_degree, cfg.max_shear_degree);
    d[4] = affine_uniform(rand_u32(key, 4u), -cfg.max_translate_ratio, cfg.max_translate_ratio);
    d[5] = affine_uniform(rand_u32(key, 5u), -cfg.max_translate_ratio, cfg.max_translate_ratio);
    const double to_rad = 3.14159265358979323846 / 180.0;                 // math.radians: x * (pi / 180)
    const double rad = d[0] * to_rad;
    const float co = (float)cos(rad), si = (float)sin(rad), sc = (float)d[1];
    const float R[9] = {co, -si, 0.0f, si, co, 0.0f, 0.0f, 0.0f, 1.0f};
    const float Sc[9] = {sc, 0.0f, 0.0f, 0.0f, sc, 0.0f, 0.0f, 0.0f, 1.0f};
    const float Sh[9] = {1.0f, (float)tan(d[2] * to_rad), 0.0f, (float)tan(d[3] * to_rad), 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    const float T[9] = {1.0f, 0.0f, (float)(d[4] * (double)S), 0.0f, 1.0f, (float)(d[5] * (double)S), 0.0f, 0.0f, 1.0f};
    float A[9], B[9], M[9];
    affine_matmul(T, Sh, A);
    affine_matmul(A, R, B);
    affine_matmul(B, Sc, M);

    const float fS = (float)S;
    const bool clip = cfg.bbox_clip_border != 0, filter = cfg.skip_filter == 0;
    const float* bx = in_boxes + (size_t)n * gmax * 4;
    const float* kp = in_kps + (size_t)n * gmax * 15;
    float* ob = out_boxes + (size_t)n * gmax * 4;
    float* ok = out_kps + (size_t)n * gmax * 15;
    int kept = 0;
    for (int base = 0; base < G; base += 64) {
        const int g = base + lane;
        bool keep = false;
        float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, w3 = 0.0f;
        if (g < G) {
            const float* b = bx + 4 * g;
            const float px[4] = {b[0], b[0], b[2], b[2]}, py[4] = {b[1], b[3], b[3], b[1]};
            float xs[4], ys[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                xs[c] = (M[0] * px[c] + M[1] * py[c]) + M[2];
                ys[c] = (M[3] * px[c] + M[4] * py[c]) + M[5];
            }
            w0 = affine_clip(fminf(fminf(xs[0], xs[1]), fminf(xs[2], xs[3])), fS, clip);
            w1 = affine_clip(fminf(fminf(ys[0], ys[1]), fminf(ys[2], ys[3])), fS, clip);
            w2 = affine_clip(fmaxf(fmaxf(xs[0], xs[1]), fmaxf(xs[2], xs[3])), fS, clip);
            w3 = affine_clip(fmaxf(fmaxf(ys[0], ys[1]), fmaxf(ys[2], ys[3])), fS, clip);
            keep = w0 < fS && w2 > 0.0f && w1 < fS && w3 > 0.0f;                           // find_inside_bboxes
            if (filter) {                                                                  // filter_gt_bboxes
                const float ow = b[2] * sc - b[0] * sc, oh = b[3] * sc - b[1] * sc;        // bboxes * scaling_ratio
                const float ww = w2 - w0, wh = w3 - w1;
                const float aspect = fmaxf(ww / (wh + 1e-16f), wh / (ww + 1e-16f));
                keep = keep && ww > cfg.min_bbox_size && wh > cfg.min_bbox_size &&
                       ww * wh / (ow * oh + 1e-16f) > cfg.min_area_ratio && aspect < cfg.max_aspect_ratio;
            }
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int idx = kept + __popcll(m & ((1ull << lane) - 1ull));       // idx <= g < gmax
            float* o = ob + 4 * idx;
            o[0] = w0; o[1] = w1; o[2] = w2; o[3] = w3;
            const float* k = kp + 15 * g;
            float* q = ok + 15 * idx;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float x = k[3 * j], y = k[3 * j + 1];
                q[3 * j + 0] = affine_clip((M[0] * x + M[1] * y) + M[2], fS, clip);
                q[3 * j + 1] = affine_clip((M[3] * x + M[4] * y) + M[5], fS, clip);
                q[3 * j + 2] = k[3 * j + 2];
            }
        }
        kept += __popcll(m);
    }
    for (int i = kept * 4 + lane; i < gmax * 4; i += 64) ob[i] = 0.0f;
    for (int i = kept * 15 + lane; i < gmax * 15; i += 64) ok[i] = 0.0f;
    if (lane == 0) {
        const double a = M[0], b = M[1], c = M[2], e = M[3], f = M[4], h = M[5];
        const double det = a * f - b * e;
        double* t = table + (size_t)n * YUNET_AFFINE_WORDS;
#pragma unroll
        for (int i = 0; i < 6; ++i) t[YUNET_AFFINE_DRAWS + i] = d[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) t[YUNET_AFFINE_M + i] = (double)M[i];
        double* v = t + YUNET_AFFINE_INV;
        v[0] = f / det; v[1] = -b / det; v[2] = (b * h - c * f) / det;
        v[3] = -e / det; v[4] = a / det; v[5] = (c * e - a * h) / det;
        t[YUNET_AFFINE_ROWS_IN] = (double)G; t[YUNET_AFFINE_ROWS_OUT] = (double)kept; t[YUNET_AFFINE_EDGE] = (double)S;
        out_count[n] = kept;
    }
}

// One thread per pixel of the E x E plane, one row of workgroups per image (blockIdx.x = n * blocks_per_image + block):
// consecutive lanes store consecutive pixels of each of the three planes; coordinates, taps and weights are worked out
// once per pixel and shared by the channels.  PARAMS as in aug_cutout_kernel; pixels at or beyond S_n are 0.
template <bool PARAMS>
__global__ __launch_bounds__(256) void aug_affine_pixels_kernel(
    const double* __restrict__ table, float bv0, float bv1, float bv2, int E, int blocks_per_image,
    const int32_t* __restrict__ params, const float* __restrict__ in, float* __restrict__ out) {
    const int n = blockIdx.x / blocks_per_image;
    const int i = (blockIdx.x - n * blocks_per_image) * 256 + threadIdx.x;
    if (i >= E * E) return;
    int S = PARAMS ? params[8 * n + AUG_P_SIZE] : E;
    S = S > E ? E : S;
    const int y = i / E, x = i - y * E;
    const size_t plane = (size_t)E * E;
    const float* src = in + (size_t)n * 3 * plane;
    float* dst = out + (size_t)n * 3 * plane + i;
    if (x >= S || y >= S) {
        dst[0] = 0.0f; dst[plane] = 0.0f; dst[2 * plane] = 0.0f;
        return;
    }
    const double* t = table + (size_t)n * YUNET_AFFINE_WORDS + YUNET_AFFINE_INV;
    const float fx_ = (float)x, fy_ = (float)y;
    const float sx = ((float)t[0] * fx_ + (float)t[1] * fy_) + (float)t[2];
    const float sy = ((float)t[3] * fx_ + (float)t[4] * fy_) + (float)t[5];
    float v0 = bv0, v1 = bv1, v2 = bv2;
    // all four taps outside (or a coordinate that is not a number): border_val; the test also keeps x0 / y0 within int
    if (sx > -1.0f && sx < (float)S && sy > -1.0f && sy < (float)S) {
        const float flx = floorf(sx), fly = floorf(sy);
        const int x0 = (int)flx, y0 = (int)fly;                 // in [-1, S - 1]
        const float ax = sx - flx, ay = sy - fly;
        const float w00 = (1.0f - ax) * (1.0f - ay), w01 = ax * (1.0f - ay), w10 = (1.0f - ax) * ay, w11 = ax * ay;
        const bool inx0 = x0 >= 0, inx1 = x0 + 1 < S, iny0 = y0 >= 0, iny1 = y0 + 1 < S;
        const float* p = src + (ptrdiff_t)y0 * E + x0;          // dereferenced only at taps inside [0, S) x [0, S)
        const float bv[3] = {bv0, bv1, bv2};
        float r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pc = p + c * plane;
            const float t00 = iny0 && inx0 ? pc[0] : bv[c], t01 = iny0 && inx1 ? pc[1] : bv[c];
            const float t10 = iny1 && inx0 ? pc[E] : bv[c], t11 = iny1 && inx1 ? pc[E + 1] : bv[c];
            // a coordinate on the pixel grid copies its pixel (the sum would turn a -0.0 into +0.0)
            r[c] = ax == 0.0f && ay == 0.0f ? t00 : ((w00 * t00 + w01 * t01) + w10 * t10) + w11 * t11;
        }
        v0 = r[0]; v1 = r[1]; v2 = r[2];
    }
    dst[0] = v0; dst[plane] = v1; dst[2 * plane] = v2;
}

// ---- MixUp (transforms.py:2523-2783; include/yunet_hip.h YUNET_MIXUP_*) ------------------------------------------------
__device__ __forceinline__ uint32_t mixup_key(uint32_t seed, uint32_t iteration, uint32_t image) {
    return mix32(stream_key(seed, iteration, image) ^ YUNET_MIXUP_SALT);
}

// One 64-lane workgroup per image: the draws and the geometry (wave-uniform integers / doubles, every lane computes
// them, lane 0 stores the table row), then the image's own rows and the partner's rows in steps of 64 -- a ballot gives
// the surviving rows their places in order, as in aug_affine_decide_kernel.  in_* and out_* are different buffers.
// PARAMS as in aug_cutout_kernel.
template <bool PARAMS>
__global__ __launch_bounds__(64) void aug_mixup_decide_kernel(
    const YunetMixupCfg cfg, uint32_t iteration, int E, const int32_t* __restrict__ params, int M,
    const int32_t* __restrict__ store_hw, const int32_t* __restrict__ store_goff, const int32_t* __restrict__ store_gcnt,
    const float* __restrict__ store_boxes, const float* __restrict__ store_kps, const float* __restrict__ in_boxes,
    const float* __restrict__ in_kps, const int32_t* __restrict__ in_count, float* __restrict__ out_boxes,
    float* __restrict__ out_kps, int32_t* __restrict__ out_count, double* __restrict__ table) {
    const int n = blockIdx.x, lane = threadIdx.x;
    int T = PARAMS ? params[8 * n + AUG_P_SIZE] : E;
    T = T > E ? E : T < 0 ? 0 : T;
    const int gmax = cfg.gmax, D = cfg.img_scale;
    const int G = in_count[n] < 0 ? 0 : in_count[n] > gmax ? gmax : in_count[n];
    const uint32_t key = mixup_key(cfg.seed, iteration, (uint32_t)n);
    uint32_t ctr = 0;
    int partner = 0, pg = 0;
    for (int i = 0; i < cfg.max_iters; ++i) {                               // get_indexes
        partner = bounded(rand_u32(key, ctr++), M);
        pg = store_gcnt[partner];
        if (pg != 0) break;
    }
    const int index_draws = (int)ctr;
    bool applied = pg > 0;
    int status = 0, J = 0, rw = 0, rh = 0, xoff = 0, yoff = 0;
    double jit = 0.0, sr = 0.0, sx = 0.0, sy = 0.0;
    bool flip = false;
    const int h = store_hw[2 * partner], w = store_hw[2 * partner + 1];
    if (applied) {
        jit = cfg.ratio_lo + (cfg.ratio_hi - cfg.ratio_lo) * ((double)rand_u32(key, ctr++) * (1.0 / 4294967296.0));
        flip = (double)rand_u32(key, ctr++) * (1.0 / 4294967296.0) > cfg.flip_ratio;
        if (h > 0 && w > 0) {
            const double rh_ = (double)D / (double)h, rw_ = (double)D / (double)w;
            sr = rh_ < rw_ ? rh_ : rw_;
            rw = (int)((double)w * sr);
            rh = (int)((double)h * sr);
        }
        const double dj = (double)D * jit;
        J = dj < 1073741824.0 ? (int)dj : 1073741824;
        if (rw < 1 || rh < 1 || J < 1) {
            applied = false; status |= 4;
        } else {
            sr *= jit;
            sx = 1.0 / ((double)rw / (double)w);
            sy = 1.0 / ((double)rh / (double)h);
            if (J > T) {
                yoff = bounded(rand_u32(key, ctr++), J - T);
                xoff = bounded(rand_u32(key, ctr++), J - T);
            }
        }
    }
    const float fT = (float)T, fJ = (float)J, fsr = (float)sr, fxo = (float)xoff, fyo = (float)yoff;
    const bool clip = cfg.bbox_clip_border != 0, filter = cfg.skip_filter == 0;
    const float* bx = in_boxes + (size_t)n * gmax * 4;
    const float* kp = in_kps + (size_t)n * gmax * 15;
    float* ob = out_boxes + (size_t)n * gmax * 4;
    float* ok = out_kps + (size_t)n * gmax * 15;
    int kept = 0;
    for (int base = 0; base < G; base += 64) {          // the image's own rows
        const int g = base + lane;
        bool keep = g < G;
        float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (keep) {
#pragma unroll
            for (int e = 0; e < 4; ++e) b[e] = bx[4 * g + e];
            if (applied) keep = b[0] < fT && b[2] > 0.0f && b[1] < fT && b[3] > 0.0f;      // find_inside_bboxes
        }
        const unsigned long long m = __ballot(keep);
        const int at = kept + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && at < gmax) {
            float* o = ob + 4 * at;
            o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
            const float* k = kp + 15 * g;
            float* q = ok + 15 * at;
#pragma unroll
            for (int j = 0; j < 15; ++j) q[j] = k[j];
        }
        kept += __popcll(m);
    }
    if (applied) {                                      // the partner's rows
        const float* pb = store_boxes + (size_t)store_goff[partner] * 4;
        const float* pk = store_kps + (size_t)store_goff[partner] * 15;
        for (int base = 0; base < pg; base += 64) {
            const int g = base + lane;
            bool keep = g < pg;
            float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (keep) {
                float b[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) b[e] = affine_clip(pb[4 * g + e] * fsr, fJ, clip);
                if (flip) { const float t = b[0]; b[0] = fJ - b[2]; b[2] = fJ - t; }
                c[0] = affine_clip(b[0] - fxo, fT, clip); c[2] = affine_clip(b[2] - fxo, fT, clip);
                c[1] = affine_clip(b[1] - fyo, fT, clip); c[3] = affine_clip(b[3] - fyo, fT, clip);
                if (filter) {                                                              // _filter_box_candidates
                    const float w1 = b[2] - b[0], h1 = b[3] - b[1], w2 = c[2] - c[0], h2 = c[3] - c[1];
                    const float ar = fmaxf(w2 / (h2 + 1e-16f), h2 / (w2 + 1e-16f));
                    keep = w2 > cfg.min_bbox_size && h2 > cfg.min_bbox_size &&
                           w2 * h2 / (w1 * h1 + 1e-16f) > cfg.min_area_ratio && ar < cfg.max_aspect_ratio;
                }
                keep = keep && c[0] < fT && c[2] > 0.0f && c[1] < fT && c[3] > 0.0f;       // find_inside_bboxes
            }
            const unsigned long long m = __ballot(keep);
            const int at = kept + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && at < gmax) {
                float* o = ob + 4 * at;
                o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
                const float* k = pk + 15 * g;
                float* q = ok + 15 * at;
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const int js = flip ? (j == 0 ? 1 : j == 1 ? 0 : j == 3 ? 4 : j == 4 ? 3 : 2) : j;
                    float x = affine_clip(k[3 * js] * fsr, fJ, clip), y = affine_clip(k[3 * js + 1] * fsr, fJ, clip);
                    if (flip) x = fJ - x;
                    q[3 * j] = affine_clip(x - fxo, fT, clip);
                    q[3 * j + 1] = affine_clip(y - fyo, fT, clip);
                    q[3 * j + 2] = k[3 * js + 2];
                }
            }
            kept += __popcll(m);
        }
    }
    const int count = kept < gmax ? kept : gmax;
    for (int i = count * 4 + lane; i < gmax * 4; i += 64) ob[i] = 0.0f;
    for (int i = count * 15 + lane; i < gmax * 15; i += 64) ok[i] = 0.0f;
    if (lane == 0) {
        double* t = table + (size_t)n * YUNET_MIXUP_WORDS;
        t[YUNET_MIXUP_PARTNER] = (double)partner; t[YUNET_MIXUP_APPLIED] = applied ? 1.0 : 0.0;
        t[YUNET_MIXUP_INDEX_DRAWS] = (double)index_draws; t[YUNET_MIXUP_JIT] = jit; t[YUNET_MIXUP_FLIP] = flip ? 1.0 : 0.0;
        t[YUNET_MIXUP_J] = (double)J; t[YUNET_MIXUP_RW] = (double)rw; t[YUNET_MIXUP_RH] = (double)rh;
        t[YUNET_MIXUP_XOFF] = (double)xoff; t[YUNET_MIXUP_YOFF] = (double)yoff;
        t[YUNET_MIXUP_SX] = sx; t[YUNET_MIXUP_SY] = sy;
        t[YUNET_MIXUP_ROWS_IN] = (double)G; t[YUNET_MIXUP_ROWS_OUT] = (double)kept;
        t[YUNET_MIXUP_STATUS] = (double)(status | (kept > gmax ? 2 : 0)); t[YUNET_MIXUP_EDGE] = (double)T;
        t[YUNET_MIXUP_DRAWS] = (double)ctr; t[YUNET_MIXUP_SR] = sr;
        out_count[n] = count;
    }
}

// One canvas tap (u, v) of the D x D pad_val canvas that holds the resized partner in its top-left rw x rh corner: the
// float bilinear value of the raw image, horizontal pass then vertical pass as mosaic_tap has it.  lin_coef_s clamps
// both taps to the source, so nothing outside the partner image is read.
__device__ __forceinline__ void mixup_tap(const uint8_t* __restrict__ im, int w, int h, int rw, int rh, double sx,
                                          double sy, int u, int v, float pad, float* __restrict__ o) {
    if (u >= rw || v >= rh) {
        o[0] = pad; o[1] = pad; o[2] = pad;
        return;
    }
    int x0, x1, y0, y1;
    float a0, a1, b0, b1;
    lin_coef_s(u, sx, w, x0, x1, a0, a1);
    lin_coef_s(v, sy, h, y0, y1, b0, b1);
    const uint8_t* r0 = im + (size_t)y0 * w * 3;
    const uint8_t* r1 = im + (size_t)y1 * w * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t0 = (float)r0[3 * x0 + c] * a0 + (float)r0[3 * x1 + c] * a1;
        const float t1 = (float)r1[3 * x0 + c] * a0 + (float)r1[3 * x1 + c] * a1;
        o[c] = t0 * b0 + t1 * b1;
    }
}

// One thread per pixel of the E x E plane, the workgroups of an image in a row (blockIdx.x = n * blocks_per_image +
// block): consecutive lanes take consecutive pixels of each plane; coordinates, taps and weights are worked out once
// per pixel and shared by the channels.  In place: a thread reads and writes its own pixel only.  PARAMS as in
// aug_cutout_kernel; pixels at or beyond S_n and images that are not applied are not touched.
template <bool PARAMS>
__global__ __launch_bounds__(256) void aug_mixup_pixels_kernel(
    const double* __restrict__ table, int D, float pad, int E, int blocks_per_image, const int32_t* __restrict__ params,
    int M, const uint8_t* __restrict__ store, const long long* __restrict__ store_off,
    const int32_t* __restrict__ store_hw, float* __restrict__ img) {
    const int n = blockIdx.x / blocks_per_image;
    const int i = (blockIdx.x - n * blocks_per_image) * 256 + threadIdx.x;
    const double* t = table + (size_t)n * YUNET_MIXUP_WORDS;
    if (i >= E * E || t[YUNET_MIXUP_APPLIED] == 0.0) return;
    int T = PARAMS ? params[8 * n + AUG_P_SIZE] : E;
    T = T > E ? E : T;
    const int y = i / E, x = i - y * E;
    if (x >= T || y >= T) return;
    const int partner = (int)t[YUNET_MIXUP_PARTNER], J = (int)t[YUNET_MIXUP_J], rw = (int)t[YUNET_MIXUP_RW],
              rh = (int)t[YUNET_MIXUP_RH], xoff = (int)t[YUNET_MIXUP_XOFF], yoff = (int)t[YUNET_MIXUP_YOFF];
    if (partner < 0 || partner >= M || J < 1 || rw < 1 || rh < 1 || xoff < 0 || yoff < 0) return;
    const int h = store_hw[2 * partner], w = store_hw[2 * partner + 1];
    if (h < 1 || w < 1) return;
    const size_t plane = (size_t)E * E;
    float* p = img + (size_t)n * 3 * plane + i;
    float b[3] = {0.0f, 0.0f, 0.0f};
    const int X = x + xoff, Y = y + yoff;
    if (X < J && Y < J) {
        const int Xf = t[YUNET_MIXUP_FLIP] != 0.0 ? J - 1 - X : X;
        const double cs = 1.0 / ((double)J / (double)D);
        const double sx = t[YUNET_MIXUP_SX], sy = t[YUNET_MIXUP_SY];
        int u0, u1, v0, v1;
        float A0, A1, B0, B1;
        lin_coef_s(Xf, cs, D, u0, u1, A0, A1);
        lin_coef_s(Y, cs, D, v0, v1, B0, B1);
        const uint8_t* im = store + store_off[partner];
        float c00[3], c01[3], c10[3], c11[3];
        mixup_tap(im, w, h, rw, rh, sx, sy, u0, v0, pad, c00);
        mixup_tap(im, w, h, rw, rh, sx, sy, u1, v0, pad, c01);
        mixup_tap(im, w, h, rw, rh, sx, sy, u0, v1, pad, c10);
        mixup_tap(im, w, h, rw, rh, sx, sy, u1, v1, pad, c11);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t0 = c00[c] * A0 + c01[c] * A1;         // horizontal pass
            const float t1 = c10[c] * A0 + c11[c] * A1;
            b[c] = truncf(t0 * B0 + t1 * B1);                   // vertical pass; padded_img is uint8
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = 0.5f * p[c * plane] + 0.5f * b[c];
        p[c * plane] = truncf(fminf(fmaxf(v, 0.0f), 255.0f));
    }
}

}  // namespace

static bool mixup_cfg_ok(const YunetMixupCfg* c) {
    if (!c) return false;
    const double v[3] = {c->ratio_lo, c->ratio_hi, c->flip_ratio};
    for (double x : v)
        if (!std::isfinite(x)) return false;
    const float f[4] = {c->pad_val, c->min_bbox_size, c->min_area_ratio, c->max_aspect_ratio};
    for (float x : f)
        if (!std::isfinite(x)) return false;
    return c->ratio_lo > 0.0 && c->ratio_lo <= c->ratio_hi && c->img_scale >= 1 &&
           c->img_scale <= YUNET_AUG_MAX_EDGE / 2 && (double)c->img_scale * c->ratio_hi < 1073741824.0 &&
           c->max_iters >= 1 && c->gmax >= 1 && c->gmax <= 4096;
}

static bool affine_cfg_ok(const YunetAffineCfg* c) {
    if (!c) return false;
    const double v[5] = {c->max_rotate_degree, c->max_translate_ratio, c->scale_lo, c->scale_hi, c->max_shear_degree};
    for (double x : v)
        if (!std::isfinite(x)) return false;
    const float f[6] = {c->min_bbox_size, c->min_area_ratio, c->max_aspect_ratio, c->border_val[0], c->border_val[1],
                        c->border_val[2]};
    for (float x : f)
        if (!std::isfinite(x)) return false;
    return c->max_translate_ratio >= 0.0 && c->max_translate_ratio <= 1.0 && c->scale_lo > 0.0 &&
           c->scale_lo <= c->scale_hi && std::fabs(c->max_shear_degree) < YUNET_AFFINE_MAX_SHEAR && c->gmax >= 1 &&
           c->gmax <= 4096;
}

static bool cutout_cfg_ok(const YunetCutoutCfg* c) {
    if (!c || c->n_lo < 0 || c->n_lo > c->n_hi || c->n_hi > YUNET_CUTOUT_MAX_HOLES || c->n_cand < 1 ||
        c->n_cand > YUNET_CUTOUT_MAX_CANDIDATES)
        return false;
    for (int i = 0; i < c->n_cand; ++i)
        for (int k = 0; k < 2; ++k)
            if (!std::isfinite(c->cand[i][k]) || c->cand[i][k] < 0.0) return false;
    return std::isfinite(c->fill[0]) && std::isfinite(c->fill[1]) && std::isfinite(c->fill[2]);
}

static bool aug_cfg_ok(const YunetAugCfg* cfg) {
    return cfg && cfg->n_choice >= 1 && cfg->n_choice <= 8 && cfg->gmax >= 1 && cfg->max_attempts >= 1 &&
           cfg->max_retries >= 1;
}

static bool photo_cfg_ok(const YunetPhotoCfg* c) {
    const double v[6] = {c->brightness_delta, c->contrast_lower, c->contrast_upper, c->saturation_lower,
                         c->saturation_upper, c->hue_delta};
    for (double x : v)
        if (!std::isfinite(x)) return false;
    return c->brightness_delta >= 0.0 && c->hue_delta >= 0.0 && c->hue_delta <= 360.0 &&
           c->contrast_lower <= c->contrast_upper && c->saturation_lower <= c->saturation_upper &&
           (c->position == YUNET_PHOTO_PRE || c->position == YUNET_PHOTO_POST);
}

static bool mosaic_cfg_ok(const YunetMosaicCfg* c) {
    return c && c->img_scale >= 1 && c->img_scale <= YUNET_AUG_MAX_EDGE / 2 && c->gmax >= 1 &&
           std::isfinite(c->center_lo) && std::isfinite(c->center_hi) && c->center_lo >= 0.0 &&
           c->center_lo <= c->center_hi && c->center_hi <= 2.0 && c->prob >= 0.0 && c->prob <= 1.0 &&
           std::isfinite(c->min_bbox_size) && std::isfinite(c->pad_val);
}

// A run-time choice as a template argument: f(std::bool_constant<b>{}), f(std::integral_constant<int, position>{}).
template <class F>
static void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <class F>
static void with_position(int position, F&& f) {
    if (position == YUNET_PHOTO_PRE) f(std::integral_constant<int, YUNET_PHOTO_PRE>{});
    else if (position == YUNET_PHOTO_POST) f(std::integral_constant<int, YUNET_PHOTO_POST>{});
    else f(std::integral_constant<int, YUNET_PHOTO_NONE>{});
}

extern "C" int yunet_aug_decide(const int32_t* src_hw, const float* boxes, const float* kps, const int32_t* gt_idx,
                                int in_gmax, const YunetAugCfg* cfg, int multiscale, int scale_lo, int scale_hi,
                                uint32_t iteration, int N, int32_t* params, float* out_boxes, float* out_kps,
                                int32_t* out_count, void* stream) {
    if (!aug_cfg_ok(cfg) || N < 1 || in_gmax < 0) return YUNET_EINVAL;
    if (multiscale ? (scale_lo < 32 || scale_hi < scale_lo || scale_hi > YUNET_AUG_MAX_EDGE) : cfg->out_size < 1)
        return YUNET_EINVAL;
    if (!multiscale) scale_lo = scale_hi = 0;
    with_bool(multiscale != 0, [&](auto ms) {
        with_bool(in_gmax > 0, [&](auto pad) {
            hipLaunchKernelGGL((aug_decide_kernel<decltype(ms)::value, decltype(pad)::value>), dim3(N), dim3(64), 0,
                               (hipStream_t)stream, src_hw, boxes, kps, gt_idx, *cfg, scale_lo, scale_hi, iteration,
                               params, out_boxes, out_kps, out_count, in_gmax);
        });
    });
    return hip_status();
}

extern "C" int yunet_aug_ignore(const int32_t* params, const float* ign_boxes, const int32_t* ign_off, int out_size, int N,
                                int imax, float* out_ign, int32_t* out_icount, void* stream) {
    // ign_boxes may be NULL when the batch holds no ignore box at all (ign_off all equal): nothing is read through it
    if (!params || !ign_off || !out_ign || !out_icount || N < 1 || imax < 1 || out_size < 1 || out_size > YUNET_AUG_MAX_EDGE)
        return YUNET_EINVAL;
    hipLaunchKernelGGL(aug_ignore_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, params, ign_boxes, ign_off, out_size,
                       imax, out_ign, out_icount);
    return hip_status();
}

extern "C" int yunet_aug_photometric(const YunetPhotoCfg* cfg, uint32_t seed, uint32_t iteration, int N,
                                     float* pparams, void* stream) {
    if (!cfg || !photo_cfg_ok(cfg) || N < 1 || !pparams) return YUNET_EINVAL;
    hipLaunchKernelGGL(aug_photometric_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, *cfg, seed,
                       iteration, N, pparams);
    return hip_status();
}

// Every refusal of the pixel pass, before any launch.  The two forms that are not built -- mosaic over a window buffer,
// mosaic with the distortion in the PRE position -- are refused here, so the dispatch below never meets them.
static bool aug_pixels_ok(const YunetAugPixels* a, const YunetAugCfg* cfg, int N, const float* out_img) {
    if (!a || !cfg || N < 1 || !out_img || !a->src || !a->src_off || !a->src_hw || !a->params) return false;
    const bool photo = a->position == YUNET_PHOTO_PRE || a->position == YUNET_PHOTO_POST;
    if ((!photo && a->position != YUNET_PHOTO_NONE) || (photo && !a->pparams)) return false;
    if (a->out_hw < 0 || a->out_hw > YUNET_AUG_MAX_EDGE || (a->out_hw == 0 && cfg->out_size < 1)) return false;
    if ((a->geom != nullptr) != (a->mosaic != nullptr)) return false;
    if (a->geom && (!mosaic_cfg_ok(a->mosaic) || a->rect || a->position == YUNET_PHOTO_PRE)) return false;
    return true;
}

extern "C" int yunet_aug_pixels(const YunetAugPixels* a, const YunetAugCfg* cfg, int N, float* out_img, void* stream) {
    if (!aug_pixels_ok(a, cfg, N, out_img)) return YUNET_EINVAL;
    const int C = a->out_hw ? a->out_hw : cfg->out_size;      // the grid covers the canvas, border included
    int bx = (C * C + 255) / 256;
    if (bx > 64) bx = 64;                                     // grid-stride over the pixels of one image
    with_bool(a->rect != nullptr, [&](auto win) {
        with_position(a->position, [&](auto ph) {
            with_bool(a->out_hw > 0, [&](auto canvas) {
                with_bool(a->geom != nullptr, [&](auto mosaic) {
                    constexpr bool WIN = decltype(win)::value, CANVAS = decltype(canvas)::value,
                                   MOSAIC = decltype(mosaic)::value;
                    constexpr int PH = decltype(ph)::value;
                    // the kernel's mosaic form takes the store's offset table apart from src_off
                    if constexpr (!(MOSAIC && (WIN || PH == YUNET_PHOTO_PRE)))
                        hipLaunchKernelGGL((aug_pixels_kernel<WIN, PH, CANVAS, MOSAIC>), dim3(bx, N), dim3(256), 0,
                                           (hipStream_t)stream, a->src, MOSAIC ? nullptr : a->src_off, a->src_hw,
                                           a->rect, a->params, a->pparams, C, cfg->pad_value, out_img, a->geom,
                                           MOSAIC ? a->src_off : nullptr, MOSAIC ? a->mosaic->pad_val : 0.0f);
                });
            });
        });
    });
    return hip_status();
}

extern "C" int yunet_aug_mosaic_decide(const int32_t* idx, int N, int M, const int32_t* store_hw,
                                       const int32_t* store_goff, const int32_t* store_gcnt, const float* store_boxes,
                                       const float* store_kps, const YunetMosaicCfg* cfg, uint32_t iteration,
                                       int32_t* geom, int32_t* out_hw, float* out_boxes, float* out_kps,
                                       int32_t* out_count, void* stream) {
    if (!mosaic_cfg_ok(cfg) || N < 1 || M < 1 || !idx || !store_hw || !store_goff || !store_gcnt || !store_boxes ||
        !store_kps || !geom || !out_hw || !out_boxes || !out_kps || !out_count)
        return YUNET_EINVAL;
    hipLaunchKernelGGL(mosaic_decide_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, idx, M, store_hw, store_goff,
                       store_gcnt, store_boxes, store_kps, *cfg, iteration, geom, out_hw, out_boxes, out_kps,
                       out_count);
    return hip_status();
}

extern "C" int yunet_aug_mosaic_canvas(const uint8_t* store, const long long* store_off, const int32_t* geom,
                                       const YunetMosaicCfg* mcfg, int N, float* canvas, void* stream) {
    if (!mosaic_cfg_ok(mcfg) || N < 1 || !store || !store_off || !geom || !canvas) return YUNET_EINVAL;
    const int E = 2 * mcfg->img_scale;
    int bx = (E * E + 255) / 256;
    if (bx > 256) bx = 256;
    hipLaunchKernelGGL(mosaic_canvas_kernel, dim3(bx, N), dim3(256), 0, (hipStream_t)stream, store, store_off, geom,
                       mcfg->img_scale, mcfg->pad_val, canvas);
    return hip_status();
}

extern "C" int yunet_aug_cutout(const YunetCutoutCfg* cfg, uint32_t iteration, int N, int E, const int32_t* params,
                                float* img, int32_t* holes, void* stream) {
    if (!cutout_cfg_ok(cfg) || N < 1 || N > INT32_MAX / YUNET_CUTOUT_MAX_HOLES || E < 1 || E > YUNET_AUG_MAX_EDGE ||
        !img || !holes)
        return YUNET_EINVAL;
    with_bool(params != nullptr, [&](auto ms) {
        hipLaunchKernelGGL((aug_cutout_kernel<decltype(ms)::value>), dim3(N * YUNET_CUTOUT_MAX_HOLES), dim3(256), 0,
                           (hipStream_t)stream, *cfg, iteration, E, params, img, holes);
    });
    return hip_status();
}

extern "C" int yunet_aug_affine_decide(const YunetAffineCfg* cfg, uint32_t iteration, int N, int E, const int32_t* params,
                                       const float* in_boxes, const float* in_kps, const int32_t* in_count,
                                       float* out_boxes, float* out_kps, int32_t* out_count, double* table,
                                       void* stream) {
    if (!affine_cfg_ok(cfg) || N < 1 || E < 1 || E > YUNET_AUG_MAX_EDGE || !in_boxes || !in_kps || !in_count ||
        !out_boxes || !out_kps || !out_count || !table || in_boxes == out_boxes || in_kps == out_kps ||
        in_count == out_count)
        return YUNET_EINVAL;
    with_bool(params != nullptr, [&](auto ms) {
        hipLaunchKernelGGL((aug_affine_decide_kernel<decltype(ms)::value>), dim3(N), dim3(64), 0, (hipStream_t)stream,
                           *cfg, iteration, E, params, in_boxes, in_kps, in_count, out_boxes, out_kps, out_count, table);
    });
    return hip_status();
}

extern "C" int yunet_aug_affine_pixels(const double* table, const float border_val[3], int N, int E,
                                       const int32_t* params, const float* in, float* out, void* stream) {
    if (!table || !border_val || !in || !out || in == out || N < 1 || E < 1 || E > YUNET_AUG_MAX_EDGE ||
        !std::isfinite(border_val[0]) || !std::isfinite(border_val[1]) || !std::isfinite(border_val[2]))
        return YUNET_EINVAL;
    const long long per_image = ((long long)E * E + 255) / 256;
    if (per_image * N > INT32_MAX) return YUNET_EINVAL;
    with_bool(params != nullptr, [&](auto ms) {
        hipLaunchKernelGGL((aug_affine_pixels_kernel<decltype(ms)::value>), dim3((unsigned)(per_image * N)), dim3(256), 0,
                           (hipStream_t)stream, table, border_val[0], border_val[1], border_val[2], E, (int)per_image,
                           params, in, out);
    });
    return hip_status();
}

extern "C" int yunet_aug_mixup_decide(const YunetMixupCfg* cfg, uint32_t iteration, int N, int E, const int32_t* params,
                                      int M, const int32_t* store_hw, const int32_t* store_goff,
                                      const int32_t* store_gcnt, const float* store_boxes, const float* store_kps,
                                      const float* in_boxes, const float* in_kps, const int32_t* in_count,
                                      float* out_boxes, float* out_kps, int32_t* out_count, double* table,
                                      void* stream) {
    if (!mixup_cfg_ok(cfg) || N < 1 || M < 1 || E < 1 || E > YUNET_AUG_MAX_EDGE || !store_hw || !store_goff ||
        !store_gcnt || !store_boxes || !store_kps || !in_boxes || !in_kps || !in_count || !out_boxes || !out_kps ||
        !out_count || !table || in_boxes == out_boxes || in_kps == out_kps || in_count == out_count)
        return YUNET_EINVAL;
    with_bool(params != nullptr, [&](auto ms) {
        hipLaunchKernelGGL((aug_mixup_decide_kernel<decltype(ms)::value>), dim3(N), dim3(64), 0, (hipStream_t)stream,
                           *cfg, iteration, E, params, M, store_hw, store_goff, store_gcnt, store_boxes, store_kps,
                           in_boxes, in_kps, in_count, out_boxes, out_kps, out_count, table);
    });
    return hip_status();
}

extern "C" int yunet_aug_mixup_pixels(const double* table, int D, float pad_val, int N, int E, const int32_t* params,
                                      int M, const uint8_t* store, const long long* store_off, const int32_t* store_hw,
                                      float* img, void* stream) {
    if (!table || !store || !store_off || !store_hw || !img || N < 1 || M < 1 || D < 1 || D > YUNET_AUG_MAX_EDGE / 2 ||
        E < 1 || E > YUNET_AUG_MAX_EDGE || !std::isfinite(pad_val))
        return YUNET_EINVAL;
    const long long per_image = ((long long)E * E + 255) / 256;
    if (per_image * N > INT32_MAX) return YUNET_EINVAL;
    with_bool(params != nullptr, [&](auto ms) {
        hipLaunchKernelGGL((aug_mixup_pixels_kernel<decltype(ms)::value>), dim3((unsigned)(per_image * N)), dim3(256), 0,
                           (hipStream_t)stream, table, D, pad_val, E, (int)per_image, params, M, store, store_off,
                           store_hw, img);
    });
    return hip_status();
}
