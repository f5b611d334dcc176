// test_pipeline.hip -- the reference TEST input pipeline of a batch on the device:
//   LoadImageFromFile -> MultiScaleFlipAug(Resize(keep_ratio=True) -> RandomFlip -> Normalize(0, 1) -> Pad) -> collate
// (mmdet/datasets/pipelines/test_time_aug.py:54-114, transforms.py:643-703; configs/yunet_n.py:57-102 there).
//
//   test_pixels_kernel : four output pixels of one row per thread.  Inside the image's nh x nw corner:
//       cv2.resize(uint8, INTER_LINEAR) in OpenCV's 11-bit fixed point -- the arithmetic of imresize.resize_linear_u8,
//       restated per pixel in oracle/cv2_resize_oracle.py -- of column nw - 1 - x for a flipped view, as fp32;
//       outside it 0 (Pad(pad_val=0) and the collate padding).  Planar NCHW, one 16-byte store per plane and thread.
//   rescale_dets_kernel: dets[n, :count[n], :4] /= scale_factor[n], kps[n, :count[n]] /= scale_factor[n][:2] in place
//       (yunet_head.py:357-361), so that a batch leaves the device in one copy.
//
// Built with -ffp-contract=off: the coefficient steps are OpenCV's single rounded double / float operations.
#include <cmath>

#include "common.h"

namespace {

// One destination coordinate d of an axis: taps t0 / t1 (clamped to the source) and their weights scaled by 2^11.
// `scale` = 1.0 / ((double)dst / (double)src).  border: the column rule (sx < 0 -> (0, 0); sx >= src - 1 ->
// (src - 1, 0)); rows only clamp their taps (imresize._axis_tables).
__device__ __forceinline__ void fixed_coef(int d, double scale, int src, bool border, int& t0, int& t1, int& w0,
                                           int& w1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (border) {
        if (s < 0) { f = 0.0f; s = 0; }
        if (s >= src - 1) { f = 0.0f; s = src - 1; }
    }
    const float c0 = 1.0f - f;
    w0 = (int)rintf(c0 * 2048.0f);          // cvRound: ties to even
    w1 = (int)rintf(f * 2048.0f);
    t0 = s < 0 ? 0 : s > src - 1 ? src - 1 : s;
    t1 = s + 1 < 0 ? 0 : s + 1 > src - 1 ? src - 1 : s + 1;
}

#define TEST_T_NH 0
#define TEST_T_NW 1
#define TEST_T_FLIP 2

// grid (blocks over the canvas' pixel quads, N); canvas Hc x Wc with Wc % 4 == 0.  Every source index is clamped into
// [0, h) x [0, w) of the image's own src_hw, so whatever the table holds nothing outside image n is read.
__global__ __launch_bounds__(256) void test_pixels_kernel(const uint8_t* __restrict__ src,
                                                          const long long* __restrict__ src_off,
                                                          const int32_t* __restrict__ src_hw,
                                                          const int32_t* __restrict__ table, int Hc, int Wc,
                                                          float* __restrict__ out) {
    const int n = blockIdx.y;
    const int h = src_hw[2 * n], w = src_hw[2 * n + 1];
    const int32_t* t = table + 4 * n;
    const bool ok = h > 0 && w > 0 && t[TEST_T_NH] > 0 && t[TEST_T_NW] > 0;
    const int nh = ok ? t[TEST_T_NH] : 0, nw = ok ? t[TEST_T_NW] : 0;
    const bool flip = t[TEST_T_FLIP] != 0;
    const bool same = nw == w && nh == h;                               // cv2: copy
    const bool half = !same && w == 2 * nw && h == 2 * nh;              // cv2: INTER_AREA fast path of exact 2 x
    const double sx = ok ? 1.0 / ((double)nw / (double)w) : 1.0;
    const double sy = ok ? 1.0 / ((double)nh / (double)h) : 1.0;
    const uint8_t* im = src + src_off[n];
    const size_t pitch = (size_t)w * 3, plane = (size_t)Hc * Wc;
    float* o = out + (size_t)n * 3 * plane;
    const int Wq = Wc >> 2, quads = Hc * Wq;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < quads; i += gridDim.x * 256) {
        const int dy = i / Wq, x4 = (i - dy * Wq) * 4;
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = 0.0f;
        if (dy < nh && x4 < nw) {
            int y0, y1, b0, b1;
            if (same) { y0 = y1 = dy; b0 = b1 = 0; }
            else if (half) { y0 = 2 * dy; y1 = 2 * dy + 1; b0 = b1 = 0; }
            else fixed_coef(dy, sy, h, false, y0, y1, b0, b1);
            const uint8_t* r0 = im + (size_t)y0 * pitch;
            const uint8_t* r1 = im + (size_t)y1 * pitch;
            int x0[4], x1[4], a0[4], a1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int dx = x4 + j < nw ? x4 + j : nw - 1;                 // a quad that straddles the corner's edge
                if (flip) dx = nw - 1 - dx;
                if (same) { x0[j] = x1[j] = dx; a0[j] = a1[j] = 0; }
                else if (half) { x0[j] = 2 * dx; x1[j] = 2 * dx + 1; a0[j] = a1[j] = 0; }
                else fixed_coef(dx, sx, w, true, x0[j], x1[j], a0[j], a1[j]);
            }
            // all 48 byte loads of the quad are issued before the first is consumed
            int p00[4][3], p01[4][3], p10[4][3], p11[4][3];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    p00[j][c] = r0[3 * x0[j] + c]; p01[j][c] = r0[3 * x1[j] + c];
                    p10[j][c] = r1[3 * x0[j] + c]; p11[j][c] = r1[3 * x1[j] + c];
                }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    int r;
                    if (same) {
                        r = p00[j][c];
                    } else if (half) {
                        r = (p00[j][c] + p01[j][c] + p10[j][c] + p11[j][c] + 2) >> 2;
                    } else {
                        const int H0 = (p00[j][c] * a0[j] + p01[j][c] * a1[j]) >> 4;
                        const int H1 = (p10[j][c] * a0[j] + p11[j][c] * a1[j]) >> 4;
                        r = (((H0 * b0) >> 16) + ((H1 * b1) >> 16) + 2) >> 2;
                        r = r < 0 ? 0 : r > 255 ? 255 : r;
                    }
                    v[c][j] = x4 + j < nw ? (float)r : 0.0f;
                }
        }
        const size_t at = (size_t)dy * Wc + x4;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(o + c * plane + at) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    }
}

__global__ __launch_bounds__(256) void rescale_dets_kernel(float* __restrict__ dets, float* __restrict__ kps,
                                                           const int32_t* __restrict__ count,
                                                           const float* __restrict__ sf, int max_out) {
    const int n = blockIdx.y;
    int cnt = count[n];
    cnt = cnt < 0 ? 0 : cnt > max_out ? max_out : cnt;
    const float s0 = sf[4 * n], s1 = sf[4 * n + 1], s2 = sf[4 * n + 2], s3 = sf[4 * n + 3];
    for (int r = blockIdx.x * 256 + threadIdx.x; r < cnt; r += gridDim.x * 256) {
        float* d = dets + ((size_t)n * max_out + r) * 5;
        d[0] = d[0] / s0; d[1] = d[1] / s1; d[2] = d[2] / s2; d[3] = d[3] / s3;
        if (kps) {
            float* k = kps + ((size_t)n * max_out + r) * 10;
#pragma unroll
            for (int j = 0; j < 5; ++j) { k[2 * j] = k[2 * j] / s0; k[2 * j + 1] = k[2 * j + 1] / s1; }
        }
    }
}

}  // namespace

extern "C" int yunet_test_pixels(const uint8_t* src, const long long* src_off, const int32_t* src_hw,
                                 const int32_t* table, int N, int Hc, int Wc, float* out_img, void* stream) {
    if (!src || !src_off || !src_hw || !table || !out_img || N < 1 || N > 65535 || Hc < 1 || Wc < 4 || (Wc & 3) ||
        Hc > YUNET_AUG_MAX_EDGE || Wc > YUNET_AUG_MAX_EDGE)
        return YUNET_EINVAL;
    const int quads = Hc * (Wc / 4);
    int cap = 4096 / N;                         // enough workgroups for 256 CUs at N = 1, grid-stride beyond
    if (cap < 16) cap = 16;
    int bx = (quads + 255) / 256;
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(test_pixels_kernel, dim3(bx, N), dim3(256), 0, (hipStream_t)stream, src, src_off, src_hw, table,
                       Hc, Wc, out_img);
    return hip_status();
}

extern "C" int yunet_rescale_dets(float* dets, float* kps, const int32_t* count, const float* scale_factor, int N,
                                  int max_out, void* stream) {
    if (!dets || !count || !scale_factor || N < 1 || N > 65535 || max_out < 0) return YUNET_EINVAL;
    if (max_out == 0) return 0;
    int bx = (max_out + 255) / 256;
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(rescale_dets_kernel, dim3(bx, N), dim3(256), 0, (hipStream_t)stream, dets, kps, count,
                       scale_factor, max_out);
    return hip_status();
}
