/*
 * yunet_hip.h -- C ABI of libyunet_hip.so, the MI355X (gfx950) kernels of the YuNet
 * training hot path.  Plain pointers and sizes only: every pointer is a DEVICE pointer
 * unless stated otherwise, `stream` is a hipStream_t passed as void*, every function
 * returns 0 on success or a negative YUNET_E* / the hipError_t of the failed launch.
 * No ownership is transferred; nothing is allocated; nothing synchronises (the inbox set-up of the
 * one-shot all-reduce at the end of this file is the one exception, and says so).
 *
 * The reference (ShiqiYu/libfacedetection.train) has no FFI: its drop-in boundary is
 * the mmcv Registry.  The registered Python classes of
 * libfacedetection.train_amd/ bind these entry points with ctypes; each entry point
 * names the reference code it replaces (paths relative to the reference root).
 *
 * Layouts: activations are NHWC fp32; parameters keep the reference's OIHW fp32
 * shapes (pointwise [Co,Ci,1,1], depthwise [C,1,3,3], stem [16,3,3,3]); images enter
 * as the reference delivers them, NCHW fp32.
 */
#ifndef YUNET_HIP_H
#define YUNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YUNET_ABI_VERSION 12

#define YUNET_EINVAL (-1)   /* bad argument / unsupported channel count */
#define YUNET_EOPCODE (-2)  /* unknown opcode in an op list            */

/* Train-mode BatchNorm description shared by producers and consumers.
 * The producer of a tensor accumulates `stats` = {sum[C], sumsq[C]} (fp64) over all
 * N*H*W positions; consumers derive scale = gamma*invstd, shift = beta - mean*scale in
 * their prologue (nn.BatchNorm2d defaults, mmdet/models/utils/yunet_layer.py:26,60).
 * In backward, consumers accumulate `bstats` = {sum dy[C], sum dy*xhat[C]} (fp64), i.e.
 * d(beta) and d(gamma); the producer's backward turns dy into dz with them. */
typedef struct YunetBN {
    const double* stats;   /* [slots][2*C] forward sums (zeroed before the step)      */
    double* bstats;        /* [slots][2*C] backward sums (zeroed before the step) or NULL */
    const float* gamma;    /* [C]                                                     */
    const float* beta;     /* [C]                                                     */
    int32_t count;         /* N*H*W of the normalised tensor                          */
    float eps;
    int32_t slots;         /* replicas of the sum blocks (0 and 1: one).  Workgroup b adds its partial sums
                            * into replica b % slots and every reader adds the replicas up: the fp64 atomics
                            * that end a kernel spread over `slots` times as many cache lines (at the 10 x 10
                            * and 20 x 20 levels ~250 workgroups x 128 atomics on eight lines cost 4-5 us of a
                            * 14-30 us launch)                  */
    int32_t det_rows;      /* 0: as above.  R > 0 (the deterministic mode, fp32 storage only): both sum blocks are
                            * [1 + R][2*C] and `slots` is 1 -- row 0 holds the sums every reader takes, workgroup b of a
                            * kernel that PRODUCES sums adds its partial sums, accumulated inside the workgroup in a
                            * fixed order, to row 1 + b with plain loads and stores (no atomics; a launch whose grid
                            * exceeds R is refused), and yunet_bn_fold adds rows 1 .. R into row 0 in a fixed order
                            * before the first reader runs.  Rows are zeroed before the step like the blocks above.
                            * R | YUNET_DET_FAST: the same blocks and rows, produced by the order-fixed forms of the
                            * kernels the default mode uses (below: the deterministic mode). */
} YunetBN;
/* Flag in YunetBN.det_rows, above the row count (every reader masks it off): the fast deterministic level. */
#define YUNET_DET_FAST (1 << 30)
#define YUNET_DET_ROWS(det_rows) ((det_rows) & (YUNET_DET_FAST - 1))

/* Input transform of a fused unit (how it reads its input tensor). */
enum { YUNET_T_IDENTITY = 0, YUNET_T_BNRELU = 1 };

/* Storage type of ACTIVATION tensors (raw conv outputs, pool / upsample-add outputs).  YUNET_BF16 is
 * BASELINE.json configs[2] "bf16 fwd / fp32 grads": activations are kept as bf16 in HBM and the
 * forward pointwise GEMM runs on the bf16 matrix instruction; gradients, the head output
 * [N,P,16], BatchNorm sums, parameters and the optimizer stay fp32.  (The reference's analogue is
 * its fp16 path: mmdet/apis/train.py:181-185, detectors/base.py:168, yunet_head.py:418 force_fp32.) */
enum { YUNET_F32 = 0, YUNET_BF16 = 1 };

/* One ConvDPUnit: 1x1 pointwise (bias) -> 3x3 depthwise (bias, zero-pads the pointwise
 * output) [-> BN -> ReLU applied by the consumer].
 * mmdet/models/utils/yunet_layer.py:4-36.  cin in {16,32,64}, cout in {16,32,64}. */
typedef struct YunetDP {
    int32_t N, H, W, cin, cout;
    int32_t in_transform;      /* YUNET_T_*: applied to x on load                     */
    int32_t out_has_bn;        /* 1: unit is followed by BN+ReLU (stats are produced) */
    int32_t accumulate_dx;     /* bwd: dx += instead of dx =                          */
    int64_t x_img_stride;      /* elements between images of x  (>= H*W*cin)          */
    int64_t z_img_stride;      /* elements between images of z  (>= H*W*cout)         */
    const float* x;            /* [N,H,W,cin] producer's raw output                   */
    YunetBN in_bn;             /* BN of the producer (when in_transform == BNRELU)    */
    const float* w_pw;         /* [cout,cin]                                          */
    const float* b_pw;         /* [cout]                                              */
    const float* w_dw;         /* [cout,9]                                            */
    const float* b_dw;         /* [cout]                                              */
    float* z;                  /* [N,H,W,cout] raw (pre-BN) output                    */
    YunetBN out_bn;            /* this unit's BN (stats written fwd, bstats read bwd) */
    /* backward only */
    const float* dy;           /* [N,H,W,cout] grad wrt BN output (or wrt z if no BN) */
    const float* dy_scale;     /* [cout] per-channel factor on dy (device) or NULL; read only when out_has_bn == 0 (the
                                  fused heads): behind an output BN the kernels fold that BN's backward into dz and
                                  ignore dy_scale */
    float* dx;                 /* [N,H,W,cin] grad wrt the BN output of the producer
                                  (ReLU mask applied) or wrt x if IDENTITY; NULL skips: no input gradient is written AND
                                  in_bn.bstats is left untouched (the producer's BN-backward sums are added only by a
                                  launch that writes dx); the weight and bias gradients are those of the launch with a dx,
                                  bit for bit.  x, dx and (with their own stride) z, dy may be strided: image i starts
                                  i * x_img_stride / i * z_img_stride elements after the pointer; the elements between
                                  the images are neither read nor written.  Every image must start on a 16-byte boundary
                                  (the kernels use 128-bit accesses): that is the caller's responsibility, the entry
                                  points do not check it (dense tensors and the [N,P,16] fp32 head output always do).
                                  A pooled dy (pool_idx), pool_out and pool_idx are always dense. */
    float* wgrad_partials;     /* [nblocks, cout*cin + cout + cout*9 + cout] fp32     */
    int32_t wgrad_blocks;      /* number of partial rows (= launch grid)              */
    unsigned long long* prof;  /* optional [grid,8] per-workgroup phase cycle counters (or NULL) */
    int32_t x_dtype;           /* YUNET_F32 | YUNET_BF16: storage of x (and of z unless z_dtype says otherwise) */
    int32_t z_dtype;           /* storage of z: equals x_dtype, except the fused heads, whose z is the fp32 [N,P,16] */
    /* Fused max_pool2d(2) of this unit's BN+ReLU output (both NULL: none).  Where yunet_dp_pool_fusion_ok()
     * says so and the pool is the output's ONLY consumer:
     *   forward : pool_out [N,H/2,W/2,cout] (activation storage type) receives, per 2x2 window and channel, the
     *             RAW z that wins the window after BN+ReLU (the maximum for gamma > 0, the minimum for gamma < 0,
     *             the first element for gamma == 0) and pool_idx [N,H/2,W/2,cout] its window position 2*dy + dx
     *             (ties: the smaller position, as F.max_pool2d).  The consumer reads pool_out with
     *             in_transform = BNRELU and THIS unit's BN (count = N*H*W): relu(bn(.)) is monotone, so that is
     *             max_pool2d(relu(bn(z))) exactly, and its backward yields the BN-backward sums unchanged.
     *   backward: pool_idx != NULL: dy is the POOLED gradient [N,H/2,W/2,cout] the consumer wrote as its dx
     *             (ReLU mask applied); it reaches the recorded window position while the tile is staged -- no
     *             full-size gradient of z exists.
     *   z == NULL: where nobody reads the full-size output -- the pool its only consumer, and a backward that
     *             recomputes z (yunet_dp_bwd_reads_z() == 0) -- yunet_dp_fwd accepts a NULL z for the 16 -> 16 unit
     *             with pool_out set that runs on the wave-streaming kernel (option "fwd16s", not deterministic -- or at its fast level --, no
     *             prof): the kernel then skips the z path and writes pool_out, pool_idx and the BN sums only, the same
     *             bytes as with a z.  yunet_dp_bwd accepts a NULL z exactly where yunet_dp_bwd_reads_z() is 0.  Every
     *             other unit, kernel and entry (yunet_dp_fwd_group included) returns YUNET_EINVAL for a NULL z and
     *             launches nothing. */
    float* pool_out;
    uint8_t* pool_idx;
} YunetDP;

/* ---- conv stack (mmdet/models/utils/yunet_layer.py, backbones/yunet_backbone.py:33-41,
 *      necks/tfpn.py:33-45, dense_heads/yunet_head.py:175-247) ------------------- */

/* ABI 10: n <= YUNET_DP_GROUP_MAX mutually INDEPENDENT ConvDPUnit forwards in one launch where the kernels allow it (plain
 * 64 -> 64 units on the wave-streaming kernel: the share convs of the pyramid levels, yunet_head.py:175-247, which the
 * reference walks in a Python loop); otherwise the units are launched one after the other.  Every unit computes exactly
 * what yunet_dp_fwd computes for it (same grid, same band height); only launch boundaries disappear.  Nothing may
 * connect the units: no output of one is an input (or a BatchNorm sum block) of another. */
#define YUNET_DP_GROUP_MAX 3
int yunet_dp_fwd_group(const YunetDP* const* units, int n, void* stream);

/* Conv_head.conv1: 3x3 stride-2 conv 3->cmid (+bias), NCHW image in, NHWC raw out,
 * BN statistics accumulated (yunet_layer.py:51-52,58). cmid must be 16. */
int yunet_stem_fwd(const float* img, const float* w, const float* b, float* z,
                   double* stats, int N, int H, int W, int cmid, void* stream);
/* weight/bias gradient of the stem (no input gradient: the image is a leaf).
 * dy is the grad wrt bn1's output with the ReLU mask applied; partials
 * [blocks, cmid*27 + cmid] are reduced by yunet_reduce_partials. */
int yunet_stem_bwd(const float* img, const float* z, const float* dy, const YunetBN* bn,
                   float* wgrad_partials, int wgrad_blocks, int N, int H, int W, int cmid,
                   void* stream);

/* The same weight gradient with z RECOMPUTED from the image (w [cmid,3,3,3], b [cmid]: the stem's parameters) instead of
 * read -- 112 instead of 176 bytes per output pixel -- as two matrix products on the matrix cores.  fp32 storage only. */
int yunet_stem_bwd_rz(const float* img, const float* w, const float* b, const float* dy, const YunetBN* bn,
                      float* wgrad_partials, int wgrad_blocks, int N, int H, int W, int cmid, void* stream);

/* Gradient with respect to the image: the backward-data of Conv_head.conv1 through bn1 (additive: the ABI number stays).
 *   dz = scale (dy - (sum dy + xhat sum(dy xhat)) / count) per z pixel and channel, from `bn` exactly as the weight-gradient
 *   entries above derive it (a frozen layer's reader descriptor has zero bstats: dz = scale dy, and z is not read);
 *   dimg[n][c][y][x] = sum_k sum_(ky,kx) w[k][c][ky][kx] dz[n][(y + 1 - ky) / 2][(x + 1 - kx) / 2][k] over the taps whose
 *   quotients are integers inside the map, in fp32 FMAs in a fixed order (no atomics: same input, same bits).
 * z [N,H/2,W/2,cmid] the stem's raw output as stored (fp32; bf16 for the _bf16 entry), dy [N,H/2,W/2,cmid] fp32 = the
 * gradient w.r.t. bn1's output with the ReLU mask applied (what yunet_stem_bwd reads), w [cmid,3,3,3], dimg [N,3,H,W] fp32
 * NCHW, 16-byte aligned: every element is written exactly once with plain stores.  YUNET_EINVAL, nothing launched, for a
 * NULL pointer (z, dy, bn and its four pointers, w, dimg), odd H or W, cmid != 16 or N < 1.
 * In an op list: YUNET_OP_STEM_BWD_DX. */
int yunet_stem_bwd_dx(const float* z, const float* dy, const YunetBN* bn, const float* w, float* dimg,
                      int N, int H, int W, int cmid, void* stream);

int yunet_dp_fwd(const YunetDP* d, void* stream);
int yunet_dp_bwd(const YunetDP* d, void* stream);

/* ---- deterministic mode (YunetBN.det_rows > 0) ------------------------------------------------------------------
 * The kernels that produce BatchNorm sums have a second form whose sums do not depend on the order in which waves
 * and workgroups happen to run: yunet_dp_fwd (out_bn.det_rows), yunet_dp_bwd (in_bn.det_rows), yunet_pool_bwd(_add),
 * yunet_upadd_bwd (bn->det_rows) select it from the descriptor, per launch: a launch that produces sums then runs on
 * the tile kernels (no wave-streaming kernels, no split-bf16 backward); a launch that produces none -- a unit without an
 * output BN in forward, a unit with an identity input transform in backward -- dispatches as without det_rows.  The
 * stem has the entry below.  Same inputs, same library and
 * same device model give the same bytes.  YUNET_EINVAL with bf16 activation storage.
 * The fast level (det_rows = R | YUNET_DET_FAST; same blocks, rows and fold): yunet_dp_fwd and yunet_dp_bwd take the
 * dispatch of the default mode -- the same predicates, tiles, grids and options -- and a launch that produces sums runs
 * the DET instance of the kernel chosen there: the wave-streaming kernels (16 -> 16, 16 -> 64, 64 -> 64 forward, 16 -> 16
 * backward; each wave adds its bands into an fp64 row of its own in LDS, the rows are added in wave order), the
 * split-bf16 64 -> 64 and 32 -> 64 backward, the whole-tile instances.  The arithmetic of everything but the sums is that
 * of the default mode, bit for bit; the bytes differ from the plain level's (other kernels).  A NULL z and
 * yunet_dp_bwd_reads_z() == 0 hold for the pooled 16 -> 16 unit as in the default mode; yunet_dp_fwd_group launches such
 * units one by one.  The element-wise kernels, the stem entry and yunet_bn_fold ignore the flag. */
/* yunet_stem_fwd with stats = a [1 + det_rows][2*cmid] block (det_rows >= 768, the kernel's grid). */
int yunet_stem_fwd_det(const float* img, const float* w, const float* b, float* z, double* stats, int det_rows,
                       int N, int H, int W, int cmid, void* stream);
/* block[0][j] = sum of block[1 .. rows][j], j < 2*C, in a fixed order: slice s (0 .. 15) adds rows 1 + s, 1 + s + 16,
 * ... in ascending order starting from 0.0, then the sixteen slice sums are added in ascending s starting from 0.0.
 * In an op list: YUNET_OP_BN_FOLD with p[0] = block, i[0] = rows, i[1] = C. */
int yunet_bn_fold(double* block, int rows, int C, void* stream);
/* rows of wgrad_partials (= persistent grid) yunet_dp_bwd / yunet_stem_bwd use for a shape */
int yunet_dp_bwd_blocks(int N, int H, int W, int cin, int cout);
/* 1 if yunet_dp_fwd / yunet_dp_bwd accept YunetDP.pool_out / pool_idx for this shape (the unpacked
 * 16->16 units on maps >= 32x64, the 32->64 units and the unpacked 64->64 units; H, W even) */
int yunet_dp_pool_fusion_ok(int N, int H, int W, int cin, int cout);
/* 0 if the kernel yunet_dp_bwd selects for this (backward) descriptor does not read YunetDP.z, under the options the
 * process runs with now: today the wave-streaming 16 -> 16 backward (option "bwd16s"; a big-tile map, out_has_bn, a plain
 * dx, no deterministic sums, no prof), which recomputes z from x.  1 for every other unit.  Host only. */
int yunet_dp_bwd_reads_z(const YunetDP* d);
/* The kernel instance yunet_dp_fwd (backward = 0) or yunet_dp_bwd (backward != 0) selects for this descriptor, under the
 * options the process runs with now, as the kernel's own name with every template argument and no blanks -- e.g.
 * dp_fwd_kernel<64,64,8,16,true,false,false>, dp_fwd16s_kernel<16,true,false>, dp_bwd64_kernel<4,false,true,false> -- the
 * name a profiler shows, the last argument (the deterministic form) included.  The storage build is the one d->x_dtype
 * names.  0 and the NUL-terminated name in name[0 .. cap); YUNET_EINVAL, nothing written, for a descriptor the entry would
 * refuse before it launches (a refusal that needs the grid or the device is the launch's own), a NULL d or name, or a cap
 * the name does not fit.  Host only: no device is touched. */
int yunet_dp_route(const YunetDP* d, int backward, char* name, int cap);
/* 1 if yunet_dp_fwd_group (the build units[0]->x_dtype names) launches these n units as one grid under the options the
 * process runs with now, 0 if it launches them one by one or refuses the call.  Host only. */
int yunet_dp_fwd_group_one_grid(const YunetDP* const* units, int n);
int yunet_stem_bwd_blocks(int N, int H, int W);

/* F.max_pool2d(relu(bn(z)), 2)  (yunet_backbone.py:39-40).  out [N,H/2,W/2,C]. */
int yunet_pool_fwd(const float* z, const YunetBN* bn, float* out, int N, int H, int W, int C,
                   void* stream);
/* dy_out [N,H/2,W/2,C] -> dz-side grad wrt bn output (mask applied) [N,H,W,C]; accumulates
 * bn->bstats.  accumulate != 0: dx += . */
int yunet_pool_bwd(const float* z, const YunetBN* bn, const float* dy_out, float* dx,
                   int accumulate, int N, int H, int W, int C, void* stream);
/* The same with a second, full-size gradient of relu(bn(z)) added under the same mask: dx = mask (extra +
 * route(dy_out)), one set of bn->bstats sums.  `extra` [N,H,W,C] fp32 (NULL = yunet_pool_bwd).  Used where a pyramid
 * tap feeds both max_pool2d (yunet_backbone.py:39-40) and the identity branch of the TFPN merge (tfpn.py:39-40):
 * autograd adds the two gradients of the tap; here yunet_upadd_bwd(dxa = NULL) leaves its share to this call (ABI 8). */
int yunet_pool_bwd_add(const float* z, const YunetBN* bn, const float* dy_out, const float* extra, float* dx,
                       int accumulate, int N, int H, int W, int C, void* stream);

/* TFPN merge: out = relu(bn_a(za)) + nearest_up2(relu(bn_b(zb)))  (tfpn.py:39-40).
 * za [N,H,W,C], zb [N,H/2,W/2,C]. */
int yunet_upadd_fwd(const float* za, const YunetBN* bna, const float* zb, const YunetBN* bnb,
                    float* out, int N, int H, int W, int C, void* stream);
/* dxa == NULL: the share of the fine tensor (mask_a dout, and bna->bstats) is NOT produced -- the caller hands `dout`
 * to yunet_pool_bwd_add as `extra`; za is then not read. */
int yunet_upadd_bwd(const float* za, const YunetBN* bna, const float* zb, const YunetBN* bnb,
                    const float* dout, float* dxa, int accumulate_a, float* dxb,
                    int accumulate_b, int N, int H, int W, int C, void* stream);

/* BatchNorm running statistics: running = (1-m)*running + m*batch (unbiased var)
 * for `count` BN layers described by parallel arrays (host pointers to device ptrs). */
int yunet_bn_update_running(const double* stats, float* running_mean, float* running_var,
                            int C, int count, float momentum, void* stream);

/* Final BN parameter gradients: d(gamma) = bstats[C:2C], d(beta) = bstats[0:C] (a single-replica block). */
int yunet_bn_param_grad(const double* bstats, float* dgamma, float* dbeta, int C,
                        int accumulate, void* stream);

/* All BatchNorm layers of the model in ONE launch.  table (device, int32 [n,7]) rows:
 * {stats offset (doubles, into stats_base), C, count, running offset (floats),
 *  dgamma offset, dbeta offset (floats, into grad_base), slots (YunetBN::slots of the [slots][2C] block)}.
 * mode 0: running_mean/var update from the forward sums at stats_base + off;
 * mode 1: d(gamma), d(beta) from the backward sums at stats_base + off;
 * mode 2: eval() -- WRITES sums at stats_base + off whose mean / variance equal the running
 *         statistics, so the same forward kernels apply BatchNorm in eval mode. */
int yunet_bn_batch(const int32_t* table, int n, const double* stats_base, float* running_mean,
                   float* running_var, float momentum, float* grad_base, int mode, void* stream);

/* out[j] (+)= sum_b partials[b, j]  for j < width, deterministic order. */
int yunet_reduce_partials(const float* partials, int blocks, int width, float* out,
                          int accumulate, void* stream);

/* The same reduction for a whole table of partial buffers in ONE launch (all weight-gradient
 * reductions of a backward pass: ~20 tiny kernels otherwise).  `jobs` is a DEVICE array;
 * chunk0 = index of the job's first 64-column chunk in the grid (running sum of
 * ceil(width / 64)), total_chunks = the grid size. */
typedef struct YunetReduceJob {
    const float* partials;   /* [blocks, width] */
    float* out;              /* [width] */
    int32_t blocks, width, accumulate, chunk0;
} YunetReduceJob;
int yunet_reduce_partials_batch(const YunetReduceJob* jobs, int njobs, int total_chunks, void* stream);

/* ---- loss step (mmdet/models/dense_heads/yunet_head.py:418-604) ---------------------- */

#define YUNET_MAX_LEVELS 5
typedef struct YunetLevels {
    int32_t num_levels;
    int32_t h[YUNET_MAX_LEVELS], w[YUNET_MAX_LEVELS], stride[YUNET_MAX_LEVELS];
} YunetLevels;

/* Fused MlvlPointGenerator priors (core/anchor/point_generator.py:80-175, offset 0) +
 * _bbox_decode (yunet_head.py:376-386) + SimOTAAssigner._assign
 * (core/bbox/assigners/sim_ota_assigner.py:95-257, bbox_overlaps
 * core/bbox/iou_calculators/iou2d_calculator.py:232-253) + PseudoSampler, three launches: compaction
 * of the valid priors, top-k per (image, GT) pair, conflict resolution per image (two interchangeable sets of launches:
 * option "assign_v2" below; identical outputs).
 * flat [N,P,16] = cls | dx dy dw dh | obj | 10 kps.
 * gt_boxes [N,Gmax,4] xyxy, gt_kps [N,Gmax,5,3] (x,y,vis), gt_labels [N,Gmax] or NULL,
 * gt_count [N].  Outputs: gt_inds [N,P] int32 (1-based, 0 = background),
 * labels [N,P] int32 (-1 background) or NULL, max_overlaps [N,P] (-1e5 background),
 * img_stats [N,2] = {num_pos, sum of kps weights}.  scratch: [N,P,12] fp32 (ABI 3; 8 words before).
 * Ties at the k-th cost are broken towards the lowest prior index.
 * Limits (YUNET_EINVAL beyond them): P <= 65535 priors per image (16-bit candidate indices:
 * a 1760x1760 training crop; the shipped configs train at 320 - 640, P <= 8400), Gmax <= 4096. */
int yunet_assign(const float* flat, const float* gt_boxes, const float* gt_kps,
                 const int32_t* gt_labels, const int32_t* gt_count, const YunetLevels* lv,
                 int N, int P, int Gmax, float center_radius, int32_t* gt_inds,
                 int32_t* labels, float* max_overlaps, float* img_stats, float* scratch,
                 void* stream);

/* SimOTAAssigner's constructor arguments (sim_ota_assigner.py:25-33; ABI 6 -- rounds 1-3 compiled 10 / 3.0 / 1.0 in):
 * cost = cls_cost * cls_weight + iou_cost * iou_weight (+1e5 outside box-and-centre); dynamic k from the
 * candidate_topk largest IoUs (1 <= candidate_topk <= 16; the per-lane lists are compiled for 10 and for 16). */
typedef struct YunetAssignCfg {
    float center_radius;
    int32_t candidate_topk;
    float iou_weight, cls_weight;
} YunetAssignCfg;
/* yunet_assign_ex with explicit assigner parameters; in an op list YUNET_OP_ASSIGN reads f[0] = center_radius,
 * i[3] = candidate_topk (0: 10), f[1] = iou_weight, f[2] = cls_weight (both 0: 3.0 / 1.0). */
int yunet_assign_cfg(const float* flat, const float* pre_scores, const float* pre_boxes,
                     const float* gt_boxes, const float* gt_kps, const int32_t* gt_labels,
                     const int32_t* gt_count, const YunetLevels* lv, int N, int P, int Gmax,
                     const YunetAssignCfg* cfg, int32_t* gt_inds, int32_t* labels, float* max_overlaps,
                     float* img_stats, float* scratch, void* stream);

/* Same kernel driven through SimOTAAssigner.assign()'s own signature
 * (sim_ota_assigner.py:38-93): pred_scores [N,P] = sigmoid(cls)*sigmoid(obj) and
 * decoded_bboxes [N,P,4] are given instead of being derived from `flat` (flat may be NULL). */
int yunet_assign_ex(const float* flat, const float* pre_scores, const float* pre_boxes,
                    const float* gt_boxes, const float* gt_kps, const int32_t* gt_labels,
                    const int32_t* gt_count, const YunetLevels* lv, int N, int P, int Gmax,
                    float center_radius, int32_t* gt_inds, int32_t* labels, float* max_overlaps,
                    float* img_stats, float* scratch, void* stream);

/* norm[0] = sum_n num_pos / world (the rank-local term of reduce_mean, yunet_head.py:493-497,
 * to be all-reduced by the caller when world > 1), norm[1] = sum_n kps weight. */
int yunet_loss_norm(const float* img_stats, int N, float inv_world, float* norm, void* stream);

/* box losses of mmdet/models/losses/iou_loss.py: EIoULoss :194-227 | DIoULoss :137-172 | IoULoss :14-50 (mode linear /
 * square / log; YuNet_Head's own default is mode 'square', yunet_head.py:59-64) | GIoULoss :103-120 | CIoULoss :230-293 */
enum { YUNET_BOX_EIOU = 0, YUNET_BOX_DIOU = 1, YUNET_BOX_IOU_LINEAR = 2, YUNET_BOX_IOU_SQUARE = 3, YUNET_BOX_IOU_LOG = 4,
       YUNET_BOX_GIOU = 5, YUNET_BOX_CIOU = 6,
       YUNET_BOX_BOUNDED = 7   /* BoundedIoULoss, iou_loss.py:55-97: beta in smooth_point, eps in box_eps; runs in the second
                                * instance of the loss kernel (yunet_loss_terms, or yunet_loss, which forwards this code) */ };
typedef struct YunetLossCfg {
    int32_t box_loss;            /* YUNET_BOX_*  (losses/iou_loss.py:194-227 / 137-172) */
    float w_cls, w_box, w_obj, w_kps;   /* loss_weight of each term                    */
    float box_eps;               /* EIoULoss/DIoULoss eps (1e-6)                       */
    float smooth_point;          /* EIoU 0.1                                           */
    float kps_beta;              /* SmoothL1 beta (1/9)                                */
    int32_t defer_num_total;     /* ABI 6, multi-GPU: 1 = norm[0] is NOT read -- loss_cls / loss_bbox / loss_obj and
                                  * their d/d(flat) leave yunet_loss un-normalised; yunet_loss_finalize_ex applies
                                  * 1 / max(num_total, 1) once the all-reduce of num_pos (yunet_head.py:493-497) has
                                  * landed, so that collective runs beside the loss kernel instead of in front of it */
} YunetLossCfg;

/* The four YuNet_Head losses and d(loss_i)/d(flat) in one pass (yunet_head.py:506-532,
 * losses/cross_entropy_loss.py:85-145, iou_loss.py, smooth_l1_loss.py:10-32,
 * losses/utils.py:29-55).  norm[0] is the (all-reduced) mean num_pos, clamped to >= 1
 * inside.  dflat [N,P,16] receives d(loss_c)/d(flat) for the loss that owns channel c,
 * each with unit upstream gradient.  dflat may be NULL (here, in yunet_loss_terms and as p[6] of a YUNET_OP_LOSS):
 * a value-only instance of the kernel runs, which stores no gradient and writes the same partial rows bit for bit
 * (a validation step; cfg.defer_num_total works as in the other form).  partials [blocks,4] -> losses via
 * yunet_loss_finalize: losses[5] = {cls, bbox, obj, kps, total}, total = ((cls+bbox)+obj)+kps
 * in fp32 -- the sum _parse_losses builds (mmdet/models/detectors/base.py:206-209).
 * `mirror` (nullable) receives the same five floats a second time: the host keeps it behind
 * the flat gradient buffer so that the logged scalars ride in the gradient all-reduce. */
int yunet_loss(const float* flat, const int32_t* gt_inds, const float* max_overlaps,
               const float* gt_boxes, const float* gt_kps, const YunetLevels* lv,
               const YunetLossCfg* cfg, const float* norm, int N, int P, int Gmax,
               float* dflat, float* partials, int blocks, void* stream);
int yunet_loss_finalize(const float* partials, int blocks, float* losses, float* mirror,
                        void* stream);
/* Which loss each term uses, beyond the default selection (additive; NOT a member of YunetOp, whose layout is pinned).
 * All-zero = sigmoid BCE for cls and obj, smooth-L1 for kps: then yunet_loss_terms IS yunet_loss (same kernel, same bits).
 *   VarifocalLoss  (losses/varifocal_loss.py:11-56)  cls: positives, t = max_overlaps; obj: every prior, t in {0, 1}.  The
 *                  focal weight alpha |sigmoid(x) - t|^gamma of the t <= 0 side is differentiated (the reference does not
 *                  detach it).  gamma >= 1 and alpha >= 0 (YUNET_EINVAL otherwise).
 *   L1Loss (smooth_l1_loss.py:36-52) | MSELoss (mse_loss.py:9-12) | BalancedL1Loss (balanced_l1_loss.py:13-53; beta =
 *                  YunetLossCfg.kps_beta): the targets, visibility weight and normaliser of the smooth-L1 term.
 * In an op list: YUNET_OP_LOSS with i[4] = cls_loss, i[5] = obj_loss, i[6] = kps_loss, i[7] = cls_iou_weighted |
 * obj_iou_weighted << 1, f[0..5] = cls_alpha, cls_gamma, obj_alpha, obj_gamma, kps_alpha, kps_gamma. */
enum { YUNET_CLS_BCE = 0, YUNET_CLS_VARIFOCAL = 1 };
enum { YUNET_KPS_SMOOTH_L1 = 0, YUNET_KPS_L1 = 1, YUNET_KPS_MSE = 2, YUNET_KPS_BALANCED_L1 = 3 };
typedef struct YunetLossTerms {
    int32_t cls_loss, obj_loss;  /* YUNET_CLS_*                                        */
    int32_t kps_loss;            /* YUNET_KPS_*                                        */
    int32_t cls_iou_weighted, obj_iou_weighted;   /* VarifocalLoss.iou_weighted         */
    float cls_alpha, cls_gamma;  /* VarifocalLoss of loss_cls (0.75, 2.0)              */
    float obj_alpha, obj_gamma;  /* VarifocalLoss of loss_obj                          */
    float kps_alpha, kps_gamma;  /* BalancedL1Loss (0.5, 1.5)                          */
} YunetLossTerms;
/* yunet_loss with the terms chosen by `terms` (NULL = all-zero). */
int yunet_loss_terms(const float* flat, const int32_t* gt_inds, const float* max_overlaps,
                     const float* gt_boxes, const float* gt_kps, const YunetLevels* lv,
                     const YunetLossCfg* cfg, const YunetLossTerms* terms, const float* norm, int N, int P, int Gmax,
                     float* dflat, float* partials, int blocks, void* stream);
/* yunet_loss_finalize with the deferred normaliser of YunetLossCfg.defer_num_total: num_total (device, nullable) = the
 * all-reduced mean num_pos; the first three losses are multiplied by 1 / max(num_total[0], 1) and dy_norm [16]
 * (nullable) receives the per-channel factor of d(loss)/d(flat) -- that value for cls | dx dy dw dh | obj, 1 for the
 * ten kps channels (normalised by the rank-local weight sum inside yunet_loss) -- which the fused head units take
 * as YunetDP.dy_scale.  (x * 1.0 is exact: gradients are bit-identical to the undeferred form.)
 * In an op list: YUNET_OP_LOSS_FINALIZE with p[3] = num_total, p[4] = dy_norm. */
int yunet_loss_finalize_ex(const float* partials, int blocks, float* losses, float* mirror,
                           const float* num_total, float* dy_norm, void* stream);
int yunet_loss_blocks(int N, int P);

/* ---- ignore regions (additive) ------------------------------------------------------------
 * yunet_ignore_mark: ign_boxes [N,Imax,4] xyxy fp32 (16-byte aligned), ign_count [N] int32 (clamped to 0 .. Imax; rows at
 * and beyond an image's count are never read), Imax <= 1024.  The candidate box of prior (x, y, s) is its cell
 * [x, y, x+s, y+s]; in fp32 iw = max(min(x2, x+s) - max(x1, x), 0), ih likewise, iof = iw * ih / (s * s).  A prior with
 * gt_inds == 0 whose largest iof over its image's boxes is > thr (strict; thr >= 0) gets gt_inds = -1, mmdet's
 * AssignResult convention; positives keep their assignment.  n_marked [N] int32 (nullable) receives the number of
 * priors marked per image (zeroed by a memset in front of the launch).  One launch, between yunet_assign* and yunet_loss*; img_stats and
 * the normalisers are not touched.
 * In an op list: YUNET_OP_IGNORE_MARK with p[0] = ign_boxes, p[1] = ign_count, p[2] = gt_inds, p[3] = n_marked,
 * i[0] = N, i[1] = P, i[2] = Imax, f[0] = thr, lv. */
int yunet_ignore_mark(const float* ign_boxes, const int32_t* ign_count, const YunetLevels* lv, int N, int P, int Imax,
                      float thr, int32_t* gt_inds, int32_t* n_marked, void* stream);
/* yunet_loss_terms with a flag word.  YUNET_LOSS_IGNORE: priors with gt_inds < 0 add nothing to loss_obj (BCE and
 * Varifocal) and all 16 channels of their dflat row are 0; num_total, loss_cls, loss_bbox and loss_kps are over the
 * positives and do not change.  Separate instances of the kernel: flags = 0 IS yunet_loss_terms, and a flagged launch
 * over gt_inds without a negative entry writes the same bytes.  In an op list: YUNET_OP_LOSS with i[8] = flags. */
enum { YUNET_LOSS_IGNORE = 1 };
int yunet_loss_terms_ex(const float* flat, const int32_t* gt_inds, const float* max_overlaps,
                        const float* gt_boxes, const float* gt_kps, const YunetLevels* lv,
                        const YunetLossCfg* cfg, const YunetLossTerms* terms, int flags, const float* norm, int N, int P,
                        int Gmax, float* dflat, float* partials, int blocks, void* stream);

/* out[i] = a[i] + b[i] (ABI 9).  The one place the reference's head concatenates predictions that come from DIFFERENT
 * inputs: with per-level towers (YuNet_Head(stacked_convs > 0), yunet_head.py:115-147, 191-207) the cls map is computed
 * from the cls tower and bbox / obj / kps from the reg tower, then flattened side by side (:456-472).  Here each tower
 * feeds one fused 64 -> 16 head unit whose rows for the other tower's channels are zero, and the two [N,P,16] outputs
 * (exact zeros in the foreign channels) are added.  `out` may alias `a`. */
int yunet_add(const float* a, const float* b, float* out, size_t n, void* stream);

/* ---- optimizer (torch.optim.SGD semantics, configs/yunet_n.py:1) --------------------- */
/* g = grad*grad_scale + wd*p;  buf = first ? g : momentum*buf + g;  p -= lr*buf.
 * lr is read from device memory (lr_dev[0]) so schedules do not need a re-capture. */
int yunet_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n,
                   const float* lr_dev, float momentum, float weight_decay, float grad_scale,
                   int first_step, void* stream);
/* ABI 9: the remaining arguments of torch.optim.SGD (torch/optim/sgd.py _single_tensor_sgd):
 *   buf = first ? g : momentum*buf + (1 - dampening)*g;   p -= lr * (nesterov ? g + momentum*buf : buf);
 * momentum == 0: p -= lr*g and momentum_buf is not touched (may be NULL).  nesterov needs momentum > 0 and
 * dampening == 0 (YUNET_EINVAL otherwise, like torch's ValueError). */
int yunet_sgd_step_ex(float* params, const float* grads, float* momentum_buf, int64_t n,
                      const float* lr_dev, float momentum, float dampening, int nesterov,
                      float weight_decay, float grad_scale, int first_step, void* stream);

/* ---- optimizer surface: gradient clipping, parameter groups, Adam / AdamW (csrc/optim.hip) ---------------------------
 * The calls above stay the default path (one group, no clipping).  These serve optimizer.paramwise_cfg,
 * optimizer_config.grad_clip and optimizer.type = 'Adam' | 'AdamW'. */
#define YUNET_NORM_BLOCK 256          /* threads per block of yunet_grad_norm */
#define YUNET_NORM_TILE 4096          /* floats one block folds per trip */
#define YUNET_NORM_MAX_BLOCKS 256     /* its grid is min(ceil(n / TILE), MAX_BLOCKS): beyond that a block takes several tiles */
#define YUNET_NORM_SCRATCH_BYTES (8 + 8 * YUNET_NORM_MAX_BLOCKS)
enum { YUNET_NORM_INF = 0, YUNET_NORM_L1 = 1, YUNET_NORM_L2 = 2 };
#define YUNET_OPT_ROW 4               /* doubles per group: lr, weight_decay, momentum (SGD) | beta1 (Adam), beta2 */
#define YUNET_OPT_MAX_GROUPS 255
#define YUNET_OPT_FROZEN 255          /* byte of the group map that means NO UPDATE (group ids end at 254): the grouped kernels
                                       * leave such an element's parameter and state (momentum | exp_avg, exp_avg_sq) untouched
                                       * and read neither its gradient nor a table row -- parameters with requires_grad = False
                                       * and elements no group covers (optim.py) */

/* torch.nn.utils.clip_grad_norm_ without its host side: out[0] = || grads * grad_scale ||_p  (norm_type YUNET_NORM_*),
 * out[1] = min(1, max_norm / (out[0] + 1e-6)), both written by the one launch, nothing read back.  The sum runs in fp64 in
 * a fixed order (no float atomics): the same input gives the same bits, whatever the alignment of `grads`.
 * `scratch`: YUNET_NORM_SCRATCH_BYTES of device memory, 8-byte aligned, ZERO when first used and owned by these calls
 * afterwards (a launch leaves it ready for the next one: no memset in between); one scratch per stream. */
int yunet_grad_norm(const float* grads, int64_t n, float grad_scale, int norm_type, float max_norm, void* scratch,
                    float* out, void* stream);
/* yunet_sgd_step_ex with lr / weight_decay / momentum per parameter group: element i belongs to group group_of_elem[i]
 * (< n_groups <= YUNET_OPT_MAX_GROUPS; YUNET_OPT_FROZEN: the element is skipped) and reads row group_of_elem[i] of `table`
 * ([n_groups, YUNET_OPT_ROW] doubles in device memory, rounded to fp32 the way torch rounds its python scalars).  The gradient is multiplied by
 * grad_scale * clip_coef[0]; clip_coef is out + 1 of yunet_grad_norm, or NULL for no clipping.  A group with momentum 0
 * leaves its part of momentum_buf alone.  One group and clip_coef = NULL give the bits of yunet_sgd_step_ex. */
int yunet_sgd_step_grouped(float* params, const float* grads, float* momentum_buf, int64_t n,
                           const uint8_t* group_of_elem, const double* table, int n_groups, float dampening,
                           int nesterov, float grad_scale, const float* clip_coef, int first_step, void* stream);
/* torch.optim.Adam (decoupled = 0: weight decay added to the gradient) / AdamW (decoupled = 1: p *= 1 - lr * wd), the
 * single-tensor form without amsgrad / maximize / capturable; `step` >= 1 counts this update (bias corrections
 * 1 - beta^step are formed in fp64 on the device).  exp_avg / exp_avg_sq are flat like params, zero before step 1. */
int yunet_adam_step_grouped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                            const uint8_t* group_of_elem, const double* table, int n_groups, float eps, int decoupled,
                            int step, float grad_scale, const float* clip_coef, void* stream);
/* Gradient accumulation over the flat gradient (the parameter range only, never the logged scalars in front of it):
 *   YUNET_ACCUM_SAVE   acc[i] = grads[i]              in front of a backward that is to ADD to what grads holds
 *   YUNET_ACCUM_ADD    grads[i] = acc[i] + grads[i]   behind it: one fp32 add per element (NaN / Inf propagate, -0 + -0 = -0)
 * Element-wise, 16-byte accesses where grads and acc reach a 16-byte boundary after the same number of elements (scalar
 * head and tail; everything scalar otherwise); both pointers 4-byte aligned, any n >= 0 (n = 0: nothing is launched).  No
 * atomics: the same input gives the same bits.  One launch on `stream`. */
enum { YUNET_ACCUM_SAVE = 0, YUNET_ACCUM_ADD = 1 };
int yunet_grad_accum(float* acc, float* grads, int64_t n, int mode, void* stream);

/* ---- op-list executor ---------------------------------------------------------------- */
/* A training step is a fixed sequence of the calls above; the host builds it once as an
 * array of YunetOp and replays it with one FFI call per phase. */
enum {
    YUNET_OP_STEM_FWD = 1, YUNET_OP_STEM_BWD, YUNET_OP_DP_FWD, YUNET_OP_DP_BWD,
    YUNET_OP_POOL_FWD, YUNET_OP_POOL_BWD, YUNET_OP_UPADD_FWD, YUNET_OP_UPADD_BWD,
    YUNET_OP_BN_RUNNING, YUNET_OP_BN_PARAM_GRAD, YUNET_OP_REDUCE_PARTIALS,
    YUNET_OP_ASSIGN, YUNET_OP_LOSS_NORM, YUNET_OP_LOSS, YUNET_OP_LOSS_FINALIZE,
    YUNET_OP_SGD, YUNET_OP_MEMSET, YUNET_OP_BN_BATCH, YUNET_OP_REDUCE_BATCH,
    YUNET_OP_FORK, YUNET_OP_JOIN,
    YUNET_OP_ADD,     /* ABI 9: yunet_add(p[0], p[1], p[2], n = i[1] << 32 | i[0]) */
    YUNET_OP_BN_FOLD, /* yunet_bn_fold(p[0], i[0], i[1]); YUNET_OP_STEM_FWD with i[4] = det_rows > 0 is yunet_stem_fwd_det */
    YUNET_OP_STEM_BWD_DX, /* yunet_stem_bwd_dx[_bf16 by i[11]](z = p[1], dy = p[2], &bn[0], w = p[3], dimg = p[0],
                             N = i[0], H = i[1], W = i[2], cmid = i[3]) */
    YUNET_OP_IGNORE_MARK  /* yunet_ignore_mark(p[0], p[1], &lv, i[0], i[1], i[2], f[0], gt_inds = p[2], n_marked = p[3]) */
};
/* Lanes (ABI 4).  The head chains of the pyramid levels (share conv -> fused head, and their backward) are
 * mutually independent: mmdet/models/dense_heads/yunet_head.py:175-247 walks them in a Python loop, and on the
 * small levels one launch has ~200 tiles for 256 CUs.  An op with i[YUNET_OP_LANE] = L > 0 is launched on the
 * executor's side stream L (two side streams, created on first use) instead of `stream`:
 *   YUNET_OP_FORK  i[0] = bit mask of lanes: those side streams wait for everything enqueued on `stream` so far;
 *   YUNET_OP_JOIN  i[0] = bit mask of lanes: `stream` waits for everything enqueued on those side streams.
 * A list must JOIN every lane it FORKed before it ends.  yunet_exec_lanes(0) makes the executor ignore lanes
 * (everything on `stream`, FORK / JOIN become no-ops): per-launch timing, debugging. */
#define YUNET_OP_LANE 10
#define YUNET_MAX_LANES 2
/* Groups (ABI 10).  A YUNET_OP_DP_FWD op with i[YUNET_OP_GROUP] = g in 2 .. YUNET_DP_GROUP_MAX declares that it and the
 * g - 1 ops after it (all YUNET_OP_DP_FWD, same lane, same storage type) are mutually independent: the executor hands them
 * to yunet_dp_fwd_group in one call.  0 / 1: an ordinary op.  An executor call that starts in the middle of a group (a
 * one-op replay for timing) runs the ops one by one. */
#define YUNET_OP_GROUP 9
typedef struct YunetOp {
    int32_t opcode;
    int32_t i[12];
    float f[8];
    void* p[12];
    YunetBN bn[2];
    YunetDP dp;
    YunetLevels lv;
    YunetLossCfg loss;
} YunetOp;
int yunet_exec(const YunetOp* ops /* HOST array */, int n_ops, void* stream);
int yunet_exec_lanes(int enable);   /* returns the previous setting */

/* ---- the conv stack with bf16 activation storage (YUNET_BF16, see the enum above) ----------------
 * Same arguments as the entry points without the suffix; pointers to ACTIVATION tensors (z, x, pool /
 * upsample-add inputs and outputs) then address bf16 elements, everything else (image, dy, dx, the
 * heads' [N,P,16] output, weights, partials, BN sums) is fp32 / fp64 as before.  yunet_exec selects
 * them per op (YunetDP.x_dtype, YunetOp.i[11]). */
int yunet_stem_fwd_bf16(const float* img, const float* w, const float* b, float* z, double* stats,
                        int N, int H, int W, int cmid, void* stream);
int yunet_stem_bwd_bf16(const float* img, const float* z, const float* dy, const YunetBN* bn,
                        float* wgrad_partials, int wgrad_blocks, int N, int H, int W, int cmid,
                        void* stream);
int yunet_stem_bwd_dx_bf16(const float* z, const float* dy, const YunetBN* bn, const float* w, float* dimg,
                           int N, int H, int W, int cmid, void* stream);
int yunet_dp_fwd_bf16(const YunetDP* d, void* stream);
int yunet_dp_fwd_group_bf16(const YunetDP* const* units, int n, void* stream);
int yunet_dp_bwd_bf16(const YunetDP* d, void* stream);
int yunet_pool_fwd_bf16(const float* z, const YunetBN* bn, float* out, int N, int H, int W, int C,
                        void* stream);
int yunet_pool_bwd_bf16(const float* z, const YunetBN* bn, const float* dy_out, float* dx,
                        int accumulate, int N, int H, int W, int C, void* stream);
int yunet_pool_bwd_add_bf16(const float* z, const YunetBN* bn, const float* dy_out, const float* extra, float* dx,
                            int accumulate, int N, int H, int W, int C, void* stream);
int yunet_upadd_fwd_bf16(const float* za, const YunetBN* bna, const float* zb, const YunetBN* bnb,
                         float* out, int N, int H, int W, int C, void* stream);
int yunet_upadd_bwd_bf16(const float* za, const YunetBN* bna, const float* zb, const YunetBN* bnb,
                         const float* dout, float* dxa, int accumulate_a, float* dxb,
                         int accumulate_b, int N, int H, int W, int C, void* stream);

/* ---- detection post-processing -------------------------------------
 * YuNet_Head.get_bboxes (mmdet/models/dense_heads/yunet_head.py:290-416): priors, sigmoid scores
 * (cls * obj) >= score_thr, _bbox_decode, then mmcv.ops.batched_nms for the single face class =
 * greedy NMS (IoU with offset 0, suppress when IoU > iou_thr), survivors in descending score.
 *  flat [N,P,16] raw head outputs of an eval-mode forward; any P (candidates above the threshold
 *  are compacted first; up to 16384 of them sort in LDS, more in the scratch -- an origin-size
 *  WIDER image of 1024x1024 has P = 21504, tools/test_widerface.py --mode 2).
 *  dets [N,max_out,5] = x1 y1 x2 y2 score; kps [N,max_out,10] decoded landmarks or NULL
 *  (_kps_decode, yunet_head.py:388-393); count [N]; scratch >= yunet_detect_scratch_bytes(N, P). */
size_t yunet_detect_scratch_bytes(int N, int P);
/* mmcv.ops.batched_nms for ONE class on explicit candidates (the merge step of test-time
 * augmentation, mmdet/models/dense_heads/dense_test_mixins.py:89-103): per set n the first
 * counts[n] (or all K when counts == NULL) rows of boxes [N,K,4] / scores [N,K] with
 * score >= score_thr, greedy NMS in descending score (ties: lower index first).
 * dets [N,max_out,5], keep [N,max_out] (indices into the set, or NULL), count [N];
 * scratch >= yunet_detect_scratch_bytes(N, K). */
int yunet_nms(const float* boxes, const float* scores, const int32_t* counts, int N, int K,
              float score_thr, float iou_thr, int max_out, float* dets, int32_t* keep,
              int32_t* count, void* scratch, void* stream);
int yunet_detect(const float* flat, const YunetLevels* lv, int N, int P, float score_thr,
                 float iou_thr, int max_out, float* dets, float* kps, int32_t* count, void* scratch,
                 void* stream);
/* Soft-NMS (test_cfg.nms = dict(type='soft_nms', iou_threshold, sigma, min_score, method)): the two entry points above
 * with mmcv.ops.soft_nms in place of the greedy sweep, for ONE class and offset 0 (additive: the ABI number stays).
 * Restated from mmcv 1.3.17's softnms_cpu -- mmcv is not part of the reference tree, so this is unpinned against it
 * (as the greedy NMS is).  Candidates: score >= score_thr with the score BEFORE any decay.  Then
 * rounds: the live candidate with the largest CURRENT score goes out with that score; every other live candidate's
 * score is multiplied (one fp32 multiply) by
 *    NAIVE    0 when IoU >= iou_thr, else 1
 *    LINEAR   1 - IoU when IoU >= iou_thr, else 1
 *    GAUSSIAN expf(-(IoU * IoU) / sigma), always (iou_thr unused)
 * and the candidate is dropped when its score is then below min_score -- also when the factor was 1, so a candidate
 * that starts below min_score (score_thr < min_score) survives only as the first selection.  Emitted scores are
 * non-increasing; at most max_out rows (= truncating the full result).  Equal current scores: the lower index first --
 * upstream's choice depends on its swap history, so EXACT score ties may resolve differently from mmcv.  NaN scores
 * are unsupported.  Outputs and scratch as yunet_detect / yunet_nms (kps: landmarks of the selected priors; keep:
 * indices into the set).  YUNET_EINVAL: soft == NULL, a method outside 0..2, a non-finite iou_thr / min_score, or
 * (GAUSSIAN) sigma <= 0 or non-finite. */
#define YUNET_SOFTNMS_NAIVE 0
#define YUNET_SOFTNMS_LINEAR 1
#define YUNET_SOFTNMS_GAUSSIAN 2
typedef struct YunetSoftNms {
    int32_t method;                 /* YUNET_SOFTNMS_* */
    float iou_thr, sigma, min_score;
} YunetSoftNms;
int yunet_detect_soft(const float* flat, const YunetLevels* lv, int N, int P, float score_thr,
                      const YunetSoftNms* soft, int max_out, float* dets, float* kps, int32_t* count,
                      void* scratch, void* stream);
int yunet_soft_nms(const float* boxes, const float* scores, const int32_t* counts, int N, int K,
                   float score_thr, const YunetSoftNms* soft, int max_out, float* dets, int32_t* keep,
                   int32_t* count, void* scratch, void* stream);

/* ---- device input pipeline ----------------------------------------
 * The reference's TRAIN pipeline (configs/yunet_n.py:36-56) on the device:
 *   RandomSquareCrop  mmdet/datasets/pipelines/transforms.py:975-1169
 *   Resize(keep_ratio=False)          transforms.py:242-299 (mmcv.imresize -> cv2 INTER_LINEAR)
 *   RandomFlip + 5-landmark swap      transforms.py:425-546
 *   collate to padded GT              mmdet/datasets/pipelines/formatting.py:206-249
 * Random draws come from a counter-based 32-bit generator keyed by (seed, iteration, image) --
 * restated in oracle/pipeline_oracle.py and pinned against the unmodified reference classes. */
typedef struct YunetAugCfg {
    int32_t out_size;        /* S of Resize(img_scale=(S, S)) */
    int32_t n_choice;        /* entries used in crop_choice, 1..8 */
    double crop_choice[8];   /* RandomSquareCrop(crop_choice=...); double: cw = int(scale * short) */
    double flip_ratio;       /* RandomFlip(flip_ratio=...) */
    float pad_value;         /* fill outside the source image (128, transforms.py:1128) */
    uint32_t seed;
    int32_t max_attempts;    /* window draws per scale (250, transforms.py:1058) */
    int32_t max_retries;     /* scale re-draws before giving up (the reference loops forever) */
    int32_t gmax;            /* rows of the padded GT outputs */
} YunetAugCfg;

/* Per image: decide scale / window / flip, transform and compact the kept boxes + keypoints.  One wavefront per image.
 *  src_hw [N,2] (h, w); boxes [*,4] xyxy; kps [*,5,3]; the GT rows of image n, by in_gmax:
 *      in_gmax == 0: ragged GT, gt_idx [N+1] prefix offsets -- rows [gt_idx[n], gt_idx[n+1]);
 *      in_gmax  > 0: padded GT [N, in_gmax, .] (the merged GT of yunet_aug_mosaic_decide), gt_idx [N] counts -- rows
 *                    [n * in_gmax, n * in_gmax + gt_idx[n]), the count clamped to [0, in_gmax].
 *  multiscale == 0: Resize(img_scale=(S, S)), S = cfg->out_size >= 1; scale_lo / scale_hi are ignored.
 *  multiscale != 0: Resize(img_scale=(a, b), multiscale_mode='square_range', keep_ratio=False), the reference's own
 *      addition to mmdet's Resize (transforms.py:99, 128-149, 226-228): one more draw per image, in the reference's
 *      position -- after the crop draws, before the flip draw: edge = scale_lo + floor(u32 / 2^32 * (scale_hi + 1 -
 *      scale_lo)) (numpy.random.randint(lo, hi + 1)), S_n = edge / 32 * 32.  Boxes, keypoints, clipping and flip are the
 *      fixed-size arithmetic with S_n in place of cfg->out_size (which is ignored).  An image with status 1 makes the
 *      draw too (no GT: it is its only draw).  YUNET_EINVAL unless 32 <= scale_lo <= scale_hi <= YUNET_AUG_MAX_EDGE.
 *  params [N,8] int32 = left, top, cw (0 = failed), flip, kept, draws, status, S_n (0 when multiscale == 0)
 *      status 0 ok, 1 no window with a box centre inside (or no GT), 2 kept > gmax (truncated);
 *  out_boxes [N,gmax,4], out_kps [N,gmax,5,3] (rows >= count zeroed), out_count [N].
 * The draws and the arithmetic do not depend on the GT layout: the same GT ragged or padded gives the same outputs. */
#define YUNET_AUG_MAX_EDGE 8192
int yunet_aug_decide(const int32_t* src_hw, const float* boxes, const float* kps, const int32_t* gt_idx, int in_gmax,
                     const YunetAugCfg* cfg, int multiscale, int scale_lo, int scale_hi, uint32_t iteration, int N,
                     int32_t* params, float* out_boxes, float* out_kps, int32_t* out_count, void* stream);

/* gt_bboxes_ignore through the same three transforms (it is a key of bbox_fields).  After yunet_aug_decide on the same
 * stream, one wavefront per image: reads the window, flip and S_n of params [N,8] and takes the ragged ignore boxes
 * ign_boxes [sum I,4] (rows of image n: ign_off[n] .. ign_off[n + 1]; NULL when there is none) through the arithmetic
 * of the GT boxes -- rows whose centre is strictly inside the patch, clipped to it, shifted (transforms.py:1099-1109),
 * scaled by the decide's factor (cfg out_size, or S_n when params[:,7] > 0) and clipped, flipped.  out_ign [N,imax,4]
 * (kept rows in order, the first imax of them; rows >= count zeroed), out_icount [N].  An image whose decide failed
 * (cw == 0) gets count 0.  Draws nothing: every other output of the pipeline keeps its bytes. */
int yunet_aug_ignore(const int32_t* params, const float* ign_boxes, const int32_t* ign_off, int out_size, int N, int imax,
                     float* out_ign, int32_t* out_icount, void* stream);

/* PhotoMetricDistortion (transforms.py:1211-1312) inside the pixel pass.  Positions in the pipeline list:
 *   PRE : between LoadAnnotations and RandomSquareCrop -- each in-image source tap is distorted after its uint8 ->
 *         float load; the crop's pad_value fill is not distorted (it is written after the transform);
 *   POST: between RandomFlip and Normalize -- every output pixel (pad pixels included) after the vertical pass.
 * Draws come from a SUB-STREAM of the counter-based generator: key mix32(stream_key(seed, iteration, image) ^
 * YUNET_PHOTO_SALT), counter from 0, so crop windows / flips / GT do not depend on whether or where the transform
 * sits.  The draws follow the reference's call order (conditional draws included):
 *   randint(2) brightness [uniform(-d, d)]; randint(2) mode; mode 1: randint(2) contrast [uniform];
 *   randint(2) saturation [uniform]; randint(2) hue [uniform]; mode 0: randint(2) contrast [uniform];
 *   randint(2) swap [permutation(3)]
 * randint(2) = u32 >> 31; uniform(a, b) = a + (b - a) * (u32 / 2^32) in double, then rounded to fp32 once (numpy 2 weak
 * Python-float scalar on a float32 image); permutation(3) = numpy's legacy Fisher-Yates, i = 2 then 1,
 * j = floor(u32 / 2^32 * (i + 1)).  Pixel arithmetic is fp32 in the reference's order, with cv2.cvtColor's scalar
 * float BGR<->HSV (h in degrees) restated -- unpinned against the cv2 binary, which is not available. */
#define YUNET_PHOTO_NONE 0
#define YUNET_PHOTO_PRE 1
#define YUNET_PHOTO_POST 2
#define YUNET_PHOTO_SALT 0x50484D44u   /* "PHMD" */
/* pparams [N, YUNET_PHOTO_WORDS] fp32 per image: flags are 0 / 1, the permutation entries 0..2 */
#define YUNET_PHOTO_WORDS 16
#define YUNET_PHOTO_BRIGHT 0     /* brightness fired */
#define YUNET_PHOTO_DELTA 1      /* its delta */
#define YUNET_PHOTO_MODE 2       /* 1: contrast before the HSV round trip, 0: after */
#define YUNET_PHOTO_CONTRAST 3   /* contrast fired */
#define YUNET_PHOTO_ALPHA 4
#define YUNET_PHOTO_SAT 5        /* saturation fired */
#define YUNET_PHOTO_SAT_F 6
#define YUNET_PHOTO_HUE 7        /* hue fired */
#define YUNET_PHOTO_HUE_D 8
#define YUNET_PHOTO_SWAP 9       /* channel swap fired */
#define YUNET_PHOTO_PERM 10      /* 10..12: output channel c = input channel perm[c] (identity when not fired) */
#define YUNET_PHOTO_DRAWS 13     /* u32 draws consumed from the sub-stream; 14, 15 zero */
typedef struct YunetPhotoCfg {
    double brightness_delta;     /* 32 */
    double contrast_lower, contrast_upper;        /* (0.5, 1.5) */
    double saturation_lower, saturation_upper;    /* (0.5, 1.5) */
    double hue_delta;            /* 18; at most 360 */
    int32_t position;            /* YUNET_PHOTO_PRE / YUNET_PHOTO_POST */
    int32_t reserved_;
} YunetPhotoCfg;
/* One thread per image: the draws of (seed, iteration, image) -> pparams.  YUNET_EINVAL for a bad cfg (lower > upper,
 * a negative or non-finite delta, hue_delta > 360, position not PRE / POST) or N < 1. */
int yunet_aug_photometric(const YunetPhotoCfg* cfg, uint32_t seed, uint32_t iteration, int N, float* pparams,
                          void* stream);
/* Mosaic(use_kps=True) (transforms.py:2218-2519) under MultiImageMixDataset (dataset_wrappers.py:338-444), in front of
 * RandomSquareCrop.
 *
 * Draws of image n come from a SUB-STREAM of the generator: key mix32(stream_key(seed, iteration, n) ^
 * YUNET_MOSAIC_SALT), counter from 0, in the reference's call order:
 *   3 x partner index  floor(u32 / 2^32 * M) over the M images of the store  (get_indexes: transforms.py imports
 *                      numpy's `random`, whose randint(0, len(dataset)) is [0, M) as well)
 *   1 x uniform(0, 1)  > prob: the image passes through unchanged (geom[YUNET_MOSAIC_APPLIED] = 0)
 *   2 x uniform(lo, hi) = lo + (hi - lo) * (u32 / 2^32) in double: center_x = int(. * S), then center_y
 * so the crop / size / flip / photometric draws are the same numbers with Mosaic present or absent.
 *
 * geom [N, YUNET_MOSAIC_WORDS] int32 per image: the header words below, then from word YUNET_MOSAIC_QUAD one block
 * of YUNET_MOSAIC_QWORDS words per sub-image in the order top-left (the image itself), top-right, bottom-left,
 * bottom-right. */
#define YUNET_MOSAIC_SALT 0x4D4F5341u  /* "MOSA" */
#define YUNET_MOSAIC_WORDS 80
#define YUNET_MOSAIC_APPLIED 0   /* 1: mosaic made, 0: skipped by prob */
#define YUNET_MOSAIC_CX 1        /* centre (0 when skipped) */
#define YUNET_MOSAIC_CY 2
#define YUNET_MOSAIC_DRAWS 3     /* u32 draws consumed from the sub-stream (6; 4 when skipped) */
#define YUNET_MOSAIC_KEPT 4      /* merged GT rows before the truncation to gmax */
#define YUNET_MOSAIC_STATUS 5    /* 0 ok, 2 kept > gmax (truncated), | 4 a sub-image resized to an empty size (not pasted) */
#define YUNET_MOSAIC_QUAD 16
#define YUNET_MOSAIC_QWORDS 16
#define YUNET_MOSAIC_Q_IDX 0     /* store index of the sub-image */
#define YUNET_MOSAIC_Q_H 1       /* its source size */
#define YUNET_MOSAIC_Q_W 2
#define YUNET_MOSAIC_Q_RW 3      /* resized size int(w * r), int(h * r), r = min(S / h, S / w) */
#define YUNET_MOSAIC_Q_RH 4
#define YUNET_MOSAIC_Q_PX1 5     /* paste rectangle on the canvas (_mosaic_combine) */
#define YUNET_MOSAIC_Q_PY1 6
#define YUNET_MOSAIC_Q_PX2 7
#define YUNET_MOSAIC_Q_PY2 8
#define YUNET_MOSAIC_Q_CX1 9     /* top-left corner of the crop rectangle in the resized sub-image */
#define YUNET_MOSAIC_Q_CY1 10
#define YUNET_MOSAIC_Q_SX 12     /* 12-13, 14-15: double 1 / (rw / w), 1 / (rh / h), the cv2 coordinate scales */
#define YUNET_MOSAIC_Q_SY 14
typedef struct YunetMosaicCfg {
    int32_t img_scale;           /* S of Mosaic(img_scale=(S, S)): the canvas is 2S x 2S */
    int32_t gmax;                /* rows of the merged GT outputs */
    double center_lo, center_hi; /* center_ratio_range, 0 <= lo <= hi <= 2 */
    double prob;
    float min_bbox_size;         /* used when skip_filter == 0 */
    float pad_val;               /* canvas fill (114) */
    uint32_t seed;
    int32_t bbox_clip_border;
    int32_t skip_filter;
    int32_t reserved_;
} YunetMosaicCfg;
/* One wavefront per image.  idx [N]: the batch's store indices (an index outside [0, M) is an empty image); store_*:
 * the tables of yunet_aug_gather.  Writes geom, out_hw [N,2] (2S x 2S, or the image's own size when skipped) and the
 * merged GT -- boxes / keypoints r * v + pad in fp32, clipped to the canvas (bbox_clip_border), filtered by
 * min_bbox_size (skip_filter == 0) and by find_inside_bboxes, compacted in the four-image order; the third keypoint
 * column travels untouched -- into out_boxes [N,gmax,4], out_kps [N,gmax,5,3] (rows >= count zeroed), out_count [N]:
 * the input of yunet_aug_decide (in_gmax = gmax).  A skipped image's own GT is copied through.  YUNET_EINVAL unless
 * 1 <= S <= YUNET_AUG_MAX_EDGE / 2, M >= 1, 0 <= lo <= hi <= 2, 0 <= prob <= 1. */
int yunet_aug_mosaic_decide(const int32_t* idx, int N, int M, const int32_t* store_hw, const int32_t* store_goff,
                            const int32_t* store_gcnt, const float* store_boxes, const float* store_kps,
                            const YunetMosaicCfg* cfg, uint32_t iteration, int32_t* geom, int32_t* out_hw,
                            float* out_boxes, float* out_kps, int32_t* out_count, void* stream);
/* The pixel pass, one launch per batch: crop (cfg->pad_value, 128, outside the source) -> bilinear resize -> flip, from
 * uint8 HWC sources (BGR as loaded) to planar fp32 out_img [N,3,E,E]; `params` from yunet_aug_decide.  Four independent
 * axes select the form; the crop / resize / flip float operations are the same in every form, so two forms that
 * describe the same pixels give bit-identical output.
 *
 *  rect     NULL: image n is the whole source at src + src_off[n], row pitch w * 3.
 *           else: a compact window buffer -- image n is the source rectangle rect[n] = (row0, col0, rows, cols) stored
 *                 at src + src_off[n] with row pitch cols * 3 (yunet_aug_window_plan, yunet_upload_windows /
 *                 yunet_fetch_windows); src_hw are the FULL source sizes.  Bit-identical to rect == NULL for the plan
 *                 of `params`; the rectangles do not depend on the output size.  A tap outside its rectangle (a plan
 *                 that does not belong to these params) reads pad instead of leaving the buffer.
 *  position YUNET_PHOTO_NONE: no distortion, pparams unused.  PRE / POST: PhotoMetricDistortion with the table pparams
 *           (yunet_aug_photometric of the same iteration).  PRE distorts each in-image source tap after its uint8 ->
 *           float load: the crop's pad fill is not distorted.  POST distorts every output pixel of the image (pad
 *           pixels included) after the vertical pass, never the zero border of a canvas.
 *  out_hw   0: E = cfg->out_size for every image (yunet_aug_decide with multiscale == 0).
 *           > 0: a multi-scale batch on a canvas, E = out_hw (the batch's max S_n): image n fills the top-left
 *                S_n x S_n corner, S_n = params[n][7], with exactly the floats out_hw == 0 gives at out_size = S_n;
 *                every other canvas pixel is 0.0f -- DefaultFormatBundle's padding_value (formatting.py:202, 231) as
 *                mmcv's collate applies it, bottom and right (the placement is mmcv's rule; mmcv is not part of the
 *                reference tree and is unpinned here).  A larger S_n is cut at the canvas, S_n <= 0 gives an all-zero
 *                image.  cfg->out_size is ignored.
 *  geom     NULL: no mosaic.
 *           else: Mosaic in front of the crop, geom / src_hw = the table and out_hw of yunet_aug_mosaic_decide, params
 *                 made from them by yunet_aug_decide (in_gmax > 0), `mosaic` its configuration, src the whole store and
 *                 src_off the STORE's offset table [M].  The mosaic canvas is never materialised: each tap of the
 *                 crop's bilinear resolves through geom -- outside the canvas cfg->pad_value, quadrant by the centre,
 *                 outside the paste rectangle mosaic->pad_val, else the inner bilinear tap of the uint8 sub-image
 *                 (src + src_off[idx]), rounded to fp32 as the reference's resized sub-image is, before the outer
 *                 interpolation reads it.  A skipped image reads its own source as geom == NULL does.
 *
 * Built: every combination of rect, position and out_hw without geom; with geom, rect == NULL and position NONE / POST
 * (a window buffer does not hold the partner images; PRE would distort the mosaic canvas, pad included).
 * YUNET_EINVAL, nothing launched: a NULL a, cfg, src, src_off, src_hw, params or out_img; N < 1; a position other than
 * the three; PRE / POST without pparams; out_hw < 0 or > YUNET_AUG_MAX_EDGE; out_hw == 0 with cfg->out_size < 1; geom
 * without mosaic or mosaic without geom; a bad mosaic configuration (yunet_aug_mosaic_decide); geom with rect or with
 * PRE. */
typedef struct YunetAugPixels {
    const uint8_t* src;            /* whole sources | window buffer | the whole store (mosaic) */
    const long long* src_off;      /* [N] byte offset of image n in src; mosaic: the store's offset table */
    const int32_t* src_hw;         /* [N,2] full source sizes; mosaic: out_hw of yunet_aug_mosaic_decide */
    const int32_t* rect;           /* NULL: whole images; else [N,4] of yunet_aug_window_plan */
    const int32_t* params;         /* [N,8] of yunet_aug_decide */
    const float* pparams;          /* table of yunet_aug_photometric; required unless position == YUNET_PHOTO_NONE */
    const int32_t* geom;           /* NULL: no mosaic; else the table of yunet_aug_mosaic_decide */
    const YunetMosaicCfg* mosaic;  /* non-NULL iff geom */
    int32_t position;              /* YUNET_PHOTO_NONE | PRE | POST */
    int32_t out_hw;                /* 0: every image cfg->out_size; > 0: canvas edge, image n = params[n][7] */
} YunetAugPixels;
int yunet_aug_pixels(const YunetAugPixels* a, const YunetAugCfg* cfg, int N, float* out_img, void* stream);
/* Test entry: the canvas itself through the tap function of yunet_aug_pixels' mosaic form, canvas [N, 2S, 2S, 3] fp32 HWC
 * (a skipped image's canvas is all pad_val). */
int yunet_aug_mosaic_canvas(const uint8_t* store, const long long* store_off, const int32_t* geom,
                            const YunetMosaicCfg* mcfg, int N, float* canvas, void* stream);

/* CutOut (transforms.py:2143-2214) on the finished batch tensor of yunet_aug_pixels: between RandomFlip (or a POST
 * PhotoMetricDistortion) and Normalize, so the fill value reaches the network as it is written.
 *
 * Draws of image n come from a SUB-STREAM of the generator: key mix32(stream_key(seed, iteration, n) ^
 * YUNET_CUTOUT_SALT), counter from 0, one u32 per randint in the reference's call order, with
 * randint(lo, hi) = lo + ((u32 * (hi - lo)) >> 32):
 *   draw 0          n_holes = randint(n_lo, n_hi + 1)             (made when n_lo == n_hi too)
 *   draw 1 + 3j     x1 = randint(0, w)                            hole j
 *   draw 2 + 3j     y1 = randint(0, h)
 *   draw 3 + 3j     index = randint(0, n_cand)                    (made with one candidate too)
 * so windows, flips, GT, photometric tables and mosaic geometry are the same numbers with CutOut present or absent, and
 * a hole's draws are addressed by its index.  w = h = the image's own edge S_n: E, or params[n][7] on a multi-scale
 * canvas (read on the device; a value above E counts as E, one below 1 gives the image no hole).
 *   shape mode (with_ratio == 0): (cw, ch) = cand[index], integers held as doubles
 *   ratio mode (with_ratio != 0): cw = (int)(cand[index][0] * (double)w), ch likewise -- Python's int(ratio * w)
 *   x2 = min(x1 + cw, w), y2 = min(y1 + ch, h)          (np.clip; the lower clip never acts, cw, ch >= 0)
 * and img[n, c, y1:y2, x1:x2] = fill[c].  A hole may be empty (cw or ch 0); holes never reach the zero border of a
 * multi-scale canvas; overlapping holes store the same values.
 *
 * holes [N, YUNET_CUTOUT_WORDS] int32 per image: word 0 n_holes, word 1 draws consumed (1 + 3 * n_holes), then
 * (x1, y1, x2, y2) per slot, zeros in the slots at and beyond n_holes. */
#define YUNET_CUTOUT_SALT 0x4355544Fu  /* "CUTO" */
#define YUNET_CUTOUT_MAX_HOLES 16
#define YUNET_CUTOUT_MAX_CANDIDATES 8
#define YUNET_CUTOUT_WORDS 66          /* 2 + 4 * YUNET_CUTOUT_MAX_HOLES */
typedef struct YunetCutoutCfg {
    int32_t n_lo, n_hi;          /* n_holes from the closed interval [n_lo, n_hi], 0 <= n_lo <= n_hi <= MAX_HOLES */
    int32_t n_cand;              /* entries used in cand, 1..YUNET_CUTOUT_MAX_CANDIDATES */
    int32_t with_ratio;          /* 0: cand are shapes in pixels, else ratios of the image's edge */
    double cand[YUNET_CUTOUT_MAX_CANDIDATES][2];   /* (w, h) per candidate, non-negative and finite */
    float fill[3];               /* fill_in per channel of the batch tensor (BGR) */
    uint32_t seed;
} YunetCutoutCfg;
/* One workgroup per (image, hole slot) on the current stream, in place on img [N, 3, E, E] fp32; params NULL: every
 * image's edge is E, else [N,8] of yunet_aug_decide (multiscale != 0).  YUNET_EINVAL, before any launch, for N < 1, E
 * outside [1, YUNET_AUG_MAX_EDGE], a null cfg / img / holes, n_lo < 0, n_lo > n_hi, n_hi > YUNET_CUTOUT_MAX_HOLES,
 * n_cand outside [1, YUNET_CUTOUT_MAX_CANDIDATES], a negative or non-finite candidate or a non-finite fill. */
int yunet_aug_cutout(const YunetCutoutCfg* cfg, uint32_t iteration, int N, int E, const int32_t* params, float* img,
                     int32_t* holes, void* stream);

/* RandomAffine (transforms.py:2787-3001) with the five landmarks, on the finished batch tensor and the finished GT of
 * yunet_aug_decide: after RandomFlip (and a POST PhotoMetricDistortion), in front of CutOut / Normalize.  border is
 * (0, 0): width = height = the image's own edge S_n (E, or params[n][7] on a multi-scale canvas, clamped to E).
 *
 * Draws of image n come from a SUB-STREAM: key mix32(stream_key(seed, iteration, n) ^ YUNET_AFFINE_SALT), counter from
 * 0, one u32 per random.uniform(a, b) = a + (b - a) * (u32 / 2^32) in doubles, in the reference's call order:
 *   draw 0  rotation degrees   uniform(-max_rotate_degree, max_rotate_degree)
 *   draw 1  scaling ratio      uniform(scale_lo, scale_hi)
 *   draw 2  shear x degrees    uniform(-max_shear_degree, max_shear_degree)
 *   draw 3  shear y degrees    likewise
 *   draw 4  translate x ratio  uniform(-max_translate_ratio, max_translate_ratio)     (trans_x = draw * width, a double)
 *   draw 5  translate y ratio  likewise                                               (trans_y = draw * height)
 * so windows, flips, GT, photometric tables, mosaic geometry and CutOut holes are the same numbers with the step
 * present or absent.  M = T @ Sh @ R @ Sc: cos / sin / tan of the radians in fp64, every factor rounded to fp32, the
 * 3 x 3 products in fp32 from left to right (each entry a0*b0 + a1*b1 + a2*b2, no fused multiply-add).  The bottom row
 * of M is (0, 0, 1) exactly, so the reference's division by the third coordinate is a division by 1.
 *
 * GT: the corners (x1,y1) (x1,y2) (x2,y2) (x2,y1) of a box through M in fp32, min / max, the clip to [0, S] under
 * bbox_clip_border; a row survives find_inside_bboxes (x1 < S, x2 > 0, y1 < S, y2 > 0) and, with skip_filter == 0,
 * filter_gt_bboxes on (box * (float)scale): w > min_bbox_size and h > min_bbox_size, w * h / (ow * oh + 1e-16) >
 * min_area_ratio, max(w / (h + 1e-16), h / (w + 1e-16)) < max_aspect_ratio, all in fp32.  Survivors are compacted in
 * order with their keypoint rows: (x, y) of the five points through M, clipped to [0, S] under bbox_clip_border, the
 * third value as it was.  Rows at and beyond the new count are 0.
 *
 * table [N, YUNET_AFFINE_WORDS] doubles per image: the six draws, M row-major (fp32 values), the upper two rows of
 * M^-1 row-major (computed in fp64 from M), rows before, rows after, S. */
#define YUNET_AFFINE_SALT 0x41464649u  /* "AFFI" */
#define YUNET_AFFINE_WORDS 24
#define YUNET_AFFINE_DRAWS 0           /* 6 */
#define YUNET_AFFINE_M 6               /* 9 */
#define YUNET_AFFINE_INV 15            /* 6: i00 i01 i02 i10 i11 i12 */
#define YUNET_AFFINE_ROWS_IN 21
#define YUNET_AFFINE_ROWS_OUT 22
#define YUNET_AFFINE_EDGE 23
#define YUNET_AFFINE_MAX_SHEAR 45.0    /* degrees: below it det(Sh) = 1 - tan(sx) tan(sy) > 0, so M never mirrors */
typedef struct YunetAffineCfg {
    double max_rotate_degree;    /* finite */
    double max_translate_ratio;  /* in [0, 1] */
    double scale_lo, scale_hi;   /* 0 < scale_lo <= scale_hi, finite */
    double max_shear_degree;     /* |.| < YUNET_AFFINE_MAX_SHEAR */
    float min_bbox_size, min_area_ratio, max_aspect_ratio;   /* finite; read with skip_filter == 0 */
    float border_val[3];         /* per channel of the batch tensor (BGR), finite */
    int32_t bbox_clip_border, skip_filter;
    int32_t gmax;                /* padded GT rows per image, in and out: 1..4096 */
    uint32_t seed;
} YunetAffineCfg;
/* One workgroup per image on the current stream.  in_boxes [N, gmax, 4], in_kps [N, gmax, 15], in_count [N] (a count
 * outside [0, gmax] is clamped) -> out_boxes / out_kps / out_count of the same shapes (other buffers than the inputs)
 * and table.  params NULL: every image's edge is E, else [N,8] of yunet_aug_decide (multiscale != 0).  YUNET_EINVAL,
 * before any launch, for a null cfg / in / out / table pointer, N < 1, E outside [1, YUNET_AUG_MAX_EDGE], an output
 * that is its input, and a configuration outside the ranges above. */
int yunet_aug_affine_decide(const YunetAffineCfg* cfg, uint32_t iteration, int N, int E, const int32_t* params,
                            const float* in_boxes, const float* in_kps, const int32_t* in_count, float* out_boxes,
                            float* out_kps, int32_t* out_count, double* table, void* stream);
/* The pixels of cv2.warpPerspective(img, M, (S, S), borderValue=border_val), bilinear: out[n, c, y, x] for x, y < S_n
 * samples in[n, c] at (sx, sy) = M^-1 (x, y, 1) -- the table's six inverse words rounded to fp32, sx = (i00 * x + i01 * y)
 * + i02 in fp32 -- with x0 = floor(sx), fx = sx - x0 and the weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy; a tap outside
 * [0, S_n) contributes border_val[c], a pixel whose four taps are all outside is border_val[c]; a coordinate
 * on the pixel grid (fx = fy = 0) copies its pixel.  Pixels at or beyond
 * S_n (the multi-scale canvas) are 0.  cv2's fixed-point coordinate table (1/32 pixel) is not reproduced.  in and out
 * [N, 3, E, E] fp32, different buffers; only the YUNET_AFFINE_INV words of table are read.  YUNET_EINVAL, before any
 * launch, for a null table / border_val / in / out, in == out, N < 1, E outside [1, YUNET_AUG_MAX_EDGE], more than 2^31 - 1
 * workgroups (N * ceil(E * E / 256)) or a non-finite border_val. */
int yunet_aug_affine_pixels(const double* table, const float border_val[3], int N, int E, const int32_t* params,
                            const float* in, float* out, void* stream);

/* MixUp (transforms.py:2523-2783) with the five landmarks, on the finished batch tensor and the finished GT: after
 * RandomFlip (a POST PhotoMetricDistortion, RandomAffine), in front of CutOut / Normalize.  The partner is a raw decoded
 * image of the store with its raw GT (what MultiImageMixDataset hands over as mix_results).  T = the image's own edge
 * S_n (E, or params[n][7] on a multi-scale canvas, clamped to E); D = img_scale.
 *
 * Draws of image n come from a SUB-STREAM: key mix32(stream_key(seed, iteration, n) ^ YUNET_MIXUP_SALT), counter from
 * 0, in the reference's call order (its `random` is numpy's: randint excludes the upper end):
 *   up to max_iters  partner = (u32 * M) >> 32, stopping at the first with store_gcnt != 0          (get_indexes)
 *   -- the last partner drawn has no boxes: NOT APPLIED; no further draw, the GT is copied, the pixels keep their bytes
 *   jit  = lo + (hi - lo) * (u32 / 2^32)            random.uniform(*ratio_range), doubles
 *   flip = (u32 / 2^32) > flip_ratio                the reference's inequality
 *   y_offset = (u32 * (P - T)) >> 32  only if P > T, then x_offset likewise          P = max(J, T)
 * so windows, flips, GT before MixUp, photometric tables, mosaic geometry, affine tables and CutOut holes are the same
 * numbers with the step present or absent.  Geometry in integers and doubles, as the Python code has it: partner h x w,
 * sr = min(D / h, D / w), rw = (int)(w * sr), rh = (int)(h * sr), J = (int)(D * jit), sr *= jit.  rw, rh or J below 1
 * (cv2 would refuse the empty size): status 4, not applied.
 *
 * GT, fp32 with one rounding per operation.  Partner box: * (float)sr; clip to [0, J] under bbox_clip_border; flipped:
 * (x1, x2) = (J - x2, J - x1); then the copy: minus the offsets, clip to [0, T] under bbox_clip_border.  With
 * skip_filter == 0 a partner row survives _filter_box_candidates(before the offsets, after): w2 > min_bbox_size,
 * h2 > min_bbox_size, w2 * h2 / (w1 * h1 + 1e-16) > min_area_ratio, max(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16)) <
 * max_aspect_ratio.  The image's own rows come first, then the partner's; find_inside_bboxes (x1 < T, x2 > 0, y1 < T,
 * y2 > 0) runs over all of them, the image's own included; survivors are compacted in order, rows at and beyond the
 * count are 0, rows beyond gmax are dropped (status 2).  The partner's landmarks: (x, y) * (float)sr, clip to [0, J]
 * under bbox_clip_border, flipped x = J - x with the points permuted [1, 0, 2, 4, 3], minus the offsets, clip to [0, T]
 * under bbox_clip_border; the third value as it was.
 *
 * table [N, YUNET_MIXUP_WORDS] doubles per image (integers held exactly). */
#define YUNET_MIXUP_SALT 0x4D495855u   /* "MIXU" */
#define YUNET_MIXUP_WORDS 18
#define YUNET_MIXUP_PARTNER 0          /* store index of the last partner drawn */
#define YUNET_MIXUP_APPLIED 1
#define YUNET_MIXUP_INDEX_DRAWS 2      /* partner draws made, 1..max_iters */
#define YUNET_MIXUP_JIT 3
#define YUNET_MIXUP_FLIP 4
#define YUNET_MIXUP_J 5
#define YUNET_MIXUP_RW 6
#define YUNET_MIXUP_RH 7
#define YUNET_MIXUP_XOFF 8
#define YUNET_MIXUP_YOFF 9
#define YUNET_MIXUP_SX 10              /* 1 / ((double)rw / w): raw-image coordinate scale of the first resize */
#define YUNET_MIXUP_SY 11              /* 1 / ((double)rh / h) */
#define YUNET_MIXUP_ROWS_IN 12         /* the image's own rows */
#define YUNET_MIXUP_ROWS_OUT 13        /* survivors, before the truncation to gmax */
#define YUNET_MIXUP_STATUS 14          /* bit 2: rows beyond gmax dropped; bit 4: an empty resize, not applied */
#define YUNET_MIXUP_EDGE 15            /* T */
#define YUNET_MIXUP_DRAWS 16           /* draws consumed in all */
#define YUNET_MIXUP_SR 17              /* sr * jit, the box scale as a double */
typedef struct YunetMixupCfg {
    double ratio_lo, ratio_hi;   /* 0 < lo <= hi, finite */
    double flip_ratio;           /* finite */
    float pad_val;               /* finite: the D x D canvas outside the resized partner */
    float min_bbox_size, min_area_ratio, max_aspect_ratio;   /* finite; read with skip_filter == 0 */
    int32_t img_scale;           /* D, 1..YUNET_AUG_MAX_EDGE / 2 */
    int32_t max_iters;           /* >= 1 */
    int32_t bbox_clip_border, skip_filter;
    int32_t gmax;                /* padded GT rows per image, in and out: 1..4096 */
    uint32_t seed;
} YunetMixupCfg;
/* One 64-lane workgroup per image on the current stream.  store_* : the tables of the M images of the store (hw [M,2],
 * first GT row / GT count [M], boxes [*,4], kps [*,15]).  in_boxes [N, gmax, 4], in_kps [N, gmax, 15], in_count [N] (a
 * count outside [0, gmax] is clamped) -> out_* of the same shapes (other buffers than the inputs) and table.  params
 * NULL: every image's edge is E, else [N,8] of yunet_aug_decide (multiscale != 0).  YUNET_EINVAL, before any launch, for
 * a null pointer, N < 1, M < 1, E outside [1, YUNET_AUG_MAX_EDGE], an output that is its input, and a configuration
 * outside the ranges above. */
int yunet_aug_mixup_decide(const YunetMixupCfg* cfg, uint32_t iteration, int N, int E, const int32_t* params, int M,
                           const int32_t* store_hw, const int32_t* store_goff, const int32_t* store_gcnt,
                           const float* store_boxes, const float* store_kps, const float* in_boxes, const float* in_kps,
                           const int32_t* in_count, float* out_boxes, float* out_kps, int32_t* out_count, double* table,
                           void* stream);
/* The blend, in place on img [N, 3, E, E] fp32: one thread per pixel, each reads and writes only its own pixel; an
 * image that is not applied is left alone.  For (x, y) with x, y < T of an applied image: (X, Y) = (x + x_offset,
 * y + y_offset); X >= J or Y >= J: b' = 0 (the zero padding of padded_img).  Else Xf = flip ? J - 1 - X : X and b is
 * the float bilinear value (cv2's float path: f = (float)((d + 0.5) * scale - 0.5), both border rules) of (Xf, Y) in
 * the D x D canvas at scale 1 / ((double)J / D).  A canvas tap (u, v) with u < rw and v < rh is the float bilinear value
 * of the raw partner image (uint8, w x h) at scales SX / SY; any other tap is pad_val.
 * Order of summation, every product and sum rounded to fp32 (no fused multiply-add), per channel:
 *   raw level     r0 = p[y0][x0] * a0 + p[y0][x1] * a1;   r1 = p[y1][x0] * a0 + p[y1][x1] * a1;   c = r0 * b0 + r1 * b1
 *   canvas level  t0 = c00 * A0 + c01 * A1;               t1 = c10 * A0 + c11 * A1;               b = t0 * B0 + t1 * B1
 * (horizontal pass, then vertical pass; weight w0 = 1 - f, w1 = f).  b' = trunc(b) (the reference's uint8 padded_img)
 * and out = trunc(min(max(0.5f * a + 0.5f * b', 0), 255)) (its mixup_img.astype(np.uint8); the saturation is this
 * project's: a may lie outside [0, 255] after a POST PhotoMetricDistortion, where numpy's cast is undefined).  Pixels at
 * or beyond T (the border of a multi-scale canvas) are not touched.  Only table and the store are read besides img.
 * YUNET_EINVAL, before any launch, for a null pointer, N < 1, M < 1, D outside [1, YUNET_AUG_MAX_EDGE / 2], E outside
 * [1, YUNET_AUG_MAX_EDGE], a non-finite pad_val or more than 2^31 - 1 workgroups (N * ceil(E * E / 256)).  A table row
 * that is not the decide's (partner outside [0, M), J, rw, rh below 1) leaves its image alone. */
int yunet_aug_mixup_pixels(const double* table, int D, float pad_val, int N, int E, const int32_t* params, int M,
                           const uint8_t* store, const long long* store_off, const int32_t* store_hw, float* img,
                           void* stream);

/* The TEST pipeline of a batch (test_pipeline.DeviceTestPipeline; csrc/test_pipeline.hip), one launch: decoded uint8
 * HWC sources addressed as for yunet_aug_pixels (src, src_off [N], src_hw [N,2]) -> out_img [N, 3, Hc, Wc] fp32 planar.
 * table [N,4] int32 (device, written by the host) = (nh, nw, flip, 0) per image.  Inside the top-left nh x nw corner:
 * cv2.resize(uint8, INTER_LINEAR) of the source to nw x nh in OpenCV's 11-bit fixed point (same size: copy; exactly
 * 2 x down in both directions: (a + b + c + d + 2) >> 2), column nw - 1 - x when flip != 0, as fp32; everywhere else
 * 0.0f.  The corner is clipped to the canvas; an image with a non-positive size writes zeros.  Every source index is
 * clamped into the image's own src_hw.  1 <= N <= 65535, 1 <= Hc, 4 <= Wc <= YUNET_AUG_MAX_EDGE, Wc % 4 == 0,
 * out_img 16-byte aligned; otherwise YUNET_EINVAL and nothing is launched. */
int yunet_test_pixels(const uint8_t* src, const long long* src_off, const int32_t* src_hw, const int32_t* table, int N,
                      int Hc, int Wc, float* out_img, void* stream);
/* get_bboxes(rescale=True) for a batch, in place: dets [N, max_out, 5] rows r < count[n]: columns 0..3 divided by
 * scale_factor[n][0..3]; kps [N, max_out, 10] (or NULL): x by scale_factor[n][0], y by scale_factor[n][1] -- the
 * correctly rounded fp32 division.  scale_factor [N,4] fp32 on the device. */
int yunet_rescale_dets(float* dets, float* kps, const int32_t* count, const float* scale_factor, int N, int max_out,
                       void* stream);

/* ---- scoring a detection set (evaluation.py with device=...; csrc/score.hip) ------------------------------------------
 * The integer stages of the two protocols; every table is device memory, offsets are int64 [I + 1] (exclusive scans of
 * the per-image row counts, checked on the device against the totals P / G / D before they address anything).
 * Totals above INT_MAX, a negative count or a missing pointer: YUNET_EINVAL, nothing launched.
 *
 * yunet_score_wider: widerface.py norm_score + image_eval + img_pr_info summed over the images.
 *   pred [P,5] fp64 x y w h score, gt [G,4] fp64 x y w h, gt_bits [G] (bit s: the box is in subset s = easy, medium,
 *   hard), thr [n_thr] fp64 the score thresholds in non-increasing order (1 <= n_thr <= YUNET_SCORE_MAX_THRESH).
 *   minmax [2] <- min(2.0, scores), max(-1.0, scores) (the reference's starting values); a row's score is
 *   (s - min) / (max - min) in fp64.  Per prediction the fp64 inclusive-pixel IoU against every box of its image, best =
 *   first index of the maximum, hit = IoU >= iou_thresh; a row is its box's first hit when no earlier row of the image
 *   hit that box.  counts [3, n_thr, 2] uint64 <- sum over the images that have predictions and boxes of
 *   (cumsum(proposal_s)[last], cumsum(first_s)[last]), last = the LAST row index whose score passes thr[t] (nothing is
 *   added when no row does), first_s = hit & in_s(best) & first hit, proposal_s = !(hit & !in_s(best)).
 *   Scratch the caller allocates: best [P] int32, hit [P] uint8, first [G] int32, keys [2] uint64.
 * yunet_score_wider_match: the matching stage alone (best, hit and first as above). */
#define YUNET_SCORE_BLOCK 256       /* threads of a scoring workgroup = rows of a prediction tile */
#define YUNET_SCORE_GT_CHUNK 256    /* ground truths staged in LDS at a time (any count per image) */
#define YUNET_SCORE_MAX_THRESH 1024
int yunet_score_wider(const double* pred, const long long* pred_off, const double* gt, const long long* gt_off,
                      const uint8_t* gt_bits, int I, long long P, long long G, double iou_thresh, const double* thr,
                      int n_thr, int32_t* best, uint8_t* hit, int32_t* first, unsigned long long* keys,
                      unsigned long long* counts, double* minmax, void* stream);
int yunet_score_wider_match(const double* pred, const long long* pred_off, const double* gt, const long long* gt_off,
                            int I, long long P, long long G, double iou_thresh, int32_t* best, uint8_t* hit,
                            int32_t* first, void* stream);
/* yunet_score_map_tpfp: mean_ap.py tpfp_default for one class without area ranges.  dets [D,5] fp32 x1 y1 x2 y2 score;
 * per image its kept boxes followed by its ignored ones in gts [G,4] fp32 (gt_off), kept [I] int32 the kept count;
 * order [D] int32: per image, the row (relative to the image) visited k-th.  fp32 IoU (no +1, union >= 1e-6f), first
 * index of the maximum over kept and ignored boxes together; a best IoU below iou_thr: fp; a best box that is ignored:
 * neither; the first visit of a kept box: tp, a later one: fp; an image with no box at all: fp for every row.
 * tp, fp [D] fp32 in row order.  Scratch: code [D] int32, first [G] int32. */
int yunet_score_map_tpfp(const float* dets, const long long* det_off, const float* gts, const long long* gt_off,
                         const int32_t* kept, const int32_t* order, int I, long long D, long long G, float iou_thr,
                         int32_t* code, int32_t* first, float* tp, float* fp, void* stream);
/* The ranking and the curve of that protocol (evaluation.eval_map_single_class(rank='device')).  A score ranks by an
 * order-preserving integer key of its fp32 bits: descending score, ties in row order -- np.argsort(-s, kind='stable')
 * for finite scores (-0.0 and NaN are not supported: -0.0 ranks after +0.0, a NaN by its bit pattern).
 * yunet_score_rank_images: order [D] int32 as yunet_score_map_tpfp takes it: per image (det_off), entry k is the local
 *   row visited k-th.  One workgroup per image; up to YUNET_RANK_SEG_CAP rows the image's keys sit in LDS at once,
 *   longer images pass through it in chunks of that size.  Entries of an image whose offsets are not sane stay -1.
 * yunet_score_rank_global: rank [D] int32, the same order over all D rows (ties: image, then row), by a least-
 *   significant-digit radix sort of (key, row) pairs in tiles of YUNET_RANK_RADIX_TILE; the result is the same on
 *   every run.  scratch: yunet_score_rank_scratch_bytes(D) bytes, 8-byte aligned (0 for a D the calls refuse).
 * yunet_score_map_curve: tp, fp [D] fp32 in row order (as yunet_score_map_tpfp writes them) and rank -> in ranked
 *   order ctp, cfp [D] = the cumulative counts, summed as integers and converted to fp32; prec = ctp / max(ctp + cfp,
 *   2^-23) in fp32, one rounding per operation; env[k] = max(prec[k ..]).  No atomics.  D >= YUNET_RANK_CURVE_MAX:
 *   YUNET_EINVAL (below it fp32 cumulative sums are exact, so these are numpy's float32 results bit for bit).
 *   scratch: as yunet_score_rank_global (the same buffer serves both calls, one after the other). */
#define YUNET_RANK_SEG_CAP 1024       /* rows of an image ranked in LDS at once */
#define YUNET_RANK_RADIX_TILE 4096    /* elements of a radix-sort / scan tile */
#define YUNET_RANK_CURVE_MAX 16777216
size_t yunet_score_rank_scratch_bytes(long long D);
int yunet_score_rank_images(const float* dets, const long long* det_off, int I, long long D, int32_t* order,
                            void* stream);
int yunet_score_rank_global(const float* dets, long long D, int32_t* rank, void* scratch, void* stream);
int yunet_score_map_curve(const float* tp, const float* fp, const int32_t* rank, long long D, float* ctp, float* cfp,
                          float* prec, float* env, void* scratch, void* stream);

/* Decoded-source store (pipelines.SourceStore).  One launch builds a batch's SourceBatch tables from the store's
 * per-image tables (M images: byte offset, (h, w), first GT row, GT count; boxes [*,4], kps [*,5,3]) and a device
 * index vector idx [N] (repeats allowed, 1 <= N <= 8192): src_off [N], src_hw [N,2], gt_off [N+1] (exclusive scan of
 * the picked counts), boxes [G,4] / kps [G,5,3] packed in order; rows at or beyond g_cap are not written.  An index
 * outside [0, M) picks an empty image. */
int yunet_aug_gather(const int32_t* idx, int N, int M, const long long* store_off, const int32_t* store_hw,
                     const int32_t* store_goff, const int32_t* store_gcnt, const float* store_boxes,
                     const float* store_kps, int g_cap, long long* src_off, int32_t* src_hw, int32_t* gt_off,
                     float* boxes, float* kps, void* stream);
/* From yunet_aug_decide's params [N,8] and src_hw [N,2]: rect [N,4] int32 = (row0, col0, rows, cols), the source
 * pixels yunet_aug_pixels can read -- rows [max(top,0), min(top+cw,h)), cols [max(left,0), min(left+cw,w)), all zero
 * when cw == 0 or the window misses the image -- and win_off [N+1] int64, the exclusive scan of rows * cols * 3
 * (win_off[N] = bytes of the compact window buffer).  One workgroup. */
int yunet_aug_window_plan(const int32_t* params, const int32_t* src_hw, int N, int32_t* rect, long long* win_off,
                          void* stream);
/* Host code: one hipMemcpy2DAsync per non-empty rectangle, from image n of a pinned host store (host_src + src_off[n],
 * uint8 HWC, src_hw[n]) to win + win_off[n] on `stream`.  src_off, src_hw, rect, win_off are HOST arrays (the plan
 * copied back); the plan is checked against the image sizes and win_bytes before the first copy (YUNET_EINVAL). */
int yunet_upload_windows(const uint8_t* host_src, const long long* src_off, const int32_t* src_hw, const int32_t* rect,
                         const long long* win_off, int N, uint8_t* win, long long win_bytes, void* stream);
/* The window buffer of yunet_upload_windows, read by the GPU itself from the pinned host store (host_src, store_bytes:
 * all of it pinned host memory with a device mapping, else YUNET_EINVAL and nothing is launched; 1 <= N <= 8192).
 * src_off, src_hw (the SourceBatch tables), rect and win_off (yunet_aug_window_plan) are DEVICE arrays: no host
 * round trip.  Validated on the device: an image whose rectangle leaves src_hw[n], whose source span leaves
 * [0, store_bytes) or whose destination leaves [0, win_bytes), [win_off[n], win_off[n+1]] or starts before an earlier
 * win_off is neither read nor written, and its YUNET_FETCH_BAD_* bits are OR-ed into *status (device int32, left
 * as it is otherwise).  Non-persistent grid of 48 KiB chunks (image, row band). */
#define YUNET_FETCH_BAD_RECT 1  /* rectangle outside its image (or negative) */
#define YUNET_FETCH_BAD_SRC 2   /* source span outside the store */
#define YUNET_FETCH_BAD_DST 4   /* destination outside win_bytes / its win_off slot, or before an earlier one */
int yunet_fetch_windows(const uint8_t* host_src, long long store_bytes, const long long* src_off, const int32_t* src_hw,
                        const int32_t* rect, const long long* win_off, int N, uint8_t* win, long long win_bytes,
                        int32_t* status, void* stream);

/* ---- custom training hooks (csrc/hooks.hip) -------------------------------------------------------------------------
 * yunet_ema_update: ExpMomentumEMAHook / LinearMomentumEMAHook (mmdet/core/hook/ema.py) over up to
 * YUNET_EMA_MAX_SEGMENTS flat fp32 segments in ONE launch:  ema_i[k] = fma(m, src_i[k], ema_i[k] * keep)  -- the
 * rounding of torch's  ema.mul_(1 - momentum).add_(src, alpha=momentum)  on a ROCm fp32 tensor, with keep =
 * (float)(1 - momentum) and m = (float)momentum formed on the host in double.  src, ema, n are HOST arrays of nseg
 * entries (device pointers, 4-byte aligned; n[i] >= 0, n[i] == 0 allows NULL pointers).  16-byte accesses where
 * src_i and ema_i share their alignment, scalar accesses otherwise.  YUNET_EINVAL (nothing launched) on a bad
 * argument; nothing is launched when every n[i] is 0. */
#define YUNET_EMA_MAX_SEGMENTS 3
int yunet_ema_update(const float* const* src, float* const* ema, const long long* n, int nseg, float keep, float m,
                     void* stream);
/* yunet_box_size_hist: YuNetSampleSizeStatisticsHook's per-batch work on the device.  Box g < counts[n] of image n
 * (boxes [N, Gmax, 4] fp32 xyxy, counts [N] int32, device) falls into bin (w, h) = (trunc(x2 - x1), trunc(y2 - y1))
 * of a persistent grid [(H + 1) x (W + 1)] (row h, column w):  bin_count += 1  and  bin_first = min(bin_first,
 * (iteration << 32) | (n * Gmax + g))  (64-bit integer atomics: the result does not depend on arrival order;
 * bin_first starts at all ones).  totals[YUNET_HIST_TOTAL] counts every box, totals[YUNET_HIST_NOIMG] every image
 * with counts[n] == 0.  A box whose (w, h) lies outside [0, W] x [0, H] (or is NaN) is not binned: it is appended to
 * spill [spill_cap, 2] as (key, fp32 bits of w | fp32 bits of h << 32) at slot totals[YUNET_HIST_SPILLED]++ and
 * YUNET_HIST_SPILL is OR-ed into totals[YUNET_HIST_STATUS]; past spill_cap YUNET_HIST_OVERFLOW is set instead.  A count
 * outside [0, Gmax] is clamped and sets YUNET_HIST_BAD_COUNT.  All int64 arrays are device memory.  YUNET_EINVAL
 * (nothing launched) on NULL pointers, N < 0, Gmax < 1, N * Gmax >= 2^31, W or H outside [0, 65535], iteration
 * outside [0, 2^31), spill_cap < 0 (or spill == NULL with spill_cap > 0).  N == 0 launches nothing. */
#define YUNET_HIST_TOTAL 0
#define YUNET_HIST_NOIMG 1
#define YUNET_HIST_SPILLED 2
#define YUNET_HIST_STATUS 3
#define YUNET_HIST_SPILL 1
#define YUNET_HIST_OVERFLOW 2
#define YUNET_HIST_BAD_COUNT 4
int yunet_box_size_hist(const float* boxes, const int32_t* counts, int N, int Gmax, long long iteration, int W, int H,
                        long long* bin_count, long long* bin_first, long long* totals, long long* spill, int spill_cap,
                        void* stream);

/* Measurement switches of the dispatchers (ABI 6).  The library reads the environment ONCE, the first time an
 * option is needed (YUNET_NO_PACK, YUNET_BWD_FP32MMA, YUNET_BWD64_NW, YUNET_EW_GRID, YUNET_DP_FWD_BLOCKS_PER_CU);
 * after that only this call changes them -- no launch calls getenv.  Names:
 *   "no_pack"            1: the 20x20 / 10x10 levels on per-image tiles instead of the packed canvas
 *   "bwd_fp32mma"        1: every backward GEMM on the exact-fp32 matrix instruction (bench.py: exact_fp32_bwd)
 *   "bwd64_nw"           0 (by shape) | 4 | 8: waves per workgroup of the 64 -> 64 backward kernel
 *   "ew_grid"            workgroup cap of the element-wise backward kernels (0 restores the default, 768)
 *   "fwd_blocks_per_cu"  0 (occupancy API) | 1..4: resident forward workgroups per CU
 *   "fwd64s"             0: every fp32 64 -> 64 forward unit on the tile kernel | 1: the plain and fused-pooling units on
 *                        the wave-streaming kernel | 2 (default): the 20x20 / 10x10 levels too
 *   "fwd64s_rows"        0 (by shape) | rows per band of the wave-streaming kernel
 *   "bwd16s"             1 (default): the fp32 16 -> 16 backward unit on maps >= 32 x 64 on the wave-streaming kernel that
 *                        recomputes z (it does not read YunetDP.z) | 0: the tile kernel;  "bwd16s_rows": rows per band
 *   "fwd16s"             1 (default): the fp32 16 -> 16 / 16 -> 64 forward units on the wave-streaming kernels | 0: the tile kernels
 *   "stem_mma"           1 (default): the fp32 stem (yunet_stem_fwd; YUNET_OP_STEM_BWD with the stem's parameters in p[4],
 *                        p[5] -> yunet_stem_bwd_rz) as matrix products on the matrix cores | 0: the VALU tile kernels
 *   "bwd32_split"        1 (default): the 32 -> 64 backward unit (YuNet_s) on the split-bf16 matrix path | 0: exact-fp32 MFMA
 *   "upadd_coarse"       1 (default): yunet_upadd_bwd with dxa = NULL on the dedicated coarse-gradient kernel | 0: general kernel
 *   "assign_v2"          1 (default): yunet_assign* on the round-5 launches (compaction per 256-prior chunk, one workgroup per
 *                        (image, GT) pair with a candidate-pruned walk, one wave per conflict; needs Gmax < P, N <= 65535) | 0: one
 *                        workgroup per image for compaction / conflicts, every pair evaluated in full.  Same outputs, bit for bit.
 *   "fwd_group"          1 (default): yunet_dp_fwd_group puts independent plain 64 -> 64 units into one grid | 0: one launch each
 *   "oneshot_timeout_ms" how long yunet_allreduce waits for a peer (default 120 000; env YUNET_ONESHOT_TIMEOUT_MS)
 * "no_pack" and "bwd64_nw" change yunet_dp_bwd_blocks(): set them before any plan is built.
 * Returns the previous value, or YUNET_EINVAL for an unknown name / a value out of range. */
int yunet_set_option(const char* name, int value);

/* ---- gradient / num_pos exchange between the GPUs of one node (csrc/collective.hip) ---------------------
 * Replaces, for this path, what the reference gets from torch DDP over NCCL (mmdet/apis/train.py:152-163:
 * MMDistributedDataParallel averages the ~300 KB of gradients) and from reduce_mean
 * (mmdet/core/utils/dist_utils.py:68-74, called at yunet_head.py:493-497 for num_pos).  The messages are
 * latency-bound and xGMI is a point-to-point mesh, so instead of a ring every rank STORES its message into a
 * slot of every peer's inbox (peer-mapped device memory), raises a flag behind it, waits for the world's flags
 * in its own inbox and adds the slots in rank order: one kernel per rank, results bit-identical on all ranks.
 *
 * These are the only entry points that allocate: an inbox is uncached device memory that peers map through
 * hipIpc* handles (one process per GPU).  Set-up, per rank: yunet_comm_alloc -> yunet_comm_export -> exchange the
 * 64-byte handles over any host channel -> yunet_comm_open on every peer's handle -> fill a YunetComm.
 * Every rank must issue the same sequence of yunet_allreduce calls on a given YunetComm (one YunetComm per stream
 * that carries collectives).  A peer that never arrives makes the wait give up after option "oneshot_timeout_ms"
 * (default 120 000 = 2 min: a step lasts milliseconds, a peer that is two minutes late is gone): yunet_comm_status() then returns the
 * sequence number of that call and the buffer is POISONED with NaN (the shares of the blocks that gave up), so a
 * caller that never reads the status word cannot train on un-reduced gradients unnoticed. */
#define YUNET_MAX_RANKS 8
#define YUNET_IPC_HANDLE_BYTES 64
/* bytes in front of the message slots of an inbox (ABI 11: flags per (parity, rank, piece) + the local send counter;
 * messages above 64 KB travel as 2 / 4 / 8 pieces, one workgroup per peer and piece) */
#define YUNET_COMM_HEADER_BYTES 20480
typedef struct YunetComm {
    int32_t rank, world;
    uint32_t seq;                    /* calls made so far; incremented by yunet_allreduce (start at 0)          */
    int32_t reserved_;
    uint64_t slot_bytes;             /* capacity of one message: (inbox bytes - YUNET_COMM_HEADER_BYTES) / (2 * world) */
    void* inbox[YUNET_MAX_RANKS];    /* inbox of rank r as mapped into THIS process (own rank: the allocation) */
    int32_t* status;                 /* HOST word from yunet_comm_alloc                                        */
} YunetComm;
size_t yunet_comm_inbox_bytes(int world, size_t max_msg_bytes);
int yunet_comm_alloc(size_t bytes, void** inbox, int32_t** status);
int yunet_comm_free(void* inbox, int32_t* status);
int yunet_comm_export(void* inbox, void* handle64 /* HOST, YUNET_IPC_HANDLE_BYTES */);
int yunet_comm_open(const void* handle64 /* HOST */, void** mapped);
int yunet_comm_close(void* mapped);
/* buf[0..n) <- sum over ranks (mean != 0: divided by world), in place, n * 4 <= slot_bytes. */
int yunet_allreduce(YunetComm* c /* HOST */, float* buf, size_t n, int mean, void* stream);
int yunet_comm_status(const YunetComm* c /* HOST */);

int yunet_abi_version(void);
/* grid size the fused conv kernels are launched with (rows of wgrad_partials). */
int yunet_conv_blocks(void);

#ifdef __cplusplus
}
#endif
#endif /* YUNET_HIP_H */
