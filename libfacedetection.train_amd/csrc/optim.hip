// optim.hip -- the optimizer surface beyond the default single-group SGD of api.hip: the norm of the flat gradient with
// torch's clip coefficient (clip_grad_norm_), and the SGD / Adam / AdamW updates over parameter groups.
//
// Groups: a byte per element of the flat buffer names its group, a table of YUNET_OPT_ROW doubles per group carries
// {lr, weight_decay, momentum | beta1, beta2}.  Doubles because torch derives 1 - beta, 1 - lr*wd and the bias corrections
// from python floats: 1 - 0.999f is 6e-5 away from 1 - 0.999, far more than the update's fp32 rounding.  Every block turns
// the rows into the fp32 constants torch hands its kernels once (thread t = group t: one load per thread, no loop) and
// keeps them in LDS; the elements are one per thread like sgd_kernel, so a group boundary may fall anywhere.
// The byte YUNET_OPT_FROZEN is no group: such an element is left alone -- parameter and state keep their bytes.
//
// Gradient accumulation (yunet_grad_accum): SAVE copies the flat gradient aside in front of a backward, ADD puts the saved
// total back on top of what the backward wrote -- one fp32 add per element, no multiply near it, no atomics.
#include "common.h"

namespace {

constexpr int NT = YUNET_NORM_BLOCK;                      // threads per block of every kernel here
constexpr int VPT = YUNET_NORM_TILE / (4 * NT);           // float4 per thread and tile
static_assert(VPT * 4 * NT == YUNET_NORM_TILE, "tile = whole float4 per thread");
static_assert(YUNET_NORM_MAX_BLOCKS <= NT, "the last block folds one partial per thread");
static_assert(YUNET_OPT_MAX_GROUPS <= NT, "one thread per group row");
static_assert(YUNET_OPT_FROZEN >= YUNET_OPT_MAX_GROUPS && YUNET_OPT_FROZEN <= 255, "the frozen byte is no group id");

struct NormScratch {
    unsigned int arrived;                                 // ticket counter: zero between launches
    unsigned int pad_;
    double partial[YUNET_NORM_MAX_BLOCKS];
};
static_assert(sizeof(NormScratch) == YUNET_NORM_SCRATCH_BYTES, "yunet_hip.h");

template <int MODE> __device__ __forceinline__ double fold(double a, double b) {
    return MODE == YUNET_NORM_INF ? (b != b ? b : (a != a ? a : (a > b ? a : b))) : a + b;      // max carries NaN like torch
}

template <int MODE> __device__ __forceinline__ double term(float g, float gscale) {
    const float x = g * gscale;                           // the element torch would see after grad.mul_(1 / loss_scale)
    return MODE == YUNET_NORM_L2 ? (double)x * (double)x : (double)fabsf(x);
}

// fixed order: lanes by halving distance, waves in index order through LDS; every thread returns the block's value
template <int MODE> __device__ __forceinline__ double block_fold(double v, double* lds) {
    for (int d = 32; d > 0; d >>= 1) v = fold<MODE>(v, __shfl_down(v, d, 64));
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                      // lds may still be read from the previous use
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    double r = lds[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = fold<MODE>(r, lds[w]);
    return r;
}

// ||grad * gscale||_p and min(1, max_norm / (norm + 1e-6)) in ONE launch, no float atomics: every block folds its tiles
// in fp64 and publishes one partial; the block that draws the last ticket folds the partials in index order, writes the
// two floats and puts the ticket counter back to zero, so the next launch needs no memset.  The result depends on n and
// the grid only (VEC only changes how the same elements are fetched).
template <int MODE, bool VEC>
__global__ __launch_bounds__(NT) void grad_norm_kernel(const float* __restrict__ g, long long n, float gscale,
                                                       float max_norm, NormScratch* __restrict__ scratch,
                                                       float* __restrict__ out) {
    __shared__ double lds[NT / 64 + 1];
    double acc = 0.0;
    const long long ntiles = (n + YUNET_NORM_TILE - 1) / YUNET_NORM_TILE;
    // a trip issues VPT independent 16-byte loads before it consumes any (tests/test_isa_guard.py's rule)
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long base = tile * YUNET_NORM_TILE + (long long)threadIdx.x * 4;
        float4 v[VPT];
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const long long e = base + (long long)k * (4 * NT);
            if (VEC && e + 3 < n) {
                v[k] = *reinterpret_cast<const float4*>(g + e);
            } else {
                v[k].x = e < n ? g[e] : 0.0f;
                v[k].y = e + 1 < n ? g[e + 1] : 0.0f;
                v[k].z = e + 2 < n ? g[e + 2] : 0.0f;
                v[k].w = e + 3 < n ? g[e + 3] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            acc = fold<MODE>(acc, term<MODE>(v[k].x, gscale));
            acc = fold<MODE>(acc, term<MODE>(v[k].y, gscale));
            acc = fold<MODE>(acc, term<MODE>(v[k].z, gscale));
            acc = fold<MODE>(acc, term<MODE>(v[k].w, gscale));
        }
    }
    const double mine = block_fold<MODE>(acc, lds);
    // publish: partial -> drained -> agent release -> ticket; the last arriver acquires before it reads the partials
    if (threadIdx.x == 0) {
        scratch->partial[blockIdx.x] = mine;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int t = __hip_atomic_fetch_add(&scratch->arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        lds[NT / 64] = last ? 1.0 : 0.0;
    }
    __syncthreads();
    if (lds[NT / 64] == 0.0) return;
    const double part = threadIdx.x < gridDim.x
                            ? __hip_atomic_load(&scratch->partial[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                            : 0.0;
    const double total = block_fold<MODE>(part, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)(MODE == YUNET_NORM_L2 ? sqrt(total) : total);
        const float c = max_norm / (norm + 1e-6f);        // torch/nn/utils/clip_grad.py
        out[0] = norm;
        out[1] = c > 1.0f ? 1.0f : c;                      // clamp(max=1); NaN stays NaN
        __hip_atomic_store(&scratch->arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ int group_of(const unsigned char* __restrict__ gid, long long i, int ngroups) {
    const int k = gid[i];
    return k < ngroups ? k : ngroups - 1;                 // a byte past the table must not read past it
}

__device__ __forceinline__ float clip_scale(float gscale, const float* __restrict__ coef) {
    return coef ? gscale * coef[0] : gscale;
}

// sgd_kernel (api.hip) with lr / weight decay / momentum per group; the expressions are the same ones, so one group
// and no clipping gives the same bits
__global__ __launch_bounds__(NT) void sgd_grouped_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ buf, long long n,
                                                         const unsigned char* __restrict__ gid,
                                                         const double* __restrict__ table, int ngroups, float undamped,
                                                         int nesterov, float gscale_in, const float* __restrict__ coef,
                                                         int first) {
    __shared__ float4 row[YUNET_OPT_MAX_GROUPS];
    if ((int)threadIdx.x < ngroups) {
        const double* t = table + (long long)threadIdx.x * YUNET_OPT_ROW;
        row[threadIdx.x] = make_float4((float)t[0], (float)t[1], (float)t[2], 0.0f);
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n || gid[i] == YUNET_OPT_FROZEN) return;      // frozen: no load of p / g / buf, no store
    const float4 r = row[group_of(gid, i, ngroups)];
    const float lr = r.x, wd = r.y, momentum = r.z;
    const float gscale = clip_scale(gscale_in, coef);
    const float w = p[i];
    const float d = g[i] * gscale + wd * w;
    float step = d;
    if (momentum != 0.0f) {
        const float b = first ? d : buf[i] * momentum + undamped * d;
        buf[i] = b;
        step = nesterov ? d + momentum * b : b;
    }
    p[i] = w - lr * step;
}

struct AdamRow {
    float keep;            // 1 - lr * wd (AdamW's p *= ...), 1 where it does not apply
    float wd;              // coupled L2 (Adam), 0 where it does not apply
    float beta2, omb1, omb2;
    float step_size;       // lr / (1 - beta1^step)
    float bc2_sqrt;        // sqrt(1 - beta2^step)
    float pad_;
};

__device__ __forceinline__ double ipow(double b, int e) {
    double r = 1.0;
    for (; e > 0; e >>= 1, b *= b)
        if (e & 1) r *= b;
    return r;
}

// torch/optim/adam.py _single_tensor_adam (not capturable, no amsgrad, no maximize), operation by operation
__global__ __launch_bounds__(NT) void adam_grouped_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                          long long n, const unsigned char* __restrict__ gid,
                                                          const double* __restrict__ table, int ngroups, float eps,
                                                          int decoupled, int step, float gscale_in,
                                                          const float* __restrict__ coef) {
    __shared__ AdamRow row[YUNET_OPT_MAX_GROUPS];
    if ((int)threadIdx.x < ngroups) {
        const double* t = table + (long long)threadIdx.x * YUNET_OPT_ROW;
        const double lr = t[0], wd = t[1], b1 = t[2], b2 = t[3];
        AdamRow r;
        r.keep = (decoupled && wd != 0.0) ? (float)(1.0 - lr * wd) : 1.0f;
        r.wd = decoupled ? 0.0f : (float)wd;
        r.beta2 = (float)b2;
        r.omb1 = (float)(1.0 - b1);
        r.omb2 = (float)(1.0 - b2);
        r.step_size = (float)(lr / (1.0 - ipow(b1, step)));
        r.bc2_sqrt = (float)sqrt(1.0 - ipow(b2, step));
        r.pad_ = 0.0f;
        row[threadIdx.x] = r;
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n || gid[i] == YUNET_OPT_FROZEN) return;      // frozen: parameter and both moments keep their bytes
    const AdamRow r = row[group_of(gid, i, ngroups)];
    const float gscale = clip_scale(gscale_in, coef);
    float w = p[i];
    float d = g[i] * gscale;
    if (r.wd != 0.0f) d = d + r.wd * w;                    // grad.add(param, alpha=weight_decay)
    w = w * r.keep;                                        // param.mul_(1 - lr * weight_decay)
    float m = exp_avg[i], v = exp_avg_sq[i];
    m = m + r.omb1 * (d - m);                              // exp_avg.lerp_(grad, 1 - beta1)
    v = v * r.beta2 + r.omb2 * d * d;                      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    exp_avg[i] = m;
    exp_avg_sq[i] = v;
    const float denom = sqrtf(v) / r.bc2_sqrt + eps;
    p[i] = w - r.step_size * (m / denom);                  // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// One unit per thread, no loop: a float4 of the 16-byte aligned body [head, head + 4 * nvec), and -- the first three threads
// at most -- one element of the scalar head [0, head) and one of the scalar tail [head + 4 * nvec, n).  The host picks
// `head` so that grad + head is 16-byte aligned and takes nvec = 0 (everything scalar, one element per thread) when
// acc + head is not.  ADD is one fp32 add per element (v_pk_add_f32 over the pairs of a float4, v_add_f32 in the scalar
// parts) with no multiply to contract with: NaN / Inf propagate, -0 + -0 stays -0.
template <int MODE>
__global__ __launch_bounds__(NT) void grad_accum_kernel(float* __restrict__ acc, float* __restrict__ g, long long n,
                                                        int head, long long nvec, int scalar) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t < nvec) {
        float4* gp = reinterpret_cast<float4*>(g + head) + t;
        float4* ap = reinterpret_cast<float4*>(acc + head) + t;
        if (MODE == YUNET_ACCUM_SAVE) {
            *ap = *gp;
        } else {
            const float4 a = *ap, b = *gp;
            *gp = make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
        }
    }
    if (scalar) {                                         // no 16-byte body: element t
        if (t < n) {
            if (MODE == YUNET_ACCUM_SAVE) acc[t] = g[t];
            else g[t] = __fadd_rn(acc[t], g[t]);
        }
        return;
    }
    const long long tail0 = head + 4 * nvec;
    long long e = -1;
    if (t < head) e = t;                                  // head and tail are at most 3 elements each: threads 0..2 take
    else if (t >= 4 && t - 4 < n - tail0) e = tail0 + (t - 4);      // the head, threads 4..6 the tail (the same wave)
    if (e >= 0) {
        if (MODE == YUNET_ACCUM_SAVE) acc[e] = g[e];
        else g[e] = __fadd_rn(acc[e], g[e]);
    }
}

template <int MODE>
void launch_norm(bool vec, unsigned blocks, hipStream_t s, const float* g, long long n, float gscale, float max_norm,
                 NormScratch* scratch, float* out) {
    if (vec)
        hipLaunchKernelGGL((grad_norm_kernel<MODE, true>), dim3(blocks), dim3(NT), 0, s, g, n, gscale, max_norm, scratch, out);
    else
        hipLaunchKernelGGL((grad_norm_kernel<MODE, false>), dim3(blocks), dim3(NT), 0, s, g, n, gscale, max_norm, scratch, out);
}

bool grouped_args_ok(const void* p, const void* g, int64_t n, const void* gid, const void* table, int ngroups) {
    return p && g && gid && table && n >= 1 && ngroups >= 1 && ngroups <= YUNET_OPT_MAX_GROUPS &&
           (n + NT - 1) / NT <= 0x7fffffffll;
}

}  // namespace

extern "C" int yunet_grad_norm(const float* grads, int64_t n, float grad_scale, int norm_type, float max_norm,
                               void* scratch, float* out, void* stream) {
    if (!grads || !scratch || !out || n < 1) return YUNET_EINVAL;
    if ((reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(grads) & 3)) return YUNET_EINVAL;
    const long long tiles = (n + YUNET_NORM_TILE - 1) / YUNET_NORM_TILE;
    const unsigned blocks = (unsigned)(tiles < YUNET_NORM_MAX_BLOCKS ? tiles : YUNET_NORM_MAX_BLOCKS);
    const bool vec = (reinterpret_cast<uintptr_t>(grads) & 15) == 0;
    NormScratch* sc = static_cast<NormScratch*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    switch (norm_type) {
        case YUNET_NORM_L2: launch_norm<YUNET_NORM_L2>(vec, blocks, s, grads, n, grad_scale, max_norm, sc, out); break;
        case YUNET_NORM_L1: launch_norm<YUNET_NORM_L1>(vec, blocks, s, grads, n, grad_scale, max_norm, sc, out); break;
        case YUNET_NORM_INF: launch_norm<YUNET_NORM_INF>(vec, blocks, s, grads, n, grad_scale, max_norm, sc, out); break;
        default: return YUNET_EINVAL;
    }
    return hip_status();
}

extern "C" int yunet_sgd_step_grouped(float* params, const float* grads, float* momentum_buf, int64_t n,
                                      const uint8_t* group_of_elem, const double* table, int n_groups, float dampening,
                                      int nesterov, float grad_scale, const float* clip_coef, int first_step,
                                      void* stream) {
    if (!grouped_args_ok(params, grads, n, group_of_elem, table, n_groups) || !momentum_buf) return YUNET_EINVAL;
    if (nesterov && dampening != 0.0f) return YUNET_EINVAL;
    const unsigned blocks = (unsigned)((n + NT - 1) / NT);
    hipLaunchKernelGGL(sgd_grouped_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, params, grads, momentum_buf,
                       (long long)n, group_of_elem, table, n_groups, 1.0f - dampening, nesterov ? 1 : 0, grad_scale,
                       clip_coef, first_step);
    return hip_status();
}

extern "C" int yunet_adam_step_grouped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                       const uint8_t* group_of_elem, const double* table, int n_groups, float eps,
                                       int decoupled, int step, float grad_scale, const float* clip_coef,
                                       void* stream) {
    if (!grouped_args_ok(params, grads, n, group_of_elem, table, n_groups) || !exp_avg || !exp_avg_sq || step < 1)
        return YUNET_EINVAL;
    const unsigned blocks = (unsigned)((n + NT - 1) / NT);
    hipLaunchKernelGGL(adam_grouped_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, params, grads, exp_avg,
                       exp_avg_sq, (long long)n, group_of_elem, table, n_groups, eps, decoupled ? 1 : 0, step,
                       grad_scale, clip_coef);
    return hip_status();
}

extern "C" int yunet_grad_accum(float* acc, float* grads, int64_t n, int mode, void* stream) {
    if (n < 0 || (mode != YUNET_ACCUM_SAVE && mode != YUNET_ACCUM_ADD)) return YUNET_EINVAL;
    if (n == 0) return 0;
    if (!acc || !grads || (reinterpret_cast<uintptr_t>(acc) & 3) || (reinterpret_cast<uintptr_t>(grads) & 3)) return YUNET_EINVAL;
    // elements in front of the first 16-byte boundary of grads; acc must reach a boundary with the same count
    long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(grads) & 15)) & 15) / 4;
    if (head > n) head = n;
    const bool vec = ((reinterpret_cast<uintptr_t>(acc) + 4 * (uintptr_t)head) & 15) == 0;
    const long long nvec = vec ? (n - head) / 4 : 0;
    long long threads = vec ? nvec : n;
    if (threads < 8) threads = 8;                          // threads 0..2 and 4..6 carry the head and the tail
    const long long blocks = (threads + NT - 1) / NT;
    if (blocks > 0x7fffffffll) return YUNET_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (mode == YUNET_ACCUM_SAVE)
        hipLaunchKernelGGL((grad_accum_kernel<YUNET_ACCUM_SAVE>), dim3((unsigned)blocks), dim3(NT), 0, s, acc, grads,
                           (long long)n, (int)head, nvec, vec ? 0 : 1);
    else
        hipLaunchKernelGGL((grad_accum_kernel<YUNET_ACCUM_ADD>), dim3((unsigned)blocks), dim3(NT), 0, s, acc, grads,
                           (long long)n, (int)head, nvec, vec ? 0 : 1);
    return hip_status();
}
