// dp_route.h -- which kernel instance runs a ConvDPUnit: one rule per direction.  yunet_dp_fwd / yunet_dp_bwd (conv_fwd.hip,
// conv_bwd.hip) compute the route and map it to its instance, yunet_dp_fwd_group and yunet_dp_bwd_reads_z ask it, and
// yunet_dp_route (conv_bwd_host.hip) tells a caller the instance by name.  The rules read the descriptor and
// yunet_options() only: no HIP call, no allocation.  Tile sizes and grids come from bwd_grid.h and common.h.
#pragma once
#include "bwd_grid.h"

enum { DP_NONE = 0, DP_TILE, DP_FWD16S, DP_FWD64S, DP_BWD16S, DP_BWD64 };
struct DpRoute {
    int family;              // DP_*; DP_NONE until the rule has chosen
    int cin, cout, th, tw;   // DP_TILE (DP_FWD16S: cout)
    bool packed;             // DP_TILE, DP_BWD64: the packed canvas of the small levels
    bool pool;               // forward: fused pooling (POOL); backward: dy is the pooled gradient (POOLDY)
    int gemm;                // backward DP_TILE: 1 = split-bf16 GEMMs, 0 = exact fp32
    bool full;               // backward DP_TILE: the whole-tile instance
    bool det;                // the instance that writes its BatchNorm sums into order-fixed rows
    int nw;                  // DP_BWD64: waves per workgroup
};

// The tile instances that exist, each written once: the dispatchers instantiate exactly these, and a route to any other is
// refused.  Forward X(cin, cout, th, tw, packed, pool, det_too): det_too = 0 where there is no DET instance (the 64 -> 16 heads).
#define DP_FWD_TILE_INSTANCES(X)                                                                          \
    X(16, 16, 16, 32, false, true, 1) X(32, 64, 8, 16, false, true, 1) X(64, 64, 8, 16, false, true, 1)   \
    X(16, 16, 16, 32, false, false, 1) X(64, 64, 8, 16, true, false, 1) X(64, 16, 8, 16, true, false, 0)  \
    X(16, 16, 8, 16, false, false, 1) X(16, 32, 8, 16, false, false, 1) X(16, 64, 8, 16, false, false, 1) \
    X(32, 32, 8, 16, false, false, 1) X(32, 64, 8, 16, false, false, 1) X(64, 64, 8, 16, false, false, 1) \
    X(64, 16, 8, 16, false, false, 0)
// Backward X(cin, cout, th, tw, packed, gemm, pooldy, full_too): full_too = 1 where the whole-tile twin exists as well.  With
// fp32 storage every one has its DET twin, with bf16 storage none.
#define DP_BWD_TILE_INSTANCES(X)                                                                                \
    X(16, 16, 16, 32, false, 0, true, 1) X(32, 64, 8, 16, false, 1, true, 1) X(32, 64, 8, 16, false, 0, true, 1) \
    X(64, 64, 8, 16, false, 0, true, 0) X(16, 16, 16, 32, false, 0, false, 1) X(64, 64, 8, 16, true, 0, false, 0) \
    X(64, 16, 8, 16, true, 0, false, 0) X(32, 64, 8, 16, false, 1, false, 1) X(16, 16, 8, 16, false, 0, false, 0) \
    X(16, 32, 8, 16, false, 0, false, 1) X(16, 64, 8, 16, false, 0, false, 1) X(32, 32, 8, 16, false, 0, false, 1) \
    X(32, 64, 8, 16, false, 0, false, 0) X(64, 64, 8, 16, false, 0, false, 0) X(64, 16, 8, 16, false, 0, false, 0)
#define DP_FWD_IS(r, ci, co, th_, pk, pl) ((r).cin == ci && (r).cout == co && (r).th == th_ && (r).packed == pk && (r).pool == pl)
#define DP_BWD_IS(r, ci, co, th_, pk, g, pl) (DP_FWD_IS(r, ci, co, th_, pk, pl) && (r).gemm == g)
static inline bool dp_fwd_tile_exists(const DpRoute& r) {
#define X(ci, co, th_, tw_, pk, pl, dt) if (DP_FWD_IS(r, ci, co, th_, pk, pl)) return !r.det || dt;
    DP_FWD_TILE_INSTANCES(X)
#undef X
    return false;
}
static inline bool dp_bwd_tile_exists(const DpRoute& r) {
#define X(ci, co, th_, tw_, pk, g, pl, ft) if (DP_BWD_IS(r, ci, co, th_, pk, g, pl)) return !r.full || ft;
    DP_BWD_TILE_INSTANCES(X)
#undef X
    return false;
}
static inline bool dp_ptr_aligned4(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 3); }

// The three levels are one rule: `plain` (YunetBN.det_rows = R) keeps the choice inside the tile family with exact-fp32
// GEMMs and no whole-tile instance; the fast level (R | YUNET_DET_FAST, fp32 storage) is the default choice with det set.
// act_dtype: the storage build that would launch (YUNET_F32 | YUNET_BF16).
static inline int dp_fwd_route(const YunetDP* d, int act_dtype, DpRoute* r) {
    *r = DpRoute{};
    if (d->x_dtype != act_dtype) return YUNET_EINVAL;
    if (d->z_dtype != act_dtype && !(d->cout == 16 && d->z_dtype == YUNET_F32)) return YUNET_EINVAL;   // (the heads: fp32 z)
    if (d->in_transform != YUNET_T_IDENTITY && d->in_transform != YUNET_T_BNRELU) return YUNET_EINVAL;
    const YunetOptions& o = yunet_options();
    const bool act_z = d->z_dtype == act_dtype;
    r->det = d->out_has_bn && YUNET_DET_ROWS(d->out_bn.det_rows);
    const bool plain = r->det && !bn_det_fast(d->out_bn);
    r->pool = d->pool_out != nullptr;
    const bool pool_ok = r->pool && yunet_dp_pool_fusion_ok(d->N, d->H, d->W, d->cin, d->cout) &&
                         d->out_bn.gamma && d->pool_idx && dp_ptr_aligned4(d->pool_idx);      // (out_has_bn may be 0: eval())
    // fp32 storage only, and never a head
    const bool det_ok = !r->det || (act_dtype == YUNET_F32 && act_z && d->out_bn.stats);
    r->cin = d->cin, r->cout = d->cout;
    // 16 input channels: the wave-streaming kernel (conv_fwd16.hip); any prof keeps a unit off it, a head never streams.
    // A null z (include/yunet_hip.h): the pooled 16 -> 16 unit on that kernel alone; every other kernel stores through it
    if (!plain && d->cin == 16 && (d->cout == 16 ? (!r->pool || pool_ok) : (d->cout == 64 && !r->pool)) && act_z && !d->prof &&
        o.fwd16s) {
        r->family = DP_FWD16S;
        return det_ok && (d->z || r->pool) ? 0 : YUNET_EINVAL;
    }
    if (!d->z || !det_ok || (r->pool && !pool_ok)) return YUNET_EINVAL;
    const bool pack = dp_use_pack(d->N, d->H, d->W, d->cin, d->cout);
    // 64 -> 64: the wave-streaming kernel (conv_fwd64.hip), on the packed levels from fwd64s = 2; the phase-clock debug mode
    // (prof = a pointer; ablation masks are below 64) stays on the tile kernel
    if (!plain && d->cin == 64 && d->cout == 64 && act_z && (unsigned long long)d->prof < 64ull && o.fwd64s &&
        (r->pool || !(pack && o.fwd64s < 2))) {
        r->family = DP_FWD64S;
        return 0;
    }
    r->family = DP_TILE;
    const bool big = d->cin == 16 && d->cout == 16 && d->W >= 64 && d->H >= 32;   // 160x160 / 80x80 levels (pooled: always)
    r->th = big ? 16 : 8, r->tw = big ? 32 : 16;
    // 20x20 / 10x10 levels: packed canvas (in the default mode a phase-clock run under fwd64s = 2 is on per-image tiles)
    r->packed = !r->pool && pack && !(d->cout == 64 && !r->det && act_z && o.fwd64s >= 2);
    return dp_fwd_tile_exists(*r) ? 0 : YUNET_EINVAL;
}
// yunet_dp_fwd_group launches its units as one grid where every one of them, on its own, takes the plain non-deterministic
// 64 -> 64 wave-streaming instance and carries no prof of any kind (an ablation mask runs on that kernel alone, not in the
// grouped one); otherwise they go out one after the other.
static inline bool dp_fwd_one_grid(const YunetDP* const* units, int n, int act_dtype) {
    bool one_grid = units && n >= 2 && n <= YUNET_DP_GROUP_MAX && yunet_options().fwd_group != 0;
    for (int i = 0; i < n && one_grid; ++i) {
        DpRoute r;
        one_grid = units[i] && !units[i]->prof && dp_fwd_route(units[i], act_dtype, &r) == 0 && r.family == DP_FWD64S &&
                   !r.pool && !r.det;
    }
    return one_grid;
}

// a launch that produces the producer's BN-backward sums into order-fixed rows
static inline bool dp_bwd_det(const YunetDP* d) {
    return d->in_transform == YUNET_T_BNRELU && d->dx && d->in_bn.bstats && YUNET_DET_ROWS(d->in_bn.det_rows);
}
// The family is chosen before anything is refused (r->family says so even where the return value is YUNET_EINVAL), so that
// yunet_dp_bwd_reads_z answers for a descriptor whose buffers are not bound yet.
static inline int dp_bwd_route(const YunetDP* d, int act_dtype, DpRoute* r) {
    *r = DpRoute{};
    const YunetOptions& o = yunet_options();
    r->det = dp_bwd_det(d);
    const bool plain = r->det && !(bn_det_fast(d->in_bn) && act_dtype == YUNET_F32);
    r->pool = d->pool_idx != nullptr;
    r->cin = d->cin, r->cout = d->cout;
    const bool big = dp_bwd_big_tile(d->H, d->W, d->cin, d->cout);
    // The 16 -> 16 unit on a big-tile map, followed by BatchNorm, with a plain (non-accumulating) dx, outside the phase-clock
    // debug mode: the wave-streaming kernel (conv_bwd16.hip), which recomputes z from x and never reads YunetDP.z
    if (!plain && big && d->out_has_bn && d->dx && !d->accumulate_dx && !d->prof && o.bwd16s &&
        (!r->pool || (yunet_dp_pool_fusion_ok(d->N, d->H, d->W, 16, 16) && dp_ptr_aligned4(d->pool_idx))))
        r->family = DP_BWD16S;
    if (d->x_dtype != act_dtype) return YUNET_EINVAL;
    if (!d->wgrad_partials || d->wgrad_blocks != yunet_dp_bwd_blocks(d->N, d->H, d->W, d->cin, d->cout))
        return YUNET_EINVAL;   // the partial buffer must have exactly the rows the grid writes
    if (d->in_transform != YUNET_T_IDENTITY && d->in_transform != YUNET_T_BNRELU) return YUNET_EINVAL;
    if (r->det && act_dtype != YUNET_F32) return YUNET_EINVAL;
    if (r->family == DP_BWD16S) return 0;
    if (!d->z) return YUNET_EINVAL;      // a null z: only where the kernel recomputes it
    // dy is the pooled gradient + argmax bytes (max_pool2d backward while staging)
    if (r->pool && (!yunet_dp_pool_fusion_ok(d->N, d->H, d->W, d->cin, d->cout) || !d->out_has_bn)) return YUNET_EINVAL;
    r->packed = !r->pool && dp_use_pack_bwd(d->N, d->H, d->W, d->cin, d->cout);      // 20x20 / 10x10 levels
    // exact-fp32 GEMMs (option bwd_fp32mma, the plain deterministic level): no dp_bwd64, no split-bf16 32 -> 64
    const bool exact = o.bwd_fp32mma != 0 || plain;
    if (d->cin == 64 && d->cout == 64 && !exact) {
        r->family = DP_BWD64;
        r->nw = bwd64_nw(d->N, d->H, d->W);      // (also the rows of wgrad_partials: yunet_dp_bwd_blocks)
        return 0;
    }
    r->family = DP_TILE;
    r->th = big ? 16 : 8, r->tw = big ? 32 : 16;
    r->gemm = d->cin == 32 && d->cout == 64 && !exact && o.bwd32_split;
    // the whole-tile instance where the map is whole tiles and the instance exists
    r->full = !plain && d->H % r->th == 0 && d->W % r->tw == 0;
    if (r->full && !dp_bwd_tile_exists(*r)) r->full = false;
    return dp_bwd_tile_exists(*r) ? 0 : YUNET_EINVAL;
}
static inline bool dp_bwd_streams16(const YunetDP* d) { DpRoute r; dp_bwd_route(d, d->x_dtype, &r); return r.family == DP_BWD16S; }
