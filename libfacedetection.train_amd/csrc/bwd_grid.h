// bwd_grid.h -- grid sizes of the backward launches: what the grid-size queries (conv_bwd_host.hip) and the launches
// (conv_bwd.hip, conv_bwd64.hip, conv_bwd_ew.hip) must agree on, each defined once.
#pragma once
#include "common.h"

#define DP_BWD_MAX_BLOCKS 256     // 512 threads, up to 138 KB LDS: one workgroup per CU
#define STEM_BWD_MAX_BLOCKS 768   // 256 threads, 35 KB LDS: three per CU
#define SB_TW 32                  // stem_bwd_kernel: output pixels per tile
#define SB_TH 8
// the 16 -> 16 unit on the 160 x 160 / 80 x 80 levels runs on 16 x 32 tiles
static inline bool dp_bwd_big_tile(int H, int W, int cin, int cout) {
    return cin == 16 && cout == 16 && W >= 64 && H >= 32;
}
// Waves per workgroup of dp_bwd64 (the 64 -> 64 units): 8 = one 512-thread workgroup per CU on 8 x 16 tiles,
// 4 = two independent 256-thread workgroups per CU on 8 x 8 tiles.  Measured (tools/ubench/bwd_ab, N = 256):
// 80 x 80 0.415 vs 0.429 ms, 40 x 40 0.139 vs 0.126 ms (a 40-wide map fills 8 x 8 tiles exactly, 17 % of every
// 8 x 16 tile row is padding), packed 20 x 20 / 10 x 10 canvases 0.052 / 0.023 vs 0.055 / 0.028 ms.  So: 8 x 8
// tiles where the width is a multiple of 8 but not of 16, 8 x 16 otherwise.  The option bwd64_nw = 4 | 8 forces one
// (A/B runs).  The choice fixes the persistent grid, i.e. the rows of wgrad_partials.
static inline int bwd64_nw(int N, int H, int W) {
    const int forced = yunet_options().bwd64_nw;
    if (forced == 4 || forced == 8) return forced;
    if (dp_pack_geom(N, H, W).on) return 8;
    return (W % 16 != 0 && W % 8 == 0) ? 4 : 8;
}

// Grid of the element-wise backward kernels (pool / upsample-add).  Every workgroup ends with 2 * C fp64 atomics on
// the producer's BN-backward sums -- the same 128 addresses for the whole launch: with 2048 workgroups those 262 k
// same-address atomics, not the 59 - 370 MB of traffic, set the time (pool_bwd + upadd_bwd 0.260 ms per step).
// Measured: cap 1024 0.223 ms, 768 0.213, 512 0.216, 384 0.242, 256 0.295 (too few waves in flight).
// With the sums in eight replicas (YunetBN::slots) the order is the same -- 768 0.209 ms, 1536 0.255, 2048 0.257,
// 4096 0.302: it is the NUMBER of fp64 atomics of a launch (2 * C per workgroup), not only their addresses.
static inline int ew_grid(long long total) {
    long long b = (total + 255) / 256;
    const long long cap = yunet_options().ew_grid;      // 768 unless a measurement changed it
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
