// prep_common.h — ordered workgroup scans shared by csrc/prepare.hip and, through grid_sort.h, by csrc/knn.hip,
// csrc/cluster.hip and csrc/register.hip; and GG_REQUIRE_FILL, the one way their calls give up on a failed fill.
//
// A workgroup of PP_THREADS lanes owns PP_TILE = PP_THREADS x PP_ITEMS consecutive items, PP_ITEMS consecutive
// items per lane; pp_block_scan gives each lane the number of items before its own in the tile.  Exclusive
// offsets of per-tile (or per-cell) int32 counts come from one workgroup walking them in order
// (pp_scan_single_kernel) or, for long arrays, from per-tile sums + that walk + a per-tile apply (pp_scan_long).
// Integer adds only: every offset is exact and independent of scheduling.
#pragma once
#include "gg_common.h"

// e: the hipError_t of a gg_fill_async (or of a kn_sort, whose only failures are its fills), between gg_prof_begin
// and gg_prof_end of kernel `id` on stream s.
#define GG_REQUIRE_FILL(id, s, e)                                                    \
    do {                                                                             \
        const hipError_t e__ = (e);                                                  \
        if (e__ != hipSuccess) {                                                     \
            gg_prof_end(id, s);                                                      \
            gg_set_error("%s: fill failed: %s", __func__, hipGetErrorString(e__));   \
            return GG_ERR_LAUNCH;                                                    \
        }                                                                            \
    } while (0)

#define PP_THREADS 256
#define PP_ITEMS 4
#define PP_TILE (PP_THREADS * PP_ITEMS)

// Exclusive prefix of v over the workgroup (PP_THREADS lanes); `total` = the sum.  Contains __syncthreads():
// every lane of the workgroup calls it.  s_w: PP_THREADS / 64 ints of LDS.
__device__ __forceinline__ int pp_block_scan(int v, int *s_w, int &total) {
    const int lane = threadIdx.x & (GG_WAVE - 1), wid = threadIdx.x / GG_WAVE;
    int x = v;
#pragma unroll
    for (int o = 1; o < GG_WAVE; o <<= 1) {
        const int y = __shfl_up(x, o, GG_WAVE);
        if (lane >= o) x += y;
    }
    if (lane == GG_WAVE - 1) s_w[wid] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < PP_THREADS / GG_WAVE; ++w) {
        const int t = s_w[w];
        base += w < wid ? t : 0;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base + x - v;
}

// offsets[i] = counts[0] + ... + counts[i-1] for i < n, *total = the sum (int64); one workgroup, tiles of PP_TILE
// walked in order with a running carry.  The carry stays below 2^31 (callers bound the item count).
static __global__ __launch_bounds__(PP_THREADS) void pp_scan_single_kernel(const int32_t *__restrict__ counts, int n,
                                                                          int32_t *__restrict__ offsets,
                                                                          int64_t *__restrict__ total) {
    __shared__ int s_w[PP_THREADS / GG_WAVE];
    int carry = 0;
    for (int t0 = 0; t0 < n; t0 += PP_TILE) {
        const int i0 = t0 + threadIdx.x * PP_ITEMS;
        int c[PP_ITEMS], sum = 0;
#pragma unroll
        for (int j = 0; j < PP_ITEMS; ++j) {
            c[j] = i0 + j < n ? counts[i0 + j] : 0;
            sum += c[j];
        }
        int tile;
        int o = carry + pp_block_scan(sum, s_w, tile);
#pragma unroll
        for (int j = 0; j < PP_ITEMS; ++j) {
            if (i0 + j < n) offsets[i0 + j] = o;
            o += c[j];
        }
        carry += tile;
    }
    if (threadIdx.x == 0 && total) *total = carry;
}

// Long arrays: tile sums, then pp_scan_single_kernel over them, then each tile's exclusive offsets.
static __global__ __launch_bounds__(PP_THREADS) void pp_scan_reduce_kernel(const int32_t *__restrict__ counts, int n,
                                                                          int32_t *__restrict__ tile_sums) {
    __shared__ int s_w[PP_THREADS / GG_WAVE];
    const int i0 = blockIdx.x * PP_TILE + threadIdx.x * PP_ITEMS;
    int sum = 0;
#pragma unroll
    for (int j = 0; j < PP_ITEMS; ++j) sum += i0 + j < n ? counts[i0 + j] : 0;
    int tile;
    pp_block_scan(sum, s_w, tile);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = tile;
}

static __global__ __launch_bounds__(PP_THREADS) void pp_scan_apply_kernel(const int32_t *__restrict__ counts, int n,
                                                                         const int32_t *__restrict__ tile_offsets,
                                                                         int32_t *__restrict__ offsets) {
    __shared__ int s_w[PP_THREADS / GG_WAVE];
    const int i0 = blockIdx.x * PP_TILE + threadIdx.x * PP_ITEMS;
    int c[PP_ITEMS], sum = 0;
#pragma unroll
    for (int j = 0; j < PP_ITEMS; ++j) {
        c[j] = i0 + j < n ? counts[i0 + j] : 0;
        sum += c[j];
    }
    int tile;
    int o = tile_offsets[blockIdx.x] + pp_block_scan(sum, s_w, tile);
#pragma unroll
    for (int j = 0; j < PP_ITEMS; ++j) {
        if (i0 + j < n) offsets[i0 + j] = o;
        o += c[j];
    }
}

// The long form on stream s: offsets[i] = counts[0] + ... + counts[i-1] for i < n, *total = the sum.  tile_sums and
// tile_offs hold one int32 per tile of PP_TILE items.
static inline void pp_scan_long(const int32_t *counts, int n, int32_t *tile_sums, int32_t *tile_offs, int32_t *offsets,
                                int64_t *total, hipStream_t s) {
    const int tiles = (n + PP_TILE - 1) / PP_TILE;
    hipLaunchKernelGGL(pp_scan_reduce_kernel, dim3((unsigned)tiles), dim3(PP_THREADS), 0, s, counts, n, tile_sums);
    hipLaunchKernelGGL(pp_scan_single_kernel, dim3(1), dim3(PP_THREADS), 0, s, tile_sums, tiles, tile_offs, total);
    hipLaunchKernelGGL(pp_scan_apply_kernel, dim3((unsigned)tiles), dim3(PP_THREADS), 0, s, counts, n, tile_offs,
                       offsets);
}
