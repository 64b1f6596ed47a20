// ordered_sum.h — the sums whose order of additions is part of a contract: the fp64 sums of gg_icp_step
// (csrc/register.hip), gg_plane_classify (csrc/support_plane.hip) and the image and geometry losses
// (csrc/imgloss.hip), and the wave reductions of csrc/cluster.hip, csrc/objmask.hip and csrc/losses.hip.  No
// floating-point atomics anywhere here: the same inputs give the same bits.  The orders, each stated once:
//
//   wave       gg_wave_sum / gg_wave_min / gg_wave_max: an xor butterfly over the 64 lanes, offsets 32, 16, ... 1.
//              Both partners of a step combine the same two numbers, so every lane ends with the same bits.
//   block row  gg_block_row<W>: a workgroup of 256 lanes with W values per lane.  Each value by the wave order, lane 0
//              of every wave stores its W sums to LDS, and lanes k < W write ((w0 + w1) + w2) + w3 of column k.
//   chains     gg_chain_sum<W, CHAINS>: one workgroup sums the nrows rows of a slab of W columns.  Chain c adds
//              rows c, c + CHAINS, c + 2 CHAINS, ... of column k in that order, starting from 0; then lane k < W adds
//              the chains 0, 1, ... CHAINS - 1 in order.  gg_icp_step and gg_plane_classify use GG_SUM_CHAINS.
//              The order depends on W, CHAINS and nrows only, not on LANES.
//   tree       gg_tree_sum<W>: one workgroup of 256 lanes sums n partials of W columns.  Lane t adds partials t,
//              t + 256, ... in that order, starting from 0; then an LDS tree with strides 128, 64, ... 1, lane t
//              adding entry t + stride to its own.  The losses' order: it is NOT the chains' order, and the numpy
//              restatements in tests/ hold each to its own.
#pragma once
#include "gg_common.h"

#define GG_SUM_CHAINS 16

template <class T>
__device__ __forceinline__ T gg_wave_sum(T v) {
#pragma unroll
    for (int o = GG_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, GG_WAVE);
    return v;
}

// 32-bit integers (int32_t, uint32_t): exact, so the order is free
template <class T>
__device__ __forceinline__ T gg_wave_min(T v) {
    static_assert(sizeof(T) == 4, "32-bit integers");
#pragma unroll
    for (int o = GG_WAVE / 2; o > 0; o >>= 1) v = min(v, (T)__shfl_xor((int)v, o, GG_WAVE));
    return v;
}
template <class T>
__device__ __forceinline__ T gg_wave_max(T v) {
    static_assert(sizeof(T) == 4, "32-bit integers");
#pragma unroll
    for (int o = GG_WAVE / 2; o > 0; o >>= 1) v = max(v, (T)__shfl_xor((int)v, o, GG_WAVE));
    return v;
}

// row[k] = the workgroup's sum of v[k], k < W.  256 lanes; contains __syncthreads(): every lane calls it.
template <int W>
__device__ __forceinline__ void gg_block_row(const double (&v)[W], double (&s_w)[4][W], double *__restrict__ row) {
    const int lane = threadIdx.x & (GG_WAVE - 1), wave = threadIdx.x / GG_WAVE;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const double t = gg_wave_sum(v[k]);
        if (lane == 0) s_w[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < W) {
        const int k = threadIdx.x;
        row[k] = ((s_w[0][k] + s_w[1][k]) + s_w[2][k]) + s_w[3][k];
    }
}

// Lane k < W returns the sum of column k of slab (nrows x W); the other lanes return 0.  One workgroup of
// CHAINS x LANES lanes, LANES >= W per chain, of which the first W work; contains __syncthreads(): every lane
// calls it.
template <int W, int CHAINS, int LANES = W>
__device__ __forceinline__ double gg_chain_sum(int nrows, const double *__restrict__ slab, double (&s_c)[CHAINS][W]) {
    const int k = threadIdx.x % LANES, c = threadIdx.x / LANES;
    if (k < W) {
        double a = 0.0;
        for (int r = c; r < nrows; r += CHAINS) a += slab[(size_t)W * r + k];
        s_c[c][k] = a;
    }
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < W) {
        t = s_c[0][threadIdx.x];
        for (int cc = 1; cc < CHAINS; ++cc) t += s_c[cc][threadIdx.x];
    }
    return t;
}

// red[k][0] = the sum of column k of partials (n x W), for every lane to read.  One workgroup of 256 lanes;
// contains __syncthreads(): every lane calls it.
template <int W>
__device__ __forceinline__ void gg_tree_sum(int n, const double *__restrict__ partials, double (&red)[W][256]) {
    const int tid = threadIdx.x;
    double v[W];
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = 0.0;
    for (int b = tid; b < n; b += 256)
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] += partials[W * (size_t)b + k];
#pragma unroll
    for (int k = 0; k < W; ++k) red[k][tid] = v[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
#pragma unroll
            for (int k = 0; k < W; ++k) red[k][tid] += red[k][tid + s];
        __syncthreads();
    }
}
