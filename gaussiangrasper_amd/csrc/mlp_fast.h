// mlp_fast.h — the fast feature up-projection forward's packed weights and helpers, shared by gg_mlp_fwd_fast
// (mlp.hip) and gg_clip_query (query.hip), which read the same workspace layout.
#pragma once
#include "gg_common.h"

#ifndef MLP_HID
#define MLP_HID 128
#endif

// ---------------------------------------------------------------------------------------------
// Fast forward (round 3): both layers as fp32-grade products of fp16 two-piece operands on
// v_mfma_f32_16x16x32_f16 (gg_common.h: four 16-cycle MFMAs per 16 x 16 x 32 block where the fp32 instruction takes
// eight of 32 cycles) — a quarter of the matrix cycles of the kernels above, at the same or better accuracy against
// a double-precision sum (tools/check_f16split.hip), but NOT the oracle's summation order: results agree with
// oracle/gg_oracle.c:mlp_fwd to ~1e-6 of the largest output instead of bit for bit (gg_mlp_fwd stays the exact-order
// call).  The reference's side is cuBLAS behind nn.Linear — no summation order to match there.
//
//   * gg_mlp_pack (once per weight set): every row of W1 and W2 gets a power-of-two scale (row maximum into
//     [2^14, 2^15)) and is written as (hi, lo) fp16 pieces in the A-operand order of the MFMA — per (16-row tile,
//     k-step of 32, piece) 64 lanes x 16 bytes, lane = (row % 16) + 16 (k-block) — so that staging a 128-row
//     slice into LDS is a 64 KB copy and every A operand one conflict-free ds_read_b128.  W2's k order is the order
//     layer 1's accumulators hold the hidden units in (below); 1 / scale per row goes beside them.
//   * transposed chain as above: H^T = W1 X^T, Y^T = W2 H^T, N = 16 pixels per MFMA.  Lane (p = lane % 16,
//     q = lane / 16) loads x[pixel p][32 ks + 8 q .. + 7] (two float4), scales by the pixel's power of two (row
//     maximum over the lane's values and the three other q lanes: two permlane swaps) and splits: the B operand of
//     layer 1.  Layer 1's accumulators — lane (p, q) holds hidden units 16 t + 4 q + r of pixel p — become layer 2's
//     B operand WITHOUT moving: k-step ks of layer 2 contracts the hidden units of tiles 2 ks and 2 ks + 1, slot j of
//     k-block q is hidden unit 16 (2 ks + j / 4) + 4 q + j % 4 (mlpf_hidden_of); W2 is packed in that order.
//     Bias, un-scaling and ReLU are one multiply, one fma and one max per hidden value; the pixel's second scale
//     comes from the ReLU outputs the same way as the first.
//   * persistent workgroups of 8 waves (two per SIMD), 256 pixels per iteration, 32 per wave as two 16-pixel blocks
//     (each A operand read feeds 8 MFMAs); two tiles x two blocks = four independent accumulator chains.  The five
//     weight slices of an iteration (W1, four of W2 at out = 512) go through a two-deep ring of 64 KB LDS buffers:
//     the next slice is requested from L2 into registers before a slice's MFMAs and written to the other buffer
//     after them — one barrier per slice.
// ---------------------------------------------------------------------------------------------
#define MLPF_THREADS 512
#ifndef MLPF_NPB
#define MLPF_NPB 4   // 16-pixel blocks per wave and iteration (2: measured below)
#endif
#ifndef MLPF_ABL
#define MLPF_ABL 0   // measurement builds: 1 no output stores, 2 no layer-2 MFMAs, 3 no stores and layer 2's A operands read once
#endif
#define GG_MLP_FAST_MAX_OUT 3968                 // (160 KB - 2 x 64 KB slices) / 4 B = 8192 floats = 2 x 128 + 2 x out_dim
#define MLPF_SLICE_Q 4096                        // uint4 per 64 KB slice: 8 tiles x 4 k-steps x 2 pieces x 64 lanes
__host__ __device__ __forceinline__ int mlpf_hidden_of(int ks, int q, int j) { return 16 * (2 * ks + (j >> 2)) + 4 * q + (j & 3); }

// one wave per weight row: rows [0, 128) are W1's, [128, 128 + out) W2's
template <int IN>
__global__ __launch_bounds__(64) void mlpf_pack_kernel(int out_dim, const float *__restrict__ w1,
                                                       const float *__restrict__ w2, uint4 *__restrict__ packed,
                                                       float *__restrict__ inv_s) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const bool first = row < MLP_HID;
    const int K = first ? IN : MLP_HID, KS = K / 32;
    const float *src = first ? w1 + (size_t)row * IN : w2 + (size_t)(row - MLP_HID) * MLP_HID;
    float m = 0.0f;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(src[k]));
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    const float sc = pow2_scale(m);
    if (lane == 0) inv_s[row] = pow2_inv(sc);
    // lane = (ks, q): 8 values of this row
    const int ks = lane >> 2, q = lane & 3;
    if (ks >= KS) return;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[first ? 32 * ks + 8 * q + j : mlpf_hidden_of(ks, q, j)] * sc;
    unsigned hi[4], lo[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) split2h(v[2 * t], v[2 * t + 1], hi[t], lo[t]);
    const int r2 = first ? row : row - MLP_HID;
    const int slice = r2 >> 7, tile = (r2 & 127) >> 4, l16 = r2 & 15;
    // W1's slice has KS1 k-steps per tile, W2's four
    uint4 *base = packed + (first ? (size_t)0 : (size_t)8 * (IN / 32) * 2 * 64 + (size_t)slice * MLPF_SLICE_Q);
    uint4 *dst = base + ((size_t)(tile * KS + ks) * 2) * 64 + 16 * q + l16;
    dst[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    dst[64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

__device__ __forceinline__ float mlpf_max_over_q(float m) {   // maximum over the four lanes p, p + 16, p + 32, p + 48
    auto r16 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, m), __builtin_bit_cast(unsigned, m), false, false);
    m = fmaxf(__builtin_bit_cast(float, (unsigned)r16[0]), __builtin_bit_cast(float, (unsigned)r16[1]));
    auto r32 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, m), __builtin_bit_cast(unsigned, m), false, false);
    return fmaxf(__builtin_bit_cast(float, (unsigned)r32[0]), __builtin_bit_cast(float, (unsigned)r32[1]));
}

// The packed workspace of gg_mlp_fwd_fast_workspace(in_dim, 128, out_dim) bytes: the fp16 pieces of W1 and W2 in slice
// order, then 1 / scale per weight row (128 + out_dim floats).  mlpf_pack enqueues mlpf_pack_kernel (in_dim 32, 64 or
// 128) and returns where the scales start.
static inline size_t mlpf_packed_quads(int in_dim, int out_dim) {
    return (size_t)8 * (in_dim / 32) * 2 * 64 + (((size_t)out_dim + 127) / 128) * MLPF_SLICE_Q;
}
float *mlpf_pack(int in_dim, int out_dim, const float *w1, const float *w2, void *ws, hipStream_t s);

