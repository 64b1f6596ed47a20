// query.hip — language query of the feature field: fea_up and the CLIP relevancy in one kernel.
//
// The fea_up output y = W2 relu(W1 x + b1) + b2 (512 floats per pixel at the reference's size) exists only to be
// compared with a few text embeddings: s_k = (y . q_k) / max(|y|, 1e-12) for Q <= GG_QUERY_MAX unit query rows and,
// with canonical negatives, LERF's relevancy r_p = min_j softmax(tau [s_p, s_nj])_0 = 1 / (1 + exp(tau (max_j s_nj -
// s_p))).  This is gg_mlp_fwd_fast's kernel (mlp.hip, the packed workspace of mlp_fast.h) with the output stores
// replaced by register reductions, so y never reaches memory:
//   * |y|^2: each lane sums o^2 over the four outputs it holds of every 16-row tile of layer 2;
//   * y . q_k = h . (W2^T q_k) + b2 . q_k, formed in hidden space right after layer 1 (32 fmas per lane and query
//     instead of 128 in the layer-2 epilogue; across layer 2 a lane keeps only the queries it owns).  A small kernel
//     forms v_k = W2^T q_k and c_k = b2 . q_k once per call; they sit in LDS beside the two slice buffers and the
//     biases (129 floats per query);
//   * the pixel's four lanes (p, p + 16, p + 32, p + 48) add their partial sums with the permlane swaps of
//     mlpf_max_over_q; lane q4 keeps the queries k = 4 j + q4, and writes their s and r.
// Every sum runs in one fixed order, without atomics: results are identical run to run.
// The body is a copy of mlp_fwd_f16_kernel's rather than a template shared with it: instantiating a shared body
// with a store epilogue changed that kernel's instruction schedule, and gg_mlp_fwd_fast is kept as it is.
#include <cmath>

#include "mlp_fast.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define CQ_OWN ((GG_QUERY_MAX + 3) / 4)   // queries a lane owns: k = 4 j + q4
#define CQ_NPB 2                          // 16-pixel blocks per wave and iteration (mlp_fwd_f16_kernel: 4)

__device__ __forceinline__ float cq_sum_over_q(float v) {   // v_p + v_{p+16} + v_{p+32} + v_{p+48}, the same in all four
    auto r16 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    v = __builtin_bit_cast(float, (unsigned)r16[0]) + __builtin_bit_cast(float, (unsigned)r16[1]);
    auto r32 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    return __builtin_bit_cast(float, (unsigned)r32[0]) + __builtin_bit_cast(float, (unsigned)r32[1]);
}

template <int IN>
__global__ __launch_bounds__(MLPF_THREADS) void clip_query_kernel(long P, int out_dim, const float *__restrict__ x,
                                                                  const uint4 *__restrict__ packed,
                                                                  const float *__restrict__ inv_s,
                                                                  const float *__restrict__ b1,
                                                                  const float *__restrict__ b2, int nq, int np,
                                                                  const float *__restrict__ qv, float tau,
                                                                  float *__restrict__ sims, float *__restrict__ rel) {
    constexpr int KS1 = IN / 32;
    constexpr int W1_Q = 8 * KS1 * 2 * 64;                      // uint4 of the W1 slice
    constexpr int PF = MLPF_SLICE_Q / MLPF_THREADS;             // uint4 a thread carries of a slice in flight (8)
    extern __shared__ uint4 ldsq[];
    uint4 *buf0 = ldsq, *buf1 = ldsq + MLPF_SLICE_Q;
    float *tab = reinterpret_cast<float *>(ldsq + 2 * MLPF_SLICE_Q);
    float *b1s = tab, *i1s = tab + MLP_HID, *b2s = tab + 2 * MLP_HID, *i2s = b2s + out_dim;
    const int lane = threadIdx.x & 63, l16 = lane & 15, q4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nsl = (out_dim + 127) >> 7;                       // slices of W2
    const uint4 *w2p = packed + W1_Q;
    for (int i = threadIdx.x; i < MLP_HID; i += MLPF_THREADS) { b1s[i] = b1[i]; i1s[i] = inv_s[i]; }
    for (int i = threadIdx.x; i < out_dim; i += MLPF_THREADS) { b2s[i] = b2[i]; i2s[i] = inv_s[MLP_HID + i]; }
    float *vs = i2s + out_dim;                                  // [nq][128] W2^T q_k, then [nq] b2 . q_k
    for (int i = threadIdx.x; i < nq * (MLP_HID + 1); i += MLPF_THREADS) vs[i] = qv[i];
    const float *cs = vs + nq * MLP_HID;
    for (int i = threadIdx.x; i < W1_Q; i += MLPF_THREADS) buf0[i] = packed[i];
    __syncthreads();
    int g = 0;   // stages done: the current stage's weights are in buffer g & 1
    // request a slice (W2's slice sl, or W1 for sl < 0): global_load_lds_dwordx4 copies it straight into the buffer the
    // NEXT stage reads — 1 KB per wave and instruction (lane l: 16 bytes at base + 16 l), no registers in between (with
    // the slice held in 32 registers per thread across a stage's MFMAs the four-block build spilled 26-57 of them).
    // The other buffer is free: every wave passed the barrier that ended the stage which read it.
    auto request = [&](int sl) {
        const uint4 *src = sl < 0 ? packed : w2p + (size_t)sl * MLPF_SLICE_Q;
        const int n = sl < 0 ? W1_Q : min(MLPF_SLICE_Q, (out_dim - 128 * sl) / 16 * 4 * 2 * 64);
        uint4 *dst = (g & 1) ? buf0 : buf1;
        const int wbase = wave * 64;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int i0 = wbase + u * MLPF_THREADS;          // first uint4 of this wave's 1 KB (wave-uniform)
            if (i0 < n)
                __builtin_amdgcn_global_load_lds(src + i0 + lane, (__attribute__((address_space(3))) void *)(dst + i0), 16, 0, 0);
        }
    };
    auto deliver = [&]() {
        __builtin_amdgcn_s_waitcnt(0);     // (vmcnt, lgkmcnt, expcnt = 0: the copies have landed)
        __syncthreads();
        ++g;
    };
    // CQ_NPB pixel blocks of 16 per wave and iteration: two, not the store kernel's four — with four, the query's own
    // live registers (the dots, |y|^2, the NaN marks, six more arguments) pushed the kernel into 30-85 spilled VGPRs.
    constexpr int NPB = CQ_NPB;
    constexpr int PIX_PER_WG = (MLPF_THREADS / 64) * 16 * NPB;      // 256
    const long nblocks = (P + PIX_PER_WG - 1) / PIX_PER_WG;
    for (long blkid = blockIdx.x; blkid < nblocks; blkid += gridDim.x) {   // (every wave runs every barrier)
        long pix[NPB];
        bool ok[NPB];
#pragma unroll
        for (int b = 0; b < NPB; ++b) {
            pix[b] = blkid * PIX_PER_WG + wave * (16 * NPB) + 16 * b + l16;
            ok[b] = pix[b] < P;
        }
        // per lane and pixel block: the sum of o^2 over the outputs this lane holds (4 per 16-row tile), and y . q_k for
        // the queries k = 4 j + q4 this lane owns
        float ss[NPB], dt[NPB][CQ_OWN];
#pragma unroll
        for (int b = 0; b < NPB; ++b) ss[b] = 0.0f;
        unsigned hh[NPB][4][4], hl[NPB][4][4];
        float inv_sh[NPB];
        bool bad[NPB];
#pragma unroll
        for (int half = 0; half < NPB / 2; ++half) {
            if (half == NPB / 2 - 1) request(0);       // (in flight during the last pair's layer 1)
            // ---------------- x: scale per pixel, two fp16 pieces ---------------------------------------
            unsigned xh[2][KS1][4], xl[2][KS1][4];
            float inv_sx[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int pb = 2 * half + b;
                float xv[KS1][8];
                const float *xp = x + (size_t)(ok[pb] ? pix[pb] : 0) * IN + 8 * q4;
                float m = 0.0f, nan = 0.0f;
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) {
                    const float4 v0 = *reinterpret_cast<const float4 *>(xp + 32 * ks), v1 = *reinterpret_cast<const float4 *>(xp + 32 * ks + 4);
                    const float t[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        xv[ks][j] = ok[pb] ? t[j] : 0.0f;
                        m = fmaxf(m, fabsf(xv[ks][j]));
                        nan = xv[ks][j] != xv[ks][j] ? 1.0f : nan;
                    }
                }
                // a NaN feature would vanish in the scale's maximum and the ReLU (fmaxf drops NaN): the row is marked
                // and its outputs are NaN, as torch's relu and F.normalize give
                bad[pb] = mlpf_max_over_q(nan) != 0.0f;
                const float sx = pow2_scale(mlpf_max_over_q(m));
                inv_sx[b] = pow2_inv(sx);
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks)
#pragma unroll
                    for (int t = 0; t < 4; ++t) split2h(xv[ks][2 * t] * sx, xv[ks][2 * t + 1] * sx, xh[b][ks][t], xl[b][ks][t]);
            }
            // ---------------- layer 1: H^T = relu(W1 X^T + b1) -------------------------------------------
            float h[2][32];
            {
                const uint4 *wb = (g & 1) ? buf1 : buf0;
#pragma unroll
                for (int tp = 0; tp < 4; ++tp) {
                    f32x4 acc[2][2];
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int b = 0; b < 2; ++b) acc[u][b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int ks = 0; ks < KS1; ++ks) {
                        h16x8 Ah[2], Al[2], Bh[2], Bl[2];
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const uint4 ah = wb[(((2 * tp + u) * KS1 + ks) * 2) * 64 + lane], al = wb[(((2 * tp + u) * KS1 + ks) * 2 + 1) * 64 + lane];
                            Ah[u] = H8(ah.x, ah.y, ah.z, ah.w);
                            Al[u] = H8(al.x, al.y, al.z, al.w);
                            Bh[u] = H8(xh[u][ks][0], xh[u][ks][1], xh[u][ks][2], xh[u][ks][3]);      // (u doubles as the pixel block)
                            Bl[u] = H8(xl[u][ks][0], xl[u][ks][1], xl[u][ks][2], xl[u][ks][3]);
                        }
#pragma unroll
                        for (int pr = 0; pr < 4; ++pr)
#pragma unroll
                            for (int u = 0; u < 2; ++u)
#pragma unroll
                                for (int b = 0; b < 2; ++b)
                                    acc[u][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16((pr >> 1) ? Ah[u] : Al[u], (pr & 1) ? Bh[b] : Bl[b],
                                                                                       acc[u][b], 0, 0, 0);
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int m0 = 16 * (2 * tp + u) + 4 * q4;       // hidden units m0 .. m0 + 3
                        const float4 bi = *reinterpret_cast<const float4 *>(b1s + m0), iv = *reinterpret_cast<const float4 *>(i1s + m0);
                        const float bb[4] = {bi.x, bi.y, bi.z, bi.w}, ii[4] = {iv.x, iv.y, iv.z, iv.w};
#pragma unroll
                        for (int b = 0; b < 2; ++b)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                h[b][4 * (2 * tp + u) + r] = fmaxf(__builtin_fmaf(acc[u][b][r], ii[r] * inv_sx[b], bb[r]), 0.0f);
                    }
                }
            }
            // ---------------- y . q_k = h . (W2^T q_k) + b2 . q_k: lane (p, q4) holds hidden units 16 T + 4 q4 + r ---
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float d[GG_QUERY_MAX];
#pragma unroll
                for (int k = 0; k < GG_QUERY_MAX; ++k) {
                    d[k] = 0.0f;
                    if (k >= nq) continue;
                    float a = 0.0f;
#pragma unroll
                    for (int T = 0; T < 8; ++T) {
                        const float4 v = *reinterpret_cast<const float4 *>(vs + k * MLP_HID + 16 * T + 4 * q4);
                        a = __builtin_fmaf(h[b][4 * T + 3], v.w, __builtin_fmaf(h[b][4 * T + 2], v.z,
                            __builtin_fmaf(h[b][4 * T + 1], v.y, __builtin_fmaf(h[b][4 * T], v.x, a))));
                    }
                    d[k] = cq_sum_over_q(a) + cs[k];
                }
#pragma unroll
                for (int j = 0; j < CQ_OWN; ++j) {        // keep d[4 j + q4] (selects: no dynamic register index)
                    float own = d[4 * j];
#pragma unroll
                    for (int r = 1; r < 4; ++r) own = q4 == r ? d[4 * j + r] : own;
                    dt[2 * half + b][j] = own;
                }
            }
            // ---------------- hidden: second scale per pixel, two fp16 pieces ----------------------------
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int pb = 2 * half + b;
                float m = 0.0f;
#pragma unroll
                for (int i = 0; i < 32; ++i) m = fmaxf(m, h[b][i]);
                const float sh = pow2_scale(mlpf_max_over_q(m));
                inv_sh[pb] = pow2_inv(sh);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        split2h(h[b][8 * ks + 2 * t] * sh, h[b][8 * ks + 2 * t + 1] * sh, hh[pb][ks][t], hl[pb][ks][t]);
            }
        }
        deliver();
        // ---------------- layer 2, slice by slice ------------------------------------------------------
        for (int sl = 0; sl < nsl; ++sl) {
            request(sl + 1 < nsl ? sl + 1 : -1);       // (after the last slice: W1 for the next iteration)
            const uint4 *wb = (g & 1) ? buf1 : buf0;
            const int nt = min(8, (out_dim - 128 * sl) >> 4);
            for (int tp = 0; 2 * tp < nt; ++tp) {
                f32x4 acc[2][NPB];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int b = 0; b < NPB; ++b) acc[u][b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    h16x8 Ah[2], Al[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int tile = min(2 * tp + u, nt - 1);
                        const int aidx = ((tile * 4 + ks) * 2) * 64;
                        const uint4 ah = wb[aidx + lane], al = wb[aidx + 64 + lane];
                        Ah[u] = H8(ah.x, ah.y, ah.z, ah.w);
                        Al[u] = H8(al.x, al.y, al.z, al.w);
                    }
#pragma unroll
                    for (int pr = 0; pr < 4; ++pr)
#pragma unroll
                        for (int u = 0; u < 2; ++u)
#pragma unroll
                            for (int b = 0; b < NPB; ++b) {
                                const h16x8 Bp = (pr & 1) ? H8(hh[b][ks][0], hh[b][ks][1], hh[b][ks][2], hh[b][ks][3])
                                                          : H8(hl[b][ks][0], hl[b][ks][1], hl[b][ks][2], hl[b][ks][3]);
                                acc[u][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16((pr >> 1) ? Ah[u] : Al[u], Bp, acc[u][b], 0, 0, 0);
                            }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (2 * tp + u >= nt) break;
                    const int m0 = 128 * sl + 16 * (2 * tp + u) + 4 * q4;   // outputs m0 .. m0 + 3
                    const float4 bi = *reinterpret_cast<const float4 *>(b2s + m0), iv = *reinterpret_cast<const float4 *>(i2s + m0);
#pragma unroll
                    for (int b = 0; b < NPB; ++b) {
                        if (!ok[b]) continue;
                        float4 o;
                        o.x = __builtin_fmaf(acc[u][b][0], iv.x * inv_sh[b], bi.x);
                        o.y = __builtin_fmaf(acc[u][b][1], iv.y * inv_sh[b], bi.y);
                        o.z = __builtin_fmaf(acc[u][b][2], iv.z * inv_sh[b], bi.z);
                        o.w = __builtin_fmaf(acc[u][b][3], iv.w * inv_sh[b], bi.w);
                        ss[b] = __builtin_fmaf(o.w, o.w, __builtin_fmaf(o.z, o.z, __builtin_fmaf(o.y, o.y, __builtin_fmaf(o.x, o.x, ss[b]))));
                    }
                }
            }
            deliver();
        }
        // ---------------- the row's numbers: |y| over the pixel's four lanes, s, the negatives' maximum, r ----------
#pragma unroll
        for (int b = 0; b < NPB; ++b) {
            const float nrm = fmaxf(sqrtf(cq_sum_over_q(ss[b])), 1e-12f);      // F.normalize's max(|y|, eps)
            float s[CQ_OWN], mneg = -INFINITY;
#pragma unroll
            for (int j = 0; j < CQ_OWN; ++j) {
                const int k = 4 * j + q4;
                s[j] = bad[b] ? __builtin_nanf("") : dt[b][j] / nrm;
                if (k >= np && k < nq) mneg = fmaxf(mneg, s[j]);
            }
            mneg = mlpf_max_over_q(mneg);
            if (!ok[b]) continue;
#pragma unroll
            for (int j = 0; j < CQ_OWN; ++j) {
                const int k = 4 * j + q4;
                if (sims && k < nq) sims[(size_t)pix[b] * nq + k] = s[j];
                if (rel && k < np) rel[(size_t)pix[b] * np + k] = 1.0f / (1.0f + expf(tau * (mneg - s[j])));
            }
        }
    }
}

// v_k = W2^T q_k (fp32, c = 0, 1, ... in order) and c_k = b2 . q_k: one workgroup per query, one lane per hidden unit
__global__ __launch_bounds__(MLP_HID) void clip_query_prep_kernel(int out_dim, const float *__restrict__ w2,
                                                                 const float *__restrict__ b2,
                                                                 const float *__restrict__ queries, float *__restrict__ qv,
                                                                 int nq) {
    const int k = blockIdx.x, i = threadIdx.x;
    const float *q = queries + (size_t)k * out_dim;
    float a = 0.0f;
    for (int c = 0; c < out_dim; ++c) a = __builtin_fmaf(w2[(size_t)c * MLP_HID + i], q[c], a);
    qv[k * MLP_HID + i] = a;
    if (i == 0) {
        float cb = 0.0f;
        for (int c = 0; c < out_dim; ++c) cb = __builtin_fmaf(b2[c], q[c], cb);
        qv[nq * MLP_HID + k] = cb;
    }
}

// LDS: two 64 KB slice buffers + [2 x 128 + 2 x out_dim + 129 nq] floats must fit the CU's 160 KB
static inline bool cq_lds_fits(int out_dim, int nq) { return 2 * (size_t)out_dim + (size_t)(MLP_HID + 1) * nq + 2 * MLP_HID <= 8192; }
// the workspace: gg_mlp_fwd_fast's packed weights, then v_k and c_k
static inline size_t cq_qv_offset(int in_dim, int out_dim) { return gg_align_up(gg_mlp_fwd_fast_workspace(in_dim, MLP_HID, out_dim), 16); }

extern "C" size_t gg_clip_query_workspace(int in_dim, int hidden_dim, int out_dim, int num_queries) {
    if ((in_dim != 32 && in_dim != 64 && in_dim != 128) || num_queries < 1 || num_queries > GG_QUERY_MAX ||
        out_dim <= 0 || !cq_lds_fits(out_dim, num_queries))
        return 0;
    if (hidden_dim != MLP_HID || out_dim % 16 || out_dim > GG_MLP_FAST_MAX_OUT) return 0;
    return cq_qv_offset(in_dim, out_dim) + sizeof(float) * (size_t)(MLP_HID + 1) * num_queries;
}

extern "C" int gg_clip_query(int64_t num_rows, int in_dim, int hidden_dim, int out_dim, const float *x,
                             const float *w1, const float *b1, const float *w2, const float *b2, int num_queries,
                             int num_positives, const float *queries, float temperature, float *sims,
                             float *relevancy, void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(num_rows >= 0, "num_rows < 0");
    GG_REQUIRE(hidden_dim == MLP_HID, "hidden_dim must be 128 (the reference's fea_up)");
    GG_REQUIRE(in_dim == 32 || in_dim == 64 || in_dim == 128, "in_dim must be 32, 64 or 128");
    GG_REQUIRE(out_dim > 0 && out_dim % 16 == 0 && out_dim <= GG_MLP_FAST_MAX_OUT,
               "out_dim must be a multiple of 16, at most 3968");
    GG_REQUIRE(num_queries >= 1 && num_queries <= GG_QUERY_MAX, "num_queries must be in [1, GG_QUERY_MAX]");
    GG_REQUIRE(cq_lds_fits(out_dim, num_queries),
               "2 x out_dim + 129 x num_queries + 256 floats exceed the 32 KB of LDS beside the weight slices");
    GG_REQUIRE(num_positives >= 0 && num_positives <= num_queries, "num_positives must be in [0, num_queries]");
    GG_REQUIRE(!relevancy || (num_positives >= 1 && num_positives < num_queries),
               "relevancy needs at least one positive and one negative (num_positives < num_queries)");
    GG_REQUIRE(std::isfinite(temperature) && temperature > 0.0f, "temperature must be finite and > 0");
    if (num_rows == 0) return GG_OK;
    GG_REQUIRE(sims || relevancy, "both outputs are NULL: nothing to compute");
    GG_REQUIRE(x && w1 && b1 && w2 && b2 && queries, "null pointer");
    GG_REQUIRE(((uintptr_t)x & 15) == 0, "x must be 16-byte aligned");
    GG_REQUIRE((((uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2) & 3) == 0,
               "w1, b1, w2 and b2 must be 4-byte aligned");
    GG_REQUIRE((((uintptr_t)queries | (uintptr_t)sims | (uintptr_t)relevancy) & 3) == 0,
               "queries, sims and relevancy must be 4-byte aligned");
    if (ws == nullptr || ws_bytes < gg_clip_query_workspace(in_dim, hidden_dim, out_dim, num_queries) ||
        ((uintptr_t)ws & 15)) {
        gg_set_error("gg_clip_query: workspace of gg_clip_query_workspace() bytes, 16-byte aligned, expected");
        return GG_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    const long nblocks = (num_rows + 128 * CQ_NPB - 1) / (128 * CQ_NPB);
    const int grid = (int)(nblocks < cus ? nblocks : cus);
    const size_t lds_bytes =
        sizeof(uint4) * 2 * MLPF_SLICE_Q + sizeof(float) * ((size_t)2 * MLP_HID + 2 * (size_t)out_dim + (MLP_HID + 1) * num_queries);
    const int np = relevancy ? num_positives : 0;
    hipError_t e = hipSuccess;
    gg_prof_begin(GG_K_QUERY, s);
    const float *inv_s = mlpf_pack(in_dim, out_dim, w1, w2, ws, s);
    const uint4 *packed = reinterpret_cast<const uint4 *>(ws);
    float *qv = reinterpret_cast<float *>(reinterpret_cast<char *>(ws) + cq_qv_offset(in_dim, out_dim));
    hipLaunchKernelGGL(clip_query_prep_kernel, dim3(num_queries), dim3(MLP_HID), 0, s, out_dim, w2, b2, queries, qv,
                       num_queries);
#define CQ_LAUNCH(IN_)                                                                                                \
    do {                                                                                                             \
        e = hipFuncSetAttribute((const void *)clip_query_kernel<IN_>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                (int)lds_bytes);                                                                     \
        if (e == hipSuccess)                                                                                         \
            hipLaunchKernelGGL((clip_query_kernel<IN_>), dim3(grid), dim3(MLPF_THREADS), lds_bytes, s, (long)num_rows, \
                               out_dim, x, packed, inv_s, b1, b2, num_queries, np, qv, temperature, sims,            \
                               relevancy);                                                                           \
    } while (0)
    if (in_dim == 32) CQ_LAUNCH(32);
    else if (in_dim == 64) CQ_LAUNCH(64);
    else CQ_LAUNCH(128);
#undef CQ_LAUNCH
    gg_prof_end(GG_K_QUERY, s);
    if (e != hipSuccess) {
        gg_set_error("gg_clip_query: cannot reserve %zu bytes of LDS: %s", lds_bytes, hipGetErrorString(e));
        return GG_ERR_LAUNCH;
    }
    GG_CHECK_LAUNCH();
    return GG_OK;
}
