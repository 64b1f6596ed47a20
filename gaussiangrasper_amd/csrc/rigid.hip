// rigid.hip — the rigid move of a subset of the Gaussians as a differentiable operator: gg_rigid_fwd moves the
// selected rows' means and quaternions by a pose that lives on the device, gg_rigid_bwd carries the cotangents back to
// the rows and to the pose's sixteen numbers.  The contract is in include/gg_raster.h and PARITY.md "Object pose
// refinement"; the design in DESIGN.md §3.27.
//
// Forward, one launch: one lane per row.  The pose (12 + 4 floats) is read by every lane from the same addresses.
//
// Backward, two launches, the fixed orders of ordered_sum.h: rg_bwd_kernel, one lane per row and 256 rows per
// workgroup, writes the per-row gradients (when asked for) and one slab row of 16 sums per workgroup (the block row);
// rg_finish_kernel, one workgroup, sums the slab's rows by the chains, rounds to fp32 and writes.  No atomics.
// Everything is fp64 on fp32 inputs, every expression in the order the header states, no contraction.
#include "gg_common.h"
#include "ordered_sum.h"

#define RG_SUMS 16
#define RG_ROWS 256              // rows (Gaussians) per workgroup of the backward: one per lane
#define RG_FIN_THREADS (GG_SUM_CHAINS * RG_SUMS)

// a (x) b, the Hamilton product of wxyz quaternions: each component four products added left to right
__device__ __forceinline__ void rg_quat_mul(const double (&a)[4], const double (&b)[4], double (&o)[4]) {
    o[0] = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
    o[1] = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
    o[2] = ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1];
    o[3] = ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0];
}

__device__ __forceinline__ void rg_load4(const float *__restrict__ p, size_t i, double (&o)[4]) {
    const float4 v = *reinterpret_cast<const float4 *>(p + i * 4);
    o[0] = (double)v.x;
    o[1] = (double)v.y;
    o[2] = (double)v.z;
    o[3] = (double)v.w;
}

__device__ __forceinline__ void rg_store4(float *__restrict__ p, size_t i, const double (&v)[4]) {
    *reinterpret_cast<float4 *>(p + i * 4) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

__global__ __launch_bounds__(256) void rg_fwd_kernel(int N, const float *__restrict__ means,
                                                     const float *__restrict__ quats,
                                                     const uint8_t *__restrict__ mask, const float *__restrict__ rt,
                                                     const float *__restrict__ qt, float *__restrict__ means_out,
                                                     float *__restrict__ quats_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const size_t r = (size_t)i;
    if (mask != nullptr && mask[r] == 0) {                        // the row's bytes, whatever they are
        const uint32_t *m = reinterpret_cast<const uint32_t *>(means) + r * 3;
        uint32_t *mo = reinterpret_cast<uint32_t *>(means_out) + r * 3;
        mo[0] = m[0];
        mo[1] = m[1];
        mo[2] = m[2];
        reinterpret_cast<uint4 *>(quats_out)[r] = reinterpret_cast<const uint4 *>(quats)[r];
        return;
    }
    const double x = (double)means[r * 3], y = (double)means[r * 3 + 1], z = (double)means[r * 3 + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        means_out[r * 3 + a] = (float)((((double)rt[a * 4] * x + (double)rt[a * 4 + 1] * y) + (double)rt[a * 4 + 2] * z) +
                                       (double)rt[a * 4 + 3]);
    double t[4], q[4], o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = (double)qt[k];
    rg_load4(quats, r, q);
    rg_quat_mul(t, q, o);
    rg_store4(quats_out, r, o);
}

__global__ __launch_bounds__(RG_ROWS) void rg_bwd_kernel(int N, const float *__restrict__ means,
                                                         const float *__restrict__ quats,
                                                         const uint8_t *__restrict__ mask,
                                                         const float *__restrict__ rt, const float *__restrict__ qt,
                                                         const float *__restrict__ g_means,
                                                         const float *__restrict__ g_quats,
                                                         float *__restrict__ v_means, float *__restrict__ v_quats,
                                                         double *__restrict__ slab) {
    __shared__ double s_w[4][RG_SUMS];
    double v[RG_SUMS];
#pragma unroll
    for (int k = 0; k < RG_SUMS; ++k) v[k] = 0.0;
    const long long i = (long long)blockIdx.x * RG_ROWS + threadIdx.x;
    const size_t r = (size_t)i;
    const bool in = i < N;
    const bool sel = in && (mask == nullptr || mask[r] != 0);
    if (in && !sel) {                                             // copied: the cotangent's bytes, or zeros
        if (v_means != nullptr) {
            uint32_t *o = reinterpret_cast<uint32_t *>(v_means) + r * 3;
            uint32_t g[3] = {0u, 0u, 0u};
            if (g_means != nullptr) {
                const uint32_t *src = reinterpret_cast<const uint32_t *>(g_means) + r * 3;
                g[0] = src[0];
                g[1] = src[1];
                g[2] = src[2];
            }
            o[0] = g[0];
            o[1] = g[1];
            o[2] = g[2];
        }
        if (v_quats != nullptr)
            reinterpret_cast<uint4 *>(v_quats)[r] =
                g_quats ? reinterpret_cast<const uint4 *>(g_quats)[r] : make_uint4(0u, 0u, 0u, 0u);
    }
    if (sel) {
        if (g_means != nullptr) {
            const double g[3] = {(double)g_means[r * 3], (double)g_means[r * 3 + 1], (double)g_means[r * 3 + 2]};
            const double p[3] = {(double)means[r * 3], (double)means[r * 3 + 1], (double)means[r * 3 + 2]};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) v[a * 4 + b] = g[a] * p[b];
                v[a * 4 + 3] = g[a];
            }
            if (v_means != nullptr) {
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    v_means[r * 3 + b] =
                        (float)(((double)rt[b] * g[0] + (double)rt[4 + b] * g[1]) + (double)rt[8 + b] * g[2]);
            }
        } else if (v_means != nullptr) {
            v_means[r * 3] = 0.f;
            v_means[r * 3 + 1] = 0.f;
            v_means[r * 3 + 2] = 0.f;
        }
        if (g_quats != nullptr) {
            double g[4], q[4], c[4], o[4];
            rg_load4(g_quats, r, g);
            rg_load4(quats, r, q);
            c[0] = q[0];
            c[1] = -q[1];
            c[2] = -q[2];
            c[3] = -q[3];
            rg_quat_mul(g, c, o);                                 // g_q (x) conj(q): this row's term of v_qt
#pragma unroll
            for (int k = 0; k < 4; ++k) v[12 + k] = o[k];
            if (v_quats != nullptr) {
                c[0] = (double)qt[0];
                c[1] = -(double)qt[1];
                c[2] = -(double)qt[2];
                c[3] = -(double)qt[3];
                rg_quat_mul(c, g, o);                             // conj(qt) (x) g_q
                rg_store4(v_quats, r, o);
            }
        } else if (v_quats != nullptr) {
            reinterpret_cast<float4 *>(v_quats)[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    double *row = slab + (size_t)RG_SUMS * blockIdx.x;
    if (__syncthreads_or(sel ? 1 : 0) == 0) {                     // workgroup-uniform: nothing selected here
        if (threadIdx.x < RG_SUMS) row[threadIdx.x] = 0.0;
        return;
    }
    gg_block_row<RG_SUMS>(v, s_w, row);
}

// One workgroup: the slab's columns by gg_chain_sum, rounded once.  Columns 0..11 are v_rt, 12..15 v_qt.
__global__ __launch_bounds__(RG_FIN_THREADS) void rg_finish_kernel(int nrows, const double *__restrict__ slab,
                                                                   float *__restrict__ v_rt,
                                                                   float *__restrict__ v_qt) {
    __shared__ double s_c[GG_SUM_CHAINS][RG_SUMS];
    const double t = gg_chain_sum<RG_SUMS, GG_SUM_CHAINS>(nrows, slab, s_c);
    if (threadIdx.x < 12)
        v_rt[threadIdx.x] = (float)t;
    else if (threadIdx.x < RG_SUMS)
        v_qt[threadIdx.x - 12] = (float)t;
}

static int rg_blocks(int N) { return (int)(((long long)N + RG_ROWS - 1) / RG_ROWS); }

static size_t rg_bwd_bytes(int N) {
    const size_t b = gg_align_up((size_t)rg_blocks(N) * RG_SUMS * sizeof(double), 256);
    return b < 256 ? 256 : b;                // never 0 for a count in range: 0 says "out of range"
}

extern "C" size_t gg_rigid_bwd_workspace(int num_points) {
    if (num_points < 0) return 0;
    return rg_bwd_bytes(num_points);
}

#define RG_ALIGNED(p, a) (((uintptr_t)(p) & ((a) - 1)) == 0)

extern "C" int gg_rigid_fwd(int num_points, const float *means, const float *quats, const uint8_t *mask,
                            const float *rt, const float *qt, float *means_out, float *quats_out,
                            gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0, "num_points < 0");
    if (num_points == 0) return GG_OK;
    GG_REQUIRE(means, "null pointer: means");
    GG_REQUIRE(quats, "null pointer: quats");
    GG_REQUIRE(rt, "null pointer: rt");
    GG_REQUIRE(qt, "null pointer: qt");
    GG_REQUIRE(means_out, "null pointer: means_out");
    GG_REQUIRE(quats_out, "null pointer: quats_out");
    GG_REQUIRE(RG_ALIGNED(means, 4), "means misaligned (4 bytes)");
    GG_REQUIRE(RG_ALIGNED(means_out, 4), "means_out misaligned (4 bytes)");
    GG_REQUIRE(RG_ALIGNED(rt, 4), "rt misaligned (4 bytes)");
    GG_REQUIRE(RG_ALIGNED(qt, 4), "qt misaligned (4 bytes)");
    GG_REQUIRE(RG_ALIGNED(quats, 16), "quats misaligned (16 bytes)");
    GG_REQUIRE(RG_ALIGNED(quats_out, 16), "quats_out misaligned (16 bytes)");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rg_fwd_kernel, dim3((unsigned)rg_blocks(num_points)), dim3(256), 0, s, num_points, means,
                       quats, mask, rt, qt, means_out, quats_out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_rigid_bwd(int num_points, const float *means, const float *quats, const uint8_t *mask,
                            const float *rt, const float *qt, const float *g_means, const float *g_quats,
                            float *v_means, float *v_quats, float *v_rt, float *v_qt, void *ws, size_t ws_bytes,
                            gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0, "num_points < 0");
    GG_REQUIRE(v_rt, "null pointer: v_rt");
    GG_REQUIRE(v_qt, "null pointer: v_qt");
    GG_REQUIRE(RG_ALIGNED(v_rt, 4), "v_rt misaligned (4 bytes)");
    GG_REQUIRE(RG_ALIGNED(v_qt, 4), "v_qt misaligned (4 bytes)");
    hipStream_t s = (hipStream_t)stream;
    const int blocks = rg_blocks(num_points);
    if (num_points > 0) {
        GG_REQUIRE(means, "null pointer: means");
        GG_REQUIRE(quats, "null pointer: quats");
        GG_REQUIRE(rt, "null pointer: rt");
        GG_REQUIRE(qt, "null pointer: qt");
        GG_REQUIRE(RG_ALIGNED(means, 4), "means misaligned (4 bytes)");
        GG_REQUIRE(RG_ALIGNED(g_means, 4), "g_means misaligned (4 bytes)");
        GG_REQUIRE(RG_ALIGNED(v_means, 4), "v_means misaligned (4 bytes)");
        GG_REQUIRE(RG_ALIGNED(rt, 4), "rt misaligned (4 bytes)");
        GG_REQUIRE(RG_ALIGNED(qt, 4), "qt misaligned (4 bytes)");
        GG_REQUIRE(RG_ALIGNED(quats, 16), "quats misaligned (16 bytes)");
        GG_REQUIRE(RG_ALIGNED(g_quats, 16), "g_quats misaligned (16 bytes)");
        GG_REQUIRE(RG_ALIGNED(v_quats, 16), "v_quats misaligned (16 bytes)");
        const size_t need = rg_bwd_bytes(num_points);
        GG_REQUIRE_WS(ws, ws_bytes, need);
        hipLaunchKernelGGL(rg_bwd_kernel, dim3((unsigned)blocks), dim3(RG_ROWS), 0, s, num_points, means, quats, mask,
                           rt, qt, g_means, g_quats, v_means, v_quats, (double *)ws);
    }
    // no rows: the slab is not read, the sixteen totals are zeros
    hipLaunchKernelGGL(rg_finish_kernel, dim3(1), dim3(RG_FIN_THREADS), 0, s, blocks, (const double *)ws, v_rt, v_qt);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
