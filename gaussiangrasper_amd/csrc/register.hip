// register.hip — coloured ICP (Park, Zhou, Koltun 2017; the reference's coloricp, scripts/generate_data.py:47-83):
// per-point surface frames of a target cloud, and one Gauss-Newton linearisation of a source cloud against it.
// The contract is in include/gg_raster.h (gg_cloud_frames, gg_icp_step) and PARITY.md "Registration"; the design
// and the measured resource usage in DESIGN.md §3.19.  The per-point arithmetic is in register_math.h.
//
// Both calls sort the target into the uniform grid of grid_sort.h with FILTER (finite points; for gg_icp_step also
// valid != 0) and a cell edge of kn_radius_cell, so the 27 cells around a query hold everything within the radius.
//
// gg_cloud_frames: one lane per sorted slot walks its neighbours three times: count and mean; covariance about the
// mean; the rows of the colour-gradient system.  Slot order within a cell follows the sort's atomics, so the fp64
// sums may differ in their last bits from call to call; count and valid never do.
//
// gg_icp_step: one lane per source point.  The lane moves its point, finds the nearest sorted target (smallest
// (distance, index) pair: no dependence on slot order) and forms the 32 terms of register_math.h.  The terms are
// summed in the fixed orders of ordered_sum.h: one block row of 32 (64 with abs_sums) sums per workgroup of 256
// source points into a slab, then the chains over the slab's rows.  The same inputs give the same bits.
#include <limits.h>
#include <math.h>

#include "gg_common.h"
#include "grid_sort.h"
#include "ordered_sum.h"
#include "register_math.h"

#define RG_FIN_THREADS (GG_SUM_CHAINS * 2 * RG_SUMS)

// ------------------------------------------------------------------------------------------------
// surface frames
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_frames_init_kernel(int n, float *__restrict__ normals,
                                                             float *__restrict__ gradients,
                                                             int32_t *__restrict__ count,
                                                             uint8_t *__restrict__ valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < 3; ++k) {
        normals[3 * (size_t)i + k] = NAN;
        gradients[3 * (size_t)i + k] = 0.0f;
    }
    count[i] = 0;
    valid[i] = 0;
}

__global__ __launch_bounds__(256) void rg_frames_kernel(int n, const int64_t *__restrict__ total, KnGrid G,
                                                        const int32_t *__restrict__ start,
                                                        const int32_t *__restrict__ counts,
                                                        const float4 *__restrict__ sorted,
                                                        const float *__restrict__ intensity, double r2,
                                                        float *__restrict__ normals, float *__restrict__ gradients,
                                                        int32_t *__restrict__ count, uint8_t *__restrict__ valid) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= n || slot >= *total) return;
    const float4 q = sorted[slot];
    const int id = __float_as_int(q.w);
    const double p[3] = {(double)q.x, (double)q.y, (double)q.z};
    int c = 0;
    double sum[3] = {0.0, 0.0, 0.0};
    kn_ball(G, start, counts, sorted, p[0], p[1], p[2], r2, [&](int, const float4 &o, double) {
        ++c;
        sum[0] += (double)o.x;
        sum[1] += (double)o.y;
        sum[2] += (double)o.z;
    });
    count[id] = c;
    if (c < 3) return;                               // normal NaN, gradient 0, valid 0 from the init kernel
    const double mean[3] = {sum[0] / (double)c, sum[1] / (double)c, sum[2] / (double)c};
    double cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    kn_ball(G, start, counts, sorted, p[0], p[1], p[2], r2, [&](int, const float4 &o, double) {
        const double x = (double)o.x - mean[0], y = (double)o.y - mean[1], z = (double)o.z - mean[2];
        cov[0] += x * x;
        cov[1] += x * y;
        cov[2] += x * z;
        cov[3] += y * y;
        cov[4] += y * z;
        cov[5] += z * z;
    });
    double nrm[3];
    rg_smallest_eigvec(cov, nrm);
    double d[3] = {0.0, 0.0, 0.0};
    if (c >= 4) {
        const double ii = (double)intensity[id];
        double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, rhs[3] = {0.0, 0.0, 0.0}, tr = 0.0;
        kn_ball(G, start, counts, sorted, p[0], p[1], p[2], r2, [&](int, const float4 &o, double) {
            const int jd = __float_as_int(o.w);
            if (jd == id) return;
            const double u[3] = {(double)o.x - p[0], (double)o.y - p[1], (double)o.z - p[2]};
            const double un = rg_dot(u, nrm);
            const double a[3] = {u[0] - un * nrm[0], u[1] - un * nrm[1], u[2] - un * nrm[2]};
            const double b = (double)intensity[jd] - ii;
            m[0] += a[0] * a[0];
            m[1] += a[0] * a[1];
            m[2] += a[0] * a[2];
            m[3] += a[1] * a[1];
            m[4] += a[1] * a[2];
            m[5] += a[2] * a[2];
            rhs[0] += a[0] * b;
            rhs[1] += a[1] * b;
            rhs[2] += a[2] * b;
            tr += rg_dot(a, a);
        });
        const double k = (double)(c - 1);
        const double kn[3] = {k * nrm[0], k * nrm[1], k * nrm[2]};
        m[0] += kn[0] * kn[0];
        m[1] += kn[0] * kn[1];
        m[2] += kn[0] * kn[2];
        m[3] += kn[1] * kn[1];
        m[4] += kn[1] * kn[2];
        m[5] += kn[2] * kn[2];
        double x[3];
        const double det = rg_solve_sym3(m, rhs, x);
        if (!rg_gradient_singular(det, k, tr)) {
            d[0] = x[0];
            d[1] = x[1];
            d[2] = x[2];
        }
    }
    for (int k = 0; k < 3; ++k) {
        normals[3 * (size_t)id + k] = (float)nrm[k];
        gradients[3 * (size_t)id + k] = (float)d[k];
    }
    valid[id] = 1;
}

extern "C" size_t gg_cloud_frames_workspace(int num_points, const int32_t *dims) {
    if (num_points < 1 || num_points > GG_REGISTER_MAX_POINTS || !kn_dims_ok(dims)) return 0;
    return kn_layout(num_points, dims, nullptr, nullptr) + 256;
}

extern "C" int gg_cloud_frames(int num_points, const float *points, const float *intensity, double radius,
                               const double *grid, const int32_t *dims, float *normals, float *gradients,
                               int32_t *count, uint8_t *valid, void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(num_points >= 1 && num_points <= GG_REGISTER_MAX_POINTS, "need 1 <= num_points <= GG_REGISTER_MAX_POINTS");
    GG_REQUIRE(isfinite(radius) && radius > 0.0, "radius must be finite and > 0");
    GG_REQUIRE_GRID(grid, dims);
    GG_REQUIRE(points && intensity && normals && gradients && count && valid, "null pointer");
    GG_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)intensity & 3) == 0 && ((uintptr_t)normals & 3) == 0 &&
                   ((uintptr_t)gradients & 3) == 0 && ((uintptr_t)count & 3) == 0,
               "points / intensity / normals / gradients / count misaligned");
    const size_t sort_bytes = kn_layout(num_points, dims, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, sort_bytes + 256);
    const KnGrid G = kn_grid(grid, dims, radius);
    GG_REQUIRE(isfinite(G.cell) && isfinite(radius * radius), "radius too large");
    KnWs w;
    kn_layout(num_points, dims, &w, (char *)ws);
    int64_t *total = (int64_t *)((char *)ws + sort_bytes);
    const unsigned pb = (unsigned)((num_points + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    gg_prof_begin(GG_K_CLOUD_FRAMES, s);
    hipLaunchKernelGGL(rg_frames_init_kernel, dim3(pb), dim3(256), 0, s, num_points, normals, gradients, count, valid);
    GG_REQUIRE_FILL(GG_K_CLOUD_FRAMES, s, kn_sort<true>(num_points, points, nullptr, G, w, total, s));
    hipLaunchKernelGGL(rg_frames_kernel, dim3(pb), dim3(256), 0, s, num_points, total, G, w.start, w.counts, w.sorted,
                       intensity, radius * radius, normals, gradients, count, valid);
    gg_prof_end(GG_K_CLOUD_FRAMES, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------
// one Gauss-Newton linearisation
// ------------------------------------------------------------------------------------------------
struct RgPose {
    double m[12];
};

// slab row of this block (gg_block_row): W = 32 sums, or 64 with the sums of absolute values behind them
template <bool ABS>
__global__ __launch_bounds__(256) void rg_step_kernel(int m, const float *__restrict__ source,
                                                      const float *__restrict__ source_intensity, RgPose T, KnGrid G,
                                                      const int32_t *__restrict__ start,
                                                      const int32_t *__restrict__ counts,
                                                      const float4 *__restrict__ sorted,
                                                      const float *__restrict__ intensity,
                                                      const float *__restrict__ normals,
                                                      const float *__restrict__ gradients, double md2, double wg,
                                                      double wp, int32_t *__restrict__ corr,
                                                      double *__restrict__ slab) {
    constexpr int W = ABS ? 2 * RG_SUMS : RG_SUMS;
    __shared__ double s_w[4][W];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v[W];
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = 0.0;
    if (i < m) {
        const double x = (double)source[3 * (size_t)i], y = (double)source[3 * (size_t)i + 1],
                     z = (double)source[3 * (size_t)i + 2];
        double s[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) s[r] = ((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3];
        double best = INFINITY;
        int bi = INT_MAX;
        float4 bq = make_float4(0.f, 0.f, 0.f, 0.f);
        // x - x is 0 for a finite x and NaN for NaN and +-inf
        if ((s[0] - s[0]) + (s[1] - s[1]) + (s[2] - s[2]) == 0.0)
            kn_ball(G, start, counts, sorted, s[0], s[1], s[2], md2, [&](int, const float4 &o, double d2) {
                const int jd = __float_as_int(o.w);
                if (d2 < best || (d2 == best && jd < bi)) {
                    best = d2;
                    bi = jd;
                    bq = o;
                }
            });
        const bool hit = bi != INT_MAX;
        if (corr) corr[i] = hit ? bi : -1;
        if (hit) {
            const double q[3] = {(double)bq.x, (double)bq.y, (double)bq.z};
            double n[3], d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                n[k] = (double)normals[3 * (size_t)bi + k];
                d[k] = (double)gradients[3 * (size_t)bi + k];
            }
            rg_terms(s, q, n, d, (double)source_intensity[i], (double)intensity[bi], best, wg, wp, v,
                     ABS ? v + RG_SUMS : nullptr);
        }
    }
    gg_block_row<W>(v, s_w, slab + (size_t)W * blockIdx.x);
}

// One workgroup: the slab's columns by gg_chain_sum.  RG_FIN_THREADS lanes for either W: 2 RG_SUMS lanes per chain.
template <bool ABS>
__global__ __launch_bounds__(RG_FIN_THREADS) void rg_finish_kernel(int nrows, const double *__restrict__ slab,
                                                                   double *__restrict__ sums,
                                                                   double *__restrict__ abs_sums) {
    constexpr int W = ABS ? 2 * RG_SUMS : RG_SUMS;
    __shared__ double s_c[GG_SUM_CHAINS][W];
    const double a = gg_chain_sum<W, GG_SUM_CHAINS, 2 * RG_SUMS>(nrows, slab, s_c);
    if (threadIdx.x < RG_SUMS)
        sums[threadIdx.x] = a;
    else if (threadIdx.x < W)
        abs_sums[threadIdx.x - RG_SUMS] = a;
}

static size_t rg_step_layout(int num_source, int num_target, const int32_t *dims, size_t *sort_bytes) {
    const size_t sb = kn_layout(num_target, dims, nullptr, nullptr);
    if (sort_bytes) *sort_bytes = sb;
    const size_t blocks = ((size_t)num_source + 255) / 256;
    return sb + 256 + gg_align_up(blocks * 2 * RG_SUMS * sizeof(double), 256);
}

extern "C" size_t gg_icp_step_workspace(int num_source, int num_target, const int32_t *dims) {
    if (num_source < 1 || num_source > GG_REGISTER_MAX_POINTS || num_target < 1 ||
        num_target > GG_REGISTER_MAX_POINTS || !kn_dims_ok(dims))
        return 0;
    return rg_step_layout(num_source, num_target, dims, nullptr);
}

extern "C" int gg_icp_step(int num_source, const float *source, const float *source_intensity, int num_target,
                           const float *points, const float *intensity, const float *normals, const float *gradients,
                           const uint8_t *valid, const double *grid, const int32_t *dims, const double *transform,
                           double max_dist, double lambda_geometric, int reuse_sort, double *sums, double *abs_sums,
                           int32_t *corr, void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(num_source >= 1 && num_source <= GG_REGISTER_MAX_POINTS, "need 1 <= num_source <= GG_REGISTER_MAX_POINTS");
    GG_REQUIRE(num_target >= 1 && num_target <= GG_REGISTER_MAX_POINTS, "need 1 <= num_target <= GG_REGISTER_MAX_POINTS");
    GG_REQUIRE(isfinite(max_dist) && max_dist > 0.0 && isfinite(max_dist * max_dist),
               "max_dist must be finite and > 0");
    GG_REQUIRE(lambda_geometric >= 0.0 && lambda_geometric <= 1.0, "lambda_geometric must be in [0, 1]");
    GG_REQUIRE_GRID(grid, dims);
    GG_REQUIRE(source && source_intensity && points && intensity && normals && gradients && valid && transform && sums,
               "null pointer");
    for (int k = 0; k < 12; ++k) GG_REQUIRE(isfinite(transform[k]), "transform must be finite");
    GG_REQUIRE(((uintptr_t)source & 3) == 0 && ((uintptr_t)source_intensity & 3) == 0 && ((uintptr_t)points & 3) == 0 &&
                   ((uintptr_t)intensity & 3) == 0 && ((uintptr_t)normals & 3) == 0 &&
                   ((uintptr_t)gradients & 3) == 0 && ((uintptr_t)corr & 3) == 0 && ((uintptr_t)sums & 7) == 0 &&
                   ((uintptr_t)abs_sums & 7) == 0,
               "source / source_intensity / points / intensity / normals / gradients / corr / sums / abs_sums "
               "misaligned");
    size_t sort_bytes = 0;
    const size_t need = rg_step_layout(num_source, num_target, dims, &sort_bytes);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    const KnGrid G = kn_grid(grid, dims, max_dist);
    GG_REQUIRE(isfinite(G.cell), "max_dist too large for the grid");
    KnWs w;
    kn_layout(num_target, dims, &w, (char *)ws);
    int64_t *total = (int64_t *)((char *)ws + sort_bytes);
    double *slab = (double *)((char *)ws + sort_bytes + 256);
    RgPose T;
    for (int k = 0; k < 12; ++k) T.m[k] = transform[k];
    const double wg = sqrt(lambda_geometric), wp = sqrt(1.0 - lambda_geometric);
    const int blocks = (num_source + 255) / 256;
    hipStream_t s = (hipStream_t)stream;
    gg_prof_begin(GG_K_ICP_STEP, s);
    if (!reuse_sort) GG_REQUIRE_FILL(GG_K_ICP_STEP, s, kn_sort<true>(num_target, points, valid, G, w, total, s));
    if (abs_sums) {
        hipLaunchKernelGGL(rg_step_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, num_source, source,
                           source_intensity, T, G, w.start, w.counts, w.sorted, intensity, normals, gradients,
                           max_dist * max_dist, wg, wp, corr, slab);
        hipLaunchKernelGGL(rg_finish_kernel<true>, dim3(1), dim3(RG_FIN_THREADS), 0, s, blocks, slab, sums, abs_sums);
    } else {
        hipLaunchKernelGGL(rg_step_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, num_source, source,
                           source_intensity, T, G, w.start, w.counts, w.sorted, intensity, normals, gradients,
                           max_dist * max_dist, wg, wp, corr, slab);
        hipLaunchKernelGGL(rg_finish_kernel<false>, dim3(1), dim3(RG_FIN_THREADS), 0, s, blocks, slab, sums, abs_sums);
    }
    gg_prof_end(GG_K_ICP_STEP, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
