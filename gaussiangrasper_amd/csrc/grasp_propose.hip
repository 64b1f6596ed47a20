// grasp_propose.hip — antipodal parallel-jaw grasp candidates from oriented points: for every seed point, the two
// farthest points of the object inside a thin tube around the seed's normal line are the finger contacts; a seed
// whose contacts are a gripper's width apart and face along the line yields K GraspGroup rows, one per approach
// direction around the closing axis.  The contract is in include/gg_raster.h (gg_grasp_propose) and PARITY.md
// "Grasp proposals"; the design in DESIGN.md §3.17.
//
// Per usable seed (index in range, point taking part, n.n > 0), fp64 from the fp32 inputs, no contraction:
//   nn = (n0 n0 + n1 n1) + n2 n2;  per point j taking part: d = p_j - p, s = (n0 d0 + n1 d1) + n2 d2,
//   dd = (d0 d0 + d1 d1) + d2 d2;  in the tube iff dd nn - s s <= (r r) nn and s s <= (W W) nn;
//   (s_lo, j_lo) / (s_hi, j_hi) the extremes of s over the tube (smallest index on a tie), tube_count their number;
//   valid iff q = s_hi - s_lo has (w0 w0) nn <= q q <= ((W - 2c)(W - 2c)) nn and both contact normals pass
//   g g >= (min_align min_align)(nn m), m > 0.  No square root and no division decides anything.
// Tiling (grasp.hip's): one lane per seed, GC_TILE seeds per workgroup (grid.y), the seed's fp64 state in registers;
// grid.x splits the points into C chunks of `len` points, a multiple of GC_STAGE, staged through LDS GC_STAGE at a
// time and read as broadcasts, walked in increasing index order.
// Cull: the tube lies in the fp32 box |x_k - p_k| <= W |b_k| + r, widened by GC_MARGIN (W + r + |p_k|) and rounded
// outward (gp_load); six fp32 compares per pair, only pairs inside take the fp64 test.  The widening is ~1e9 times
// the fp64 test's rounding, so the cull never changes a decision.  A point that takes no part is staged as NaN.
// Determinism: no atomics.  Each (chunk, seed) writes (count, s_lo, j_lo, s_hi, j_hi); propose_reduce_kernel
// combines the C partials in chunk order with strict < / >: min, max, the smallest index reaching them and an
// integer count are the same for every chunking, so the result does not depend on the launch geometry.
// propose_rows_kernel then writes the K rows of each seed, one thread per row.
#include "grasp_common.h"

#define GP_FRAME 14              // per-seed frame in ws: m (3), b (3), a_0 (3), c_0 (3), width, score

struct GpParams {
    double r, W, c, depth, height, min_weight;
    double rr, ww, w0w0, wcwc, aa;       // r r, W W, w0 w0, (W - 2c)(W - 2c), min_align min_align
    double up[3];
    int K;
};

struct GpSeed {
    double p[3], n[3], nn, rrnn, wwnn;
    float lo[3], hi[3];          // fp32 cull box: empty for a seed that is not usable
    bool usable;
};

struct GpWs {
    int *cnt, *jlo, *jhi;        // [C][S]
    double *slo, *shi;           // [C][S]
    double *frame;               // [S][GP_FRAME]
};

// `idx` is the seed's point index, or any value outside [0, N) for a lane past the last seed.
__device__ void gp_load(int idx, int N, const float *__restrict__ points, const float *__restrict__ normals,
                        const float *__restrict__ weights, const GpParams &P, bool box, GpSeed &g) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.p[k] = 0.0;
        g.n[k] = 0.0;
        g.lo[k] = INFINITY;
        g.hi[k] = -INFINITY;
    }
    g.nn = g.rrnn = g.wwnn = 0.0;
    g.usable = false;
    const size_t i3 = (size_t)idx * 3;
    if (idx < 0 || idx >= N || !gc_part(points + i3, normals + i3, weights[idx], P.min_weight)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.p[k] = (double)points[i3 + k];
        g.n[k] = (double)normals[i3 + k];
    }
    g.nn = (g.n[0] * g.n[0] + g.n[1] * g.n[1]) + g.n[2] * g.n[2];
    if (!(g.nn > 0.0)) return;
    g.usable = true;
    g.rrnn = P.rr * g.nn;
    g.wwnn = P.ww * g.nn;
    if (!box) return;
    const double sq = sqrt(g.nn);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double e = P.W * (fabs(g.n[k]) / sq) + P.r;
        const double w = e + GC_MARGIN * ((P.W + P.r) + fabs(g.p[k]));
        const bool fin = isfinite(w);
        g.lo[k] = fin ? gc_down(g.p[k] - w) : -INFINITY;
        g.hi[k] = fin ? gc_up(g.p[k] + w) : INFINITY;
    }
}

__global__ __launch_bounds__(GC_TILE) void propose_search_kernel(int N, const float *__restrict__ points,
                                                                 const float *__restrict__ normals,
                                                                 const float *__restrict__ weights, int S,
                                                                 const int32_t *__restrict__ seeds, GpParams P,
                                                                 int len, GpWs ws) {
    __shared__ float4 s_p[GC_STAGE];
    const int g = blockIdx.y * blockDim.x + threadIdx.x;
    GpSeed G;
    gp_load(g < S ? seeds[g] : -1, N, points, normals, weights, P, true, G);
    int cnt = 0, jlo = -1, jhi = -1;
    double slo = INFINITY, shi = -INFINITY;
    const int i0 = blockIdx.x * len, i1 = min(N, i0 + len);
    for (int s0 = i0; s0 < i1; s0 += GC_STAGE) {
        const int ns = min(GC_STAGE, i1 - s0);
        gc_stage(s0, ns, points, normals, weights, P.min_weight, s_p, nullptr);
        __syncthreads();
        for (int k = 0; k < ns; ++k) {
            const float4 a = s_p[k];
            if (!gc_in_box(G.lo, G.hi, a)) continue;
            const double d0 = (double)a.x - G.p[0], d1 = (double)a.y - G.p[1], d2 = (double)a.z - G.p[2];
            const double s = (G.n[0] * d0 + G.n[1] * d1) + G.n[2] * d2;
            const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
            const double ss = s * s;
            if (!(dd * G.nn - ss <= G.rrnn && ss <= G.wwnn)) continue;
            ++cnt;
            if (s < slo) {
                slo = s;
                jlo = s0 + k;
            }
            if (s > shi) {
                shi = s;
                jhi = s0 + k;
            }
        }
        __syncthreads();
    }
    if (g < S) {
        const size_t o = (size_t)blockIdx.x * S + g;
        ws.cnt[o] = cnt;
        ws.jlo[o] = jlo;
        ws.jhi[o] = jhi;
        ws.slo[o] = slo;
        ws.shi[o] = shi;
    }
}

// g = n . n_j, m = n_j . n_j of contact j; align iff m > 0 and g g >= aa (nn m)
__device__ __forceinline__ bool gp_align(const GpSeed &G, int j, const float *__restrict__ normals, double aa,
                                         double &gj, double &mj) {
    gj = mj = 0.0;
    if (j < 0) return false;
    const double a0 = (double)normals[(size_t)j * 3], a1 = (double)normals[(size_t)j * 3 + 1],
                 a2 = (double)normals[(size_t)j * 3 + 2];
    gj = (G.n[0] * a0 + G.n[1] * a1) + G.n[2] * a2;
    mj = (a0 * a0 + a1 * a1) + a2 * a2;
    return mj > 0.0 && gj * gj >= aa * (G.nn * mj);
}

// Per seed, in chunk order: contacts, count, span and validity; the frame of a valid seed goes to ws.frame.
__global__ __launch_bounds__(256) void propose_reduce_kernel(int N, const float *__restrict__ points,
                                                            const float *__restrict__ normals,
                                                            const float *__restrict__ weights, int S,
                                                            const int32_t *__restrict__ seeds, GpParams P, int C,
                                                            GpWs ws, int32_t *__restrict__ pair_idx,
                                                            int32_t *__restrict__ tube_count,
                                                            float *__restrict__ span, uint8_t *__restrict__ valid) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= S) return;
    GpSeed G;
    gp_load(seeds[g], N, points, normals, weights, P, false, G);
    int cnt = 0, jlo = -1, jhi = -1;
    double slo = INFINITY, shi = -INFINITY;
    for (int c = 0; c < C; ++c) {
        const size_t o = (size_t)c * S + g;
        if (!ws.cnt[o]) continue;
        cnt += ws.cnt[o];
        if (ws.slo[o] < slo) {
            slo = ws.slo[o];
            jlo = ws.jlo[o];
        }
        if (ws.shi[o] > shi) {
            shi = ws.shi[o];
            jhi = ws.jhi[o];
        }
    }
    if (!G.usable || cnt == 0) {
        pair_idx[2 * (size_t)g] = -1;
        pair_idx[2 * (size_t)g + 1] = -1;
        tube_count[g] = 0;
        span[g] = NAN;
        valid[g] = 0;
        return;
    }
    const double q = shi - slo, qq = q * q, sq = sqrt(G.nn);
    double glo, mlo, ghi, mhi;
    const bool al = gp_align(G, jlo, normals, P.aa, glo, mlo), ah = gp_align(G, jhi, normals, P.aa, ghi, mhi);
    const bool ok = qq >= P.w0w0 * G.nn && qq <= P.wcwc * G.nn && al && ah;
    const double sp = q / sq;
    pair_idx[2 * (size_t)g] = jlo;
    pair_idx[2 * (size_t)g + 1] = jhi;
    tube_count[g] = cnt;
    span[g] = (float)sp;
    valid[g] = ok ? 1 : 0;
    if (!ok) return;
    double b[3], m[3], v[3], e[3];
    const double mid = (slo + shi) / (2.0 * sq);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b[k] = G.n[k] / sq;
        m[k] = G.p[k] + b[k] * mid;
        v[k] = -P.up[k];
    }
    double bv = (b[0] * v[0] + b[1] * v[1]) + b[2] * v[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = v[k] - b[k] * bv;
    double ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    const double vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (ee < 1e-12 * vv) {       // b parallel to up: approach along the coordinate axis least aligned with b
        int ax = 0;
        if (fabs(b[1]) < fabs(b[ax])) ax = 1;
        if (fabs(b[2]) < fabs(b[ax])) ax = 2;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = k == ax ? 1.0 : 0.0;
        bv = (b[0] * v[0] + b[1] * v[1]) + b[2] * v[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = v[k] - b[k] * bv;
        ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    }
    const double le = sqrt(ee);
    const double a0 = e[0] / le, a1 = e[1] / le, a2 = e[2] / le;
    double *f = ws.frame + (size_t)g * GP_FRAME;
    f[0] = m[0];
    f[1] = m[1];
    f[2] = m[2];
    f[3] = b[0];
    f[4] = b[1];
    f[5] = b[2];
    f[6] = a0;
    f[7] = a1;
    f[8] = a2;
    f[9] = a1 * b[2] - a2 * b[1];        // c_0 = a_0 x b
    f[10] = a2 * b[0] - a0 * b[2];
    f[11] = a0 * b[1] - a1 * b[0];
    f[12] = sp + 2.0 * P.c;
    f[13] = (fabs(glo) * fabs(ghi)) / (G.nn * sqrt(mlo * mhi));
}

// One thread per (seed, approach): row = [score, width, height, depth, R (a_k, b, c_k as columns), t_k, 0].
__global__ __launch_bounds__(256) void propose_rows_kernel(int S, GpParams P, const double *__restrict__ frame,
                                                          const uint8_t *__restrict__ valid,
                                                          float *__restrict__ rows) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)S * P.K) return;
    const size_t g = t / P.K;
    const int k = (int)(t % P.K);
    float *o = rows + t * GC_ROW;
    if (!valid[g]) {
#pragma unroll
        for (int i = 0; i < GC_ROW; ++i) o[i] = NAN;
        return;
    }
    const double *f = frame + g * GP_FRAME;
    const double phi = (2.0 * M_PI * (double)k) / (double)P.K;
    const double cs = cos(phi), sn = sin(phi);
    const double b0 = f[3], b1 = f[4], b2 = f[5];
    const double a0 = cs * f[6] + sn * f[9], a1 = cs * f[7] + sn * f[10], a2 = cs * f[8] + sn * f[11];
    const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
    const double h = 0.5 * P.depth;
    o[0] = (float)f[13];
    o[1] = (float)f[12];
    o[2] = (float)P.height;
    o[3] = (float)P.depth;
    o[4] = (float)a0;
    o[5] = (float)b0;
    o[6] = (float)c0;
    o[7] = (float)a1;
    o[8] = (float)b1;
    o[9] = (float)c1;
    o[10] = (float)a2;
    o[11] = (float)b2;
    o[12] = (float)c2;
    o[13] = (float)(f[0] - h * a0);
    o[14] = (float)(f[1] - h * a1);
    o[15] = (float)(f[2] - h * a2);
    o[16] = 0.0f;
}

static size_t gp_layout(int N, int S, GpWs *w, char *base) {
    int C, len;
    gc_chunks(N, S, &C, &len);
    const size_t cs = (size_t)C * S;
    GgCarve cv{base, 0};
    GpWs t;
    t.cnt = (int *)cv.take(cs * 4);
    t.jlo = (int *)cv.take(cs * 4);
    t.jhi = (int *)cv.take(cs * 4);
    t.slo = (double *)cv.take(cs * 8);
    t.shi = (double *)cv.take(cs * 8);
    t.frame = (double *)cv.take((size_t)S * GP_FRAME * 8);
    if (w) *w = t;
    return cv.off;
}

extern "C" size_t gg_grasp_propose_workspace(int num_points, int num_seeds) {
    if (num_points < 0 || num_points > GG_GRASP_MAX_POINTS || num_seeds <= 0 || num_seeds > GG_PROPOSE_MAX_SEEDS)
        return 0;
    return gp_layout(num_points, num_seeds, nullptr, nullptr);
}

extern "C" int gg_grasp_propose(int num_points, const float *points, const float *normals, const float *weights,
                                int num_seeds, const int32_t *seeds, double tube_radius, double max_width,
                                double min_width, double clearance, double depth, double height, double min_weight,
                                double min_align, const double *up, int num_approach, int32_t *pair_idx,
                                int32_t *tube_count, float *span, uint8_t *valid, float *rows, void *ws,
                                size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0, "num_points < 0");
    GG_REQUIRE(num_seeds >= 0, "num_seeds < 0");
    GG_REQUIRE(num_points <= GG_GRASP_MAX_POINTS, "num_points > GG_GRASP_MAX_POINTS");
    GG_REQUIRE(num_seeds <= GG_PROPOSE_MAX_SEEDS, "num_seeds > GG_PROPOSE_MAX_SEEDS");
    GG_REQUIRE(isfinite(tube_radius) && tube_radius >= 0.0, "tube_radius must be finite and >= 0");
    GG_REQUIRE(isfinite(max_width) && max_width > 0.0, "max_width must be finite and > 0");
    GG_REQUIRE(isfinite(min_width) && min_width >= 0.0, "min_width must be finite and >= 0");
    GG_REQUIRE(isfinite(clearance) && clearance >= 0.0 && 2.0 * clearance <= max_width,
               "clearance must be finite, >= 0 and at most max_width / 2");
    GG_REQUIRE(isfinite(depth) && depth >= 0.0, "depth must be finite and >= 0");
    GG_REQUIRE(isfinite(height) && height > 0.0, "height must be finite and > 0");
    GG_REQUIRE(!isnan(min_weight), "min_weight is NaN");
    GG_REQUIRE(min_align >= 0.0 && min_align <= 1.0, "min_align must be in [0, 1]");
    GG_REQUIRE(up != nullptr, "null pointer: up");
    GG_REQUIRE(isfinite(up[0]) && isfinite(up[1]) && isfinite(up[2]) && (up[0] != 0.0 || up[1] != 0.0 || up[2] != 0.0),
               "up must be finite and not zero");
    GG_REQUIRE(num_approach >= 1 && num_approach <= GG_PROPOSE_MAX_APPROACH,
               "num_approach must be in 1..GG_PROPOSE_MAX_APPROACH");
    if (num_seeds == 0) return GG_OK;
    GG_REQUIRE(seeds && pair_idx && tube_count && span && valid && rows, "null pointer: seeds / outputs");
    GG_REQUIRE(num_points == 0 || (points && normals && weights), "null pointer: points / normals / weights");
    GG_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)normals & 3) == 0 && ((uintptr_t)weights & 3) == 0 &&
                   ((uintptr_t)seeds & 3) == 0,
               "points / normals / weights / seeds misaligned");
    GG_REQUIRE((((uintptr_t)pair_idx | (uintptr_t)tube_count | (uintptr_t)span | (uintptr_t)rows) & 3) == 0,
               "pair_idx / tube_count / span / rows misaligned");
    const size_t need = gp_layout(num_points, num_seeds, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    GpWs w;
    gp_layout(num_points, num_seeds, &w, (char *)ws);
    int C, len;
    gc_chunks(num_points, num_seeds, &C, &len);
    GpParams P;
    P.r = tube_radius;
    P.W = max_width;
    P.c = clearance;
    P.depth = depth;
    P.height = height;
    P.min_weight = min_weight;
    P.rr = tube_radius * tube_radius;
    P.ww = max_width * max_width;
    P.w0w0 = min_width * min_width;
    const double wc = max_width - 2.0 * clearance;
    P.wcwc = wc * wc;
    P.aa = min_align * min_align;
    P.up[0] = up[0];
    P.up[1] = up[1];
    P.up[2] = up[2];
    P.K = num_approach;
    hipStream_t s = (hipStream_t)stream;
    const int S = num_seeds;
    dim3 grid, block;
    gc_launch_shape(C, S, &grid, &block);
    const size_t nrows = (size_t)S * num_approach;
    gg_prof_begin(GG_K_GRASP_PROPOSE, s);
    if (C > 0)
        hipLaunchKernelGGL(propose_search_kernel, grid, block, 0, s, num_points, points, normals, weights, S,
                           seeds, P, len, w);
    hipLaunchKernelGGL(propose_reduce_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, num_points, points,
                       normals, weights, S, seeds, P, C, w, pair_idx, tube_count, span, valid);
    hipLaunchKernelGGL(propose_rows_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, s, S, P, w.frame,
                       valid, rows);
    gg_prof_end(GG_K_GRASP_PROPOSE, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
