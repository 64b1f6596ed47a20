// grasp.hip — normal-guided grasp filtering (GaussianGrasper step 4) against oriented points: for every grasp
// candidate (graspnetAPI GraspGroup row), the contacts of the two fingers with the points between them, the
// outward patch normals there, their angles to the closing direction, and the friction-cone test.  The contract is
// in include/gg_raster.h (gg_grasp_contacts) and PARITY.md "Grasp filtering"; the design in DESIGN.md §3.12.
//
// Tiling: one lane per grasp, GC_TILE grasps per workgroup (grid.y), each lane holding its grasp's fp64 frame in
// registers; grid.x splits the points into C chunks of `len` points, a multiple of GC_STAGE, staged through LDS
// GC_STAGE at a time and read as broadcasts.  Every lane walks the staged points in increasing index order.
// Cull: each grasp's region + finger boxes are bounded by a world-space fp32 box (gc_cull_box: fp64 inverse of R,
// half-extents widened by GC_MARGIN relative, bounds rounded outward), tested with six fp32 compares per pair;
// only pairs inside it take the fp64 test.  A point that takes no part is staged as NaN and fails every compare.
// Determinism: no atomics.  Each (chunk, grasp) writes its partial state; a per-grasp kernel combines the C
// partials in chunk order (strict < / > keeps the earliest chunk, the lanes' strict < / > the earliest index in a
// chunk: the smallest index wins), and fp64 sums are added in chunk order.  C depends on (N, M) only.
// Two passes over the points, because the patches need the contacts: pass 1 (region count, contacts, weights),
// reduce, pass 2 (patch normal sums), finalize.
#include "grasp_common.h"

struct GcParams {
    double depth_base, finger_width, band, min_weight, max_collision, max_angle;
};

struct GcGrasp {
    double R[9], t[3];           // R row-major: column 0 approach a, 1 closing b, 2 height c
    double depth, hw, hh, lo1, hi1;
    float lo[3], hi[3];          // fp32 cull box: empty for a grasp that is not valid
};

// `row` may be null (a lane past the last grasp): the grasp is then not valid.
__device__ void gc_load(const float *row, const GcParams &P, GcGrasp &g) {
    float v[GC_ROW];
    bool ok = row != nullptr;
#pragma unroll
    for (int k = 0; k < GC_ROW; ++k) {
        v[k] = row ? row[k] : 0.0f;
        ok = ok && isfinite(v[k]);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) g.R[k] = (double)v[4 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) g.t[k] = (double)v[13 + k];
    g.depth = (double)v[3];
    g.hw = 0.5 * (double)v[1];
    g.hh = 0.5 * (double)v[2];
    g.lo1 = -g.hw - P.finger_width;
    g.hi1 = g.hw + P.finger_width;
    ok = ok && v[1] > 0.0f && v[2] > 0.0f && g.depth >= -P.depth_base;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.lo[k] = INFINITY;
        g.hi[k] = -INFINITY;
    }
    if (!ok) return;
    // the local box is u0 in [-d_base, depth], |u1| <= hi1, |u2| <= hh (region and both finger boxes)
    const double m[3] = {0.5 * (g.depth - P.depth_base), 0.0, 0.0};
    const double h[3] = {0.5 * (g.depth + P.depth_base), g.hi1, g.hh};
    gc_cull_box(g.R, g.t, m, h, g.lo, g.hi);
}

struct GcWs {
    int *cnt, *il, *ir;          // [C][M]
    double *yl, *yr, *rw, *cw;   // [C][M]
    double *nrm;                 // [6][C][M]: N_L xyz, N_R xyz
    int *gcnt;                   // [M]
    double *gyl, *gyr, *gcw;     // [M]
};

__global__ __launch_bounds__(GC_TILE) void grasp_pass1_kernel(int N, const float *__restrict__ points,
                                                              const float *__restrict__ normals,
                                                              const float *__restrict__ weights, int M,
                                                              const float *__restrict__ grasps, GcParams P, int len,
                                                              GcWs ws) {
    __shared__ float4 s_p[GC_STAGE];
    const int g = blockIdx.y * blockDim.x + threadIdx.x;
    GcGrasp G;
    gc_load(g < M ? grasps + (size_t)g * GC_ROW : nullptr, P, G);
    const double nb = -P.depth_base;
    int cnt = 0, il = -1, ir = -1;
    double yl = INFINITY, yr = -INFINITY, rw = 0.0, cw = 0.0;
    const int i0 = blockIdx.x * len, i1 = min(N, i0 + len);
    for (int s0 = i0; s0 < i1; s0 += GC_STAGE) {
        const int ns = min(GC_STAGE, i1 - s0);
        gc_stage(s0, ns, points, normals, weights, P.min_weight, s_p, nullptr);
        __syncthreads();
        for (int k = 0; k < ns; ++k) {
            const float4 a = s_p[k];
            if (!gc_in_box(G.lo, G.hi, a)) continue;
            double u0, u1, u2;
            gc_local(G.R, G.t, a, u0, u1, u2);
            if (!(u0 >= nb && u0 <= G.depth && fabs(u2) <= G.hh)) continue;
            const double w = (double)a.w;
            if (fabs(u1) <= G.hw) {
                ++cnt;
                rw += w;
                if (u1 < yl) {
                    yl = u1;
                    il = s0 + k;
                }
                if (u1 > yr) {
                    yr = u1;
                    ir = s0 + k;
                }
            } else if ((u1 >= G.lo1 && u1 < -G.hw) || (u1 > G.hw && u1 <= G.hi1)) {
                cw += w;
            }
        }
        __syncthreads();
    }
    if (g < M) {
        const size_t o = (size_t)blockIdx.x * M + g;
        ws.cnt[o] = cnt;
        ws.il[o] = il;
        ws.ir[o] = ir;
        ws.yl[o] = yl;
        ws.yr[o] = yr;
        ws.rw[o] = rw;
        ws.cw[o] = cw;
    }
}

// Per grasp, in chunk order: contacts, counts and weights.
__global__ __launch_bounds__(256) void grasp_reduce1_kernel(int M, int C, GcWs ws, int32_t *__restrict__ contact_idx,
                                                           int32_t *__restrict__ region_count,
                                                           float *__restrict__ region_weight,
                                                           float *__restrict__ collision_weight) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= M) return;
    int cnt = 0, il = -1, ir = -1;
    double yl = INFINITY, yr = -INFINITY, rw = 0.0, cw = 0.0;
    for (int c = 0; c < C; ++c) {
        const size_t o = (size_t)c * M + g;
        if (ws.cnt[o]) {
            cnt += ws.cnt[o];
            if (ws.yl[o] < yl) {
                yl = ws.yl[o];
                il = ws.il[o];
            }
            if (ws.yr[o] > yr) {
                yr = ws.yr[o];
                ir = ws.ir[o];
            }
        }
        rw += ws.rw[o];
        cw += ws.cw[o];
    }
    contact_idx[2 * (size_t)g] = il;
    contact_idx[2 * (size_t)g + 1] = ir;
    region_count[g] = cnt;
    region_weight[g] = (float)rw;
    collision_weight[g] = (float)cw;
    ws.gcnt[g] = cnt;
    ws.gyl[g] = yl;
    ws.gyr[g] = yr;
    ws.gcw[g] = cw;
}

__global__ __launch_bounds__(GC_TILE) void grasp_pass2_kernel(int N, const float *__restrict__ points,
                                                              const float *__restrict__ normals,
                                                              const float *__restrict__ weights, int M,
                                                              const float *__restrict__ grasps, GcParams P, int len,
                                                              int C, GcWs ws) {
    __shared__ float4 s_p[GC_STAGE];
    __shared__ float4 s_n[GC_STAGE];
    const int g = blockIdx.y * blockDim.x + threadIdx.x;
    const bool any = g < M && ws.gcnt[g] > 0;
    GcGrasp G;
    gc_load(any ? grasps + (size_t)g * GC_ROW : nullptr, P, G);
    const double nb = -P.depth_base;
    const double tl = any ? ws.gyl[g] + P.band : -INFINITY, tr = any ? ws.gyr[g] - P.band : INFINITY;
    const double b0 = G.R[1], b1 = G.R[4], b2 = G.R[7];
    double L0 = 0.0, L1 = 0.0, L2 = 0.0, R0 = 0.0, R1 = 0.0, R2 = 0.0;
    const int i0 = blockIdx.x * len, i1 = min(N, i0 + len);
    for (int s0 = i0; s0 < i1; s0 += GC_STAGE) {
        const int ns = min(GC_STAGE, i1 - s0);
        gc_stage(s0, ns, points, normals, weights, P.min_weight, s_p, s_n);
        __syncthreads();
        for (int k = 0; k < ns; ++k) {
            const float4 a = s_p[k];
            if (!gc_in_box(G.lo, G.hi, a)) continue;
            double u0, u1, u2;
            gc_local(G.R, G.t, a, u0, u1, u2);
            if (!(u0 >= nb && u0 <= G.depth && fabs(u2) <= G.hh && fabs(u1) <= G.hw)) continue;
            const bool left = u1 <= tl, right = u1 >= tr;
            if (!left && !right) continue;
            const float4 nf = s_n[k];
            const double w = (double)a.w, n0 = (double)nf.x, n1 = (double)nf.y, n2 = (double)nf.z;
            const double bn = (b0 * n0 + b1 * n1) + b2 * n2;
            const double t0 = w * n0, t1 = w * n1, t2 = w * n2;
            if (left) {
                const double s = bn > 0.0 ? -1.0 : 1.0;
                L0 += s * t0;
                L1 += s * t1;
                L2 += s * t2;
            }
            if (right) {
                const double s = bn < 0.0 ? -1.0 : 1.0;
                R0 += s * t0;
                R1 += s * t1;
                R2 += s * t2;
            }
        }
        __syncthreads();
    }
    if (g < M) {
        const size_t o = (size_t)blockIdx.x * M + g, st = (size_t)C * M;
        ws.nrm[o] = L0;
        ws.nrm[o + st] = L1;
        ws.nrm[o + 2 * st] = L2;
        ws.nrm[o + 3 * st] = R0;
        ws.nrm[o + 4 * st] = R1;
        ws.nrm[o + 5 * st] = R2;
    }
}

// atan2(|x × b|, x . b)
__device__ __forceinline__ double gc_angle(double x0, double x1, double x2, double b0, double b1, double b2) {
    const double c0 = x1 * b2 - x2 * b1, c1 = x2 * b0 - x0 * b2, c2 = x0 * b1 - x1 * b0;
    return atan2(sqrt((c0 * c0 + c1 * c1) + c2 * c2), (x0 * b0 + x1 * b1) + x2 * b2);
}

// Per grasp, in chunk order: patch normals, angles, feasibility.
__global__ __launch_bounds__(256) void grasp_finalize_kernel(int M, int C, const float *__restrict__ grasps,
                                                            GcParams P, GcWs ws, float *__restrict__ normals_out,
                                                            float *__restrict__ angles,
                                                            uint8_t *__restrict__ feasible) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= M) return;
    double N[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const size_t st = (size_t)C * M;
    for (int c = 0; c < C; ++c) {
        const size_t o = (size_t)c * M + g;
#pragma unroll
        for (int k = 0; k < 6; ++k) N[k] += ws.nrm[o + k * st];
    }
    const double ll = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
    const double lr = sqrt((N[3] * N[3] + N[4] * N[4]) + N[5] * N[5]);
    const bool valid = ws.gcnt[g] > 0 && ws.gyl[g] < ws.gyr[g] && ll > 0.0 && lr > 0.0;
    float *no = normals_out + (size_t)g * 6;
    if (!valid) {
#pragma unroll
        for (int k = 0; k < 6; ++k) no[k] = NAN;
        angles[2 * (size_t)g] = NAN;
        angles[2 * (size_t)g + 1] = NAN;
        feasible[g] = 0;
        return;
    }
    const float *row = grasps + (size_t)g * GC_ROW;
    const double b0 = (double)row[5], b1 = (double)row[8], b2 = (double)row[11];     // R[:,1]
    double h[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        h[k] = N[k] / ll;
        h[3 + k] = N[3 + k] / lr;
    }
    const double al = gc_angle(-h[0], -h[1], -h[2], b0, b1, b2);
    const double ar = gc_angle(h[3], h[4], h[5], b0, b1, b2);
#pragma unroll
    for (int k = 0; k < 6; ++k) no[k] = (float)h[k];
    angles[2 * (size_t)g] = (float)al;
    angles[2 * (size_t)g + 1] = (float)ar;
    feasible[g] = (fmax(al, ar) <= P.max_angle && ws.gcw[g] <= P.max_collision) ? 1 : 0;
}

static size_t gc_layout(int N, int M, GcWs *w, char *base) {
    int C, len;
    gc_chunks(N, M, &C, &len);
    const size_t cm = (size_t)C * M;
    GgCarve cv{base, 0};
    GcWs t;
    t.cnt = (int *)cv.take(cm * 4);
    t.il = (int *)cv.take(cm * 4);
    t.ir = (int *)cv.take(cm * 4);
    t.yl = (double *)cv.take(cm * 8);
    t.yr = (double *)cv.take(cm * 8);
    t.rw = (double *)cv.take(cm * 8);
    t.cw = (double *)cv.take(cm * 8);
    t.nrm = (double *)cv.take(6 * cm * 8);
    t.gcnt = (int *)cv.take((size_t)M * 4);
    t.gyl = (double *)cv.take((size_t)M * 8);
    t.gyr = (double *)cv.take((size_t)M * 8);
    t.gcw = (double *)cv.take((size_t)M * 8);
    if (w) *w = t;
    return cv.off;
}

extern "C" size_t gg_grasp_contacts_workspace(int num_points, int num_grasps) {
    if (num_points < 0 || num_points > GG_GRASP_MAX_POINTS || num_grasps <= 0 || num_grasps > GG_GRASP_MAX)
        return 0;
    return gc_layout(num_points, num_grasps, nullptr, nullptr);
}

extern "C" int gg_grasp_contacts(int num_points, const float *points, const float *normals, const float *weights,
                                 int num_grasps, const float *grasps, double depth_base, double finger_width,
                                 double band, double mu, double min_weight, double max_collision,
                                 int32_t *contact_idx, float *normals_out, float *angles, int32_t *region_count,
                                 float *region_weight, float *collision_weight, uint8_t *feasible, void *ws,
                                 size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0, "num_points < 0");
    GG_REQUIRE(num_grasps >= 0, "num_grasps < 0");
    GG_REQUIRE(num_points <= GG_GRASP_MAX_POINTS, "num_points > GG_GRASP_MAX_POINTS");
    GG_REQUIRE(num_grasps <= GG_GRASP_MAX, "num_grasps > GG_GRASP_MAX");
    GG_REQUIRE(isfinite(depth_base) && depth_base >= 0.0, "depth_base must be finite and >= 0");
    GG_REQUIRE(isfinite(finger_width) && finger_width >= 0.0, "finger_width must be finite and >= 0");
    GG_REQUIRE(isfinite(band) && band >= 0.0, "band must be finite and >= 0");
    GG_REQUIRE(isfinite(mu) && mu >= 0.0, "mu must be finite and >= 0");
    GG_REQUIRE(!isnan(min_weight), "min_weight is NaN");
    GG_REQUIRE(!isnan(max_collision), "max_collision is NaN (pass +inf for no limit)");
    if (num_grasps == 0) return GG_OK;
    GG_REQUIRE(grasps && contact_idx && normals_out && angles && region_count && region_weight &&
                   collision_weight && feasible,
               "null pointer: grasps / outputs");
    GG_REQUIRE(num_points == 0 || (points && normals && weights), "null pointer: points / normals / weights");
    GG_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)normals & 3) == 0 && ((uintptr_t)weights & 3) == 0 &&
                   ((uintptr_t)grasps & 3) == 0,
               "points / normals / weights / grasps misaligned");
    GG_REQUIRE((((uintptr_t)contact_idx | (uintptr_t)normals_out | (uintptr_t)angles | (uintptr_t)region_count |
                 (uintptr_t)region_weight | (uintptr_t)collision_weight) & 3) == 0,
               "contact_idx / normals_out / angles / region_count / region_weight / collision_weight misaligned");
    const size_t need = gc_layout(num_points, num_grasps, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    GcWs w;
    gc_layout(num_points, num_grasps, &w, (char *)ws);
    int C, len;
    gc_chunks(num_points, num_grasps, &C, &len);
    const GcParams P{depth_base, finger_width, band, min_weight, max_collision, atan(mu)};
    hipStream_t s = (hipStream_t)stream;
    const int M = num_grasps;
    dim3 grid, block;
    gc_launch_shape(C, M, &grid, &block);
    const unsigned per_grasp = (unsigned)((M + 255) / 256);
    gg_prof_begin(GG_K_GRASP, s);
    if (C > 0)
        hipLaunchKernelGGL(grasp_pass1_kernel, grid, block, 0, s, num_points, points, normals, weights, M,
                           grasps, P, len, w);
    hipLaunchKernelGGL(grasp_reduce1_kernel, dim3(per_grasp), dim3(256), 0, s, M, C, w, contact_idx, region_count,
                       region_weight, collision_weight);
    if (C > 0)
        hipLaunchKernelGGL(grasp_pass2_kernel, grid, block, 0, s, num_points, points, normals, weights, M,
                           grasps, P, len, C, w);
    hipLaunchKernelGGL(grasp_finalize_kernel, dim3(per_grasp), dim3(256), 0, s, M, C, grasps, P, w, normals_out,
                       angles, feasible);
    gg_prof_end(GG_K_GRASP, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
