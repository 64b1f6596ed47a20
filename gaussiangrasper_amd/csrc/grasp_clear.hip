// grasp_clear.hip — gripper clearance: every grasp candidate's whole gripper (a model of up to GG_CLEAR_MAX_PARTS
// boxes in the gripper frame, each bound affine in the row's width, depth and height) against every point, at the
// final pose (body) and over the straight approach that leads to it (sweep).  The contract is in include/gg_raster.h
// (gg_grasp_clearance) and PARITY.md "Gripper clearance"; the design in DESIGN.md §3.20.
//
// Tiling as in grasp.hip: one lane per grasp, GC_TILE grasps per workgroup (grid.y), each lane holding its grasp's
// fp64 frame, its parts' bounds and its 2P sums and 2P counts in registers (the kernel is a template over P, so that
// every per-part array is indexed at compile time); grid.x splits the points into C chunks, staged through LDS
// GC_STAGE at a time and read as broadcasts.
// Cull: the union of every part's body and sweep volume is one box of the gripper frame; its world-space fp32
// bounding box (gc_cull_box: fp64 inverse of R, half-extents widened by GC_MARGIN relative, rounded outward) is
// tested with six fp32 compares per pair, and only pairs inside it take the fp64 test.  A point that takes no part
// is staged as NaN and fails every compare.
// Determinism: no atomics.  Each (chunk, part, grasp) writes its partial counts and fp64 sums; a per-grasp kernel
// adds them in chunk order, rounds, and decides `clear`.  C depends on (N, M) only.
#include "grasp_common.h"

struct ClParts {
    double c[GG_CLEAR_MAX_PARTS * 24];      // [part][bound: x_lo x_hi y_lo y_hi z_lo z_hi][c0 cw cd ch]
};

struct ClWs {
    int *bc, *sc;                // [C][P][M]: grasps innermost, so that a wave's stores are contiguous
    double *bs, *ss;             // [C][P][M]
};

template <int NP>
struct ClGrasp {
    double R[9], t[3];           // R row-major: column 0 approach a, 1 closing b, 2 height c
    double xs[NP], xl[NP], xh[NP], yl[NP], yh[NP], zl[NP], zh[NP];      // xs = x_lo - approach
    float lo[3], hi[3];          // fp32 cull box: empty for a grasp that is not valid or has no part that is not empty
};

__device__ __forceinline__ bool cl_row_valid(const float *v) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < GC_ROW; ++k) ok = ok && isfinite(v[k]);
    return ok && v[1] > 0.0f && v[2] > 0.0f;
}

// `row` may be null (a lane past the last grasp): the grasp is then not valid.
template <int NP>
__device__ void cl_load(const float *row, const ClParts &parts, double approach, ClGrasp<NP> &g) {
    float v[GC_ROW];
#pragma unroll
    for (int k = 0; k < GC_ROW; ++k) v[k] = row ? row[k] : 0.0f;
    const bool ok = row != nullptr && cl_row_valid(v);
#pragma unroll
    for (int k = 0; k < 9; ++k) g.R[k] = (double)v[4 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) g.t[k] = (double)v[13 + k];
    const double width = (double)v[1], height = (double)v[2], depth = (double)v[3];
    // the union of the body and sweep volumes of the parts that are not empty, in the gripper frame
    double L[3] = {INFINITY, INFINITY, INFINITY}, H[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        double b[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double *c = parts.c + (p * 6 + k) * 4;
            b[k] = ((c[0] + c[1] * width) + c[2] * depth) + c[3] * height;
        }
        bool full = ok;
#pragma unroll
        for (int k = 0; k < 6; ++k) full = full && isfinite(b[k]);
        full = full && b[0] <= b[1] && b[2] <= b[3] && b[4] <= b[5];
        const double xs = b[0] - approach;
        g.xs[p] = xs;
        g.xl[p] = b[0];
        g.xh[p] = b[1];
        g.yl[p] = full ? b[2] : INFINITY;       // an empty part: no u_1 passes
        g.yh[p] = full ? b[3] : -INFINITY;
        g.zl[p] = b[4];
        g.zh[p] = b[5];
        if (full) {
            L[0] = fmin(L[0], xs);
            H[0] = fmax(H[0], b[1]);
            L[1] = fmin(L[1], b[2]);
            H[1] = fmax(H[1], b[3]);
            L[2] = fmin(L[2], b[4]);
            H[2] = fmax(H[2], b[5]);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.lo[k] = INFINITY;
        g.hi[k] = -INFINITY;
    }
    if (!(L[0] <= H[0])) return;                // not valid, or every part empty: nothing to count
    double m[3], h[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m[k] = 0.5 * L[k] + 0.5 * H[k];
        h[k] = 0.5 * H[k] - 0.5 * L[k];
    }
    gc_cull_box(g.R, g.t, m, h, g.lo, g.hi);
}

template <int NP>
__global__ __launch_bounds__(GC_TILE) void grasp_clear_pass_kernel(int N, const float *__restrict__ points,
                                                                   const float *__restrict__ weights, int M,
                                                                   const float *__restrict__ grasps, ClParts parts,
                                                                   double approach, double min_weight, int len,
                                                                   ClWs ws) {
    __shared__ float4 s_p[GC_STAGE];
    const int g = blockIdx.y * blockDim.x + threadIdx.x;
    ClGrasp<NP> G;
    cl_load<NP>(g < M ? grasps + (size_t)g * GC_ROW : nullptr, parts, approach, G);
    int bc[NP], sc[NP];
    double bs[NP], ss[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        bc[p] = 0;
        sc[p] = 0;
        bs[p] = 0.0;
        ss[p] = 0.0;
    }
    const int i0 = blockIdx.x * len, i1 = min(N, i0 + len);
    for (int s0 = i0; s0 < i1; s0 += GC_STAGE) {
        const int ns = min(GC_STAGE, i1 - s0);
        gc_stage(s0, ns, points, nullptr, weights, min_weight, s_p, nullptr);
        __syncthreads();
        for (int k = 0; k < ns; ++k) {
            const float4 a = s_p[k];
            if (!gc_in_box(G.lo, G.hi, a)) continue;
            double u0, u1, u2;
            gc_local(G.R, G.t, a, u0, u1, u2);
            const double w = (double)a.w;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (!(u1 >= G.yl[p] && u1 <= G.yh[p] && u2 >= G.zl[p] && u2 <= G.zh[p])) continue;
                if (u0 >= G.xl[p]) {
                    if (u0 <= G.xh[p]) {
                        ++bc[p];
                        bs[p] += w;
                    }
                } else if (u0 >= G.xs[p]) {
                    ++sc[p];
                    ss[p] += w;
                }
            }
        }
        __syncthreads();
    }
    if (g < M) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const size_t o = ((size_t)blockIdx.x * NP + p) * M + g;
            ws.bc[o] = bc[p];
            ws.sc[o] = sc[p];
            ws.bs[o] = bs[p];
            ws.ss[o] = ss[p];
        }
    }
}

// Per grasp: the C partials of every part in chunk order, the totals in part order, valid and clear.
__global__ __launch_bounds__(256) void grasp_clear_reduce_kernel(int M, int C, int P, const float *__restrict__ grasps,
                                                                 double max_body, double max_sweep, ClWs ws,
                                                                 int32_t *__restrict__ body_count,
                                                                 float *__restrict__ body_weight,
                                                                 int32_t *__restrict__ sweep_count,
                                                                 float *__restrict__ sweep_weight,
                                                                 uint8_t *__restrict__ valid,
                                                                 uint8_t *__restrict__ clear) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= M) return;
    float v[GC_ROW];
#pragma unroll
    for (int k = 0; k < GC_ROW; ++k) v[k] = grasps[(size_t)g * GC_ROW + k];
    const bool ok = cl_row_valid(v);
    double tb = 0.0, ts = 0.0;
    for (int p = 0; p < P; ++p) {
        int bc = 0, sc = 0;
        double bs = 0.0, ss = 0.0;
        for (int c = 0; c < C; ++c) {
            const size_t o = ((size_t)c * P + p) * M + g;
            bc += ws.bc[o];
            sc += ws.sc[o];
            bs += ws.bs[o];
            ss += ws.ss[o];
        }
        const size_t o = (size_t)g * P + p;
        body_count[o] = bc;
        sweep_count[o] = sc;
        body_weight[o] = (float)bs;
        sweep_weight[o] = (float)ss;
        tb += bs;
        ts += ss;
    }
    valid[g] = ok ? 1 : 0;
    clear[g] = (ok && tb <= max_body && ts <= max_sweep) ? 1 : 0;
}

static size_t cl_layout(int N, int M, int P, ClWs *w, char *base) {
    int C, len;
    gc_chunks(N, M, &C, &len);
    const size_t n = (size_t)C * M * P;
    GgCarve cv{base, 0};
    ClWs t;
    t.bc = (int *)cv.take(n * 4);
    t.sc = (int *)cv.take(n * 4);
    t.bs = (double *)cv.take(n * 8);
    t.ss = (double *)cv.take(n * 8);
    if (w) *w = t;
    return cv.off < 256 ? 256 : cv.off;     // never 0 for counts in range: 0 says "out of range"
}

extern "C" size_t gg_grasp_clearance_workspace(int num_points, int num_grasps, int num_parts) {
    if (num_points < 0 || num_points > GG_GRASP_MAX_POINTS || num_grasps <= 0 || num_grasps > GG_GRASP_MAX ||
        num_parts < 1 || num_parts > GG_CLEAR_MAX_PARTS)
        return 0;
    return cl_layout(num_points, num_grasps, num_parts, nullptr, nullptr);
}

template <int NP>
static void cl_launch_pass(dim3 grid, dim3 block, hipStream_t s, int N, const float *points, const float *weights,
                           int M, const float *grasps, const ClParts &parts, double approach, double min_weight,
                           int len, const ClWs &w) {
    hipLaunchKernelGGL(grasp_clear_pass_kernel<NP>, grid, block, 0, s, N, points, weights, M, grasps, parts, approach,
                       min_weight, len, w);
}

extern "C" int gg_grasp_clearance(int num_points, const float *points, const float *weights, int num_grasps,
                                  const float *grasps, int num_parts, const double *parts, double approach,
                                  double min_weight, double max_body, double max_sweep, int32_t *body_count,
                                  float *body_weight, int32_t *sweep_count, float *sweep_weight, uint8_t *valid,
                                  uint8_t *clear, void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0, "num_points < 0");
    GG_REQUIRE(num_grasps >= 0, "num_grasps < 0");
    GG_REQUIRE(num_points <= GG_GRASP_MAX_POINTS, "num_points > GG_GRASP_MAX_POINTS");
    GG_REQUIRE(num_grasps <= GG_GRASP_MAX, "num_grasps > GG_GRASP_MAX");
    GG_REQUIRE(num_parts >= 1 && num_parts <= GG_CLEAR_MAX_PARTS, "num_parts must be in 1..GG_CLEAR_MAX_PARTS");
    GG_REQUIRE(parts, "null pointer: parts");
    ClParts cp;
    for (int k = 0; k < GG_CLEAR_MAX_PARTS * 24; ++k) {
        cp.c[k] = k < num_parts * 24 ? parts[k] : 0.0;
        GG_REQUIRE(isfinite(cp.c[k]), "parts: every coefficient must be finite");
    }
    GG_REQUIRE(isfinite(approach) && approach >= 0.0, "approach must be finite and >= 0");
    GG_REQUIRE(!isnan(min_weight), "min_weight is NaN");
    GG_REQUIRE(!isnan(max_body), "max_body is NaN (pass +inf for no limit)");
    GG_REQUIRE(!isnan(max_sweep), "max_sweep is NaN (pass +inf for no limit)");
    if (num_grasps == 0) return GG_OK;
    GG_REQUIRE(grasps && body_count && body_weight && sweep_count && sweep_weight && valid && clear,
               "null pointer: grasps / outputs");
    GG_REQUIRE(num_points == 0 || (points && weights), "null pointer: points / weights");
    GG_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)weights & 3) == 0 && ((uintptr_t)grasps & 3) == 0 &&
                   ((uintptr_t)body_count & 3) == 0 && ((uintptr_t)body_weight & 3) == 0 &&
                   ((uintptr_t)sweep_count & 3) == 0 && ((uintptr_t)sweep_weight & 3) == 0,
               "points / weights / grasps / counts / sums misaligned");
    const size_t need = cl_layout(num_points, num_grasps, num_parts, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    ClWs w;
    cl_layout(num_points, num_grasps, num_parts, &w, (char *)ws);
    int C, len;
    gc_chunks(num_points, num_grasps, &C, &len);
    hipStream_t s = (hipStream_t)stream;
    const int M = num_grasps;
    dim3 grid, block;
    gc_launch_shape(C, M, &grid, &block);
    gg_prof_begin(GG_K_GRASP_CLEAR, s);
    if (C > 0) {
#define CL_CASE(NP)                                                                                           \
    case NP:                                                                                                  \
        cl_launch_pass<NP>(grid, block, s, num_points, points, weights, M, grasps, cp, approach, min_weight, len, \
                           w);                                                                                \
        break;
        switch (num_parts) {
            CL_CASE(1)
            CL_CASE(2)
            CL_CASE(3)
            CL_CASE(4)
            CL_CASE(5)
            CL_CASE(6)
            CL_CASE(7)
            CL_CASE(8)
        }
#undef CL_CASE
    }
    hipLaunchKernelGGL(grasp_clear_reduce_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, M, C,
                       num_parts, grasps, max_body, max_sweep, w, body_count, body_weight, sweep_count, sweep_weight,
                       valid, clear);
    gg_prof_end(GG_K_GRASP_CLEAR, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
