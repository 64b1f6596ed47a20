// support_plane.hip — the support plane (the table): a RANSAC consensus of H three-point hypotheses against N points
// (gg_plane_consensus) and the labels and moments of one plane against N points (gg_plane_classify).  The contract is
// in include/gg_raster.h and PARITY.md "Support plane"; the design in DESIGN.md §3.22.
//
// Consensus, three launches:
//   sp_hyp_kernel      one lane per hypothesis: its record (p_a, n, (dist dist) nn: 7 doubles in a row of 8), valid and
//                      count = 0.  A hypothesis that is not valid gets n = 0 and a limit of -1, so that no point is its
//                      inlier (s s = 0 <= -1 fails) and the pass needs no branch on valid.
//   sp_count_kernel    one lane per point, SP_TILE points per pass of a workgroup, grid.x the point chunks, grid.y the
//                      hypothesis chunks of SP_HCHUNK.  The chunk's records are staged through LDS once and read as
//                      broadcasts; a wave's inliers of one record are one ballot and one popcount, added to the
//                      record's LDS counter by lane 0 (an integer ds_add); at the end the workgroup adds its non-zero
//                      counters to count[] with integer atomics.  Integer sums: exact in any order.
//   sp_best_kernel     one workgroup: the valid hypothesis with the largest count, the smaller index on ties.
// There is no fp32 cull: the fp64 test is 10 operations a pair, and a conservative fp32 bound on |s| needs most of them.
//
// Classify, two launches, the fixed orders of ordered_sum.h: sp_classify_kernel writes height and side and one slab
// row of 16 sums per workgroup (a lane's SP_CL_ITEMS points in index order, then the block row); sp_finish_kernel,
// one workgroup, sums the slab's rows by the chains.  No atomics.
#include <math.h>

#include "gg_common.h"
#include "ordered_sum.h"

#define SP_TILE 256              // points per pass of a workgroup (one per lane)
#define SP_HCHUNK 256            // hypothesis records per workgroup: 16 KB of LDS
#define SP_REC 8                 // doubles per record row: p_a (3), n (3), limit, pad
#define SP_TARGET_BLOCKS 4096    // point chunks x hypothesis chunks aimed for: 16 workgroups per CU
#define SP_MIN_CHUNK 1024        // fewest points a chunk is given
#define SP_SUMS 16
#define SP_CL_ITEMS 4            // points per lane of the classify kernel
#define SP_FIN_THREADS (GG_SUM_CHAINS * SP_SUMS)

struct SpUp {
    double u[3], uu, cos2;
    int on;
};

struct SpPlane {
    double n[3], d, o[3], dist;
};

__device__ __forceinline__ bool sp_takes_part(const float *__restrict__ points, const float *__restrict__ weights,
                                              size_t i, double min_weight, float *p) {
    p[0] = points[i * 3];
    p[1] = points[i * 3 + 1];
    p[2] = points[i * 3 + 2];
    const bool fin = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    return fin && (weights == nullptr || (double)weights[i] > min_weight);
}

__global__ __launch_bounds__(256) void sp_hyp_kernel(int N, const float *__restrict__ points,
                                                     const float *__restrict__ weights, double min_weight, int H,
                                                     const int32_t *__restrict__ hyp, double dd, double min_sin2,
                                                     SpUp up, double *__restrict__ rec, int32_t *__restrict__ count,
                                                     uint8_t *__restrict__ valid) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    const int a = hyp[(size_t)h * 3], b = hyp[(size_t)h * 3 + 1], c = hyp[(size_t)h * 3 + 2];
    bool ok = a >= 0 && a < N && b >= 0 && b < N && c >= 0 && c < N && a != b && a != c && b != c;
    double pa[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0}, nn = 0.0;
    if (ok) {
        float fa[3], fb[3], fc[3];
        ok = sp_takes_part(points, weights, (size_t)a, min_weight, fa);
        ok = sp_takes_part(points, weights, (size_t)b, min_weight, fb) && ok;
        ok = sp_takes_part(points, weights, (size_t)c, min_weight, fc) && ok;
        double e1[3], e2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pa[k] = (double)fa[k];
            e1[k] = (double)fb[k] - (double)fa[k];
            e2[k] = (double)fc[k] - (double)fa[k];
        }
        n[0] = e1[1] * e2[2] - e1[2] * e2[1];
        n[1] = e1[2] * e2[0] - e1[0] * e2[2];
        n[2] = e1[0] * e2[1] - e1[1] * e2[0];
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
        const double ee1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
        const double ee2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
        ok = ok && isfinite(nn) && nn > min_sin2 * (ee1 * ee2);
        if (up.on) {
            const double g = (n[0] * up.u[0] + n[1] * up.u[1]) + n[2] * up.u[2];
            ok = ok && g * g >= up.cos2 * (nn * up.uu);
        }
    }
    double *r = rec + (size_t)h * SP_REC;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r[k] = ok ? pa[k] : 0.0;
        r[3 + k] = ok ? n[k] : 0.0;
    }
    r[6] = ok ? dd * nn : -1.0;
    r[7] = 0.0;
    count[h] = 0;
    valid[h] = ok ? 1 : 0;
}

__global__ __launch_bounds__(SP_TILE) void sp_count_kernel(int N, const float *__restrict__ points,
                                                           const float *__restrict__ weights, double min_weight,
                                                           int H, const double *__restrict__ rec, int len,
                                                           int32_t *__restrict__ count) {
    __shared__ double s_rec[SP_HCHUNK * SP_REC];
    __shared__ int s_cnt[SP_HCHUNK];
    const int h0 = blockIdx.y * SP_HCHUNK, nh = min(SP_HCHUNK, H - h0);
    for (int k = threadIdx.x; k < nh * SP_REC; k += SP_TILE) s_rec[k] = rec[(size_t)h0 * SP_REC + k];
    for (int k = threadIdx.x; k < SP_HCHUNK; k += SP_TILE) s_cnt[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (GG_WAVE - 1);
    // i0 <= N - 1 and len <= 2^30 rounded up to SP_TILE: 64-bit, so that i0 + len cannot wrap
    const long long i0 = (long long)blockIdx.x * len, i1 = min((long long)N, i0 + (long long)len);
    for (long long t0 = i0; t0 < i1; t0 += SP_TILE) {             // no barrier inside
        const long long i = t0 + threadIdx.x;
        float p[3] = {0.f, 0.f, 0.f};
        const bool part = i < i1 && sp_takes_part(points, weights, (size_t)i, min_weight, p);
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        for (int k = 0; k < nh; ++k) {
            const double *r = s_rec + k * SP_REC;
            // s = (n0 d0 + n1 d1) + n2 d2, d = p - p_a: fp64, no contraction
            const double d0 = x - r[0], d1 = y - r[1], d2 = z - r[2];
            const double s = (r[3] * d0 + r[4] * d1) + r[5] * d2;
            const unsigned long long in = __ballot(part && s * s <= r[6]);
            if (lane == 0 && in != 0ull) atomicAdd(&s_cnt[k], __popcll(in));
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nh; k += SP_TILE) {
        const int v = s_cnt[k];
        if (v != 0) atomicAdd(&count[h0 + k], v);
    }
}

// (count, index) order: the larger count, then the smaller index; index -1 = none
__device__ __forceinline__ bool sp_better(int c, int i, int bc, int bi) {
    return i >= 0 && (bi < 0 || c > bc || (c == bc && i < bi));
}

__global__ __launch_bounds__(256) void sp_best_kernel(int H, const int32_t *__restrict__ count,
                                                      const uint8_t *__restrict__ valid, int32_t *__restrict__ best) {
    __shared__ int s_c[256], s_i[256];
    int bc = 0, bi = -1;
    for (int h = threadIdx.x; h < H; h += 256) {
        if (!valid[h]) continue;
        const int c = count[h];
        if (sp_better(c, h, bc, bi)) {
            bc = c;
            bi = h;
        }
    }
    s_c[threadIdx.x] = bc;
    s_i[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {                           // uniform trip count
        if ((int)threadIdx.x < o && sp_better(s_c[threadIdx.x + o], s_i[threadIdx.x + o], s_c[threadIdx.x],
                                              s_i[threadIdx.x])) {
            s_c[threadIdx.x] = s_c[threadIdx.x + o];
            s_i[threadIdx.x] = s_i[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        best[0] = s_i[0];
        best[1] = s_i[0] < 0 ? 0 : s_c[0];
    }
}

// C point chunks of len points (len a multiple of SP_TILE) from (N, H) only
static void sp_chunks(int N, int H, int *C, int *len) {
    *C = 0;
    *len = 0;
    if (N <= 0 || H <= 0) return;
    const int hc = (H + SP_HCHUNK - 1) / SP_HCHUNK;
    long long c = SP_TARGET_BLOCKS / hc;
    const long long most = ((long long)N + SP_MIN_CHUNK - 1) / SP_MIN_CHUNK;
    c = c < 1 ? 1 : c;
    c = c > most ? most : c;
    long long l = ((long long)N + c - 1) / c;
    l = (l + SP_TILE - 1) / SP_TILE * SP_TILE;
    *len = (int)l;                                               // <= 2^30 + SP_TILE
    *C = (int)(((long long)N + l - 1) / l);
}

static bool sp_counts_ok(int N, int H) {
    return N >= 0 && N <= GG_GRASP_MAX_POINTS && H >= 0 && H <= GG_PLANE_MAX_HYPOTHESES;
}

static size_t sp_consensus_bytes(int H) {
    const size_t b = gg_align_up((size_t)H * SP_REC * sizeof(double), 256);
    return b < 256 ? 256 : b;                // never 0 for counts in range: 0 says "out of range"
}

extern "C" size_t gg_plane_consensus_workspace(int num_points, int num_hypotheses) {
    if (!sp_counts_ok(num_points, num_hypotheses)) return 0;
    return sp_consensus_bytes(num_hypotheses);
}

extern "C" int gg_plane_consensus(int num_points, const float *points, const float *weights, double min_weight,
                                  int num_hypotheses, const int32_t *hyp, double dist, double min_sin2,
                                  const double *up, double cos2_tilt, int32_t *count, uint8_t *valid, int32_t *best,
                                  void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0, "num_points < 0");
    GG_REQUIRE(num_hypotheses >= 0, "num_hypotheses < 0");
    GG_REQUIRE(num_points <= GG_GRASP_MAX_POINTS, "num_points > GG_GRASP_MAX_POINTS");
    GG_REQUIRE(num_hypotheses <= GG_PLANE_MAX_HYPOTHESES, "num_hypotheses > GG_PLANE_MAX_HYPOTHESES");
    GG_REQUIRE(!isnan(min_weight), "min_weight is NaN");
    GG_REQUIRE(isfinite(dist) && dist >= 0.0 && isfinite(dist * dist), "dist must be finite and >= 0");
    GG_REQUIRE(min_sin2 >= 0.0 && min_sin2 <= 1.0, "min_sin2 must be in [0, 1]");
    SpUp u;
    u.on = up ? 1 : 0;
    u.u[0] = u.u[1] = u.u[2] = u.uu = u.cos2 = 0.0;
    if (up) {
        GG_REQUIRE(isfinite(up[0]) && isfinite(up[1]) && isfinite(up[2]), "up must be finite");
        for (int k = 0; k < 3; ++k) u.u[k] = up[k];
        u.uu = (up[0] * up[0] + up[1] * up[1]) + up[2] * up[2];
        GG_REQUIRE(isfinite(u.uu) && u.uu > 0.0, "up must not be zero");
        GG_REQUIRE(cos2_tilt >= 0.0 && cos2_tilt <= 1.0, "cos2_tilt must be in [0, 1]");
        u.cos2 = cos2_tilt;
    }
    if (num_hypotheses == 0) return GG_OK;
    GG_REQUIRE(hyp && count && valid && best, "null pointer: hyp / count / valid / best");
    GG_REQUIRE(num_points == 0 || points, "null pointer: points");
    GG_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)weights & 3) == 0 && ((uintptr_t)hyp & 3) == 0 &&
                   ((uintptr_t)count & 3) == 0 && ((uintptr_t)best & 3) == 0,
               "points / weights / hyp / count / best misaligned");
    const size_t need = sp_consensus_bytes(num_hypotheses);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    double *rec = (double *)ws;
    const int N = num_points, H = num_hypotheses;
    int C, len;
    sp_chunks(N, H, &C, &len);
    hipStream_t s = (hipStream_t)stream;
    gg_prof_begin(GG_K_SUPPORT_PLANE, s);
    hipLaunchKernelGGL(sp_hyp_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, s, N, points, weights,
                       min_weight, H, hyp, dist * dist, min_sin2, u, rec, count, valid);
    if (C > 0)
        hipLaunchKernelGGL(sp_count_kernel, dim3((unsigned)C, (unsigned)((H + SP_HCHUNK - 1) / SP_HCHUNK)),
                           dim3(SP_TILE), 0, s, N, points, weights, min_weight, H, rec, len, count);
    hipLaunchKernelGGL(sp_best_kernel, dim3(1), dim3(256), 0, s, H, count, valid, best);
    gg_prof_end(GG_K_SUPPORT_PLANE, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------
// one plane against every point: labels, heights and the 16 sums
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sp_classify_kernel(int N, const float *__restrict__ points,
                                                          const float *__restrict__ weights, double min_weight,
                                                          SpPlane P, float *__restrict__ height,
                                                          uint8_t *__restrict__ side, double *__restrict__ slab) {
    __shared__ double s_w[4][SP_SUMS];
    double v[SP_SUMS];
#pragma unroll
    for (int k = 0; k < SP_SUMS; ++k) v[k] = 0.0;
    const long long base = (long long)blockIdx.x * (256 * SP_CL_ITEMS) + threadIdx.x;
#pragma unroll
    for (int it = 0; it < SP_CL_ITEMS; ++it) {
        const long long i = base + (long long)it * 256;
        if (i >= N) continue;
        const float px = points[(size_t)i * 3], py = points[(size_t)i * 3 + 1], pz = points[(size_t)i * 3 + 2];
        const bool fin = isfinite(px) && isfinite(py) && isfinite(pz);
        const double w = weights ? (double)weights[i] : 1.0;
        const bool part = fin && (weights == nullptr || w > min_weight);
        const double x = (double)px, y = (double)py, z = (double)pz;
        const double h = ((P.n[0] * x + P.n[1] * y) + P.n[2] * z) + P.d;
        height[i] = fin ? (float)h : NAN;
        const int sd = !part ? 3 : h < -P.dist ? 0 : h <= P.dist ? 1 : 2;
        side[i] = (uint8_t)sd;
        if (sd == 1) {
            const double q0 = x - P.o[0], q1 = y - P.o[1], q2 = z - P.o[2];
            v[0] += 1.0;
            v[3] += h * h;
            v[4] += q0;
            v[5] += q1;
            v[6] += q2;
            v[7] += q0 * q0;
            v[8] += q0 * q1;
            v[9] += q0 * q2;
            v[10] += q1 * q1;
            v[11] += q1 * q2;
            v[12] += q2 * q2;
            v[13] += w;
        } else if (sd == 2) {
            v[1] += 1.0;
            v[14] += w;
        } else if (sd == 0) {
            v[2] += 1.0;
            v[15] += w;
        }
    }
    gg_block_row<SP_SUMS>(v, s_w, slab + (size_t)SP_SUMS * blockIdx.x);
}

// One workgroup: the slab's columns by gg_chain_sum.
__global__ __launch_bounds__(SP_FIN_THREADS) void sp_finish_kernel(int nrows, const double *__restrict__ slab,
                                                                   double *__restrict__ sums) {
    __shared__ double s_c[GG_SUM_CHAINS][SP_SUMS];
    const double t = gg_chain_sum<SP_SUMS, GG_SUM_CHAINS>(nrows, slab, s_c);
    if (threadIdx.x < SP_SUMS) sums[threadIdx.x] = t;
}

static int sp_classify_blocks(int N) { return (int)(((long long)N + 256 * SP_CL_ITEMS - 1) / (256 * SP_CL_ITEMS)); }

static size_t sp_classify_bytes(int N) {
    const size_t b = gg_align_up((size_t)sp_classify_blocks(N) * SP_SUMS * sizeof(double), 256);
    return b < 256 ? 256 : b;
}

extern "C" size_t gg_plane_classify_workspace(int num_points) {
    if (num_points < 0 || num_points > GG_GRASP_MAX_POINTS) return 0;
    return sp_classify_bytes(num_points);
}

extern "C" int gg_plane_classify(int num_points, const float *points, const float *weights, double min_weight,
                                 const double *plane, const double *origin, double dist, float *height, uint8_t *side,
                                 double *sums, void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0, "num_points < 0");
    GG_REQUIRE(num_points <= GG_GRASP_MAX_POINTS, "num_points > GG_GRASP_MAX_POINTS");
    GG_REQUIRE(!isnan(min_weight), "min_weight is NaN");
    GG_REQUIRE(isfinite(dist) && dist >= 0.0, "dist must be finite and >= 0");
    GG_REQUIRE(plane && origin, "null pointer: plane / origin");
    SpPlane P;
    for (int k = 0; k < 3; ++k) {
        GG_REQUIRE(isfinite(plane[k]) && isfinite(origin[k]), "plane normal and origin must be finite");
        P.n[k] = plane[k];
        P.o[k] = origin[k];
    }
    GG_REQUIRE(plane[0] != 0.0 || plane[1] != 0.0 || plane[2] != 0.0, "plane normal must not be zero");
    GG_REQUIRE(isfinite(plane[3]), "plane offset must be finite");
    P.d = plane[3];
    P.dist = dist;
    GG_REQUIRE(sums, "null pointer: sums");
    GG_REQUIRE(num_points == 0 || (points && height && side), "null pointer: points / height / side");
    GG_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)weights & 3) == 0 && ((uintptr_t)height & 3) == 0 &&
                   ((uintptr_t)sums & 7) == 0,
               "points / weights / height / sums misaligned");
    const size_t need = sp_classify_bytes(num_points);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    double *slab = (double *)ws;
    const int blocks = sp_classify_blocks(num_points);
    hipStream_t s = (hipStream_t)stream;
    gg_prof_begin(GG_K_SUPPORT_PLANE, s);
    if (blocks > 0)
        hipLaunchKernelGGL(sp_classify_kernel, dim3((unsigned)blocks), dim3(256), 0, s, num_points, points, weights,
                           min_weight, P, height, side, slab);
    hipLaunchKernelGGL(sp_finish_kernel, dim3(1), dim3(SP_FIN_THREADS), 0, s, blocks, slab, sums);
    gg_prof_end(GG_K_SUPPORT_PLANE, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
