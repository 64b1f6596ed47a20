// grasp_common.h — the point sweep that grasp.hip (gg_grasp_contacts), grasp_clear.hip (gg_grasp_clearance) and
// grasp_propose.hip (gg_grasp_propose) share: one lane per grasp or seed, points staged through LDS GC_STAGE at a
// time, the point range split into chunks from (N, M) only, and every pair culled against an fp32 world-space box
// before it takes the fp64 test.  Here: the tiling constants, the chunk plan and launch shape, the staging loop,
// the cull box of a rotated box (margin, conditioning rule, outward rounding), the box test and the local transform.
#ifndef GG_GRASP_COMMON_H
#define GG_GRASP_COMMON_H
#include <math.h>

#include "gg_common.h"

#define GC_TILE 256              // grasps per workgroup (one per lane)
#define GC_STAGE 256             // points per LDS stage
#define GC_TARGET_BLOCKS 2048    // chunks x grasp tiles aimed for: 8 workgroups per CU
#define GC_MIN_CHUNK 512         // fewest points a chunk is given
#define GC_MARGIN 1e-6           // relative widening of the cull box (>> the fp64 test's rounding)
#define GC_MAX_COND 1e3          // max|R| max|R^-T| above this: no cull for that grasp
#define GC_ROW 17

__device__ __forceinline__ float gc_down(double x) {
    float f = (float)x;
    return (double)f > x ? nextafterf(f, -INFINITY) : f;
}
__device__ __forceinline__ float gc_up(double x) {
    float f = (float)x;
    return (double)f < x ? nextafterf(f, INFINITY) : f;
}

// The fp32 world-space bounds [lo, hi] of the box with centre m and half-extents h in the frame u = R^T (p - t):
// p = t + Q u with Q = R^-T = cofactor(R) / det(R).  Each half-extent is widened by GC_MARGIN times the sum of the
// magnitudes of every term of the bound (|t| + |Q m| termwise + e) and the bounds are rounded outward; a frame that
// is singular, not finite or conditioned worse than GC_MAX_COND, or a box that is not finite, gets (-inf, +inf): no
// cull.  The box is only a cull: it admits a superset of the pairs and the fp64 test decides every one of them, so
// its exact width never shows in an output (it is >= the |t + Q m| + e that the contacts used before they shared it).
__device__ __forceinline__ void gc_cull_box(const double *R, const double *t, const double *m, const double *h,
                                            float *lo, float *hi) {
    double Q[9];
    Q[0] = R[4] * R[8] - R[5] * R[7];
    Q[1] = R[5] * R[6] - R[3] * R[8];
    Q[2] = R[3] * R[7] - R[4] * R[6];
    Q[3] = R[2] * R[7] - R[1] * R[8];
    Q[4] = R[0] * R[8] - R[2] * R[6];
    Q[5] = R[1] * R[6] - R[0] * R[7];
    Q[6] = R[1] * R[5] - R[2] * R[4];
    Q[7] = R[2] * R[3] - R[0] * R[5];
    Q[8] = R[0] * R[4] - R[1] * R[3];
    const double det = (R[0] * Q[0] + R[1] * Q[1]) + R[2] * Q[2];
    double qmax = 0.0, rmax = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        Q[k] = Q[k] / det;
        qmax = fmax(qmax, fabs(Q[k]));       // fmax drops a NaN: checked below
        rmax = fmax(rmax, fabs(R[k]));
    }
    bool cull = det != 0.0 && qmax * rmax <= GC_MAX_COND;
#pragma unroll
    for (int k = 0; k < 9; ++k) cull = cull && isfinite(Q[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) cull = cull && isfinite(m[k]) && isfinite(h[k]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (!cull) {
            lo[i] = -INFINITY;
            hi[i] = INFINITY;
            continue;
        }
        const double c = t[i] + ((Q[i * 3] * m[0] + Q[i * 3 + 1] * m[1]) + Q[i * 3 + 2] * m[2]);
        const double e = fabs(Q[i * 3]) * h[0] + fabs(Q[i * 3 + 1]) * h[1] + fabs(Q[i * 3 + 2]) * h[2];
        const double w = e + GC_MARGIN * (((fabs(t[i]) + fabs(Q[i * 3] * m[0])) + fabs(Q[i * 3 + 1] * m[1])) +
                                          fabs(Q[i * 3 + 2] * m[2]) + e);
        lo[i] = gc_down(c - w);
        hi[i] = gc_up(c + w);
    }
}

__device__ __forceinline__ bool gc_in_box(const float *lo, const float *hi, float4 a) {
    return a.x >= lo[0] && a.x <= hi[0] && a.y >= lo[1] && a.y <= hi[1] && a.z >= lo[2] && a.z <= hi[2];
}

// u_j = (R[0][j] d0 + R[1][j] d1) + R[2][j] d2, d = (double)p - t: fp64, no contraction (-ffp-contract=off)
__device__ __forceinline__ void gc_local(const double *R, const double *t, float4 a, double &u0, double &u1,
                                         double &u2) {
    const double d0 = (double)a.x - t[0], d1 = (double)a.y - t[1], d2 = (double)a.z - t[2];
    u0 = (R[0] * d0 + R[3] * d1) + R[6] * d2;
    u1 = (R[1] * d0 + R[4] * d1) + R[7] * d2;
    u2 = (R[2] * d0 + R[5] * d1) + R[8] * d2;
}

// Whether a point takes part: finite coordinates, weight > min_weight and, with `n` non-null, a finite normal there.
__device__ __forceinline__ bool gc_part(const float *p, const float *n, float w, double min_weight) {
    bool part = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && (double)w > min_weight;
    if (n) part = part && isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]);
    return part;
}

// Stage points [s0, s0 + ns) into LDS: (x, y, z, w), x/y/z NaN when the point takes no part (it then fails every
// compare of gc_in_box); with s_n non-null, the normals as they are.
__device__ __forceinline__ void gc_stage(int s0, int ns, const float *__restrict__ points,
                                         const float *__restrict__ normals, const float *__restrict__ weights,
                                         double min_weight, float4 *s_p, float4 *s_n) {
    for (int k = threadIdx.x; k < ns; k += blockDim.x) {
        const size_t i = (size_t)(s0 + k);
        const float *p = points + i * 3, *n = normals ? normals + i * 3 : nullptr;
        const float px = p[0], py = p[1], pz = p[2], w = weights[i];
        s_p[k] = gc_part(p, n, w, min_weight) ? make_float4(px, py, pz, w) : make_float4(NAN, NAN, NAN, 0.0f);
        if (s_n) s_n[k] = make_float4(n[0], n[1], n[2], 0.0f);
    }
}

// C chunks of len points (len a multiple of GC_STAGE), from (N, M) only, so that a call's summation order never
// depends on the device.
static void gc_chunks(int N, int M, int *C, int *len) {
    *C = 0;
    *len = 0;
    if (N <= 0 || M <= 0) return;
    const int tiles = (M + GC_TILE - 1) / GC_TILE;
    int c = GC_TARGET_BLOCKS / tiles;
    c = max(1, min(c, (N + GC_MIN_CHUNK - 1) / GC_MIN_CHUNK));
    int l = (N + c - 1) / c;
    l = (l + GC_STAGE - 1) / GC_STAGE * GC_STAGE;
    *len = l;
    *C = (N + l - 1) / l;
}

// The sweep's launch shape: one lane per grasp in whole waves, at most GC_TILE; chunks on grid.x, tiles on grid.y.
static void gc_launch_shape(int C, int M, dim3 *grid, dim3 *block) {
    const unsigned threads = (unsigned)min(GC_TILE, (M + GG_WAVE - 1) / GG_WAVE * GG_WAVE);
    *grid = dim3((unsigned)C, (unsigned)((M + threads - 1) / threads));
    *block = dim3(threads);
}

#endif /* GG_GRASP_COMMON_H */
