// field_observe.hip — known free space of the distance field's volume: which cells a depth frame has SEEN to be empty,
// through all of their volume.  The contract is in include/gg_raster.h (gg_depth_min_pyramid, gg_field_observe) and
// PARITY.md "Known free space"; the rule, its proof and the brick cull's margin in DESIGN.md §3.36.
//
// gg_depth_min_pyramid  level 0 (the sanitised frame) and level 1 in one launch, a thread per level-1 texel (the raw
//                       frame is read once); then one launch per further level, a thread per texel.  A minimum is
//                       exact: the bytes do not depend on the schedule.
// gg_field_observe      one launch: a workgroup owns a 4 x 8 x 8 brick of cells, one thread per cell, z fastest within
//                       a wave, the cell's two counts in registers across all views (no atomics, one load and one
//                       store per cell and counter).  The view's record (12 + 4 doubles) is read at a wave-uniform
//                       address; the level offsets sit in LDS.  Per view the workgroup first decides, from the eight
//                       corners of the box of its cells' centres, whether any of its cells can be looked at; if none
//                       can, the view is skipped by the whole brick (wave-uniform branch, no gathers).
#include <math.h>

#include "field_volume.h"

#define FO_THREADS 256
#define FO_BX 4                    // brick: 4 x 8 x 8 cells, z fastest (one wave = one x slice of 8 x 8)
#define FO_BY 8
#define FO_BZ 8
#define FO_TOL 1e-9                // brick test margin, relative (fp64 rounding of the per-cell path: ~1e-15)
#define FO_SANE 16777216.0         // 2^24: the brick test is used only for views with fx, fy, |cx|, |cy| <= this
#define FO_PAD 9.5367431640625e-07 // 2^-20 pixel
#define FO_MAX_LEVELS 17           // levels of a pyramid with sides <= GG_TSDF_MAX_SIDE = 2^15: 16
#define FP_THREADS 256

// ---------------------------------------------------------------------------------------------------------------
// pyramid
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fp_clean(float d) { return d > 0.f ? d : 0.f; }      // NaN compares false: 0

// Levels 0 and 1.  Thread t of a view owns level-1 texel (y1, x1) = (t / W1, t % W1) and its up-to-four pixels.  With
// H == W == 1 there is no level 1 (two_levels == 0): the thread writes the one pixel of level 0.
__global__ __launch_bounds__(FP_THREADS) void depth_pyramid_base_kernel(long long total, int H, int W, int H1, int W1,
                                                                        long long S, int two_levels,
                                                                        const float *__restrict__ depth,
                                                                        float *__restrict__ pyr) {
    const long long per = (long long)H1 * W1;
    for (long long t = (long long)blockIdx.x * FP_THREADS + threadIdx.x; t < total;
         t += (long long)gridDim.x * FP_THREADS) {
        const long long view = t / per;
        const int r = (int)(t - view * per), y1 = r / W1, x1 = r - y1 * W1;
        const float *src = depth + view * ((long long)H * W);
        float *dst = pyr + view * S;
        float m = INFINITY;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int y = 2 * y1 + dy, x = 2 * x1 + dx;
                if (y < H && x < W) {
                    const float d = fp_clean(src[(long long)y * W + x]);
                    dst[(long long)y * W + x] = d;
                    m = fminf(m, d);
                }
            }
        if (two_levels) dst[(long long)H * W + r] = m;
    }
}

// Level l + 1 (Hd x Wd, at offset `to`) from level l (Hs x Ws, at offset `from`).
__global__ __launch_bounds__(FP_THREADS) void depth_pyramid_level_kernel(long long total, int Hs, int Ws, int Hd, int Wd,
                                                                         long long S, long long from, long long to,
                                                                         float *pyr) {
    const long long per = (long long)Hd * Wd;
    for (long long t = (long long)blockIdx.x * FP_THREADS + threadIdx.x; t < total;
         t += (long long)gridDim.x * FP_THREADS) {
        const long long view = t / per;
        const int r = (int)(t - view * per), y1 = r / Wd, x1 = r - y1 * Wd;
        const float *src = pyr + view * S + from;
        float m = INFINITY;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int y = 2 * y1 + dy, x = 2 * x1 + dx;
                if (y < Hs && x < Ws) m = fminf(m, src[(long long)y * Ws + x]);
            }
        pyr[view * S + to + r] = m;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// observe
// ---------------------------------------------------------------------------------------------------------------
struct FoParams {
    FieldGrid g;
    int V, H, W, levels;
    int nby, nbz;                  // bricks along y, z
    long long S;
    double radius, margin, near;
    unsigned off[FO_MAX_LEVELS];   // offset of every level within a view's pyramid (S < 2^31)
};

// false only if no cell of the brick [lo, hi] (cell indices) can be looked at in this view.  Every
// lane evaluates corner (lane & 7) of the box of the cells' centres; the answer is wave-uniform.  A cell's centre, as
// the per-cell path computes it, lies in that box (lo + ((double)i + 0.5) h is monotone in i), and every quantity
// tested is linear in the centre, so its value at a cell lies between its values at the corners.
__device__ __forceinline__ bool fo_brick_sees(const FoParams &p, const double *__restrict__ E,
                                              const double *__restrict__ K, const int *lo, const int *hi) {
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    // a view outside these ranges (NaN included) is never culled: the per-cell rule alone decides
    if (!(fx > 0.0 && fx <= FO_SANE && fy > 0.0 && fy <= FO_SANE && fabs(cx) <= FO_SANE && fabs(cy) <= FO_SANE))
        return true;
    const int c = threadIdx.x & 7;
    double q[3], pmax[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double l = p.g.lo[a] + ((double)lo[a] + 0.5) * p.g.h;
        const double h = p.g.lo[a] + ((double)hi[a] + 0.5) * p.g.h;
        q[a] = ((c >> (2 - a)) & 1) ? h : l;
        pmax[a] = fmax(fabs(l), fabs(h));
    }
    double cc[3], B[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double e0 = E[4 * r], e1 = E[4 * r + 1], e2 = E[4 * r + 2], e3 = E[4 * r + 3];
        cc[r] = ((e0 * q[0] + e1 * q[1]) + e2 * q[2]) + e3;
        B[r] = ((fabs(e0) * pmax[0] + fabs(e1) * pmax[1]) + fabs(e2) * pmax[2]) + fabs(e3);
    }
    const double W = p.W, H = p.H;
    // zn = p_2 - radius < near in every cell: the view takes no part
    if (__all(cc[2] - p.radius < p.near - FO_TOL * ((B[2] + p.radius) + p.near))) return false;
    // A looked-at cell has p_2 >= near + radius > 0 and 0 < ul <= u_c <= uh < n for the projection u_c of its centre:
    // fx p_0 + cx p_2 > 0 and fx p_0 + (cx - W) p_2 < 0, and the same in y.
    const double mu = FO_TOL * (fx * B[0] + (fabs(cx) + W) * B[2]);
    const double mv = FO_TOL * (fy * B[1] + (fabs(cy) + H) * B[2]);
    if (__all(fx * cc[0] + cx * cc[2] < -mu)) return false;
    if (__all(fx * cc[0] + (cx - W) * cc[2] > mu)) return false;
    if (__all(fy * cc[1] + cy * cc[2] < -mv)) return false;
    if (__all(fy * cc[1] + (cy - H) * cc[2] > mv)) return false;
    return true;
}

// The pixel bounds [A, B] of one axis of the ball's bounding box; false when they leave 0..n - 1 (or are NaN).
__device__ __forceinline__ bool fo_axis(double a, double radius, double zn, double zf, double f, double cc, int n, int &A,
                                        int &B) {
    const double xl = a - radius, xh = a + radius;
    const double ul = f * (xl / (xl < 0.0 ? zn : zf)) + cc;
    const double uh = f * (xh / (xh > 0.0 ? zn : zf)) + cc;
    double Ad = floor(ul - FO_PAD), Bd = floor(uh + FO_PAD);
    if (!(Ad >= 0.0 && Bd <= (double)(n - 1))) return false;
    // With f > 0 every step from xl <= xh to A <= B is monotone, so 0 <= A <= B <= n - 1 and the two lines below change
    // nothing.  With an f the contract excludes they keep every gather inside the level.
    Bd = fmax(Bd, 0.0);
    Ad = fmin(Ad, Bd);
    A = (int)Ad;
    B = (int)Bd;
    return true;
}

__global__ __launch_bounds__(FO_THREADS) void field_observe_kernel(FoParams p, const float *__restrict__ pyr,
                                                                   const double *__restrict__ intr,
                                                                   const double *__restrict__ w2c,
                                                                   unsigned short *__restrict__ seen,
                                                                   unsigned short *__restrict__ looked) {
    __shared__ unsigned s_off[FO_MAX_LEVELS];
    const int t = threadIdx.x;
#pragma unroll
    for (int l = 0; l < FO_MAX_LEVELS; ++l)      // constant indices: the record stays in scalar registers
        if (t == l) s_off[l] = p.off[l];
    __syncthreads();
    const int b = blockIdx.x;
    const int bz = b % p.nbz, r = b / p.nbz, by = r % p.nby, bx = r / p.nby;
    const int i = bx * FO_BX + (t >> 6), j = by * FO_BY + ((t >> 3) & 7), k = bz * FO_BZ + (t & 7);
    const bool live = i < p.g.X && j < p.g.Y && k < p.g.Z;
    const int lo[3] = {bx * FO_BX, by * FO_BY, bz * FO_BZ};
    const int hi[3] = {min(lo[0] + FO_BX, p.g.X) - 1, min(lo[1] + FO_BY, p.g.Y) - 1, min(lo[2] + FO_BZ, p.g.Z) - 1};
    const double c0 = p.g.lo[0] + ((double)i + 0.5) * p.g.h;
    const double c1 = p.g.lo[1] + ((double)j + 0.5) * p.g.h;
    const double c2 = p.g.lo[2] + ((double)k + 0.5) * p.g.h;
    const double radius = p.radius;
    unsigned n_seen = 0u, n_looked = 0u;
    for (int view = 0; view < p.V; ++view) {
        const double *E = w2c + 12 * (size_t)view;
        const double *K = intr + 4 * (size_t)view;
        if (!fo_brick_sees(p, E, K, lo, hi)) continue;
        if (!live) continue;
        const double p2 = ((E[8] * c0 + E[9] * c1) + E[10] * c2) + E[11];
        const double zn = p2 - radius, zf = p2 + radius;
        if (!(zn >= p.near)) continue;
        const double p0 = ((E[0] * c0 + E[1] * c1) + E[2] * c2) + E[3];
        const double p1 = ((E[4] * c0 + E[5] * c1) + E[6] * c2) + E[7];
        int Au, Bu, Av, Bv;
        if (!fo_axis(p0, radius, zn, zf, K[0], K[2], p.W, Au, Bu)) continue;
        if (!fo_axis(p1, radius, zn, zf, K[1], K[3], p.H, Av, Bv)) continue;
        ++n_looked;
        int l = 0;
        while (l < p.levels - 1 && ((Bu >> l) - (Au >> l) > 1 || (Bv >> l) - (Av >> l) > 1)) ++l;
        const int Wl = (p.W + (1 << l) - 1) >> l;
        const float *lev = pyr + (size_t)view * (size_t)p.S + s_off[l];
        const int x0 = Au >> l, x1 = Bu >> l, y0 = Av >> l, y1 = Bv >> l;
        const float m = fminf(fminf(lev[(size_t)y0 * Wl + x0], lev[(size_t)y0 * Wl + x1]),
                              fminf(lev[(size_t)y1 * Wl + x0], lev[(size_t)y1 * Wl + x1]));
        if ((double)m > zf + p.margin) ++n_seen;
    }
    if (live) {
        const size_t idx = p.g.at(i, j, k);
        seen[idx] = (unsigned short)min(65535u, (unsigned)seen[idx] + n_seen);
        if (looked) looked[idx] = (unsigned short)min(65535u, (unsigned)looked[idx] + n_looked);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
// the levels of an H x W frame: their offsets into `off` (when given), their number, and the total S
static int fo_levels(int H, int W, long long *off, long long *S) {
    long long at = 0;
    int l = 0;
    for (;; ++l) {
        const long long h = ((long long)H + (1ll << l) - 1) >> l, w = ((long long)W + (1ll << l) - 1) >> l;
        if (off) off[l] = at;
        at += h * w;
        if (h == 1 && w == 1) break;
    }
    *S = at;
    return l + 1;
}

static bool fo_frame_ok(int H, int W) { return H >= 1 && W >= 1 && H <= GG_TSDF_MAX_SIDE && W <= GG_TSDF_MAX_SIDE; }

extern "C" int64_t gg_depth_min_pyramid_size(int height, int width) {
    if (!fo_frame_ok(height, width)) return 0;
    long long S;
    fo_levels(height, width, nullptr, &S);
    return (int64_t)S;
}

static unsigned fp_blocks(long long total) {
    const long long b = (total + FP_THREADS - 1) / FP_THREADS;
    return (unsigned)(b < (1ll << 30) ? b : (1ll << 30));      // the kernels stride over what is left
}

extern "C" int gg_depth_min_pyramid(int num_views, int height, int width, const float *depth, float *pyr,
                                    gg_stream_t stream) {
    GG_REQUIRE(num_views >= 0 && num_views <= GG_TSDF_MAX_VIEWS, "need 0 <= num_views <= GG_TSDF_MAX_VIEWS");
    GG_REQUIRE(fo_frame_ok(height, width), "need 1 <= height, width <= GG_TSDF_MAX_SIDE");
    if (num_views == 0) return GG_OK;
    GG_REQUIRE(depth && pyr, "null pointer: depth / pyr");
    GG_REQUIRE((((uintptr_t)depth | (uintptr_t)pyr) & 3) == 0, "depth / pyr misaligned");
    long long off[FO_MAX_LEVELS], S;
    const int levels = fo_levels(height, width, off, &S);
    hipStream_t s = (hipStream_t)stream;
    const int H1 = (height + 1) >> 1, W1 = (width + 1) >> 1;
    gg_prof_begin(GG_K_DEPTH_PYRAMID, s);
    long long total = (long long)num_views * H1 * W1;
    hipLaunchKernelGGL(depth_pyramid_base_kernel, dim3(fp_blocks(total)), dim3(FP_THREADS), 0, s, total, height, width,
                       H1, W1, S, levels > 1 ? 1 : 0, depth, pyr);
    for (int l = 2; l < levels; ++l) {
        const int Hs = (height + (1 << (l - 1)) - 1) >> (l - 1), Ws = (width + (1 << (l - 1)) - 1) >> (l - 1);
        const int Hd = (height + (1 << l) - 1) >> l, Wd = (width + (1 << l) - 1) >> l;
        total = (long long)num_views * Hd * Wd;
        hipLaunchKernelGGL(depth_pyramid_level_kernel, dim3(fp_blocks(total)), dim3(FP_THREADS), 0, s, total, Hs, Ws, Hd,
                           Wd, S, off[l - 1], off[l], pyr);
    }
    gg_prof_end(GG_K_DEPTH_PYRAMID, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_field_observe(const int32_t *dims, const double *grid, int num_views, int height, int width,
                                const float *pyr, const double *intrinsics, const double *w2c, double radius,
                                double margin, double near, uint16_t *seen, uint16_t *looked, gg_stream_t stream) {
    GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
    GG_REQUIRE(grid, "null pointer: grid (a host array of 4 doubles)");
    FieldGrid g;
    GG_REQUIRE(field_grid(dims, grid, &g), FIELD_GRID_MSG);
    GG_REQUIRE(num_views >= 0 && num_views <= GG_TSDF_MAX_VIEWS, "need 0 <= num_views <= GG_TSDF_MAX_VIEWS");
    GG_REQUIRE(fo_frame_ok(height, width), "need 1 <= height, width <= GG_TSDF_MAX_SIDE");
    GG_REQUIRE(isfinite(radius) && radius > 0.0, "radius must be finite and > 0");
    GG_REQUIRE(isfinite(margin) && margin >= 0.0, "margin must be finite and >= 0");
    GG_REQUIRE(isfinite(near) && near > 0.0, "near must be finite and > 0");
    if (num_views == 0) return GG_OK;
    GG_REQUIRE(seen, "null pointer: seen");
    GG_REQUIRE(pyr && intrinsics && w2c, "null pointer: pyr / intrinsics / w2c");
    GG_REQUIRE(((uintptr_t)pyr & 3) == 0 && (((uintptr_t)intrinsics | (uintptr_t)w2c) & 7) == 0 &&
                   (((uintptr_t)seen | (uintptr_t)looked) & 1) == 0,
               "pyr / intrinsics / w2c / seen / looked misaligned");
    FoParams p;
    p.g = g;
    p.V = num_views, p.H = height, p.W = width;
    p.nby = (g.Y + FO_BY - 1) / FO_BY, p.nbz = (g.Z + FO_BZ - 1) / FO_BZ;
    p.radius = radius, p.margin = margin, p.near = near;
    long long off[FO_MAX_LEVELS], S;
    p.levels = fo_levels(height, width, off, &S);
    p.S = S;
    for (int l = 0; l < FO_MAX_LEVELS; ++l) p.off[l] = (unsigned)off[l < p.levels ? l : p.levels - 1];
    const int64_t nbx = (g.X + FO_BX - 1) / FO_BX;
    const unsigned blocks = (unsigned)(nbx * p.nby * p.nbz);      // <= 2^27 / 256 bricks of whole cells, and edges
    hipStream_t s = (hipStream_t)stream;
    gg_prof_begin(GG_K_FIELD_OBSERVE, s);
    hipLaunchKernelGGL(field_observe_kernel, dim3(blocks), dim3(FO_THREADS), 0, s, p, pyr, intrinsics, w2c,
                       reinterpret_cast<unsigned short *>(seen), reinterpret_cast<unsigned short *>(looked));
    gg_prof_end(GG_K_FIELD_OBSERVE, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
