// field.hip — the scene as a distance field: Gaussians splatted into integer occupancy mass, the exact squared
// Euclidean distance transform of the occupied cells, and many gripper paths tested against it.  The contract is in
// include/gg_raster.h (gg_field_*) and PARITY.md "Distance field"; the design in DESIGN.md §3.25.
//
// gg_field_splat      one launch, a thread per row.  A row whose reach is at most FS_THREAD_REACH cells walks its own
//                     box (at most 125 cells).  The rows of a wave that reach further are then taken one at a time
//                     by the whole wave (ballot, wave-uniform row index): the 64 lanes stride over the flattened box,
//                     z fastest, so that a wave's atomics fall on runs of neighbouring cells.  Votes are int64 and
//                     added with 64-bit integer atomics: no order of the adds changes a bit of `mass`.
// gg_field_distance   (and gg_field_distance_known, the same passes with one more seed rule) three launches of one
//                     kernel, z then y then x: a workgroup stages FD_TILE whole lines in LDS,
//                     and every thread finds its cell's minimum by an outward search that ends at delta^2 >= best.
//                     A pass reads and writes only its own lines, so y runs in place on the workspace.
// gg_field_paths      a thread per pose with the spheres in LDS, then a thread per path for first_hit.  No atomics.
// gg_field_route      the cost-to-go over the free cells.  The volume is cut into bricks of FR_BRICK^3
//                     cells.  A round is one launch with a workgroup per brick; the workgroup of a brick that is
//                     not flagged returns, an active one loads its costs and free bits with a one-cell halo into
//                     LDS, relaxes the 26 moves there until nothing changes, writes back what fell and flags (for the
//                     next round) the neighbours that read a changed outer cell.  No workgroup waits for another:
//                     every dependency is a launch boundary, and the host reads one array of counters per FR_BATCH
//                     rounds to see that a round flagged nothing.
// gg_field_descend    a wave per path: lane m < 27 tests move m, a ballot's lowest set lane is the tie rule.
// gg_field_sight      a lane per segment: the integer boundary walk between two cell centres over its whole cover
//                     (DESIGN.md §3.30); a tie of two or three crossings opens every cell that touches the point.
// gg_field_shortcut   a workgroup per path: its 256 lanes walk 256 candidate segments from the anchor, each leaving
//                     at its first cell that is not free; the highest set lane of each wave's ballot, and the largest
//                     of the four in LDS, is the farthest clear candidate.
#include <math.h>

#include "field_volume.h"

#define FS_THREADS 256
#define FS_THREAD_REACH 2          // rows that reach further are walked by their whole wave
#define FD_THREADS 256
#define FD_TILE 8                  // lines per workgroup of a distance pass
#define FP_THREADS 256
#define FR_BRICK 8                 // cells per brick edge
#define FR_HALO 10                 // FR_BRICK + 2: the brick with its one-cell halo
#define FR_THREADS 256             // two cells of a brick per thread; four paths (waves) per workgroup of the descent;
                                   // one path per workgroup of the shortcut
#define FR_BATCH 16                // rounds enqueued between two read-backs of the counters

// ---------------------------------------------------------------------------------------------------------------
// splat
// ---------------------------------------------------------------------------------------------------------------
struct FsRow {
    double m[3], R[9], A[3], rhs;
    int c[3];                      // the mean's cell, per axis, inside the volume or not
    int reach;
    long long q;
    bool ok, cut;
};

// Row i as every lane that works on it needs it; i >= N gives a row that takes no part (and is not counted).
__device__ __forceinline__ void fs_row(const FieldGrid &g, int i, int N, const float *__restrict__ means,
                                       const float *__restrict__ rot, const float *__restrict__ scales,
                                       const float *__restrict__ weights, double k, int max_reach, double min_weight,
                                       FsRow &r) {
    r.ok = false;
    r.cut = false;
    r.reach = 0;
    r.q = 0;
    r.rhs = 0.0;
    r.c[0] = r.c[1] = r.c[2] = 0;
    if (i >= N) return;
    bool fin = true;
    float smax = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float m = means[(size_t)i * 3 + a], s = scales[(size_t)i * 3 + a];
        fin = fin && isfinite(m) && isfinite(s) && s > 0.0f;
        r.m[a] = (double)m;
        r.A[a] = (double)s * (double)s;
        smax = fmaxf(smax, s);
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) {
        const float v = rot[(size_t)i * 9 + a];
        fin = fin && isfinite(v);
        r.R[a] = (double)v;
    }
    const float wf = weights[i];
    const double w = (double)wf;
    if (!(fin && isfinite(wf) && min_weight < w && w < 32768.0)) return;
    r.ok = true;
    r.q = (long long)(w * 65536.0);            // exact product, truncated: |q| < 2^31
    r.rhs = (k * k) * ((r.A[0] * r.A[1]) * r.A[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) r.c[a] = field_cell(r.m[a] - g.lo[a], g.h);
    // n: the smallest integer >= 0 with n h >= k smax, followed as far as GG_FIELD_MAX_REACH + 1: the division
    // proposes, the comparisons decide
    const double rad = k * (double)smax;
    const double e = ceil(rad / g.h);
    int n = e >= (double)(GG_FIELD_MAX_REACH + 1) ? GG_FIELD_MAX_REACH + 1 : (int)e;
    while (n > 0 && (double)(n - 1) * g.h >= rad) --n;
    while (n <= GG_FIELD_MAX_REACH && (double)n * g.h < rad) ++n;
    r.cut = n + 1 > max_reach;
    r.reach = r.cut ? max_reach : n + 1;
}

// Cell (x, y, z) of the volume: the mean's cell votes always, another one when its centre is in the closed ellipsoid.
__device__ __forceinline__ void fs_cell(const FieldGrid &g, const FsRow &r, int x, int y, int z,
                                        unsigned long long vote, unsigned long long *__restrict__ mass) {
    bool hit = x == r.c[0] && y == r.c[1] && z == r.c[2];
    if (!hit) {
        const double d0 = (g.lo[0] + ((double)x + 0.5) * g.h) - r.m[0];
        const double d1 = (g.lo[1] + ((double)y + 0.5) * g.h) - r.m[1];
        const double d2 = (g.lo[2] + ((double)z + 0.5) * g.h) - r.m[2];
        const double u0 = (r.R[0] * d0 + r.R[3] * d1) + r.R[6] * d2;
        const double u1 = (r.R[1] * d0 + r.R[4] * d1) + r.R[7] * d2;
        const double u2 = (r.R[2] * d0 + r.R[5] * d1) + r.R[8] * d2;
        const double lhs =
            ((u0 * u0) * (r.A[1] * r.A[2]) + (u1 * u1) * (r.A[0] * r.A[2])) + (u2 * u2) * (r.A[0] * r.A[1]);
        hit = lhs <= r.rhs;
    }
    if (hit) atomicAdd(mass + g.at(x, y, z), vote);
}

// The row's box cut to the volume: lo[a] <= hi[a] on every axis, or false.  c is within +-2^30 and reach <= 64.
__device__ __forceinline__ bool fs_box(const FieldGrid &g, const FsRow &r, int *lo, int *hi) {
    const int dim[3] = {g.X, g.Y, g.Z};
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = max(r.c[a] - r.reach, 0);
        hi[a] = min(r.c[a] + r.reach, dim[a] - 1);
        any = any && lo[a] <= hi[a];
    }
    return any;
}

__global__ __launch_bounds__(FS_THREADS) void field_splat_kernel(FieldGrid g, int N, const float *__restrict__ means,
                                                                 const float *__restrict__ rot,
                                                                 const float *__restrict__ scales,
                                                                 const float *__restrict__ weights, double k,
                                                                 int max_reach, double min_weight, int sign,
                                                                 unsigned long long *__restrict__ mass,
                                                                 unsigned long long *__restrict__ skipped,
                                                                 unsigned long long *__restrict__ truncated) {
    const int i = blockIdx.x * FS_THREADS + threadIdx.x;      // N <= 2^30 and the grid covers N: no overflow
    const int lane = threadIdx.x & 63;
    FsRow r;
    fs_row(g, i, N, means, rot, scales, weights, k, max_reach, min_weight, r);
    const uint64_t skip = __ballot(i < N && !r.ok), cut = __ballot(r.ok && r.cut);
    if (lane == 0) {
        if (skip) atomicAdd(skipped, (unsigned long long)__builtin_popcountll(skip));
        if (cut) atomicAdd(truncated, (unsigned long long)__builtin_popcountll(cut));
    }
    int lo[3], hi[3];
    const bool wide = r.ok && r.reach > FS_THREAD_REACH;
    if (r.ok && !wide && fs_box(g, r, lo, hi)) {
        const unsigned long long vote = sign > 0 ? (unsigned long long)r.q : 0ull - (unsigned long long)r.q;
        for (int x = lo[0]; x <= hi[0]; ++x)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int z = lo[2]; z <= hi[2]; ++z) fs_cell(g, r, x, y, z, vote, mass);
    }
    // the wave's wide rows, one at a time, by all of its lanes
    const int wave_first = i - lane;
    for (uint64_t rem = __ballot(wide); rem != 0ull; rem &= rem - 1ull) {
        const int src = __builtin_amdgcn_readfirstlane(wave_first + (int)__builtin_ctzll(rem));
        FsRow b;
        fs_row(g, src, N, means, rot, scales, weights, k, max_reach, min_weight, b);
        if (!fs_box(g, b, lo, hi)) continue;
        const unsigned long long vote = sign > 0 ? (unsigned long long)b.q : 0ull - (unsigned long long)b.q;
        const int ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
        const int total = (hi[0] - lo[0] + 1) * ny * nz;      // <= 129^3
        for (int t = lane; t < total; t += 64) {
            const int xy = t / nz, z = t - xy * nz;
            const int x = xy / ny, y = xy - x * ny;
            fs_cell(g, b, lo[0] + x, lo[1] + y, lo[2] + z, vote, mass);
        }
    }
}

__global__ void field_zero2_kernel(unsigned long long *a, unsigned long long *b) {
    *a = 0ull;
    *b = 0ull;
}

// ---------------------------------------------------------------------------------------------------------------
// distance transform
// ---------------------------------------------------------------------------------------------------------------
// One min-plus pass along an axis of length L and element stride B: line n (of cells / L) starts at
// (n / B) L B + n % B.  z: B = 1; y: B = Z; x: B = Y Z.  A workgroup owns FD_TILE consecutive lines and keeps them in
// LDS as tile[l][t], or tile[t][l] (one int of padding per line) when the lines themselves are contiguous (UNIT:
// B == 1), so that in both cases neighbouring threads read neighbouring addresses of memory and of LDS.
// FIRST: the input is the mass (f = seed ? 0 : FAR, fd_seed).  LAST: the output is clamped to FAR.
// The seed rule, in this one place: a cell seeds the transform iff it is occupied or, with `seen` given
// (gg_field_distance_known), not seen free by min_views views.
__device__ __forceinline__ bool fd_seed(const long long *__restrict__ mass, long long threshold,
                                        const unsigned short *__restrict__ seen, int min_views, long long at) {
    return mass[at] >= threshold || (seen && (int)seen[at] < min_views);
}

template <bool UNIT, bool FIRST, bool LAST>
__global__ __launch_bounds__(FD_THREADS) void field_distance_kernel(int L, long long B, long long lines,
                                                                    const long long *__restrict__ mass,
                                                                    long long threshold,
                                                                    const unsigned short *__restrict__ seen,
                                                                    int min_views, const int *src, int *dst) {
    extern __shared__ int fd_tile[];
    const long long line0 = (long long)blockIdx.x * FD_TILE;
    const int nt = (int)min((long long)FD_TILE, lines - line0);
    const int work = nt * L;
    for (int idx = threadIdx.x; idx < work; idx += FD_THREADS) {
        const int t = UNIT ? idx / L : idx % nt, l = UNIT ? idx - t * L : idx / nt;
        const long long n = line0 + t;
        const long long at = (n / B) * ((long long)L * B) + n % B + (long long)l * B;
        int f;
        if (FIRST)
            f = fd_seed(mass, threshold, seen, min_views, at) ? 0 : GG_FIELD_FAR;
        else
            f = src[at];
        fd_tile[UNIT ? t * (L + 1) + l : l * FD_TILE + t] = f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < work; idx += FD_THREADS) {
        const int t = UNIT ? idx / L : idx % nt, l = UNIT ? idx - t * L : idx / nt;
        const int *col = fd_tile + (UNIT ? t * (L + 1) : t);
        const int step = UNIT ? 1 : FD_TILE;
        int best = col[l * step];
        // outward: a candidate at distance d is at least d^2, so the search ends once d^2 >= best
        for (int d = 1; d < L; ++d) {
            const int dd = d * d;
            if (dd >= best) break;
            const bool below = l - d >= 0, above = l + d < L;
            if (!below && !above) break;
            if (below) best = min(best, col[(l - d) * step] + dd);
            if (above) best = min(best, col[(l + d) * step] + dd);
        }
        if (LAST) best = min(best, GG_FIELD_FAR);
        const long long n = line0 + t;
        dst[(n / B) * ((long long)L * B) + n % B + (long long)l * B] = best;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// paths
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FP_THREADS) void field_paths_kernel(FieldGrid g, const int *__restrict__ dist2,
                                                                 int poses_total, const float *__restrict__ poses,
                                                                 int S, const float *__restrict__ spheres,
                                                                 const int *__restrict__ need2, int outside,
                                                                 int *__restrict__ slack) {
    __shared__ float s_c[GG_FIELD_MAX_SPHERES * 3];
    __shared__ int s_need[GG_FIELD_MAX_SPHERES];
    for (int k = threadIdx.x; k < S; k += FP_THREADS) {
        s_c[3 * k] = spheres[3 * k];
        s_c[3 * k + 1] = spheres[3 * k + 1];
        s_c[3 * k + 2] = spheres[3 * k + 2];
        s_need[k] = need2[k];
    }
    __syncthreads();
    const int i = blockIdx.x * FP_THREADS + threadIdx.x;      // poses_total <= 2^26
    if (i >= poses_total) return;
    double T[12];
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float v = poses[(size_t)i * 12 + k];
        fin = fin && isfinite(v);
        T[k] = (double)v;
    }
    if (!fin) {
        slack[i] = INT32_MIN;
        return;
    }
    int m = GG_FIELD_FAR;
    for (int s = 0; s < S; ++s) {
        const int d = field_probe(g, dist2, T, (double)s_c[3 * s], (double)s_c[3 * s + 1], (double)s_c[3 * s + 2], outside);
        m = min(m, d - s_need[s]);
    }
    slack[i] = m;
}

__global__ __launch_bounds__(FP_THREADS) void field_first_hit_kernel(int P, int W, const int *__restrict__ slack,
                                                                     int *__restrict__ first_hit) {
    const int p = blockIdx.x * FP_THREADS + threadIdx.x;
    if (p >= P) return;
    int w = 0;
    while (w < W && slack[(size_t)p * W + w] >= 0) ++w;
    first_hit[p] = w;
}

// ---------------------------------------------------------------------------------------------------------------
// route: the cost-to-go over the free cells, and the descent along it
// ---------------------------------------------------------------------------------------------------------------
// Move m = (dx + 1) 9 + (dy + 1) 3 + (dz + 1); m == 13 is no move.  Its weight is 3, 4 or 5 (the 3-4-5 chamfer).
__device__ __forceinline__ constexpr int fr_dx(int m) { return m / 9 - 1; }
__device__ __forceinline__ constexpr int fr_dy(int m) { return (m / 3) % 3 - 1; }
__device__ __forceinline__ constexpr int fr_dz(int m) { return m % 3 - 1; }
__device__ __forceinline__ constexpr int fr_weight(int m) {
    return 2 + (fr_dx(m) != 0) + (fr_dy(m) != 0) + (fr_dz(m) != 0);
}
// The cells move m needs free, as bits numbered like the moves: every c + e with e_a in {0, d_a} (bit 13 is c).
__device__ __forceinline__ constexpr unsigned fr_block_mask(int m) {
    unsigned mask = 0u;
    for (int a = 0; a <= (fr_dx(m) != 0); ++a)
        for (int b = 0; b <= (fr_dy(m) != 0); ++b)
            for (int c = 0; c <= (fr_dz(m) != 0); ++c)
                mask |= 1u << ((a * fr_dx(m) + 1) * 9 + (b * fr_dy(m) + 1) * 3 + (c * fr_dz(m) + 1));
    return mask;
}

// Reads and writes of `cost` that may meet another brick's within a round: relaxed, at the device's scope.
__device__ __forceinline__ int fr_load(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fr_store(int *p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// cost = FAR, the workspace (counters and both flag arrays) and `ignored` zero
__global__ __launch_bounds__(FR_THREADS) void route_init_kernel(long long cells, int *__restrict__ cost,
                                                                long long ws_words, unsigned *__restrict__ ws,
                                                                unsigned long long *__restrict__ ignored) {
    const long long i = (long long)blockIdx.x * FR_THREADS + threadIdx.x;
    if (i < cells) cost[i] = GG_FIELD_FAR;
    if (i < ws_words) ws[i] = 0u;
    if (i == 0) *ignored = 0ull;
}

__global__ __launch_bounds__(FR_THREADS) void route_zero_kernel(unsigned *p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0u;
}

// A goal that is inside and free costs 0.  Its brick and the bricks around it start active: a goal in an outer
// layer is read by them, and no round's write-back announces it.
__global__ __launch_bounds__(FR_THREADS) void route_goals_kernel(FieldFree v, int bx, int by, int bz, int G,
                                                                 const int *__restrict__ goals, int *cost,
                                                                 unsigned *flags,
                                                                 unsigned long long *__restrict__ ignored) {
    const int i = blockIdx.x * FR_THREADS + threadIdx.x;      // G <= GG_FIELD_MAX_GOALS
    if (i >= G) return;
    const int x = goals[(size_t)i * 3], y = goals[(size_t)i * 3 + 1], z = goals[(size_t)i * 3 + 2];
    if (!v.open(x, y, z)) {
        atomicAdd(ignored, 1ull);
        return;
    }
    fr_store(cost + v.at(x, y, z), 0);
    const int ix = x / FR_BRICK, iy = y / FR_BRICK, iz = z / FR_BRICK;
    for (int a = max(ix - 1, 0); a <= min(ix + 1, bx - 1); ++a)
        for (int b = max(iy - 1, 0); b <= min(iy + 1, by - 1); ++b)
            for (int c = max(iz - 1, 0); c <= min(iz + 1, bz - 1); ++c) flags[((size_t)a * by + b) * bz + c] = 1u;
}

// One round, one workgroup per brick.  `cur` holds this round's flags, `next` the next round's: a brick clears its
// own flag in cur, other bricks only set flags in next, so cur is all zero when the round is over and serves as the
// round after next's `next` without a fill.  *counter: the flags this round turned from 0 to 1.
__global__ __launch_bounds__(FR_THREADS) void route_round_kernel(FieldFree v, int bx, int by, int bz, int *cost,
                                                                 unsigned *cur, unsigned *next, unsigned *counter) {
    __shared__ int s_cost[FR_HALO * FR_HALO * FR_HALO];
    __shared__ unsigned char s_free[FR_HALO * FR_HALO * FR_HALO];
    __shared__ unsigned s_active, s_dirs;
    const int tid = threadIdx.x;
    const int brick = blockIdx.x;
    if (tid == 0) {
        s_active = cur[brick];
        s_dirs = 0u;
        if (s_active) cur[brick] = 0u;
    }
    __syncthreads();
    if (!s_active) return;
    const int iz = brick % bz, iy = (brick / bz) % by, ix = brick / (bz * by);
    const int x0 = ix * FR_BRICK, y0 = iy * FR_BRICK, z0 = iz * FR_BRICK;
    for (int i = tid; i < FR_HALO * FR_HALO * FR_HALO; i += FR_THREADS) {
        const int x = x0 + i / (FR_HALO * FR_HALO) - 1, y = y0 + (i / FR_HALO) % FR_HALO - 1, z = z0 + i % FR_HALO - 1;
        const bool open = v.open(x, y, z);
        s_free[i] = open ? 1 : 0;
        s_cost[i] = open ? fr_load(cost + v.at(x, y, z)) : GG_FIELD_FAR;
    }
    __syncthreads();
    // two cells per thread: their place in LDS, the cost they were loaded with, and the moves they may make
    int at[2], loaded[2], own[2];
    unsigned allow[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = tid + k * FR_THREADS;
        at[k] = (((i >> 6) + 1) * FR_HALO + ((i >> 3) & 7) + 1) * FR_HALO + (i & 7) + 1;
        loaded[k] = own[k] = s_cost[at[k]];
        unsigned open = 0u;
#pragma unroll
        for (int m = 0; m < 27; ++m)
            open |= (unsigned)s_free[at[k] + (fr_dx(m) * FR_HALO + fr_dy(m)) * FR_HALO + fr_dz(m)] << m;
        allow[k] = 0u;
#pragma unroll
        for (int m = 0; m < 27; ++m)
            if (m != 13 && (open & fr_block_mask(m)) == fr_block_mask(m)) allow[k] |= 1u << m;
    }
    // Jacobi sweeps in LDS: all read, then all write.  Every sweep that goes on lowers a cell, costs are integers
    // >= 0, so the loop ends; it waits for nothing outside this workgroup.
    for (;;) {
        int nv[2];
        bool fell = false;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            nv[k] = own[k];
#pragma unroll
            for (int m = 0; m < 27; ++m)
                if (m != 13 && (allow[k] >> m & 1u))
                    nv[k] = min(nv[k], s_cost[at[k] + (fr_dx(m) * FR_HALO + fr_dy(m)) * FR_HALO + fr_dz(m)] + fr_weight(m));
            fell = fell || nv[k] < own[k];
        }
        if (!__syncthreads_or(fell)) break;
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (nv[k] < own[k]) s_cost[at[k]] = own[k] = nv[k];
        __syncthreads();
    }
    // write back what fell; a changed cell of the outer layer is read by the bricks on its side(s)
    unsigned dirs = 0u;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (own[k] >= loaded[k]) continue;
        const int i = tid + k * FR_THREADS;
        const int lx = i >> 6, ly = (i >> 3) & 7, lz = i & 7;
        fr_store(cost + v.at(x0 + lx, y0 + ly, z0 + lz), own[k]);
#pragma unroll
        for (int m = 0; m < 27; ++m) {
            const bool reads = (fr_dx(m) == 0 || lx == (fr_dx(m) < 0 ? 0 : FR_BRICK - 1)) &&
                               (fr_dy(m) == 0 || ly == (fr_dy(m) < 0 ? 0 : FR_BRICK - 1)) &&
                               (fr_dz(m) == 0 || lz == (fr_dz(m) < 0 ? 0 : FR_BRICK - 1));
            if (m != 13 && reads) dirs |= 1u << m;
        }
    }
    if (dirs) atomicOr(&s_dirs, dirs);
    __syncthreads();
    if (tid < 27 && (s_dirs >> tid & 1u)) {
        const int a = ix + fr_dx(tid), b = iy + fr_dy(tid), c = iz + fr_dz(tid);
        if (a >= 0 && a < bx && b >= 0 && b < by && c >= 0 && c < bz)
            if (atomicExch(next + ((size_t)a * by + b) * bz + c, 1u) == 0u) atomicAdd(counter, 1u);
    }
}

// One wave per path.  The walk ends by construction: every step lowers the cost by at least 3.
__global__ __launch_bounds__(FR_THREADS) void route_descend_kernel(FieldFree v, const int *__restrict__ cost, int P,
                                                                   const int *__restrict__ starts, int max_cells,
                                                                   int *__restrict__ cells, int *__restrict__ length) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * (FR_THREADS / 64) + (threadIdx.x >> 6);      // P max_cells <= GG_FIELD_MAX_POSES
    if (p >= P) return;                                                     // the same for the whole wave
    int c[3] = {starts[(size_t)p * 3], starts[(size_t)p * 3 + 1], starts[(size_t)p * 3 + 2]};
    int *row = cells + (size_t)p * max_cells * 3;
    int here = v.open(c[0], c[1], c[2]) ? cost[v.at(c[0], c[1], c[2])] : GG_FIELD_FAR;
    int n = 0;
    if (here < GG_FIELD_FAR) {
        const int m = lane, dx = fr_dx(m), dy = fr_dy(m), dz = fr_dz(m), w = fr_weight(m);
        const int bound = here / 3 + 1;
        if (lane == 0) row[0] = c[0], row[1] = c[1], row[2] = c[2];
        n = 1;
        for (int step = 0; step < bound && here > 0; ++step) {
            bool take = false;
            if (m < 27 && m != 13) {
                bool ok = true;
                for (int a = 0; a <= (dx != 0); ++a)
                    for (int b = 0; b <= (dy != 0); ++b)
                        for (int e = 0; e <= (dz != 0); ++e)
                            ok = ok && v.open(c[0] + a * dx, c[1] + b * dy, c[2] + e * dz);
                take = ok && cost[v.at(c[0] + dx, c[1] + dy, c[2] + dz)] + w == here;
            }
            const uint64_t found = __ballot(take);
            if (found == 0ull) break;                      // `cost` is no fixed point of this dist2 and need
            const int pick = (int)__builtin_ctzll(found);  // the lowest move number: the tie rule
            c[0] += fr_dx(pick), c[1] += fr_dy(pick), c[2] += fr_dz(pick);
            here -= fr_weight(pick);
            if (lane == 0 && n < max_cells) row[3 * n] = c[0], row[3 * n + 1] = c[1], row[3 * n + 2] = c[2];
            ++n;
        }
        if (here > 0) n = 0;
    }
    if (n == 0) c[0] = c[1] = c[2] = -1;
    for (int r = n + lane; r < max_cells; r += 64) row[3 * r] = c[0], row[3 * r + 1] = c[1], row[3 * r + 2] = c[2];
    if (lane == 0) length[p] = n;
}

// ---------------------------------------------------------------------------------------------------------------
// sight: the cover of a segment between two cell centres, and greedy string pulling on top of it
// ---------------------------------------------------------------------------------------------------------------
struct FrSight {
    int cover, blocked;
};

// The boundary walk from cell a to cell b, both inside the volume.  With n_a = |b_a - a_a| the segment crosses the
// k-th boundary of axis a at t_a = (2 k + 1) / (2 n_a); t_a < t_b iff (2 k_a + 1) n_b < (2 k_b + 1) n_a, products
// below 2^22.  An axis with n_a == 0 compares as t = infinity; one whose crossings are used up has t > 1, past every
// crossing still open.  A step takes every axis at the smallest t (the set `first`): the segment goes through a
// face, an edge or a corner there, and the 1, 3 or 7 cells c + e s, e a subset of `first` other than 0, are the cells
// that touch that point and have not been counted.  At most n_x + n_y + n_z steps, every cell inside the box of a, b.
// FIRST: return at the first cell that is not free (cover is then the cells counted so far).
template <bool FIRST>
__device__ __forceinline__ FrSight fr_walk(const FieldFree &v, int ax, int ay, int az, int bx, int by, int bz) {
    auto shut = [&](int x, int y, int z) { return v.dist2[v.at(x, y, z)] < v.need ? 1 : 0; };
    const int n0 = abs(bx - ax), n1 = abs(by - ay), n2 = abs(bz - az);
    const int s0 = bx > ax ? 1 : -1, s1 = by > ay ? 1 : -1, s2 = bz > az ? 1 : -1;
    int x = ax, y = ay, z = az, k0 = 0, k1 = 0, k2 = 0;
    FrSight r{1, shut(x, y, z)};
    if (FIRST && r.blocked) return r;
    const int total = n0 + n1 + n2;
    // the axis at the smallest t always has its flag set, so every step uses up a crossing; `step` bounds it anyway
    for (int done = 0, step = 0; done < total && step < total; ++step) {
        const int u0 = 2 * k0 + 1, u1 = 2 * k1 + 1, u2 = 2 * k2 + 1;
        const bool f0 = u0 * n1 <= u1 * n0 && u0 * n2 <= u2 * n0;
        const bool f1 = u1 * n0 <= u0 * n1 && u1 * n2 <= u2 * n1;
        const bool f2 = u2 * n0 <= u0 * n2 && u2 * n1 <= u1 * n2;
        const int first = (f0 ? 1 : 0) | (f1 ? 2 : 0) | (f2 ? 4 : 0);
#pragma unroll
        for (int e = 1; e < 8; ++e) {
            if ((e & ~first) != 0) continue;
            r.cover += 1;
            r.blocked += shut(x + ((e & 1) ? s0 : 0), y + ((e & 2) ? s1 : 0), z + ((e & 4) ? s2 : 0));
            if (FIRST && r.blocked) return r;
        }
        if (f0) x += s0, ++k0, ++done;
        if (f1) y += s1, ++k1, ++done;
        if (f2) z += s2, ++k2, ++done;
    }
    return r;
}

// One lane per segment, the whole cover.
__global__ __launch_bounds__(FR_THREADS) void route_sight_kernel(FieldFree v, int S, const int *__restrict__ a,
                                                                 const int *__restrict__ b, int *__restrict__ cover,
                                                                 int *__restrict__ blocked) {
    const int i = blockIdx.x * FR_THREADS + threadIdx.x;      // S <= GG_FIELD_MAX_POSES
    if (i >= S) return;
    const int ax = a[(size_t)i * 3], ay = a[(size_t)i * 3 + 1], az = a[(size_t)i * 3 + 2];
    const int bx = b[(size_t)i * 3], by = b[(size_t)i * 3 + 1], bz = b[(size_t)i * 3 + 2];
    FrSight r{0, -1};
    if (v.inside(ax, ay, az) && v.inside(bx, by, bz)) r = fr_walk<false>(v, ax, ay, az, bx, by, bz);
    cover[i] = r.cover;
    blocked[i] = r.blocked;
}

// One workgroup per path.  From anchor i the 256 lanes take 256 candidates j, chunk by chunk from the far end of the
// window towards i; lane l of a chunk that ends at `top` has j = top - 255 + l.  Each wave's ballot gives its largest
// clear j; the four meet in LDS (two buffers, used in turn, so one barrier per chunk is enough) and the largest of
// them is the chunk's answer.  The first chunk with a clear lane ends the scan.  i, top and next are the same in
// every lane of the workgroup, so every lane reaches every barrier.
__global__ __launch_bounds__(FR_THREADS) void route_shortcut_kernel(FieldFree v, int P, int max_cells,
                                                                    const int *__restrict__ cells,
                                                                    const int *__restrict__ length, int window,
                                                                    int *__restrict__ keep, int *__restrict__ count,
                                                                    int *__restrict__ blocked) {
    __shared__ int s_best[2][FR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;                                               // P max_cells <= GG_FIELD_MAX_POSES
    const int *row = cells + (size_t)p * max_cells * 3;
    int *out = keep + (size_t)p * max_cells;
    const int n = min(length[p], max_cells);
    int kept = 0, bad = 0, pad = -1, turn = 0;
    if (n > 0) {
        if (tid == 0) out[0] = 0;
        kept = 1;
        pad = n - 1;
        for (int i = 0; i < n - 1;) {
            const int ax = row[3 * i], ay = row[3 * i + 1], az = row[3 * i + 2];
            const bool from = v.inside(ax, ay, az);
            const int far = (int)min((long long)i + window, (long long)n - 1);
            int next = -1;
            for (int top = far; top > i && next < 0; top -= FR_THREADS) {
                const int j = top - (FR_THREADS - 1) + tid;
                bool clear = false;
                if (j > i && from) {
                    const int bx = row[3 * j], by = row[3 * j + 1], bz = row[3 * j + 2];
                    clear = v.inside(bx, by, bz) && fr_walk<true>(v, ax, ay, az, bx, by, bz).blocked == 0;
                }
                const uint64_t seen = __ballot(clear);
                if (lane == 0)
                    s_best[turn][wave] = seen != 0ull ? top - (FR_THREADS - 1) + wave * 64 + 63 - __builtin_clzll(seen) : -1;
                __syncthreads();
#pragma unroll
                for (int w = 0; w < FR_THREADS / 64; ++w) next = max(next, s_best[turn][w]);
                turn ^= 1;
            }
            if (next < 0) next = i + 1, ++bad;                              // no candidate is clear, i + 1 among them
            if (tid == 0) out[kept] = next;
            ++kept;
            i = next;
        }
    }
    for (int r = kept + tid; r < max_cells; r += FR_THREADS) out[r] = pad;
    if (tid == 0) count[p] = kept, blocked[p] = bad;
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
// num_paths rows of max_cells cells each, as gg_field_descend writes and gg_field_shortcut reads them
#define GG_REQUIRE_FIELD_PATHS(num_paths, max_cells)                                                              \
    GG_REQUIRE((num_paths) >= 0 && (max_cells) >= 1 && (int64_t)(num_paths) * (max_cells) <= GG_FIELD_MAX_POSES, \
               "need num_paths >= 0, max_cells >= 1 and num_paths max_cells <= GG_FIELD_MAX_POSES")

static FieldFree field_free(const int32_t *dims, const int32_t *dist2, int32_t need) {
    return FieldFree{{dims[0], dims[1], dims[2]}, dist2, need};
}

extern "C" int gg_field_splat(const int32_t *dims, const double *grid, int num_rows, const float *means,
                              const float *rot, const float *scales, const float *weights, double extent,
                              int max_reach, double min_weight, int sign, int64_t *mass, int64_t *skipped,
                              int64_t *truncated, gg_stream_t stream) {
    GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
    GG_REQUIRE(grid, "null pointer: grid (a host array of 4 doubles)");
    FieldGrid g;
    GG_REQUIRE(field_grid(dims, grid, &g), FIELD_GRID_MSG);
    GG_REQUIRE(num_rows >= 0 && num_rows <= GG_FIELD_MAX_ROWS, "need 0 <= num_rows <= GG_FIELD_MAX_ROWS");
    GG_REQUIRE(isfinite(extent) && extent >= 0.0, "extent must be finite and >= 0");
    GG_REQUIRE(max_reach >= 0 && max_reach <= GG_FIELD_MAX_REACH, "max_reach must be in 0..GG_FIELD_MAX_REACH");
    GG_REQUIRE(!isnan(min_weight), "min_weight is NaN");
    GG_REQUIRE(sign == 1 || sign == -1, "sign must be +1 or -1");
    if (num_rows == 0) return GG_OK;
    GG_REQUIRE(means && rot && scales && weights, "null pointer: means / rot / scales / weights");
    GG_REQUIRE(mass && skipped && truncated, "null pointer: mass / skipped / truncated");
    GG_REQUIRE((((uintptr_t)means | (uintptr_t)rot | (uintptr_t)scales | (uintptr_t)weights) & 3) == 0 &&
                   (((uintptr_t)mass | (uintptr_t)skipped | (uintptr_t)truncated) & 7) == 0,
               "means / rot / scales / weights / mass / skipped / truncated misaligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(field_zero2_kernel, dim3(1), dim3(1), 0, s, reinterpret_cast<unsigned long long *>(skipped),
                       reinterpret_cast<unsigned long long *>(truncated));
    hipLaunchKernelGGL(field_splat_kernel, dim3((unsigned)((num_rows + FS_THREADS - 1) / FS_THREADS)),
                       dim3(FS_THREADS), 0, s, g, num_rows, means, rot, scales, weights, extent, max_reach, min_weight,
                       sign, reinterpret_cast<unsigned long long *>(mass),
                       reinterpret_cast<unsigned long long *>(skipped),
                       reinterpret_cast<unsigned long long *>(truncated));
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" size_t gg_field_distance_workspace(const int32_t *dims) {
    if (!field_dims_ok(dims)) return 0;
    return gg_align_up((size_t)field_cells(dims) * 4, 256);
}

template <bool UNIT, bool FIRST, bool LAST>
static void field_distance_pass(hipStream_t s, int L, int64_t B, int64_t cells, const int64_t *mass, int64_t threshold,
                                const uint16_t *seen, int min_views, const int *src, int *dst) {
    const int64_t lines = cells / L;
    hipLaunchKernelGGL((field_distance_kernel<UNIT, FIRST, LAST>), dim3((unsigned)((lines + FD_TILE - 1) / FD_TILE)),
                       dim3(FD_THREADS), (size_t)FD_TILE * (L + 1) * sizeof(int), s, L, (long long)B, (long long)lines,
                       reinterpret_cast<const long long *>(mass), (long long)threshold,
                       reinterpret_cast<const unsigned short *>(seen), min_views, src, dst);
}

// The three passes of both distance entries; seen null: occupied cells alone seed.
static void field_distance_passes(hipStream_t s, const int32_t *dims, const int64_t *mass, int64_t threshold,
                                  const uint16_t *seen, int min_views, int32_t *dist2, void *ws) {
    const int64_t cells = field_cells(dims);
    const int Y = dims[1], Z = dims[2];
    int *f = (int *)ws;
    field_distance_pass<true, true, false>(s, Z, 1, cells, mass, threshold, seen, min_views, nullptr, f);
    if (Z == 1)
        field_distance_pass<true, false, false>(s, Y, 1, cells, nullptr, 0, nullptr, 0, f, f);
    else
        field_distance_pass<false, false, false>(s, Y, Z, cells, nullptr, 0, nullptr, 0, f, f);
    if ((int64_t)Y * Z == 1)
        field_distance_pass<true, false, true>(s, dims[0], 1, cells, nullptr, 0, nullptr, 0, f, dist2);
    else
        field_distance_pass<false, false, true>(s, dims[0], (int64_t)Y * Z, cells, nullptr, 0, nullptr, 0, f, dist2);
}

extern "C" int gg_field_distance(const int32_t *dims, const int64_t *mass, int64_t threshold, int32_t *dist2, void *ws,
                                 size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
    GG_REQUIRE(threshold >= 1, "threshold must be >= 1");
    GG_REQUIRE(mass && dist2, "null pointer: mass / dist2");
    GG_REQUIRE(((uintptr_t)mass & 7) == 0 && ((uintptr_t)dist2 & 3) == 0, "mass / dist2 misaligned");
    GG_REQUIRE_WS(ws, ws_bytes, gg_field_distance_workspace(dims));
    field_distance_passes((hipStream_t)stream, dims, mass, threshold, nullptr, 0, dist2, ws);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_field_distance_known(const int32_t *dims, const int64_t *mass, int64_t threshold,
                                       const uint16_t *seen, int min_views, int32_t *dist2, void *ws, size_t ws_bytes,
                                       gg_stream_t stream) {
    GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
    GG_REQUIRE(threshold >= 1, "threshold must be >= 1");
    GG_REQUIRE(min_views >= 1 && min_views <= 65535, "min_views must be in 1..65535");
    GG_REQUIRE(mass && seen && dist2, "null pointer: mass / seen / dist2");
    GG_REQUIRE(((uintptr_t)mass & 7) == 0 && ((uintptr_t)seen & 1) == 0 && ((uintptr_t)dist2 & 3) == 0,
               "mass / seen / dist2 misaligned");
    GG_REQUIRE_WS(ws, ws_bytes, gg_field_distance_workspace(dims));
    hipStream_t s = (hipStream_t)stream;
    gg_prof_begin(GG_K_FIELD_DISTANCE_KNOWN, s);
    field_distance_passes(s, dims, mass, threshold, seen, min_views, dist2, ws);
    gg_prof_end(GG_K_FIELD_DISTANCE_KNOWN, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_field_paths(const int32_t *dims, const double *grid, const int32_t *dist2, int num_paths,
                              int num_waypoints, const float *poses, int num_spheres, const float *spheres,
                              const int32_t *need2, int32_t outside, int32_t *slack, int32_t *first_hit,
                              gg_stream_t stream) {
    GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
    GG_REQUIRE(grid, "null pointer: grid (a host array of 4 doubles)");
    FieldGrid g;
    GG_REQUIRE(field_grid(dims, grid, &g), FIELD_GRID_MSG);
    GG_REQUIRE(num_paths >= 0 && num_waypoints >= 0, "num_paths / num_waypoints < 0");
    GG_REQUIRE((int64_t)num_paths * num_waypoints <= GG_FIELD_MAX_POSES,
               "num_paths num_waypoints > GG_FIELD_MAX_POSES");
    GG_REQUIRE(num_spheres >= 0 && num_spheres <= GG_FIELD_MAX_SPHERES,
               "num_spheres must be in 0..GG_FIELD_MAX_SPHERES");
    GG_REQUIRE(outside >= 0 && outside <= GG_FIELD_FAR, "outside must be in 0..GG_FIELD_FAR");
    if (num_paths == 0 || num_waypoints == 0) return GG_OK;
    GG_REQUIRE(dist2 && poses && slack && first_hit, "null pointer: dist2 / poses / slack / first_hit");
    GG_REQUIRE(num_spheres == 0 || (spheres && need2), "null pointer: spheres / need2");
    GG_REQUIRE((((uintptr_t)dist2 | (uintptr_t)poses | (uintptr_t)spheres | (uintptr_t)need2 | (uintptr_t)slack |
                 (uintptr_t)first_hit) & 3) == 0,
               "dist2 / poses / spheres / need2 / slack / first_hit misaligned");
    hipStream_t s = (hipStream_t)stream;
    const int total = num_paths * num_waypoints;
    hipLaunchKernelGGL(field_paths_kernel, dim3((unsigned)((total + FP_THREADS - 1) / FP_THREADS)), dim3(FP_THREADS), 0,
                       s, g, dist2, total, poses, num_spheres, spheres, need2, outside, slack);
    hipLaunchKernelGGL(field_first_hit_kernel, dim3((unsigned)((num_paths + FP_THREADS - 1) / FP_THREADS)),
                       dim3(FP_THREADS), 0, s, num_paths, num_waypoints, slack, first_hit);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

static void route_bricks(const int32_t *dims, int *b) {
    for (int a = 0; a < 3; ++a) b[a] = (dims[a] + FR_BRICK - 1) / FR_BRICK;
}

// the counters of one batch of rounds, then the two flag arrays: one 32-bit word each
static size_t route_ws_words(const int32_t *dims) {
    int b[3];
    route_bricks(dims, b);
    return (size_t)FR_BATCH + 2 * ((size_t)b[0] * b[1] * b[2]);
}

extern "C" size_t gg_field_route_workspace(const int32_t *dims) {
    if (!field_dims_ok(dims)) return 0;
    return gg_align_up(route_ws_words(dims) * 4, 256);
}

extern "C" int gg_field_route(const int32_t *dims, const int32_t *dist2, int32_t need, int num_goals,
                              const int32_t *goals, int32_t *cost, int64_t *ignored, int max_rounds, int *rounds_out,
                              void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
    GG_REQUIRE_FIELD_NEED(need);
    GG_REQUIRE(num_goals >= 0 && num_goals <= GG_FIELD_MAX_GOALS, "need 0 <= num_goals <= GG_FIELD_MAX_GOALS");
    GG_REQUIRE(max_rounds >= 1, "max_rounds must be >= 1");
    GG_REQUIRE(rounds_out, "null pointer: rounds_out (a host int)");
    GG_REQUIRE(dist2 && cost && ignored, "null pointer: dist2 / cost / ignored");
    GG_REQUIRE(num_goals == 0 || goals, "null pointer: goals");
    GG_REQUIRE((((uintptr_t)dist2 | (uintptr_t)goals | (uintptr_t)cost) & 3) == 0 && ((uintptr_t)ignored & 7) == 0,
               "dist2 / goals / cost / ignored misaligned");
    GG_REQUIRE_WS(ws, ws_bytes, gg_field_route_workspace(dims));
    hipStream_t s = (hipStream_t)stream;
    const int64_t cells = field_cells(dims);
    const int64_t words = (int64_t)route_ws_words(dims);
    int b[3];
    route_bricks(dims, b);
    const int64_t bricks = (int64_t)b[0] * b[1] * b[2];
    const FieldFree v = field_free(dims, dist2, need);
    unsigned *counters = (unsigned *)ws, *flags = counters + FR_BATCH;
    *rounds_out = 0;
    const int64_t span = cells > words ? cells : words;
    hipLaunchKernelGGL(route_init_kernel, dim3((unsigned)((span + FR_THREADS - 1) / FR_THREADS)), dim3(FR_THREADS), 0,
                       s, (long long)cells, cost, (long long)words, counters,
                       reinterpret_cast<unsigned long long *>(ignored));
    if (num_goals == 0) {
        GG_CHECK_LAUNCH();
        return GG_OK;
    }
    hipLaunchKernelGGL(route_goals_kernel, dim3((unsigned)((num_goals + FR_THREADS - 1) / FR_THREADS)),
                       dim3(FR_THREADS), 0, s, v, b[0], b[1], b[2], num_goals, goals, cost, flags,
                       reinterpret_cast<unsigned long long *>(ignored));
    GG_CHECK_LAUNCH();
    // Rounds in batches; after each batch the counters come back.  Once a round has flagged nothing the rounds
    // behind it find no active brick.  The loop is bounded by max_rounds, and no kernel in it can wait.
    unsigned flagged[FR_BATCH];
    for (int done = 0; done < max_rounds;) {
        const int n = max_rounds - done < FR_BATCH ? max_rounds - done : FR_BATCH;
        if (done > 0) hipLaunchKernelGGL(route_zero_kernel, dim3(1), dim3(FR_THREADS), 0, s, counters, FR_BATCH);
        for (int r = 0; r < n; ++r) {
            unsigned *cur = flags + (size_t)((done + r) & 1) * bricks, *next = flags + (size_t)((done + r + 1) & 1) * bricks;
            hipLaunchKernelGGL(route_round_kernel, dim3((unsigned)bricks), dim3(FR_THREADS), 0, s, v, b[0], b[1],
                               b[2], cost, cur, next, counters + r);
        }
        GG_CHECK_LAUNCH();
        hipError_t e = hipMemcpyAsync(flagged, counters, sizeof(unsigned) * n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            gg_set_error("%s: reading the round counters back failed: %s", __func__, hipGetErrorString(e));
            return GG_ERR_LAUNCH;
        }
        for (int r = 0; r < n; ++r)
            if (flagged[r] == 0u) {
                *rounds_out = done + r + 1;
                return GG_OK;
            }
        done += n;
    }
    *rounds_out = max_rounds;
    gg_set_error("%s: no convergence within max_rounds = %d rounds; cost holds upper bounds", __func__, max_rounds);
    return GG_ERR_NOT_CONVERGED;
}

extern "C" int gg_field_descend(const int32_t *dims, const int32_t *dist2, int32_t need, const int32_t *cost,
                                int num_paths, const int32_t *starts, int max_cells, int32_t *cells, int32_t *length,
                                gg_stream_t stream) {
    GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
    GG_REQUIRE_FIELD_NEED(need);
    GG_REQUIRE_FIELD_PATHS(num_paths, max_cells);
    if (num_paths == 0) return GG_OK;
    GG_REQUIRE(dist2 && cost && starts && cells && length, "null pointer: dist2 / cost / starts / cells / length");
    GG_REQUIRE((((uintptr_t)dist2 | (uintptr_t)cost | (uintptr_t)starts | (uintptr_t)cells | (uintptr_t)length) & 3) == 0,
               "dist2 / cost / starts / cells / length misaligned");
    const int per = FR_THREADS / 64;
    hipLaunchKernelGGL(route_descend_kernel, dim3((unsigned)((num_paths + per - 1) / per)), dim3(FR_THREADS), 0,
                       (hipStream_t)stream, field_free(dims, dist2, need), cost, num_paths, starts, max_cells, cells,
                       length);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_field_sight(const int32_t *dims, const int32_t *dist2, int32_t need, int num_segments,
                              const int32_t *a, const int32_t *b, int32_t *cover, int32_t *blocked,
                              gg_stream_t stream) {
    GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
    GG_REQUIRE_FIELD_NEED(need);
    GG_REQUIRE(num_segments >= 0 && num_segments <= GG_FIELD_MAX_POSES,
               "need 0 <= num_segments <= GG_FIELD_MAX_POSES");
    if (num_segments == 0) return GG_OK;
    GG_REQUIRE(dist2 && a && b && cover && blocked, "null pointer: dist2 / a / b / cover / blocked");
    GG_REQUIRE((((uintptr_t)dist2 | (uintptr_t)a | (uintptr_t)b | (uintptr_t)cover | (uintptr_t)blocked) & 3) == 0,
               "dist2 / a / b / cover / blocked misaligned");
    hipLaunchKernelGGL(route_sight_kernel, dim3((unsigned)((num_segments + FR_THREADS - 1) / FR_THREADS)),
                       dim3(FR_THREADS), 0, (hipStream_t)stream, field_free(dims, dist2, need), num_segments, a, b,
                       cover, blocked);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_field_shortcut(const int32_t *dims, const int32_t *dist2, int32_t need, int num_paths,
                                 int max_cells, const int32_t *cells, const int32_t *length, int window,
                                 int32_t *keep, int32_t *count, int32_t *blocked, gg_stream_t stream) {
    GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
    GG_REQUIRE_FIELD_NEED(need);
    GG_REQUIRE_FIELD_PATHS(num_paths, max_cells);
    GG_REQUIRE(window >= 1, "window must be >= 1");
    if (num_paths == 0) return GG_OK;
    GG_REQUIRE(dist2 && cells && length && keep && count && blocked,
               "null pointer: dist2 / cells / length / keep / count / blocked");
    GG_REQUIRE((((uintptr_t)dist2 | (uintptr_t)cells | (uintptr_t)length | (uintptr_t)keep | (uintptr_t)count |
                 (uintptr_t)blocked) & 3) == 0,
               "dist2 / cells / length / keep / count / blocked misaligned");
    hipLaunchKernelGGL(route_shortcut_kernel, dim3((unsigned)num_paths), dim3(FR_THREADS), 0,
                       (hipStream_t)stream, field_free(dims, dist2, need), num_paths, max_cells, cells, length, window,
                       keep, count, blocked);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
