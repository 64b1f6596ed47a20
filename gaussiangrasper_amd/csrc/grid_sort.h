// grid_sort.h — the uniform-grid counting sort and its call path, shared by csrc/knn.hip, csrc/cluster.hip and
// csrc/register.hip.
//
// The caller gives the grid (lower corner, cell edge, cells per axis); a point's cell is floor((p - lo) / cell) per
// axis, clamped into the grid, so points outside the grid sit in its border cells.  Counts per cell (integer
// atomics), exclusive offsets (prep_common.h scans), a scatter of (x, y, z, index) into cell order.  With FILTER the
// sort takes only the points that are finite and, when a byte mask is given, have a non-zero byte; *total (device,
// int64) then holds how many were taken.  Slot order within a cell follows the atomics.
// kn_ball walks the sorted points within a radius of a query point (csrc/cluster.hip, csrc/register.hip): with a
// cell edge of kn_radius_cell the 27 cells around the query's cell hold them all.
// A call checks its grid with GG_REQUIRE_GRID, fills a KnGrid with kn_grid, lays its workspace out with kn_layout and
// sorts with kn_sort under GG_REQUIRE_FILL.
#pragma once
#include <math.h>

#include "gg_common.h"
#include "prep_common.h"

struct KnGrid {
    double lo[3], cell;
    int dims[3];
};

__device__ __forceinline__ int kn_axis(double p, double lo, double cell, int dim) {
    const double t = floor((p - lo) / cell);
    return !(t >= 0.0) ? 0 : (t >= (double)(dim - 1) ? dim - 1 : (int)t);
}

__device__ __forceinline__ int kn_cell(const KnGrid &G, float x, float y, float z, int &cx, int &cy, int &cz) {
    cx = kn_axis((double)x, G.lo[0], G.cell, G.dims[0]);
    cy = kn_axis((double)y, G.lo[1], G.cell, G.dims[1]);
    cz = kn_axis((double)z, G.lo[2], G.cell, G.dims[2]);
    return (cz * G.dims[1] + cy) * G.dims[0] + cx;
}

// The cell edge of a sort that is searched within `radius`: max(cell, radius) (1 + 2^-20), so that the cells of two
// points within the radius differ by at most 1 per axis.  2^-20 of slack covers the rounding of (p - lo) / cell:
// |quotient| < 2^27 inside the grid, two roundings of 2^-53 relative each, against a real difference of at most
// 1 / (1 + 2^-20) between neighbours.  Clamping into the grid is monotone and 1-Lipschitz in the cell index, so it
// holds for points outside the grid too.
static inline double kn_radius_cell(double cell, double radius) { return fmax(cell, radius) * (1.0 + 0x1p-20); }

// The caller's grid (lower corner and cell edge) and dims, before anything reads them.
#define GG_REQUIRE_GRID(grid, dims)                                                                            \
    do {                                                                                                       \
        GG_REQUIRE((grid) && isfinite((grid)[0]) && isfinite((grid)[1]) && isfinite((grid)[2]) &&              \
                       isfinite((grid)[3]) && (grid)[3] > 0.0,                                                 \
                   "grid: lower corner finite, cell edge finite and > 0");                                     \
        GG_REQUIRE(kn_dims_ok(dims), "dims: each >= 1, product <= GG_KNN_MAX_CELLS");                          \
    } while (0)

// The grid as given (gg_knn: any cell edge is exact there), and the grid of a sort that is searched within `radius`.
static inline KnGrid kn_grid(const double *grid, const int32_t *dims) {
    KnGrid G;
    for (int d = 0; d < 3; ++d) {
        G.lo[d] = grid[d];
        G.dims[d] = dims[d];
    }
    G.cell = grid[3];
    return G;
}
static inline KnGrid kn_grid(const double *grid, const int32_t *dims, double radius) {
    KnGrid G = kn_grid(grid, dims);
    G.cell = kn_radius_cell(grid[3], radius);
    return G;
}

// f(slot j, sorted[j], squared distance) for every sorted point o with (dx dx + dy dy) + dz dz <= r2 in fp64, dx the
// fp64 difference o - q; q = (px, py, pz), fp64, need not be a sorted point.  The grid's cell edge
// must be kn_radius_cell(., sqrt(r2)).  A row of 3 cells along x is contiguous in slot order: 9 slot ranges.
template <class F>
__device__ __forceinline__ void kn_ball(const KnGrid &G, const int32_t *__restrict__ start,
                                        const int32_t *__restrict__ counts, const float4 *__restrict__ sorted, double px,
                                        double py, double pz, double r2, F f) {
    const int X = G.dims[0], Y = G.dims[1], Z = G.dims[2];
    const int cx = kn_axis(px, G.lo[0], G.cell, X), cy = kn_axis(py, G.lo[1], G.cell, Y);
    const int cz = kn_axis(pz, G.lo[2], G.cell, Z);
    const int x0 = max(0, cx - 1), x1 = min(X - 1, cx + 1);
    for (int zz = max(0, cz - 1); zz <= min(Z - 1, cz + 1); ++zz)
        for (int yy = max(0, cy - 1); yy <= min(Y - 1, cy + 1); ++yy) {
            const int row = (zz * Y + yy) * X;
            const int a = start[row + x0], e = start[row + x1] + counts[row + x1];
            for (int j = a; j < e; ++j) {
                const float4 o = sorted[j];
                const double dx = (double)o.x - px, dy = (double)o.y - py, dz = (double)o.z - pz;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 <= r2) f(j, o, d2);
            }
        }
}

template <bool FILTER>
__device__ __forceinline__ bool kn_takes(float x, float y, float z, const uint8_t *__restrict__ active, int i) {
    if (!FILTER) return true;
    // x - x is 0 for a finite x and NaN for NaN and +-inf
    return (active == nullptr || active[i] != 0) && (x - x) + (y - y) + (z - z) == 0.0f;
}

template <bool FILTER>
static __global__ __launch_bounds__(256) void knn_count_kernel(int n, const float *__restrict__ points,
                                                               const uint8_t *__restrict__ active, KnGrid G,
                                                               int32_t *__restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
    if (!kn_takes<FILTER>(x, y, z, active, i)) return;
    int cx, cy, cz;
    atomicAdd(&counts[kn_cell(G, x, y, z, cx, cy, cz)], 1);
}

// Slot order within a cell follows the atomics.  For gg_knn distances never depend on it, and neither do indices
// except among exact duplicates: the search stops at the first k points at distance 0 it meets, so which of several
// points at distance 0 is returned may differ from call to call.  Nothing gg_cluster_dbscan writes depends on it.
template <bool FILTER>
static __global__ __launch_bounds__(256) void knn_scatter_kernel(int n, const float *__restrict__ points,
                                                                 const uint8_t *__restrict__ active, KnGrid G,
                                                                 const int32_t *__restrict__ start,
                                                                 int32_t *__restrict__ cursor,
                                                                 float4 *__restrict__ sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
    if (!kn_takes<FILTER>(x, y, z, active, i)) return;
    int cx, cy, cz;
    const int c = kn_cell(G, x, y, z, cx, cy, cz);
    sorted[start[c] + atomicAdd(&cursor[c], 1)] = make_float4(x, y, z, __int_as_float(i));
}

struct KnWs {
    int32_t *counts, *cursor, *start, *tile_sums, *tile_offs;
    float4 *sorted;
};

static inline bool kn_dims_ok(const int32_t *dims) {
    if (!dims) return false;
    int64_t cells = 1;
    for (int d = 0; d < 3; ++d) {
        if (dims[d] < 1 || dims[d] > GG_KNN_MAX_CELLS) return false;
        cells *= dims[d];
        if (cells > GG_KNN_MAX_CELLS) return false;
    }
    return true;
}

// The sort's arrays behind `base` (nullptr: sizes only), every one 256-byte aligned; returns the bytes taken.
static inline size_t kn_layout(int n, const int32_t *dims, KnWs *w, char *base) {
    const int64_t cells = (int64_t)dims[0] * dims[1] * dims[2];
    const int64_t tiles = (cells + PP_TILE - 1) / PP_TILE;
    GgCarve cv{base, 0};
    KnWs t;
    t.counts = (int32_t *)cv.take((size_t)cells * 4);
    t.cursor = (int32_t *)cv.take((size_t)cells * 4);
    t.start = (int32_t *)cv.take((size_t)cells * 4);
    t.tile_sums = (int32_t *)cv.take((size_t)tiles * 4);
    t.tile_offs = (int32_t *)cv.take((size_t)tiles * 4);
    t.sorted = (float4 *)cv.take((size_t)n * 16);
    if (w) *w = t;
    return cv.off;
}

// counts, start and sorted of the points (FILTER: of those that take part) on stream s; hipSuccess unless a fill
// could not be launched (the caller's GG_REQUIRE_FILL).  Launch errors of the kernels are left for the caller's
// GG_CHECK_LAUNCH.
template <bool FILTER>
static inline hipError_t kn_sort(int n, const float *points, const uint8_t *active, const KnGrid &G, const KnWs &w,
                                 int64_t *total, hipStream_t s) {
    const int cells = G.dims[0] * G.dims[1] * G.dims[2];
    const unsigned pb = (unsigned)((n + 255) / 256);
    hipError_t e = gg_fill_async(w.counts, 0, (size_t)cells * 4, s);
    if (e == hipSuccess) e = gg_fill_async(w.cursor, 0, (size_t)cells * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(knn_count_kernel<FILTER>, dim3(pb), dim3(256), 0, s, n, points, active, G, w.counts);
    pp_scan_long(w.counts, cells, w.tile_sums, w.tile_offs, w.start, total, s);
    hipLaunchKernelGGL(knn_scatter_kernel<FILTER>, dim3(pb), dim3(256), 0, s, n, points, active, G, w.start, w.cursor,
                       w.sorted);
    return hipSuccess;
}
