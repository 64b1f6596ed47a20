// knn.hip — exact k nearest neighbours of every point among the others (the k_nearest_sklearn of the reference's
// gaussian_splatting.py:315-331, whose distances set the first log-scales).  The contract is in
// include/gg_raster.h (gg_knn) and PARITY.md "Scene preparation"; the design in DESIGN.md §3.13.
//
// Uniform grid, counting sort (grid_sort.h: the grid, the sort and the call path shared with csrc/cluster.hip and
// csrc/register.hip).  Points outside the caller's grid sit in its border cells.  One lane per sorted slot then
// searches Chebyshev shells of cells around its own cell, r = 0, 1, ...
// and stops after shell r when its k-th squared distance is <= b^2, b a lower bound of the distance to every cell
// outside the searched cube:
//   b = min over the faces of the cube that have cells beyond them of the distance from p to that face plane,
//       less a rounding margin (KN_SLOP relative to the coordinates' magnitude).
// A point in a cell beyond a face lies beyond that face's plane — clamping moves a cell index toward the inside,
// never across p's own cell — so b is a bound for any grid and any point; the grid only sets the speed.  Once the
// cube covers the grid, everything has been seen.  A k-th distance of 0 ends the search at once (inside a cell), so
// a pile of identical points costs O(k) per point, not a walk of the pile.
// Exact: squared distances are fp64 ((dx*dx + dy*dy) + dz*dz, dx the fp64 difference of the fp32 coordinates),
// the kept set is the k smallest (distance, index) pairs, and the sqrt is rounded to fp32 at the end.
// Cost: every lane reads every point of every cell it visits, so the total is O(N x max cell occupancy) plus the
// cells walked.  A point whose neighbours are far in cell units walks every cell of the grid once and reads every
// point once; a grid that does not fit the cloud's density (a cloud of a few dense clusters far apart along every
// axis) crowds each cluster into a few cells, O(N^2) at worst.  DESIGN.md §3.13 measures far outliers and piles.
#include <limits.h>
#include <math.h>

#include "gg_common.h"
#include "grid_sort.h"

#define KN_SLOP 1e-12

template <int K>
__device__ __forceinline__ void kn_visit(int c, const int32_t *__restrict__ start, const int32_t *__restrict__ counts,
                                         const float4 *__restrict__ sorted, int self, double px, double py, double pz,
                                         double (&bs)[K], int (&bi)[K]) {
    const int a = start[c], e = a + counts[c];
    for (int j = a; j < e && bs[K - 1] != 0.0; ++j) {       // k at distance 0: nothing can come closer
        const float4 o = sorted[j];
        const int id = __float_as_int(o.w);
        const double dx = (double)o.x - px, dy = (double)o.y - py, dz = (double)o.z - pz;
        const double s = (dx * dx + dy * dy) + dz * dz;
        if (id == self || !(s < bs[K - 1] || (s == bs[K - 1] && id < bi[K - 1]))) continue;
        double cs = s;
        int ci = id;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const bool lt = cs < bs[t] || (cs == bs[t] && ci < bi[t]);
            const double ts = bs[t];
            const int ti = bi[t];
            bs[t] = lt ? cs : ts;
            bi[t] = lt ? ci : ti;
            cs = lt ? ts : cs;
            ci = lt ? ti : ci;
        }
    }
}

template <int K>
__global__ __launch_bounds__(256) void knn_search_kernel(int n, KnGrid G, const int32_t *__restrict__ start,
                                                         const int32_t *__restrict__ counts,
                                                         const float4 *__restrict__ sorted, float *__restrict__ dist,
                                                         int64_t *__restrict__ idx) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= n) return;
    const float4 q = sorted[slot];
    const int self = __float_as_int(q.w);
    const double p[3] = {(double)q.x, (double)q.y, (double)q.z};
    int c[3];
    kn_cell(G, q.x, q.y, q.z, c[0], c[1], c[2]);
    const int X = G.dims[0], Y = G.dims[1], Z = G.dims[2];
    double slop = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d)
        slop = fmax(slop, KN_SLOP * ((fabs(G.lo[d]) + (double)G.dims[d] * G.cell) + fabs(p[d])));
    double bs[K];
    int bi[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        bs[t] = INFINITY;
        bi[t] = INT_MAX;
    }
    for (int r = 0;; ++r) {
        const int x0 = max(0, c[0] - r), x1 = min(X - 1, c[0] + r);
        const int y0 = max(0, c[1] - r), y1 = min(Y - 1, c[1] + r);
        const int z0 = max(0, c[2] - r), z1 = min(Z - 1, c[2] + r);
        for (int z = z0; z <= z1; ++z) {
            const bool zf = abs(z - c[2]) == r;
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * Y + y) * X;
                if (zf || abs(y - c[1]) == r) {
                    for (int x = x0; x <= x1; ++x) kn_visit<K>(row + x, start, counts, sorted, self, p[0], p[1], p[2], bs, bi);
                } else {
                    if (c[0] - r >= 0) kn_visit<K>(row + c[0] - r, start, counts, sorted, self, p[0], p[1], p[2], bs, bi);
                    if (r > 0 && c[0] + r < X) kn_visit<K>(row + c[0] + r, start, counts, sorted, self, p[0], p[1], p[2], bs, bi);
                }
            }
        }
        if (bs[K - 1] == 0.0) break;
        double b = INFINITY;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (c[d] - r > 0) b = fmin(b, p[d] - (G.lo[d] + (double)(c[d] - r) * G.cell));
            if (c[d] + r < G.dims[d] - 1) b = fmin(b, (G.lo[d] + (double)(c[d] + r + 1) * G.cell) - p[d]);
        }
        if (b == INFINITY) break;                // the cube covers the grid
        b -= slop;
        if (b > 0.0 && bs[K - 1] <= b * b) break;
    }
    const size_t o = (size_t)self * K;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        dist[o + t] = (float)sqrt(bs[t]);
        idx[o + t] = bi[t];
    }
}

extern "C" size_t gg_knn_workspace(int num_points, const int32_t *dims) {
    if (num_points < 0 || num_points > GG_KNN_MAX_POINTS || !kn_dims_ok(dims)) return 0;
    return kn_layout(num_points, dims, nullptr, nullptr);
}

extern "C" int gg_knn(int num_points, const float *points, int k, const double *grid, const int32_t *dims,
                      float *dist, int64_t *idx, void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(k >= 1 && k <= GG_KNN_MAX_K, "need 1 <= k <= GG_KNN_MAX_K");
    GG_REQUIRE(num_points > k && num_points <= GG_KNN_MAX_POINTS, "need k < num_points <= GG_KNN_MAX_POINTS");
    GG_REQUIRE_GRID(grid, dims);
    GG_REQUIRE(points && dist && idx, "null pointer");
    GG_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)dist & 3) == 0 && ((uintptr_t)idx & 7) == 0,
               "points / dist / idx misaligned");
    const size_t need = kn_layout(num_points, dims, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    KnWs w;
    kn_layout(num_points, dims, &w, (char *)ws);
    const KnGrid G = kn_grid(grid, dims);
    const unsigned pb = (unsigned)((num_points + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    gg_prof_begin(GG_K_KNN, s);
    GG_REQUIRE_FILL(GG_K_KNN, s, kn_sort<false>(num_points, points, nullptr, G, w, nullptr, s));
    switch (k) {
#define KN_CASE(KK)                                                                                                  \
    case KK:                                                                                                         \
        hipLaunchKernelGGL(knn_search_kernel<KK>, dim3(pb), dim3(256), 0, s, num_points, G, w.start, w.counts,       \
                           w.sorted, dist, idx);                                                                     \
        break;
        KN_CASE(1)
        KN_CASE(2)
        KN_CASE(3)
        KN_CASE(4)
        KN_CASE(5)
        KN_CASE(6)
        KN_CASE(7)
        KN_CASE(8)
#undef KN_CASE
    }
    gg_prof_end(GG_K_KNN, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
