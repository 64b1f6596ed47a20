// cluster.hip — DBSCAN of a point set and per-cluster statistics: object instances among the Gaussians a query
// selects.  The contract is in include/gg_raster.h (gg_cluster_dbscan, gg_cluster_stats) and PARITY.md "Object
// instances"; the design, the termination argument and the cost model in DESIGN.md §3.18.
//
// gg_cluster_dbscan, all on the caller's stream:
//   init     labels -1, core 0, neighbor_count 0, parent[i] = i, root flags 0 for every point
//   sort     grid_sort.h with FILTER: the active finite points in cell order, M of them (device int64)
//   core     one lane per sorted slot: the exact neighbour count over the 27 cells around its own
//   union    one lane per core slot: unite(i, j) for every core neighbour j < i  (lock-free union-find, below)
//   roots    core: labels[i] = find(i), flag the roots;  border: labels[i] = min find(j) over core neighbours j
//   relabel  ordered scan of the root flags (prep_common.h) -> dense ids in ascending root order; num_clusters
// The grid's cell edge is max(cell, eps) (1 + 2^-20), so the cells of two neighbours differ by at most 1 per axis
// (kn_radius_cell, grid_sort.h): clamping into the grid is monotone and 1-Lipschitz in the cell index, so that holds
// for points outside the grid too.  The 27 cells are a superset of every point's neighbours; the exact fp64 test decides.
// A row of 3 cells along x is contiguous in slot order, so a lane walks 9 slot ranges.
//
// Union-find.  parent[] is indexed by point.  Invariant: parent[v] <= v, with equality exactly for roots.  Two
// kinds of writes, both 32-bit device-scope atomics that can only lower a word: the hook atomicCAS(&parent[hi], hi,
// lo) with lo < hi, which succeeds only while hi is a root, and the compression atomicMin(&parent[x], g) with g an
// ancestor of x.  A tree's root is therefore its smallest member, and when all core-core pairs are united the root
// of a component is its smallest core index whatever the schedule.  No lane ever waits for another: cl_find walks
// strictly decreasing indices, and every pass of cl_unite's loop strictly lowers a + b (a failed hook returns the
// word's new, smaller value), so both end after at most (their start values) steps on their own.
//
// Cost: (active points) x (points within the 27 cells) x 3 passes.  An eps so large that the cloud falls into a few
// cells is quadratic; the caller must avoid it.
#include <limits.h>
#include <math.h>

#include "gg_common.h"
#include "grid_sort.h"
#include "ordered_sum.h"

__device__ __forceinline__ int cl_load(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree at some moment of the call, halving the path on the way.  x decreases every step.
__device__ __forceinline__ int cl_find(int32_t *parent, int x) {
    int p = cl_load(&parent[x]);
    while (p != x) {
        const int g = cl_load(&parent[p]);
        if (g != p) atomicMin(&parent[x], g);
        x = p;
        p = g;
    }
    return x;
}

// a + b decreases every pass: the finds do not raise them, and after a failed hook hi gives way to old < hi.
__device__ __forceinline__ void cl_unite(int32_t *parent, int a, int b) {
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

// f(slot j, index of j) for every sorted point within eps of q, q itself included
template <class F>
__device__ __forceinline__ void cl_neighbours(const KnGrid &G, const int32_t *__restrict__ start,
                                              const int32_t *__restrict__ counts, const float4 *__restrict__ sorted,
                                              const float4 q, double eps2, F f) {
    kn_ball(G, start, counts, sorted, (double)q.x, (double)q.y, (double)q.z, eps2,
            [&](int j, const float4 &o, double) { f(j, __float_as_int(o.w)); });
}

__global__ __launch_bounds__(256) void cl_init_kernel(int n, int32_t *__restrict__ labels, uint8_t *__restrict__ core,
                                                      int32_t *__restrict__ ncount, int32_t *__restrict__ parent,
                                                      int32_t *__restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    labels[i] = -1;
    core[i] = 0;
    ncount[i] = 0;
    parent[i] = i;
    flags[i] = 0;
}

__global__ __launch_bounds__(256) void cl_core_kernel(int n, const int64_t *__restrict__ total, KnGrid G,
                                                      const int32_t *__restrict__ start,
                                                      const int32_t *__restrict__ counts,
                                                      const float4 *__restrict__ sorted, double eps2, int min_points,
                                                      int32_t *__restrict__ ncount, uint8_t *__restrict__ core,
                                                      uint8_t *__restrict__ core_s) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= n || slot >= *total) return;
    const float4 q = sorted[slot];
    int c = 0;
    cl_neighbours(G, start, counts, sorted, q, eps2, [&](int, int) { ++c; });
    const int id = __float_as_int(q.w);
    const uint8_t is_core = c >= min_points ? 1 : 0;
    ncount[id] = c;
    core[id] = is_core;
    core_s[slot] = is_core;
}

__global__ __launch_bounds__(256) void cl_union_kernel(int n, const int64_t *__restrict__ total, KnGrid G,
                                                       const int32_t *__restrict__ start,
                                                       const int32_t *__restrict__ counts,
                                                       const float4 *__restrict__ sorted, double eps2,
                                                       const uint8_t *__restrict__ core_s, int32_t *parent) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= n || slot >= *total || !core_s[slot]) return;
    const float4 q = sorted[slot];
    const int id = __float_as_int(q.w);
    cl_neighbours(G, start, counts, sorted, q, eps2, [&](int j, int jd) {
        if (jd < id && core_s[j]) cl_unite(parent, id, jd);
    });
}

// After the union kernel no hook happens any more: roots are final and cl_find returns them.  labels[] holds root
// indices (or -1) until the relabel kernel.
__global__ __launch_bounds__(256) void cl_root_kernel(int n, const int64_t *__restrict__ total, KnGrid G,
                                                      const int32_t *__restrict__ start,
                                                      const int32_t *__restrict__ counts,
                                                      const float4 *__restrict__ sorted, double eps2,
                                                      const uint8_t *__restrict__ core_s, int32_t *parent,
                                                      int32_t *__restrict__ labels, int32_t *__restrict__ flags) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= n || slot >= *total) return;
    const float4 q = sorted[slot];
    const int id = __float_as_int(q.w);
    if (core_s[slot]) {
        const int r = cl_find(parent, id);
        labels[id] = r;
        if (r == id) flags[id] = 1;
        return;
    }
    int best = INT_MAX;
    cl_neighbours(G, start, counts, sorted, q, eps2, [&](int j, int jd) {
        if (core_s[j]) best = min(best, cl_find(parent, jd));
    });
    labels[id] = best == INT_MAX ? -1 : best;
}

__global__ __launch_bounds__(256) void cl_relabel_kernel(int n, const int32_t *__restrict__ rank,
                                                         const int64_t *__restrict__ num_roots,
                                                         int32_t *__restrict__ labels,
                                                         int32_t *__restrict__ num_clusters) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *num_clusters = (int32_t)*num_roots;
    if (i >= n) return;
    const int r = labels[i];
    if (r >= 0) labels[i] = rank[r];
}

struct ClWs {
    KnWs sort;
    int64_t *totals;                   // [0] active points, [1] roots
    int32_t *parent, *flags, *rank, *tile_sums, *tile_offs;
    uint8_t *core_s;
};

static size_t cl_layout(int n, const int32_t *dims, ClWs *w, char *base) {
    const size_t tiles = ((size_t)n + PP_TILE - 1) / PP_TILE;
    GgCarve cv{base, kn_layout(n, dims, w ? &w->sort : nullptr, base)};
    ClWs t;
    t.totals = (int64_t *)cv.take(16);
    t.parent = (int32_t *)cv.take((size_t)n * 4);
    t.flags = (int32_t *)cv.take((size_t)n * 4);
    t.rank = (int32_t *)cv.take((size_t)n * 4);
    t.tile_sums = (int32_t *)cv.take(tiles * 4);
    t.tile_offs = (int32_t *)cv.take(tiles * 4);
    t.core_s = (uint8_t *)cv.take((size_t)n);
    if (w) {
        t.sort = w->sort;
        *w = t;
    }
    return cv.off;
}

extern "C" size_t gg_cluster_workspace(int num_points, const int32_t *dims) {
    if (num_points < 0 || num_points > GG_CLUSTER_MAX_POINTS || !kn_dims_ok(dims)) return 0;
    return cl_layout(num_points, dims, nullptr, nullptr);
}

extern "C" int gg_cluster_dbscan(int num_points, const float *points, const uint8_t *active, double eps,
                                 int min_points, const double *grid, const int32_t *dims, int32_t *labels,
                                 uint8_t *core, int32_t *neighbor_count, int32_t *num_clusters, void *ws,
                                 size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0 && num_points <= GG_CLUSTER_MAX_POINTS, "need 0 <= num_points <= GG_CLUSTER_MAX_POINTS");
    GG_REQUIRE(isfinite(eps) && eps > 0.0, "eps must be finite and > 0");
    GG_REQUIRE(min_points >= 1, "min_points must be >= 1");
    GG_REQUIRE_GRID(grid, dims);
    if (num_points == 0) return GG_OK;
    GG_REQUIRE(points && labels && core && neighbor_count && num_clusters, "null pointer");
    GG_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)neighbor_count & 3) == 0 &&
                   ((uintptr_t)num_clusters & 3) == 0,
               "points / labels / neighbor_count / num_clusters misaligned");
    const size_t need = cl_layout(num_points, dims, nullptr, nullptr);
    GG_REQUIRE(ws && ((uintptr_t)ws & 255) == 0, "ws must be non-null and 256-byte aligned");
    if (ws_bytes < need) {
        gg_set_error("%s: workspace too small: %zu < %zu bytes", __func__, ws_bytes, need);
        return GG_ERR_INVALID_ARG;
    }
    ClWs w;
    cl_layout(num_points, dims, &w, (char *)ws);
    const KnGrid G = kn_grid(grid, dims, eps);
    GG_REQUIRE(isfinite(G.cell), "eps too large for the grid");
    const double eps2 = eps * eps;
    const int n = num_points;
    const unsigned pb = (unsigned)((n + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    gg_prof_begin(GG_K_CLUSTER, s);
    hipLaunchKernelGGL(cl_init_kernel, dim3(pb), dim3(256), 0, s, n, labels, core, neighbor_count, w.parent, w.flags);
    GG_REQUIRE_FILL(GG_K_CLUSTER, s, kn_sort<true>(n, points, active, G, w.sort, w.totals, s));
    hipLaunchKernelGGL(cl_core_kernel, dim3(pb), dim3(256), 0, s, n, w.totals, G, w.sort.start, w.sort.counts,
                       w.sort.sorted, eps2, min_points, neighbor_count, core, w.core_s);
    hipLaunchKernelGGL(cl_union_kernel, dim3(pb), dim3(256), 0, s, n, w.totals, G, w.sort.start, w.sort.counts,
                       w.sort.sorted, eps2, w.core_s, w.parent);
    hipLaunchKernelGGL(cl_root_kernel, dim3(pb), dim3(256), 0, s, n, w.totals, G, w.sort.start, w.sort.counts,
                       w.sort.sorted, eps2, w.core_s, w.parent, labels, w.flags);
    pp_scan_long(w.flags, n, w.tile_sums, w.tile_offs, w.rank, w.totals + 1, s);
    hipLaunchKernelGGL(cl_relabel_kernel, dim3(pb), dim3(256), 0, s, n, w.rank, w.totals + 1, labels, num_clusters);
    gg_prof_end(GG_K_CLUSTER, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------
// per-cluster statistics
// ------------------------------------------------------------------------------------------------
// fp32 -> uint32 with the same order (-0 below +0); NaN never gets here (members are finite points)
__device__ __forceinline__ uint32_t cl_encode(float f) {
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float cl_decode(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? u ^ 0x80000000u : ~u);
}

__global__ __launch_bounds__(256) void cl_stats_init_kernel(int k, unsigned long long *__restrict__ count,
                                                            double *__restrict__ weight, double *__restrict__ sums,
                                                            uint32_t *__restrict__ box) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    count[c] = 0;
    weight[c] = 0.0;
    for (int a = 0; a < 3; ++a) {
        sums[3 * (size_t)c + a] = 0.0;
        box[6 * (size_t)c + a] = 0xffffffffu;
        box[6 * (size_t)c + 3 + a] = 0u;
    }
}

// One lane per point.  A wave takes its labels one at a time (at most 64 rounds: every round retires the lanes of
// one label), sums that label's lanes with a butterfly and lets one lane add the result, so the atomics per wave
// are one set per distinct label, not one per point.
__global__ __launch_bounds__(256) void cl_stats_kernel(int n, int k, const float *__restrict__ points,
                                                       const float *__restrict__ weights,
                                                       const int32_t *__restrict__ labels,
                                                       unsigned long long *__restrict__ count,
                                                       double *__restrict__ weight, double *__restrict__ sums,
                                                       uint32_t *__restrict__ box) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & (GG_WAVE - 1);
    int lab = i < n ? labels[i] : -1;
    if (lab >= k) lab = -1;
    float x = 0.f, y = 0.f, z = 0.f;
    double w = 0.0;
    if (lab >= 0) {
        x = points[3 * (size_t)i];
        y = points[3 * (size_t)i + 1];
        z = points[3 * (size_t)i + 2];
        w = (double)weights[i];
    }
    unsigned long long todo = __ballot(lab >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int L = __shfl(lab, leader, GG_WAVE);
        const bool mine = lab == L;
        const unsigned long long m = __ballot(mine);
        const double sw = gg_wave_sum(mine ? w : 0.0);
        const double sx = gg_wave_sum(mine ? w * (double)x : 0.0);
        const double sy = gg_wave_sum(mine ? w * (double)y : 0.0);
        const double sz = gg_wave_sum(mine ? w * (double)z : 0.0);
        const uint32_t lx = gg_wave_min(mine ? cl_encode(x) : 0xffffffffu), hx = gg_wave_max(mine ? cl_encode(x) : 0u);
        const uint32_t ly = gg_wave_min(mine ? cl_encode(y) : 0xffffffffu), hy = gg_wave_max(mine ? cl_encode(y) : 0u);
        const uint32_t lz = gg_wave_min(mine ? cl_encode(z) : 0xffffffffu), hz = gg_wave_max(mine ? cl_encode(z) : 0u);
        if (lane == leader) {
            atomicAdd(&count[L], (unsigned long long)__popcll(m));
            atomicAdd(&weight[L], sw);
            atomicAdd(&sums[3 * (size_t)L], sx);
            atomicAdd(&sums[3 * (size_t)L + 1], sy);
            atomicAdd(&sums[3 * (size_t)L + 2], sz);
            uint32_t *b = box + 6 * (size_t)L;
            atomicMin(&b[0], lx);
            atomicMin(&b[1], ly);
            atomicMin(&b[2], lz);
            atomicMax(&b[3], hx);
            atomicMax(&b[4], hy);
            atomicMax(&b[5], hz);
        }
        todo &= ~m;
    }
}

__global__ __launch_bounds__(256) void cl_stats_finish_kernel(int k, const double *__restrict__ weight,
                                                              double *__restrict__ sums, uint32_t *__restrict__ box) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    const double w = weight[c];
    for (int a = 0; a < 3; ++a) sums[3 * (size_t)c + a] = sums[3 * (size_t)c + a] / w;
    for (int a = 0; a < 6; ++a) box[6 * (size_t)c + a] = __float_as_uint(cl_decode(box[6 * (size_t)c + a]));
}

extern "C" int gg_cluster_stats(int num_points, const float *points, const float *weights, const int32_t *labels,
                                int num_clusters, int64_t *count, double *weight, double *centroid, float *bbox,
                                gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0 && num_points <= GG_CLUSTER_MAX_POINTS, "need 0 <= num_points <= GG_CLUSTER_MAX_POINTS");
    GG_REQUIRE(num_clusters >= 0 && num_clusters <= num_points, "need 0 <= num_clusters <= num_points");
    if (num_clusters == 0) return GG_OK;
    GG_REQUIRE(points && weights && labels && count && weight && centroid && bbox, "null pointer");
    GG_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)weights & 3) == 0 && ((uintptr_t)labels & 3) == 0 &&
                   ((uintptr_t)count & 7) == 0 && ((uintptr_t)weight & 7) == 0 && ((uintptr_t)centroid & 7) == 0 &&
                   ((uintptr_t)bbox & 3) == 0,
               "points / weights / labels / count / weight / centroid / bbox misaligned");
    hipStream_t s = (hipStream_t)stream;
    const unsigned kb = (unsigned)((num_clusters + 255) / 256), pb = (unsigned)((num_points + 255) / 256);
    unsigned long long *cnt = (unsigned long long *)count;
    uint32_t *box = (uint32_t *)bbox;
    gg_prof_begin(GG_K_CLUSTER_STATS, s);
    hipLaunchKernelGGL(cl_stats_init_kernel, dim3(kb), dim3(256), 0, s, num_clusters, cnt, weight, centroid, box);
    hipLaunchKernelGGL(cl_stats_kernel, dim3(pb), dim3(256), 0, s, num_points, num_clusters, points, weights, labels,
                       cnt, weight, centroid, box);
    hipLaunchKernelGGL(cl_stats_finish_kernel, dim3(kb), dim3(256), 0, s, num_clusters, weight, centroid, box);
    gg_prof_end(GG_K_CLUSTER_STATS, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
