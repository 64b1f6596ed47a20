// roadmap.hip — the arm roadmap's two graph primitives (include/gg_raster.h "Arm roadmap").
//
// gg_roadmap_neighbours   the k nearest nodes of every query in a weighted joint metric, ties by the lowest index.
//                         A wave per query, RM_WAVES queries a workgroup; the workgroup stages tiles of RM_TILE nodes
//                         in LDS, joint-major, and every wave strides its lanes over the tile's candidates.  The
//                         wave's best k sit sorted in lanes 0..k-1; a ballot finds the candidates that beat the k-th
//                         and they are inserted one at a time by a shift of one lane.  Every loop is the same for
//                         the whole wave and all 64 lanes stay active in it: no predicate has to outlive a loop that
//                         lanes leave at different times.
// gg_roadmap_route        cost-to-go over a CSR graph for Q goal sets: rounds of pull relaxation in place, a thread
//                         per (query, node) that walks its own row, one launch a round, a changed flag per round
//                         read back once per batch of RM_BATCH rounds.  No kernel waits for another workgroup.
// gg_roadmap_descend      a wave per path: the lanes stride over the row, a ballot's lowest set lane of the first
//                         chunk with a fitting edge is the lowest row position.
#include <math.h>

#include <type_traits>

#include "gg_common.h"

#define RM_THREADS 256
#define RM_WAVES (RM_THREADS / GG_WAVE)
#define RM_TILE GG_ROADMAP_TILE
#define RM_PITCH (RM_TILE + 1)           // doubles between two joints' rows in LDS: staging writes spread over banks
#define RM_BATCH 16
#define RM_MAX_EDGES (1 << 27)

__device__ __forceinline__ int rm_load(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rm_store(int *p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the value of lane `lane` (the same in every lane: a scalar) in all lanes
__device__ __forceinline__ int rm_lane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ double rm_lane_d(double v, int lane) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// (d, i) before (e, j) in the order of the contract
__device__ __forceinline__ bool rm_before(double d, int i, double e, int j) { return d < e || (d == e && i < j); }

struct RmMetric {
    double m[GG_ARM_MAX_JOINTS];
};

template <int J>
__global__ __launch_bounds__(RM_THREADS) void roadmap_neighbours_kernel(RmMetric metric, int N,
                                                                        const double *__restrict__ nodes, int M,
                                                                        const double *__restrict__ queries,
                                                                        const int *__restrict__ skip,
                                                                        const unsigned char *__restrict__ valid, int k,
                                                                        int *__restrict__ idx, double *__restrict__ d2) {
    __shared__ double s_node[J * RM_PITCH];
    __shared__ unsigned char s_valid[RM_TILE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int m = blockIdx.x * RM_WAVES + (tid >> 6);          // the same for the whole wave
    const bool have = m < M;
    double q[J];
    bool finite = true;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        q[j] = have ? queries[(size_t)m * J + j] : 0.0;
        finite = finite && isfinite(q[j]);
    }
    const int avoid = have && skip ? skip[m] : -1;
    const bool work = __builtin_amdgcn_readfirstlane((int)(have && finite)) != 0;
    double bd = INFINITY;                                       // lanes 0..k-1: the best so far, ascending
    int bi = -1;
    for (int tile = 0; tile < N; tile += RM_TILE) {
        const int cnt = min(RM_TILE, N - tile);
        __syncthreads();                                        // the tile before this one has been read
        for (int e = tid; e < cnt * J; e += RM_THREADS)
            s_node[(e % J) * RM_PITCH + e / J] = nodes[(size_t)tile * J + e];
        for (int c = tid; c < cnt; c += RM_THREADS) s_valid[c] = valid ? valid[tile + c] : (unsigned char)1;
        __syncthreads();
        if (!work) continue;
        for (int base = 0; base < cnt; base += GG_WAVE) {
            const int c = base + lane;
            const int i = tile + c;
            const int cc = min(c, cnt - 1);                     // a lane past the end reads a node it does not use
            double e0 = metric.m[0] * (q[0] - s_node[cc]);
            double d = e0 * e0;
#pragma unroll
            for (int j = 1; j < J; ++j) {
                const double e = metric.m[j] * (q[j] - s_node[j * RM_PITCH + cc]);
                d = d + e * e;
            }
            // an entry of the node that is not finite makes d +inf or NaN: `d < inf` is then false as well
            const bool in = c < cnt && s_valid[cc] != 0 && i != avoid && d < INFINITY;
            const double kd = rm_lane_d(bd, k - 1);
            const int ki = rm_lane_i(bi, k - 1);
            unsigned long long beat = __ballot(in && rm_before(d, i, kd, ki));
            while (beat) {                                      // a scalar loop: `beat` is the same in every lane
                const int src = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(beat));
                beat &= beat - 1ull;
                const double cd = rm_lane_d(d, src);
                const int ci = rm_lane_i(i, src);
                // the k-th may have fallen since the ballot
                if (!rm_before(cd, ci, rm_lane_d(bd, k - 1), rm_lane_i(bi, k - 1))) continue;
                const int p = (int)__builtin_popcountll(__ballot(lane < k && rm_before(bd, bi, cd, ci)));
                const double ud = __shfl_up(bd, 1, GG_WAVE);
                const int ui = __shfl_up(bi, 1, GG_WAVE);
                if (lane < k && lane >= p) {
                    bd = lane == p ? cd : ud;
                    bi = lane == p ? ci : ui;
                }
            }
        }
    }
    if (have && lane < k) {
        idx[(size_t)m * k + lane] = finite ? bi : -1;
        d2[(size_t)m * k + lane] = finite ? bd : (double)NAN;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// route
// ---------------------------------------------------------------------------------------------------------------
struct RmGraph {
    int N, E, max_weight;
    const int *offsets, *targets, *weights;
    // the row of node i, cut to 0..E whatever `offsets` holds
    __device__ __forceinline__ void row(int i, int &lo, int &hi) const {
        lo = min(max(offsets[i], 0), E);
        hi = min(max(offsets[i + 1], lo), E);
    }
    __device__ __forceinline__ bool usable(int t, int w) const { return t >= 0 && t < N && w >= 1 && w <= max_weight; }
};

// cost = FAR, the round flags and `ignored` zero
__global__ __launch_bounds__(RM_THREADS) void roadmap_init_kernel(long long cells, int *__restrict__ cost,
                                                                  unsigned *__restrict__ flags,
                                                                  unsigned long long *__restrict__ ignored) {
    const long long i = (long long)blockIdx.x * RM_THREADS + threadIdx.x;
    if (i < cells) cost[i] = GG_FIELD_FAR;
    if (i < RM_BATCH) flags[i] = 0u;
    if (i == 0) *ignored = 0ull;
}

__global__ __launch_bounds__(RM_THREADS) void roadmap_zero_kernel(unsigned *p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0u;
}

// the edges of the rows that are not usable: an integer sum, so its order does not show
__global__ __launch_bounds__(RM_THREADS) void roadmap_ignored_kernel(RmGraph g,
                                                                     unsigned long long *__restrict__ ignored) {
    const int i = blockIdx.x * RM_THREADS + threadIdx.x;
    int bad = 0;
    if (i < g.N) {
        int lo, hi;
        g.row(i, lo, hi);
        for (int e = lo; e < hi; ++e) bad += g.usable(g.targets[e], g.weights[e]) ? 0 : 1;
    }
    for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, GG_WAVE);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(ignored, (unsigned long long)bad);
}

// goal g belongs to the query q with goal_offsets[q] <= g < goal_offsets[q + 1]
__global__ __launch_bounds__(RM_THREADS) void roadmap_goals_kernel(int N, int Q, int G,
                                                                   const int *__restrict__ goal_offsets,
                                                                   const int *__restrict__ goals, int *cost) {
    const int g = blockIdx.x * RM_THREADS + threadIdx.x;
    if (g >= G) return;
    const int node = goals[g];
    if (node < 0 || node >= N) return;
    int lo = 0, hi = Q;                                         // the last q with goal_offsets[q] <= g
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (goal_offsets[mid] <= g) lo = mid;
        else hi = mid;
    }
    rm_store(cost + (size_t)lo * N + node, 0);
}

// One round: every (query, node) takes the minimum over its own row.  The update is in place: a value read is this
// round's or the one before's, both weights of real walks, and the fixed point does not depend on which.
__global__ __launch_bounds__(RM_THREADS) void roadmap_round_kernel(RmGraph g, long long cells, int *cost,
                                                                   unsigned *flag) {
    const long long at = (long long)blockIdx.x * RM_THREADS + threadIdx.x;
    if (at >= cells) return;
    const int i = (int)(at % g.N);
    int *mine = cost + (at - i);
    const int cur = rm_load(mine + i);
    if (cur == 0) return;
    int lo, hi;
    g.row(i, lo, hi);
    int best = cur;
    for (int e = lo; e < hi; ++e) {
        const int t = g.targets[e], w = g.weights[e];
        if (g.usable(t, w)) best = min(best, w + rm_load(mine + t));        // < 2^31: both are <= 2^30
    }
    if (best < cur) {
        rm_store(mine + i, best);
        *flag = 1u;
    }
}

// One wave per path.  The cost falls by the edge's weight >= 1 at every step, so a walk visits no node twice.
__global__ __launch_bounds__(RM_THREADS) void roadmap_descend_kernel(RmGraph g, int Q, const int *__restrict__ cost,
                                                                     int P, const int *__restrict__ query,
                                                                     const int *__restrict__ starts, int max_nodes,
                                                                     int *__restrict__ path, int *__restrict__ length) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * RM_WAVES + (threadIdx.x >> 6);               // P max_nodes <= GG_FIELD_MAX_POSES
    if (p >= P) return;                                                     // the same for the whole wave
    const int q = __builtin_amdgcn_readfirstlane(query[p]);
    int node = __builtin_amdgcn_readfirstlane(starts[p]);
    int *row = path + (size_t)p * max_nodes;
    const bool inside = q >= 0 && q < Q && node >= 0 && node < g.N;
    const int *mine = cost + (size_t)(inside ? q : 0) * g.N;
    int here = __builtin_amdgcn_readfirstlane(inside ? mine[node] : GG_FIELD_FAR);
    int n = 0;
    if (here < GG_FIELD_FAR) {
        if (lane == 0) row[0] = node;
        n = 1;
        for (int step = 0; step < g.N && here != 0; ++step) {
            int lo, hi;
            g.row(node, lo, hi);
            int next = -1, w_next = 0;
            for (int base = lo; base < hi && next < 0; base += GG_WAVE) {   // scalar: `next` comes from a ballot
                const int e = base + lane;
                bool take = false;
                int t = 0, w = 0;
                if (e < hi) {
                    t = g.targets[e], w = g.weights[e];
                    take = g.usable(t, w) && mine[t] + w == here;
                }
                const unsigned long long found = __ballot(take);
                if (found) {
                    const int src = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(found));
                    next = rm_lane_i(t, src);
                    w_next = rm_lane_i(w, src);
                }
            }
            if (next < 0) break;                                // `cost` is no fixed point of this graph
            node = next;
            here -= w_next;
            if (lane == 0 && n < max_nodes) row[n] = node;
            ++n;
        }
        if (here != 0) n = 0;
    }
    if (n == 0) node = -1;
    for (int r = n + lane; r < max_nodes; r += GG_WAVE) row[r] = node;
    if (lane == 0) length[p] = n;
}

// ---------------------------------------------------------------------------------------------------------------
// the C ABI
// ---------------------------------------------------------------------------------------------------------------
template <typename F>
static void roadmap_dispatch(int J, F &&launch) {
    switch (J) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 3: launch(std::integral_constant<int, 3>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 5: launch(std::integral_constant<int, 5>{}); break;
        case 6: launch(std::integral_constant<int, 6>{}); break;
        case 7: launch(std::integral_constant<int, 7>{}); break;
        default: launch(std::integral_constant<int, 8>{}); break;
    }
}

extern "C" int gg_roadmap_neighbours(int num_joints, int num_nodes, const double *nodes, int num_queries,
                                     const double *queries, const double *metric, const int32_t *skip,
                                     const uint8_t *valid, int k, int32_t *idx, double *d2, gg_stream_t stream) {
    GG_REQUIRE(num_joints >= 1 && num_joints <= GG_ARM_MAX_JOINTS, "num_joints must be in 1..GG_ARM_MAX_JOINTS");
    GG_REQUIRE(num_nodes >= 0 && num_nodes <= GG_ROADMAP_MAX_NODES, "need 0 <= num_nodes <= GG_ROADMAP_MAX_NODES");
    GG_REQUIRE(num_queries >= 0 && num_queries <= GG_FIELD_MAX_POSES, "need 0 <= num_queries <= GG_FIELD_MAX_POSES");
    GG_REQUIRE(k >= 1 && k <= GG_ROADMAP_MAX_K, "k must be in 1..GG_ROADMAP_MAX_K");
    GG_REQUIRE(metric, "null pointer: metric (a host array of num_joints doubles)");
    RmMetric mt{};
    for (int j = 0; j < num_joints; ++j) {
        GG_REQUIRE(isfinite(metric[j]) && metric[j] >= 0.0, "metric: every entry must be finite and >= 0");
        mt.m[j] = metric[j];
    }
    if (num_queries == 0) return GG_OK;
    GG_REQUIRE(queries && idx && d2, "null pointer: queries / idx / d2");
    GG_REQUIRE(num_nodes == 0 || nodes, "null pointer: nodes");
    GG_REQUIRE((((uintptr_t)nodes | (uintptr_t)queries | (uintptr_t)d2) & 7) == 0, "nodes / queries / d2 misaligned");
    GG_REQUIRE((((uintptr_t)skip | (uintptr_t)idx) & 3) == 0, "skip / idx misaligned");
    roadmap_dispatch(num_joints, [&](auto joints) {
        hipLaunchKernelGGL((roadmap_neighbours_kernel<decltype(joints)::value>),
                           dim3((unsigned)((num_queries + RM_WAVES - 1) / RM_WAVES)), dim3(RM_THREADS), 0,
                           (hipStream_t)stream, mt, num_nodes, nodes, num_queries, queries, skip, valid, k, idx, d2);
    });
    GG_CHECK_LAUNCH();
    return GG_OK;
}

static bool roadmap_graph_ok(int N, int E, int max_weight) {
    return N >= 0 && N <= GG_ROADMAP_MAX_NODES && E >= 0 && E <= RM_MAX_EDGES && max_weight >= 1 &&
           (int64_t)N * max_weight < (int64_t)GG_FIELD_FAR;
}
#define RM_GRAPH_MSG                                                                                            \
    "need 0 <= num_nodes <= GG_ROADMAP_MAX_NODES, 0 <= num_edges <= 2^27, max_weight >= 1 and num_nodes max_weight " \
    "< 2^30"

// the round flags of one batch, then goal_offsets [Q + 1]
extern "C" size_t gg_roadmap_route_workspace(int num_nodes, int num_queries) {
    if (num_nodes < 0 || num_nodes > GG_ROADMAP_MAX_NODES || num_queries < 0 ||
        (int64_t)num_queries * (num_nodes > 0 ? num_nodes : 1) > (int64_t)RM_MAX_EDGES)
        return 0;
    return gg_align_up(sizeof(unsigned) * RM_BATCH, 256) + gg_align_up(sizeof(int32_t) * ((size_t)num_queries + 1), 256);
}

extern "C" int gg_roadmap_route(int num_nodes, int num_edges, const int32_t *offsets, const int32_t *targets,
                                const int32_t *weights, int32_t max_weight, int num_queries,
                                const int32_t *goal_offsets, const int32_t *goals, int32_t *cost, int64_t *ignored,
                                int max_rounds, int *rounds_out, void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(roadmap_graph_ok(num_nodes, num_edges, max_weight), RM_GRAPH_MSG);
    GG_REQUIRE(num_queries >= 0 && (int64_t)num_queries * (num_nodes > 0 ? num_nodes : 1) <= (int64_t)RM_MAX_EDGES,
               "need num_queries >= 0 and num_queries num_nodes <= 2^27");
    GG_REQUIRE(max_rounds >= 1, "max_rounds must be >= 1");
    GG_REQUIRE(rounds_out, "null pointer: rounds_out (a host int)");
    GG_REQUIRE(goal_offsets, "null pointer: goal_offsets (a host array of num_queries + 1 ints)");
    GG_REQUIRE(goal_offsets[0] == 0, "goal_offsets[0] must be 0");
    for (int q = 0; q < num_queries; ++q)
        GG_REQUIRE(goal_offsets[q + 1] >= goal_offsets[q], "goal_offsets must not decrease");
    const int G = goal_offsets[num_queries];
    GG_REQUIRE(G <= RM_MAX_EDGES, "goal_offsets: more than 2^27 goals");
    GG_REQUIRE(offsets && ignored, "null pointer: offsets / ignored");
    GG_REQUIRE(num_edges == 0 || (targets && weights), "null pointer: targets / weights");
    GG_REQUIRE(G == 0 || goals, "null pointer: goals");
    const int64_t cells = (int64_t)num_queries * num_nodes;
    GG_REQUIRE(cells == 0 || cost, "null pointer: cost");
    GG_REQUIRE((((uintptr_t)offsets | (uintptr_t)targets | (uintptr_t)weights | (uintptr_t)goals | (uintptr_t)cost) & 3) == 0 &&
                   ((uintptr_t)ignored & 7) == 0,
               "offsets / targets / weights / goals / cost / ignored misaligned");
    GG_REQUIRE_WS(ws, ws_bytes, gg_roadmap_route_workspace(num_nodes, num_queries));
    hipStream_t s = (hipStream_t)stream;
    unsigned *flags = (unsigned *)ws;
    int32_t *goal_dev = (int32_t *)((char *)ws + gg_align_up(sizeof(unsigned) * RM_BATCH, 256));
    const RmGraph g{num_nodes, num_edges, max_weight, offsets, targets, weights};
    *rounds_out = 0;
    const int64_t span = cells > RM_BATCH ? cells : RM_BATCH;
    hipLaunchKernelGGL(roadmap_init_kernel, dim3((unsigned)((span + RM_THREADS - 1) / RM_THREADS)), dim3(RM_THREADS), 0,
                       s, (long long)cells, cost, flags, reinterpret_cast<unsigned long long *>(ignored));
    if (num_nodes > 0)
        hipLaunchKernelGGL(roadmap_ignored_kernel, dim3((unsigned)((num_nodes + RM_THREADS - 1) / RM_THREADS)),
                           dim3(RM_THREADS), 0, s, g, reinterpret_cast<unsigned long long *>(ignored));
    GG_CHECK_LAUNCH();
    if (cells == 0 || G == 0) return GG_OK;
    hipError_t e = hipMemcpyAsync(goal_dev, goal_offsets, sizeof(int32_t) * ((size_t)num_queries + 1),
                                  hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        gg_set_error("%s: sending goal_offsets failed: %s", __func__, hipGetErrorString(e));
        return GG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(roadmap_goals_kernel, dim3((unsigned)((G + RM_THREADS - 1) / RM_THREADS)), dim3(RM_THREADS), 0,
                       s, num_nodes, num_queries, G, goal_dev, goals, cost);
    GG_CHECK_LAUNCH();
    // Rounds in batches; after each batch the flags come back.  A round that lowered nothing read a fixed point,
    // and the rounds behind it change nothing.  The loop is bounded by max_rounds, and no kernel in it can wait.
    unsigned changed[RM_BATCH];
    const unsigned blocks = (unsigned)((cells + RM_THREADS - 1) / RM_THREADS);
    for (int done = 0; done < max_rounds;) {
        const int n = max_rounds - done < RM_BATCH ? max_rounds - done : RM_BATCH;
        if (done > 0) hipLaunchKernelGGL(roadmap_zero_kernel, dim3(1), dim3(RM_THREADS), 0, s, flags, RM_BATCH);
        for (int r = 0; r < n; ++r)
            hipLaunchKernelGGL(roadmap_round_kernel, dim3(blocks), dim3(RM_THREADS), 0, s, g, (long long)cells, cost,
                               flags + r);
        GG_CHECK_LAUNCH();
        e = hipMemcpyAsync(changed, flags, sizeof(unsigned) * n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            gg_set_error("%s: reading the round flags back failed: %s", __func__, hipGetErrorString(e));
            return GG_ERR_LAUNCH;
        }
        for (int r = 0; r < n; ++r)
            if (changed[r] == 0u) {
                *rounds_out = done + r + 1;
                return GG_OK;
            }
        done += n;
    }
    *rounds_out = max_rounds;
    gg_set_error("%s: no convergence within max_rounds = %d rounds; cost holds upper bounds", __func__, max_rounds);
    return GG_ERR_NOT_CONVERGED;
}

extern "C" int gg_roadmap_descend(int num_nodes, int num_edges, const int32_t *offsets, const int32_t *targets,
                                  const int32_t *weights, int32_t max_weight, int num_queries, const int32_t *cost,
                                  int num_paths, const int32_t *query, const int32_t *starts, int max_nodes,
                                  int32_t *path, int32_t *length, gg_stream_t stream) {
    GG_REQUIRE(roadmap_graph_ok(num_nodes, num_edges, max_weight), RM_GRAPH_MSG);
    GG_REQUIRE(num_queries >= 0 && (int64_t)num_queries * (num_nodes > 0 ? num_nodes : 1) <= (int64_t)RM_MAX_EDGES,
               "need num_queries >= 0 and num_queries num_nodes <= 2^27");
    GG_REQUIRE(num_paths >= 0 && max_nodes >= 1 && (int64_t)num_paths * max_nodes <= GG_FIELD_MAX_POSES,
               "need num_paths >= 0, max_nodes >= 1 and num_paths max_nodes <= GG_FIELD_MAX_POSES");
    if (num_paths == 0) return GG_OK;
    GG_REQUIRE(offsets && query && starts && path && length, "null pointer: offsets / query / starts / path / length");
    GG_REQUIRE(num_edges == 0 || (targets && weights), "null pointer: targets / weights");
    GG_REQUIRE((int64_t)num_queries * num_nodes == 0 || cost, "null pointer: cost");
    GG_REQUIRE((((uintptr_t)offsets | (uintptr_t)targets | (uintptr_t)weights | (uintptr_t)cost | (uintptr_t)query |
                 (uintptr_t)starts | (uintptr_t)path | (uintptr_t)length) & 3) == 0,
               "offsets / targets / weights / cost / query / starts / path / length misaligned");
    const RmGraph g{num_nodes, num_edges, max_weight, offsets, targets, weights};
    hipLaunchKernelGGL(roadmap_descend_kernel, dim3((unsigned)((num_paths + RM_WAVES - 1) / RM_WAVES)),
                       dim3(RM_THREADS), 0, (hipStream_t)stream, g, num_queries, cost, num_paths, query, starts,
                       max_nodes, path, length);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
