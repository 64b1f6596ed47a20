// grasp_nms.hip — greedy pose-distance non-maximum suppression over GraspGroup rows, in the caller's order.  The
// contract is in include/gg_raster.h (gg_grasp_nms) and PARITY.md "Grasp NMS"; the design in DESIGN.md §3.21.
//
// Everything works in ORDER SPACE: position p = 0 .. A-1 of `order`, 64 positions to a word, W = ceil(A / 64) words.
//   1. nms_gather_kernel: keep = 0 and suppressor = -2 for every row; the pose (R, t: 12 fp32) of order[p] into the
//      workspace, every entry NaN for a position that does not take part (entry out of range, or an R / t entry that
//      is not finite), and one bit per position, by a wave-wide ballot, that says whether it takes part.  With NaN
//      poses the pair test below needs no flag: dd is NaN and NaN <= tt is false.
//   2. nms_pairs_kernel: the bit matrix near[p][q], A rows of W words, row-major.  One lane per row p, GN_TILE rows per
//      workgroup (grid.y), GN_WORDS words of partners per workgroup (grid.x), the partners' poses staged through LDS 64
//      at a time as fp64 and read as broadcasts; each lane builds its 64-bit word in registers and stores it.  The pair
//      test is bitwise symmetric (products commute, d -> -d squares the same), so only words at or right of the
//      diagonal are ever read, and workgroups wholly left of it leave at once.  The rotation is only looked at for
//      pairs that pass the translation test.
//   3. nms_walk_kernel: ONE workgroup, thread w owning word w of the `removed` bitset in a register (hence
//      GG_NMS_MAX_ORDER = 64 x 1024).  Step b = 0 .. W-1 resolves the 64 positions of block b: thread b publishes its
//      word through LDS (one barrier, each slot written once), every wave resolves the 64 x 64 diagonal block from
//      the diagonal words held one per lane, serially and redundantly in scalar registers, and then thread w > b ORs
//      the matrix rows of the block's newly kept positions, in order, into its word.  A bit can only turn on once, and
//      whoever turns it on writes that row's suppressor: the first kept row near it.
//      The step loop and the diagonal loop have trip counts W and 64 for every thread; the barrier sits in the step
//      loop only, outside every data-dependent branch.  The data-dependent loops (over the block's kept positions:
//      uniform, at most 64; over the bits a lane turns on: at most 64 over the whole kernel) hold no barrier.
// Determinism: no atomics; every output byte is a function of the inputs.
#include "grasp_common.h"

#define GN_TILE 256              // rows per workgroup of the pair kernel (one per lane)
#define GN_WORDS 4               // 64-partner words per workgroup of the pair kernel
#define GN_MAX_WORDS (GG_NMS_MAX_ORDER / 64)
#define GN_BATCH 8               // matrix rows a walk thread has in flight

struct NmsWs {
    float *pose;                 // [A][12]: R row-major, then t; NaN for a position that does not take part
    uint64_t *part;              // [W]: bit = the position takes part
    uint64_t *mat;               // [A][W]
};

__global__ __launch_bounds__(256) void nms_gather_kernel(int M, const float *__restrict__ grasps, int A,
                                                         const int32_t *__restrict__ order,
                                                         uint8_t *__restrict__ keep, int32_t *__restrict__ suppressor,
                                                         NmsWs ws) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < M) {
        keep[i] = 0;
        suppressor[i] = -2;
    }
    // no lane leaves before the ballot: a wave covers one word of positions (A padded to whole words by the grid)
    float v[12];
    bool ok = false;
    if (i < A) {
        const int r = order[i];
        ok = r >= 0 && r < M;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                v[k] = grasps[(size_t)r * GC_ROW + 4 + k];
                ok = ok && isfinite(v[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) ws.pose[(size_t)i * 12 + k] = ok ? v[k] : NAN;
    }
    const uint64_t word = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && i < A) ws.part[i >> 6] = word;
}

__global__ __launch_bounds__(GN_TILE) void nms_pairs_kernel(int A, int W, double tt, double bound, int symmetric,
                                                            NmsWs ws) {
    __shared__ double s_p[64][12];
    const int i0 = blockIdx.y * GN_TILE;
    const int w0 = blockIdx.x * GN_WORDS, w1 = min(W, w0 + GN_WORDS);
    if (w1 * 64 <= i0) return;                  // wholly left of the diagonal (uniform: before any barrier)
    const int i = i0 + threadIdx.x;
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = i < A ? (double)ws.pose[(size_t)i * 12 + k] : (double)NAN;
    for (int w = max(w0, i0 / 64); w < w1; ++w) {
        for (int k = threadIdx.x; k < 64 * 12; k += GN_TILE) {
            const int q = w * 64 + k / 12;
            s_p[k / 12][k % 12] = q < A ? (double)ws.pose[(size_t)w * 64 * 12 + k] : (double)NAN;
        }
        __syncthreads();
        uint64_t word = 0;
        for (int j = 0; j < 64; ++j) {
            const double *Q = s_p[j];
            const double d0 = P[9] - Q[9], d1 = P[10] - Q[10], d2 = P[11] - Q[11];
            const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
            if (!(dd <= tt)) continue;
            const double c0 = (P[0] * Q[0] + P[3] * Q[3]) + P[6] * Q[6];
            const double c1 = (P[1] * Q[1] + P[4] * Q[4]) + P[7] * Q[7];
            const double c2 = (P[2] * Q[2] + P[5] * Q[5]) + P[8] * Q[8];
            const double tr = (c0 + c1) + c2, trs = (c0 - c1) - c2;
            if (tr >= bound || (symmetric && trs >= bound)) word |= (uint64_t)1 << j;
        }
        if (i < A) ws.mat[(size_t)i * W + w] = word;
        __syncthreads();
    }
}

__device__ __forceinline__ uint64_t nms_uniform(uint64_t x) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(1024) void nms_walk_kernel(int A, int W, const int32_t *__restrict__ order, NmsWs ws,
                                                        uint8_t *__restrict__ keep, int32_t *__restrict__ suppressor,
                                                        int32_t *__restrict__ kept, int32_t *__restrict__ num_kept) {
    __shared__ uint64_t s_rem[GN_MAX_WORDS];
    const int w = threadIdx.x, lane = w & 63;
    const uint64_t *__restrict__ mat = ws.mat;
    uint64_t rem = w < W ? ~ws.part[w] : ~(uint64_t)0;       // removed: not kept whatever comes
    const uint64_t above = ~(((uint64_t)2 << lane) - 1);     // the bits of the positions after this lane's
    const uint64_t mine = (uint64_t)1 << lane;
    int count = 0;
    uint64_t d = lane < A ? mat[(size_t)lane * W] : 0;       // the diagonal block's rows, one per lane
    for (int b = 0; b < W; ++b) {
        if (w == b) s_rem[b] = rem;
        uint64_t dn = 0;
        if (b + 1 < W && (b + 1) * 64 + lane < A) dn = mat[(size_t)((b + 1) * 64 + lane) * W + (b + 1)];
        __syncthreads();
        // the diagonal block, serially, the same in every wave: r and km live in scalar registers
        uint64_t r = nms_uniform(s_rem[b]);
        uint64_t km = 0;
        int by = -1;                                         // in-block position that suppresses this lane's
        d &= above;
        const uint32_t dlo = (uint32_t)d, dhi = (uint32_t)(d >> 32);
#pragma unroll
        for (int k = 0; k < 64; ++k) {
            const uint64_t dk = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)dhi, k) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)dlo, k);
            if (!((r >> k) & 1)) {
                km |= (uint64_t)1 << k;
                if ((dk & ~r) & mine) by = k;
                r |= dk;
            }
        }
        const int base = b * 64;
        if (w < 64) {                                        // wave 0 writes the block's kept and in-block suppressed
            const int p = base + lane;
            if (km & mine) {
                const int row = order[p];
                keep[row] = 1;
                suppressor[row] = -1;
                kept[count + __popcll(km & (mine - 1))] = row;
            } else if (by >= 0) {
                suppressor[order[p]] = order[base + by];
            }
        }
        count += __popcll(km);
        if (w > b && w < W) {
            uint64_t todo = km;
            while (todo) {                                   // uniform: km is the same in every thread
                uint64_t m[GN_BATCH];
                int ks[GN_BATCH];
#pragma unroll
                for (int u = 0; u < GN_BATCH; ++u) {
                    ks[u] = todo ? __builtin_ctzll(todo) : -1;
                    todo &= todo - 1;
                    m[u] = ks[u] >= 0 ? mat[(size_t)(base + ks[u]) * W + w] : 0;
                }
#pragma unroll
                for (int u = 0; u < GN_BATCH; ++u) {
                    uint64_t on = m[u] & ~rem;
                    rem |= on;
                    if (on) {
                        const int by_row = order[base + ks[u]];
                        while (on) {
                            const int q = __builtin_ctzll(on);
                            on &= on - 1;
                            suppressor[order[w * 64 + q]] = by_row;
                        }
                    }
                }
            }
        }
        d = dn;
    }
    for (int p = count + threadIdx.x; p < A; p += blockDim.x) kept[p] = -1;
    if (threadIdx.x == 0) *num_kept = count;
}

__global__ __launch_bounds__(256) void nms_empty_kernel(int M, uint8_t *__restrict__ keep,
                                                        int32_t *__restrict__ suppressor,
                                                        int32_t *__restrict__ num_kept) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < M) {
        keep[i] = 0;
        suppressor[i] = -2;
    }
    if (i == 0) *num_kept = 0;
}

static size_t nms_layout(int A, NmsWs *w, char *base) {
    const size_t W = ((size_t)A + 63) / 64;
    GgCarve cv{base, 0};
    NmsWs t;
    t.pose = (float *)cv.take((size_t)A * 12 * 4);
    t.part = (uint64_t *)cv.take(W * 8);
    t.mat = (uint64_t *)cv.take((size_t)A * W * 8);
    if (w) *w = t;
    return cv.off < 256 ? 256 : cv.off;     // never 0 for a count in range: 0 says "out of range"
}

extern "C" size_t gg_grasp_nms_workspace(int num_order) {
    if (num_order < 0 || num_order > GG_NMS_MAX_ORDER) return 0;
    return nms_layout(num_order, nullptr, nullptr);
}

extern "C" int gg_grasp_nms(int num_grasps, const float *grasps, int num_order, const int32_t *order,
                            double translation, double cos_rotation, int symmetric, uint8_t *keep,
                            int32_t *suppressor, int32_t *kept, int32_t *num_kept, void *ws, size_t ws_bytes,
                            gg_stream_t stream) {
    GG_REQUIRE(num_grasps >= 0, "num_grasps < 0");
    GG_REQUIRE(num_grasps <= GG_GRASP_MAX, "num_grasps > GG_GRASP_MAX");
    GG_REQUIRE(num_order >= 0, "num_order < 0");
    GG_REQUIRE(num_order <= GG_NMS_MAX_ORDER, "num_order > GG_NMS_MAX_ORDER");
    GG_REQUIRE(isfinite(translation) && translation >= 0.0, "translation must be finite and >= 0");
    GG_REQUIRE(cos_rotation >= -1.0 && cos_rotation <= 1.0, "cos_rotation must be in [-1, 1]");
    if (num_grasps == 0 && num_order == 0) return GG_OK;
    GG_REQUIRE(num_kept, "null pointer: num_kept");
    GG_REQUIRE(num_grasps == 0 || (grasps && keep && suppressor), "null pointer: grasps / keep / suppressor");
    GG_REQUIRE(num_order == 0 || (order && kept), "null pointer: order / kept");
    GG_REQUIRE(((uintptr_t)grasps & 3) == 0 && ((uintptr_t)order & 3) == 0 && ((uintptr_t)suppressor & 3) == 0 &&
                   ((uintptr_t)kept & 3) == 0 && ((uintptr_t)num_kept & 3) == 0,
               "grasps / order / suppressor / kept / num_kept misaligned");
    hipStream_t s = (hipStream_t)stream;
    const int M = num_grasps, A = num_order;
    if (A == 0) {
        gg_prof_begin(GG_K_GRASP_NMS, s);
        hipLaunchKernelGGL(nms_empty_kernel, dim3((unsigned)((max(M, 1) + 255) / 256)), dim3(256), 0, s, M, keep,
                           suppressor, num_kept);
        gg_prof_end(GG_K_GRASP_NMS, s);
        GG_CHECK_LAUNCH();
        return GG_OK;
    }
    const size_t need = nms_layout(A, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    NmsWs w;
    nms_layout(A, &w, (char *)ws);
    const int W = (A + 63) / 64;
    const double tt = translation * translation, bound = 1.0 + 2.0 * cos_rotation;
    gg_prof_begin(GG_K_GRASP_NMS, s);
    hipLaunchKernelGGL(nms_gather_kernel, dim3((unsigned)((max(M, W * 64) + 255) / 256)), dim3(256), 0, s, M, grasps,
                       A, order, keep, suppressor, w);
    hipLaunchKernelGGL(nms_pairs_kernel, dim3((unsigned)((W + GN_WORDS - 1) / GN_WORDS),
                                              (unsigned)((A + GN_TILE - 1) / GN_TILE)),
                       dim3(GN_TILE), 0, s, A, W, tt, bound, symmetric, w);
    hipLaunchKernelGGL(nms_walk_kernel, dim3(1), dim3((unsigned)((W + 63) / 64 * 64)), 0, s, A, W, order, w, keep,
                       suppressor, kept, num_kept);
    gg_prof_end(GG_K_GRASP_NMS, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
