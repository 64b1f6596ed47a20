// place.hip — where an object can be put down: points to integer height maps over a plane grid, and the exact resting
// search of an object's underside maps over the scene's top map (a max-plus correlation over every yaw and anchor).
// The contract is in include/gg_raster.h (gg_height_map, gg_place_search) and PARITY.md "Placement"; the design in
// DESIGN.md §3.28.
//
// gg_height_map     one launch, a thread per point, the frames in LDS: per frame the point's cell by field_cell's rule
//                   (field_cell.h) and its level by the same rule, then one integer atomicMax.  Maxima commute: the map
//                   is the same from run to run.  `dropped` is counted per wave (ballot) and frame.
// gg_place_search   one launch, a workgroup per PS_TILE x PS_TILE anchors of one yaw.  The scene tile with its halo,
//                   (PS_TILE + A - 1) x (PS_TILE + B - 1) ints, sits in LDS; a lane owns PS_ROWS anchors of one column
//                   j, PS_TILE / PS_ROWS rows apart, so a half wave reads 32 consecutive ints of one tile row: no bank
//                   conflict at any pitch.  The object's cells are never listed in memory: every wave loads a row of
//                   `under` (two ints per lane), a ballot marks its cells and the wave walks the set bits, the cell's
//                   value read out of the owning lane, so that empty cells cost nothing and the row's loads wait on
//                   vmcnt, not on the counter the LDS reads use.  Two sweeps: the maximum (and the smallest scene
//                   level met, which tells whether a covered cell was empty), then the cells within `tol` of it.
//                   Integers only, no atomics, ordinary vector stores.
#include <math.h>

#include "field_cell.h"
#include "gg_common.h"

#define PH_THREADS 256
#define PS_THREADS 256
#define PS_TILE 32                 // anchors per tile edge
#define PS_ROWS 4                  // anchors per lane
#define PS_ROW_STEP (PS_TILE / PS_ROWS)

static_assert(PS_THREADS == PS_ROW_STEP * PS_TILE, "a workgroup's lanes times PS_ROWS cover the tile");
static_assert(GG_PLACE_MAX_FOOT <= 128, "a lane holds two cells of a row of `under`; a row's count fits 8 bits");

struct PlaceGrid {
    int U, V;
    double lo_u, lo_v, h, hz;
};

// ---------------------------------------------------------------------------------------------------------------
// height maps
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PH_THREADS) void place_height_kernel(PlaceGrid g, int N, const float *__restrict__ points,
                                                                  const float *__restrict__ weights, double min_weight,
                                                                  int F, const double *__restrict__ frames,
                                                                  int *__restrict__ map,
                                                                  unsigned long long *__restrict__ dropped) {
    __shared__ double s_fr[GG_PLACE_MAX_YAWS * 12];
    for (int t = threadIdx.x; t < F * 12; t += PH_THREADS) s_fr[t] = frames[t];
    __syncthreads();
    const int i = blockIdx.x * PH_THREADS + threadIdx.x;      // N <= 2^30 and the grid covers N: no overflow
    const int lane = threadIdx.x & 63;
    bool part = false;
    double p[3] = {0.0, 0.0, 0.0};
    if (i < N) {
        part = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = points[(size_t)i * 3 + a];
            part = part && isfinite(v);
            p[a] = (double)v;
        }
        if (weights) part = part && min_weight < (double)weights[i];      // false for a NaN weight
    }
    for (int f = 0; f < F; ++f) {
        const double *fr = s_fr + f * 12;
        bool landed = false;
        if (part) {
            const double d0 = p[0] - fr[0], d1 = p[1] - fr[1], d2 = p[2] - fr[2];
            const double c0 = (d0 * fr[3] + d1 * fr[4]) + d2 * fr[5];
            const double c1 = (d0 * fr[6] + d1 * fr[7]) + d2 * fr[8];
            const double c2 = (d0 * fr[9] + d1 * fr[10]) + d2 * fr[11];
            const double du = c0 - g.lo_u, dv = c1 - g.lo_v;
            if (isfinite(du) && isfinite(dv) && isfinite(c2)) {
                const int a = field_cell(du, g.h), b = field_cell(dv, g.h);
                if (a >= 0 && a < g.U && b >= 0 && b < g.V) {
                    int z = field_cell(c2, g.hz);
                    z = max(-GG_PLACE_MAX_LEVEL, min(GG_PLACE_MAX_LEVEL, z));
                    atomicMax(map + ((size_t)f * g.U + a) * g.V + b, z);
                    landed = true;
                }
            }
        }
        const uint64_t out = __ballot(i < N && !landed);
        if (lane == 0 && out) atomicAdd(dropped + f, (unsigned long long)__builtin_popcountll(out));
    }
}

__global__ void place_zero_kernel(unsigned long long *p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0ull;
}

// ---------------------------------------------------------------------------------------------------------------
// resting search
// ---------------------------------------------------------------------------------------------------------------
typedef unsigned short ps_u16x2 __attribute__((ext_vector_type(2)));

// t + u with wrap-around: an empty scene cell (INT32_MIN) gives a sum that is never used (the anchor is invalid)
__device__ __forceinline__ int ps_sum(int t, int u) { return (int)((unsigned)t + (unsigned)u); }

// A lane's two cells of row `urow` of an underside map: b = lane and b = lane + 64.
__device__ __forceinline__ void ps_load_row(const int *__restrict__ urow, int B, int lane, int &u0, int &u1) {
    u0 = lane < B ? urow[lane] : GG_PLACE_EMPTY;
    u1 = lane + 64 < B ? urow[lane + 64] : GG_PLACE_EMPTY;
}

__global__ __launch_bounds__(PS_THREADS) void place_search_kernel(int V, int A, int B, int I, int J, int tol,
                                                                  const int *__restrict__ top,
                                                                  const int *__restrict__ under, int *__restrict__ rest,
                                                                  int *__restrict__ contact,
                                                                  int *__restrict__ support) {
    extern __shared__ int ps_tile[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int k = blockIdx.z, i0 = blockIdx.y * PS_TILE, j0 = blockIdx.x * PS_TILE;
    const int P = PS_TILE + B - 1;                                   // the tile's pitch, ints
    const int rows = min(PS_TILE, I - i0) + A - 1, cols = min(PS_TILE, J - j0) + B - 1;      // i0 + rows <= U
    for (int r = tid >> 6; r < rows; r += PS_THREADS / 64)
        for (int c = lane; c < cols; c += 64) ps_tile[r * P + c] = top[(size_t)(i0 + r) * V + j0 + c];
    __syncthreads();
    // the lane's anchors: column j0 + tj, rows i0 + ti0 + r PS_ROW_STEP.  An anchor past I or J reads tile cells that
    // were not loaded (inside the allocation: row < PS_TILE + A - 1, column < P) and stores nothing.
    const int tj = tid & (PS_TILE - 1), ti0 = tid / PS_TILE;
    const int *__restrict__ mine = ps_tile + ti0 * P + tj;
    const int *__restrict__ um = under + (size_t)k * A * B;
    const int rstep = PS_ROW_STEP * P;

    int best[PS_ROWS], low[PS_ROWS];
#pragma unroll
    for (int r = 0; r < PS_ROWS; ++r) best[r] = INT32_MIN, low[r] = INT32_MAX;
    int cells = 0;
    int nx[2];                                          // the next row of `under`, requested a row ahead
    ps_load_row(um, B, lane, nx[0], nx[1]);
    for (int a = 0; a < A; ++a) {
        const int uu[2] = {nx[0], nx[1]};
        if (a + 1 < A) ps_load_row(um + (a + 1) * B, B, lane, nx[0], nx[1]);
        const int *__restrict__ trow = mine + a * P;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            uint64_t m = __ballot(uu[half] != GG_PLACE_EMPTY);
            cells += __builtin_popcountll(m);
            for (; m != 0ull; m &= m - 1ull) {
                const int bl = (int)__builtin_ctzll(m);
                const int u = __builtin_amdgcn_readlane(uu[half], bl);
                const int *__restrict__ at = trow + bl + 64 * half;
#pragma unroll
                for (int r = 0; r < PS_ROWS; ++r) {
                    const int t = at[r * rstep];
                    best[r] = max(best[r], ps_sum(t, u));
                    low[r] = min(low[r], t);
                }
            }
        }
    }

    bool ok[PS_ROWS];
    int thr[PS_ROWS], cnt[PS_ROWS], sa[PS_ROWS], sb[PS_ROWS], amin[PS_ROWS], amax[PS_ROWS];
    ps_u16x2 bb[PS_ROWS];
#pragma unroll
    for (int r = 0; r < PS_ROWS; ++r) {
        ok[r] = cells > 0 && low[r] != GG_PLACE_EMPTY;
        thr[r] = ps_sum(best[r], -tol);                 // valid anchors: |best| < 2^30, tol <= 2^28
        cnt[r] = sa[r] = sb[r] = 0;
        amin[r] = amax[r] = -1;
        bb[r] = (ps_u16x2){0, 0};
    }
    ps_load_row(um, B, lane, nx[0], nx[1]);
    for (int a = 0; a < A; ++a) {
        const int uu[2] = {nx[0], nx[1]};
        if (a + 1 < A) ps_load_row(um + (a + 1) * B, B, lane, nx[0], nx[1]);
        const int *__restrict__ trow = mine + a * P;
        unsigned acc[PS_ROWS];                          // of this row of the object: count | sum of b << 8
#pragma unroll
        for (int r = 0; r < PS_ROWS; ++r) acc[r] = 0u;
        bool any = false;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            uint64_t m = __ballot(uu[half] != GG_PLACE_EMPTY);
            any = any || m != 0ull;
            for (; m != 0ull; m &= m - 1ull) {
                const int bl = (int)__builtin_ctzll(m);
                const int u = __builtin_amdgcn_readlane(uu[half], bl);
                const int b = bl + 64 * half;
                const unsigned one = 1u | ((unsigned)b << 8);
                const unsigned box = (unsigned)(b + 1) | ((unsigned)(GG_PLACE_MAX_FOOT - b) << 16);
                const int *__restrict__ at = trow + b;
#pragma unroll
                for (int r = 0; r < PS_ROWS; ++r) {
                    const bool c = ps_sum(at[r * rstep], u) >= thr[r];
                    acc[r] += c ? one : 0u;
                    bb[r] = __builtin_elementwise_max(bb[r], __builtin_bit_cast(ps_u16x2, c ? box : 0u));
                }
            }
        }
        if (any) {
#pragma unroll
            for (int r = 0; r < PS_ROWS; ++r) {
                const int n = (int)(acc[r] & 0xffu);
                cnt[r] += n;
                sb[r] += (int)(acc[r] >> 8);
                sa[r] += a * n;
                amax[r] = n ? a : amax[r];
                amin[r] = (n && amin[r] < 0) ? a : amin[r];
            }
        }
    }

    const int j = j0 + tj;
#pragma unroll
    for (int r = 0; r < PS_ROWS; ++r) {
        const int i = i0 + ti0 + r * PS_ROW_STEP;
        if (i >= I || j >= J) continue;
        const size_t o = ((size_t)k * I + i) * J + j;
        int *__restrict__ sp = support + o * 6;
        if (ok[r]) {
            rest[o] = best[r];
            contact[o] = cnt[r];
            sp[0] = sa[r];
            sp[1] = sb[r];
            sp[2] = amin[r];
            sp[3] = amax[r];
            sp[4] = GG_PLACE_MAX_FOOT - (int)bb[r][1];
            sp[5] = (int)bb[r][0] - 1;
        } else {
            rest[o] = GG_PLACE_EMPTY;
            contact[o] = 0;
            sp[0] = sp[1] = 0;
            sp[2] = sp[3] = sp[4] = sp[5] = -1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
static bool place_dims_ok(const int32_t *dims) {
    return dims && dims[0] >= 1 && dims[0] <= GG_PLACE_MAX_DIM && dims[1] >= 1 && dims[1] <= GG_PLACE_MAX_DIM;
}

#define PLACE_DIMS_MSG "dims: need a host array U, V with 1 <= each <= GG_PLACE_MAX_DIM"

extern "C" int gg_height_map(int num_points, const float *points, const float *weights, double min_weight,
                             int num_frames, const double *frames, const double *grid, const int32_t *dims,
                             int32_t *map, int64_t *dropped, gg_stream_t stream) {
    GG_REQUIRE(place_dims_ok(dims), PLACE_DIMS_MSG);
    GG_REQUIRE(num_frames >= 1 && num_frames <= GG_PLACE_MAX_YAWS, "num_frames must be in 1..GG_PLACE_MAX_YAWS");
    GG_REQUIRE(num_points >= 0 && num_points <= GG_PLACE_MAX_POINTS, "need 0 <= num_points <= GG_PLACE_MAX_POINTS");
    GG_REQUIRE(grid, "null pointer: grid (a host array of 4 doubles)");
    GG_REQUIRE(isfinite(grid[0]) && isfinite(grid[1]) && isfinite(grid[2]) && isfinite(grid[3]) && grid[2] > 0.0 &&
                   grid[3] > 0.0,
               "grid: lo_u, lo_v must be finite, the cell edge h and the level height hz finite and > 0");
    GG_REQUIRE(!isnan(min_weight), "min_weight is NaN");
    GG_REQUIRE(dropped, "null pointer: dropped");
    GG_REQUIRE(((uintptr_t)dropped & 7) == 0, "dropped misaligned");
    if (num_points > 0) {
        GG_REQUIRE(points && frames && map, "null pointer: points / frames / map");
        GG_REQUIRE((((uintptr_t)points | (uintptr_t)weights | (uintptr_t)map) & 3) == 0 &&
                       ((uintptr_t)frames & 7) == 0,
                   "points / weights / map / frames misaligned");
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *drop = reinterpret_cast<unsigned long long *>(dropped);
    hipLaunchKernelGGL(place_zero_kernel, dim3(1), dim3(GG_PLACE_MAX_YAWS), 0, s, drop, num_frames);
    if (num_points == 0) {
        GG_CHECK_LAUNCH();
        return GG_OK;
    }
    const PlaceGrid g{dims[0], dims[1], grid[0], grid[1], grid[2], grid[3]};
    hipLaunchKernelGGL(place_height_kernel, dim3((unsigned)((num_points + PH_THREADS - 1) / PH_THREADS)),
                       dim3(PH_THREADS), 0, s, g, num_points, points, weights, min_weight, num_frames, frames, map,
                       drop);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_place_search(const int32_t *dims, const int32_t *top, int num_yaws, const int32_t *foot,
                               const int32_t *under, int32_t tol, int32_t *rest, int32_t *contact, int32_t *support,
                               gg_stream_t stream) {
    GG_REQUIRE(place_dims_ok(dims), PLACE_DIMS_MSG);
    GG_REQUIRE(num_yaws >= 0 && num_yaws <= GG_PLACE_MAX_YAWS, "num_yaws must be in 0..GG_PLACE_MAX_YAWS");
    GG_REQUIRE(foot && foot[0] >= 1 && foot[0] <= GG_PLACE_MAX_FOOT && foot[1] >= 1 && foot[1] <= GG_PLACE_MAX_FOOT,
               "foot: need a host array A, B with 1 <= each <= GG_PLACE_MAX_FOOT");
    GG_REQUIRE(foot[0] <= dims[0] && foot[1] <= dims[1], "foot: need A <= U and B <= V");
    GG_REQUIRE(tol >= 0 && tol <= GG_PLACE_MAX_LEVEL, "tol must be in 0..GG_PLACE_MAX_LEVEL");
    if (num_yaws == 0) return GG_OK;
    GG_REQUIRE(top && under && rest && contact && support, "null pointer: top / under / rest / contact / support");
    GG_REQUIRE((((uintptr_t)top | (uintptr_t)under | (uintptr_t)rest | (uintptr_t)contact | (uintptr_t)support) & 3) ==
                   0,
               "top / under / rest / contact / support misaligned");
    const int V = dims[1], A = foot[0], B = foot[1];
    const int I = dims[0] - A + 1, J = V - B + 1;
    const size_t lds = sizeof(int) * (size_t)(PS_TILE + A - 1) * (size_t)(PS_TILE + B - 1);      // <= 159^2 ints
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)place_search_kernel,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            gg_set_error("%s: %zu bytes of LDS refused: %s", __func__, lds, hipGetErrorString(e));
            return GG_ERR_LAUNCH;
        }
    }
    hipLaunchKernelGGL(place_search_kernel,
                       dim3((unsigned)((J + PS_TILE - 1) / PS_TILE), (unsigned)((I + PS_TILE - 1) / PS_TILE),
                            (unsigned)num_yaws),
                       dim3(PS_THREADS), lds, (hipStream_t)stream, V, A, B, I, J, (int)tol, top, under, rest, contact,
                       support);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
