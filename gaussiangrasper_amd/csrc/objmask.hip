// objmask.hip — per-view masks of a moved object (the reference's scripts/project_hull.py :83-121, step "scene
// update" of the paper's pipeline): project the object's points into every camera before and after the gripper's
// motion, take the exact convex hull of each projection's integer pixels, fill it closed, dilate, and reduce the
// masks' boxes.  The contract is in include/gg_raster.h (gg_object_masks) and PARITY.md "Scene update"; the design
// in DESIGN.md §3.14.
//
// A job is one (view, pose); job j = 2 view + pose, pose 0 = before, 1 = after.  Five launches, no host round trip
// between them:
//   1. om_bounds_kernel   one lane per point, OM_VIEWS views per workgroup: project, truncate, wave-reduce the
//                         job's integer bounds and drop count, one atomic per wave and quantity.
//   2. om_rows_init_kernel  the job's row span from its bounds; a span above max_rows flags the view (status =
//                         the smallest such view), otherwise the span's rows of the row table are reset.
//   3. om_rows_kernel     the same projection again; per row of each job the smallest and largest x (an atomic
//                         only where the lane's x lies outside the row's extremes as last read).
//                         The hull of a point set is the hull of its row extremes, and those come sorted by row.
//   4. om_hull_kernel     one wave per job: Andrew's monotone chain over the left extremes (lower hull in (y, x))
//                         and over the right extremes (upper hull), int64 cross products, wave-uniform.
//   5. om_fill_kernel     one workgroup per (view, image row): the closed hull's interval of each source row of the
//                         k x k dilation from the chains, exact integer floor / ceil division; three uint8 masks and
//                         the rows' contributions to the boxes (int32 atomics).
//   6. om_boxes_kernel    boxes and centres from the reduced extremes (-1 / NaN for an empty mask), drop counts.
// When a view is flagged, passes 3-6 write nothing; the call reads the status word back once, at its end.
#include <math.h>

#include "gg_common.h"
#include "ordered_sum.h"

#define OM_THREADS 256
#define OM_VIEWS 8                // views per workgroup of the projection passes (each lane's point is read once)
#define OM_EMPTY_LO 0x7fffffff
#define OM_EMPTY_HI (-0x7fffffff - 1)
#define OM_LIM 1073741824.0      // 2^30: |u|, |v| at or above it are dropped

struct OmMotion {
    double t[12];                 // [R | t], row-major 3 x 4
};

struct OmParams {
    int M, V, H, W, dilate, max_rows;
};

// per-job record of the workspace (int32): the bounds of the kept pixels, the drop count, the chain lengths
enum { JB_XMIN, JB_XMAX, JB_YMIN, JB_YMAX, JB_DROP, JB_NL, JB_NR, JB_WORDS = 8 };

// the contract's projection: c = E q, u = ((fx cx) + (cx0 cz)) / cz, truncated toward zero; false = dropped
__device__ __forceinline__ bool om_project(const double *__restrict__ E, const double *__restrict__ K, double q0,
                                           double q1, double q2, int &ix, int &iy) {
    const double c0 = ((E[0] * q0 + E[1] * q1) + E[2] * q2) + E[3];
    const double c1 = ((E[4] * q0 + E[5] * q1) + E[6] * q2) + E[7];
    const double cz = ((E[8] * q0 + E[9] * q1) + E[10] * q2) + E[11];
    if (!(cz > 0.0)) return false;
    const double u = ((K[0] * c0) + (K[2] * cz)) / cz;
    const double v = ((K[1] * c1) + (K[3] * cz)) / cz;
    if (!(fabs(u) < OM_LIM) || !(fabs(v) < OM_LIM)) return false;     // NaN / inf fail the comparison
    ix = (int)u;
    iy = (int)v;
    return true;
}

// the point of lane i, before (p) and after (T p)
__device__ __forceinline__ void om_points(const OmMotion &T, const double *__restrict__ P, int i, double *q) {
    const double x = P[3 * (size_t)i], y = P[3 * (size_t)i + 1], z = P[3 * (size_t)i + 2];
    q[0] = x;
    q[1] = y;
    q[2] = z;
#pragma unroll
    for (int r = 0; r < 3; ++r) q[3 + r] = ((T.t[4 * r] * x + T.t[4 * r + 1] * y) + T.t[4 * r + 2] * z) + T.t[4 * r + 3];
}

__device__ __forceinline__ int64_t om_span(const int32_t *jb) {
    return jb[JB_YMIN] > jb[JB_YMAX] ? 0 : (int64_t)jb[JB_YMAX] - (int64_t)jb[JB_YMIN] + 1;
}

// ---------------------------------------------------------------------------------------------------------------
// 1. bounds and drop counts
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OM_THREADS) void om_bounds_kernel(OmParams p, OmMotion T, const double *__restrict__ P,
                                                               const double *__restrict__ intr,
                                                               const double *__restrict__ w2c,
                                                               int32_t *__restrict__ jb) {
    const int i = blockIdx.x * OM_THREADS + threadIdx.x;
    const bool live = i < p.M;
    double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) om_points(T, P, i, q);
    const int v_end = min(p.V, (int)(blockIdx.y + 1) * OM_VIEWS);
    for (int v = blockIdx.y * OM_VIEWS; v < v_end; ++v) {
#pragma unroll
        for (int pose = 0; pose < 2; ++pose) {
            int ix = 0, iy = 0;
            const bool kept = live && om_project(w2c + 12 * (size_t)v, intr + 4 * (size_t)v, q[3 * pose],
                                                 q[3 * pose + 1], q[3 * pose + 2], ix, iy);
            const unsigned long long dropped = __ballot(live && !kept);
            const int xmin = gg_wave_min(kept ? ix : OM_EMPTY_LO), xmax = gg_wave_max(kept ? ix : OM_EMPTY_HI);
            const int ymin = gg_wave_min(kept ? iy : OM_EMPTY_LO), ymax = gg_wave_max(kept ? iy : OM_EMPTY_HI);
            if ((threadIdx.x & (GG_WAVE - 1)) == 0) {
                int32_t *r = jb + JB_WORDS * (size_t)(2 * v + pose);
                if (xmin != OM_EMPTY_LO) {
                    atomicMin(r + JB_XMIN, xmin);
                    atomicMax(r + JB_XMAX, xmax);
                    atomicMin(r + JB_YMIN, ymin);
                    atomicMax(r + JB_YMAX, ymax);
                }
                if (dropped) atomicAdd(r + JB_DROP, (int)__popcll(dropped));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 2. capacity check and row-table reset (only the span's rows)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OM_THREADS) void om_rows_init_kernel(OmParams p, const int32_t *__restrict__ jb,
                                                                  int2 *__restrict__ rows, int32_t *__restrict__ status) {
    const int j = blockIdx.y;
    const int64_t span = om_span(jb + JB_WORDS * (size_t)j);
    if (span > p.max_rows) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicMin(status, j >> 1);
        return;
    }
    int2 *r = rows + (size_t)j * p.max_rows;
    for (int64_t k = (int64_t)blockIdx.x * OM_THREADS + threadIdx.x; k < span; k += (int64_t)gridDim.x * OM_THREADS)
        r[k] = make_int2(OM_EMPTY_LO, OM_EMPTY_HI);
}

// ---------------------------------------------------------------------------------------------------------------
// 3. row extremes
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OM_THREADS) void om_rows_kernel(OmParams p, OmMotion T, const double *__restrict__ P,
                                                             const double *__restrict__ intr,
                                                             const double *__restrict__ w2c,
                                                             const int32_t *__restrict__ jb, int2 *__restrict__ rows) {
    const int i = blockIdx.x * OM_THREADS + threadIdx.x;
    if (i >= p.M) return;
    double q[6];
    om_points(T, P, i, q);
    const int v_end = min(p.V, (int)(blockIdx.y + 1) * OM_VIEWS);
    for (int v = blockIdx.y * OM_VIEWS; v < v_end; ++v) {
#pragma unroll
        for (int pose = 0; pose < 2; ++pose) {
            const int j = 2 * v + pose;
            const int32_t *b = jb + JB_WORDS * (size_t)j;
            const int64_t span = om_span(b);
            if (span > p.max_rows) continue;                     // flagged: nothing of this job is written
            int ix, iy;
            if (!om_project(w2c + 12 * (size_t)v, intr + 4 * (size_t)v, q[3 * pose], q[3 * pose + 1],
                            q[3 * pose + 2], ix, iy))
                continue;
            const int64_t r = (int64_t)iy - b[JB_YMIN];           // in [0, span): the same projection as pass 1
            if (r < 0 || r >= span) continue;
            int2 *row = rows + (size_t)j * p.max_rows + r;
            // the extremes only move outward, so a stale read can only cause a needless atomic, never a missed one:
            // once a row's extremes are near their final values, interior points issue none
            const int2 seen = *row;
            if (ix < seen.x) atomicMin(&row->x, ix);
            if (ix > seen.y) atomicMax(&row->y, ix);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 4. monotone chains.  Every lane of the wave runs the same chain (wave-uniform values); 64 rows at a time are
// loaded one per lane and taken in order with a shuffle.  The stacks are relative row indices (uint16: max_rows
// <= 65536) in the workspace; the top two entries of each are kept in registers, so only a pop that uncovers a
// third entry reads memory.  Every lane writes the (same) entry it may read back later: each lane reads only its
// own stores.
// ---------------------------------------------------------------------------------------------------------------
struct OmChain {
    int n;
    int64_t y1, x1, y2, x2;       // top (1) and the entry below it (2)
};

// in (y, x) coordinates: (a - o) x (b - o)
__device__ __forceinline__ int64_t om_cross(int64_t oy, int64_t ox, int64_t ay, int64_t ax, int64_t by, int64_t bx) {
    return (ay - oy) * (bx - ox) - (ax - ox) * (by - oy);
}

template <bool LEFT>
__device__ __forceinline__ void om_chain_push(OmChain &c, uint16_t *__restrict__ st, const int2 *__restrict__ rows,
                                              int64_t y, int64_t x) {
    while (c.n >= 2) {
        const int64_t cr = om_cross(c.y2, c.x2, c.y1, c.x1, y, x);
        if (LEFT ? cr > 0 : cr < 0) break;
        --c.n;                                                    // pop: the entry below becomes the top
        c.y1 = c.y2;
        c.x1 = c.x2;
        if (c.n >= 2) {
            const int r = st[c.n - 2];
            c.y2 = r;
            c.x2 = LEFT ? rows[r].x : rows[r].y;
        }
    }
    st[c.n] = (uint16_t)y;
    c.y2 = c.y1;
    c.x2 = c.x1;
    c.y1 = y;
    c.x1 = x;
    ++c.n;
}

__global__ __launch_bounds__(GG_WAVE) void om_hull_kernel(OmParams p, int32_t *__restrict__ jb,
                                                          const int2 *__restrict__ rows, uint16_t *__restrict__ chains) {
    const int j = blockIdx.x;
    int32_t *b = jb + JB_WORDS * (size_t)j;
    const int64_t span = om_span(b);
    if (span > p.max_rows) return;
    const int2 *rt = rows + (size_t)j * p.max_rows;
    uint16_t *sl = chains + (size_t)j * 2 * p.max_rows, *sr = sl + p.max_rows;
    const int lane = threadIdx.x;
    OmChain L{0, 0, 0, 0, 0}, R{0, 0, 0, 0, 0};
    for (int base = 0; base < (int)span; base += GG_WAVE) {
        const int2 mine = base + lane < span ? rt[base + lane] : make_int2(OM_EMPTY_LO, OM_EMPTY_HI);
        const int cnt = min(GG_WAVE, (int)span - base);
        for (int k = 0; k < cnt; ++k) {
            const int lo = __shfl(mine.x, k, GG_WAVE), hi = __shfl(mine.y, k, GG_WAVE);
            if (lo == OM_EMPTY_LO) continue;                      // no point on this row
            om_chain_push<true>(L, sl, rt, base + k, lo);
            om_chain_push<false>(R, sr, rt, base + k, hi);
        }
    }
    if (lane == 0) {
        b[JB_NL] = L.n;
        b[JB_NR] = R.n;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 5. fill
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t om_floor_div(int64_t a, int64_t d) {      // d > 0
    const int64_t q = a / d;
    return q - ((a % d != 0 && a < 0) ? 1 : 0);
}

// the closed hull's pixel interval [lo, hi] on absolute row y of job j, clipped to [0, W); lo > hi when empty
__device__ void om_row_interval(const OmParams &p, const int32_t *__restrict__ b, const int2 *__restrict__ rt,
                                const uint16_t *__restrict__ sl, const uint16_t *__restrict__ sr, int y, int &lo,
                                int &hi) {
    lo = 1;
    hi = 0;
    const int64_t span = om_span(b);
    const int64_t r = (int64_t)y - b[JB_YMIN];
    if (span == 0 || r < 0 || r >= span) return;
    int64_t e[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const uint16_t *st = side == 0 ? sl : sr;
        const int n = b[side == 0 ? JB_NL : JB_NR];
        int a = 0, z = n - 1;                                     // largest i with st[i] <= r: st[0] = 0 <= r
        while (a < z) {
            const int m = (a + z + 1) >> 1;
            if ((int64_t)st[m] <= r) a = m;
            else z = m - 1;
        }
        const int64_t ya = st[a];
        const int64_t xa = side == 0 ? rt[ya].x : rt[ya].y;
        if (ya == r) {
            e[side] = xa;
        } else {                                                  // ya < r < yb = st[a + 1]
            const int64_t yb = st[a + 1];
            const int64_t xb = side == 0 ? rt[yb].x : rt[yb].y;
            const int64_t num = (xb - xa) * (r - ya), den = yb - ya;
            e[side] = xa + (side == 0 ? -om_floor_div(-num, den) : om_floor_div(num, den));
        }
    }
    const int64_t l = e[0] < 0 ? 0 : e[0], h = e[1] > p.W - 1 ? p.W - 1 : e[1];
    if (l > h) return;
    lo = (int)l;
    hi = (int)h;
}

__global__ __launch_bounds__(OM_THREADS) void om_fill_kernel(OmParams p, const int32_t *__restrict__ jb,
                                                             const int2 *__restrict__ rows,
                                                             const uint16_t *__restrict__ chains,
                                                             const int32_t *__restrict__ status,
                                                             uint8_t *__restrict__ before, uint8_t *__restrict__ after,
                                                             uint8_t *__restrict__ uni, int32_t *__restrict__ box_ws,
                                                             int vec) {
    __shared__ int s_lo[2][GG_OBJMASK_MAX_DILATE], s_hi[2][GG_OBJMASK_MAX_DILATE];
    if (*status != OM_EMPTY_LO) return;                          // a view was flagged: no mask is written
    const int y = blockIdx.x, v = blockIdx.y;
    const int kk = max(p.dilate, 1), anc = kk / 2;
    const int t = threadIdx.x;
    if (t < 2 * kk) {
        const int pose = t / kk, dy = t - pose * kk;
        const int ys = y - anc + dy;                              // source row of the dilation
        int lo = 1, hi = 0;
        if (ys >= 0 && ys < p.H) {
            const int j = 2 * v + pose;
            const uint16_t *sl = chains + (size_t)j * 2 * p.max_rows;
            om_row_interval(p, jb + JB_WORDS * (size_t)j, rows + (size_t)j * p.max_rows, sl, sl + p.max_rows, ys, lo,
                            hi);
        }
        if (lo <= hi) {                                           // widen by the anchor, clip again
            lo = max(lo - (kk - 1 - anc), 0);
            hi = min(hi + anc, p.W - 1);
        }
        s_lo[pose][dy] = lo;
        s_hi[pose][dy] = hi;
    }
    __syncthreads();
    if (t == 0) {
        int cmin[2] = {OM_EMPTY_LO, OM_EMPTY_LO}, cmax[2] = {OM_EMPTY_HI, OM_EMPTY_HI};
        for (int pose = 0; pose < 2; ++pose)
            for (int d = 0; d < kk; ++d)
                if (s_lo[pose][d] <= s_hi[pose][d]) {
                    cmin[pose] = min(cmin[pose], s_lo[pose][d]);
                    cmax[pose] = max(cmax[pose], s_hi[pose][d]);
                }
        for (int m = 0; m < 3; ++m) {
            const int c0 = m < 2 ? cmin[m] : min(cmin[0], cmin[1]), c1 = m < 2 ? cmax[m] : max(cmax[0], cmax[1]);
            if (c0 > c1) continue;
            int32_t *bx = box_ws + 4 * (3 * (size_t)v + m);       // rmin, rmax, cmin, cmax
            atomicMin(bx + 0, y);
            atomicMax(bx + 1, y);
            atomicMin(bx + 2, c0);
            atomicMax(bx + 3, c1);
        }
    }
    const size_t off = ((size_t)v * p.H + y) * p.W;
    auto px = [&](int x, int pose) {
        bool in = false;
        for (int d = 0; d < kk; ++d) in |= (s_lo[pose][d] <= x) & (x <= s_hi[pose][d]);
        return in;
    };
    if (vec) {                                                    // W % 4 == 0, 4-byte aligned rows
        for (int x0 = 4 * t; x0 < p.W; x0 += 4 * OM_THREADS) {
            uint32_t wb = 0, wa = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                wb |= (uint32_t)px(x0 + e, 0) << (8 * e);
                wa |= (uint32_t)px(x0 + e, 1) << (8 * e);
            }
            *reinterpret_cast<uint32_t *>(before + off + x0) = wb;
            *reinterpret_cast<uint32_t *>(after + off + x0) = wa;
            *reinterpret_cast<uint32_t *>(uni + off + x0) = wb | wa;
        }
    } else {
        for (int x = t; x < p.W; x += OM_THREADS) {
            const bool b0 = px(x, 0), b1 = px(x, 1);
            before[off + x] = b0;
            after[off + x] = b1;
            uni[off + x] = b0 | b1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 6. boxes, centres, drop counts
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OM_THREADS) void om_boxes_kernel(int V, const int32_t *__restrict__ jb,
                                                              const int32_t *__restrict__ box_ws,
                                                              const int32_t *__restrict__ status,
                                                              int32_t *__restrict__ boxes, double *__restrict__ centres,
                                                              int32_t *__restrict__ dropped) {
    const int i = blockIdx.x * OM_THREADS + threadIdx.x;         // (view, mask)
    if (i >= 3 * V || *status != OM_EMPTY_LO) return;
    const int32_t *w = box_ws + 4 * (size_t)i;
    int32_t *o = boxes + 4 * (size_t)i;
    double *c = centres + 2 * (size_t)i;
    if (w[0] > w[1]) {
        o[0] = o[1] = o[2] = o[3] = -1;
        c[0] = c[1] = __builtin_nan("");
    } else {
        for (int k = 0; k < 4; ++k) o[k] = w[k];
        c[0] = 0.5 * (double)((int64_t)w[1] + w[0]);
        c[1] = 0.5 * (double)((int64_t)w[3] + w[2]);
    }
    const int v = i / 3, m = i - 3 * v;
    if (m < 2) dropped[2 * v + m] = jb[JB_WORDS * (size_t)(2 * v + m) + JB_DROP];
}

// jb reset: bounds to the empty sentinels, counts to 0; box extremes to the sentinels; status to "none"
__global__ __launch_bounds__(OM_THREADS) void om_reset_kernel(int V, int32_t *__restrict__ jb,
                                                              int32_t *__restrict__ box_ws,
                                                              int32_t *__restrict__ status) {
    const int i = blockIdx.x * OM_THREADS + threadIdx.x;
    if (i < 2 * V * JB_WORDS) {
        const int w = i % JB_WORDS;
        jb[i] = (w == JB_XMIN || w == JB_YMIN) ? OM_EMPTY_LO : (w == JB_XMAX || w == JB_YMAX) ? OM_EMPTY_HI : 0;
    }
    if (i < 12 * V) box_ws[i] = (i & 1) ? OM_EMPTY_HI : OM_EMPTY_LO;
    if (i == 0) *status = OM_EMPTY_LO;
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
struct OmLayout {
    int32_t *jb, *box_ws, *status;
    int2 *rows;
    uint16_t *chains;
};

static bool om_shape_ok(int V, int max_rows) {
    return V >= 0 && V <= GG_OBJMASK_MAX_VIEWS && max_rows >= 1 && max_rows <= GG_OBJMASK_MAX_ROWS;
}

static size_t om_layout(int V, int max_rows, OmLayout *L, char *base) {
    const size_t J = 2 * (size_t)V;
    GgCarve cv{base, 0};
    int32_t *jb = (int32_t *)cv.take(J * JB_WORDS * 4);
    int32_t *box_ws = (int32_t *)cv.take((size_t)V * 12 * 4);
    int32_t *status = (int32_t *)cv.take(4);
    int2 *rows = (int2 *)cv.take(J * (size_t)max_rows * sizeof(int2));
    uint16_t *chains = (uint16_t *)cv.take(J * 2 * (size_t)max_rows * sizeof(uint16_t));
    if (L) *L = OmLayout{jb, box_ws, status, rows, chains};
    return cv.off;
}

extern "C" size_t gg_object_masks_workspace(int num_views, int max_rows) {
    if (!om_shape_ok(num_views, max_rows)) return 0;
    return om_layout(num_views, max_rows, nullptr, nullptr);
}

extern "C" int gg_object_masks(int num_points, const double *points, const double *transform, int num_views,
                               const double *intrinsics, const double *w2c, int height, int width, int dilate,
                               int max_rows, uint8_t *before, uint8_t *after, uint8_t *union_mask, int32_t *boxes,
                               double *centres, int32_t *dropped, void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0, "num_points < 0");
    GG_REQUIRE(om_shape_ok(num_views, max_rows),
               "need 0 <= num_views <= GG_OBJMASK_MAX_VIEWS and 1 <= max_rows <= GG_OBJMASK_MAX_ROWS");
    GG_REQUIRE(height >= 1 && width >= 1 && height <= GG_OBJMASK_MAX_SIDE && width <= GG_OBJMASK_MAX_SIDE,
               "need 1 <= height, width <= GG_OBJMASK_MAX_SIDE");
    GG_REQUIRE(dilate >= 0 && dilate <= GG_OBJMASK_MAX_DILATE, "need 0 <= dilate <= GG_OBJMASK_MAX_DILATE");
    GG_REQUIRE(transform, "null pointer: transform (a host array of 12 doubles)");
    GG_REQUIRE(num_views == 0 || (intrinsics && w2c && before && after && union_mask && boxes && centres && dropped),
               "null pointer: cameras / outputs");
    GG_REQUIRE(num_points == 0 || points, "null pointer: points");
    GG_REQUIRE(((uintptr_t)points & 7) == 0 && ((uintptr_t)intrinsics & 7) == 0 && ((uintptr_t)w2c & 7) == 0 &&
                   ((uintptr_t)centres & 7) == 0 && ((uintptr_t)boxes & 3) == 0 && ((uintptr_t)dropped & 3) == 0,
               "points / intrinsics / w2c / centres / boxes / dropped misaligned");
    const size_t need = om_layout(num_views, max_rows, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    if (num_views == 0) return GG_OK;
    OmLayout L;
    om_layout(num_views, max_rows, &L, (char *)ws);
    OmMotion T;
    for (int k = 0; k < 12; ++k) T.t[k] = transform[k];
    const OmParams P{num_points, num_views, height, width, dilate, max_rows};
    const int vec = (width & 3) == 0 && (((uintptr_t)before | (uintptr_t)after | (uintptr_t)union_mask) & 3) == 0;
    hipStream_t s = (hipStream_t)stream;
    const unsigned J = 2u * (unsigned)num_views;
    const unsigned pblocks = (unsigned)((num_points + OM_THREADS - 1) / OM_THREADS);
    const unsigned vgroups = (unsigned)((num_views + OM_VIEWS - 1) / OM_VIEWS);
    gg_prof_begin(GG_K_OBJMASK, s);
    hipLaunchKernelGGL(om_reset_kernel, dim3((unsigned)((2 * num_views * JB_WORDS + OM_THREADS - 1) / OM_THREADS)),
                       dim3(OM_THREADS), 0, s, num_views, L.jb, L.box_ws, L.status);
    if (pblocks > 0)
        hipLaunchKernelGGL(om_bounds_kernel, dim3(pblocks, vgroups), dim3(OM_THREADS), 0, s, P, T, points, intrinsics,
                           w2c, L.jb);
    const unsigned iblocks = (unsigned)min((max_rows + OM_THREADS - 1) / OM_THREADS, 16);
    hipLaunchKernelGGL(om_rows_init_kernel, dim3(iblocks, J), dim3(OM_THREADS), 0, s, P, L.jb, L.rows, L.status);
    if (pblocks > 0)
        hipLaunchKernelGGL(om_rows_kernel, dim3(pblocks, vgroups), dim3(OM_THREADS), 0, s, P, T, points, intrinsics,
                           w2c, L.jb, L.rows);
    hipLaunchKernelGGL(om_hull_kernel, dim3(J), dim3(GG_WAVE), 0, s, P, L.jb, L.rows, L.chains);
    hipLaunchKernelGGL(om_fill_kernel, dim3((unsigned)height, (unsigned)num_views), dim3(OM_THREADS), 0, s, P, L.jb,
                       L.rows, L.chains, L.status, before, after, union_mask, L.box_ws, vec);
    hipLaunchKernelGGL(om_boxes_kernel, dim3((unsigned)((3 * num_views + OM_THREADS - 1) / OM_THREADS)),
                       dim3(OM_THREADS), 0, s, num_views, L.jb, L.box_ws, L.status, boxes, centres, dropped);
    gg_prof_end(GG_K_OBJMASK, s);
    GG_CHECK_LAUNCH();
    int32_t flagged = OM_EMPTY_LO;                                // the one read-back of the call
    hipError_t e = hipMemcpyAsync(&flagged, L.status, sizeof(flagged), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        gg_set_error("%s: reading the status back failed: %s", __func__, hipGetErrorString(e));
        return GG_ERR_LAUNCH;
    }
    if (flagged != OM_EMPTY_LO) {
        gg_set_error("%s: view %d: the object's projection spans more than max_rows = %d pixel rows; nothing was "
                     "written (raise max_rows)", __func__, flagged, max_rows);
        return GG_ERR_UNSUPPORTED;
    }
    return GG_OK;
}
