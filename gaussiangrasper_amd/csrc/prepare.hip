// prepare.hip — scene preparation from RGB-D frames (the reference's scripts/generate_data.py, step (a) of the
// paper's pipeline): back-projection of depth frames to a base-frame seed cloud, its uniform subsample, and
// per-view world-frame normal maps.  The contract is in include/gg_raster.h (gg_backproject, gg_subsample,
// gg_depth_normals) and PARITY.md "Scene preparation"; the design in DESIGN.md §3.13.
//
// Order: every output row sits where the reference's frame-major, row-major boolean indexing puts it.  A
// workgroup owns PP_TILE consecutive items (4 per lane, consecutive); a count pass writes one count per workgroup,
// one workgroup scans the counts in order (pp_scan_single), and the emit pass writes each kept item at its
// workgroup's offset plus its in-workgroup rank.  No atomics decide a position: two calls are bit-identical.
// All arithmetic is fp64 in the stated order, no contraction (-ffp-contract=off).
#include <math.h>

#include "gg_common.h"
#include "prep_common.h"

#define PP_SEL_BINS 65536        // radix-select digit bins (16 bits)

// ---------------------------------------------------------------------------------------------------------------
// back-projection
// ---------------------------------------------------------------------------------------------------------------
struct BpParams {
    int F, H, W;
    double d_lo, d_hi, z_lo, z_hi;
};

// Pixel p (frame-major, row-major) -> kept?  and its base-frame point.
__device__ __forceinline__ bool bp_point(const BpParams &P, const double *__restrict__ depth,
                                         const uint8_t *__restrict__ mask, const double *__restrict__ intr,
                                         const double *__restrict__ c2w, int64_t p, double &x, double &y,
                                         double &z) {
    const double d = depth[p];
    if (!(mask[p] != 0 && d > P.d_lo && d < P.d_hi)) return false;
    const int64_t hw = (int64_t)P.H * P.W;
    const int f = (int)(p / hw);
    const int64_t r = p - (int64_t)f * hw;
    const int v = (int)(r / P.W), u = (int)(r - (int64_t)v * P.W);
    const double *K = intr + 4 * (size_t)f;       // fx fy cx cy
    const double X = (((double)u - K[2]) * d) / K[0];
    const double Y = (((double)v - K[3]) * d) / K[1];
    const double Z = d;
    const double *T = c2w + 16 * (size_t)f;
    z = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
    if (!(z > P.z_lo && z < P.z_hi)) return false;
    x = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
    y = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
    return true;
}

__global__ __launch_bounds__(PP_THREADS) void backproject_count_kernel(BpParams P, const double *__restrict__ depth,
                                                                       const uint8_t *__restrict__ mask,
                                                                       const double *__restrict__ intr,
                                                                       const double *__restrict__ c2w,
                                                                       int32_t *__restrict__ counts) {
    __shared__ int s_w[PP_THREADS / GG_WAVE];
    const int64_t n = (int64_t)P.F * P.H * P.W;
    const int64_t p0 = (int64_t)blockIdx.x * PP_TILE + (int64_t)threadIdx.x * PP_ITEMS;
    int c = 0;
#pragma unroll
    for (int j = 0; j < PP_ITEMS; ++j) {
        double x, y, z;
        if (p0 + j < n && bp_point(P, depth, mask, intr, c2w, p0 + j, x, y, z)) ++c;
    }
    int total;
    pp_block_scan(c, s_w, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PP_THREADS) void backproject_emit_kernel(BpParams P, const double *__restrict__ depth,
                                                                      const uint8_t *__restrict__ mask,
                                                                      const uint8_t *__restrict__ rgb,
                                                                      const double *__restrict__ intr,
                                                                      const double *__restrict__ c2w,
                                                                      const int32_t *__restrict__ offsets,
                                                                      double *__restrict__ points,
                                                                      uint8_t *__restrict__ colors) {
    __shared__ int s_w[PP_THREADS / GG_WAVE];
    const int64_t n = (int64_t)P.F * P.H * P.W;
    const int64_t p0 = (int64_t)blockIdx.x * PP_TILE + (int64_t)threadIdx.x * PP_ITEMS;
    double x[PP_ITEMS], y[PP_ITEMS], z[PP_ITEMS];
    bool k[PP_ITEMS];
    int c = 0;
#pragma unroll
    for (int j = 0; j < PP_ITEMS; ++j) {
        k[j] = p0 + j < n && bp_point(P, depth, mask, intr, c2w, p0 + j, x[j], y[j], z[j]);
        c += k[j] ? 1 : 0;
    }
    int total;
    int64_t o = (int64_t)offsets[blockIdx.x] + pp_block_scan(c, s_w, total);
#pragma unroll
    for (int j = 0; j < PP_ITEMS; ++j) {
        if (!k[j]) continue;
        const int64_t p = p0 + j;
        points[3 * o] = x[j];
        points[3 * o + 1] = y[j];
        points[3 * o + 2] = z[j];
        colors[3 * o] = rgb[3 * p];
        colors[3 * o + 1] = rgb[3 * p + 1];
        colors[3 * o + 2] = rgb[3 * p + 2];
        ++o;
    }
}

static int64_t bp_tiles(int F, int H, int W) { return ((int64_t)F * H * W + PP_TILE - 1) / PP_TILE; }

static size_t bp_layout(int F, int H, int W, int32_t **counts, int32_t **offsets, char *base) {
    const int64_t nb = bp_tiles(F, H, W);
    GgCarve cv{base, 0};
    int32_t *c = (int32_t *)cv.take((size_t)nb * 4);
    int32_t *o = (int32_t *)cv.take((size_t)nb * 4);
    if (counts) *counts = c;
    if (offsets) *offsets = o;
    return cv.off;
}

static bool bp_shape_ok(int F, int H, int W) {
    return F >= 0 && H >= 1 && W >= 1 && (int64_t)F * H * W <= GG_PREP_MAX_ROWS;
}

extern "C" size_t gg_backproject_workspace(int num_frames, int height, int width) {
    if (!bp_shape_ok(num_frames, height, width)) return 0;
    return bp_layout(num_frames, height, width, nullptr, nullptr, nullptr);
}

extern "C" int gg_backproject(int num_frames, int height, int width, const double *depth, const uint8_t *mask,
                              const uint8_t *rgb, const double *intrinsics, const double *c2w, double d_lo,
                              double d_hi, double z_lo, double z_hi, double *points, uint8_t *colors,
                              int64_t *count, void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(bp_shape_ok(num_frames, height, width),
               "need num_frames >= 0, height >= 1, width >= 1, frames x height x width <= GG_PREP_MAX_ROWS");
    GG_REQUIRE(!isnan(d_lo) && !isnan(d_hi) && !isnan(z_lo) && !isnan(z_hi), "a range bound is NaN");
    GG_REQUIRE(count, "null pointer: count");
    GG_REQUIRE(num_frames == 0 || (depth && mask && rgb && intrinsics && c2w && points && colors),
               "null pointer: frames / outputs");
    GG_REQUIRE(((uintptr_t)depth & 7) == 0 && ((uintptr_t)intrinsics & 7) == 0 && ((uintptr_t)c2w & 7) == 0 &&
                   ((uintptr_t)points & 7) == 0 && ((uintptr_t)count & 7) == 0,
               "depth / intrinsics / c2w / points / count misaligned");
    const size_t need = bp_layout(num_frames, height, width, nullptr, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    int32_t *counts, *offsets;
    bp_layout(num_frames, height, width, &counts, &offsets, (char *)ws);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = bp_tiles(num_frames, height, width);
    const BpParams P{num_frames, height, width, d_lo, d_hi, z_lo, z_hi};
    gg_prof_begin(GG_K_BACKPROJECT, s);
    if (nb > 0) {
        hipLaunchKernelGGL(backproject_count_kernel, dim3((unsigned)nb), dim3(PP_THREADS), 0, s, P, depth, mask,
                           intrinsics, c2w, counts);
    }
    hipLaunchKernelGGL(pp_scan_single_kernel, dim3(1), dim3(PP_THREADS), 0, s, counts, (int)nb, offsets, count);
    if (nb > 0) {
        hipLaunchKernelGGL(backproject_emit_kernel, dim3((unsigned)nb), dim3(PP_THREADS), 0, s, P, depth, mask, rgb,
                           intrinsics, c2w, offsets, points, colors);
    }
    gg_prof_end(GG_K_BACKPROJECT, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// subsample: exactly m = num / keep distinct rows, those with the m smallest SplitMix64 keys of (seed, index),
// emitted in ascending index order.  The key of row i is splitmix64(seed + (i + 1) * golden); the mix is a
// bijection of 2^64 and golden is odd, so no two rows share a key and "the m smallest" is one set.  The m-th
// smallest key is found by a 4-digit radix select (16-bit digits, integer histograms), then rows with key <= it
// are compacted in order.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t pp_key(uint64_t seed, int64_t i) {
    uint64_t z = seed + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct SelState {
    uint64_t prefix;             // digits chosen so far
    int64_t rem;                 // rank (1-based) of the wanted key among keys with that prefix
};

__global__ __launch_bounds__(PP_THREADS) void subsample_hist_kernel(int64_t num, uint64_t seed, int pass,
                                                                    const SelState *__restrict__ st,
                                                                    uint32_t *__restrict__ hist) {
    const int64_t i = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x;
    if (i >= num) return;
    const uint64_t key = pp_key(seed, i);
    const int sh = 48 - 16 * pass;
    if (pass > 0 && (key >> (sh + 16)) != st->prefix) return;
    atomicAdd(&hist[(key >> sh) & 0xffffu], 1u);
}

// One workgroup: the digit whose bin holds the rem-th key; the histogram is zeroed for the next pass.
__global__ __launch_bounds__(PP_THREADS) void subsample_pick_kernel(int pass, int64_t m, SelState *__restrict__ st,
                                                                    uint32_t *__restrict__ hist) {
    __shared__ int s_w[PP_THREADS / GG_WAVE];
    const int64_t rem = pass == 0 ? m : st->rem;           // written by the previous launch
    const uint64_t prefix = pass == 0 ? 0ull : st->prefix;
    const int per = PP_SEL_BINS / PP_THREADS;    // 256 consecutive bins per lane
    int64_t mine = 0;
    for (int b = 0; b < per; ++b) mine += hist[threadIdx.x * per + b];
    // bins sum to at most 2^31: an int scan is exact
    int total;
    const int64_t before = pp_block_scan((int)mine, s_w, total);
    if (before < rem && rem <= before + mine) {
        int64_t c = before;
        for (int b = 0; b < per; ++b) {
            const int64_t h = hist[threadIdx.x * per + b];
            if (rem <= c + h) {
                st->prefix = (prefix << 16) | (uint64_t)(threadIdx.x * per + b);
                st->rem = rem - c;
                break;
            }
            c += h;
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < PP_SEL_BINS; b += PP_THREADS) hist[b] = 0u;
}

__global__ __launch_bounds__(PP_THREADS) void subsample_count_kernel(int64_t num, uint64_t seed,
                                                                     const SelState *__restrict__ st,
                                                                     int32_t *__restrict__ counts) {
    __shared__ int s_w[PP_THREADS / GG_WAVE];
    const uint64_t t = st->prefix;
    const int64_t i0 = (int64_t)blockIdx.x * PP_TILE + (int64_t)threadIdx.x * PP_ITEMS;
    int c = 0;
#pragma unroll
    for (int j = 0; j < PP_ITEMS; ++j) c += (i0 + j < num && pp_key(seed, i0 + j) <= t) ? 1 : 0;
    int total;
    pp_block_scan(c, s_w, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PP_THREADS) void subsample_emit_kernel(int64_t num, int64_t m, uint64_t seed,
                                                                    const SelState *__restrict__ st,
                                                                    const int32_t *__restrict__ offsets,
                                                                    const double *__restrict__ points,
                                                                    const uint8_t *__restrict__ colors,
                                                                    double *__restrict__ out_points,
                                                                    uint8_t *__restrict__ out_colors,
                                                                    int64_t *__restrict__ out_index) {
    __shared__ int s_w[PP_THREADS / GG_WAVE];
    const uint64_t t = st->prefix;
    const int64_t i0 = (int64_t)blockIdx.x * PP_TILE + (int64_t)threadIdx.x * PP_ITEMS;
    bool k[PP_ITEMS];
    int c = 0;
#pragma unroll
    for (int j = 0; j < PP_ITEMS; ++j) {
        k[j] = i0 + j < num && pp_key(seed, i0 + j) <= t;
        c += k[j] ? 1 : 0;
    }
    int total;
    int64_t o = (int64_t)offsets[blockIdx.x] + pp_block_scan(c, s_w, total);
#pragma unroll
    for (int j = 0; j < PP_ITEMS; ++j) {
        if (!k[j] || o >= m) continue;      // exactly m rows pass the key test; the bound only guards the buffers
        const int64_t i = i0 + j;
        out_index[o] = i;
        if (out_points) {
            out_points[3 * o] = points[3 * i];
            out_points[3 * o + 1] = points[3 * i + 1];
            out_points[3 * o + 2] = points[3 * i + 2];
        }
        if (out_colors) {
            out_colors[3 * o] = colors[3 * i];
            out_colors[3 * o + 1] = colors[3 * i + 1];
            out_colors[3 * o + 2] = colors[3 * i + 2];
        }
        ++o;
    }
}

static size_t ss_layout(int64_t num, SelState **st, uint32_t **hist, int32_t **counts, int32_t **offsets,
                        int64_t **total, char *base) {
    const int64_t nb = (num + PP_TILE - 1) / PP_TILE;
    GgCarve cv{base, 0};
    SelState *a = (SelState *)cv.take(sizeof(SelState));
    uint32_t *h = (uint32_t *)cv.take((size_t)PP_SEL_BINS * 4);
    int32_t *c = (int32_t *)cv.take((size_t)nb * 4);
    int32_t *o = (int32_t *)cv.take((size_t)nb * 4);
    int64_t *t = (int64_t *)cv.take(8);
    if (st) *st = a;
    if (hist) *hist = h;
    if (counts) *counts = c;
    if (offsets) *offsets = o;
    if (total) *total = t;
    return cv.off;
}

extern "C" size_t gg_subsample_workspace(int64_t num) {
    if (num < 0 || num > GG_PREP_MAX_ROWS) return 0;
    return ss_layout(num, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int gg_subsample(int64_t num, int64_t keep, uint64_t seed, const double *points, const uint8_t *colors,
                            double *out_points, uint8_t *out_colors, int64_t *out_index, void *ws, size_t ws_bytes,
                            gg_stream_t stream) {
    GG_REQUIRE(num >= 0 && num <= GG_PREP_MAX_ROWS, "need 0 <= num <= GG_PREP_MAX_ROWS");
    GG_REQUIRE(keep >= 1, "keep < 1");
    const int64_t m = num / keep;
    if (m == 0) return GG_OK;
    GG_REQUIRE(out_index, "null pointer: out_index");
    GG_REQUIRE(!out_points || points, "out_points needs points");
    GG_REQUIRE(!out_colors || colors, "out_colors needs colors");
    GG_REQUIRE(((uintptr_t)points & 7) == 0 && ((uintptr_t)out_points & 7) == 0 && ((uintptr_t)out_index & 7) == 0,
               "points / out_points / out_index misaligned");
    const size_t need = ss_layout(num, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    SelState *st;
    uint32_t *hist;
    int32_t *counts, *offsets;
    int64_t *total;
    ss_layout(num, &st, &hist, &counts, &offsets, &total, (char *)ws);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (num + PP_TILE - 1) / PP_TILE;
    const unsigned rows_blocks = (unsigned)((num + PP_THREADS - 1) / PP_THREADS);
    gg_prof_begin(GG_K_SUBSAMPLE, s);
    GG_REQUIRE_FILL(GG_K_SUBSAMPLE, s, gg_fill_async(hist, 0, (size_t)PP_SEL_BINS * 4, s));
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(subsample_hist_kernel, dim3(rows_blocks), dim3(PP_THREADS), 0, s, num, (unsigned long long)seed,
                           pass, st, hist);
        hipLaunchKernelGGL(subsample_pick_kernel, dim3(1), dim3(PP_THREADS), 0, s, pass, m, st, hist);
    }
    hipLaunchKernelGGL(subsample_count_kernel, dim3((unsigned)nb), dim3(PP_THREADS), 0, s, num, (unsigned long long)seed,
                       st, counts);
    hipLaunchKernelGGL(pp_scan_single_kernel, dim3(1), dim3(PP_THREADS), 0, s, counts, (int)nb, offsets, total);
    hipLaunchKernelGGL(subsample_emit_kernel, dim3((unsigned)nb), dim3(PP_THREADS), 0, s, num, m, (unsigned long long)seed,
                       st, offsets, points, colors, out_points, out_colors, out_index);
    gg_prof_end(GG_K_SUBSAMPLE, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// depth -> world-frame normal maps (cal_normal, generate_data.py:204-229), fp64, one lane per pixel
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double nm_depth(const double *__restrict__ d, int64_t i) {
    const double x = d[i];
    return x < 0.01 ? 1e-5 : x;
}

__global__ __launch_bounds__(256) void depth_normals_kernel(int F, int H, int W, const double *__restrict__ depth,
                                                            const double *__restrict__ intr,
                                                            const double *__restrict__ c2w,
                                                            double *__restrict__ out) {
    const int64_t hw = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)F * hw) return;
    const int f = (int)(p / hw);
    const int64_t r = p - (int64_t)f * hw;
    const int v = (int)(r / W), u = (int)(r - (int64_t)v * W);
    const double *D = depth + (int64_t)f * hw;
    // np.gradient, edge_order 1: interior (f[i+1] - f[i-1]) / 2, edges one-sided (/ 1, exact)
    double gu, gv;
    const int64_t row = (int64_t)v * W;
    if (u == 0)
        gu = nm_depth(D, row + 1) - nm_depth(D, row);
    else if (u == W - 1)
        gu = nm_depth(D, row + u) - nm_depth(D, row + u - 1);
    else
        gu = (nm_depth(D, row + u + 1) - nm_depth(D, row + u - 1)) / 2.0;
    if (v == 0)
        gv = nm_depth(D, W + u) - nm_depth(D, u);
    else if (v == H - 1)
        gv = nm_depth(D, row + u) - nm_depth(D, row - W + u);
    else
        gv = (nm_depth(D, row + W + u) - nm_depth(D, row - W + u)) / 2.0;
    const double d = nm_depth(D, row + u);
    const double *K = intr + 4 * (size_t)f;
    const double a = -(gu * (K[0] / d)), b = -(gv * (K[1] / d)), c = 1.0;
    const double nrm = sqrt((a * a + b * b) + c * c);
    double n0 = a / nrm, n1 = b / nrm, n2 = c / nrm;
    if (!(isfinite(n0) && isfinite(n1) && isfinite(n2))) {
        n0 = 0.0;
        n1 = 0.0;
        n2 = 1.0;
    }
    const double *T = c2w + 16 * (size_t)f;
    double *o = out + 3 * p;
    o[0] = (T[0] * n0 + T[1] * n1) + T[2] * n2;
    o[1] = (T[4] * n0 + T[5] * n1) + T[6] * n2;
    o[2] = (T[8] * n0 + T[9] * n1) + T[10] * n2;
}

extern "C" int gg_depth_normals(int num_frames, int height, int width, const double *depth, const double *intrinsics,
                                const double *c2w, double *normals, gg_stream_t stream) {
    GG_REQUIRE(num_frames >= 0 && height >= 2 && width >= 2 &&
                   (int64_t)num_frames * height * width <= GG_PREP_MAX_ROWS,
               "need num_frames >= 0, height >= 2, width >= 2, frames x height x width <= GG_PREP_MAX_ROWS");
    if (num_frames == 0) return GG_OK;
    GG_REQUIRE(depth && intrinsics && c2w && normals, "null pointer");
    GG_REQUIRE(((uintptr_t)depth & 7) == 0 && ((uintptr_t)intrinsics & 7) == 0 && ((uintptr_t)c2w & 7) == 0 &&
                   ((uintptr_t)normals & 7) == 0,
               "depth / intrinsics / c2w / normals misaligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)num_frames * height * width;
    gg_prof_begin(GG_K_NORMALS, s);
    hipLaunchKernelGGL(depth_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, num_frames, height,
                       width, depth, intrinsics, c2w, normals);
    gg_prof_end(GG_K_NORMALS, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
