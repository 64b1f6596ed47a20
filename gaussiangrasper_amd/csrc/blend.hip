// blend.hip — C ABI of the alpha-blending step and the record-packing kernel.
// The blend kernels themselves live in blend2.hip (their design notes are in its header and in
// DESIGN.md §3.4-3.5).
#include <stdlib.h>

#include "blend_launch.h"

// ---------------------------------------------------------------------------------------------
// prep: pack xys / conics / opacity into 32-byte records (one gather per list entry later)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void blend_prep_kernel(int N, const float *__restrict__ xys,
                                                         const float *__restrict__ conics,
                                                         const float *__restrict__ opacity,
                                                         GRec *__restrict__ rec) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    grec_pack(xys[2 * (size_t)i], xys[2 * (size_t)i + 1], opacity[i], conics[3 * (size_t)i], conics[3 * (size_t)i + 1],
              conics[3 * (size_t)i + 2], rec + i);
}

extern "C" size_t gg_blend_workspace(int num_points) {
    return gg_align_up(sizeof(GRec) * (size_t)(num_points > 0 ? num_points : 1), 256);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
size_t gg_sort_pairs_workspace(int64_t n);   // binning.hip: stable LSD radix sort of (key, value) pairs
int gg_sort_pairs(int64_t n, uint32_t *keys, uint32_t *vals, int bits, void *ws, size_t ws_bytes, hipStream_t s);

// GG_REQUIRE under the name of the public entry (`entry`) instead of the helper's __func__
#define BLEND_REQUIRE(cond, msg)                 \
    do {                                         \
        if (!(cond)) {                           \
            gg_set_error("%s: %s", entry, msg);  \
            return GG_ERR_INVALID_ARG;           \
        }                                        \
    } while (0)

// Channel chunking: calls with <= 3 channels (rgb / depth / normal) use the narrow kernels with
// the colours inside the LDS record; anything wider is processed in chunks of 32 channels on the
// MFMA kernels (a final partial chunk is zero-padded), each chunk re-walking the tile lists.
// (A 64-channel-per-walk variant — two 32-column MFMA blocks, V_OUT operands streamed per flush —
// was built and measured: 231 VGPRs / occupancy 2 backward, 143 registers forward; the fused
// 39-channel call ran at 98 views/s against 122 with two 32-channel walks, so it was dropped.)
// 4..8 remaining channels (the rgb | depth | normal tail of a fused call) go to the 8-wide narrow
// kernels: on the wide kernels such a tail cost as much as a full 32-channel chunk.
static int chunk_width(int remaining) { return remaining <= 3 ? remaining : remaining <= 8 ? 8 : 32; }
// Defaults (tools/fwdblocks_bench.py, 5 M Gaussians, 1920x1080, 128 + 7 channels, forward kernels per view): pair walk of
// one block + one walk of the other three 1.51 ms (three waves per SIMD, 147 registers); all four blocks in the pair walk
// 1.50 (two waves, 201 registers); 2 + 2 1.74; one block per walk 2.0-2.2.  The headline's 32-channel array is one block.
#ifndef GG_FWD_BLOCKS_PAIR
#define GG_FWD_BLOCKS_PAIR 1
#endif
#ifndef GG_FWD_BLOCKS_CHUNK
#define GG_FWD_BLOCKS_CHUNK 3
#endif

// Forward walks over several 32-channel blocks at once (csrc/blend2.hip, NCB; r03): how many blocks the pair walk and
// the walks of the remaining chunks of a wide first array take.  Tuning entry (tools/): returns the previous pair value.
static int g_fwd_blocks_pair = GG_FWD_BLOCKS_PAIR, g_fwd_blocks_chunk = GG_FWD_BLOCKS_CHUNK;
extern "C" int gg_debug_set_fwd_blocks(int pair_blocks, int chunk_blocks) {
    const int prev = g_fwd_blocks_pair;
    g_fwd_blocks_pair = pair_blocks == 4 ? 4 : (pair_blocks == 2 ? 2 : 1);
    g_fwd_blocks_chunk = chunk_blocks >= 2 && chunk_blocks <= 4 ? chunk_blocks : 1;
    return prev;
}

// The chunk plan: f(chunk, index) for every walk of channels [off0, C), in launch order.  max_blocks > 1 (forward
// walks with 16-byte aligned rows) lets a walk take up to that many full 32-channel blocks; the backward walks, and
// with them the deterministic slab's columns (det_chunks), take one chunk each.
template <typename F>
static void for_each_chunk(int C, int off0, int max_blocks, F &&f) {
    int index = 0;
    for (int off = off0; off < C; ++index) {
        const int blocks = off % 4 == 0 ? min((C - off) / 32, max_blocks) : 1;
        const int w = blocks >= 2 ? 32 : chunk_width(C - off);
        const BlendChunk ch = {off, w, min(w, C - off), blocks >= 2 ? blocks : 1};
        f(ch, index);
        off += ch.n * ch.blocks;
    }
}
static bool rows_aligned16(int C, const void *rows) { return C % 4 == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0; }

// What every blend entry is handed besides its colour arrays and outputs.
struct BlendCall {
    int N, img_h, img_w;
    const int32_t *ids, *tile_bins;
    const float *xys, *conics, *opacity;
    void *ws;
    size_t ws_bytes;
    gg_stream_t stream;
};
// The prologue of every entry: validate, check the workspace, pack the records unless the workspace holds them
// already (records_ready: gg_blend_fwd_pair_packed, GG_BWD_WS_FROM_FORWARD), compute the tile grid, fill the walk.
// ptrs_always / ptrs_points: the entry's own pointers that must be set whatever N is / when N > 0.  A backward
// entry has nothing to do for N == 0: the prologue returns GG_OK before it looks at pointers, and the entry returns.
static int blend_begin(const char *entry, const BlendCall &c, bool backward, bool ptrs_always, bool ptrs_points,
                       bool records_ready, BlendWalk &w) {
    BLEND_REQUIRE(c.N >= 0, "num_points < 0");
    BLEND_REQUIRE(c.img_h > 0 && c.img_w > 0, "empty image");
    if (backward && c.N == 0) return GG_OK;
    BLEND_REQUIRE(c.tile_bins && ptrs_always, "null pointer");
    BLEND_REQUIRE(c.N == 0 || (c.ids && ptrs_points), "null pointer");
    if (c.ws == nullptr || c.ws_bytes < gg_blend_workspace(c.N)) {
        gg_set_error("%s: workspace too small", entry);
        return GG_ERR_WORKSPACE;
    }
    // the kernels read a packed record as two float4 (blend2.hip, votes.hip, hits.hip)
    BLEND_REQUIRE((reinterpret_cast<uintptr_t>(c.ws) & 15) == 0, "ws must be 16-byte aligned");
    w.s = (hipStream_t)c.stream;
    if (c.N > 0 && !records_ready) {
        gg_prof_begin(GG_K_BLEND_PREP, w.s);
        hipLaunchKernelGGL(blend_prep_kernel, dim3((c.N + 255) / 256), dim3(256), 0, w.s, c.N, c.xys, c.conics,
                           c.opacity, (GRec *)c.ws);
        gg_prof_end(GG_K_BLEND_PREP, w.s);
    }
    w.img_h = c.img_h;
    w.img_w = c.img_w;
    w.tiles_x = (c.img_w + GG_BLOCK - 1) / GG_BLOCK;
    w.ntiles = w.tiles_x * ((c.img_h + GG_BLOCK - 1) / GG_BLOCK);
    w.ids = c.ids;
    w.bins = c.tile_bins;
    w.rec = (const GRec *)c.ws;
    return GG_OK;
}

// the forward walks of channels [off0, C) of `src`: as many 32-channel blocks per walk as the policy allows (16-byte
// aligned rows), then the usual chunks; the first of them writes final_Ts / final_idx when asked to
static void fwd_chunks(const BlendWalk &w, const BlendColors &src, int off0, const BlendFwdOut &out,
                       bool first_writes_final) {
    const int max_blocks = rows_aligned16(src.C, out.out_img) ? g_fwd_blocks_chunk : 1;
    for_each_chunk(src.C, off0, max_blocks, [&](const BlendChunk &ch, int index) {
        gg_prof_begin(GG_K_BLEND_FWD + gg_width_index(ch.width), w.s);
        gg_launch_blend2_fwd(w, src, ch, out, first_writes_final && index == 0);
        gg_prof_end(GG_K_BLEND_FWD + gg_width_index(ch.width), w.s);
    });
}

#ifdef GG_ABLATION
// Measurement build only (libgg_raster_abl.so, tools/kbench.py): level > 0 makes the backward run an
// ABLATED kernel (wrong results) so its time can be attributed.  Not declared in gg_raster.h, not
// compiled into libgg_raster.so.
static int g_ablate = 0;
extern "C" int gg_debug_set_ablation(int level) {
    int prev = g_ablate;
    g_ablate = level;
    return prev;
}
#endif

extern "C" int gg_blend_fwd(int C, int N, int img_h, int img_w, const int32_t *ids,
                            const int32_t *tile_bins, const float *xys, const float *conics,
                            const float *colors, const float *opacity, const float *background,
                            float *out_img, float *final_Ts, int32_t *final_idx, void *ws,
                            size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(C >= 1, "channels < 1");
    BlendWalk w;
    const int rc = blend_begin(__func__, {N, img_h, img_w, ids, tile_bins, xys, conics, opacity, ws, ws_bytes, stream},
                               false, background && out_img && final_Ts && final_idx,
                               xys && conics && colors && opacity, false, w);
    if (rc != GG_OK) return rc;
    fwd_chunks(w, {C, colors, background}, 0, {out_img, final_Ts, final_idx}, true);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// first array (>= 32 channels) and second array (<= 8) of the pair entries
struct BlendPairIn {
    BlendColors src, src2;
};

static int blend_fwd_pair_impl(const char *entry, const BlendCall &c, const BlendPairIn &in, const BlendFwdOut &out,
                               float *out_img2, bool fast, bool records_ready) {
    const int C = in.src.C, C2 = in.src2.C, N = c.N;
    BLEND_REQUIRE(C >= 32, "the first colour array needs >= 32 channels (its first chunk carries the second array)");
    BLEND_REQUIRE(C2 >= 1 && C2 <= 8, "the second colour array has 1..8 channels");
    BlendWalk w;
    const int rc = blend_begin(entry, c, false,
                               in.src.background && in.src2.background && out.out_img && out_img2 && out.final_Ts &&
                                   out.final_idx,
                               in.src.colors && in.src2.colors && (records_ready || (c.xys && c.conics && c.opacity)),
                               records_ready, w);
    if (rc != GG_OK) return rc;
    // the batched kernel (fp32-grade images, not the exact summation order) needs 16-byte aligned image rows; without
    // them the exact-order kernel runs (its scalar-store epilogue takes any layout)
    // ... and reads the colour rows through buffer descriptors with 32-bit offsets (id x row bytes as a 24-bit multiply)
    const uint64_t bytes1 = (uint64_t)(N > 0 ? N : 1) * (uint64_t)C * 4u, bytes2 = (uint64_t)(N > 0 ? N : 1) * (uint64_t)C2 * 4u;
    const bool aligned = rows_aligned16(C, out.out_img);
    fast = fast && aligned && ((reinterpret_cast<uintptr_t>(in.src.background) & 15) == 0) && N < (1 << 24) &&
           C < (1 << 20) && bytes1 < ((uint64_t)1 << 32) && bytes2 < ((uint64_t)1 << 32);
    // the pair walk takes 1, 2 or 4 blocks of the first array (aligned rows)
    int pair_blocks = 1;
    if (!fast && aligned) {
        if (g_fwd_blocks_pair >= 4 && C >= 128) pair_blocks = 4;
        else if (g_fwd_blocks_pair >= 2 && C >= 64) pair_blocks = 2;
    }
    gg_prof_begin(GG_K_BLEND_FWD_PAIR, w.s);
    gg_launch_blend2_fwd_pair(w, in.src, in.src2, out, out_img2, pair_blocks, fast, (unsigned)bytes1, (unsigned)bytes2);
    gg_prof_end(GG_K_BLEND_FWD_PAIR, w.s);
    fwd_chunks(w, in.src, 32 * pair_blocks, out, false);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_blend_fwd_pair(int C, int C2, int N, int img_h, int img_w, const int32_t *ids,
                                 const int32_t *tile_bins, const float *xys, const float *conics,
                                 const float *colors, const float *colors2, const float *opacity,
                                 const float *background, const float *background2, float *out_img,
                                 float *out_img2, float *final_Ts, int32_t *final_idx, void *ws,
                                 size_t ws_bytes, gg_stream_t stream) {
    return blend_fwd_pair_impl(__func__, {N, img_h, img_w, ids, tile_bins, xys, conics, opacity, ws, ws_bytes, stream},
                               {{C, colors, background}, {C2, colors2, background2}}, {out_img, final_Ts, final_idx},
                               out_img2, false, false);
}

extern "C" int gg_blend_fwd_pair_fast(int C, int C2, int N, int img_h, int img_w, const int32_t *ids,
                                      const int32_t *tile_bins, const float *xys, const float *conics,
                                      const float *colors, const float *colors2, const float *opacity,
                                      const float *background, const float *background2, float *out_img,
                                      float *out_img2, float *final_Ts, int32_t *final_idx, void *ws,
                                      size_t ws_bytes, gg_stream_t stream) {
    return blend_fwd_pair_impl(__func__, {N, img_h, img_w, ids, tile_bins, xys, conics, opacity, ws, ws_bytes, stream},
                               {{C, colors, background}, {C2, colors2, background2}}, {out_img, final_Ts, final_idx},
                               out_img2, true, false);
}

// gg_blend_fwd_pair / gg_blend_fwd_pair_fast on a workspace that ALREADY holds the packed records of these Gaussians
// (gg_view_fwd's `records` output, or an earlier forward over the same xys / conics / opacity): no packing pass
extern "C" int gg_blend_fwd_pair_packed(int C, int C2, int N, int img_h, int img_w, const int32_t *ids,
                                        const int32_t *tile_bins, const float *colors, const float *colors2,
                                        const float *background, const float *background2, float *out_img,
                                        float *out_img2, float *final_Ts, int32_t *final_idx, void *ws,
                                        size_t ws_bytes, int fast, gg_stream_t stream) {
    return blend_fwd_pair_impl(__func__, {N, img_h, img_w, ids, tile_bins, nullptr, nullptr, nullptr, ws, ws_bytes, stream},
                               {{C, colors, background}, {C2, colors2, background2}}, {out_img, final_Ts, final_idx},
                               out_img2, fast != 0, true);
}

// gg_blend_votes: the per-Gaussian sums of the forward walk's blend weights by pixel label (kernel: votes.hip)
extern "C" int gg_blend_votes(int num_labels, int N, int img_h, int img_w, const int32_t *ids, const int32_t *tile_bins,
                              const float *xys, const float *conics, const float *opacity, const uint8_t *labels,
                              int64_t *votes, void *ws, size_t ws_bytes, int ws_packed, gg_stream_t stream) {
    GG_REQUIRE(num_labels >= 1 && num_labels <= 255, "num_labels must be 1..255");
    GG_REQUIRE(labels != nullptr, "labels is null");
    GG_REQUIRE(N == 0 || votes != nullptr, "votes is null");
    GG_REQUIRE((reinterpret_cast<uintptr_t>(votes) & 7) == 0, "votes must be 8-byte aligned");
    GG_REQUIRE(N <= 0 || ids != nullptr, "gaussian_ids_sorted is null");
    GG_REQUIRE(tile_bins != nullptr, "tile_bins is null");
    GG_REQUIRE(N <= 0 || ws_packed != 0 || (xys && conics && opacity), "xys, conics or opacity is null");
    BlendWalk w;
    const int rc = blend_begin(__func__, {N, img_h, img_w, ids, tile_bins, xys, conics, opacity, ws, ws_bytes, stream},
                               false, true, true, ws_packed != 0, w);
    if (rc != GG_OK || N == 0) return rc;
    gg_prof_begin(GG_K_BLEND_VOTES, w.s);
    gg_launch_blend_votes(w, num_labels, N, labels, votes);
    gg_prof_end(GG_K_BLEND_VOTES, w.s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// gg_blend_hits: what the forward walk finds under every pixel (kernel: hits.hip).  No profiling id: the ids of the
// forward's range are taken, so tools/hits_bench.py times the call with device events.
extern "C" int gg_blend_hits(int N, int img_h, int img_w, const int32_t *ids, const int32_t *tile_bins, const float *xys,
                             const float *conics, const float *opacity, float t_hit, int32_t *hit_idx, int32_t *top_idx,
                             float *top_vis, int32_t *count, void *ws, size_t ws_bytes, int ws_packed,
                             gg_stream_t stream) {
    auto misaligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; };
    GG_REQUIRE(N >= 0, "num_points < 0");
    GG_REQUIRE(img_h > 0 && img_w > 0, "img_height and img_width must be > 0");
    GG_REQUIRE(t_hit > GG_T_EPS && t_hit < 1.0f, "t_hit must be in (1e-4, 1)");   // NaN fails
    GG_REQUIRE(hit_idx != nullptr, "hit_idx is null");
    GG_REQUIRE((top_idx != nullptr) == (top_vis != nullptr) && (top_idx != nullptr) == (count != nullptr),
               "top_idx, top_vis and count are given together or not at all");
    GG_REQUIRE(!misaligned(hit_idx), "hit_idx must be 4-byte aligned");
    GG_REQUIRE(!misaligned(top_idx), "top_idx must be 4-byte aligned");
    GG_REQUIRE(!misaligned(top_vis), "top_vis must be 4-byte aligned");
    GG_REQUIRE(!misaligned(count), "count must be 4-byte aligned");
    GG_REQUIRE(N == 0 || ids != nullptr, "gaussian_ids_sorted is null");
    GG_REQUIRE(tile_bins != nullptr, "tile_bins is null");
    GG_REQUIRE(N == 0 || ws_packed != 0 || (xys && conics && opacity), "xys, conics or opacity is null");
    BlendWalk w;
    const int rc = blend_begin(__func__, {N, img_h, img_w, ids, tile_bins, xys, conics, opacity, ws, ws_bytes, stream},
                               false, true, true, ws_packed != 0, w);
    if (rc != GG_OK) return rc;
    gg_launch_blend_hits(w, N, t_hit, hit_idx, top_idx, top_vis, count);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ---------------------------------------------------------------------------------------------
// deterministic backward: slab of per-(list entry, quadrant) totals + ordered per-Gaussian sums
// ---------------------------------------------------------------------------------------------
struct DetWs {
    float *slab;              // I * 4 * ks
    uint32_t *keys, *vals;    // I each: Gaussian id / list entry, sorted by id (stable: entries ascend)
    int32_t *seg;             // 2 N: [first, last) of each Gaussian's run in keys
    void *sort_ws;
    size_t sort_bytes, bytes;
};
static int det_chunks(int C) {   // the backward walks of C channels: bwd_chunks launches exactly these
    int nc = 0;
    for_each_chunk(C, 0, 1, [&](const BlendChunk &, int) { ++nc; });
    return nc;
}
static DetWs det_ws_layout(void *ws, int N, int C, int64_t I) {
    DetWs w;
    size_t off = 0;
    auto take = [&](size_t nbytes) {
        char *p = ws ? (char *)ws + off : nullptr;
        off += gg_align_up(nbytes, 256);
        return (void *)p;
    };
    const size_t i = (size_t)(I > 0 ? I : 1), n = (size_t)(N > 0 ? N : 1);
    const size_t ks = (size_t)C + 6 * (size_t)det_chunks(C);
    w.slab = (float *)take(sizeof(float) * 4 * ks * i);
    w.keys = (uint32_t *)take(4 * i);
    w.vals = (uint32_t *)take(4 * i);
    w.seg = (int32_t *)take(8 * n);
    w.sort_bytes = gg_sort_pairs_workspace((int64_t)i);
    w.sort_ws = take(w.sort_bytes);
    w.bytes = off;
    return w;
}
extern "C" size_t gg_blend_bwd_deterministic_workspace(int num_points, int channels, int64_t num_intersects) {
    if (channels < 1) return 0;
    return det_ws_layout(nullptr, num_points, channels, num_intersects).bytes;
}

__global__ void det_pairs_kernel(int64_t I, const int32_t *__restrict__ ids, uint32_t *__restrict__ keys,
                                 uint32_t *__restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= I) return;
    keys[e] = (uint32_t)ids[e];
    vals[e] = (uint32_t)e;
}
__global__ void det_edges_kernel(int64_t I, int N, const uint32_t *__restrict__ keys, int32_t *__restrict__ seg) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= I) return;
    const uint32_t k = keys[e];
    if (k >= (uint32_t)N) return;
    if (e == 0 || keys[e - 1] != k) seg[2 * (size_t)k] = (int32_t)e;
    if (e == I - 1 || keys[e + 1] != k) seg[2 * (size_t)k + 1] = (int32_t)e + 1;
}
// One wave per Gaussian; lane l owns output column l (and l + 64, ...): colour channel c < C or geometry
// component m = column - C.  Every sum runs over the Gaussian's list entries in ascending order, quadrants
// 0..3 inside an entry and (geometry) channel chunks inside a quadrant: one fixed order, no atomics.
__global__ __launch_bounds__(256) void det_reduce_kernel(int N, int C, int nchunks, int ks,
                                                         const float *__restrict__ slab,
                                                         const uint32_t *__restrict__ vals,
                                                         const int32_t *__restrict__ seg, float *v_xy, float *v_conic,
                                                         float *v_colors, float *v_opacity, int gstride, int cstride) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= N) return;
    const int first = seg[2 * (size_t)g], last = seg[2 * (size_t)g + 1];
    if (last <= first) return;
    for (int col = lane; col < C + 6; col += 64) {
        float sum = 0.0f;
        const bool geom = col >= C;
        const int c0 = geom ? C + (col - C) : col;
        for (int r = first; r < last; ++r) {
            const float *row = slab + (size_t)vals[r] * 4 * ks;
            for (int w = 0; w < 4; ++w) {
                if (geom)
                    for (int c = 0; c < nchunks; ++c) sum += row[(size_t)w * ks + c0 + 6 * c];
                else
                    sum += row[(size_t)w * ks + c0];
            }
        }
        float *dst;
        if (!geom) dst = v_colors + (size_t)g * (cstride ? cstride : C) + col;
        else {
            const int m = col - C;
            if (m < 2) dst = v_xy + (size_t)g * (gstride ? gstride : 2) + m;
            else if (m < 5) dst = v_conic + (size_t)g * (gstride ? gstride : 3) + (m - 2);
            else dst = v_opacity + (size_t)g * (gstride ? gstride : 1);
        }
        *dst += sum;   // the arrays start at zero (or hold what earlier calls added: the accumulate flags)
    }
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
// The kernels accumulate with atomics, so the gradient arrays start at zero.  Which regions a call clears:
//   geometry   interleaved records {xy, conic, opacity[, colours | second array]} of gstride floats per Gaussian: the
//              whole records; dense: v_xy, v_conic, v_opacity.  GG_BWD_ACCUMULATE_GEOM (a later segment of a
//              multi-segment call): none — the geometry gradients, and colours inside the record, keep what the
//              earlier segments added.
//   colours    the (stride-padded) rows, unless GG_BWD_ACCUMULATE_COLORS is set or a single-array call has them inside
//              the record.  A pair call always clears its first array's rows.
//   second     the pair call's second array (g2), unless it lives inside the record.
// One fill covers everything when a single-array call laid dense arrays back to back: v_xy | v_conic | v_opacity |
// v_colors.  The order is the one the entries have always issued: a single-array call clears dense colours between
// v_conic and v_opacity, a pair call after the second array.
struct BlendFills {
    int count;
    struct {
        float *p;
        size_t floats;
    } f[5];
};
static int grad_zero_plan(const char *entry, const BlendGradOut &g, int C, const BlendGrad2 *g2, int C2, int flags,
                          size_t n, BlendFills &fills) {
    const bool acc_colors = (flags & GG_BWD_ACCUMULATE_COLORS) != 0, acc_geom = (flags & GG_BWD_ACCUMULATE_GEOM) != 0;
    const bool colors_in_record = !g2 && g.gstride > 0 && g.cstride == g.gstride && g.v_colors == g.v_xy + 6;
    const bool second_in_record = g2 && g.gstride > 0 && g2->cstride == g.gstride && g2->v_colors == g.v_xy + 6;
    BLEND_REQUIRE(g.gstride == 0 || g.gstride >= 6, "geom_stride must be 0 (dense) or >= 6");
    BLEND_REQUIRE(g.cstride == 0 || g.cstride >= C, "color_stride must be 0 (dense) or >= channels");
    BLEND_REQUIRE(!g2 || g2->cstride == 0 || g2->cstride >= C2, "color_stride2 must be 0 (dense) or >= channels2");
    BLEND_REQUIRE(!acc_colors || !colors_in_record,
                  "GG_BWD_ACCUMULATE_COLORS needs v_colors outside the interleaved geometry record");
    BLEND_REQUIRE(g.gstride == 0 || (g.v_conic == g.v_xy + 2 && g.v_opacity == g.v_xy + 5),
                  "interleaved geometry gradients: v_conic = v_xy + 2 and v_opacity = v_xy + 5 expected");
    BLEND_REQUIRE(!second_in_record || g.gstride >= 6 + C2, "the record is too short for the second array's gradients");
    fills.count = 0;
    auto add = [&](float *p, size_t floats) {
        fills.f[fills.count].p = p;
        fills.f[fills.count++].floats = floats;
    };
    const bool zero_colors = !acc_colors && !colors_in_record;
    const size_t crow = g.cstride ? g.cstride : C;
    if (!g2 && !acc_geom && zero_colors && g.gstride == 0 && g.cstride == 0 && g.v_conic == g.v_xy + 2 * n &&
        g.v_opacity == g.v_conic + 3 * n && g.v_colors == g.v_opacity + n) {
        add(g.v_xy, (6 + (size_t)C) * n);
        return GG_OK;
    }
    const bool colors_first = !g2 && !acc_geom && g.gstride == 0;   // ... before v_opacity
    if (!acc_geom) {
        if (g.gstride > 0) {
            add(g.v_xy, (size_t)g.gstride * n);
        } else {
            add(g.v_xy, 2 * n);
            add(g.v_conic, 3 * n);
            if (colors_first && zero_colors) add(g.v_colors, crow * n);
            add(g.v_opacity, n);
        }
    }
    if (g2 && !second_in_record) add(g2->v_colors, (size_t)(g2->cstride ? g2->cstride : C2) * n);
    if (!colors_first && zero_colors) add(g.v_colors, crow * n);
    return GG_OK;
}
static int zero_grads(const char *entry, const BlendGradOut &g, int C, const BlendGrad2 *g2, int C2, int flags, size_t n,
                      hipStream_t s) {
    BlendFills fills;
    const int rc = grad_zero_plan(entry, g, C, g2, C2, flags, n, fills);
    if (rc != GG_OK) return rc;
    bool fail = false;
    for (int k = 0; k < fills.count; ++k)
        fail |= gg_fill_async(fills.f[k].p, 0, sizeof(float) * fills.f[k].floats, s) != hipSuccess;
    if (fail) {
        gg_set_error("%s: memset failed", entry);
        return GG_ERR_LAUNCH;
    }
    return GG_OK;
}

// the backward walks of channels [off0, C) of `src`, one chunk each (the plan det_chunks counts), adding to `g` — or,
// with a slab (det.p), storing into the columns of their chunk
static void bwd_chunks(const BlendWalk &w, const BlendColors &src, int off0, const BlendBwdIn &in, const BlendGradOut &g,
                       DetSlab det) {
    for_each_chunk(src.C, off0, 1, [&](const BlendChunk &ch, int index) {
        det.coff = ch.off;
        det.goff = src.C + 6 * index;
        gg_prof_begin(GG_K_BLEND_BWD + gg_width_index(ch.width), w.s);
#ifdef GG_ABLATION
        if ((ch.width == 3 && g_ablate > 0 && g_ablate < 10) || (ch.width == 32 && ch.n == 32 && g_ablate > 10))
            gg_launch_blend2_bwd_ablate(g_ablate, w, src, ch, in, g);
        else
#endif
            gg_launch_blend2_bwd(w, src, ch, in, g, det);
        gg_prof_end(GG_K_BLEND_BWD + gg_width_index(ch.width), w.s);
    });
}

// gg_blend_bwd, and gg_blend_bwd_deterministic (det_ws != nullptr or I == 0 with `deterministic`)
static int blend_bwd_impl(const char *entry, const BlendCall &c, const BlendColors &src, const BlendBwdIn &in,
                          const BlendGradOut &g, int flags, bool deterministic, int64_t I, void *det_ws) {
    const int C = src.C, N = c.N;
    BLEND_REQUIRE(C >= 1, "channels < 1");
    BlendWalk w;
    int rc = blend_begin(entry, c, true, true,
                         c.xys && c.conics && src.colors && c.opacity && src.background && in.final_Ts && in.final_idx &&
                             in.v_out && g.v_xy && g.v_conic && g.v_colors && g.v_opacity,
                         (flags & GG_BWD_WS_FROM_FORWARD) != 0, w);
    if (rc != GG_OK || N == 0) return rc;
    rc = zero_grads(entry, g, C, nullptr, 0, flags, (size_t)N, w.s);
    if (rc != GG_OK) return rc;
    DetSlab det = DetSlab();
    DetWs dw;
    const int nchunks = det_chunks(C);
    if (deterministic) {
        if (I == 0) return GG_OK;   // empty lists: the zeroed (or untouched) arrays are the answer
        dw = det_ws_layout(det_ws, N, C, I);
        det.p = dw.slab;
        det.ks = C + 6 * nchunks;
        if (gg_fill_async(dw.slab, 0, sizeof(float) * 4 * (size_t)det.ks * (size_t)I, w.s) != hipSuccess ||
            gg_fill_async(dw.seg, 0, 8 * (size_t)N, w.s) != hipSuccess) {
            gg_set_error("gg_blend_bwd_deterministic: memset failed");
            return GG_ERR_LAUNCH;
        }
    }
    bwd_chunks(w, src, 0, in, g, det);
    if (deterministic) {
        const unsigned nb = (unsigned)((I + 255) / 256);
        hipLaunchKernelGGL(det_pairs_kernel, dim3(nb), dim3(256), 0, w.s, I, c.ids, dw.keys, dw.vals);
        int bits = 1;
        while (((int64_t)1 << bits) < (int64_t)N) ++bits;
        rc = gg_sort_pairs(I, dw.keys, dw.vals, bits, dw.sort_ws, dw.sort_bytes, w.s);
        if (rc != GG_OK) {
            gg_set_error("gg_blend_bwd_deterministic: sort failed");
            return rc;
        }
        hipLaunchKernelGGL(det_edges_kernel, dim3(nb), dim3(256), 0, w.s, I, N, dw.keys, dw.seg);
        hipLaunchKernelGGL(det_reduce_kernel, dim3((N + 3) / 4), dim3(256), 0, w.s, N, C, nchunks, det.ks, dw.slab,
                           dw.vals, dw.seg, g.v_xy, g.v_conic, g.v_colors, g.v_opacity, g.gstride, g.cstride);
    }
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_blend_bwd(int C, int N, int img_h, int img_w, const int32_t *ids,
                            const int32_t *tile_bins, const float *xys, const float *conics,
                            const float *colors, const float *opacity, const float *background,
                            const float *final_Ts, const int32_t *final_idx, const float *v_out,
                            float *v_xy, float *v_conic, float *v_colors, float *v_opacity,
                            int geom_stride, int color_stride, void *ws, size_t ws_bytes,
                            int flags, gg_stream_t stream) {
    return blend_bwd_impl(__func__, {N, img_h, img_w, ids, tile_bins, xys, conics, opacity, ws, ws_bytes, stream},
                          {C, colors, background}, {final_Ts, final_idx, v_out},
                          {v_xy, v_conic, v_colors, v_opacity, geom_stride, color_stride}, flags, false, 0, nullptr);
}

extern "C" int gg_blend_bwd_pair(int C, int C2, int N, int img_h, int img_w, const int32_t *ids,
                                 const int32_t *tile_bins, const float *xys, const float *conics,
                                 const float *colors, const float *colors2, const float *opacity,
                                 const float *background, const float *background2, const float *final_Ts,
                                 const int32_t *final_idx, const float *v_out, const float *const *v_out2_parts,
                                 const int *v_out2_channels, int num_parts, float *v_xy,
                                 float *v_conic, float *v_colors, float *v_colors2, float *v_opacity,
                                 int geom_stride, int color_stride, int color_stride2, void *ws, size_t ws_bytes,
                                 int flags, gg_stream_t stream) {
    const char *entry = __func__;
    const BlendColors src = {C, colors, background}, src2 = {C2, colors2, background2};
    const BlendBwdIn in = {final_Ts, final_idx, v_out};
    const BlendGradOut g = {v_xy, v_conic, v_colors, v_opacity, geom_stride, color_stride};
    const BlendGrad2 g2 = {v_out2_parts, v_out2_channels, num_parts, v_colors2, color_stride2};
    BLEND_REQUIRE((flags & GG_BWD_ACCUMULATE_GEOM) == 0, "gg_blend_bwd_pair writes the geometry gradients itself");
    BLEND_REQUIRE(C >= 32, "the first colour array needs >= 32 channels (its first chunk carries the second array)");
    BLEND_REQUIRE(C2 >= 1 && C2 <= 8, "the second colour array has 1..8 channels");
    BlendWalk w;
    int rc = blend_begin(entry, {N, img_h, img_w, ids, tile_bins, xys, conics, opacity, ws, ws_bytes, stream}, true, true,
                         xys && conics && colors && colors2 && opacity && background && background2 && final_Ts &&
                             final_idx && v_out && v_out2_parts && v_out2_channels && v_xy && v_conic && v_colors &&
                             v_colors2 && v_opacity,
                         (flags & GG_BWD_WS_FROM_FORWARD) != 0, w);
    if (rc != GG_OK || N == 0) return rc;
    BLEND_REQUIRE(num_parts >= 1 && num_parts <= 3, "the second cotangent comes as 1..3 images");
    int total = 0;
    for (int k = 0; k < num_parts; ++k) {
        BLEND_REQUIRE(v_out2_parts[k] != nullptr && v_out2_channels[k] >= 1, "empty part of the second cotangent");
        total += v_out2_channels[k];
    }
    BLEND_REQUIRE(total == C2, "the parts of the second cotangent must add up to channels2");
    rc = zero_grads(entry, g, C, &g2, C2, flags, (size_t)N, w.s);
    if (rc != GG_OK) return rc;
    gg_prof_begin(GG_K_BLEND_BWD_PAIR, w.s);
    gg_launch_blend2_bwd_pair(w, src, in, g, src2, g2);
    gg_prof_end(GG_K_BLEND_BWD_PAIR, w.s);
    bwd_chunks(w, src, 32, in, g, DetSlab());   // further chunks of the first array: their own walks, same arrays
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_blend_bwd_deterministic(int C, int N, int img_h, int img_w, const int32_t *ids,
                                          const int32_t *tile_bins, const float *xys, const float *conics,
                                          const float *colors, const float *opacity, const float *background,
                                          const float *final_Ts, const int32_t *final_idx, const float *v_out,
                                          float *v_xy, float *v_conic, float *v_colors, float *v_opacity,
                                          int geom_stride, int color_stride, void *ws, size_t ws_bytes,
                                          int flags, int64_t num_intersects, void *det_ws, size_t det_ws_bytes,
                                          gg_stream_t stream) {
    GG_REQUIRE(C >= 1, "channels < 1");
    GG_REQUIRE(num_intersects >= 0 && num_intersects < ((int64_t)1 << 31), "num_intersects out of range");
    if (num_intersects > 0 &&
        (det_ws == nullptr || det_ws_bytes < gg_blend_bwd_deterministic_workspace(N, C, num_intersects))) {
        gg_set_error("gg_blend_bwd_deterministic: deterministic workspace too small");
        return GG_ERR_WORKSPACE;
    }
    return blend_bwd_impl(__func__, {N, img_h, img_w, ids, tile_bins, xys, conics, opacity, ws, ws_bytes, stream},
                          {C, colors, background}, {final_Ts, final_idx, v_out},
                          {v_xy, v_conic, v_colors, v_opacity, geom_stride, color_stride}, flags, true, num_intersects,
                          det_ws);
}
