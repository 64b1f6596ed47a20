// hits.hip — what is under a pixel: the forward walk without colours, with per-pixel outputs (gg_blend_hits; contract
// in include/gg_raster.h, design notes in DESIGN.md §3.26).
//
// The walk is the vote walk's (votes.hip vote_walk, itself blend2.hip blend2_fwd_kernel's): one wave per 8x8 quadrant,
// 64-entry chunks culled with rec_hits_rect and compacted into LDS in list order, HGRP survivors per iteration with the
// branch-free T recurrence, the __ballot(!done) exits — and the same sigma / gg_expf_walk / alpha / T operations in the
// same order, so T, T_after and vis = alpha T carry the forward's bits.  A record is two float4 (2.3 KB of LDS per
// wave).  The four results of a pixel live in registers and leave as one coalesced store per array at the end: no
// atomics, no matrix instructions, and every pixel inside the image is written exactly once, empty tiles included.
#include "blend_launch.h"

#define HGRP 4          // survivors per loop iteration
#define HLIST_CAP 72    // 4 leading pads + 64 + 4 trailing pads

struct HitList {
    float4 a[HLIST_CAP];  // x, y, opacity, cut-off
    float4 b[HLIST_CAP];  // conic a, b, c, Gaussian id (int bits; -1: pad)
};

__device__ __forceinline__ int hit_lane_prefix(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// what a lane knows of its pixel at the end of the walk
struct HitOut {
    int hit, top, count;
    float top_vis;
};

// The walk of one quadrant.  FULL: walk to the forward's stop and keep the largest vis and the count; otherwise a lane
// is done at its hit (a quadrant of opaque pixels leaves after a few entries).  Two builds, so that the hit-only loop
// carries neither the other's registers nor its instructions.
template <bool FULL>
__device__ __forceinline__ HitOut hit_walk(HitList &Lst, const int lane, const int2 range, const float px, const float py,
                                           const float xlo, const float xhi, const float ylo, const float yhi,
                                           const bool inside, const float t_hit, const int32_t *__restrict__ ids,
                                           const GRec *__restrict__ rec) {
    HitOut o = {-1, -1, 0, 0.0f};
    float T = 1.0f;
    bool done = !inside;
    for (int base = range.x; base < range.y; base += 64) {
        if (__ballot(!done) == 0ull) break;
        const int e = base + lane;
        const bool valid = e < range.y;
        const int g = valid ? ids[e] : 0;
        // stage: the survivors of the exact ellipse-vs-quadrant cull in list order, HGRP null records on both sides
        const float4 ra = reinterpret_cast<const float4 *>(rec + g)[0];
        const float4 rb = reinterpret_cast<const float4 *>(rec + g)[1];
        const bool hit = valid && rec_hits_rect(ra, rb, xlo, xhi, ylo, yhi);
        const uint64_t m = __ballot(hit);
        const int cnt = __builtin_popcountll(m);
        if (hit) {
            const int pos = HGRP + hit_lane_prefix(m);
            Lst.a[pos] = ra;
            Lst.b[pos] = make_float4(rb.x, rb.y, rb.z, __builtin_bit_cast(float, g));
        }
        if (lane < 2 * HGRP) {   // null pads: opacity 0 -> alpha = 0 < 1/255
            const int q = (lane < HGRP) ? lane : (cnt + lane);
            Lst.a[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            Lst.b[q] = make_float4(0.f, 0.f, 0.f, __builtin_bit_cast(float, -1));
        }
        __builtin_amdgcn_wave_barrier();
        for (int k = 0; k < cnt; k += HGRP) {
            if (k > 0 && __ballot(!done) == 0ull) break;
            float4 A[HGRP], B[HGRP];
#pragma unroll
            for (int q = 0; q < HGRP; ++q) {
                A[q] = Lst.a[HGRP + k + q];
                B[q] = Lst.b[HGRP + k + q];
            }
            float alpha[HGRP];
            bool pass[HGRP];
#pragma unroll
            for (int q = 0; q < HGRP; ++q) {
                const float dx = A[q].x - px, dy = A[q].y - py;
                const float sigma = __builtin_fmaf(
                    0.5f, __builtin_fmaf(B[q].x * dx, dx, (B[q].z * dy) * dy), (B[q].y * dx) * dy);
                alpha[q] = fminf(GG_ALPHA_MAX_FWD, A[q].z * gg_expf_walk(-sigma));
                pass[q] = sigma >= 0.0f && !(alpha[q] < GG_ALPHA_MIN);
            }
#pragma unroll
            for (int q = 0; q < HGRP; ++q) {
                const float next_T = T * (1.0f - alpha[q]);
                const bool live = pass[q] && !done;
                const bool stop = live && (next_T <= GG_T_EPS);
                const bool blend = live && !stop;
                const int gid = __builtin_bit_cast(int, B[q].w);
                const bool first = blend && o.hit < 0 && next_T <= t_hit;
                o.hit = first ? gid : o.hit;
                if (FULL) {
                    const float vis = blend ? alpha[q] * T : 0.0f;
                    const bool more = vis > o.top_vis;      // strict: the earliest of equal values stays
                    o.top = more ? gid : o.top;
                    o.top_vis = more ? vis : o.top_vis;
                    o.count += blend ? 1 : 0;
                }
                T = blend ? next_T : T;
                done = done || stop || (!FULL && first);
            }
        }
        __builtin_amdgcn_wave_barrier();  // the list is rewritten by the next chunk
    }
    return o;
}

template <bool FULL>
__global__ __launch_bounds__(64 * GG_WPB_OTHER) void blend_hits_kernel(
    int N, int img_h, int img_w, int tiles_x, int ntiles, const int32_t *__restrict__ ids,
    const int32_t *__restrict__ bins, const GRec *__restrict__ rec, float t_hit, int32_t *__restrict__ hit_idx,
    int32_t *__restrict__ top_idx, float *__restrict__ top_vis, int32_t *__restrict__ count) {
    __shared__ HitList lists[GG_WPB_OTHER];
    int wave;
    const int tile = blend_tile_wave<GG_WPB_OTHER>(blockIdx.x, threadIdx.x, ntiles, wave);
    if (tile < 0) return;
    const int lane = threadIdx.x & 63;
    HitList &Lst = lists[wave & (GG_WPB_OTHER - 1)];
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int qx0 = tx * GG_BLOCK + (wave & 1) * 8, qy0 = ty * GG_BLOCK + (wave >> 1) * 8;
    const int j = qx0 + (lane & 7), i = qy0 + (lane >> 3);
    const bool inside = (i < img_h) && (j < img_w);
    if (__ballot(inside) == 0ull) return;      // a quadrant outside the image owns no pixel
    const float px = (float)j, py = (float)i;
    const float xlo = (float)qx0, xhi = (float)(qx0 + 7), ylo = (float)qy0, yhi = (float)(qy0 + 7);
    // num_points == 0: the lists are not looked at, every pixel gets the defaults
    const int2 range = N > 0 ? gg_tile_range(bins, tile) : make_int2(0, 0);
    const HitOut o = hit_walk<FULL>(Lst, lane, range, px, py, xlo, xhi, ylo, yhi, inside, t_hit, ids, rec);
    if (inside) {
        const size_t p = (size_t)i * (size_t)img_w + (size_t)j;
        hit_idx[p] = o.hit;
        if (FULL) {
            top_idx[p] = o.top;
            top_vis[p] = o.top_vis;
            count[p] = o.count;
        }
    }
}

void gg_launch_blend_hits(const BlendWalk &w, int N, float t_hit, int32_t *hit_idx, int32_t *top_idx, float *top_vis,
                          int32_t *count) {
    const dim3 grid(gg_blend_grid(w.ntiles, GG_WPB_OTHER)), block(64 * GG_WPB_OTHER);
    if (top_idx)
        hipLaunchKernelGGL(blend_hits_kernel<true>, grid, block, 0, w.s, N, w.img_h, w.img_w, w.tiles_x, w.ntiles, w.ids,
                           w.bins, w.rec, t_hit, hit_idx, top_idx, top_vis, count);
    else
        hipLaunchKernelGGL(blend_hits_kernel<false>, grid, block, 0, w.s, N, w.img_h, w.img_w, w.tiles_x, w.ntiles, w.ids,
                           w.bins, w.rec, t_hit, hit_idx, top_idx, top_vis, count);
}
