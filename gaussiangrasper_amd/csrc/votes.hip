// votes.hip — the transpose of the blend: per-Gaussian sums of the forward walk's blend weights, by pixel label
// (gg_blend_votes; contract in include/gg_raster.h, design notes in DESIGN.md §3.24).
//
// The walk is the narrow forward's (blend2.hip blend2_fwd_kernel): one wave per 8x8 quadrant, 64-entry chunks culled
// with rec_hits_rect and compacted into LDS in list order, GRP survivors per iteration with the branch-free T
// recurrence, the __ballot(!done) exits — and the same sigma / gg_expf_walk / alpha / T operations in the same order,
// so vis = alpha T carries the forward's bits.  There are no colours: a record is two float4 (2.3 KB of LDS per wave,
// 3.5 KB with the cells of the several-label path), there are no accumulators and no matrix instructions.  What a wave
// adds to votes[g][l] is the sum over its pixels of label l of trunc(vis 2^24) — integers, so neither the order inside
// the wave (butterfly or LDS cells, below) nor the order of the waves' atomics changes a bit of the result.
#include "blend_launch.h"

#define VGRP 4          // survivors per loop iteration
#define VLIST_CAP 72    // 4 leading pads + 64 + 4 trailing pads
// A quadrant with this many labels or more sums a group's votes through LDS cells instead of one butterfly per label
// (see the kernel).  Measured (profiles/lift_bench.json): with one label the butterfly is faster (64
// lanes adding into one LDS cell serialise), from two labels on the cells are.
#ifndef GG_VOTE_CELLS_FROM
#define GG_VOTE_CELLS_FROM 2
#endif

struct VoteList {
    float4 a[VLIST_CAP];  // x, y, opacity, cut-off
    float4 b[VLIST_CAP];  // conic a, b, c, Gaussian id (int bits; -1: pad)
    int cell[64 * VGRP];  // [label slot][group member]: a group's sums (several-label quadrants); zero between groups
    int set_label[64];    // the labels present in the quadrant, by slot
};

__device__ __forceinline__ int vote_lane_prefix(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
template <int CTRL>
__device__ __forceinline__ int vote_dpp(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ int vote_dpp_xor4(int v) {
    int t = __builtin_amdgcn_update_dpp(0, v, 0x104 /*row_shl:4*/, 0xf, 0x5, true);
    return __builtin_amdgcn_update_dpp(t, v, 0x114 /*row_shr:4*/, 0xf, 0xa, true);
}
// Wave totals of four per-lane integers (each < 2^24, so a total stays below 2^30): a halving butterfly over lane
// bits 0 and 1 (four values -> one per lane), then four plain exchanges.  Afterwards every lane holds the wave total of
// value 2 (lane & 1) + ((lane >> 1) & 1): lanes 0, 1, 2, 3 hold values 0, 2, 1, 3.
__device__ __forceinline__ int vote_reduce4(const int (&v)[VGRP], int lane) {
    const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0;
    const int k0 = b0 ? v[2] : v[0], k1 = b0 ? v[3] : v[1];
    const int s0 = b0 ? v[0] : v[2], s1 = b0 ? v[1] : v[3];
    const int r0 = k0 + vote_dpp<0xB1>(s0);          // quad_perm [1,0,3,2]
    const int r1 = k1 + vote_dpp<0xB1>(s1);
    int r = (b1 ? r1 : r0) + vote_dpp<0x4E>(b1 ? r0 : r1);   // quad_perm [2,3,0,1]
    r += vote_dpp_xor4(r);
    r += vote_dpp<0x128>(r);                          // row_ror:8
    auto x16 = __builtin_amdgcn_permlane16_swap((unsigned)r, (unsigned)r, false, false);
    r = (int)((unsigned)x16[0] + (unsigned)x16[1]);
    auto x32 = __builtin_amdgcn_permlane32_swap((unsigned)r, (unsigned)r, false, false);
    return (int)((unsigned)x32[0] + (unsigned)x32[1]);
}

// The walk of one quadrant.  CELLS: how a group's per-(Gaussian, label) sums are formed (see the kernel); the two
// builds are separate loops so that neither carries the other's registers.
template <bool CELLS>
__device__ __forceinline__ void vote_walk(VoteList &Lst, const int lane, const int2 range, const float px, const float py,
                                          const float xlo, const float xhi, const float ylo, const float yhi,
                                          const bool counted, const int slot, const int set_label, const int nl,
                                          const int L, const int N, const int32_t *__restrict__ ids,
                                          const GRec *__restrict__ rec, unsigned long long *__restrict__ votes) {
    float T = 1.0f;
    bool done = !counted;
    for (int base = range.x; base < range.y; base += 64) {
        if (__ballot(!done) == 0ull) break;
        const int e = base + lane;
        const bool valid = e < range.y;
        const int g = valid ? ids[e] : 0;
        // stage: the survivors of the exact ellipse-vs-quadrant cull in list order, VGRP null records on both sides
        const float4 ra = reinterpret_cast<const float4 *>(rec + g)[0];
        const float4 rb = reinterpret_cast<const float4 *>(rec + g)[1];
        const bool hit = valid && rec_hits_rect(ra, rb, xlo, xhi, ylo, yhi);
        const uint64_t m = __ballot(hit);
        const int cnt = __builtin_popcountll(m);
        if (hit) {
            const int pos = VGRP + vote_lane_prefix(m);
            Lst.a[pos] = ra;
            Lst.b[pos] = make_float4(rb.x, rb.y, rb.z, __builtin_bit_cast(float, g));
        }
        if (lane < 2 * VGRP) {   // null pads: opacity 0 -> alpha = 0 < 1/255
            const int q = (lane < VGRP) ? lane : (cnt + lane);
            Lst.a[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            Lst.b[q] = make_float4(0.f, 0.f, 0.f, __builtin_bit_cast(float, -1));
        }
        __builtin_amdgcn_wave_barrier();
        for (int k = 0; k < cnt; k += VGRP) {
            if (k > 0 && __ballot(!done) == 0ull) break;
            float4 A[VGRP], B[VGRP];
#pragma unroll
            for (int q = 0; q < VGRP; ++q) {
                A[q] = Lst.a[VGRP + k + q];
                B[q] = Lst.b[VGRP + k + q];
            }
            float alpha[VGRP];
            bool pass[VGRP];
#pragma unroll
            for (int q = 0; q < VGRP; ++q) {
                const float dx = A[q].x - px, dy = A[q].y - py;
                const float sigma = __builtin_fmaf(
                    0.5f, __builtin_fmaf(B[q].x * dx, dx, (B[q].z * dy) * dy), (B[q].y * dx) * dy);
                alpha[q] = fminf(GG_ALPHA_MAX_FWD, A[q].z * gg_expf_walk(-sigma));
                pass[q] = sigma >= 0.0f && !(alpha[q] < GG_ALPHA_MIN);
            }
            int qv[VGRP];
#pragma unroll
            for (int q = 0; q < VGRP; ++q) {
                const float next_T = T * (1.0f - alpha[q]);
                const bool live = pass[q] && !done;
                const bool stop = live && (next_T <= GG_T_EPS);
                const bool blend = live && !stop;
                const float vis = blend ? alpha[q] * T : 0.0f;
                qv[q] = (int)(vis * 16777216.0f);      // exact product (vis < 1), truncated: < 2^24
                T = blend ? next_T : T;
                done = done || stop;
            }
            const int any = qv[0] | qv[1] | qv[2] | qv[3];
            if (__ballot(any != 0) == 0ull) continue;
            // the group's Gaussian of the value this lane holds after vote_reduce4 (lanes 0..3 issue the atomics)
            const int my_q = 2 * (lane & 1) + ((lane >> 1) & 1);
            const int gid = __builtin_bit_cast(int, my_q == 0 ? B[0].w : my_q == 1 ? B[1].w : my_q == 2 ? B[2].w : B[3].w);
            if (CELLS) {
                if (counted) {
#pragma unroll
                    for (int q = 0; q < VGRP; ++q)
                        if (qv[q] != 0) atomicAdd(&Lst.cell[slot * VGRP + q], qv[q]);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int cq = lane & (VGRP - 1);     // this lane's cell: group member cq of label slot s0 + (lane >> 2)
                const int cgid = __builtin_bit_cast(int, cq == 0 ? B[0].w : cq == 1 ? B[1].w : cq == 2 ? B[2].w : B[3].w);
                for (int s0 = 0; s0 < nl; s0 += 64 / VGRP) {
                    const int s = s0 + (lane >> 2);
                    if (s < nl) {
                        const int sum = Lst.cell[s * VGRP + cq];
                        if (sum != 0) {
                            Lst.cell[s * VGRP + cq] = 0;
                            if ((unsigned)cgid < (unsigned)N)
                                atomicAdd(votes + (size_t)cgid * (size_t)L + (size_t)Lst.set_label[s],
                                          (unsigned long long)sum);
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                continue;
            }
            for (int s = 0; s < nl; ++s) {
                const bool mine = slot == s;
                if (__ballot(mine && any != 0) == 0ull) continue;
                int part[VGRP];
#pragma unroll
                for (int q = 0; q < VGRP; ++q) part[q] = mine ? qv[q] : 0;
                const int sum = vote_reduce4(part, lane);
                const int l = __builtin_amdgcn_readlane(set_label, s);
                if (lane < VGRP && sum != 0 && (unsigned)gid < (unsigned)N)
                    atomicAdd(votes + (size_t)gid * (size_t)L + (size_t)l, (unsigned long long)sum);
            }
        }
        __builtin_amdgcn_wave_barrier();  // the list is rewritten by the next chunk
    }
}

__global__ __launch_bounds__(64 * GG_WPB_OTHER) void blend_votes_kernel(
    int L, int N, int img_h, int img_w, int tiles_x, int ntiles, const int32_t *__restrict__ ids,
    const int32_t *__restrict__ bins, const GRec *__restrict__ rec, const uint8_t *__restrict__ labels,
    unsigned long long *__restrict__ votes) {
    __shared__ VoteList lists[GG_WPB_OTHER];
    int wave;
    const int tile = blend_tile_wave<GG_WPB_OTHER>(blockIdx.x, threadIdx.x, ntiles, wave);
    if (tile < 0) return;
    const int lane = threadIdx.x & 63;
    VoteList &Lst = lists[wave & (GG_WPB_OTHER - 1)];
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int qx0 = tx * GG_BLOCK + (wave & 1) * 8, qy0 = ty * GG_BLOCK + (wave >> 1) * 8;
    const int j = qx0 + (lane & 7), i = qy0 + (lane >> 3);
    const bool inside = (i < img_h) && (j < img_w);
    const float px = (float)j, py = (float)i;
    const float xlo = (float)qx0, xhi = (float)(qx0 + 7), ylo = (float)qy0, yhi = (float)(qy0 + 7);
    const int2 range = gg_tile_range(bins, tile);
    if (range.y <= range.x) return;

    // A pixel outside the image or with a label >= L votes for nobody: its T need not be followed, so it counts as
    // finished from the start (a quadrant of such pixels only is left at once).
    const int lab = inside ? (int)labels[(size_t)i * img_w + j] : 255;
    const bool counted = lab < L;
    // The labels present in the quadrant, once per wave: slot = position of this lane's label in the set, and lane s
    // keeps the s-th label of the set (almost always one or two).
    int slot = -1, set_label = 0, nl = 0;
    for (uint64_t rem = __ballot(counted); rem != 0ull;) {
        const int l = __builtin_amdgcn_readlane(lab, (int)__builtin_ctzll(rem));
        const bool mine = counted && lab == l;
        rem &= ~__ballot(mine);
        slot = mine ? nl : slot;
        set_label = (lane == nl) ? l : set_label;
        ++nl;
    }
    if (nl == 0) return;
    // Two ways to a group's per-(Gaussian, label) sums.  Fewer than GG_VOTE_CELLS_FROM labels (one, in the product
    // build): one masked butterfly per label, lanes 0..3 issue the atomics (one instruction per label).  More: every
    // lane adds its four values into the LDS cells of its own label (ds_add, no return), and the cells leave 16 labels
    // at a time, one lane per cell — ONE global atomic instruction for up to 64 (Gaussian, label) sums instead of one
    // per label.  Integer sums: the same bits either way.
    if (nl >= GG_VOTE_CELLS_FROM) {
#pragma unroll
        for (int q = 0; q < VGRP; ++q) Lst.cell[lane * VGRP + q] = 0;
        Lst.set_label[lane] = set_label;
        vote_walk<true>(Lst, lane, range, px, py, xlo, xhi, ylo, yhi, counted, slot, set_label, nl, L, N, ids, rec, votes);
    } else {
        vote_walk<false>(Lst, lane, range, px, py, xlo, xhi, ylo, yhi, counted, slot, set_label, nl, L, N, ids, rec, votes);
    }
}

void gg_launch_blend_votes(const BlendWalk &w, int L, int N, const uint8_t *labels, int64_t *votes) {
    hipLaunchKernelGGL(blend_votes_kernel, dim3(gg_blend_grid(w.ntiles, GG_WPB_OTHER)), dim3(64 * GG_WPB_OTHER), 0, w.s,
                       L, N, w.img_h, w.img_w, w.tiles_x, w.ntiles, w.ids, w.bins, w.rec, labels,
                       reinterpret_cast<unsigned long long *>(votes));
}
