// blend_launch.h — the host-side interface between blend.hip (C ABI, launch plan) and blend2.hip (kernels and their
// launchers): the records that describe one blend call and the launchers that unpack them into kernel arguments.
#pragma once
#include "blend_common.h"

// what every walk of one call shares: image, tile grid, tile lists, packed records, stream
struct BlendWalk {
    int img_h, img_w, tiles_x, ntiles;
    const int32_t *ids;
    const int32_t *bins;   // the caller's (tiles, 2) int32 array, 4-byte aligned: read through gg_tile_range
    const GRec *rec;
    hipStream_t s;
};
// a colour source: (N, C) rows and the (C,) background
struct BlendColors {
    int C;
    const float *colors, *background;
};
struct BlendFwdOut {
    float *out_img, *final_Ts;
    int32_t *final_idx;
};
// what the backward reads of the forward, and the cotangent of the image
struct BlendBwdIn {
    const float *final_Ts;
    const int32_t *final_idx;
    const float *v_out;
};
// gradient outputs; a stride of 0 means dense rows
struct BlendGradOut {
    float *v_xy, *v_conic, *v_colors, *v_opacity;
    int gstride, cstride;
};
// the pair backward's second array: its cotangent as 1..3 images of `channels[k]` channels, and its gradient rows
struct BlendGrad2 {
    const float *const *v_out_parts;
    const int *v_out_channels;
    int num_parts;
    float *v_colors;
    int cstride;
};
// one walk of the chunk plan (blend.hip): `blocks` blocks of `n` channels from `off`, on the kernels of `width`
struct BlendChunk {
    int off, width, n, blocks;
};

void gg_launch_blend2_fwd(const BlendWalk &w, const BlendColors &src, const BlendChunk &ch, const BlendFwdOut &out,
                          int write_final);
void gg_launch_blend2_fwd_pair(const BlendWalk &w, const BlendColors &src, const BlendColors &src2,
                               const BlendFwdOut &out, float *out_img2, int ncb, bool fast, unsigned bytes1,
                               unsigned bytes2);
void gg_launch_blend2_bwd(const BlendWalk &w, const BlendColors &src, const BlendChunk &ch, const BlendBwdIn &in,
                          const BlendGradOut &g, const DetSlab &det);
void gg_launch_blend2_bwd_pair(const BlendWalk &w, const BlendColors &src, const BlendBwdIn &in, const BlendGradOut &g,
                               const BlendColors &src2, const BlendGrad2 &g2);
// votes.hip: the vote walk of gg_blend_votes (labels (H, W) bytes, votes (N, L) int64, added to)
void gg_launch_blend_votes(const BlendWalk &w, int L, int N, const uint8_t *labels, int64_t *votes);
// hits.hip: the walk of gg_blend_hits ((H, W) outputs, overwritten; top_idx == nullptr: the hit-only build)
void gg_launch_blend_hits(const BlendWalk &w, int N, float t_hit, int32_t *hit_idx, int32_t *top_idx, float *top_vis,
                          int32_t *count);
#ifdef GG_ABLATION
void gg_launch_blend2_bwd_ablate(int abl, const BlendWalk &w, const BlendColors &src, const BlendChunk &ch,
                                 const BlendBwdIn &in, const BlendGradOut &g);
#endif
