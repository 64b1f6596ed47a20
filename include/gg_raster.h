/*
 * gg_raster.h — C ABI of libgg_raster.so, the MI355X (gfx950) Gaussian-splatting rasterizer.
 *
 * This is the drop-in boundary for GaussianGrasper's feature-field hot path.  The reference
 * reaches the same functionality through gsplat==0.1.0's private extension module
 * (`gsplat.cuda._C`, bound with pybind11/torch types); the four autograd.Functions the
 * reference model calls — nerfstudio/models/gaussian_splatting.py:699 (ProjectGaussians),
 * :730 (SphericalHarmonics), :735/:759/:773 (RasterizeGaussians), :747 (NDRasterizeGaussians)
 * — sit directly on top of it.  Each entry point below names the binding it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / PyTorch caching allocator); the library
 *     never allocates, frees or keeps caller memory; scratch comes in through (ws, ws_bytes)
 *     whose size the matching *_workspace() query returns;
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); all work is
 *     enqueued asynchronously, nothing synchronises the host;
 *   - layouts are torch's: row-major array-of-structs, fp32, ids int32;
 *   - return 0 on success; negative on error (GG_ERR_*), message via gg_last_error().
 *
 * Arithmetic contract: SURVEY.md §8a rows a3-a12 with the constants of gg_constants.h;
 * the forward results (radii, tile counts, depth order, tile lists, images, final_T, final_idx)
 * are bit-identical to the CPU oracle (oracle/gg_oracle.c), gradients agree to fp32 summation
 * order.
 */
#ifndef GG_RASTER_H
#define GG_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GG_OK 0
#define GG_ERR_INVALID_ARG (-1)
#define GG_ERR_LAUNCH (-2)
#define GG_ERR_WORKSPACE (-3)
#define GG_ERR_UNSUPPORTED (-4)
#define GG_ERR_NOT_CONVERGED (-5) /* gg_field_route: max_rounds ran out; the output holds valid upper bounds */

typedef void *gg_stream_t; /* hipStream_t */

/* ABI version of this header (bumped on any signature change). */
int gg_abi_version(void);
/* Message for the last error returned on the calling thread ("" if none). */
const char *gg_last_error(void);

/* ---- projection ------------------------------------------------------------------------
 * Replaces gsplat `_C.project_gaussians_forward` (ProjectGaussians.forward; reference call
 * gaussian_splatting.py:699-713).  viewmat: >=12 floats row-major (the caller's viewmat[:3,:]);
 * projmat: 16 floats (projmat @ viewmat).  All six outputs are fully written (zeros for culled
 * Gaussians as the oracle documents), so they may be uninitialised on entry.  quats (N, 4) is read one row per load:
 * 16-byte aligned, here and in gg_project_fwd_count (as gg_activate_*, gg_view_* and gg_quat_to_rotmat_* require of the
 * same array); a misaligned quats is refused with GG_ERR_INVALID_ARG before any launch. */
int gg_project_fwd(int num_points, const float *means3d, const float *scales, float glob_scale,
                   const float *quats, const float *viewmat, const float *projmat, float fx,
                   float fy, float cx, float cy, int img_height, int img_width, int tiles_x,
                   int tiles_y, float clip_thresh, float *cov3d, float *xys, float *depths,
                   int32_t *radii, float *conics, int32_t *num_tiles_hit, gg_stream_t stream);

/* gg_project_fwd that also leaves sum(num_tiles_hit) in *num_intersects_out (device, int64) — what gg_count_intersects
 * computes with a launch of its own (reference: `torch.cumsum(num_tiles_hit)[-1].item()` inside every rasterize call).
 * count_ws: gg_project_count_workspace(num_points) bytes of scratch, 4-byte aligned (per-workgroup partial sums, added
 * up by a one-workgroup launch behind the projection). */
size_t gg_project_count_workspace(int num_points);
int gg_project_fwd_count(int num_points, const float *means3d, const float *scales, float glob_scale,
                         const float *quats, const float *viewmat, const float *projmat, float fx, float fy,
                         float cx, float cy, int img_height, int img_width, int tiles_x, int tiles_y,
                         float clip_thresh, float *cov3d, float *xys, float *depths, int32_t *radii, float *conics,
                         int32_t *num_tiles_hit, int64_t *num_intersects_out, void *count_ws, size_t count_ws_bytes,
                         gg_stream_t stream);

/* Replaces gsplat `_C.project_gaussians_backward` (ProjectGaussians.backward).  v_conic uses
 * gsplat's symmetric-matrix convention (v_conic[:,1] is half of dL/d conic.y).  Outputs fully
 * written (zeros where radii<=0).  quats and v_quat (N, 4) are read / written one row per access: both 16-byte aligned,
 * here and in gg_project_bwd_ex; a misaligned one is refused with GG_ERR_INVALID_ARG, its name in gg_last_error(),
 * before any launch. */
int gg_project_bwd(int num_points, const float *means3d, const float *scales, float glob_scale,
                   const float *quats, const float *viewmat, const float *projmat, float fx,
                   float fy, float cx, float cy, int img_height, int img_width,
                   const int32_t *radii, const float *conics, const float *v_xy,
                   const float *v_depth, const float *v_conic, float *v_mean3d, float *v_scale,
                   float *v_quat, gg_stream_t stream);
/* gg_project_bwd_ex: the same with v_xy / v_conic rows v_xy_stride / v_conic_stride floats apart (the blend
 * backward's interleaved gradient record {xy, conic, opacity, ...} is read in place: no compaction copies) and,
 * with accumulate_means != 0, v_mean3d added to instead of written (the caller's gradient buffer of the means,
 * which enter the projection as a leaf). */
int gg_project_bwd_ex(int num_points, const float *means3d, const float *scales, float glob_scale,
                      const float *quats, const float *viewmat, const float *projmat, float fx, float fy, float cx,
                      float cy, int img_height, int img_width, const int32_t *radii, const float *conics,
                      const float *v_xy, int v_xy_stride, const float *v_depth, const float *v_conic,
                      int v_conic_stride, float *v_mean3d, int accumulate_means, float *v_scale, float *v_quat,
                      gg_stream_t stream);

/* ---- spherical harmonics -----------------------------------------------------------------
 * Replace gsplat `_C.compute_sh_forward` / `_C.compute_sh_backward` (SphericalHarmonics;
 * reference call gaussian_splatting.py:730).  coeffs (N, num_bases, 3); num_bases in
 * {1,4,9,16,25}; degrees_to_use <= degree(num_bases). */
int gg_sh_fwd(int num_points, int num_bases, int degrees_to_use, const float *viewdirs,
              const float *coeffs, float *colors, gg_stream_t stream);
int gg_sh_bwd(int num_points, int num_bases, int degrees_to_use, const float *viewdirs,
              const float *v_colors, float *v_coeffs, gg_stream_t stream);
/* v_coeffs += (instead of =): the gradient goes straight into the caller's accumulation buffer (the
 * `.grad` of the SH parameter across the views of an optimizer step) — one read-modify-write of
 * 300 B per Gaussian instead of a 300 B store followed by autograd's separate add. */
int gg_sh_bwd_accumulate(int num_points, int num_bases, int degrees_to_use, const float *viewdirs,
                         const float *v_colors, float *v_coeffs, gg_stream_t stream);

/* gg_shade_tail_fwd / _bwd: the plugin route's 7-channel colour array in one pass each way —
 * tail (N, 7) = [ clamp(SH(viewdirs, coeffs) + 0.5, 0, 1) | depth | normal ], i.e. the reference's
 * `rgbs = torch.clamp(SphericalHarmonics.apply(n, viewdirs, colors) + 0.5, 0.0, 1.0)` (gaussian_splatting.py:
 * 730-731) packed with the depth (:765) and normal (:779) colour arrays it rasterizes next.  clamp_mask (N bytes):
 * bit c set = the gradient of colour c passes the clamp (0 <= x <= 1, torch.clamp's rule).
 * Backward: v_tail rows are v_tail_stride >= 7 floats apart (the interleaved gradient record of the blend
 * backward is read in place); v_coeffs (N, num_bases, 3) is written, or added to when accumulate != 0;
 * v_depths (N,), v_normals (N, 3) are written. */
int gg_shade_tail_fwd(int num_points, int num_bases, int degrees_to_use, const float *viewdirs,
                      const float *coeffs, const float *depths, const float *normals, float *tail,
                      uint8_t *clamp_mask, gg_stream_t stream);
/* gg_shade_tail_fwd_ex: the same; one_wave != 0 launches the kernel's build with 64-thread workgroups and a quarter of
 * the LDS per workgroup — the same bits.  For a launch that runs beside a blend kernel of another stream (forward of
 * view k + 1 beside backward of view k): a one-wave workgroup is placed where one blend workgroup has finished, the
 * four-wave one only once that kernel drains.  Alone on the GPU the four-wave build is no slower: keep it there. */
int gg_shade_tail_fwd_ex(int num_points, int num_bases, int degrees_to_use, const float *viewdirs,
                         const float *coeffs, const float *depths, const float *normals, float *tail,
                         uint8_t *clamp_mask, int one_wave, gg_stream_t stream);
int gg_shade_tail_bwd(int num_points, int num_bases, int degrees_to_use, const float *viewdirs,
                      const float *v_tail, int v_tail_stride, const uint8_t *clamp_mask, float *v_coeffs,
                      int accumulate, float *v_depths, float *v_normals, gg_stream_t stream);

/* Deferred SH gradient over the views of an optimizer step (the views of a step accumulate into one
 * gradient).  gg_shade_tail_bwd_split is the part of gg_shade_tail_bwd that cannot wait — v_depths, v_normals and
 * the clamp-masked colour cotangent v_rgb (N, 3), which is KEPT instead of being expanded; gg_sh_bwd_multi expands
 * the kept cotangents of num_views views in one pass: v_coeffs (N, num_bases, 3) = [v_coeffs +] sum_v Y(viewdirs_v)
 * (x) v_rgb_v, the views summed in order starting from the buffer's value (the bits of adding view after view).  viewdirs /
 * v_colors: host arrays of num_views device pointers to (N, 3) arrays.  One 300-byte write per Gaussian and step
 * instead of a 600-byte read-modify-write per Gaussian and view. */
int gg_shade_tail_bwd_split(int num_points, const float *v_tail, int v_tail_stride, const uint8_t *clamp_mask,
                            float *v_rgb, float *v_depths, float *v_normals, gg_stream_t stream);
int gg_sh_bwd_multi(int num_points, int num_bases, int degrees_to_use, int num_views, const float *const *viewdirs,
                    const float *const *v_colors, float *v_coeffs, int accumulate, gg_stream_t stream);

/* ---- one backward pass over the Gaussians of a view (round 4; ops.ViewGeometry of the plugin route) ------------
 * gg_shade_tail_bwd_split + gg_project_bwd_ex + gg_activate_bwd_ex in ONE kernel, for the case where every parameter has a
 * gradient buffer to add into: reads the blend backward's record of a Gaussian once — rec_stride floats apart,
 * [v_xy 0..1 | v_conic 2..4 | v_opacity 5 | v_rgb 6..8 | v_depth 9 | v_normal 10..12] — keeps the clamp-masked colour
 * cotangent v_rgb (N, 3) for gg_sh_bwd_multi and ADDS the gradients of the means (N, 3), log scales (N, 3), raw
 * quaternions (N, 4) and opacity logits (N) to v_means / v_log_scales / v_quats / v_opacities.  `scales`, `quats_n`,
 * `opac`, `axis` are gg_activate_fwd's outputs, `quats_raw` its input, `radii` / `conics` gg_project_fwd's.  The
 * per-Gaussian operation sequence is the three kernels' (shared device functions): the same bits.
 * Reference: what autograd does behind gaussian_splatting.py:699-731 in ~60 launches per view. */
int gg_view_bwd(int num_points, const float *rec, int rec_stride, const uint8_t *clamp_mask, const float *means,
                const float *scales, float glob_scale, const float *quats_raw, const float *quats_n, const float *opac,
                const int32_t *axis, const float *viewmat, const float *projmat, float fx, float fy, int img_height,
                int img_width, const int32_t *radii, const float *conics, float *v_rgb, float *v_means,
                float *v_log_scales, float *v_quats, float *v_opacities, gg_stream_t stream);

/* ---- camera pose gradients (the camera optimizer's `apply_to_camera`, reference gaussian_splatting.py:638-640) -------
 * The VJP of the projection with respect to the camera: for the visible Gaussians (radii > 0) the cotangents (v_xy,
 * v_depth, v_conic — gg_project_bwd's convention) are carried to
 *   v_viewmat (12 floats): d/d viewmat, 3 x 4 row-major (the world -> camera rows gg_project_fwd reads), and
 *   v_projmat (16 floats): d/d projmat, 4 x 4 row-major (the full projection projmat @ viewmat of the pixel centres);
 *                          row 2 (clip-space z) is read by nothing and is written as zeros.
 * Both are sums over all Gaussians, WRITTEN (not added to).  The sums are deterministic: one row of 24 partial sums per
 * workgroup of 256 Gaussians in `ws`, added up in a fixed order in fp64 by a one-workgroup launch — no float atomics,
 * the same bits on every run.  ws: gg_pose_grad_workspace(num_points) bytes, 16-byte aligned.  num_points == 0 writes
 * zeros.  Under GG_VJP_GSPLAT_COMPAT the simplified quantities of the means' VJP are used (no homogeneous-w term, no
 * FOV-clamp derivative).  Intrinsics (fx, fy, cx, cy) get no gradient.
 *
 * gg_view_bwd_pose: gg_view_bwd (same arguments, the same per-Gaussian gradients bit for bit) plus the pose sums.
 * gg_project_pose_bwd: the pose sums alone; v_xy / v_conic rows v_xy_stride / v_conic_stride floats apart (as
 * gg_project_bwd_ex takes them), quats_n 16-byte aligned; the Gaussians get no gradient. */
size_t gg_pose_grad_workspace(int num_points);
int gg_view_bwd_pose(int num_points, const float *rec, int rec_stride, const uint8_t *clamp_mask, const float *means,
                     const float *scales, float glob_scale, const float *quats_raw, const float *quats_n,
                     const float *opac, const int32_t *axis, const float *viewmat, const float *projmat, float fx,
                     float fy, int img_height, int img_width, const int32_t *radii, const float *conics, float *v_rgb,
                     float *v_means, float *v_log_scales, float *v_quats, float *v_opacities, float *v_viewmat,
                     float *v_projmat, void *ws, size_t ws_bytes, gg_stream_t stream);
int gg_project_pose_bwd(int num_points, const float *means, const float *scales, float glob_scale,
                        const float *quats_n, const float *viewmat, const float *projmat, float fx, float fy,
                        int img_height, int img_width, const int32_t *radii, const float *conics, const float *v_xy,
                        int v_xy_stride, const float *v_depth, const float *v_conic, int v_conic_stride,
                        float *v_viewmat, float *v_projmat, void *ws, size_t ws_bytes, gg_stream_t stream);

/* gg_activate_fwd + gg_project_fwd (glob_scale 1) + the intersection count in one pass over the Gaussians (round 4,
 * ops.ViewGeometry).  Outputs are those two entries' (bit for bit: shared device code) except that cov3d is not produced.
 * *num_intersects_out (device, int64) receives sum(num_tiles_hit).  `parts`: gg_view_fwd_workspace(num_points) bytes,
 * 4-byte aligned; on return it holds per workgroup of 256 Gaussians [sum of num_tiles_hit | smallest | largest depth bits
 * of its visible Gaussians] (three arrays of ceil(num_points / 256) words) — gg_bin_sort_dev_ex takes the last two
 * instead of running its own pass over depths and radii.  `records` (nullable): gg_blend_workspace(num_points) bytes,
 * 16-byte aligned — filled with the blend kernels' packed per-Gaussian records (xy, opacity, cull threshold, conic), i.e.
 * a blend workspace that gg_blend_fwd_pair_packed takes as it is. */
size_t gg_view_fwd_workspace(int num_points);
int gg_view_fwd(int num_points, const float *means, const float *log_scales, const float *quats, const float *opacities,
                const float *cam_pos, const float *viewmat, const float *projmat, float fx, float fy, float cx, float cy,
                int img_height, int img_width, int tiles_x, int tiles_y, float clip_thresh, float *scales, float *quats_n,
                float *opac, float *viewdirs, float *normals, int32_t *axis, float *xys, float *depths, int32_t *radii,
                float *conics, int32_t *num_tiles_hit, int64_t *num_intersects_out, void *parts, size_t parts_bytes,
                void *records, size_t records_bytes, gg_stream_t stream);

/* ---- quat_to_rotmat ------------------------------------------------------------------------
 * Replace gsplat `_torch_impl.quat_to_rotmat` (differentiable torch code there: ~35 elementwise
 * launches forward, ~70 backward; reference call sites gaussian_splatting.py:516,614 — the
 * normals rendered at :772-784 — and scripts/update.py:204,229).  quats (N,4) wxyz, normalised
 * as q / max(|q|, 1e-12); rot (N,3,3) row-major.  bwd: v_quats = d<rot, v_rot>/d quats, through
 * the normalisation. */
int gg_quat_to_rotmat_fwd(int num_points, const float *quats, float *rot, gg_stream_t stream);
int gg_quat_to_rotmat_bwd(int num_points, const float *quats, const float *v_rot, float *v_quats,
                          gg_stream_t stream);

/* ---- caller-side activations of one view ----------------------------------------
 * One kernel each way for what the reference's get_outputs does with torch elementwise ops before it
 * calls the rasterizer: exp(scales) (gaussian_splatting.py:701), quats / |quats| (:703),
 * sigmoid(opacities) (:742, once instead of four times), view directions (:727-728) and the
 * smallest-axis normals (:605-619 via quat_to_rotmat).  `axis` (N) is the argmin index, kept for the
 * backward.  Gradients: v_log_scales, v_quats (both the normalisation and the normal path), v_opacities
 * (logits); means get no gradient here (viewdirs are detached in the reference). */
int gg_activate_fwd(int num_points, const float *means, const float *log_scales, const float *quats,
                    const float *opacities, const float *cam_pos, float *scales, float *quats_n,
                    float *opac, float *viewdirs, float *normals, int32_t *axis, gg_stream_t stream);
int gg_activate_bwd(int num_points, const float *quats, const float *scales, const float *opac,
                    const int32_t *axis, const float *v_scales, const float *v_quats_n,
                    const float *v_opac, const float *v_normals, float *v_log_scales, float *v_quats,
                    float *v_opacities, gg_stream_t stream);
/* gg_activate_bwd_ex: v_opac entries v_opac_stride floats apart (column 5 of the blend backward's record, read in
 * place); accumulate != 0: v_log_scales, v_quats, v_opacities are added to (registered gradient buffers). */
int gg_activate_bwd_ex(int num_points, const float *quats, const float *scales, const float *opac,
                       const int32_t *axis, const float *v_scales, const float *v_quats_n, const float *v_opac,
                       int v_opac_stride, const float *v_normals, float *v_log_scales, float *v_quats,
                       float *v_opacities, int accumulate, gg_stream_t stream);

/* ---- binning -------------------------------------------------------------------------------
 * Together replace gsplat `compute_cumulative_intersects` + `bin_and_sort_gaussians`
 * (`_C.map_gaussian_to_intersects`, torch.sort, `_C.get_tile_bin_edges`) that every
 * Rasterize*.forward runs (gaussian_splatting.py:735,747,759,773).
 *
 * gg_count_intersects: *num_intersects_out (device int64) = sum(num_tiles_hit). */
size_t gg_count_workspace(int num_points);
int gg_count_intersects(int num_points, const int32_t *num_tiles_hit,
                        int64_t *num_intersects_out, void *ws, size_t ws_bytes,
                        gg_stream_t stream);

/* gg_bin_sort: given I = sum(num_tiles_hit) (read back by the caller), writes
 *   gaussian_ids_sorted (I,)  — Gaussian ids, tile-major, near-to-far, ties by ascending id:
 *                               exactly the order of the reference's sorted int64 keys
 *                               (tile_id << 32 | depth bits);
 *   tile_bins (tiles_x*tiles_y, 2) — [start,end) of each tile in that list, (0,0) if empty;
 *   isect_tile_sorted (I,) optional (may be NULL) — the tile id of every sorted entry.
 * Tile grids up to 1023 x 1023 (images up to 16 368 pixels a side): a Gaussian's tile box travels through the depth
 * sort in one 32-bit word (round 4); larger grids are rejected with GG_ERR_INVALID_ARG.  Workspace: ~44 bytes per Gaussian
 * + 12 bytes per list entry, 16-byte aligned (it holds 16-byte records and 64-bit pairs) in gg_bin_sort, gg_bin_sort_dev
 * and gg_bin_sort_dev_ex; a misaligned ws is refused with GG_ERR_INVALID_ARG before any launch. */
size_t gg_bin_sort_workspace(int num_points, int64_t num_intersects);
int gg_bin_sort(int num_points, int64_t num_intersects, const float *xys, const float *depths,
                const int32_t *radii, const int32_t *num_tiles_hit, int tiles_x, int tiles_y,
                int32_t *gaussian_ids_sorted, int32_t *tile_bins, int32_t *isect_tile_sorted,
                void *ws, size_t ws_bytes, gg_stream_t stream);

/* gg_bin_sort_dev: the same without the host knowing the count.  `capacity` sizes the outputs, the
 * workspace (gg_bin_sort_workspace(num_points, capacity)) and the launches; the kernels read the
 * actual count from *num_intersects_dev (what gg_count_intersects wrote, same stream) and process
 * min(count, capacity) entries.  The caller reads the count back later (asynchronously) and, in the
 * rare case count > capacity (lists truncated), calls again with a larger capacity.  Removes the one
 * host<->device round trip per view the reference has at this point (`.item()`). */
/* gg_bin_sort_status: kept for ABI stability.  Up to round 3 the offsets scan waited on other workgroups inside its
 * launch and a wait that gave up was reported here; since round 4 no binning kernel waits on another workgroup (the
 * offsets come out of the depth-bucket kernels), so there is nothing to report: the call synchronises the stream and
 * returns GG_OK. */
int gg_bin_sort_status(int num_points, int64_t num_intersects, const void *ws, size_t ws_bytes, gg_stream_t stream);
int gg_bin_sort_dev(int num_points, int64_t capacity, const int64_t *num_intersects_dev,
                    const float *xys, const float *depths, const int32_t *radii,
                    const int32_t *num_tiles_hit, int tiles_x, int tiles_y,
                    int32_t *gaussian_ids_sorted, int32_t *tile_bins, int32_t *isect_tile_sorted,
                    void *ws, size_t ws_bytes, gg_stream_t stream);
/* gg_bin_sort_dev_ex: the same, with the partial minima / maxima of the visible Gaussians' depth bits handed over
 * (range_parts pairs, e.g. gg_view_fwd's `parts` arrays 1 and 2): the depth buckets' own pass over depths / radii is not
 * run.  range_parts 0: gg_bin_sort_dev. */
int gg_bin_sort_dev_ex(int num_points, int64_t capacity, const int64_t *num_intersects_dev, const float *xys,
                       const float *depths, const int32_t *radii, const int32_t *num_tiles_hit, int tiles_x, int tiles_y,
                       int32_t *gaussian_ids_sorted, int32_t *tile_bins, int32_t *isect_tile_sorted, void *ws,
                       size_t ws_bytes, const uint32_t *depth_bits_min, const uint32_t *depth_bits_max, int range_parts,
                       gg_stream_t stream);

/* ---- alpha blending ----------------------------------------------------------------------
 * gg_blend_fwd replaces gsplat `_C.rasterize_forward` (C=3) and `_C.nd_rasterize_forward`
 * (any C >= 1).  colors (N,C), opacity (N,) or (N,1), background (C,), out_img (H,W,C),
 * final_Ts (H,W), final_idx (H,W).  tile_bins (tiles, 2) int32, 4-byte aligned like every int32 array here (a range's two
 * ends are read as two ints).  ws: gg_blend_workspace(num_points) bytes, 16-byte aligned (the walks read a
 * Gaussian's packed 32-byte record as two 16-byte loads) — for every entry that takes it: gg_blend_fwd, gg_blend_fwd_pair,
 * gg_blend_fwd_pair_fast, gg_blend_fwd_pair_packed, gg_blend_bwd, gg_blend_bwd_pair, gg_blend_bwd_deterministic,
 * gg_blend_votes and gg_blend_hits.  A misaligned ws is refused with GG_ERR_INVALID_ARG ("ws" in gg_last_error())
 * before any launch. */
size_t gg_blend_workspace(int num_points);
int gg_blend_fwd(int channels, int num_points, int img_height, int img_width,
                 const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                 const float *conics, const float *colors, const float *opacity,
                 const float *background, float *out_img, float *final_Ts, int32_t *final_idx,
                 void *ws, size_t ws_bytes, gg_stream_t stream);

/* gg_blend_fwd_pair: gg_blend_fwd of TWO colour arrays over the same Gaussians — colors (N, channels >= 32)
 * into out_img and colors2 (N, channels2 <= 8) into out_img2 — where the second array is blended in the
 * same walk as the first 32-channel chunk of the first (its colours ride in the LDS record, 8 more fma
 * per Gaussian on the VALU while the matrix pipe does the 32 channels).  What `ops.RasterizeSegments`
 * uses for feature | rgb+depth+normal: one forward walk per view instead of two.  Images are bit-identical
 * to two gg_blend_fwd calls. */
int gg_blend_fwd_pair(int channels, int channels2, int num_points, int img_height, int img_width,
                      const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                      const float *conics, const float *colors, const float *colors2,
                      const float *opacity, const float *background, const float *background2,
                      float *out_img, float *out_img2, float *final_Ts, int32_t *final_idx, void *ws,
                      size_t ws_bytes, gg_stream_t stream);

/* gg_blend_fwd_pair_fast (round 4): the same call on the batched kernel — the survivors of a quadrant's cull queued to
 * batches of 32, alpha T written to a slab, ONE product OUT[64 pixels x 48 channels] += VIS[64 x 32] COL[32 x 48] per
 * batch on v_mfma_f32_16x16x32_f16 with fp16 two-piece operands scaled by powers of two (csrc/blend2.hip
 * blend2_fwd_batch_kernel).  final_Ts, final_idx and every alpha / stop decision are the exact kernel's, bit for bit (the
 * walk's arithmetic is unchanged); the IMAGES agree with gg_blend_fwd_pair to fp32 rounding — |difference| <=
 * ~1e-6 (1 + |value|) for colours of ordinary range; per channel and batch the error is bounded by 2^-22 of the batch's
 * largest |colour| times the pixel's sum of alpha T — not bit for bit (the exact kernel sums in list order).  Needs
 * channels % 4 == 0 and 16-byte aligned out_img / background; otherwise it runs the exact kernel.  What gsplat computes
 * here is a CUDA fma chain with __expf (rasterize_forward / nd_rasterize_forward): no summation order that could be
 * matched bit for bit on either kernel. */
int gg_blend_fwd_pair_fast(int channels, int channels2, int num_points, int img_height, int img_width,
                           const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                           const float *conics, const float *colors, const float *colors2,
                           const float *opacity, const float *background, const float *background2,
                           float *out_img, float *out_img2, float *final_Ts, int32_t *final_idx, void *ws,
                           size_t ws_bytes, gg_stream_t stream);
/* gg_blend_fwd_pair (fast == 0) / gg_blend_fwd_pair_fast (fast != 0) on a workspace that already holds the packed
 * records of these Gaussians — gg_view_fwd's `records`, or the workspace of an earlier forward over the same xys /
 * conics / opacity: the packing pass over the Gaussians is not run.  The backward entries take that workspace as
 * always. */
int gg_blend_fwd_pair_packed(int channels, int channels2, int num_points, int img_height, int img_width,
                             const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *colors,
                             const float *colors2, const float *background, const float *background2, float *out_img,
                             float *out_img2, float *final_Ts, int32_t *final_idx, void *ws, size_t ws_bytes, int fast,
                             gg_stream_t stream);

/* gg_blend_bwd replaces gsplat `_C.rasterize_backward` / `_C.nd_rasterize_backward`.
 * v_xy (N,2), v_conic (N,3), v_colors (N,C), v_opacity (N,) are fully written.
 * ws_from_forward != 0: `ws` is the very workspace the matching gg_blend_fwd call (same xys, conics,
 * opacity) ran with, untouched since — its packed per-Gaussian records are reused instead of being
 * packed again (gsplat's backward re-reads xys/conics/opacities itself; this saves one pass).
 * geom_stride / color_stride: floats between consecutive Gaussians in v_xy, v_conic, v_opacity /
 * in v_colors; 0 = the dense arrays above.  geom_stride >= 6 means ONE interleaved record per
 * Gaussian, {xy.x, xy.y, conic a, b, c, opacity[, colours]}: v_conic = v_xy + 2, v_opacity =
 * v_xy + 5 (and v_colors = v_xy + 6 with color_stride = geom_stride when the colours are part of
 * it).  The kernels add with float atomics; an interleaved record puts all of a Gaussian's
 * atomics of one instruction on one cache line instead of four.
 * Who owns the padding: with a stride the call owns num_points * stride floats starting at the row pointer — v_xy for
 * geom_stride, v_colors for color_stride (v_colors2 for color_stride2 in gg_blend_bwd_pair) — and, unless the matching
 * GG_BWD_ACCUMULATE_* flag is set, CLEARS ALL of them before it adds, the stride - width floats of padding behind every
 * row included, the last row's too.  A row pointer that is not the start of such a span (a column slice of a wider
 * array that starts at a non-zero column: the last row's padding would lie past the array's end) is the caller's
 * error.  A v_colors / v_colors2 inside the interleaved record (v_xy + 6, stride geom_stride) is part of the
 * record's span and is cleared with it. */
int gg_blend_bwd(int channels, int num_points, int img_height, int img_width,
                 const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                 const float *conics, const float *colors, const float *opacity,
                 const float *background, const float *final_Ts, const int32_t *final_idx,
                 const float *v_out_img, float *v_xy, float *v_conic, float *v_colors,
                 float *v_opacity, int geom_stride, int color_stride, void *ws, size_t ws_bytes,
                 int flags, gg_stream_t stream);
#define GG_BWD_WS_FROM_FORWARD 1
#define GG_BWD_ACCUMULATE_COLORS 2
#define GG_BWD_ACCUMULATE_GEOM 4

/* gg_blend_bwd_pair: the backward of gg_blend_fwd_pair — colors (N, channels >= 32) with v_out_img and colors2
 * (N, channels2 <= 8) with v_out_img2 — in ONE walk of the tile lists for the first 32 channels and the second
 * array together (alpha, T and the geometry gradients are those of all channels at once; D = <colour, v_out>
 * over 40 channels and both colour-gradient products run on the matrix pipe).  v_xy, v_conic, v_opacity hold
 * the geometry gradients of BOTH arrays (what autograd would sum over two gg_blend_bwd calls); v_colors /
 * v_colors2 the colour gradients, rows color_stride / color_stride2 floats apart (0 = dense; the padding is the call's,
 * as gg_blend_bwd's paragraph on strides says).  geom_stride as
 * in gg_blend_bwd; v_colors2 = v_xy + 6 with color_stride2 = geom_stride puts the second array's gradients
 * into the interleaved record.  The second cotangent (H, W, channels2) is handed over as num_parts (1..3) images
 * of v_out_img2_channels[k] consecutive channels each (host arrays) — the caller's rgb | depth | normal cotangents
 * are read where they are, not concatenated first.
 * flags: GG_BWD_WS_FROM_FORWARD, GG_BWD_ACCUMULATE_COLORS (for v_colors). */
int gg_blend_bwd_pair(int channels, int channels2, int num_points, int img_height, int img_width,
                      const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                      const float *conics, const float *colors, const float *colors2, const float *opacity,
                      const float *background, const float *background2, const float *final_Ts,
                      const int32_t *final_idx, const float *v_out_img, const float *const *v_out_img2_parts,
                      const int *v_out_img2_channels, int num_parts, float *v_xy,
                      float *v_conic, float *v_colors, float *v_colors2, float *v_opacity, int geom_stride,
                      int color_stride, int color_stride2, void *ws, size_t ws_bytes, int flags,
                      gg_stream_t stream);

/* gg_blend_bwd_deterministic: gg_blend_bwd with bit-reproducible results.  gsplat's backward
 * (csrc/backward.cu: one atomicAdd per warp per Gaussian) and gg_blend_bwd add in whatever order the
 * hardware schedules; here the kernels store the total of every (tile-list entry, 8x8 quadrant) into a slab
 * and a second pass (stable sort of the list by Gaussian id, one wave per Gaussian) sums each Gaussian's
 * entries in list order, quadrants 0..3 inside an entry.  Same arguments and flags as gg_blend_bwd plus
 * num_intersects (length of gaussian_ids_sorted) and a second workspace of
 * gg_blend_bwd_deterministic_workspace(num_points, channels, num_intersects) bytes
 * (16 (channels + 6 ceil(channels / 32)) bytes per list entry dominate). */
size_t gg_blend_bwd_deterministic_workspace(int num_points, int channels, int64_t num_intersects);
int gg_blend_bwd_deterministic(int channels, int num_points, int img_height, int img_width,
                               const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                               const float *conics, const float *colors, const float *opacity,
                               const float *background, const float *final_Ts, const int32_t *final_idx,
                               const float *v_out_img, float *v_xy, float *v_conic, float *v_colors,
                               float *v_opacity, int geom_stride, int color_stride, void *ws, size_t ws_bytes,
                               int flags, int64_t num_intersects, void *det_ws, size_t det_ws_bytes,
                               gg_stream_t stream);

/* gg_blend_votes: the transpose of the blend.  For every Gaussian, the blend weight with which the forward walk
 * blended it into the pixels of each label, as an integer sum: what lifts a 2-D label image (a segmenter's mask, a
 * thresholded relevancy image) onto the Gaussians, occlusion included (a hidden Gaussian has no weight).
 *
 *   vis(p, g)    the value by which the exact forward walk (gg_blend_fwd) multiplies g's colour at pixel p, for g in
 *                the list of p's tile: alpha T when g is blended — the same sigma, gg_exp, alpha, T operations in
 *                fp32 in the same order — and 0 when sigma < 0, when alpha < 1/255, and once the walk has stopped
 *                (the Gaussian that would take T to <= 1e-4 is not blended and gets no vote);
 *   q(p, g)      (int64) trunc(vis 2^24).  The product is exact in fp32; vis <= 0.999, so q < 2^24, and a blended
 *                pair has vis >= ~3.9e-7 (alpha >= 1/255, T > 1e-4), so q >= 6;
 *   votes[g, l] += sum over the pixels p inside the image with labels[p] == l of q(p, g).
 *
 * The call ADDS to votes (N, num_labels) int64, 8-byte aligned: the caller zeroes it once and accumulates view after
 * view.  labels (H, W) bytes, any alignment; a pixel whose label is >= num_labels (255: "ignore") takes part in no
 * sum.  Integer additions commute, so the result is a pure function of the inputs: identical bits from run to run,
 * whatever the schedule.  A vote is exact as a double below 2^53, i.e. ~5e8 fully opaque pixel hits.
 * num_labels: 1..255.  ws: gg_blend_workspace(num_points) bytes; ws_packed != 0: ws already holds these Gaussians'
 * packed records (the workspace of a gg_blend_fwd over the same xys / conics / opacity, or gg_view_fwd's `records`),
 * as GG_BWD_WS_FROM_FORWARD says for the backward — xys, conics and opacity are then not read.  Null or invalid
 * arguments: GG_ERR_INVALID_ARG with the argument's name in gg_last_error(), before any launch.  num_points == 0
 * or empty tile lists: GG_OK, nothing is written. */
int gg_blend_votes(int num_labels, int num_points, int img_height, int img_width,
                   const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                   const float *conics, const float *opacity, const uint8_t *labels /* (H, W) */,
                   int64_t *votes /* (N, num_labels) */, void *ws, size_t ws_bytes, int ws_packed,
                   gg_stream_t stream);

/* gg_blend_hits: what is under a pixel.  For every pixel p inside the image the list of p's tile is walked exactly
 * as gg_blend_fwd walks it — the same sigma, gg_exp, alpha, T operations in fp32 in the same order, the same
 * sigma < 0 and alpha < 1/255 rules, the same stop (the entry that would take T to <= 1e-4 is not blended and ends
 * the walk).  With vis = alpha T of a blended entry and T_after = T (1 - alpha):
 *
 *   hit_idx[p]   (int32) the Gaussian id of the first blended entry with T_after <= t_hit (fp32 comparison), -1 if
 *                there is none: the "median" Gaussian of the pixel for t_hit = 0.5;
 *   top_idx[p]   (int32) the id of the blended entry with the largest vis, the earliest in list order on equal
 *                values (strict >); -1 if nothing was blended;
 *   top_vis[p]   (float) that vis, or 0;
 *   count[p]     (int32) the number of blended entries.
 *
 * Every output is a pure function of the inputs: identical bits from run to run.  A pixel has a hit iff the
 * forward's final_T there is <= t_hit.  GG_T_EPS (1e-4) < t_hit < 1.  hit_idx is required; top_idx, top_vis and
 * count are given together or all NULL (the walk then leaves a pixel at its hit).  Each output (H, W), 4-byte
 * aligned.  The call OVERWRITES: every pixel inside the image is written exactly once, pixels of tiles with empty
 * lists included (-1, -1, 0, 0); with num_points == 0 every pixel gets these defaults and the lists are not read.
 * ws, ws_packed: as in gg_blend_votes.  Null, misaligned or out-of-range arguments: GG_ERR_INVALID_ARG with the
 * argument's name in gg_last_error(), before any launch. */
int gg_blend_hits(int num_points, int img_height, int img_width, const int32_t *gaussian_ids_sorted,
                  const int32_t *tile_bins, const float *xys, const float *conics, const float *opacity, float t_hit,
                  int32_t *hit_idx, int32_t *top_idx, float *top_vis, int32_t *count, void *ws, size_t ws_bytes,
                  int ws_packed, gg_stream_t stream);

/* ---- feature up-projection MLP ------------------------------------------------
 * Replaces the forward of the reference's `MLP(32, 512, hidden_list=[128])` module
 * (nerfstudio/models/gaussian_splatting.py:198-213; `self.fea_up`, called on every pixel of the
 * rendered feature image at nerfstudio/pipelines/base_pipeline.py:408):
 *     y = relu(x @ w1^T + b1) @ w2^T + b2,  x (num_rows, in_dim), w1 (128, in_dim), b1 (128),
 *     w2 (out_dim, 128), b2 (out_dim), y (num_rows, out_dim), all fp32 row-major (torch Linear
 *     layout).  hidden_dim must be 128, in_dim 8/16/32/64/128, out_dim a multiple of 32.  x, y, w1 and w2 are
 *     16-byte aligned (rows of x, y and of the weights are read and written four floats at a time), b1 and b2
 *     4-byte; a misaligned one is refused with GG_ERR_INVALID_ARG, its name in gg_last_error(), before any launch. */
int gg_mlp_fwd(int64_t num_rows, int in_dim, int hidden_dim, int out_dim, const float *x,
               const float *w1, const float *b1, const float *w2, const float *b2, float *y,
               gg_stream_t stream);

/* Tuning entry (round 3): how many 32-channel blocks of a wide colour array one forward walk takes — in the pair walk
 * of gg_blend_fwd_pair (1, 2 or 4) and in the walks of the remaining chunks / of gg_blend_fwd (1..4).  Images are
 * bit-identical for every setting; returns the previous pair value.  Defaults: see csrc/blend.hip. */
int gg_debug_set_fwd_blocks(int pair_blocks, int chunk_blocks);

/* The same forward four times faster (round 3): both layers as products of fp16 two-piece operands scaled by powers of
 * two on v_mfma_f32_16x16x32_f16 — as accurate against a double-precision sum as the fp32 matrix instruction
 * (tools/check_f16split.hip), but not gg_mlp_fwd's summation order: the two agree to ~1e-6 of the largest output
 * (tests/test_gpu_parity.py), not bit for bit.  in_dim 32 / 64 / 128, out_dim a multiple of 16 (<= 3968: LDS); `ws`:
 * gg_mlp_fwd_fast_workspace(in_dim, 128, out_dim) bytes, 16-byte aligned, rewritten by every call (the packed
 * weights: 0.3 MB at out_dim 512).  x and y 16-byte aligned; w1, w2, b1, b2 4-byte (unlike gg_mlp_fwd: the packing
 * pass reads the weights float by float).  What the reference runs here is cuBLAS behind nn.Linear
 * (gaussian_splatting.py:198-213): no summation order to match on that side. */
size_t gg_mlp_fwd_fast_workspace(int in_dim, int hidden_dim, int out_dim);
int gg_mlp_fwd_fast(int64_t num_rows, int in_dim, int hidden_dim, int out_dim, const float *x,
                    const float *w1, const float *b1, const float *w2, const float *b2, float *y,
                    void *ws, size_t ws_bytes, gg_stream_t stream);

/* Backward of the same module (the reference evaluates fea_up on 1000 sampled pixels per training
 * step, gaussian_splatting.py:917): g = dL/dy (num_rows, out_dim) -> v_x (num_rows, in_dim), v_w1 (128,
 * in_dim), v_b1 (128), v_w2 (out_dim, 128), v_b2 (out_dim), all fully written.  in_dim 8..128, out_dim
 * <= 1024.  Sized for 10^3-10^5 rows (one launch, row tiles through LDS, float atomics for the weight
 * gradients); for the 1.9 M-pixel render pass a library GEMM is the right tool. */
int gg_mlp_bwd(int64_t num_rows, int in_dim, int hidden_dim, int out_dim, const float *x,
               const float *w1, const float *b1, const float *w2, const float *g, float *v_x,
               float *v_w1, float *v_b1, float *v_w2, float *v_b2, gg_stream_t stream);

/* ---- cosine-similarity loss --------------------------------------------------------
 * Replace the reference's `cosine_similarity_loss` (gaussian_splatting.py:113-118; contrastive feature
 * loss over 800 pixel pairs per mask :909-914, `up_loss` :917-918) for a, b stored (num_points,
 * channels): sim_m = <a_m, b_m> / (max(|a_m|, 1e-12) max(|b_m|, 1e-12)); *sim_sum = sum_m sim_m (the
 * loss is 1 - sim_sum / num_points).  sim / norm_a / norm_b (num_points,) are kept for the backward,
 * which takes v_loss from device memory (1 float) and writes v_a, v_b (num_points, channels). */
int gg_cosine_loss_fwd(int64_t num_points, int channels, const float *a, const float *b, float *sim,
                       float *norm_a, float *norm_b, float *sim_sum, gg_stream_t stream);
int gg_cosine_loss_bwd(int64_t num_points, int channels, const float *a, const float *b,
                       const float *sim, const float *norm_a, const float *norm_b,
                       const float *v_loss, float *v_a, float *v_b, gg_stream_t stream);

/* ---- image-space main loss (SURVEY 8f-4 tail) ---------------------------------------------------------
 * Replace, in the reference's get_loss_dict (gaussian_splatting.py:882-885, :931; self.ssim :284 =
 * pytorch_msssim.SSIM(data_range=1.0, size_average=True, channel=3), requirements.txt:199):
 *     Ll1 = abs(gt[valid] - rgb[valid]).mean();  gt[~valid] = 0;  rgb[~valid] = 0;
 *     main_loss = (1 - ssim_lambda) * Ll1 + ssim_lambda * (1 - ssim(gt, rgb))
 * rgb, gt (H, W, 3) fp32, rgb with rgb_pixel_stride >= 3 floats between pixels (a channel slice of a wider image
 * is read in place); valid (H, W) bytes or NULL (all valid).  out3 = {main_loss, Ll1, ssim} (device).
 * The forward leaves what the backward needs (three derivative maps per channel, the valid count) in `ws`
 * (gg_image_loss_workspace bytes); the backward takes the SAME workspace, untouched, and v_main (1 float, device)
 * and writes v_rgb (H, W, 3) = v_main * d main_loss / d rgb, zero at invalid pixels.  H, W >= 11.
 * rgb, gt, out3, v_main and v_rgb 4-byte aligned, valid any address; ws 256-byte aligned, of any content on entry of
 * the forward; the backward only reads it. */
size_t gg_image_loss_workspace(int img_height, int img_width);
int gg_image_loss_fwd(int img_height, int img_width, const float *rgb, int rgb_pixel_stride, const float *gt,
                      const uint8_t *valid, float ssim_lambda, float *out3, void *ws, size_t ws_bytes,
                      gg_stream_t stream);
int gg_image_loss_bwd(int img_height, int img_width, const float *rgb, int rgb_pixel_stride, const float *gt,
                      const uint8_t *valid, float ssim_lambda, const float *v_main, const void *ws, size_t ws_bytes,
                      float *v_rgb, gg_stream_t stream);

/* Depth and normal losses of get_loss_dict (gaussian_splatting.py:879-880) over the pixels where mask != 0:
 *     depth_loss  = F.l1_loss(depth[m], gt_depth[m])
 *     normal_loss = 0.5 F.mse_loss(normal[:, m], gt_normal[:, m]) + 0.5 cosine_similarity_loss(normal[:, m], gt_normal[:, m])
 * depth / gt_depth: element p at base[p * stride]; normal / gt_normal: channel c of pixel p at
 * base[p * pixel_stride + c * channel_stride] (the model's images are pixel-major, the reference's ground truth
 * channel-major).  out3 = {depth_loss, normal_loss, number of masked pixels} (device).  The backward takes the
 * forward's workspace (gg_geom_loss_workspace bytes), the two loss cotangents from device memory (1 float each) and
 * writes dense v_depth (num_pixels,), v_normal (num_pixels, 3), zero outside the mask.
 * Every fp32 array 4-byte aligned, mask any address; ws 256-byte aligned, of any content on entry of the forward; the
 * backward only reads it. */
size_t gg_geom_loss_workspace(void);
int gg_geom_loss_fwd(int64_t num_pixels, const float *depth, int depth_stride, const float *gt_depth,
                     int gt_depth_stride, const float *normal, int normal_pixel_stride, int normal_channel_stride,
                     const float *gt_normal, int gt_normal_pixel_stride, int gt_normal_channel_stride,
                     const uint8_t *mask, float *out3, void *ws, size_t ws_bytes, gg_stream_t stream);
int gg_geom_loss_bwd(int64_t num_pixels, const float *depth, int depth_stride, const float *gt_depth,
                     int gt_depth_stride, const float *normal, int normal_pixel_stride, int normal_channel_stride,
                     const float *gt_normal, int gt_normal_pixel_stride, int gt_normal_channel_stride,
                     const uint8_t *mask, const float *v_depth_loss, const float *v_normal_loss, const void *ws,
                     size_t ws_bytes, float *v_depth, float *v_normal, gg_stream_t stream);

/* ---- densification, culling and the optimizer step ---------------------------------
 * The per-Gaussian optimizer-side work of the reference model, which it does with torch indexing,
 * torch.cat and one torch.optim.Adam per parameter group:
 *   statistics   GaussianSplattingModel.after_train          gaussian_splatting.py:373-393
 *   masks        refinement_after :412-421,:430-431 ; cull_gaussians :485-496
 *   cull         cull_gaussians :497-502 + remove_from_optim :333-350
 *   split / dup  split_gaussians :504-531, dup_gaussians :533-546, torch.cat :434-439, dup_in_optim :352-371
 *   Adam         Optimizers.optimizer_step_all               engine/optimizers.py:158-171
 * Row arrays are (num_rows, row_floats) fp32, contiguous; byte masks are 0 / non-0. */
typedef struct {
    const float *src; /* (num_rows, row_floats) */
    float *dst;       /* destination array (capacity: see each function) */
    int row_floats;
    int kind; /* GG_ROWS_* (gg_densify_rows only; ignored by gg_compact_rows) */
} gg_row_array_t;
#define GG_ROWS_COPY 0     /* appended rows copy their source row                                    */
#define GG_ROWS_MEANS 1    /* split samples: R(q/|q|) (exp(scale) * z) + mean  (:509-516); 3 floats  */
#define GG_ROWS_SCALES 2   /* split sources and samples: log(exp(scale) / size_fac) (:524-526); 3 floats */
#define GG_ROWS_ZERO_NEW 3 /* Adam moments: appended rows are zero (dup_in_optim :352-371)            */

/* bytes of scratch for gg_mask_scan / gg_compact_rows over num_rows rows */
size_t gg_rows_workspace(int num_rows);
/* ranks[i] = number of selected rows before i (selected = mask != 0, or == 0 with invert);
 * *total_out (device int64) = number selected.  One launch (decoupled look-back scan). */
int gg_mask_scan(int num_rows, const uint8_t *mask, int invert, int32_t *ranks, int64_t *total_out,
                 void *ws, size_t ws_bytes, gg_stream_t stream);
/* Stream compaction: rows with deleted_mask == 0 of every array move, in order, to the front of its
 * dst (capacity num_rows rows; src != dst).  Replaces `t[~culls]` on the 6 parameters and the 12
 * moment tensors (<= 24 arrays, one launch).  *num_kept_out (device int64) = rows kept.
 * `arrays` is a HOST array of descriptors. */
int gg_compact_rows(int num_rows, const uint8_t *deleted_mask, int num_arrays,
                    const gg_row_array_t *arrays, int64_t *num_kept_out, void *ws, size_t ws_bytes,
                    gg_stream_t stream);
/* Append rows: dst = [num_rows old | num_samples x num_split split samples (sample-major) | num_dup
 * duplicates]; dst capacity num_rows + num_samples*num_split + num_dup rows.  split_ranks / dup_ranks
 * and the counts come from gg_mask_scan; samples (num_samples*num_split, 3) are the caller's N(0,1)
 * draws (torch.randn, :508); means / scales / quats are the CURRENT parameter arrays. */
int gg_densify_rows(int num_rows, const uint8_t *split_mask, const uint8_t *dup_mask,
                    const int32_t *split_ranks, const int32_t *dup_ranks, int num_split, int num_dup,
                    int num_samples, const float *samples, float size_fac, const float *means,
                    const float *scales, const float *quats, int num_arrays,
                    const gg_row_array_t *arrays, gg_stream_t stream);
/* after_train (:373-393).  first != 0: the accumulators are (re)initialised as the reference does
 * when they are None (grad norms of every Gaussian, counts 1, max_2dsize 0 then max over visible). */
int gg_densify_stats(int num_points, const float *xys_grad, const int32_t *radii, int max_image_dim,
                     int first, float *grad_norm_accum, float *vis_counts, float *max_2dsize,
                     gg_stream_t stream);
/* split / dup masks of refinement_after (:412-421, :430-431); scales are log-scales (N,3).  The duplicate test
 * runs on the scales split_gaussians has already shrunk in place (log(exp(s) / size_fac) for the split rows,
 * :524-526), as the reference's does: a Gaussian can be in both masks. */
int gg_densify_masks(int num_points, const float *grad_norm_accum, const float *vis_counts,
                     const float *max_2dsize, const float *scales, int max_image_dim,
                     float densify_grad_thresh, float densify_size_thresh, float split_screen_size,
                     int use_screen_size, float size_fac, uint8_t *split_mask, uint8_t *dup_mask,
                     gg_stream_t stream);
/* cull mask of cull_gaussians (:485-496); opacities are logits (N,), scales log-scales (N,3). */
int gg_cull_mask(int num_points, const float *opacities, const float *scales, const float *max_2dsize,
                 float cull_alpha_thresh, float cull_scale_thresh, float cull_screen_size,
                 int use_scale, int use_screen_size, uint8_t *deleted_mask, gg_stream_t stream);

/* One Adam step (torch.optim.Adam, amsgrad off) of up to GG_ADAM_MAX_GROUPS parameter arrays in ONE
 * launch; every group has its own hyper-parameters and step count, as the reference's one optimizer
 * per group does (method_configs.py:618-660: eps 1e-15, lr 1.6e-4 ... 0.05).  step is the step
 * number being taken (>= 1).  16-byte aligned arrays take the float4 path.  zero_grad != 0 clears the gradients
 * in the same pass.  `groups` is a HOST array. */
#define GG_ADAM_MAX_GROUPS 8
typedef struct {
    float *param, *grad, *exp_avg, *exp_avg_sq;
    int64_t numel;
    double lr, beta1, beta2, eps, weight_decay;
    int64_t step;
} gg_adam_group_t;
int gg_adam_step(int num_groups, const gg_adam_group_t *groups, int zero_grad, gg_stream_t stream);

/* ---- scene update after a grasp (reference nerfstudio/scripts/update.py:141-158, 217-240, 293-328) -----------
 * One pass over num_points Gaussians: select every Gaussian whose mean lies inside a convex hull and, when rt is
 * given, move the selected ones rigidly, in place.
 *   planes: num_planes x (n0, n1, n2, d) fp64, outward normals (Qhull's `equations`); num_planes >= 4, no upper
 *           limit.  Mean x is inside iff every plane has v = ((n0*x0 + n1*x1) + n2*x2) + d <= tol, evaluated in
 *           fp64 in that order, x widened exactly from fp32; a NaN / inf mean is outside (!(v <= tol)).
 *   rt:     HOST array of 12 floats, [R | t] row-major 3 x 4, or NULL (select only: means / quats untouched,
 *           quats may be NULL).
 *   For selected rows, with rt: means' = ((R_i0*x0 + R_i1*x1) + R_i2*x2) + t_i (fp32, in that order);
 *           quats' = Shepperd(R . quat_to_rotmat(q)), where quat_to_rotmat is gg_quat_to_rotmat_fwd's bit for bit,
 *           the product is fp32, and the quaternion comes from the branch of the largest of tr, m00, m11, m22 (the
 *           tr branch is the reference's rotmat_to_quat expression by expression), sign set so that w >= 0, not
 *           renormalised.  Rows not selected are never written.
 *   mask:      (num_points) uint8, 1 = selected, fully written.
 *   count_out: DEVICE int64, the number of selected rows (zeroed by the call, so num_points == 0 leaves 0).
 * means 4-byte, planes and count_out 8-byte, quats 16-byte aligned; mask any address.  No workspace. */
int gg_hull_edit(int num_points, float *means, float *quats, int num_planes, const double *planes, double tol,
                 const float *rt, uint8_t *mask, int64_t *count_out, gg_stream_t stream);

/* ---- the moved Gaussians' colour lobes (PARITY "Scene update") ---------------------------------------
 * Rotates the spherical-harmonic coefficients of the selected rows, in place: band l (coefficients lo = l^2 ..
 * hi - 1, hi = (l + 1)^2) of every channel is multiplied by that band's (2l+1) x (2l+1) matrix D_l.
 *   coeffs: (num_points, num_bases, 3) fp32, 4-byte aligned.  num_bases in {1, 4, 9, 16, 25}; with 1 (band 0 only)
 *           the call returns without launching.
 *   mask:   (num_points) uint8 on the device, non-zero = selected (gg_hull_edit's mask as it is), or NULL: every row.
 *   bands:  HOST array, D_1, D_2, ... of the bands num_bases has, each row-major, concatenated: 9, 34, 83 or 164
 *           floats (sh_rotation.pack_bands).
 *   For a selected row, band l >= 1, output a and channel ch, in fp32, every product and every sum rounded, b
 *   ascending, no contraction:
 *           out[a][ch] = ((D[a][lo] c[lo][ch] + D[a][lo+1] c[lo+1][ch]) + ...) + D[a][hi-1] c[hi-1][ch]
 *   with every c the row's value before the call.  Band 0 and rows not selected are neither read nor written.
 * One launch, no workspace, nothing waits on the host. */
int gg_sh_rotate(int num_points, int num_bases, float *coeffs, const uint8_t *mask, const float *bands,
                 gg_stream_t stream);

/* ---- the rigid move as a differentiable operator (PARITY "Object pose refinement") ------------------
 * gg_rigid_fwd moves the selected rows by a pose held on the DEVICE (it is an autograd tensor inside an optimiser
 * loop: no host read-back); gg_rigid_bwd is its vector-Jacobian product, per row and for the pose.
 *   rt:   12 floats, [R | t] row-major 3 x 4.   qt: 4 floats, wxyz, the quaternion of R (keeping it consistent with
 *         R is the caller's job).
 *   mask: (num_points) uint8, non-zero = selected (gg_hull_edit's mask as it is), or NULL: every row.
 * Forward, a selected row, every fp32 input widened to fp64, no contraction:
 *   m'_a = (float)(((R[a][0] x + R[a][1] y) + R[a][2] z) + t[a])
 *   q'   = (float)(qt (x) q), the Hamilton product: each component four fp64 products added left to right in the
 *          order of the usual expression, rounded once:
 *            w = w1 w2 - x1 x2 - y1 y2 - z1 z2      x = w1 x2 + x1 w2 + y1 z2 - z1 y2
 *            y = w1 y2 - x1 z2 + y1 w2 + z1 x2      z = w1 z2 + x1 y2 - y1 x2 + z1 w2
 *   Nothing is normalised (the renderer normalises).  A row not selected is copied byte for byte.
 * Backward, per row: selected  v_m[b] = (float)((R[0][b] g0 + R[1][b] g1) + R[2][b] g2),
 *   v_q = (float)(conj(qt) (x) g_q); not selected: the cotangent's bytes.  g_means or g_quats NULL is read as zeros.
 *   v_means and v_quats may each be NULL (both: the pose-only pass for frozen Gaussians, where a row not selected
 *   costs its mask byte only).
 * Backward, the pose: sixteen sums over the selected rows, v_rt[a][b] = sum g_a p_b (b < 3), v_rt[a][3] = sum g_a,
 *   v_qt = sum g_q (x) conj(q) (the expression above with the second operand's x, y, z negated).  Every term is
 *   fp64; one row of 16 per workgroup of 256 Gaussians by gg_block_row<16>, then one workgroup's
 *   gg_chain_sum<16, GG_SUM_CHAINS> (csrc/ordered_sum.h).  The totals are rounded to fp32 and WRITTEN (not added).
 *   No floating-point atomics: the same inputs give the same bytes, whatever ws held on entry.  num_points == 0
 *   writes sixteen zeros and nothing else (ws is not looked at).
 * Alignment: means*, g_means, v_means, rt, qt, v_rt, v_qt 4 bytes; quats*, g_quats, v_quats 16; mask 1; ws 256,
 * gg_rigid_bwd_workspace(num_points) bytes (0 for num_points < 0).  The outputs must not overlap the inputs. */
size_t gg_rigid_bwd_workspace(int num_points);
int gg_rigid_fwd(int num_points, const float *means, const float *quats, const uint8_t *mask, const float *rt,
                 const float *qt, float *means_out, float *quats_out, gg_stream_t stream);
int gg_rigid_bwd(int num_points, const float *means, const float *quats, const uint8_t *mask, const float *rt,
                 const float *qt, const float *g_means, const float *g_quats, float *v_means, float *v_quats,
                 float *v_rt, float *v_qt, void *ws, size_t ws_bytes, gg_stream_t stream);

/* ---- per-view masks of the moved object (reference scripts/project_hull.py :83-121; DESIGN 3.14, PARITY "Scene
 * update") -----------------------------------------------------------------------------------------------------------
 * For every view v and pose (0 = before, 1 = after) — a job — in fp64, no contraction:
 *   points:   q = p (before);  q_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3 (after, get_transform :8-19, :105);
 *   project:  c_r = ((E_r0 q0 + E_r1 q1) + E_r2 q2) + E_r3 with E = w2c[v] (inv(transform_matrix), :86-87, no axis
 *             flip);  u = ((fx c0) + (cx c2)) / c2,  v = ((fy c1) + (cy c2)) / c2 (project_points_3d_to_2d :21-34,
 *             distortion ignored), both truncated toward zero to int32 (`.astype(np.int32)`, :91-92);
 *   dropped:  c2 <= 0, u or v not finite, or |u| or |v| >= 2^30 (the reference keeps points behind the camera,
 *             mirrored; PARITY) — counted per job in dropped[v][pose];
 *   hull:     the exact convex hull of the kept integer points (int64 cross products), possibly empty, a point or a
 *             segment (cv2.convexHull, :36-46);
 *   fill:     pixel (row y, col x) is set iff (x, y) lies in the CLOSED hull (boundary and degenerate hulls
 *             included) — cv2.fillConvexPoly without the LINE_AA rim (PARITY);
 *   dilate:   cv2.dilate with a k x k ones kernel, anchor k / 2, pixels outside the image contribute nothing; k = 0
 *             or 1: none (get_dialated_mask :48-53);  union = before | after (finetune_mask3, :118-121);
 *   boxes:    per view and mask m (0 before, 1 after, 2 union): boxes[v][m] = rmin, rmax, cmin, cmax of the set
 *             pixels, centres[v][m] = 0.5 (rmax + rmin), 0.5 (cmax + cmin) (center1, :101-102); -1 / NaN when empty.
 * points fp64 [M][3] (device); transform: HOST array of 12 doubles, [R | t] row-major 3 x 4; intrinsics fp64 [V][4]
 * (fx, fy, cx, cy) and w2c fp64 [V][3][4] (device).  before / after / union_mask uint8 [V][H][W] (0 / 1), boxes int32
 * [V][3][4], centres fp64 [V][3][2], dropped int32 [V][2]: every element written.
 * The kept points of a job may span at most max_rows pixel rows (the row table of the hull pass); a job above that
 * makes the call return GG_ERR_UNSUPPORTED naming the smallest such view, with nothing written to the outputs.  The
 * call reads one status word back and synchronises the stream once, at its end.  Deterministic: integer work only.
 * `ws`: gg_object_masks_workspace(V, max_rows) bytes (about 12 max_rows bytes per job), 256-byte aligned; 0 is
 * returned for counts out of range.  points, intrinsics, w2c and centres 8-byte aligned, boxes and dropped 4-byte; the
 * three masks any address (when all three are 4-byte aligned and width % 4 == 0 they are written a word at a time: the
 * same bytes).  num_views == 0 writes nothing. */
#define GG_OBJMASK_MAX_VIEWS 16384
#define GG_OBJMASK_MAX_ROWS 65536
#define GG_OBJMASK_MAX_SIDE 32768
#define GG_OBJMASK_MAX_DILATE 128
size_t gg_object_masks_workspace(int num_views, int max_rows);
int gg_object_masks(int num_points, const double *points, const double *transform, int num_views,
                    const double *intrinsics, const double *w2c, int height, int width, int dilate, int max_rows,
                    uint8_t *before, uint8_t *after, uint8_t *union_mask, int32_t *boxes, double *centres,
                    int32_t *dropped, void *ws, size_t ws_bytes, gg_stream_t stream);

/* ---- language query of the feature field ------------------------------------------------------------
 * fea_up followed by the CLIP comparison, with the 512-float fea_up output never written to memory:
 *   y   = relu(x @ w1^T + b1) @ w2^T + b2 per row, as gg_mlp_fwd_fast computes it (in_dim 32 / 64 / 128, hidden 128,
 *         out_dim a multiple of 16 and at most 3968, and 2 out_dim + 129 num_queries + 256 <= 8192: LDS);
 *   s_k = (y . q_k) / max(|y|_2, 1e-12) for the num_queries rows q_k of `queries` (num_queries x out_dim, unit norm:
 *         F.normalize(y) @ q^T); the first num_positives rows are positives, the rest canonical negatives;
 *   r_p = 1 / (1 + exp(temperature (max_j s_nj - s_p))) = min_j softmax(temperature [s_p, s_nj])[0]  (LERF).
 *   sims:      num_rows x num_queries, or NULL;  relevancy: num_rows x num_positives, or NULL (needs 1 <= num_positives
 *              < num_queries).  At least one of the two.  y = 0 gives s = 0, r = 1/2; a NaN feature makes that row's
 *              outputs NaN; num_rows = 0 does nothing.  Fixed summation orders, no atomics: identical run to run.
 * x 16-byte aligned; w1, b1, w2, b2, queries, sims and relevancy 4-byte aligned; `ws`: gg_clip_query_workspace() bytes
 * (0 = shape not supported), 16-byte aligned, of any content on entry, rewritten by every call (the packed weights of
 * gg_mlp_fwd_fast). */
#define GG_QUERY_MAX 8
size_t gg_clip_query_workspace(int in_dim, int hidden_dim, int out_dim, int num_queries);
int gg_clip_query(int64_t num_rows, int in_dim, int hidden_dim, int out_dim, const float *x, const float *w1,
                  const float *b1, const float *w2, const float *b2, int num_queries, int num_positives,
                  const float *queries, float temperature, float *sims, float *relevancy, void *ws, size_t ws_bytes,
                  gg_stream_t stream);

/* ---- normal-guided grasp filtering (PARITY "Grasp filtering") --------------------------------------
 * Every grasp candidate against every oriented point, exact in fp64, with a deterministic reduction.
 *   grasps: num_grasps x 17 fp32, graspnetAPI GraspGroup rows [score, width, height, depth, R (9, row-major),
 *           t (3), object_id]; gripper frame a = R[:,0] approach, b = R[:,1] closing (fingers at -b and +b),
 *           c = R[:,2] height.
 *   points, normals: num_points x 3 fp32 (normals any sign, any length); weights: num_points fp32.  A point takes
 *           part iff p and n are finite and (double)w > min_weight.
 * Per grasp g, in fp64 from the fp32 inputs, no contraction:
 *   d_k = (double)p_k - (double)t_k;  u_j = (R[0][j] d_0 + R[1][j] d_1) + R[2][j] d_2;
 *   region:       -depth_base <= u_0 <= depth, |u_2| <= height/2, |u_1| <= width/2;
 *   finger boxes: the same u_0 / u_2 bounds, -width/2 - finger_width <= u_1 < -width/2 or
 *                 width/2 < u_1 <= width/2 + finger_width;
 *   contacts:     y_L = min u_1, y_R = max u_1 over the region, i_L / i_R the smallest indices reaching them;
 *   patches:      left: region points with u_1 <= y_L + band, right: u_1 >= y_R - band; n oriented toward its finger
 *                 (left: s = -1 if b.n > 0 else +1; right: s = -1 if b.n < 0 else +1, b.n = (b0 n0 + b1 n1) + b2 n2);
 *                 N_L = sum_L w s n, N_R = sum_R w s n in fp64, normalised;
 *   angles:       theta_L = atan2(|x cross b|, x . b) with x = -N_L/|N_L|, theta_R the same with x = N_R/|N_R|;
 *   valid:        region not empty, y_L < y_R, |N_L| > 0 and |N_R| > 0;
 *   feasible:     valid, max(theta_L, theta_R) <= atan(mu) and collision_weight <= max_collision (fp64).
 * A grasp row with a non-finite entry, width <= 0, height <= 0 or depth < -depth_base is not valid (data, not an
 * error).  Outputs, every grasp written:
 *   contact_idx int32 [M][2] (i_L, i_R; -1 when the region is empty); normals_out fp32 [M][2][3] (unit, outward;
 *   NaN when not valid); angles fp32 [M][2] (radians, NaN when not valid); region_count int32 [M];
 *   region_weight / collision_weight fp32 [M] (sum of w over the region / over both finger boxes); feasible uint8 [M].
 * depth_base, finger_width, band and mu finite and >= 0; min_weight and max_collision not NaN (+inf: no collision
 * limit).  num_grasps == 0 does nothing; num_points == 0 marks every grasp not valid.  No atomics: per-chunk
 * partials combined in a fixed order, identical run to run.  `ws`: gg_grasp_contacts_workspace() bytes, 256-byte
 * aligned (0 bytes for num_grasps == 0; 0 is also returned for counts out of range).  Every fp32 / int32 array, inputs
 * and outputs, 4-byte aligned; feasible any address. */
#define GG_GRASP_MAX (1 << 20)
#define GG_GRASP_MAX_POINTS (1 << 30)
size_t gg_grasp_contacts_workspace(int num_points, int num_grasps);
int gg_grasp_contacts(int num_points, const float *points, const float *normals, const float *weights, int num_grasps,
                      const float *grasps, double depth_base, double finger_width, double band, double mu,
                      double min_weight, double max_collision, int32_t *contact_idx, float *normals_out, float *angles,
                      int32_t *region_count, float *region_weight, float *collision_weight, uint8_t *feasible,
                      void *ws, size_t ws_bytes, gg_stream_t stream);

/* ---- grasp proposals: antipodal candidates from the oriented points (PARITY "Grasp proposals") -------
 * Every seed point against every oriented point, exact in fp64, with a deterministic reduction; the output rows
 * have the GraspGroup layout and column meaning gg_grasp_contacts reads.
 *   points, normals, weights: as for gg_grasp_contacts (normals any sign, any length); point j takes part iff p_j
 *           and n_j are finite and (double)w_j > min_weight.
 *   seeds:  num_seeds int32 indices into the points.  A seed is usable iff its index is in [0, num_points), its
 *           point takes part and n.n > 0.  Seeds may repeat.
 * Per usable seed i, p = points[i], n = normals[i], in fp64 from the fp32 inputs, no contraction, in this order:
 *   nn = (n0 n0 + n1 n1) + n2 n2
 *   per j taking part:  d_k = (double)p_jk - (double)p_k;  s = (n0 d0 + n1 d1) + n2 d2;  dd = (d0 d0 + d1 d1) + d2 d2;
 *                       in the tube iff  dd nn - s s <= (r r) nn  and  s s <= (W W) nn
 *   s_lo = min s over the tube, j_lo the smallest index reaching it; s_hi, j_hi likewise for the max; tube_count =
 *   the number of points in the tube (the seed itself is in it with s = 0);  q = s_hi - s_lo
 *   align(j) iff m_j > 0 and g_j g_j >= (min_align min_align)(nn m_j),
 *                g_j = (n0 nj0 + n1 nj1) + n2 nj2,  m_j = (nj0 nj0 + nj1 nj1) + nj2 nj2
 *   valid iff  q q >= (w0 w0) nn  and  q q <= ((W - 2c)(W - 2c)) nn  and  align(j_lo)  and  align(j_hi)
 * (r tube_radius, W max_width, w0 min_width, c clearance).  No square root or division decides anything: indices,
 * counts and valid are exact.  The farthest points along the line are the contacts, not the first hit (a trained
 * object is full of interior Gaussians); the sign of n does not matter.  For a valid seed, K = num_approach rows:
 *   b = n / sqrt(nn);  m = p + b ((s_lo + s_hi) / (2 sqrt(nn)));  span = q / sqrt(nn);  width = span + 2c
 *   v = -up;  e = v - b (b . v);  if e.e < 1e-12 (v.v): v = the coordinate axis k with the smallest |b_k| (smallest k
 *   on a tie), e recomputed;  a_0 = e / |e|;  c_0 = a_0 x b
 *   phi_k = 2 pi k / K;  a_k = cos(phi_k) a_0 + sin(phi_k) c_0;  c_k = a_k x b;  R_k = columns (a_k, b, c_k)
 *   t_k = m - (depth / 2) a_k;  score = |g_lo| |g_hi| / (nn sqrt(m_lo m_hi))
 *   row = [score, width, height, depth, R_k row-major (9), t_k (3), 0]
 * Outputs, every seed written: pair_idx int32 [S][2] (j_lo, j_hi; -1, -1 for a seed that is not usable);
 * tube_count int32 [S] (0 when not usable); span fp32 [S] (NaN when not usable); valid uint8 [S]; rows fp32
 * [S][K][17] (all NaN for a seed that is not valid).
 * tube_radius, min_width, clearance, depth finite and >= 0; max_width, height finite and > 0; 2 clearance <=
 * max_width; min_weight not NaN; min_align in [0, 1]; up: HOST array of 3 doubles, finite, not zero; num_approach in
 * 1..GG_PROPOSE_MAX_APPROACH.  num_seeds == 0 does nothing; num_points == 0 makes every seed not usable.  No atomics:
 * per-chunk extremes combined in a fixed order; the result does not depend on the launch geometry and is identical run
 * to run.  `ws`: gg_grasp_propose_workspace() bytes, 256-byte aligned (0 is returned for counts out of range).  Every
 * fp32 / int32 array, inputs and outputs, 4-byte aligned; valid any address. */
#define GG_PROPOSE_MAX_SEEDS (1 << 20)
#define GG_PROPOSE_MAX_APPROACH 64
size_t gg_grasp_propose_workspace(int num_points, int num_seeds);
int gg_grasp_propose(int num_points, const float *points, const float *normals, const float *weights, int num_seeds,
                     const int32_t *seeds, double tube_radius, double max_width, double min_width, double clearance,
                     double depth, double height, double min_weight, double min_align, const double *up,
                     int num_approach, int32_t *pair_idx, int32_t *tube_count, float *span, uint8_t *valid,
                     float *rows, void *ws, size_t ws_bytes, gg_stream_t stream);

/* ---- gripper clearance: the whole gripper and its way in against the points (PARITY "Gripper
 * clearance") ----------------------------------------------------------------------------------------------------
 * Every grasp candidate against every point, exact in fp64, with a deterministic reduction.  Where
 * gg_grasp_contacts' collision_weight looks inside the two finger boxes at the final pose, this call looks at a model
 * of the whole gripper, at the final pose (body) and over the straight approach that leads to it (sweep).
 *   grasps: as for gg_grasp_contacts: num_grasps x 17 fp32 rows, gripper frame (a, b, c) = the columns of R.  A row is
 *           valid iff every entry is finite, width > 0 and height > 0 (depth may have either sign).
 *   points: num_points x 3 fp32; weights: num_points fp32.  A point takes part iff p is finite and
 *           (double)w > min_weight.  There are no normals.
 *   parts:  HOST array of num_parts x 6 x 4 doubles.  The gripper is num_parts boxes of the gripper frame; part p's
 *           bounds (x_lo, x_hi, y_lo, y_hi, z_lo, z_hi) = parts[p][0..5] are affine in the row's own sizes:
 *               bound = ((c0 + cw width) + cd depth) + ch height      with (c0, cw, cd, ch) = parts[p][k][0..3],
 *           in fp64 in that order, so one model serves candidates of every opening and finger length.  A part with
 *           lo > hi on some axis, or with a bound that is not finite, is empty for that row: it counts nothing, body or
 *           sweep (data, not an error).
 * Per valid grasp and point taking part, in fp64 from the fp32 inputs, no contraction:
 *   d_k = (double)p_k - (double)t_k;  u_j = (R[0][j] d_0 + R[1][j] d_1) + R[2][j] d_2     (as gg_grasp_contacts)
 *   body of part p:   x_lo <= u_0 <= x_hi,  y_lo <= u_1 <= y_hi,  z_lo <= u_2 <= z_hi     (every face closed)
 *   sweep of part p:  x_s <= u_0 < x_lo with x_s = x_lo - approach, u_1 and u_2 as for the body.  The gripper reaches t
 *                     from t - approach a, translating along +a, so in its own frame every part sweeps that extension
 *                     of itself; the interval is half-open, so body and sweep never share a point, and approach == 0
 *                     gives zero sweeps.
 * Parts are tested independently: a point inside two overlapping parts counts in both, so a model's parts should be
 * disjoint up to faces.  Outputs, every grasp written:
 *   body_count / sweep_count int32 [M][P]: the points in the body / sweep of each part;
 *   body_weight / sweep_weight fp32 [M][P]: the fp64 sum of their w, rounded to fp32;
 *   valid uint8 [M];  clear uint8 [M]: valid, sum_p body <= max_body and sum_p sweep <= max_sweep, the totals taken
 *   in fp64, in part order, from the fp64 part sums before they are rounded.
 * A row that is not valid gets zero counts, zero weights and valid = clear = 0 (data, not an error).
 * num_parts in 1..GG_CLEAR_MAX_PARTS and every coefficient finite; approach finite and >= 0; min_weight, max_body and
 * max_sweep not NaN (+inf: no limit).  num_grasps == 0 does nothing; num_points == 0 writes zeros and clear = valid.
 * No atomics: per-chunk partials combined in a fixed order, identical run to run.  No square root or division decides
 * anything: counts are exact.  `ws`: gg_grasp_clearance_workspace() bytes, 256-byte aligned (0 is returned for counts
 * out of range: the limits are GG_GRASP_MAX and GG_GRASP_MAX_POINTS). */
#define GG_CLEAR_MAX_PARTS 8
size_t gg_grasp_clearance_workspace(int num_points, int num_grasps, int num_parts);
int gg_grasp_clearance(int num_points, const float *points, const float *weights, int num_grasps, const float *grasps,
                       int num_parts, const double *parts, double approach, double min_weight, double max_body,
                       double max_sweep, int32_t *body_count, float *body_weight, int32_t *sweep_count,
                       float *sweep_weight, uint8_t *valid, uint8_t *clear, void *ws, size_t ws_bytes,
                       gg_stream_t stream);

/* ---- grasp NMS: distinct grasps from an ordered set (PARITY "Grasp NMS") ------------------------------
 * Greedy pose-distance non-maximum suppression over GraspGroup rows, in the caller's order; exact in fp64 and a pure
 * function of its inputs.
 *   grasps: as for gg_grasp_contacts: num_grasps x 17 fp32 rows, R row-major in columns 4..12, t in columns 13..15.
 *           Only R and t are read; a row takes part iff all 12 of those entries are finite.
 *   order:  num_order int32 row indices on the device, distinct, best first.  An entry outside [0, num_grasps) is
 *           skipped.  Repeated entries are the caller's error: they may give an unspecified `keep` for that row, never
 *           an access out of bounds.
 * Rows i and j that take part are NEAR iff both of the following hold, in fp64 from the fp32 inputs, no contraction:
 *   d_k = (double)t_ik - (double)t_jk;  dd = (d0 d0 + d1 d1) + d2 d2;  dd <= translation * translation;
 *   c_k = (Ri[0][k] Rj[0][k] + Ri[1][k] Rj[1][k]) + Ri[2][k] Rj[2][k] for the columns k = 0, 1, 2;
 *   tr = (c0 + c1) + c2;  tr_s = (c0 - c1) - c2 (the trace against Rj diag(1, -1, -1): the same parallel-jaw pose
 *   turned half a turn about its approach axis);  bound = 1 + 2 cos_rotation;
 *   tr >= bound, or symmetric != 0 and tr_s >= bound.
 * A rotation by the angle theta has tr = 1 + 2 cos theta, so cos_rotation = cos(largest angle that still counts as
 * near).  Both comparisons are inclusive.  No square root, acos or division decides anything.
 * The walk goes through `order` from the front: a row that takes part is KEPT iff no kept row earlier in `order` is
 * near it.  A suppressed row suppresses nothing.  Outputs, every element written:
 *   keep uint8 [num_grasps];
 *   suppressor int32 [num_grasps]: -1 for a kept row; for a suppressed row the row index of the first kept row in
 *           `order` that is near it; -2 for a row that is not in `order` or does not take part;
 *   kept int32 [num_order]: the kept row indices in `order`'s order, then -1 to the end;
 *   num_kept: device int32 [1].
 * translation finite and >= 0; cos_rotation in [-1, 1].  num_order == 0 writes keep = 0, suppressor = -2 and
 * num_kept = 0 (order, kept and ws may be null); with num_grasps == 0 as well the call does nothing and every pointer
 * may be null.  No atomics: identical output call to call.  `ws`: gg_grasp_nms_workspace() bytes, 256-byte aligned,
 * under num_order^2 / 8 + 64 num_order + 1024 bytes (0 is returned for num_order < 0 or > GG_NMS_MAX_ORDER). */
#define GG_NMS_MAX_ORDER 65536
size_t gg_grasp_nms_workspace(int num_order);
int gg_grasp_nms(int num_grasps, const float *grasps, int num_order, const int32_t *order, double translation,
                 double cos_rotation, int symmetric, uint8_t *keep, int32_t *suppressor, int32_t *kept,
                 int32_t *num_kept, void *ws, size_t ws_bytes, gg_stream_t stream);

/* ---- support plane: RANSAC consensus and the labels of one plane (PARITY "Support plane") -------------
 * gg_plane_consensus: every three-point plane hypothesis against every point, exact in fp64.
 *   points: num_points x 3 fp32; weights: num_points fp32, or NULL for "all take part".  A point takes part iff p is
 *           finite and (weights is NULL or (double)w > min_weight).
 *   hyp:    num_hypotheses x 3 int32 point indices (a, b, c) on the device.
 * Per hypothesis, in fp64 from the fp32 inputs, no contraction, in this order:
 *   e1_k = (double)p_bk - (double)p_ak;  e2_k = (double)p_ck - (double)p_ak;
 *   n = e1 x e2:  n0 = e1_1 e2_2 - e1_2 e2_1,  n1 = e1_2 e2_0 - e1_0 e2_2,  n2 = e1_0 e2_1 - e1_1 e2_0;
 *   nn = (n0 n0 + n1 n1) + n2 n2;  ee1 = (e1_0 e1_0 + e1_1 e1_1) + e1_2 e1_2,  ee2 likewise;
 *   VALID iff a, b, c are in [0, num_points) and distinct, all three points take part, nn is finite,
 *             nn > min_sin2 (ee1 ee2)  (nn / (ee1 ee2) is the squared sine of the angle at p_a: a triple that is
 *             collinear, or nearly so, defines no plane), and, with `up`,
 *             g g >= cos2_tilt (nn uu)  with g = (n0 u0 + n1 u1) + n2 u2, uu = (u0 u0 + u1 u1) + u2 u2
 *             (the plane's normal, either sign, is within the tilt limit of `up`).
 *   Point j is an INLIER of a valid hypothesis iff it takes part and  s s <= (dist dist) nn  with
 *             d_k = (double)p_jk - (double)p_ak,  s = (n0 d0 + n1 d1) + n2 d2.  The limit is inclusive.
 * No square root or division decides anything: count, valid and best are exact.  Outputs, every element written:
 *   count int32 [H]: the inliers (the hypothesis' own three points are among them); 0 when not valid;
 *   valid uint8 [H];
 *   best int32 [2]: the index of the valid hypothesis with the largest count, the smaller index on ties, and its
 *           count; (-1, 0) when no hypothesis is valid.
 * dist finite and >= 0; min_sin2 in [0, 1]; min_weight not NaN; up: HOST array of 3 doubles, finite and not zero, or
 * NULL for no tilt limit; cos2_tilt in [0, 1] (read only with up).  num_hypotheses == 0 does nothing (every pointer
 * may be null); num_points == 0 makes every hypothesis not valid.  Counts are integer sums: identical call to call.
 * `ws`: gg_plane_consensus_workspace() bytes, 256-byte aligned (0 is returned for counts out of range: the limits are
 * GG_GRASP_MAX_POINTS and GG_PLANE_MAX_HYPOTHESES).
 *
 * gg_plane_classify: one plane against every point.
 *   plane:  HOST array of 4 doubles (n0, n1, n2, d), n finite and not zero, d finite.  Distances are in units of |n|:
 *           the caller passes a unit normal.  origin: HOST array of 3 finite doubles, the point the moments are taken
 *           about (a point near the plane's inliers keeps them small).
 * Per point, in fp64, no contraction:  h = ((n0 x + n1 y) + n2 z) + d.
 *   height fp32 [N] = (float)h, NaN for a point that is not finite;
 *   side uint8 [N]: 3 = takes no part; 0 = h < -dist (below); 1 = -dist <= h <= dist (on); 2 = h > dist (above).
 *   sums: device double [16] over the points that take part, w = (double)weight (1 with weights NULL):
 *     [0] [1] [2]  the number of points on / above / below;
 *     [3]          sum of h h over "on";
 *     [4..6]       sum of q,  [7..12] sum of q q^T (xx, xy, xz, yy, yz, zz),  q_k = (double)p_k - origin_k, over "on";
 *     [13] [14] [15]  sum of w on / above / below.
 * The sums are formed in a fixed order that depends on num_points only, without floating-point atomics: the same
 * inputs give the same bits, call to call.  num_points == 0 writes 16 zeros.  dist finite and >= 0; min_weight not
 * NaN.  `ws`: gg_plane_classify_workspace() bytes, 256-byte aligned (0 is returned for num_points out of range). */
#define GG_PLANE_MAX_HYPOTHESES 65536
size_t gg_plane_consensus_workspace(int num_points, int num_hypotheses);
int gg_plane_consensus(int num_points, const float *points, const float *weights, double min_weight,
                       int num_hypotheses, const int32_t *hyp, double dist, double min_sin2, const double *up,
                       double cos2_tilt, int32_t *count, uint8_t *valid, int32_t *best, void *ws, size_t ws_bytes,
                       gg_stream_t stream);
size_t gg_plane_classify_workspace(int num_points);
int gg_plane_classify(int num_points, const float *points, const float *weights, double min_weight,
                      const double *plane, const double *origin, double dist, float *height, uint8_t *side,
                      double *sums, void *ws, size_t ws_bytes, gg_stream_t stream);

/* ---- scene preparation from RGB-D frames (PARITY "Scene preparation") --------------------------------
 * gg_backproject: depth frames to a base-frame point cloud (generate_data.py depth_image_to_point_cloud +
 * merge_point_clouds).  Frames are F x H x W, frame-major then row-major:
 *   depth fp64 [F][H][W] (metres), mask uint8 [F][H][W], rgb uint8 [F][H][W][3],
 *   intrinsics fp64 [F][4] (fx, fy, cx, cy), c2w fp64 [F][4][4] (row-major camera-to-base).
 * Pixel (f, v, u) is kept iff mask != 0 && d > d_lo && d < d_hi (NaN fails), then in fp64, no contraction:
 *   X = ((u - cx) * d) / fx,  Y = ((v - cy) * d) / fy,  Z = d,
 *   p_k = ((T[k][0] X + T[k][1] Y) + T[k][2] Z) + T[k][3],
 * and kept iff z_lo < p_2 < z_hi.  Kept points go to points fp64 [.][3] / colors uint8 [.][3] in pixel order (the
 * reference's boolean-index order); *count (device int64) = how many.  points / colors need room for F*H*W rows.
 * No atomics decide a position: identical output call to call, and the same rows whatever frames share a call.
 * `ws`: gg_backproject_workspace() bytes, 256-byte aligned (0 is returned for shapes out of range).  depth, intrinsics,
 * c2w, points and count 8-byte aligned; mask, rgb and colors any address.  Rows of points / colors past *count are not
 * written.  num_frames == 0 writes *count = 0 and nothing else. */
#define GG_PREP_MAX_ROWS (1 << 30)
size_t gg_backproject_workspace(int num_frames, int height, int width);
int gg_backproject(int num_frames, int height, int width, const double *depth, const uint8_t *mask, const uint8_t *rgb,
                   const double *intrinsics, const double *c2w, double d_lo, double d_hi, double z_lo, double z_hi,
                   double *points, uint8_t *colors, int64_t *count, void *ws, size_t ws_bytes, gg_stream_t stream);

/* gg_subsample: exactly m = num / keep distinct rows of num (save_points3D's `num // 8` of np.random.choice, same law:
 * a uniform subset), a pure function of (seed, num).  Row i has the key splitmix64(seed + (i + 1) * 0x9E3779B97F4A7C15)
 * (the SplitMix64 output function; all keys distinct); the m rows with the smallest keys are written in ascending
 * index order: out_index int64 [m], and, when given, out_points fp64 [m][3] / out_colors uint8 [m][3] gathered from
 * points fp64 [num][3] / colors uint8 [num][3].  m == 0 does nothing.  `ws`: gg_subsample_workspace(num) bytes,
 * 256-byte aligned.  points, out_points and out_index 8-byte aligned; colors and out_colors any address. */
size_t gg_subsample_workspace(int64_t num);
int gg_subsample(int64_t num, int64_t keep, uint64_t seed, const double *points, const uint8_t *colors,
                 double *out_points, uint8_t *out_colors, int64_t *out_index, void *ws, size_t ws_bytes,
                 gg_stream_t stream);

/* gg_depth_normals: world-frame normal maps of depth frames (generate_data.py cal_normal :204-229), fp64, no
 * contraction.  depth fp64 [F][H][W] (metres), H, W >= 2; intrinsics / c2w as gg_backproject (fx, fy used).
 *   d' = d < 0.01 ? 1e-5 : d;  du, dv = np.gradient(d') along columns / rows (interior (f[i+1] - f[i-1]) / 2, edges
 *   one-sided);  a = -(du * (fx / d')), b = -(dv * (fy / d')), c = 1;  n = (a, b, c) / sqrt((a a + b b) + c c);
 *   a row with a non-finite component becomes (0, 0, 1);  out_k = (R[k][0] n0 + R[k][1] n1) + R[k][2] n2, R = c2w[:3,:3].
 * normals fp64 [F][H][W][3].  Every array 8-byte aligned.  num_frames == 0 does nothing. */
int gg_depth_normals(int num_frames, int height, int width, const double *depth, const double *intrinsics,
                     const double *c2w, double *normals, gg_stream_t stream);

/* gg_knn: for every point, the k smallest sqrt(((dx dx + dy dy) + dz dz)) over all other points j != i (dx the fp64
 * difference of the fp32 coordinates), rounded to fp32 at the end: dist fp32 [N][k] ascending, idx int64 [N][k] a
 * neighbour set attaining them (ties by smallest index, except that among points at distance 0 any may be returned).
 * Exact for any input of finite points.  points fp32 [N][3]; 1 <= k <= GG_KNN_MAX_K < N.
 * grid (host, 4 doubles): lower corner x, y, z and cell edge (> 0); dims (host, 3 ints): cells per axis.  Points
 * outside the grid go to its border cells: any grid gives the same result, a grid fitted to the bulk of the points
 * gives it fast (gaussiangrasper_amd.prepare.knn_grid).  Cost: O(N x max points per cell) plus the cells walked;
 * worst case per point one walk of every cell and point, O(N^2) in all when the grid crowds the cloud into a few
 * cells.
 * `ws`: gg_knn_workspace(N, dims) bytes, 256-byte aligned (0 for sizes out of range).  points and dist 4-byte aligned,
 * idx 8-byte. */
#define GG_KNN_MAX_K 8
#define GG_KNN_MAX_POINTS (1 << 30)
#define GG_KNN_MAX_CELLS (1 << 26)
size_t gg_knn_workspace(int num_points, const int32_t *dims);
int gg_knn(int num_points, const float *points, int k, const double *grid, const int32_t *dims, float *dist,
           int64_t *idx, void *ws, size_t ws_bytes, gg_stream_t stream);

/* ---- object instances: DBSCAN of a point set and per-cluster statistics (PARITY "Object instances") ---
 * gg_cluster_dbscan.  points fp32 [N][3]; active uint8 [N] or NULL (all).  A point takes part (is active) iff its
 * byte is non-zero and its three coordinates are finite.  eps > 0 finite (fp64), min_points >= 1.
 *   neighbours:  active i and j are neighbours iff  (dx dx + dy dy) + dz dz <= eps eps,  all in fp64, dx the fp64
 *                difference of the fp32 coordinates (gg_knn's order).  No square root, no division: exact.
 *   core:        neighbour count, the point itself included, >= min_points (sklearn's min_samples convention).
 *   clusters:    the connected components of the core points under the neighbour relation, numbered 0, 1, ... in
 *                ascending order of the smallest point index among their core points.
 *   border:      a non-core active point with at least one core neighbour takes the smallest cluster number among
 *                its core neighbours.  Every other point, inactive ones included, gets label -1.
 * Outputs: labels int32 [N]; core uint8 [N]; neighbor_count int32 [N] (0 for inactive points); num_clusters, one
 * int32 on the device.  They are a pure function of the inputs: nothing depends on the schedule or on the grid, and
 * two calls give the same bits.  They equal the labels and core_sample_indices_ of sklearn.cluster.DBSCAN(eps,
 * min_samples) on the fp64 cast of the points wherever no pair sits within rounding of eps.
 * grid (host, 4 doubles) / dims (host, 3 ints): as for gg_knn.  The sort uses the cell edge max(cell, eps)
 * (1 + 2^-20), so that the 27 cells around a point hold all its neighbours; points outside the grid go to its border
 * cells.  Any grid gives the same result; one fitted to the cloud with cells of about eps gives it fast
 * (gaussiangrasper_amd.cluster.cluster_grid).
 * Cost: (active points) x (points within the 27 cells around each) x 3 passes (count, union, roots).  An eps so
 * large that the cloud falls into a few cells is quadratic: the caller must avoid it.  The union-find is lock-free
 * (32-bit device-scope atomicCAS / atomicMin, parents only decrease); no thread waits on another.
 * Everything runs on `stream`; nothing is read back.  num_points == 0 returns GG_OK and launches nothing.
 * `ws`: gg_cluster_workspace(N, dims) bytes, 256-byte aligned (0 for sizes out of range); a short or NULL workspace
 * is GG_ERR_INVALID_ARG.  points, labels, neighbor_count and num_clusters 4-byte aligned; active and core any address.
 *
 * gg_cluster_stats: per cluster c in [0, num_clusters), over the points with labels[i] == c (labels outside that
 * range are skipped):  count int64 [K] (exact);  weight fp64 [K] = sum of (double)weights[i];  centroid fp64 [K][3] =
 * (sum of (double)w_i (double)p_i) / weight (each product exact; NaN for weight 0);  bbox fp32 [K][6] = min x, y, z
 * then max x, y, z (exact; NaN for a cluster without members).  Integer atomics for count and, through an
 * order-preserving encoding, for bbox; fp64 atomic sums for weight and centroid, whose last bits may differ from
 * call to call.  points must be finite where a label is in range.  num_clusters == 0 does nothing.  points, weights,
 * labels and bbox 4-byte aligned; count, weight and centroid 8-byte. */
#define GG_CLUSTER_MAX_POINTS (1 << 30)
size_t gg_cluster_workspace(int num_points, const int32_t *dims);
int gg_cluster_dbscan(int num_points, const float *points, const uint8_t *active, double eps, int min_points,
                      const double *grid, const int32_t *dims, int32_t *labels, uint8_t *core, int32_t *neighbor_count,
                      int32_t *num_clusters, void *ws, size_t ws_bytes, gg_stream_t stream);
int gg_cluster_stats(int num_points, const float *points, const float *weights, const int32_t *labels,
                     int num_clusters, int64_t *count, double *weight, double *centroid, float *bbox,
                     gg_stream_t stream);

/* ---- registration: coloured ICP (PARITY "Registration") ------------------------------------------------
 * Park, Zhou, Koltun, "Colored Point Cloud Registration Revisited" (ICCV 2017); the reference's coloricp
 * (scripts/generate_data.py:47-83) runs Open3D's implementation of it.
 *
 * gg_cloud_frames: per-point surface frames of a cloud.  points fp32 [N][3]; intensity fp32 [N] (the mean of r, g, b
 * in [0, 1]); radius > 0 finite (fp64); grid / dims as for gg_knn (the sort's cell edge is max(cell, radius)
 * (1 + 2^-20): any grid gives the same result).  A point with a non-finite coordinate is invalid and nobody's
 * neighbour: count 0, valid 0, normal NaN, gradient 0.  For every other point i:
 *   neighbours:  j is a neighbour iff (dx dx + dy dy) + dz dz <= radius radius, in fp64 on the fp64 differences of
 *                the fp32 coordinates, i itself included.  count int32 [N] = how many.
 *   count < 3:   normal NaN, gradient 0, valid 0.  Otherwise valid 1 and:
 *   normal:      the covariance of the neighbours about their mean, fp64, two passes; the unit eigenvector of its
 *                smallest eigenvalue (cyclic Jacobi sweeps; the first axis among equal eigenvalues), signed so that
 *                its largest-magnitude component is positive (first index on ties).
 *   gradient d:  for each neighbour j != i with u = q_j - p_i the row A = u - (u.n) n, b = I_j - I_i, and one row
 *                A = (count - 1) n, b = 0;  d = (A^T A)^-1 A^T b in fp64 with the fp64 normal before it is rounded.
 *                d = 0 when count < 4 or the system is singular, which means here: det(A^T A) is not above
 *                2^-40 (count - 1)^2 (tr / 2)^2, tr the sum of the squared lengths of the neighbours' rows (det equals
 *                (count - 1)^2 times the determinant of the rows' 2 x 2 tangential moment, which (tr / 2)^2 bounds).
 * Outputs: normals fp32 [N][3], gradients fp32 [N][3], count int32 [N], valid uint8 [N].  count and valid are exact;
 * the fp64 sums run in the sort's slot order, which follows integer atomics, so normals and gradients may differ in
 * their last bits from call to call.  Every neighbour within the radius is used (Open3D's hybrid search stops at the
 * 30 nearest).  Cost: N x (points within the 27 cells around each) x 3 passes.
 * `ws`: gg_cloud_frames_workspace(N, dims) bytes, 256-byte aligned (0 for sizes out of range).  points, intensity,
 * normals, gradients and count 4-byte aligned; valid any address.  num_points >= 1.
 *
 * gg_icp_step: one Gauss-Newton linearisation of the coloured-ICP objective.  source fp32 [M][3], source_intensity
 * fp32 [M]; the target's points fp32 [N][3], intensity fp32 [N] and gg_cloud_frames' normals, gradients and valid;
 * grid / dims of the target as above (cell edge max(cell, max_dist) (1 + 2^-20)); transform (host, 12 finite
 * doubles): the row-major 3 x 4 source-to-target [R | t]; max_dist > 0 finite; 0 <= lambda_geometric <= 1.
 * Per source point p = (x, y, z), all fp64, nothing contracted to an FMA:
 *   s_r = ((R[r][0] x + R[r][1] y) + R[r][2] z) + t[r];
 *   correspondent: the target point q with valid != 0 and finite coordinates that has the smallest
 *   (dx dx + dy dy) + dz dz <= max_dist max_dist (d = q - s), the smaller index among equal distances; none (-1)
 *   when there is no such point or s is not finite.
 *   With n, d, I_q of the correspondent, I_s of the source point, a = sqrt(lambda), b = sqrt(1 - lambda),
 *   r_G = (s - q).n,  s' = s - r_G n,  I_proj = I_q + d.(s' - q),  g = -(d - (d.n) n):
 *     geometric row    a [s x n, n],  residual a r_G;      photometric row  b [s x g, g],  residual b (I_s - I_proj);
 *   the unknown is [omega (3), v (3)]: the update is [Rodrigues(omega) | v] applied on the left.
 * sums (device, fp64 [32]): the 21 upper-triangle entries of J^T J, row-major; the 6 entries of J^T r; the number of
 * source points with a correspondent; sum of squared distances; sum of r_G^2; sum of (I_s - I_proj)^2; one spare, 0.
 * abs_sums (device, fp64 [32], may be NULL): the same sums with every product replaced by its absolute value.
 * corr (device, int32 [M], may be NULL): each source point's correspondent or -1.
 * The sums are formed in a fixed order (lanes of a wave, waves of a block, blocks) without floating-point atomics,
 * and a correspondent never depends on the sort's slot order: the same inputs give the same bits.
 * reuse_sort != 0: `ws` still holds the sort a previous call made for the same points, valid, grid, dims and
 * max_dist, and it is not made again.
 * `ws`: gg_icp_step_workspace(M, N, dims) bytes, 256-byte aligned (0 for sizes out of range).  Every fp32 array and
 * corr 4-byte aligned, sums and abs_sums 8-byte, valid any address.  num_source, num_target >= 1. */
#define GG_REGISTER_MAX_POINTS (1 << 30)
size_t gg_cloud_frames_workspace(int num_points, const int32_t *dims);
int gg_cloud_frames(int num_points, const float *points, const float *intensity, double radius, const double *grid,
                    const int32_t *dims, float *normals, float *gradients, int32_t *count, uint8_t *valid, void *ws,
                    size_t ws_bytes, gg_stream_t stream);
size_t gg_icp_step_workspace(int num_source, int num_target, const int32_t *dims);
int gg_icp_step(int num_source, const float *source, const float *source_intensity, int num_target,
                const float *points, const float *intensity, const float *normals, const float *gradients,
                const uint8_t *valid, const double *grid, const int32_t *dims, const double *transform,
                double max_dist, double lambda_geometric, int reuse_sort, double *sums, double *abs_sums,
                int32_t *corr, void *ws, size_t ws_bytes, gg_stream_t stream);

/* ---- mesh export: TSDF fusion and marching tetrahedra (PARITY "Mesh export") ------------------------
 * The volume: dims (host, 3 ints) X, Y, Z lattice points, 1 <= each <= GG_TSDF_MAX_DIM, X Y Z <= GG_TSDF_MAX_POINTS;
 * grid (host, 6 floats) origin x, y, z and voxel size x, y, z (> 0, finite).  Point (i, j, k) has index
 * (i Y + j) Z + k (C order [X][Y][Z], z fastest) and sits at p_a = origin_a + (float)i_a * size_a (fp32, the
 * product rounded, then the sum).  Every array below is fp32; colour arrays are [..][3].
 *
 * gg_tsdf_integrate: fuses num_views depth frames into tsdf / weight [X][Y][Z] (in / out) and, when rgb is not NULL,
 * rgb [V][H][W][3] into color [X][Y][Z][3] / color_weight [X][Y][Z] (in / out; both NULL when rgb is NULL).
 * depth [V][H][W]; intrinsics [V][4] fx, fy, cx, cy; w2c [V][3][4] world-to-camera with OpenCV axes (x right,
 * y down, z forward).  trunc > 0 finite.  Per point, views in index order, fp32, no contraction:
 *   c_r = ((E[r][0] x + E[r][1] y) + E[r][2] z) + E[r][3];         skip the view unless c_2 > 0;
 *   u = (fx c_0) / c_2 + cx,  v = (fy c_1) / c_2 + cy;              skip unless 0 <= u < W and 0 <= v < H;
 *   d = depth[view][floor(v)][floor(u)];                             skip unless d > 0 (0, < 0, NaN: no observation;
 *                                                                    +inf: the ray saw nothing, free space);
 *   dist = d - c_2;                                                  skip unless dist >= -trunc;
 *   obs = min(1, dist / trunc);  W' = W + 1;  T' = (T W + obs) / W';
 *   with rgb, when |dist| < trunc:  K' = K + 1;  C'_c = (C_c K + rgb_c) / K'   (colour weight K, colour C).
 * One thread per point holds its state in registers across the views: no atomics, and V views in one call give the
 * same bits as V calls of one view each.  A workgroup owns a 4 x 8 x 8 brick and skips a view for the whole brick
 * only where a margin-padded test of the brick's corners (fp64) shows that no point of it can pass the tests above.
 *
 * gg_tsdf_mesh_count / gg_tsdf_mesh_emit: the zero level set by marching tetrahedra.  Cell (i, j, k) (each index <
 * dim - 1) is cut into the 6 Kuhn tetrahedra around its main diagonal: tetrahedron t = permutation (a, b, c) of the
 * axes in lexicographic order ((x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y), (z,y,x)) has the corners o, o + e_a,
 * o + e_a + e_b, o + (1,1,1).  Every edge then joins a lattice point to a neighbour in one of 7 positive directions
 * d = 0..6: +x, +y, +z, +xy, +xz, +yz, +xyz.
 *   - A cell emits only if all 8 of its corners have weight > 0 (unobserved space is never meshed); tsdf must be
 *     finite there.  A corner is inside when T < 0.
 *   - Every sign-changing edge (a, b = a + delta_d) used by an emitting cell is one shared vertex:
 *     t = T_a / (T_a - T_b);  g = (float)i_a + t * delta (per axis; delta 0 gives (float)i_a);
 *     position = origin + g * size;  normal: the TSDF gradient at a and at b, per axis
 *     (T[i+1] - T[i-1]) / (2 size) inside the volume, (T[1] - T[0]) / size and (T[n-1] - T[n-2]) / size at its
 *     borders, 0 along an axis of one point; n = g_a + t (g_b - g_a); n / sqrt((n0 n0 + n1 n1) + n2 n2), or
 *     (0, 0, 0) when that length is 0; colour: C_a + t (C_b - C_a).
 *   - Triangles of one tetrahedron (corners 0..3 in the order above, case = sum of inside(corner k) << k):
 *     one corner apart from the other three (one inside or one outside): the triangle on its three edges;
 *     two inside (p < q), two outside (r < s): the quad pq-cut split as (pr, ps, qs), (pr, qs, qr).
 *     The winding makes (v1 - v0) x (v2 - v0) point towards increasing TSDF (free space); it is fixed per
 *     tetrahedron and case from the corners' lattice positions.  A zero at a corner gives degenerate triangles: they
 *     are kept (no NaN, every index valid).
 *   - Order: vertices ascending (point index, direction); faces ascending (cell, tetrahedron, triangle); the output
 *     is a pure function of the input.  Faces are int32 vertex triples.
 * gg_tsdf_mesh_count writes counts int64 [2] (device) = (num_vertices, num_faces) and keeps the edge masks and
 * offsets in ws; gg_tsdf_mesh_emit then reads them from the same ws (the same dims and tsdf, unchanged in between)
 * and writes vertices / normals [num_vertices][3], colors [num_vertices][3] (only when both color and colors are
 * not NULL) and faces [num_faces][3]; num_vertices / num_faces are the capacities of those arrays (the counts read
 * back): nothing is written past them.  A count of -1 means the prefix scan gave up (never expected).
 * `ws`: gg_tsdf_mesh_workspace(dims) bytes (about 10 per point), 256-byte aligned, of any content on entry of
 * gg_tsdf_mesh_count, read only by gg_tsdf_mesh_emit; 0 for dims out of range.  Every fp32 array of the three calls and
 * faces 4-byte aligned, counts 8-byte.  gg_tsdf_integrate with num_views == 0 writes nothing. */
#define GG_TSDF_MAX_POINTS (1 << 27)
#define GG_TSDF_MAX_DIM 4096
#define GG_TSDF_MAX_VIEWS (1 << 20)
#define GG_TSDF_MAX_SIDE 32768
int gg_tsdf_integrate(const int32_t *dims, const float *grid, float trunc, int num_views, int height, int width,
                      const float *depth, const float *rgb, const float *intrinsics, const float *w2c, float *tsdf,
                      float *weight, float *color, float *color_weight, gg_stream_t stream);
size_t gg_tsdf_mesh_workspace(const int32_t *dims);
int gg_tsdf_mesh_count(const int32_t *dims, const float *tsdf, const float *weight, int64_t *counts, void *ws,
                       size_t ws_bytes, gg_stream_t stream);
int gg_tsdf_mesh_emit(const int32_t *dims, const float *grid, const float *tsdf, const float *color, int64_t num_vertices,
                      int64_t num_faces, float *vertices, float *normals, float *colors, int32_t *faces,
                      const void *ws, size_t ws_bytes, gg_stream_t stream);

/* ---- distance field of the scene (PARITY "Distance field") -----------------------------------------
 * The volume: dims (host, 3 ints) X, Y, Z cells, 1 <= each <= GG_FIELD_MAX_DIM, X Y Z <= GG_FIELD_MAX_CELLS; grid
 * (host, 4 doubles) the lower corner lo and ONE cubic cell edge h > 0, all finite.  Cell (i, j, k) has index
 * (i Y + j) Z + k (C order [X][Y][Z], z fastest, the TSDF volume's layout).  Along axis a, cell c contains the
 * coordinate p iff (double)c h <= d < (double)(c + 1) h with d = (double)p - lo_a: fp64 products and comparisons (a
 * division may propose c, the comparisons decide).  A cell's centre is x_a = lo_a + ((double)c + 0.5) h.
 *
 * gg_field_splat: Gaussians to integer occupancy mass.  means [N][3], rot [N][9] (row-major, the columns are the
 * axes: ops.quat_to_rotmat), scales [N][3] (activated), weights [N]: fp32.  extent k: finite, >= 0; max_reach in
 * 0..GG_FIELD_MAX_REACH; min_weight not NaN; sign +1 or -1.  A row takes part iff all 16 of its inputs are finite,
 * every scale is > 0 and min_weight < (double)w < 2^15; its vote is q = trunc((double)w 2^16) (an exact product) as
 * int64.  mass int64 [X][Y][Z], in / out: the row adds sign q to
 *   (a) the cell that contains its mean, if there is one;
 *   (b) every other cell within Chebyshev distance `reach` of that cell (found per axis by the rule above even when
 *       it lies outside the volume; cells outside the volume are dropped) whose centre x is in the closed k-sigma
 *       ellipsoid: with d = x - (double)m, u_j = (R[0][j] d_0 + R[1][j] d_1) + R[2][j] d_2, A_j = (double)s_j (double)s_j:
 *       ((u_0 u_0)(A_1 A_2) + (u_1 u_1)(A_0 A_2)) + (u_2 u_2)(A_0 A_1) <= (k k)((A_0 A_1) A_2)
 *       in fp64 with exactly this parenthesisation and no contraction.
 * reach = min(max_reach, n + 1), n the smallest integer >= 0 with (double)n h >= k (double)max_j s_j.  The box is a
 * cull; a row it cuts (n + 1 > max_reach) is data, not an error.  skipped / truncated (device, one int64 each) are
 * WRITTEN: the rows of this call that took no part / that max_reach cut.  Integer sums commute: mass is the same from
 * run to run, and a +1 call followed by a -1 call on the same rows restores it bit for bit (-1 adds the two's
 * complement).  num_rows == 0 writes nothing.  fp32 arrays 4-byte aligned, int64 arrays 8-byte.
 *
 * gg_field_distance: the exact squared Euclidean distance transform.  A cell is occupied iff mass >= threshold
 * (>= 1).  dist2 int32 [X][Y][Z] (written whole) = min over occupied cells of di^2 + dj^2 + dk^2 in cell units: 0 on
 * occupied cells, exactly GG_FIELD_FAR everywhere when no cell is occupied.  Three separable integer min-plus passes,
 * z then y then x, from f = occupied ? 0 : FAR, f'[c] = min_c' f[c'] + (c - c')^2 (values stay below 2^31: FAR +
 * 2 1023^2 < 2^31), and a final clamp to FAR.  ws: gg_field_distance_workspace(dims) bytes (0 for dims out of
 * range), 256-byte aligned, of any content.
 *
 * gg_field_paths: gripper paths against the field.  poses fp32 [P][W][12]: R row-major (9), then t (3); spheres fp32
 * [S][3]: centres in the gripper frame; need2 int32 [S], each in 0..GG_FIELD_FAR; outside in 0..GG_FIELD_FAR: the
 * dist2 taken for a centre outside the volume (FAR: free, 0: blocked).  Per pose with 12 finite entries and per
 * sphere: c_k = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t_k in fp64, its cell by the rule above (a centre that is
 * not finite is outside), d = dist2[cell].  slack int32 [P][W] = min_s (d - need2[s]); GG_FIELD_FAR when S == 0;
 * INT32_MIN for a pose that is not finite.  first_hit int32 [P] = the smallest w with slack < 0, or W.  No atomics
 * and no floating-point decision beyond the cell rule.  P W <= GG_FIELD_MAX_POSES, S <= GG_FIELD_MAX_SPHERES; with
 * P == 0 or W == 0 nothing is written.  Every array 4-byte aligned.
 *
 * Transit planning (PARITY "Transit planning"): shortest paths through the free cells, integers only.
 * A cell is FREE iff it is inside the volume and dist2[cell] >= need, need in 0..GG_FIELD_FAR.  A MOVE is a
 * d in {-1, 0, 1}^3 other than 0, numbered m = (dx + 1) 9 + (dy + 1) 3 + (dz + 1); its weight is 3, 4 or 5 for one,
 * two or three components that are not 0 (the 3-4-5 chamfer).  The move d from cell c is ALLOWED iff every cell c + e
 * with e_a in {0, d_a} is free (2, 4 or 8 cells): every point of the segment between the two centres then lies in a
 * free cell under the half-open cell rule, and no path squeezes between two blocked cells that touch by an edge or a
 * corner.
 *
 * gg_field_route: the cost-to-go.  goals int32 [G][3] cells, G in 0..GG_FIELD_MAX_GOALS; a goal outside the volume or
 * not free takes no part and is counted in ignored (device, one int64, WRITTEN); duplicates take part.  cost int32
 * [X][Y][Z] (written whole) = the smallest sum of weights over sequences of allowed moves from the cell to a goal
 * that takes part: 0 on such a goal, exactly GG_FIELD_FAR on cells that are not free, on cells no sequence leads
 * from, and everywhere when no goal takes part.  The largest finite cost is below 5 2^27 < 2^30: nothing saturates.
 * The result does not depend on the schedule.  The call runs rounds of relaxation (one launch each, no kernel waits
 * for another workgroup) until a round changes nothing that another brick reads; UNLIKE THE OTHER ENTRIES IT
 * SYNCHRONISES `stream` once per batch of rounds to read that back, so it cannot be captured into a graph.
 * max_rounds >= 1 bounds the loop; rounds_out (a HOST int, written) receives the rounds it took, the last of which
 * changed nothing (0 when G == 0), a number that may differ by a few from run to run.  When max_rounds run out the
 * call returns GG_ERR_NOT_CONVERGED and says so in gg_last_error(); cost then holds VALID UPPER BOUNDS: every value
 * below FAR is the weight of a real sequence of allowed moves to a goal, but not yet the smallest.  ws:
 * gg_field_route_workspace(dims) bytes (0 for dims out of range), 256-byte aligned, of any content.  dist2, goals
 * and cost 4-byte aligned, ignored 8-byte.
 *
 * gg_field_descend: paths down a cost-to-go.  dist2, need: as given to gg_field_route; cost: its converged result.
 * starts int32 [P][3]; max_cells >= 1, P max_cells <= GG_FIELD_MAX_POSES; cells int32 [P][max_cells][3]; length
 * int32 [P].  From a start that is free and costs less than FAR: while the cost here is not 0, take the allowed move
 * with cost[next] + weight == cost[here] that has the lowest number m.  length[p] = the cells of the whole path,
 * start and goal included (1: the start is a goal); 0 when the start is outside, not free or costs FAR (and when
 * `cost` is not route's fixed point for this dist2 and need, so that no move fits somewhere on the way).  The first
 * min(length, max_cells) rows of cells[p] are the path's cells in order: with length > max_cells the path is cut
 * and length still counts all of it (call again with more room); with 0 < length <= max_cells the rows from length
 * on repeat the last cell, so that a consumer of a fixed number of waypoints can take the array as it is; with
 * length 0 every row is -1, -1, -1.  A walk takes at most cost[start] / 3 + 1 steps.  P == 0 writes nothing.  Every
 * array 4-byte aligned.
 *
 * Line of sight: the block rule at any length.  For cells a and b inside the volume, COVER(a, b) is the
 * set of cells c whose CLOSED cube [c, c + 1]^3 (cell units) meets the closed segment between the centres a + 1/2 and
 * b + 1/2.  The segment is CLEAR iff every cell of its cover is inside the volume and free.  Where the segment goes
 * exactly through a face edge or a corner, all 4 or 8 cells that touch there belong to the cover; for b - a a move
 * the cover is exactly the 2, 4 or 8 cells of the block rule, so every move a descent made is clear.  Every decision
 * is an integer comparison: with n_a = |b_a - a_a| the segment crosses the k-th boundary of axis a at
 * t = (2 k + 1) / (2 n_a), and two crossings are ordered by (2 k + 1) n_b against (2 k' + 1) n_a, products below 2^22
 * with GG_FIELD_MAX_DIM 1024; equality is a tie, and a tie opens every cell it touches.  Every point of a clear
 * segment then lies in a free cell under the half-open cell rule, and no segment squeezes between two blocked cells
 * that touch by an edge or a corner.
 *
 * gg_field_sight: a, b int32 [S][3] cells, S in 0..GG_FIELD_MAX_POSES; cover int32 [S] = the number of cells of the
 * cover, blocked int32 [S] = how many of them are not free (0: clear).  An endpoint outside the volume gives cover 0
 * and blocked -1, with no walk; a == b gives cover 1.  The whole cover is walked, at most n_x + n_y + n_z steps.  No
 * atomics, a pure function of the inputs, symmetric in a and b.  S == 0 writes nothing.
 *
 * gg_field_shortcut: greedy string pulling of cell paths.  cells int32 [P][max_cells][3] and length int32 [P] as
 * gg_field_descend writes them (any cell sequence is accepted); n = min(length, max_cells), so a cut path is
 * shortened as far as it goes.  window >= 1; max_cells >= 1, P max_cells <= GG_FIELD_MAX_POSES.  From the anchor
 * i = 0 the next anchor is the LARGEST j in (i, min(i + window, n - 1)] whose segment cells[i] -> cells[j] is clear
 * (sight is not monotone in j); when there is none it is j = i + 1, clear or not; repeated until i = n - 1.  A cell
 * outside the volume ends no segment that is clear.  keep int32 [P][max_cells]: the anchors, ascending, the first 0,
 * the last n - 1; the rows from count on repeat n - 1.  count int32 [P]: the number of anchors (1 for n == 1, at most
 * n).  blocked int32 [P]: the kept segments that are not clear: 0 for every path a descent produced with this dist2
 * and need, the caller's to look at for any other.  length <= 0: count 0, blocked 0 and every keep row -1.
 * window == 1 returns the path itself.  No atomics, a pure function of the inputs.  P == 0 writes nothing.  Every
 * array 4-byte aligned.
 * Null, misaligned or out-of-range arguments: GG_ERR_INVALID_ARG naming the argument, before any launch. */
#define GG_FIELD_MAX_DIM 1024
#define GG_FIELD_MAX_CELLS (1 << 27)
#define GG_FIELD_FAR (1 << 30)
#define GG_FIELD_MAX_REACH 64
#define GG_FIELD_MAX_ROWS (1 << 30)
#define GG_FIELD_MAX_POSES (1 << 26)
#define GG_FIELD_MAX_SPHERES 1024
int gg_field_splat(const int32_t *dims, const double *grid, int num_rows, const float *means, const float *rot,
                   const float *scales, const float *weights, double extent, int max_reach, double min_weight,
                   int sign, int64_t *mass, int64_t *skipped, int64_t *truncated, gg_stream_t stream);
size_t gg_field_distance_workspace(const int32_t *dims);
int gg_field_distance(const int32_t *dims, const int64_t *mass, int64_t threshold, int32_t *dist2, void *ws,
                      size_t ws_bytes, gg_stream_t stream);
int gg_field_paths(const int32_t *dims, const double *grid, const int32_t *dist2, int num_paths, int num_waypoints,
                   const float *poses, int num_spheres, const float *spheres, const int32_t *need2, int32_t outside,
                   int32_t *slack, int32_t *first_hit, gg_stream_t stream);
#define GG_FIELD_MAX_GOALS (1 << 24)
size_t gg_field_route_workspace(const int32_t *dims);
int gg_field_route(const int32_t *dims, const int32_t *dist2, int32_t need, int num_goals, const int32_t *goals,
                   int32_t *cost, int64_t *ignored, int max_rounds, int *rounds_out, void *ws, size_t ws_bytes,
                   gg_stream_t stream);
int gg_field_descend(const int32_t *dims, const int32_t *dist2, int32_t need, const int32_t *cost, int num_paths,
                     const int32_t *starts, int max_cells, int32_t *cells, int32_t *length, gg_stream_t stream);
int gg_field_sight(const int32_t *dims, const int32_t *dist2, int32_t need, int num_segments, const int32_t *a,
                   const int32_t *b, int32_t *cover, int32_t *blocked, gg_stream_t stream);
int gg_field_shortcut(const int32_t *dims, const int32_t *dist2, int32_t need, int num_paths, int max_cells,
                      const int32_t *cells, const int32_t *length, int window, int32_t *keep, int32_t *count,
                      int32_t *blocked, gg_stream_t stream);

/* ---- known free space of the distance field (PARITY "Known free space") ---------------------------
 * gg_field_distance calls every cell without Gaussian mass free, whether a camera ever looked into it or not.  These
 * entries give the volume a third state: a cell is KNOWN FREE once enough depth frames have seen through all of it.
 *
 * gg_depth_min_pyramid: depth fp32 [V][H][W], along the camera's z axis in scene units, as gg_tsdf_integrate reads it.
 * pyr fp32 [V][S] (written whole): level l has H_l = ceil(H / 2^l) rows and W_l = ceil(W / 2^l) columns, row-major;
 * the levels run from l = 0 to the first with H_l = W_l = 1; level l starts at offset sum_{m<l} H_m W_m and S is the
 * sum over all levels, which gg_depth_min_pyramid_size(H, W) returns (0 for a size out of range).  Level 0 is the
 * sanitised frame d > 0 ? d : 0: +inf stays (free space seen to infinity); 0, negative and NaN become 0 ("no
 * observation: nothing is known to be in front of it").  A texel of level l + 1 is the minimum of its up-to-four
 * children (2y, 2x), (2y, 2x + 1), (2y + 1, 2x), (2y + 1, 2x + 1) of level l; children beyond the level's edge are
 * absent.  A minimum is exact: the bytes are a pure function of the input.  V <= GG_TSDF_MAX_VIEWS, H, W <=
 * GG_TSDF_MAX_SIDE; V == 0 writes nothing.  Both arrays 4-byte aligned.
 *
 * gg_field_observe: dims, grid: the field's volume (above).  pyr: gg_depth_min_pyramid's of V frames of H x W.
 * intrinsics fp64 [V][4] fx, fy, cx, cy with fx, fy > 0 (the caller's to ensure: the arrays are on the device; with
 * anything else every access stays in bounds and the counts mean nothing); w2c fp64 [V][3][4] = E, world to camera,
 * OpenCV axes.  Host doubles radius > 0, margin >= 0, near > 0, all finite.  seen uint16 [X][Y][Z], in / out; looked
 * uint16 [X][Y][Z], in / out, may be NULL.  Every cell is owned by exactly one thread; there are no atomics; the
 * output is a pure function of the inputs.  Per cell (i, j, k), all in fp64 without contraction, in this order:
 *   centre c_a = lo_a + ((double)i_a + 0.5) h;
 *   per view, in index order:
 *     p_r = ((E[r][0] c_0 + E[r][1] c_1) + E[r][2] c_2) + E[r][3];   zn = p_2 - radius,  zf = p_2 + radius;
 *     the view takes no part unless zn >= near;
 *     pixel bounds of the ball's bounding box, for x (a = p_0, f = fx, cc = cx, n = W) and for y (p_1, fy, cy, H):
 *       xl = a - radius,  xh = a + radius;
 *       ul = f (xl / (xl < 0 ? zn : zf)) + cc,   uh = f (xh / (xh > 0 ? zn : zf)) + cc;
 *       A = floor(ul - 2^-20),  B = floor(uh + 2^-20)    (the pad is many orders above the fp64 rounding of these);
 *     the view takes no part unless A >= 0 and B <= n - 1 on both axes (compared as doubles; a NaN bound fails);
 *     otherwise the cell was LOOKED AT: looked += 1;
 *     level l = the smallest with (B >> l) - (A >> l) <= 1 on both axes (the 1 x 1 top level always qualifies);
 *     m = the minimum of the up-to-four texels {A_v >> l, B_v >> l} x {A_u >> l, B_u >> l} of level l;
 *     the cell is SEEN FREE in this view iff (double)m > zf + margin: seen += 1.
 * Both counters saturate: min(65535, old + count).  V views in one call give the same counts as V calls of one view.
 * WHAT THIS GUARANTEES.  Every point q of the closed ball of `radius` around the centre has camera depth q_2 in
 * [zn, zf], zn >= near > 0, and projects, with the floor(u), floor(v) pixel rule of gg_tsdf_integrate, to a pixel
 * inside [A, B] on both axes (q_0 / q_2 is bounded by the box's extreme ratios).  Every such pixel lies in one of the
 * texels read ((B >> l) - (A >> l) <= 1), and every texel is the minimum over its pixels.  So with "seen free", along
 * every ray through the ball the measured surface lies more than `margin` beyond q: depth[pixel(q)] >= m > zf +
 * margin >= q_2 + margin.  With radius >= (sqrt(3) / 2) h the ball contains the cell's cube.  A missing reading
 * anywhere in the footprint (a texel of 0) or a footprint that leaves the image makes the view ABSTAIN: it is never
 * counted as free.  A workgroup owns a 4 x 8 x 8 brick and skips a view for the whole brick only where a
 * margin-padded test of the box of its cells' centres shows that none of them can be looked at.
 * V == 0 leaves both arrays untouched.  pyr 4-byte aligned, intrinsics and w2c 8-byte, seen and looked 2-byte.
 *
 * gg_field_distance_known: gg_field_distance with one more seed rule.  seen uint16 [X][Y][Z]; min_views in 1..65535.
 * A cell seeds the transform iff mass >= threshold OR seen < min_views: unknown space is blocked.  The same passes,
 * workspace (gg_field_distance_workspace) and output; with seen >= min_views everywhere, gg_field_distance's bits.
 * Null, misaligned or out-of-range arguments: GG_ERR_INVALID_ARG naming the argument, before any launch. */
int64_t gg_depth_min_pyramid_size(int height, int width);
int gg_depth_min_pyramid(int num_views, int height, int width, const float *depth, float *pyr, gg_stream_t stream);
int gg_field_observe(const int32_t *dims, const double *grid, int num_views, int height, int width, const float *pyr,
                     const double *intrinsics, const double *w2c, double radius, double margin, double near,
                     uint16_t *seen, uint16_t *looked, gg_stream_t stream);
int gg_field_distance_known(const int32_t *dims, const int64_t *mass, int64_t threshold, const uint16_t *seen,
                            int min_views, int32_t *dist2, void *ws, size_t ws_bytes, gg_stream_t stream);

/* ---- placement: height maps and the resting search (PARITY "Placement") ----------------------------
 * A plane grid: dims (host, 2 ints) U, V cells, 1 <= each <= GG_PLACE_MAX_DIM; grid (host, 4 doubles) lo_u, lo_v, ONE
 * square cell edge h > 0 and the level height hz > 0, all finite.  A map is int32 [U][V] (C order, v fastest) of
 * integer height levels; a cell that holds nothing is GG_PLACE_EMPTY.
 *
 * gg_height_map: points to height levels, for F frames in one call.  points fp32 [N][3]; weights fp32 [N] or null;
 * min_weight not NaN; frames fp64 [F][12] on the DEVICE, 8-byte aligned: the origin o, then the axes e0, e1, e2,
 * taken as given (the host makes them orthonormal), 1 <= F <= GG_PLACE_MAX_YAWS; N <= GG_PLACE_MAX_POINTS.  A point
 * takes part iff its three coordinates are finite and weights is null or min_weight < (double)w.  Per frame:
 * d = (double)p - o, c_a = (d_0 e_a0 + d_1 e_a1) + d_2 e_a2 in fp64 with exactly this parenthesisation and no
 * contraction.  When c_0 - lo_u, c_1 - lo_v and c_2 are all finite, the cell along u is the integer a with
 * (double)a h <= c_0 - lo_u < (double)(a + 1) h (the distance field's rule: a division may propose, the comparisons
 * decide), along v the same with c_1 - lo_v, and the level the integer z with (double)z hz <= c_2 < (double)(z + 1) hz,
 * clamped to +-GG_PLACE_MAX_LEVEL.  A point whose cell is outside the grid, or for which one of the three is not
 * finite, is dropped for that frame.  map int32 [F][U][V], in / out: map[f][a][b] = max(map[f][a][b], z) by integer
 * atomic max; the caller fills it with GG_PLACE_EMPTY first, several calls accumulate, and the result is the same from
 * run to run.  dropped int64 [F] (8-byte aligned) is WRITTEN: the points of this call that took no part or were
 * dropped for that frame.  N == 0 writes only dropped.  One mode only: the UNDERSIDE of an object is its map in a
 * frame with e2 = -n, under = max level(-c_2).  fp32 and int32 arrays 4-byte aligned.
 *
 * gg_place_search: the resting height of an object over every yaw and anchor.  top int32 [U][V]; foot (host, 2 ints)
 * A, B in 1..GG_PLACE_MAX_FOOT with A <= U, B <= V; under int32 [K][A][B], K in 0..GG_PLACE_MAX_YAWS; tol in
 * 0..GG_PLACE_MAX_LEVEL.  THE CALLER'S DUTY: every level that is not GG_PLACE_EMPTY lies within +-GG_PLACE_MAX_LEVEL,
 * so that every sum below stays under 2^30.  With I = U - A + 1, J = V - B + 1, for yaw k and anchor (i, j) in
 * [0, I) x [0, J), over the object cells (a, b) with under[k][a][b] != GG_PLACE_EMPTY:
 *   s(a, b) = top[i + a][j + b] + under[k][a][b]
 *   rest    int32 [K][I][J]    = max s
 *   contact int32 [K][I][J]    = the number of object cells with s >= rest - tol
 *   support int32 [K][I][J][6] = over those contact cells: sum a, sum b, min a, max a, min b, max b.
 * The anchor is INVALID when map k has no object cell, or when top[i + a][j + b] is GG_PLACE_EMPTY for an object cell
 * (a, b); it gets rest = GG_PLACE_EMPTY, contact = 0, support = {0, 0, -1, -1, -1, -1}.  Every output element is
 * written; no atomics and no floating point.  K == 0 writes nothing.  Every array 4-byte aligned.
 * Null, misaligned or out-of-range arguments: GG_ERR_INVALID_ARG naming the argument, before any launch. */
#define GG_PLACE_EMPTY (-2147483647 - 1) /* INT32_MIN */
#define GG_PLACE_MAX_LEVEL (1 << 28)
#define GG_PLACE_MAX_DIM 4096
#define GG_PLACE_MAX_FOOT 128
#define GG_PLACE_MAX_YAWS 256
#define GG_PLACE_MAX_POINTS (1 << 30)
int gg_height_map(int num_points, const float *points, const float *weights, double min_weight, int num_frames,
                  const double *frames, const double *grid, const int32_t *dims, int32_t *map, int64_t *dropped,
                  gg_stream_t stream);
int gg_place_search(const int32_t *dims, const int32_t *top, int num_yaws, const int32_t *foot, const int32_t *under,
                    int32_t tol, int32_t *rest, int32_t *contact, int32_t *support, gg_stream_t stream);

/* ---- arm reachability: kinematics of a serial chain against the distance field (PARITY "Arm
 * reachability") -------------------------------------------------------------------------------------------------
 * The arm: J = num_joints in 1..GG_ARM_MAX_JOINTS and `arm`, a HOST array of GG_ARM_DOUBLES(J) doubles:
 *   base[12]          world from arm base: R row-major (9), then t (3), the pose layout of gg_field_paths
 *   fixed[J + 1][12]  A_j, j < J: link j to joint j at q_j = 0; A_J: the last link to the GRIPPER frame, the frame of
 *                     the grasp rows (the columns of R are approach, closing and height)
 *   joint[J][6]       axis[3] (a unit vector in the joint frame), lo, hi, kind (0.0 revolute, 1.0 prismatic)
 * Frames: F_0 = base, F_{j+1} = (F_j A_j) M_j(q_j), F_{J+1} = F_J A_J the gripper pose.  M_j is Rodrigues' rotation
 * (I c + (1 - c) a a^T) + s [a]x with c = cos q, s = sin q, or the translation by q a for a prismatic joint.  All
 * fp64; a product X Y has R[r][c] = (X[r][0] Y[0][c] + X[r][1] Y[1][c]) + X[r][2] Y[2][c] and t[r] = ((X[r][0] t_0 +
 * X[r][1] t_1) + X[r][2] t_2) + tX[r], no contraction.  An arm is refused (GG_ERR_INVALID_ARG naming what is wrong,
 * before any launch) for an entry that is not finite, a rotation block of base or fixed with |R^T R - I|max > 1e-9,
 * an axis whose squared length is off 1 by more than 1e-9, lo > hi, or a kind that is neither 0 nor 1.
 *
 * gg_arm_fk: q fp64 [M][J] -> frames fp64 [M][J + 2][12], F_0 .. F_{J+1}.  A row with a q that is not finite gives
 * NaN in all of its frames.  Limits are not applied.  M <= GG_FIELD_MAX_POSES; M == 0 writes nothing.  Arrays 8-byte
 * aligned.
 *
 * gg_arm_follow: inverse kinematics along pose paths.  poses fp32 [P][W][12] gripper poses (what gg_field_paths
 * takes), seeds fp64 [P][S][J]; q_out fp64 [P][S][W][J], iters int32 [P][S][W], resid fp64 [P][S][W][2], first_fail
 * int32 [P][S].  Every (path, seed) is independent: waypoint 0 starts from the seed clamped into the limits, waypoint
 * w > 0 from the solution of w - 1.  Per waypoint, for it = 0, 1, ..., all in fp64:
 *   1. FK.  e_p = p* - p; R_e = R* R^T; e_r = the rotation vector of R_e through its quaternion (Shepperd's branches:
 *      the largest of trace, R00, R11, R22 is the pivot; normalised; w >= 0): 2 atan2(|v|, w) v / |v|, and 2 v when
 *      |v| < 1e-12.
 *   2. CONVERGED iff |e_p| <= tol_p and |e_r| <= tol_r: q_out = q, iters = it, resid = (|e_p|, |e_r|).
 *   3. Otherwise, it == max_iter FAILS the waypoint.
 *   4. Otherwise the geometric Jacobian: column j is [z_j x (p - o_j); L z_j] for a revolute and [z_j; 0] for a
 *      prismatic joint, z_j and o_j the joint's axis and origin in the world (of F_j A_j); e = [e_p; L e_r];
 *      lambda2 = gain (e . e) + lambda_min^2; dq = J^T (J J^T + lambda2 I)^-1 e by a 6 x 6 Cholesky solve; when
 *      max|dq| > max_step, dq is scaled by max_step / max|dq|; q <- min(max(q + dq, lo), hi).  A pivot that is not
 *      positive, or an error norm or a dq that is not finite, FAILS the waypoint.
 * A pose or a seed with an entry that is not finite fails its waypoint (the seed: waypoint 0) at once.  first_fail =
 * the failed waypoint, or W.  From the failed waypoint on: q_out NaN, iters -1, resid NaN.  No thread waits for
 * another, no atomics, max_iter in 0..GG_ARM_MAX_ITER bounds every loop, and the same inputs give the same bytes.
 * tol_p, tol_r, gain finite and >= 0; L (rot_length), lambda_min, max_step finite and > 0.  P S max(W, 1) <=
 * GG_FIELD_MAX_POSES; P == 0 or S == 0 writes nothing.  fp64 arrays 8-byte aligned, the others 4-byte.
 *
 * gg_arm_clear: the whole arm against the distance field.  dims, grid, dist2, need2, outside: as gg_field_paths takes
 * them.  q fp64 [M][J]; spheres fp32 [S][3] centres, each in the frame F_f with f = frame[s] (int32 [S], THE CALLER'S
 * DUTY: in 0..J + 1; the kernel clamps it into that range, so no read goes astray); J + 1 is the gripper frame, so the
 * sphere sets of gg_field_paths go in unchanged.  Per sphere c_k = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t_k with
 * R, t of F_f, its cell by the distance field's rule (a centre that is not finite is outside), d = dist2[cell] or
 * `outside`.  slack int32 [M] = min_s (d - need2[s]): GG_FIELD_FAR when S == 0, INT32_MIN for a row with a q that is
 * not finite.  worst int32 [M] = the lowest s that attains the minimum, -1 when S == 0 or the row is not finite.  No
 * atomics.  S <= GG_FIELD_MAX_SPHERES, M <= GG_FIELD_MAX_POSES; M == 0 writes nothing.  q 8-byte aligned, the other
 * arrays 4-byte.
 *
 * gg_arm_self and gg_arm_motion: the arm against itself, and a straight joint-space move against the field and
 * against itself.  The arm, frames, sphere centres c, cell rule, need2 and outside: exactly as gg_arm_clear states
 * them.  New inputs: radius fp64 [S] (metres; THE CALLER'S DUTY: finite, >= 0); pairs, a HOST array of
 * (J + 2) x (J + 2) bytes: the sphere pair s < t is TESTED iff pairs[frame[s]][frame[t]] != 0 (frame clamped as in
 * gg_arm_clear; the caller passes it symmetric); reach fp64 [J][S] (THE CALLER'S DUTY: finite, >= 0; below).
 * S <= GG_ARM_MAX_SELF_SPHERES for both entries.
 *
 * gg_arm_self: q fp64 [M][J].  For every tested pair d2 = (dx dx + dy dy) + dz dz with d = c_s - c_t, g = sqrt(d2) -
 * (r_s + r_t), all fp64, no contraction.  gap fp64 [M] = the minimum g; pair int32 [M][2] = the lexicographically
 * lowest (s, t) that attains it.  With no tested pair: +inf and (-1, -1).  For a q that is not finite: NaN and
 * (-1, -1).  M <= GG_FIELD_MAX_POSES; M == 0 writes nothing.  pairs must not be null here.
 *
 * gg_arm_motion: edges q_a, q_b fp64 [E][J]; res finite and > 0; 1 <= max_samples <= GG_ARM_MAX_SAMPLES; E <=
 * GG_FIELD_MAX_POSES.  Per edge:
 *   1. The sweep bound: b_s = sum_j |q_b[j] - q_a[j]| reach[j][s], added for j ascending onto 0.0; B = max_s b_s, 0
 *      when S == 0.
 *   2. If B > (double)max_samples res the edge is UNRESOLVED: samples = 0, slack = INT32_MIN, slack_at = worst =
 *      gap_at = -1, gap = NaN, pair = (-1, -1).  An edge with an entry of q_a or q_b that is not finite gets the same
 *      outputs.
 *   3. Otherwise n = the smallest integer >= 1 with (double)n res >= B (a division may propose it; these comparisons
 *      decide it), and samples i = 0 .. n at q_i[j] = q_a[j] + ((double)i / (double)n) (q_b[j] - q_a[j]), the product
 *      rounded, then the sum; sample n is q_b itself.
 *   4. Per sample gg_arm_clear's (slack, worst) and gg_arm_self's (gap, pair).  samples int32 [E] = n; slack int32 [E]
 *      = the minimum over the samples, slack_at int32 [E] = the lowest i that attains it, worst int32 [E] = the worst
 *      sphere of that sample; gap fp64 [E], gap_at int32 [E], pair int32 [E][2] likewise (with no tested pair at all:
 *      +inf, 0, (-1, -1); with S == 0: slack GG_FIELD_FAR, slack_at 0, worst -1).
 * dist2 null: no field test (dims, grid, need2 and outside are not read): slack = GG_FIELD_FAR, slack_at = worst = -1.
 * pairs null: no self test (radius is not read): gap = +inf, gap_at = -1, pair = (-1, -1).  No atomics; the same
 * inputs give the same bytes; E == 0 writes nothing.
 * WHAT THE OUTPUTS PROVE.  Assume reach[j][s] bounds the speed of sphere s's centre per unit of q_j wherever the
 * joints are within their limits (for a revolute joint: the largest distance of the centre from the joint's axis;
 * for a prismatic one: 1).  PRISMATIC JOINTS MUST BE INSIDE THEIR LIMITS ALONG THE EDGE FOR THE BOUND TO HOLD: THE
 * CALLER'S DUTY.  Along the joint-linear motion q(t) = q_a + t (q_b - q_a) every centre then moves by at most b_s <= B
 * in all, so by at most B / n <= res between consecutive samples, and every point of the motion is within res / 2 of
 * a sampled position of the same sphere.  Hence: slack >= 0 with need2 = the distance field's need2(radius + res / 2,
 * margin, h) proves that the balls of radius + margin about the centres meet no occupied cell at any time of the
 * motion; gap >= self_margin + res proves that no tested pair comes closer than self_margin at any time (from the nearer
 * of the two neighbouring samples the two centres have moved by at most res together).  DESIGN 3.33 has the proof.
 * fp64 arrays 8-byte aligned, the others 4-byte.
 * Null, misaligned or out-of-range arguments: GG_ERR_INVALID_ARG naming the argument, before any launch. */
#define GG_ARM_MAX_JOINTS 8
#define GG_ARM_MAX_ITER 1024
#define GG_ARM_MAX_SELF_SPHERES 256
#define GG_ARM_MAX_SAMPLES 4096
#define GG_ARM_DOUBLES(J) (12 * ((J) + 2) + 6 * (J))
int gg_arm_fk(int num_joints, const double *arm, int num_rows, const double *q, double *frames, gg_stream_t stream);
int gg_arm_follow(int num_joints, const double *arm, int num_paths, int num_waypoints, const float *poses,
                  int num_seeds, const double *seeds, double tol_p, double tol_r, double rot_length, double gain,
                  double lambda_min, double max_step, int max_iter, double *q_out, int32_t *iters, double *resid,
                  int32_t *first_fail, gg_stream_t stream);
int gg_arm_clear(int num_joints, const double *arm, const int32_t *dims, const double *grid, const int32_t *dist2,
                 int num_rows, const double *q, int num_spheres, const float *spheres, const int32_t *frame,
                 const int32_t *need2, int32_t outside, int32_t *slack, int32_t *worst, gg_stream_t stream);
int gg_arm_self(int num_joints, const double *arm, int num_rows, const double *q, int num_spheres,
                const float *spheres, const int32_t *frame, const double *radius, const uint8_t *pairs, double *gap,
                int32_t *pair, gg_stream_t stream);
int gg_arm_motion(int num_joints, const double *arm, const int32_t *dims, const double *grid, const int32_t *dist2,
                  int num_edges, const double *q_a, const double *q_b, int num_spheres, const float *spheres,
                  const int32_t *frame, const int32_t *need2, int32_t outside, const double *radius,
                  const uint8_t *pairs, const double *reach, double res, int max_samples, int32_t *samples,
                  int32_t *slack, int32_t *slack_at, int32_t *worst, double *gap, int32_t *gap_at, int32_t *pair,
                  gg_stream_t stream);

/* ---- arm roadmap: joint-space neighbours and exact shortest routes over a checked graph (csrc/roadmap.hip) --------
 * Source of the contract: none in the reference; the probabilistic roadmap is textbook (Kavraki et al. 1996), every
 * constant is this project's choice (PARITY.md "Arm roadmap").  All three entries are pure functions of their inputs:
 * integer or fixed-order fp64 decisions, the same inputs give the same bytes.
 *
 * gg_roadmap_neighbours: the k nearest nodes of every query in a weighted joint metric.  J = num_joints in
 * 1..GG_ARM_MAX_JOINTS; nodes fp64 [N][J], N <= GG_ROADMAP_MAX_NODES; queries fp64 [M][J], M <= GG_FIELD_MAX_POSES;
 * metric, a HOST array of J doubles, each finite and >= 0; skip int32 [M]: a node index the query must not return, or
 * -1 (null: none); valid uint8 [N], any address (null: every node is valid); k in 1..GG_ROADMAP_MAX_K.
 *   d2(m, i) = ((e_0 e_0 + e_1 e_1) + ...) + e_{J-1} e_{J-1},  e_j = metric[j] (queries[m][j] - nodes[i][j]),
 * all fp64, every operation rounded (no contraction), j ascending.  Node i TAKES PART for query m iff valid[i] != 0,
 * every entry of the node is finite, i != skip[m] and d2 < +inf.  idx int32 [M][k] and d2 fp64 [M][k]: the k nodes
 * that take part of smallest (d2, i), lexicographic, ascending; with fewer than k of them the remaining slots hold -1
 * and +inf.  A query with an entry that is not finite: every slot -1 and NaN.  A node equal to the query under
 * another index is a neighbour at distance 0.  No atomics.  M == 0 writes nothing; N == 0 writes the empty rows.
 * nodes, queries, d2 8-byte aligned; skip, idx 4-byte.
 *
 * THE GRAPH of gg_roadmap_route and gg_roadmap_descend, in CSR: offsets int32 [N + 1], targets and weights int32 [E]
 * with E = num_edges <= 2^27; the edges of node i are offsets[i] .. offsets[i + 1] - 1.  THE CALLER'S DUTY: offsets
 * does not decrease, offsets[0] == 0, offsets[N] <= E (the kernels cut every row to 0..E, so a broken table reads
 * nothing outside the arrays, and computes nothing of use).  max_weight >= 1 and (int64) N max_weight < 2^30, checked
 * on the host: with it no cost of a walk without repeated nodes reaches GG_FIELD_FAR.  Edge e of node i is USABLE iff
 * 0 <= targets[e] < N and 1 <= weights[e] <= max_weight; other edges take no part.  Self loops and parallel edges
 * are allowed.  The graph is directed: an undirected one stores both directions.
 *
 * gg_roadmap_route: cost-to-go for Q = num_queries goal sets.  goal_offsets, a HOST array of Q + 1 ints (checked:
 * starts at 0, does not decrease, at most 2^27 goals); goals int32 [G], G = goal_offsets[Q]: the goals of query q are
 * goals[goal_offsets[q] .. goal_offsets[q + 1] - 1]; a goal outside 0..N-1 takes no part, duplicates take part.
 * cost int32 [Q][N], Q N <= 2^27, written whole: the smallest sum of weights over the walks of usable edges from the
 * node to a goal of the query; 0 on a goal; exactly GG_FIELD_FAR where no walk exists, and everywhere for a query
 * without a goal that takes part.  ignored int64 (device, written): the edges of the rows that are not usable,
 * counted once per call.  The values are integers and relaxation only lowers them, so the result, the greatest fixed
 * point below GG_FIELD_FAR, does not depend on the schedule.  Rounds of pull relaxation, one launch each: every (query,
 * node) takes the minimum over its own row of weights[e] + cost[targets[e]], in place.  No kernel waits for another
 * workgroup.  A changed flag per round is read back once per batch of rounds: THE CALL SYNCHRONISES `stream` AND
 * CANNOT BE CAPTURED INTO A GRAPH.  max_rounds >= 1; rounds_out, a HOST int: the rounds run, the last of which
 * changed nothing.  When max_rounds run out before that the call returns GG_ERR_NOT_CONVERGED; cost then holds VALID
 * UPPER BOUNDS: every value below GG_FIELD_FAR is the weight of a real walk to a goal.  ws: gg_roadmap_route_workspace(N,
 * Q) bytes (0: out of range), 256-byte aligned.  Arrays 4-byte aligned, ignored 8-byte.
 *
 * gg_roadmap_descend: walks down a cost-to-go.  cost int32 [Q][N] as gg_roadmap_route wrote it; query int32 [P] and
 * starts int32 [P]; max_nodes >= 1, P max_nodes <= GG_FIELD_MAX_POSES; path int32 [P][max_nodes], length int32 [P].
 * From a start with cost < GG_FIELD_FAR: while the cost here is not 0, take the usable edge with cost[target] +
 * weight == cost[here] of the LOWEST POSITION IN THE ROW.  Weights are >= 1, so the cost falls strictly and the walk
 * visits no node twice.  length = the nodes of the whole path, start and goal included; 0 for a query or a start out
 * of range, a start at GG_FIELD_FAR, or a cost that is not route's fixed point (no edge fits).  With length >
 * max_nodes the path is cut and length still counts all of it; rows from length on repeat the last node; with
 * length 0 every row is -1: gg_field_descend's behaviour.  No atomics.  P == 0 writes nothing.  Arrays 4-byte aligned.
 *
 * Null, misaligned or out-of-range arguments: GG_ERR_INVALID_ARG naming the argument, before any launch. */
#define GG_ROADMAP_MAX_K 32
#define GG_ROADMAP_MAX_NODES 65536
#define GG_ROADMAP_TILE 256 /* nodes staged per tile by gg_roadmap_neighbours: not part of the result, the tests' edge */
int gg_roadmap_neighbours(int num_joints, int num_nodes, const double *nodes, int num_queries, const double *queries,
                          const double *metric, const int32_t *skip, const uint8_t *valid, int k, int32_t *idx,
                          double *d2, gg_stream_t stream);
size_t gg_roadmap_route_workspace(int num_nodes, int num_queries);
int gg_roadmap_route(int num_nodes, int num_edges, const int32_t *offsets, const int32_t *targets,
                     const int32_t *weights, int32_t max_weight, int num_queries, const int32_t *goal_offsets,
                     const int32_t *goals, int32_t *cost, int64_t *ignored, int max_rounds, int *rounds_out, void *ws,
                     size_t ws_bytes, gg_stream_t stream);
int gg_roadmap_descend(int num_nodes, int num_edges, const int32_t *offsets, const int32_t *targets,
                       const int32_t *weights, int32_t max_weight, int num_queries, const int32_t *cost,
                       int num_paths, const int32_t *query, const int32_t *starts, int max_nodes, int32_t *path,
                       int32_t *length, gg_stream_t stream);

/* ---- arm trajectories: blended corners and the time law under joint limits (csrc/trajectory.hip) -------
 * Source of the contract: none in the reference.  Parabolic corner blends and time parameterisation by reachability
 * over a path grid are textbook (Kunz & Stilman 2012; Pham & Pham 2018), RECALLED, NOT READ; every constant is this
 * project's choice (PARITY.md "Arm trajectories").  Both entries are pure functions of their inputs: fp64 throughout,
 * only + - * / sqrt min max, every operation rounded (no contraction), no atomics, the same inputs give the same bytes.
 *
 * THE PATH.  J = num_joints in 1..GG_ARM_MAX_JOINTS; way fp64 [P][W][J], W = num_waypoints in
 * 1..GG_TRAJ_MAX_WAYPOINTS; length int32 [P]: path p has n = length[p] waypoints, clamped into 1..W; blend fp64
 * [P][W]: f_k = min(max(blend[p][k], 0), 1/2), NaN taken as 0, and f_0 = f_{n-1} = 0 whatever the array holds.
 * d_k = w_{k+1} - w_k.  The parameter s runs over [0, n - 1]; segment k is w_k + (s - k) d_k.  About an interior
 * waypoint with f_k > 0 the corner is replaced on s in [k - f_k, k + f_k] by the quadratic Bezier curve with control
 * points w_k - f_k d_{k-1}, w_k, w_k + f_k d_k: q' runs linearly from d_{k-1} to d_k, q'' = (d_k - d_{k-1}) / (2 f_k)
 * is constant, and q' is continuous along the whole path.  An interior waypoint with f_k = 0 is a STOP, as are both
 * ends.  PIECES, in path order: for k = 0 .. n - 2, the blend about waypoint k (k >= 1 and f_k > 0), then the line of
 * segment k of parameter length L = (1 - f_k) - f_{k+1}, skipped when L <= 0 (f_k = f_{k+1} = 1/2).  Every piece is cut
 * into m = steps equal intervals of Delta = L / m (the blend: L = 2 f_k), 2 <= m <= GG_TRAJ_MAX_STEPS.  The grid has
 * G = m (pieces) <= GG_TRAJ_GRID(W, m) = Gmax intervals and G + 1 points.  With tau = (double)a / (double)m at
 * interval a of its piece, joint by joint:
 *   line   q' = d_k at both ends, q'' = 0; q at the interval's start = w_k + (f_k + tau L) d_k
 *   blend  e = d_k - d_{k-1}; q' = d_{k-1} + tau e at the start, d_{k-1} + ((double)(a + 1) / (double)m) e at the end
 *          and d_k itself when a + 1 == m; q'' = e / L; q at the start = ((w_k - f_k d_{k-1}) + tau (L d_{k-1})) +
 *          (tau tau) (f_k e).
 *
 * gg_traj_time: one launch for P paths.  v_max, a_max: HOST arrays of J doubles, finite and > 0.  Unknowns: x_i = (ds /
 * dt)^2 at grid point i and u_i = d2s / dt2, constant on interval i, so x_{i+1} = x_i + 2 Delta u_i.  On interval i,
 * with two = 2 Delta:
 *   vcap   = min_j (v_j / max(|q'_j| at the start, |q'_j| at the end))^2; a joint with q' = 0 at both ends gives none.
 *   next   = min(xbar_{i+1}, vcap).
 *   rows   per joint and per end, A = q''_j and B = q'_j at the start, or B = two q''_j + q'_j(end) at the far end:
 *          |A x + B u| <= a_j.  B != 0: the upper line u <= c + d x and the lower line u >= -c + d x with c = a_j / |B|,
 *          d = -(A / B).  B == 0 and A != 0: the cap x <= a_j / |A|.  B == 0 and A == 0: no row.
 *          One more row, 0 <= x + two u <= next: upper c = next / two, lower c = 0, both d = -(1 / two).
 *   BACKWARDS from xbar_G = 0: xbar_i = 0 when grid point i is a stop; otherwise max(0, the minimum of vcap, of the caps
 *          and of (c_hi - c_lo) / (d_lo - d_hi) over every (lower, upper) pair of rows with d_lo - d_hi > 0).  At most
 *          (2 J + 1)^2 pairs; a minimum does not depend on its order.  (x, u) = (0, 0) meets every row and the rows are
 *          linear, so the x for which some u meets them form an interval from 0, and xbar_i is its upper end.
 *   FORWARDS from x_0 = 0, t_0 = 0: u_i = min over the upper lines of c + d x_i; x_{i+1} = min(max(x_i + two u_i, 0),
 *          next); t_{i+1} = t_i + two / (sqrt(x_i) + sqrt(x_{i+1})), added in grid order.  infeasible = the largest of
 *          (max over the lower lines of c + d x_i) - u_i over the intervals, and 0: 0 in exact arithmetic.
 * Outputs: count int32 [P] = G; xbar, x, t fp64 [P][Gmax + 1]; u fp64 [P][Gmax]; q_grid fp64 [P][Gmax + 1][J], q at
 * every grid point (the last: w_{n-1} itself), null: not written; duration fp64 [P] = t_G; infeasible fp64 [P]; status
 * int32 [P]: GG_TRAJ_OK; GG_TRAJ_NOT_FINITE: a waypoint of the path is not finite; GG_TRAJ_ZERO_SEGMENT: a d_k is all
 * zeros (checked when every waypoint is finite); GG_TRAJ_NO_DURATION: t_G is not finite.  Entries past the path's own
 * (xbar, x, t, q_grid past point G; u from interval G on) are NaN.  A status that is not OK gives count 0 and NaN in
 * every row, in duration and in infeasible.  A path of one waypoint: count 0, duration 0, xbar_0 = x_0 = t_0 = 0,
 * q_grid row 0 = w_0.  Neighbouring paths do not see each other.  P (Gmax + 1) <= GG_FIELD_MAX_POSES; P == 0 writes
 * nothing.  THE CALLER'S DUTY: |w| small enough that no d_k overflows.
 *
 * gg_traj_sample: way, length, blend, steps as above; count, x, u, t, duration, status as gg_traj_time wrote them (THE
 * CALLER'S DUTY; a count that is not the path's own gives NaN rows, never a read outside the arrays).  dt finite and
 * > 0, K = num_samples >= 1, P K <= GG_FIELD_MAX_POSES.  num int32 [P] = one more than the smallest k with (double)k dt
 * >= duration (a division may propose it; these comparisons decide it), at most 2^30; 0 for a status that is not OK.
 * Sample k < num is taken at tt = min((double)k dt, duration): interval i is the last with t_i <= tt, at most G - 1;
 * tau = tt - t_i; r = sqrt(x_i); sd = r + u_i tau; ds = min(max((r + (0.5 u_i) tau) tau, 0), Delta_i); per joint, with
 * q, q', q'' of interval i's start: qp = q' + ds q''; q = (q + ds q') + ((0.5 ds) ds) q''; qd = qp sd; qdd = q'' (sd sd)
 * + qp u_i.  Outputs q, qd, qdd fp64 [P][K][J]; rows k >= num are NaN.  A path of one waypoint: w_0, 0, 0.
 *
 * WHAT THE OUTPUTS PROVE.  On an interval q'_j is linear in s, so |q'_j| takes its maximum at an end: x_i, x_{i+1} <=
 * vcap and x linear in s between them give |dq_j/dt| <= v_j at every instant.  The joint acceleration q''_j x + q'_j u
 * is linear in s as well (x and q' are, u and q'' are constant), so the rows at the two ends bound it at every instant:
 * |d2q_j/dt2| <= a_j.  Both hold up to the rounding that `infeasible` and the clamp of x_{i+1} measure.  The law is
 * the quickest ON ITS GRID; it says nothing about torque, jerk or Cartesian speed.  With f_k <= min(1/2, 2 delta /
 * B_{k-1}, 2 delta / B_k), B_k gg_arm_motion's sweep bound of segment k, no sphere centre leaves the polyline's sweep
 * by more than delta: a route whose edges passed gg_arm_motion with margin >= delta and self_margin >=
 * 2 delta stays proven clear after blending.  fp64 arrays 8-byte aligned, the others 4-byte.
 * Null, misaligned or out-of-range arguments: GG_ERR_INVALID_ARG naming the argument, before any launch. */
#define GG_TRAJ_MAX_WAYPOINTS 64
#define GG_TRAJ_MAX_STEPS 64
#define GG_TRAJ_GRID(W, m) ((W) >= 2 ? (m) * (2 * (W) - 3) : 0)
#define GG_TRAJ_OK 0
#define GG_TRAJ_NOT_FINITE 1
#define GG_TRAJ_ZERO_SEGMENT 2
#define GG_TRAJ_NO_DURATION 3
int gg_traj_time(int num_joints, int num_paths, int num_waypoints, const double *way, const int32_t *length,
                 const double *blend, const double *v_max, const double *a_max, int steps, int32_t *count, double *xbar,
                 double *x, double *u, double *t, double *q_grid, double *duration, double *infeasible, int32_t *status,
                 gg_stream_t stream);
int gg_traj_sample(int num_joints, int num_paths, int num_waypoints, const double *way, const int32_t *length,
                   const double *blend, int steps, const int32_t *count, const double *x, const double *u,
                   const double *t, const double *duration, const int32_t *status, double dt, int num_samples, double *q,
                   double *qd, double *qdd, int32_t *num, gg_stream_t stream);

/* ---- in-library kernel timing (measurement only; off by default) --------------------------------
 * When enabled, every launch of the kernels below is bracketed by a hipEvent pair recorded on the
 * launch stream, so bench.py can report the average duration of exactly that kernel over its
 * timed region (the number a rocprofv3 --kernel-trace --stats run must agree with).
 * gg_prof_get synchronises on the recorded events.  Kernel ids: */
#define GG_K_PROJECT_FWD 0
#define GG_K_PROJECT_BWD 1
#define GG_K_SH_FWD 2
#define GG_K_SH_BWD 3
#define GG_K_BIN_SORT 4   /* the whole gg_bin_sort launch sequence */
#define GG_K_BLEND_PREP 5
#define GG_K_QUAT_FWD 6
#define GG_K_QUAT_BWD 7
#define GG_K_MLP_FWD 8
#define GG_K_MLP_BWD 9
#define GG_K_BLEND_FWD 10 /* + width index: template widths {1,3,4,8,16,32} -> 0..5 */
#define GG_K_BLEND_BWD 20 /* + width index */
#define GG_K_BLEND_VOTES 14 /* gg_blend_votes' walk: in the forward's range, the slot of the 16-wide build that no chunk plan uses */
#define GG_K_BLEND_FWD_PAIR 16 /* 32 channels + a second array of <= 8 in one walk */
#define GG_K_BLEND_BWD_PAIR 17
#define GG_K_COMPACT 26
#define GG_K_DENSIFY 27
#define GG_K_ADAM 28
#define GG_K_VIEW_BWD 29      /* gg_view_bwd: the per-Gaussian backward of a view in one kernel */
#define GG_K_ACTIVATE_FWD 30
#define GG_K_ACTIVATE_BWD 31
#define GG_K_COUNT 18         /* gg_count_intersects */
#define GG_K_TAIL_SPLIT 19    /* gg_shade_tail_bwd_split */
#define GG_K_VIEW_FWD 32      /* gg_view_fwd: activations + projection of a view in one kernel */
#define GG_K_QUERY 33         /* gg_clip_query: weight packing + clip_query_kernel */
#define GG_K_GRASP 34         /* gg_grasp_contacts: both passes and both per-grasp reductions */
#define GG_K_BACKPROJECT 35   /* gg_backproject: count, scan and emit */
#define GG_K_NORMALS 36       /* gg_depth_normals */
#define GG_K_SUBSAMPLE 37     /* gg_subsample: radix select, scan and emit */
#define GG_K_KNN 38           /* gg_knn: grid counting sort and shell search */
#define GG_K_OBJMASK 39       /* gg_object_masks: all six launches */
#define GG_K_VIEW_BWD_POSE 40 /* gg_view_bwd_pose: view_bwd_kernel's pose variant (its finish launch: GG_K_POSE_FINISH) */
#define GG_K_POSE_BWD 41      /* gg_project_pose_bwd: the pose-only pass over the Gaussians */
#define GG_K_POSE_FINISH 42   /* the one-workgroup sum of the pose slab behind either */
#define GG_K_TSDF_INTEGRATE 43 /* gg_tsdf_integrate */
#define GG_K_TSDF_MESH 44     /* gg_tsdf_mesh_count and gg_tsdf_mesh_emit: all their launches */
#define GG_K_GRASP_PROPOSE 45 /* gg_grasp_propose: search, per-seed reduction and rows */
#define GG_K_CLUSTER 46       /* gg_cluster_dbscan: sort, core, union, roots, relabel */
#define GG_K_CLUSTER_STATS 47 /* gg_cluster_stats: all three launches */
#define GG_K_CLOUD_FRAMES 48  /* gg_cloud_frames: init, sort and the frames kernel */
#define GG_K_ICP_STEP 49      /* gg_icp_step: the sort (unless reused), the step kernel and its finishing workgroup */
#define GG_K_GRASP_CLEAR 50   /* gg_grasp_clearance: the pass and the per-grasp reduction */
#define GG_K_GRASP_NMS 51     /* gg_grasp_nms: gather, the pair matrix and the walk */
#define GG_K_SUPPORT_PLANE 52 /* gg_plane_consensus and gg_plane_classify: all their launches */
/* 53 names nothing and stays that way: gg_prof_name(53) is "" (it was the end of the list when tests pinned it) */
#define GG_K_DEPTH_PYRAMID 54 /* gg_depth_min_pyramid: all its launches */
#define GG_K_FIELD_OBSERVE 55 /* gg_field_observe */
#define GG_K_FIELD_DISTANCE_KNOWN 56 /* gg_field_distance_known: its three passes */
#define GG_K_IDS 57           /* ids are below this */
#define GG_PROF_NUM_KERNELS 32
int gg_prof_enable(int on);
int gg_prof_reset(void);
int gg_prof_get(int kernel_id, int *launches, double *total_ms);
const char *gg_prof_name(int kernel_id);

/* y[i] = gg_expf(x[i]) on the device — lets the tests pin the GPU exponential bit-for-bit
 * against the oracle's (gg_constants.h documents the operation sequence). */
int gg_expf_array(int n, const float *x, float *y, gg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GG_RASTER_H */
