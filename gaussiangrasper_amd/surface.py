"""Surface hits: what is under a pixel — which Gaussian, at what depth, which 3-D point, which normal.

The forward walk without colours (`gg_blend_hits`, csrc/hits.hip; contract in include/gg_raster.h) gives, per pixel,
the Gaussian at which the transmittance falls to <= t_hit (the median Gaussian for 0.5), the Gaussian with the largest
blend weight, that weight, and the number of blended Gaussians — bit for bit what the exact forward decides.  On top:

    view_hits(model_or_scene, c2w, intrinsics, h, w, mask, t_hit, full)    -> Hits (ids, depth, points, normals)
    pick(model, camera, pixels)                                            -> (Gaussian ids (M,), points (M, 3))
    pick_instance(model, camera, pixel, instances)                         -> (N,) bool mask of the clicked instance
    locate(model, cameras, positives, negatives)                           -> where the best-matching pixel is
    point_cloud(model, cameras, stride, mask, t_hit)                       -> oriented, coloured cloud of what is seen
    python -m gaussiangrasper_amd.surface --ckpt ... --transforms T.json --out cloud.ply [--pick VIEW U V ...]

A camera is (c2w nerfstudio / OpenGL (3|4, 4), intrinsics fx, fy, cx, cy, height, width), as mesh.mesh_model and
lift.lift_labels take it.  Pixel centres are at integers (u right, v down): a hit at depth z back-projects to
X = ((u - cx) z) / fx, Y = ((v - cy) z) / fy, Z = z in the OpenCV camera frame, as in mesh and prepare.
t_hit = 0.5 and "the normal of the hit Gaussian" are this project's choices (PARITY.md "Surface hits").
Inference only; no GPU work falls back to the host."""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import ArrayLike, require_hip as _require_hip
from .frames import homogeneous

T_HIT = 0.5
_GL_TO_CV = np.diag([1.0, -1.0, -1.0, 1.0])


@dataclass
class Hits:
    """One view's surface hits, device tensors.  hit_idx (H, W) int32: the Gaussian at which T falls to <= t_hit, -1:
    none; top_idx int32 / top_vis float32 / count int32 (None with full=False): the Gaussian of the largest blend
    weight, that weight, the number of blended Gaussians; depth (H, W) float32: the hit Gaussian's camera depth, +inf
    without a hit; points (H, W, 3) float32: the pixel centre back-projected to that depth (world frame), NaN without
    a hit; normals (H, W, 3) float32: the hit Gaussian's smallest axis, turned towards the camera, NaN without a hit.
    Ids index the unmasked model."""
    hit_idx: Tensor
    top_idx: Optional[Tensor]
    top_vis: Optional[Tensor]
    count: Optional[Tensor]
    depth: Tensor
    points: Tensor
    normals: Tensor


def hit_depth(depths: Tensor, hit_idx: Tensor) -> Tensor:
    """depths[hit_idx] bit for bit, +inf where hit_idx is -1."""
    hit = hit_idx >= 0
    d = depths.reshape(-1)[hit_idx.clamp_min(0).long()]
    return torch.where(hit, d, torch.full_like(d, float("inf")))


def _intrinsics(intrinsics: ArrayLike) -> Tuple[float, float, float, float]:
    K = np.asarray(intrinsics.detach().cpu().numpy() if isinstance(intrinsics, Tensor) else intrinsics,
                   dtype=np.float64).reshape(-1)
    if K.shape[0] != 4 or not np.isfinite(K).all() or K[0] == 0.0 or K[1] == 0.0:
        raise ValueError(f"intrinsics must be 4 finite numbers fx, fy, cx, cy with fx, fy != 0, got {intrinsics}")
    return tuple(float(x) for x in K)


def _size(height: int, width: int) -> Tuple[int, int]:
    h, w = int(height), int(width)
    if h != height or w != width or h < 1 or w < 1:
        raise ValueError(f"the image must have at least one pixel, got ({height}, {width})")
    return h, w


def back_project(depth: Tensor, c2w: ArrayLike, intrinsics: ArrayLike) -> Tensor:
    """(H, W, 3) float32 world points of the pixel centres at `depth` (H, W) float32: fp64 arithmetic on the fp32
    depth, rounded once; NaN where the depth is not finite."""
    fx, fy, cx, cy = _intrinsics(intrinsics)
    M = homogeneous(c2w) @ _GL_TO_CV                       # OpenCV camera-to-world
    h, w = depth.shape
    dev = depth.device
    z = depth.double()
    u = torch.arange(w, device=dev, dtype=torch.float64)[None, :]
    v = torch.arange(h, device=dev, dtype=torch.float64)[:, None]
    X = ((u - cx) * z) / fx
    Y = ((v - cy) * z) / fy
    out = [((M[k, 0] * X + M[k, 1] * Y) + M[k, 2] * z) + M[k, 3] for k in range(3)]
    pts = torch.stack(out, dim=-1)
    pts = torch.where(torch.isfinite(z)[..., None], pts, torch.full_like(pts, float("nan")))
    return pts.float()


@torch.no_grad()
def view_hits(model_or_scene, c2w: ArrayLike, intrinsics: ArrayLike, height: int, width: int,
              mask: Optional[Tensor] = None, t_hit: float = T_HIT, full: bool = True) -> Hits:
    """The surface hits of one view (projection as lift.project_view / mesh.render_depth run it, then
    ops.blend_hits on the view's tile lists).  mask (N,) bool walks only the selected Gaussians; the ids returned still
    index the whole model.  full=False: hit_idx, depth, points and normals only, from the walk that stops at the hit."""
    from . import lift, ops
    from .pipeline import smallest_axis_normals
    h, w = _size(height, width)
    _intrinsics(intrinsics)
    t_hit = ops.check_t_hit(t_hit)
    M = homogeneous(c2w)
    src = model_or_scene
    n = src.means.shape[0]
    if mask is not None and mask.numel() != n:
        raise ValueError(f"mask has {mask.numel()} entries for {n} Gaussians")
    dev = _require_hip(src.means, src.scales, src.quats, src.opacities)
    index = None
    if mask is not None:
        mask = mask.reshape(-1).to(device=dev, dtype=torch.bool)
        index = torch.nonzero(mask).reshape(-1).to(torch.int32)
        src = _Selected(src, mask)
    if src.means.shape[0] == 0:
        depths = torch.zeros(0, device=dev)
        outs = ops.blend_hits(torch.zeros(0, 2, device=dev), depths, torch.zeros(0, dtype=torch.int32, device=dev),
                              torch.zeros(0, 3, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                              torch.zeros(0, 1, device=dev), h, w, t_hit, full)
    else:
        proj = lift.project_view(src, M, intrinsics, h, w)
        depths = proj[1]
        outs = ops.blend_hits(*proj, h, w, t_hit, full)
    hit_idx, top_idx, top_vis, count = outs
    hit = hit_idx >= 0
    depth = hit_depth(depths, hit_idx) if depths.numel() else torch.full((h, w), float("inf"), device=dev)
    if index is not None:                               # ids of the unmasked model
        remap = lambda t: torch.where(t >= 0, index[t.clamp_min(0).long()], t) if index.numel() else t  # noqa: E731
        hit_idx = remap(hit_idx)
        top_idx = None if top_idx is None else remap(top_idx)
    points = back_project(depth, M, intrinsics)
    nan3 = torch.full((h, w, 3), float("nan"), device=dev)
    if n == 0 or not bool(hit.any()):
        normals = nan3
    else:
        whole = model_or_scene
        nrm = smallest_axis_normals(whole.quats.detach().float(), whole.scales.detach().float(), ops.quat_to_rotmat)
        nrm = nrm.float()[hit_idx.clamp_min(0).long()]
        cam = torch.as_tensor(M[:3, 3], device=dev, dtype=torch.float64)
        d = cam - points.double()
        nd = nrm.double()
        dot = (nd[..., 0] * d[..., 0] + nd[..., 1] * d[..., 1]) + nd[..., 2] * d[..., 2]
        nrm = torch.where((dot < 0)[..., None], -nrm, nrm)
        normals = torch.where(hit[..., None], nrm, nan3)
    return Hits(hit_idx, top_idx, top_vis, count, depth, points, normals)


class _Selected:
    """The Gaussians a mask selects, with the attributes the projection reads."""

    def __init__(self, src, mask: Tensor):
        self.means, self.scales = src.means.detach()[mask], src.scales.detach()[mask]
        self.quats, self.opacities = src.quats.detach()[mask], src.opacities.detach()[mask]


def _camera(camera) -> Tuple[np.ndarray, Tuple[float, float, float, float], int, int]:
    try:
        c2w, K, h, w = camera
    except (TypeError, ValueError):
        raise ValueError("a camera is (c2w (3|4, 4), intrinsics fx, fy, cx, cy, height, width)") from None
    h, w = _size(h, w)
    return homogeneous(c2w), _intrinsics(K), h, w


def _pixels(pixels: ArrayLike, h: int, w: int) -> np.ndarray:
    """(M, 2) int64 pixels (u, v) = (column, row) inside the (h, w) image, or ValueError."""
    a = np.asarray(pixels.detach().cpu().numpy() if isinstance(pixels, Tensor) else pixels)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"pixels must be (M, 2) integers (u, v), got {a.shape}")
    if a.size and not np.issubdtype(a.dtype, np.integer):
        if not (np.isfinite(a.astype(np.float64)).all() and (a == np.floor(a)).all()):
            raise ValueError("pixels must be whole numbers (u, v)")
    a = a.astype(np.int64)
    bad = (a[:, 0] < 0) | (a[:, 0] >= w) | (a[:, 1] < 0) | (a[:, 1] >= h)
    if bad.any():
        u, v = a[np.nonzero(bad)[0][0]]
        raise ValueError(f"pixel ({u}, {v}) is outside the {w} x {h} image")
    return a


def pick(model_or_scene, camera, pixels: ArrayLike, t_hit: float = T_HIT,
         mask: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """What is under the pixels (M, 2) int (u, v) = (column, row) of `camera`: (ids (M,) int32, points (M, 3) float32)
    of view_hits at those pixels, on the device.  A miss gives -1 / NaN; a pixel outside the image is a ValueError."""
    c2w, K, h, w = _camera(camera)
    px = _pixels(pixels, h, w)
    hits = view_hits(model_or_scene, c2w, K, h, w, mask, t_hit, full=False)
    dev = hits.hit_idx.device
    u, v = torch.as_tensor(px[:, 0], device=dev), torch.as_tensor(px[:, 1], device=dev)
    return hits.hit_idx[v, u], hits.points[v, u]


def pick_instance(model_or_scene, camera, pixel: ArrayLike, instances, t_hit: float = T_HIT) -> Tensor:
    """(N,) bool mask of the instance (cluster.Instances over the model's Gaussians) that owns the Gaussian under
    `pixel` (u, v).  A Gaussian of no instance (-1, noise) falls back to cluster.instance_mask(instances, point): the
    instance whose centroid is nearest to the hit point.  A miss is a ValueError."""
    from .cluster import instance_mask
    n = model_or_scene.means.shape[0]
    if instances.ids.shape[0] != n:
        raise ValueError(f"instances cover {instances.ids.shape[0]} points, the model has {n} Gaussians")
    ids, pts = pick(model_or_scene, camera, np.asarray(pixel).reshape(1, 2), t_hit)
    g = int(ids[0])
    if g < 0:
        raise ValueError(f"nothing is under pixel {tuple(int(x) for x in np.asarray(pixel).reshape(2))}")
    inst = int(instances.ids[g])
    if inst >= 0:
        return instances.ids == inst
    return instance_mask(instances, pts[0].double().cpu().numpy())


@torch.no_grad()
def locate(model_or_scene, cameras, positives: ArrayLike, negatives: ArrayLike, fea_up=None,
           temperature: Optional[float] = None, t_hit: float = T_HIT):
    """Where a text query is in the world: (point (3,) float32 on the device, view index, pixel (u, v), relevancy) of
    the pixel with the largest LERF relevancy (query.relevancy of the rendered feature image, the largest over the
    positives; the image is rendered as query.lift_relevancy renders it) over `cameras`, among the pixels with a hit.
    ValueError when no pixel of any view has a hit."""
    from . import lift, ops, query
    fea_up = getattr(model_or_scene, "fea_up", None) if fea_up is None else fea_up
    feat = query._gaussian_features(model_or_scene)
    dev = _require_hip(feat)
    feat = feat.float().contiguous()
    tau = query.DEFAULT_TEMPERATURE if temperature is None else temperature
    ones = torch.ones(feat.shape[0], 1, device=dev)
    best = None
    for k, cam in enumerate(cameras):
        c2w, K, h, w = _camera(cam)
        if feat.shape[0] == 0:
            continue
        proj = lift.project_view(model_or_scene, c2w, K, h, w)
        hit_idx = ops.blend_hits(*proj, h, w, t_hit, full=False)[0]      # view_hits' hits, on this projection
        hit = hit_idx >= 0
        if not bool(hit.any()):
            continue
        img = ops.rasterize_segments(*proj, h, w, [(feat, torch.zeros(feat.shape[1], device=dev)),
                                                   (ones, torch.zeros(1, device=dev))])[0]
        rel = query.relevancy(img, fea_up, positives, negatives, tau).max(dim=-1).values
        rel = torch.where(hit, rel, torch.full_like(rel, -float("inf")))
        flat = int(torch.argmax(rel.reshape(-1)))
        r = float(rel.reshape(-1)[flat])
        if best is None or r > best[3]:
            v, u = divmod(flat, w)
            best = (back_project(hit_depth(proj[1], hit_idx), c2w, K)[v, u], k, (u, v), r)
    if best is None:
        raise ValueError("no pixel of any view has a hit")
    return best


@torch.no_grad()
def point_cloud(model_or_scene, cameras, stride: int = 1, mask: Optional[Tensor] = None, t_hit: float = T_HIT):
    """An oriented, coloured cloud of what `cameras` see: (points (M, 3) float32, normals (M, 3) float32, colors
    (M, 3) float32 in [0, 1], gaussian_ids (M,) int32), one row per hit pixel of every view (every `stride`-th row and
    column), view-major, then row-major.  The colour is the rendered colour at the pixel (mesh.render_depth's rgb)."""
    from .mesh import render_depth
    s = int(stride)
    if s != stride or s < 1:
        raise ValueError(f"stride must be an integer >= 1, got {stride}")
    cams = [_camera(c) for c in cameras]
    dev = _require_hip(model_or_scene.means)
    parts = []
    for c2w, K, h, w in cams:
        hits = view_hits(model_or_scene, c2w, K, h, w, mask, t_hit, full=False)
        rgb = render_depth(model_or_scene, c2w, K, h, w, mask)[1]
        sel = hits.hit_idx[::s, ::s] >= 0
        parts.append((hits.points[::s, ::s][sel], hits.normals[::s, ::s][sel], rgb[::s, ::s][sel],
                      hits.hit_idx[::s, ::s][sel]))
    if not parts:
        z3 = torch.zeros(0, 3, device=dev)
        return z3, z3.clone(), z3.clone(), torch.zeros(0, dtype=torch.int32, device=dev)
    return tuple(torch.cat([p[k] for p in parts]) for k in range(4))


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def write_ply_cloud(path: str, points, normals, colors) -> None:
    """The cloud as a binary PLY of vertices x, y, z, nx, ny, nz, red, green, blue (mesh.write_ply_mesh's vertex
    layout, no faces)."""
    from .mesh import Mesh, write_ply_mesh
    f = lambda t: t.detach().cpu().numpy() if isinstance(t, Tensor) else np.asarray(t)  # noqa: E731
    write_ply_mesh(path, Mesh(f(points), np.zeros((0, 3), np.int32), f(normals), f(colors)))


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.surface",
                                 description="Oriented point cloud of what a scan's cameras see of a checkpoint, and "
                                             "the Gaussians and 3-D points under picked pixels.")
    ap.add_argument("--ckpt", required=True, help="step-*.ckpt of a splatting model")
    ap.add_argument("--transforms", required=True, help="the scan's transforms.json (OpenCV c2w, raw frame)")
    ap.add_argument("--transform-json", default=None, help="dataparser_transforms.json (transform_matrix, scale) from "
                                                           "the scan's frame to the checkpoint's; outputs go back")
    ap.add_argument("--out", default=None, help="output .ply: the cloud of every view's hit pixels")
    ap.add_argument("--stride", type=int, default=1, help="take every S-th row and column (default 1)")
    ap.add_argument("--t-hit", type=float, default=T_HIT, help="the transmittance at which a pixel hits (default 0.5)")
    ap.add_argument("--pick", type=int, nargs="+", default=None, metavar="N",
                    help="VIEW U V triples: frame index, column, row of pixels to pick")
    ap.add_argument("--out-pick", default=None, help="with --pick: output .json of the picks")
    return ap


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = _parser()
    a = ap.parse_args(argv)
    if not a.out and not a.pick:
        ap.error("one of --out and --pick is needed")
    if a.stride < 1:
        ap.error(f"--stride must be >= 1, got {a.stride}")
    if not 1e-4 < a.t_hit < 1.0:
        ap.error(f"--t-hit must be in (1e-4, 1), got {a.t_hit}")
    if a.pick is not None and len(a.pick) % 3 != 0:
        ap.error("--pick takes VIEW U V triples")
    if bool(a.pick) != bool(a.out_pick):
        ap.error("--pick and --out-pick go together")
    try:
        from .lift import scene_cameras
        cams, tf = scene_cameras(a.transforms, a.transform_json)
        picks = np.asarray(a.pick or [], dtype=np.int64).reshape(-1, 3)
        for view, u, v in picks:
            if not 0 <= view < len(cams):
                raise ValueError(f"--pick: view {view} of {len(cams)}")
            _pixels(np.asarray([[u, v]]), int(cams[view][2]), int(cams[view][3]))
        from ._cli import load_scene
        scene, _ = load_scene(a.ckpt)
        from .frames import directions_from_scene, points_from_scene
        if a.out:
            pts, nrm, col, ids = point_cloud(scene, cams, a.stride, None, a.t_hit)
            pts, nrm = pts.cpu().numpy(), nrm.cpu().numpy()
            if tf is not None and len(pts):
                pts = points_from_scene(pts, *tf).astype(np.float32)
                nrm = directions_from_scene(nrm, tf[0]).astype(np.float32)
            write_ply_cloud(a.out, pts, nrm, col)
            print(f"{len(pts)} points of {len(cams)} views -> {a.out}")
        if a.pick:
            rows = []
            for view, u, v in picks:
                ids, p = pick(scene, cams[view], np.asarray([[u, v]]), a.t_hit)
                g, p = int(ids[0]), p[0].double().cpu().numpy()
                if g >= 0 and tf is not None:
                    p = points_from_scene(p[None], *tf)[0]
                rows.append({"view": int(view), "pixel": [int(u), int(v)], "gaussian": g,
                             "point": [float(x) for x in p] if g >= 0 else None})
            if os.path.dirname(a.out_pick):
                os.makedirs(os.path.dirname(a.out_pick), exist_ok=True)
            with open(a.out_pick, "w") as f:
                json.dump(rows, f, indent=1)
            print(f"{sum(r['gaussian'] >= 0 for r in rows)} of {len(rows)} picks hit -> {a.out_pick}")
    except (KeyError, ValueError, OSError, _lib.GGError) as exc:
        print(f"error: {exc}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
