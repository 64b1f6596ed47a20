"""Normal-guided grasp filtering (GaussianGrasper step 4): keep a grasp candidate only when both finger contacts on
the Gaussian field satisfy the friction-cone condition.  One HIP call (`gg_grasp_contacts`, csrc/grasp.hip) tests
every candidate against every oriented point in fp64; the contract is in include/gg_raster.h and PARITY.md
"Grasp filtering".

    load_grasps        (M, 17) GraspGroup rows [score, width, height, depth, R (9), t (3), object_id]
    grasps_to_scene    grasp frame -> world (camera pose) -> scene (the edit's transform_matrix and scale)
    model_points       means, smallest-axis normals and sigmoid(opacity) [x mask] of a model or scene
    contacts           the per-grasp outputs of gg_grasp_contacts (GraspContacts)
    filter_grasps      indices of the feasible grasps, by score, descending, stable
    score_grasps       all of the above on a model in one call
    python -m gaussiangrasper_amd.grasp --ckpt IN --grasps grasps.npy [...] --out kept.npy

Grasp candidates come from outside the project (AnyGrasp): this module only scores them."""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import sys
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .ops import _ptr, _require_hip, _stream

ArrayLike = Union[np.ndarray, Tensor, Sequence]

GRASP_COLS = 17
# UNVERIFIED defaults (PARITY.md "Grasp filtering"), in grasp units (metres): graspnetAPI's gripper drawing for
# depth_base and finger_width; band, mu and min_weight are this project's choices
DEPTH_BASE = 0.02
FINGER_WIDTH = 0.004
BAND = 0.003
MU = 0.5
MIN_WEIGHT = 0.0
ORTHO_TOL = 1e-4


@dataclass
class GraspContacts:
    """Per-grasp outputs of one gg_grasp_contacts call, device tensors; M = number of grasps."""
    contact_idx: Tensor        # (M, 2) int32: left / right contact point, -1 when the region is empty
    normals: Tensor            # (M, 2, 3) float32: unit outward patch normals, NaN when not valid
    angles: Tensor             # (M, 2) float32: radians to the closing direction, NaN when not valid
    region_count: Tensor       # (M,) int32
    region_weight: Tensor      # (M,) float32
    collision_weight: Tensor   # (M,) float32
    feasible: Tensor           # (M,) bool


# ------------------------------------------------------------------------------------------------
# host side: candidates and frames (numpy, fp64)
# ------------------------------------------------------------------------------------------------
def load_grasps(path: str) -> np.ndarray:
    """(M, 17) float32 GraspGroup rows from a .npy file."""
    g = np.load(path)
    if g.ndim != 2 or g.shape[1] != GRASP_COLS:
        raise ValueError(f"{path}: expected (M, {GRASP_COLS}) GraspGroup rows, got {g.shape}")
    return np.ascontiguousarray(g, dtype=np.float32)


def _check_grasp_array(grasps: ArrayLike) -> np.ndarray:
    g = grasps.detach().cpu().numpy() if isinstance(grasps, Tensor) else np.asarray(grasps)
    if g.ndim != 2 or g.shape[1] != GRASP_COLS:
        raise ValueError(f"grasps must be (M, {GRASP_COLS}) GraspGroup rows, got {g.shape}")
    return g


def _check_rotation(R: np.ndarray, what: str) -> None:
    err = np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max(initial=0.0)
    if not err <= ORTHO_TOL:
        raise ValueError(f"{what} is not orthonormal (max |R^T R - I| = {err:.3g} > {ORTHO_TOL:g})")


def grasps_to_scene(grasps: ArrayLike, cam_to_world: Optional[ArrayLike] = None, matrix: Optional[ArrayLike] = None,
                    scale: float = 1.0) -> np.ndarray:
    """GraspGroup rows from the grasp (camera) frame into the scene frame: R' = M3 C3 R,
    t' = scale (M3 (C3 t + C_t) + M_t), width, height and depth times scale (the world -> scene mapping of
    edit.object_points_to_scene).  cam_to_world: 4x4 grasp frame -> world (None: identity); matrix: the scene's
    transform_matrix (3x4 or 4x4, None: identity).  Rows whose R is finite must be orthonormal within 1e-4, as must
    C3 and M3; rows with a non-finite entry pass through (they are not valid grasps).  Returns (M, 17) float32."""
    g = _check_grasp_array(grasps).astype(np.float64)
    C = np.eye(4) if cam_to_world is None else np.asarray(cam_to_world, dtype=np.float64)
    Mx = np.eye(4) if matrix is None else np.asarray(matrix, dtype=np.float64)
    if C.shape != (4, 4):
        raise ValueError(f"cam_to_world must be 4x4, got {C.shape}")
    if Mx.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"matrix must be 3x4 or 4x4, got {Mx.shape}")
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError(f"scale must be finite and > 0, got {scale}")
    _check_rotation(C[:3, :3], "cam_to_world rotation")
    _check_rotation(Mx[:3, :3], "matrix rotation")
    R = g[:, 4:13].reshape(-1, 3, 3)
    fin = np.isfinite(R).all(axis=(1, 2))
    _check_rotation(R[fin], "grasp rotation")
    A = Mx[:3, :3] @ C[:3, :3]
    out = g.copy()
    out[:, 4:13] = (A @ R).reshape(-1, 9)
    t = g[:, 13:16]
    out[:, 13:16] = scale * ((t @ C[:3, :3].T + C[:3, 3]) @ Mx[:3, :3].T + Mx[:3, 3])
    out[:, 1:4] *= scale
    return out.astype(np.float32)


def filter_grasps(grasps: ArrayLike, feasible: Union[GraspContacts, ArrayLike]) -> Tensor:
    """Indices (int64) of the feasible grasps, sorted by score (column 0) descending; equal scores keep their input
    order.  On the device of `feasible`."""
    f = feasible.feasible if isinstance(feasible, GraspContacts) else torch.as_tensor(feasible)
    f = f.reshape(-1).to(torch.bool)
    g = torch.as_tensor(_check_grasp_array(grasps) if not isinstance(grasps, Tensor) else grasps)
    if g.ndim != 2 or g.shape[1] != GRASP_COLS or g.shape[0] != f.shape[0]:
        raise ValueError(f"grasps {tuple(g.shape)} and feasible {tuple(f.shape)} do not match")
    idx = torch.nonzero(f).reshape(-1)
    score = g[:, 0].to(device=f.device, dtype=torch.float64)[idx]
    order = torch.sort(score, descending=True, stable=True).indices
    return idx[order]


# ------------------------------------------------------------------------------------------------
# device side: one gg_grasp_contacts call
# ------------------------------------------------------------------------------------------------
def _f32_rows(t: Tensor, name: str, width: Optional[int]) -> Tensor:
    shape_ok = t.ndim == 2 and t.shape[1] == width if width else t.ndim == 1
    if t.dtype != torch.float32 or not shape_ok:
        want = f"(N, {width})" if width else "(N,)"
        raise ValueError(f"{name} must be a float32 {want} tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _param(name: str, v: float) -> float:
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{name} must be finite and >= 0, got {v}")
    return v


def contacts(points: Tensor, normals: Tensor, weights: Tensor, grasps: Tensor, depth_base: float = DEPTH_BASE,
             finger_width: float = FINGER_WIDTH, band: float = BAND, mu: float = MU, min_weight: float = MIN_WEIGHT,
             max_collision: Optional[float] = None) -> GraspContacts:
    """Finger contacts, outward patch normals, friction-cone angles and feasibility of every grasp against the
    oriented points (include/gg_raster.h gg_grasp_contacts).  points / normals (N, 3), weights (N,), grasps (M, 17):
    float32 on the HIP device (no CPU path).  Lengths (depth_base, finger_width, band) are in the grasps' units.
    max_collision None: no collision limit.  One call; nothing waits on the host."""
    dev = _require_hip(points, normals, weights, grasps)
    points = _f32_rows(points, "points", 3)
    normals = _f32_rows(normals, "normals", 3)
    weights = _f32_rows(weights, "weights", None)
    grasps = _f32_rows(grasps, "grasps", GRASP_COLS)
    n, m = points.shape[0], grasps.shape[0]
    if normals.shape[0] != n or weights.shape[0] != n:
        raise ValueError(f"points has {n} rows, normals {normals.shape[0]}, weights {weights.shape[0]}")
    mc = math.inf if max_collision is None else float(max_collision)
    if math.isnan(mc) or math.isnan(float(min_weight)):
        raise ValueError("min_weight and max_collision must not be NaN")
    args = (_param("depth_base", depth_base), _param("finger_width", finger_width), _param("band", band),
            _param("mu", mu), float(min_weight), mc)
    lib = _lib.load()
    res = GraspContacts(
        contact_idx=torch.empty(m, 2, dtype=torch.int32, device=dev),
        normals=torch.empty(m, 2, 3, dtype=torch.float32, device=dev),
        angles=torch.empty(m, 2, dtype=torch.float32, device=dev),
        region_count=torch.empty(m, dtype=torch.int32, device=dev),
        region_weight=torch.empty(m, dtype=torch.float32, device=dev),
        collision_weight=torch.empty(m, dtype=torch.float32, device=dev),
        feasible=torch.empty(m, dtype=torch.uint8, device=dev))
    nbytes = lib.gg_grasp_contacts_workspace(n, m)
    if m > 0 and nbytes == 0:
        raise ValueError(f"{n} points x {m} grasps is beyond gg_grasp_contacts' limits")
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    _lib.check(lib.gg_grasp_contacts(n, _ptr(points), _ptr(normals), _ptr(weights), m, _ptr(grasps), *args,
                                     _ptr(res.contact_idx), _ptr(res.normals), _ptr(res.angles),
                                     _ptr(res.region_count), _ptr(res.region_weight), _ptr(res.collision_weight),
                                     _ptr(res.feasible), _ptr(ws), ctypes.c_size_t(ws.numel()), _stream(dev)),
               "gg_grasp_contacts")
    res.feasible = res.feasible.bool()
    return res


@torch.no_grad()
def model_points(model_or_scene, mask: Optional[Tensor] = None):
    """(points, normals, weights) of a model or scene: the means, the smallest-axis normals as the renderer forms
    them (pipeline.smallest_axis_normals with ops.quat_to_rotmat) and sigmoid(opacities), times `mask` (N,) bool
    or float when given.  float32 device tensors."""
    from . import ops
    from .pipeline import smallest_axis_normals
    means, quats = model_or_scene.means.detach(), model_or_scene.quats.detach()
    scales, opac = model_or_scene.scales.detach(), model_or_scene.opacities.detach()
    _require_hip(means, quats, scales, opac)
    normals = smallest_axis_normals(quats, scales, ops.quat_to_rotmat).float().contiguous()
    weights = torch.sigmoid(opac.float()).reshape(-1)
    if mask is not None:
        mask = mask.reshape(-1)
        if mask.shape[0] != weights.shape[0]:
            raise ValueError(f"mask has {mask.shape[0]} entries for {weights.shape[0]} Gaussians")
        weights = weights * mask.to(device=weights.device, dtype=torch.float32)
    return means.float().contiguous(), normals, weights.contiguous()


def score_grasps(model_or_scene, grasps: ArrayLike, mask: Optional[Tensor] = None,
                 cam_to_world: Optional[ArrayLike] = None, matrix: Optional[ArrayLike] = None, scale: float = 1.0,
                 depth_base: float = DEPTH_BASE, finger_width: float = FINGER_WIDTH, band: float = BAND,
                 mu: float = MU, min_weight: float = MIN_WEIGHT,
                 max_collision: Optional[float] = None) -> GraspContacts:
    """Candidates in the grasp frame, scored against the model's Gaussians in one call: grasps_to_scene, then
    contacts on model_points.  depth_base, finger_width and band are in grasp units and scaled with the grasps."""
    pts, nrm, w = model_points(model_or_scene, mask)
    g = grasps_to_scene(grasps, cam_to_world, matrix, scale)
    s = float(scale)
    return contacts(pts, nrm, w, torch.from_numpy(g).to(pts.device), _param("depth_base", depth_base) * s,
                    _param("finger_width", finger_width) * s, _param("band", band) * s, mu, min_weight,
                    max_collision)


# ------------------------------------------------------------------------------------------------
# command line: filter a candidate file against a checkpoint
# ------------------------------------------------------------------------------------------------
def _load_matrix(path: str, shape, name: str) -> np.ndarray:
    a = np.asarray(np.load(path), dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{name} {path}: expected {shape}, got {a.shape}")
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.grasp",
                                 description="Filter grasp candidates (GraspGroup rows) by the friction cone at both "
                                             "finger contacts on a checkpoint's Gaussians.")
    ap.add_argument("--ckpt", required=True, help="step-*.ckpt of a splatting model")
    ap.add_argument("--grasps", required=True, help=".npy (M, 17) GraspGroup rows, grasp frame")
    ap.add_argument("--camera-pose", default=None, help=".npy 4x4, grasp frame -> world")
    ap.add_argument("--transform-json", default=None, help="JSON with transform_matrix and scale (world -> scene)")
    ap.add_argument("--object-points", default=None, help="object point cloud (world frame): its convex hull "
                                                          "restricts the Gaussians")
    ap.add_argument("--positives", default=None, help=".npy text embeddings: the query restricts the Gaussians")
    ap.add_argument("--negatives", default=None, help=".npy canonical negatives (LERF relevancy)")
    ap.add_argument("--threshold", type=float, default=None, help="relevancy threshold for --positives")
    ap.add_argument("--mu", type=float, default=MU, help="friction coefficient")
    ap.add_argument("--band", type=float, default=BAND, help="contact patch depth, grasp units")
    ap.add_argument("--min-opacity", type=float, default=MIN_WEIGHT, help="a Gaussian takes part above it")
    ap.add_argument("--max-collision", type=float, default=None, help="limit on the opacity inside the fingers")
    ap.add_argument("--out", required=True, help="output .npy: feasible rows, input frame, by score")
    ap.add_argument("--report", default=None, help="output .npz: every per-grasp output, scene frame")
    a = ap.parse_args(argv)
    if a.object_points and a.positives:
        ap.error("--object-points and --positives are alternatives")
    if a.positives and (a.threshold is None or not a.negatives):
        ap.error("--positives needs --negatives and --threshold (LERF relevancy, query.select_gaussians)")
    if (a.negatives or a.threshold is not None) and not a.positives:
        ap.error("--negatives / --threshold need --positives")
    for name in ("mu", "band", "min_opacity"):
        v = getattr(a, name)
        if not (math.isfinite(v) and v >= 0.0):
            ap.error(f"--{name.replace('_', '-')} must be finite and >= 0, got {v}")
    if a.max_collision is not None and math.isnan(a.max_collision):
        ap.error("--max-collision must not be NaN")
    try:
        grasps = load_grasps(a.grasps)
        cam = _load_matrix(a.camera_pose, (4, 4), "camera pose") if a.camera_pose else None
        matrix, scale = None, 1.0
        if a.transform_json:
            with open(a.transform_json) as f:
                tj = json.load(f)
            matrix, scale = np.asarray(tj["transform_matrix"], dtype=np.float64), float(tj["scale"])
        from .interop import load_checkpoint
        scene, mlp_state, _ = load_checkpoint(a.ckpt)
        dev = torch.device("cuda")
        scene = scene.to(dev)
        mask = None
        if a.object_points:
            from . import edit
            pts = edit.filter_object_points(edit.object_points_to_scene(
                edit.load_object_points(a.object_points), np.eye(4) if matrix is None else matrix, scale))
            mask, _ = edit.select_and_move(scene.means.contiguous(), None, edit.hull_planes(pts))
        elif a.positives:
            from . import query
            keys = ("layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias")
            if any(k not in mlp_state for k in keys):
                raise KeyError(f"{a.ckpt}: no fea_up weights for --positives")
            w = tuple(mlp_state[k].to(dev) for k in keys)
            pos = query._load_embeddings(a.positives, "positives")
            neg = query._load_embeddings(a.negatives, "negatives")
            mask = query.select_gaussians(scene, w, pos, neg, a.threshold)
        res = score_grasps(scene, grasps, mask, cam, matrix, scale, band=a.band, mu=a.mu, min_weight=a.min_opacity,
                           max_collision=a.max_collision)
    except (KeyError, ValueError, OSError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    keep = filter_grasps(grasps, res).cpu().numpy()
    np.save(a.out, grasps[keep])
    if a.report:
        np.savez(a.report, grasps_scene=grasps_to_scene(grasps, cam, matrix, scale),
                 **{k: getattr(res, k).cpu().numpy() for k in ("contact_idx", "normals", "angles", "region_count",
                                                               "region_weight", "collision_weight", "feasible")})
    print(f"{len(keep)} of {len(grasps)} grasps feasible; wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
