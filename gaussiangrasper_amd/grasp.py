"""Normal-guided grasp filtering (GaussianGrasper step 4): keep a grasp candidate only when both finger contacts on
the Gaussian field satisfy the friction-cone condition.  One HIP call (`gg_grasp_contacts`, csrc/grasp.hip) tests
every candidate against every oriented point in fp64; the contract is in include/gg_raster.h and PARITY.md
"Grasp filtering".

    load_grasps        (M, 17) GraspGroup rows [score, width, height, depth, R (9), t (3), object_id]
    grasps_to_scene    grasp frame -> world (camera pose) -> scene (the edit's transform_matrix and scale)
    grasps_from_scene  its inverse
    model_points       means, smallest-axis normals and sigmoid(opacity) [x mask] of a model or scene
    contacts           the per-grasp outputs of gg_grasp_contacts (GraspContacts)
    filter_grasps      indices of the feasible grasps, by score, descending, stable
    score_grasps       all of the above on a model in one call
    python -m gaussiangrasper_amd.grasp --ckpt IN --grasps grasps.npy [...] --out kept.npy

Grasp candidates come from outside the project (AnyGrasp): this module only scores them."""
from __future__ import annotations

import argparse
import math
import sys
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (ArrayLike, f32_rows, nonneg, ptr as _ptr, require_hip as _require_hip, stream as _stream,
                    workspace as _ws)
from ._cli import REPORT_KEYS, add_object_options, check_object_options, object_mask
from .frames import ORTHO_TOL, load_transform_json, rigid_to_scene  # noqa: F401

GRASP_COLS = 17
# UNVERIFIED defaults (PARITY.md "Grasp filtering"), in grasp units (metres): graspnetAPI's gripper drawing for
# depth_base and finger_width; band, mu and min_weight are this project's choices
DEPTH_BASE = 0.02
FINGER_WIDTH = 0.004
BAND = 0.003
MU = 0.5
MIN_WEIGHT = 0.0


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


def check_grasp_array(grasps: ArrayLike) -> np.ndarray:
    """`grasps` as a host array, after checking that it is (M, 17)."""
    g = grasps.detach().cpu().numpy() if isinstance(grasps, Tensor) else np.asarray(grasps)
    if g.ndim != 2 or g.shape[1] != GRASP_COLS:
        raise ValueError(f"grasps must be (M, {GRASP_COLS}) GraspGroup rows, got {g.shape}")
    return g


def _map_grasps(grasps: ArrayLike, cam_to_world, matrix, scale: float, inverse: bool) -> np.ndarray:
    g = check_grasp_array(grasps).astype(np.float64)
    R, t, scale = rigid_to_scene(g[:, 4:13].reshape(-1, 3, 3), g[:, 13:16], cam_to_world, matrix, scale, inverse)
    g[:, 4:13], g[:, 13:16] = R.reshape(-1, 9), t
    g[:, 1:4] = g[:, 1:4] / scale if inverse else g[:, 1:4] * scale
    return g.astype(np.float32)


def grasps_to_scene(grasps: ArrayLike, cam_to_world: Optional[ArrayLike] = None, matrix: Optional[ArrayLike] = None,
                    scale: float = 1.0) -> np.ndarray:
    """GraspGroup rows from the grasp (camera) frame into the scene frame: R' = M3 C3 R,
    t' = scale (M3 (C3 t + C_t) + M_t), width, height and depth times scale (the world -> scene mapping of
    edit.object_points_to_scene).  cam_to_world: 4x4 grasp frame -> world (None: identity); matrix: the scene's
    transform_matrix (3x4 or 4x4, None: identity).  Rows whose R is finite must be orthonormal within 1e-4, as must
    C3 and M3; rows with a non-finite entry pass through (they are not valid grasps).  Returns (M, 17) float32."""
    return _map_grasps(grasps, cam_to_world, matrix, scale, False)


def grasps_from_scene(grasps: ArrayLike, cam_to_world: Optional[ArrayLike] = None,
                      matrix: Optional[ArrayLike] = None, scale: float = 1.0) -> np.ndarray:
    """The inverse of grasps_to_scene: scene-frame rows back to the grasp (camera) frame, or to the world frame
    with cam_to_world None.  R = (M3 C3)^T R', t = C3^T (M3^T (t' / scale - M_t) - C_t), width, height and depth
    divided by scale.  The same checks: C3, M3 and every finite R orthonormal within 1e-4.  Returns (M, 17)
    float32."""
    return _map_grasps(grasps, cam_to_world, matrix, scale, True)


def filter_grasps(grasps: ArrayLike, feasible: Union[GraspContacts, ArrayLike]) -> Tensor:
    """Indices (int64) of the feasible grasps, sorted by score (column 0) descending; equal scores keep their input
    order.  On the device of `feasible`."""
    f = feasible.feasible if isinstance(feasible, GraspContacts) else torch.as_tensor(feasible)
    f = f.reshape(-1).to(torch.bool)
    g = torch.as_tensor(check_grasp_array(grasps) if not isinstance(grasps, Tensor) else grasps)
    if g.ndim != 2 or g.shape[1] != GRASP_COLS or g.shape[0] != f.shape[0]:
        raise ValueError(f"grasps {tuple(g.shape)} and feasible {tuple(f.shape)} do not match")
    idx = torch.nonzero(f).reshape(-1)
    score = g[:, 0].to(device=f.device, dtype=torch.float64)[idx]
    order = torch.sort(score, descending=True, stable=True).indices
    return idx[order]


# ------------------------------------------------------------------------------------------------
# device side: one gg_grasp_contacts call
# ------------------------------------------------------------------------------------------------
def contacts(points: Tensor, normals: Tensor, weights: Tensor, grasps: Tensor, depth_base: float = DEPTH_BASE,
             finger_width: float = FINGER_WIDTH, band: float = BAND, mu: float = MU, min_weight: float = MIN_WEIGHT,
             max_collision: Optional[float] = None) -> GraspContacts:
    """Finger contacts, outward patch normals, friction-cone angles and feasibility of every grasp against the
    oriented points (include/gg_raster.h gg_grasp_contacts).  points / normals (N, 3), weights (N,), grasps (M, 17):
    float32 on the HIP device (no CPU path).  Lengths (depth_base, finger_width, band) are in the grasps' units.
    max_collision None: no collision limit.  One call; nothing waits on the host."""
    dev = _require_hip(points, normals, weights, grasps)
    points = f32_rows(points, "points", 3)
    normals = f32_rows(normals, "normals", 3)
    weights = f32_rows(weights, "weights", None)
    grasps = f32_rows(grasps, "grasps", GRASP_COLS)
    n, m = points.shape[0], grasps.shape[0]
    if normals.shape[0] != n or weights.shape[0] != n:
        raise ValueError(f"points has {n} rows, normals {normals.shape[0]}, weights {weights.shape[0]}")
    mc = math.inf if max_collision is None else float(max_collision)
    if math.isnan(mc) or math.isnan(float(min_weight)):
        raise ValueError("min_weight and max_collision must not be NaN")
    args = (nonneg("depth_base", depth_base), nonneg("finger_width", finger_width), nonneg("band", band),
            nonneg("mu", mu), float(min_weight), mc)
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
    ws = _ws(nbytes, dev)
    _lib.check(lib.gg_grasp_contacts(n, _ptr(points), _ptr(normals), _ptr(weights), m, _ptr(grasps), *args,
                                     _ptr(res.contact_idx), _ptr(res.normals), _ptr(res.angles),
                                     _ptr(res.region_count), _ptr(res.region_weight), _ptr(res.collision_weight),
                                     _ptr(res.feasible), _ptr(ws), ws.numel(), _stream(dev)),
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
    return contacts(pts, nrm, w, torch.from_numpy(g).to(pts.device), nonneg("depth_base", depth_base) * s,
                    nonneg("finger_width", finger_width) * s, nonneg("band", band) * s, mu, min_weight,
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
    add_object_options(ap, "the query restricts the Gaussians", "restricts the Gaussians")
    ap.add_argument("--mu", type=float, default=MU, help="friction coefficient")
    ap.add_argument("--band", type=float, default=BAND, help="contact patch depth, grasp units")
    ap.add_argument("--min-opacity", type=float, default=MIN_WEIGHT, help="a Gaussian takes part above it")
    ap.add_argument("--max-collision", type=float, default=None, help="limit on the opacity inside the fingers")
    ap.add_argument("--out", required=True, help="output .npy: feasible rows, input frame, by score")
    ap.add_argument("--report", default=None, help="output .npz: every per-grasp output, scene frame")
    a = ap.parse_args(argv)
    check_object_options(ap, a, "optional")
    for name in ("mu", "band", "min_opacity"):
        v = getattr(a, name)
        if not (math.isfinite(v) and v >= 0.0):
            ap.error(f"--{name.replace('_', '-')} must be finite and >= 0, got {v}")
    if a.max_collision is not None and math.isnan(a.max_collision):
        ap.error("--max-collision must not be NaN")
    try:
        grasps = load_grasps(a.grasps)
        cam = _load_matrix(a.camera_pose, (4, 4), "camera pose") if a.camera_pose else None
        matrix, scale = load_transform_json(a.transform_json) if a.transform_json else (None, 1.0)
        from .interop import load_checkpoint
        scene, mlp_state, _ = load_checkpoint(a.ckpt)
        scene = scene.to(torch.device("cuda"))
        mask = object_mask(a, scene, mlp_state, matrix, scale)
        res = score_grasps(scene, grasps, mask, cam, matrix, scale, band=a.band, mu=a.mu, min_weight=a.min_opacity,
                           max_collision=a.max_collision)
    except (KeyError, ValueError, OSError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    keep = filter_grasps(grasps, res).cpu().numpy()
    np.save(a.out, grasps[keep])
    if a.report:
        np.savez(a.report, grasps_scene=grasps_to_scene(grasps, cam, matrix, scale),
                 **{k: getattr(res, k).cpu().numpy() for k in REPORT_KEYS})
    print(f"{len(keep)} of {len(grasps)} grasps feasible; wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
