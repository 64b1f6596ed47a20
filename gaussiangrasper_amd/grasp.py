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
    default_gripper    the whole gripper as boxes whose bounds are affine in a row's sizes (box_part, check_gripper,
                       scale_gripper, load_gripper: models of one's own)
    clearance          what such a gripper holds at the final pose and sweeps on its approach, per part
                       (gg_grasp_clearance, csrc/grasp_clear.hip, PARITY.md "Gripper clearance"; GraspClearance)
    nms                distinct grasps: greedy pose-distance suppression of the active rows, best score first
                       (gg_grasp_nms, csrc/grasp_nms.hip, PARITY.md "Grasp NMS"; GraspNMS)
    plane_clear        whether the whole gripper, at the final pose and at the start of its approach, stays above a
                       support plane (support.SupportPlane, PARITY.md "Support plane")
    GraspGates         the gates after the contacts (clearance, support plane, NMS) as one record, run by apply_gates
    python -m gaussiangrasper_amd.grasp --ckpt IN --grasps grasps.npy [...] --out kept.npy

Grasp candidates come from outside the project (AnyGrasp): this module only scores them."""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (ArrayLike, f32_rows, host_ptr, nonneg, positive, ptr as _ptr, require_hip as _require_hip,
                    stream as _stream, workspace as _ws)
from ._cli import (add_grasp_options, add_object_options, check_grasp_options, check_object_options,
                   grasp_gate_kwargs, load_scene, object_mask, report_arrays, support_option_plane)
from .frames import ORTHO_TOL, load_transform_json, rigid_to_scene  # noqa: F401

GRASP_COLS = 17
# UNVERIFIED defaults (PARITY.md "Grasp filtering"), in grasp units (metres): graspnetAPI's gripper drawing for
# depth_base and finger_width; band, mu and min_weight are this project's choices
DEPTH_BASE = 0.02
FINGER_WIDTH = 0.004
BAND = 0.003
MU = 0.5
MIN_WEIGHT = 0.0
MAX_PARTS = 8                # GG_CLEAR_MAX_PARTS
# UNVERIFIED defaults (PARITY.md "Grasp NMS"): graspnetAPI's GraspGroup.nms thresholds as recalled, 3 cm and 30 degrees
NMS_TRANSLATION = 0.03
NMS_ROTATION = math.pi / 6.0
NMS_MAX_CANDIDATES = 16384
NMS_MAX_ORDER = 65536        # GG_NMS_MAX_ORDER


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
    clearance: Optional["GraspClearance"] = None     # set by score_grasps / grasp_object when a gripper is given
    nms: Optional["GraspNMS"] = None                 # set by score_grasps / grasp_object with nms_translation
    support_clear: Optional[Tensor] = None           # (M,) bool, set by score_grasps / grasp_object with support
    support_lowest: Optional[Tensor] = None          # (M,) float64: the gripper's lowest height over the plane


@dataclass
class GraspClearance:
    """Per-grasp outputs of one gg_grasp_clearance call, device tensors; M = number of grasps, P = gripper parts."""
    body_count: Tensor         # (M, P) int32: points inside each part at the final pose
    body_weight: Tensor        # (M, P) float32: their weight
    sweep_count: Tensor        # (M, P) int32: points each part passes through over the approach
    sweep_weight: Tensor       # (M, P) float32
    valid: Tensor              # (M,) bool: the row is finite with width > 0 and height > 0
    clear: Tensor              # (M,) bool: valid and both totals within their limits


@dataclass
class GraspNMS:
    """Outputs of one gg_grasp_nms call, device tensors; M = number of grasps, K = number of kept rows."""
    keep: Tensor               # (M,) bool
    suppressor: Tensor         # (M,) int32: -1 kept, the kept row that suppressed it, -2 not active / not a pose
    order: Tensor              # (K,) int64: the kept rows, best first
    support: Tensor            # (M,) int32: for a kept row 1 + the rows it suppressed, 0 elsewhere.  Many active poses
                               # around a kept one: the grasp tolerates pose error (a ranking aid, not a filter)


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
# host side: the gripper model of gg_grasp_clearance (numpy, fp64)
# ------------------------------------------------------------------------------------------------
def check_gripper(parts: ArrayLike) -> np.ndarray:
    """`parts` as a contiguous float64 (P, 6, 4) array, after checking that P is in 1..MAX_PARTS and every coefficient
    finite.  parts[p][k] = (c0, cw, cd, ch) of bound k of (x_lo, x_hi, y_lo, y_hi, z_lo, z_hi), gripper frame:
    bound = c0 + cw width + cd depth + ch height of the grasp row."""
    g = np.ascontiguousarray(np.asarray(parts, dtype=np.float64))
    if g.ndim != 3 or g.shape[1:] != (6, 4) or not 1 <= g.shape[0] <= MAX_PARTS:
        raise ValueError(f"a gripper is (P, 6, 4) coefficients with P in 1..{MAX_PARTS}, got {g.shape}")
    if not np.isfinite(g).all():
        raise ValueError("gripper coefficients must be finite")
    return g


def box_part(x: Sequence[float], y: Sequence[float], z: Sequence[float]) -> np.ndarray:
    """(6, 4) coefficients of a box fixed in the gripper frame, whatever the row's sizes: x, y, z are (lo, hi) along
    the approach, closing and height axes, in the grasps' units.  A wrist, a camera housing."""
    bounds = [float(v) for lohi in (x, y, z) for v in lohi]
    if len(bounds) != 6 or not np.isfinite(bounds).all():
        raise ValueError("box_part takes three finite (lo, hi) pairs")
    part = np.zeros((6, 4))
    part[:, 0] = bounds
    return part


def scale_gripper(parts: ArrayLike, scale: float) -> np.ndarray:
    """The gripper with every constant term times `scale` (lengths in scene units); the size coefficients stay, as
    the rows' sizes are scaled themselves."""
    g = check_gripper(parts).copy()
    g[:, :, 0] *= float(scale)
    return g


def default_gripper(depth_base: float = DEPTH_BASE, finger_width: float = FINGER_WIDTH, tail_length: float = 0.04,
                    tail_width: Optional[float] = None, tail_height: Optional[float] = None,
                    scale: float = 1.0) -> np.ndarray:
    """(4, 6, 4) model of graspnetAPI's gripper drawing as recalled (UNVERIFIED, PARITY.md "Gripper clearance"), with
    w, h, depth the row's width, height and depth and fw = finger_width:
        left finger   x [-depth_base, depth]                   y [-w/2 - fw, -w/2]      z [-h/2, h/2]
        right finger  x [-depth_base, depth]                   y [w/2, w/2 + fw]        z [-h/2, h/2]
        palm          x [-depth_base - fw, -depth_base]        y [-w/2 - fw, w/2 + fw]  z [-h/2, h/2]
        tail          x [-depth_base - fw - tail_length, -depth_base - fw]
                      y [-tail_width/2, tail_width/2]          z [-tail_height/2, tail_height/2]
    tail_width and tail_height default to fw.  The parts are disjoint up to shared faces.  Lengths are in grasp
    units (metres) and multiplied by `scale`."""
    db, fw = nonneg("depth_base", depth_base), nonneg("finger_width", finger_width)
    tl = nonneg("tail_length", tail_length)
    tw = fw if tail_width is None else nonneg("tail_width", tail_width)
    th = fw if tail_height is None else nonneg("tail_height", tail_height)
    c0, cw, cd, ch = 0, 1, 2, 3
    g = np.zeros((4, 6, 4))
    for p, sign in ((0, -1.0), (1, 1.0)):                     # the fingers
        g[p, 0, c0], g[p, 1, cd] = -db, 1.0
        inner, outer = (3, 2) if sign < 0 else (2, 3)
        g[p, inner, cw] = g[p, outer, cw] = 0.5 * sign
        g[p, outer, c0] = fw * sign
    g[2, 0, c0], g[2, 1, c0] = -db - fw, -db                  # the palm
    g[2, 2, c0], g[2, 2, cw], g[2, 3, c0], g[2, 3, cw] = -fw, -0.5, fw, 0.5
    g[:3, 4, ch], g[:3, 5, ch] = -0.5, 0.5
    g[3, :, c0] = [-db - fw - tl, -db - fw, -0.5 * tw, 0.5 * tw, -0.5 * th, 0.5 * th]       # the tail
    return scale_gripper(g, positive("scale", scale))


def load_gripper(path: str) -> np.ndarray:
    """A gripper from a JSON file: a list of parts, each six rows (x_lo, x_hi, y_lo, y_hi, z_lo, z_hi) of four
    coefficients (c0, cw, cd, ch).  `json.dump(gripper.tolist(), f)` writes one."""
    with open(path) as f:
        try:
            parts = json.load(f)
        except json.JSONDecodeError as exc:
            raise ValueError(f"{path}: not JSON: {exc}") from exc
    try:
        return check_gripper(parts)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"{path}: {exc}") from exc


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


def limit(name: str, v: Optional[float]) -> float:
    v = math.inf if v is None else float(v)
    if math.isnan(v):
        raise ValueError(f"{name} must not be NaN")
    return v


def clearance(points: Tensor, weights: Tensor, grasps: Tensor, gripper: ArrayLike, approach: float = 0.0,
              min_weight: float = MIN_WEIGHT, max_body: Optional[float] = None,
              max_sweep: Optional[float] = None) -> GraspClearance:
    """What the whole gripper (`gripper`: (P, 6, 4) coefficients, check_gripper) of every grasp holds at its final pose
    (body) and passes through on the straight way there from `approach` back along -a (sweep), per part, as point
    counts and weights (include/gg_raster.h gg_grasp_clearance).  points (N, 3), weights (N,), grasps (M, 17): float32
    on the HIP device (no CPU path).  The gripper's constant terms and approach are in the grasps' units.  clear: the
    row is valid and the body / sweep weight over all parts is <= max_body / max_sweep (None: no limit).  One call;
    nothing waits on the host."""
    dev = _require_hip(points, weights, grasps)
    points = f32_rows(points, "points", 3)
    weights = f32_rows(weights, "weights", None)
    grasps = f32_rows(grasps, "grasps", GRASP_COLS)
    n, m = points.shape[0], grasps.shape[0]
    if weights.shape[0] != n:
        raise ValueError(f"points has {n} rows, weights {weights.shape[0]}")
    parts = check_gripper(gripper)
    p = parts.shape[0]
    if math.isnan(float(min_weight)):
        raise ValueError("min_weight must not be NaN")
    args = (nonneg("approach", approach), float(min_weight), limit("max_body", max_body),
            limit("max_sweep", max_sweep))
    lib = _lib.load()
    res = GraspClearance(
        body_count=torch.empty(m, p, dtype=torch.int32, device=dev),
        body_weight=torch.empty(m, p, dtype=torch.float32, device=dev),
        sweep_count=torch.empty(m, p, dtype=torch.int32, device=dev),
        sweep_weight=torch.empty(m, p, dtype=torch.float32, device=dev),
        valid=torch.empty(m, dtype=torch.uint8, device=dev),
        clear=torch.empty(m, dtype=torch.uint8, device=dev))
    nbytes = lib.gg_grasp_clearance_workspace(n, m, p)
    if m > 0 and nbytes == 0:
        raise ValueError(f"{n} points x {m} grasps is beyond gg_grasp_clearance's limits")
    ws = _ws(nbytes, dev)
    _lib.check(lib.gg_grasp_clearance(n, _ptr(points), _ptr(weights), m, _ptr(grasps), p, host_ptr(parts), *args,
                                      _ptr(res.body_count), _ptr(res.body_weight), _ptr(res.sweep_count),
                                      _ptr(res.sweep_weight), _ptr(res.valid), _ptr(res.clear), _ptr(ws), ws.numel(),
                                      _stream(dev)), "gg_grasp_clearance")
    res.valid, res.clear = res.valid.bool(), res.clear.bool()
    return res


def nms_order(grasps: Tensor, active: Optional[Tensor] = None,
              max_candidates: int = NMS_MAX_CANDIDATES) -> Tensor:
    """The int32 order grasp.nms walks: the active rows (None: all) whose score (fp32 column 0) is not NaN, by score
    descending, equal scores by ascending index (a stable sort), cut to the best max_candidates.  On the device of
    `grasps`."""
    m = grasps.shape[0]
    k = int(max_candidates)
    if k != max_candidates or not 1 <= k <= NMS_MAX_ORDER:
        raise ValueError(f"max_candidates must be an integer in 1..{NMS_MAX_ORDER}, got {max_candidates}")
    score = grasps[:, 0].float()
    take = ~torch.isnan(score)
    if active is not None:
        active = active.reshape(-1)
        if active.shape[0] != m:
            raise ValueError(f"active has {active.shape[0]} entries for {m} grasps")
        take = take & active.to(device=score.device, dtype=torch.bool)
    idx = torch.nonzero(take).reshape(-1)
    by_score = torch.sort(score[idx], descending=True, stable=True).indices
    return idx[by_score][:k].to(torch.int32)


def nms_support(keep: Tensor, suppressor: Tensor) -> Tensor:
    """(M,) int32: for a kept row 1 + how often it is named in `suppressor`, 0 for every other row."""
    m = keep.shape[0]
    named = torch.bincount(suppressor[suppressor >= 0].long(), minlength=m)[:m]
    return torch.where(keep, named + 1, torch.zeros_like(named)).to(torch.int32)


def nms(grasps: Tensor, active: Union[None, GraspContacts, Tensor] = None, translation: float = NMS_TRANSLATION,
        rotation: float = NMS_ROTATION, symmetric: bool = True, scale: float = 1.0,
        max_candidates: int = NMS_MAX_CANDIDATES) -> GraspNMS:
    """Distinct grasps of the active rows (include/gg_raster.h gg_grasp_nms): walking nms_order(grasps, active,
    max_candidates), a row is kept unless a kept row before it is near, i.e. within `translation` (grasp units, times
    `scale`) of it and turned by at most `rotation` radians against it, or, with `symmetric`, against its half turn
    about the approach axis (the same parallel-jaw pose with the fingers swapped).  Both limits are inclusive.
    grasps (M, 17) float32 on the HIP device (no CPU path); active: (M,) bool, or a GraspContacts, whose .feasible is
    used; None: every row.  The pair matrix takes max_candidates^2 / 8 bytes of workspace.  One call and one
    read-back (the number of kept rows)."""
    dev = _require_hip(grasps)
    grasps = f32_rows(grasps, "grasps", GRASP_COLS)
    m = grasps.shape[0]
    if isinstance(active, GraspContacts):
        active = active.feasible
    elif active is not None:
        active = torch.as_tensor(active)
    t = nonneg("translation", translation) * positive("scale", scale)
    rot = float(rotation)
    if not 0.0 <= rot <= math.pi:
        raise ValueError(f"rotation must be in [0, pi] radians, got {rotation}")
    order = nms_order(grasps, active, max_candidates)
    a = order.shape[0]
    lib = _lib.load()
    keep = torch.empty(m, dtype=torch.uint8, device=dev)
    suppressor = torch.empty(m, dtype=torch.int32, device=dev)
    kept = torch.empty(a, dtype=torch.int32, device=dev)
    num_kept = torch.zeros(1, dtype=torch.int32, device=dev)
    if m > 0:
        ws = _ws(lib.gg_grasp_nms_workspace(a), dev)
        _lib.check(lib.gg_grasp_nms(m, _ptr(grasps), a, _ptr(order), t, math.cos(rot), 1 if symmetric else 0,
                                    _ptr(keep), _ptr(suppressor), _ptr(kept), _ptr(num_kept), _ptr(ws), ws.numel(),
                                    _stream(dev)), "gg_grasp_nms")
    keep = keep.bool()
    return GraspNMS(keep=keep, suppressor=suppressor, order=kept[:int(num_kept.item())].long(),
                    support=nms_support(keep, suppressor))


def check_top_k(nms_translation: Optional[float], top_k: Optional[int]) -> Optional[int]:
    """top_k as an int >= 1 or None; it needs nms_translation."""
    if top_k is None:
        return None
    if nms_translation is None:
        raise ValueError("top_k needs nms_translation: without NMS the best rows are copies of one grasp")
    if int(top_k) != top_k or int(top_k) < 1:
        raise ValueError(f"top_k must be an integer >= 1, got {top_k}")
    return int(top_k)


def apply_nms(res: GraspContacts, rows: Tensor, translation: float, rotation: float, symmetric: bool,
              scale: float, top_k: Optional[int]) -> Tensor:
    """res.nms = nms(rows, res, ...) over the feasible rows (translation in grasp units, times scale); returns
    res.nms.order[:top_k]."""
    res.nms = nms(rows, res, translation, rotation, symmetric, scale)
    return res.nms.order[:top_k]


def apply_clearance(res: GraspContacts, scene_points: Tensor, scene_weights: Tensor, rows: Tensor, gripper: ArrayLike,
                    scale: float, approach: float, min_weight: float, max_body: Optional[float],
                    max_sweep: Optional[float]) -> GraspContacts:
    """`res` with the clearance of scene-frame `rows` against the whole scene's points: the gripper's constant terms
    and approach (grasp units) times `scale`; res.clearance set and res.feasible &= clear."""
    s = float(scale)
    res.clearance = clearance(scene_points, scene_weights, rows, scale_gripper(gripper, s),
                              nonneg("approach", approach) * s, min_weight, max_body, max_sweep)
    res.feasible = res.feasible & res.clearance.clear
    return res


def plane_clear(rows: Tensor, gripper: ArrayLike, plane, approach: float = 0.0, margin: float = 0.0,
                scale: float = 1.0):
    """(clear bool (M,), lowest float64 (M,)): whether the whole gripper of every row stays above a support plane.
    rows (M, 17) scene-frame GraspGroup rows on any device (plain torch fp64, CPU included); gripper: a check_gripper
    model; plane: anything with .normal (3,) and .offset (support.SupportPlane), n.x + offset the height of x; the
    gripper's constant terms, approach and margin are in grasp units and multiplied by `scale`.  Every part's bounds
    follow check_gripper's affine rule; a part with lo > hi on an axis or a bound that is not finite is empty.  lowest
    is the smallest height over the 8 corners of every part that is not empty, at the final pose t and at the approach
    start t - approach a (+inf for a row without such a part); a box between the two lies between them, so the whole
    approach stays above when both ends do.  clear = every entry of the row is finite and lowest >= margin."""
    if rows.ndim != 2 or rows.shape[1] != GRASP_COLS:
        raise ValueError(f"rows must be (M, {GRASP_COLS}) GraspGroup rows, got {tuple(rows.shape)}")
    s = positive("scale", scale)
    dev = rows.device
    parts = torch.from_numpy(scale_gripper(gripper, s)).to(dev)                  # (P, 6, 4) float64
    n = torch.as_tensor(np.asarray(plane.normal, dtype=np.float64).reshape(3)).to(dev)
    ap, mg = nonneg("approach", approach) * s, float(margin) * s
    if math.isnan(mg):
        raise ValueError("margin must not be NaN")
    g = rows.detach().double()
    width, height, depth = g[:, 1, None, None], g[:, 2, None, None], g[:, 3, None, None]
    c = parts[None]                                                               # (1, P, 6, 4)
    b = ((c[..., 0] + c[..., 1] * width) + c[..., 2] * depth) + c[..., 3] * height           # (M, P, 6)
    full = torch.isfinite(b).all(dim=2) & (b[..., 0] <= b[..., 1]) & (b[..., 2] <= b[..., 3]) & (b[..., 4] <= b[..., 5])
    R, t = g[:, 4:13].reshape(-1, 3, 3), g[:, 13:16]
    gn = (n[None, :, None] * R).sum(dim=1)                                        # (M, 3): n . (a, b, c)
    base = (t * n[None]).sum(dim=1) + float(plane.offset)                         # (M,): height of t
    lo, hi = b[..., 0::2], b[..., 1::2]                                           # (M, P, 3)
    low = torch.minimum(gn[:, None] * lo, gn[:, None] * hi).sum(dim=2)            # (M, P): the lowest corner over t
    low = torch.where(full, low, torch.full_like(low, math.inf)).min(dim=1).values
    lowest = torch.minimum(base + low, (base - ap * gn[:, 0]) + low)
    clear = torch.isfinite(g).all(dim=1) & (lowest >= mg)
    return clear, lowest


def apply_support(res: GraspContacts, rows: Tensor, gripper: Optional[ArrayLike], support, scale: float,
                  approach: float, margin: float, max_approach_tilt: Optional[float]) -> GraspContacts:
    """`res` with a support plane applied to scene-frame `rows`: res.support_clear / res.support_lowest =
    plane_clear(...) and res.feasible &= clear; with max_approach_tilt (radians), also res.feasible &= a.(-n) >=
    cos(max_approach_tilt), a the approach axis of the row (the gripper comes down onto the table, within that tilt of
    its normal).  support None: nothing is done, and the other two must be at their defaults."""
    if support is None:
        if max_approach_tilt is not None or margin != 0.0:
            raise ValueError("support_margin and max_approach_tilt need support: they are measured against the plane")
        return res
    if gripper is None:
        raise ValueError("support needs gripper: the plane test has to know which boxes must stay above the plane")
    res.support_clear, res.support_lowest = plane_clear(rows, gripper, support, approach, margin, scale)
    res.feasible = res.feasible & res.support_clear
    if max_approach_tilt is not None:
        tilt = float(max_approach_tilt)
        if not 0.0 <= tilt <= math.pi:
            raise ValueError(f"max_approach_tilt must be in [0, pi] radians, got {max_approach_tilt}")
        n = torch.as_tensor(np.asarray(support.normal, dtype=np.float64).reshape(3)).to(rows.device)
        a = rows.detach().double()[:, [4, 7, 10]]
        res.feasible = res.feasible & (-(a * n[None]).sum(dim=1) >= math.cos(tilt))
    return res


@dataclass
class GraspGates:
    """The gates score_grasps and grasp_propose.grasp_object put after the friction cone, by their keywords, in this
    order; each is off at its default and then makes no call.  Lengths are in grasp units, times the call's `scale`.
    Clearance, with a `gripper` (default_gripper(), or any check_gripper model): clearance of the whole gripper and of
    its straight approach of length `approach` against the WHOLE scene's points (model_points(model, None), whatever
    the mask is): feasible &= clear (body weight <= max_body, sweep weight <= max_sweep; None: no limit); the record
    is .clearance.  Support, with `support` (a support.SupportPlane of the scene frame; it needs `gripper`): feasible
    &= plane_clear(rows, gripper, support, approach, support_margin, scale) and, with max_approach_tilt (radians),
    feasible &= a.(-n) >= cos(max_approach_tilt); the plane test's outputs are .support_clear and .support_lowest.
    NMS, with `nms_translation`: nms of the feasible rows (near: within nms_translation and nms_rotation radians, with
    nms_symmetric also of the half turn about the approach axis); the record is .nms and the kept rows its
    order[:top_k], the distinct grasps best first, a subsequence of what filter_grasps gives.  Without nms_translation
    there is no NMS call and .nms is None; top_k then is an error."""
    gripper: Optional[ArrayLike] = None
    approach: float = 0.0
    max_body: Optional[float] = None
    max_sweep: Optional[float] = None
    nms_translation: Optional[float] = None
    nms_rotation: float = NMS_ROTATION
    nms_symmetric: bool = True
    top_k: Optional[int] = None
    support: object = None
    support_margin: float = 0.0
    max_approach_tilt: Optional[float] = None

    def check(self) -> "GraspGates":
        """The configuration errors that need no data, before anything runs; top_k becomes an int."""
        self.top_k = check_top_k(self.nms_translation, self.top_k)
        if self.support is not None and self.gripper is None:
            raise ValueError("support needs gripper: the plane test has to know which boxes must stay above the plane")
        return self


def apply_gates(g: GraspGates, res: GraspContacts, rows: Tensor, scale: float, min_weight: float,
                scene_points: Callable[[], Tuple[Tensor, Tensor]]) -> Tensor:
    """The gates of a checked `g` on `res` and its scene-frame `rows`; returns the kept rows: res.nms.order[:top_k] with
    NMS, else filter_grasps(rows, res).  scene_points(): whole-scene (points, weights), called only with a gripper."""
    if g.gripper is not None:
        apply_clearance(res, *scene_points(), rows, g.gripper, scale, g.approach, min_weight, g.max_body, g.max_sweep)
    apply_support(res, rows, g.gripper, g.support, scale, g.approach, g.support_margin, g.max_approach_tilt)
    if g.nms_translation is not None:
        return apply_nms(res, rows, g.nms_translation, g.nms_rotation, g.nms_symmetric, scale, g.top_k)
    return filter_grasps(rows, res)


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
                 max_collision: Optional[float] = None, gripper: Optional[ArrayLike] = None, approach: float = 0.0,
                 max_body: Optional[float] = None, max_sweep: Optional[float] = None,
                 nms_translation: Optional[float] = None, nms_rotation: float = NMS_ROTATION,
                 nms_symmetric: bool = True, top_k: Optional[int] = None, support=None,
                 support_margin: float = 0.0, max_approach_tilt: Optional[float] = None) -> GraspContacts:
    """Candidates in the grasp frame, scored against the model's Gaussians in one call: grasps_to_scene, then
    contacts on model_points.  depth_base, finger_width and band are in grasp units and scaled with the grasps.
    The keywords from `gripper` on are the gates of GraspGates (clearance, support plane, NMS; its docstring says
    what each does), run in that order after the contacts; with nms_translation .nms.order is cut to the best top_k."""
    gates = GraspGates(gripper, approach, max_body, max_sweep, nms_translation, nms_rotation, nms_symmetric, top_k,
                       support, support_margin, max_approach_tilt).check()
    pts, nrm, w = model_points(model_or_scene, mask)
    rows = torch.from_numpy(grasps_to_scene(grasps, cam_to_world, matrix, scale)).to(pts.device)
    s = float(scale)
    res = contacts(pts, nrm, w, rows, nonneg("depth_base", depth_base) * s, nonneg("finger_width", finger_width) * s,
                   nonneg("band", band) * s, mu, min_weight, max_collision)
    keep = apply_gates(gates, res, rows, s, min_weight,
                       lambda: (pts, w if mask is None else model_points(model_or_scene, None)[2]))
    if res.nms is not None:
        res.nms.order = keep
    return res


# ------------------------------------------------------------------------------------------------
# command line: filter a candidate file against a checkpoint
# ------------------------------------------------------------------------------------------------
def _load_matrix(path: str, shape, name: str) -> np.ndarray:
    a = np.asarray(np.load(path), dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{name} {path}: expected {shape}, got {a.shape}")
    return a


def load_gripper_option(text: Optional[str]) -> Optional[np.ndarray]:
    """--gripper: None without it, default_gripper() for "default", else load_gripper(FILE.json)."""
    if not text:
        return None
    return default_gripper() if text == "default" else load_gripper(text)


def nms_summary(feasible: int, total: int, res: GraspContacts, written: int, what: str) -> str:
    """The command lines' summary: how many rows are feasible and, with NMS, how many survive it."""
    line = f"{feasible} of {total} {what} feasible"
    if res.nms is not None:
        line += f", {int(res.nms.keep.sum())} distinct after NMS, {written} written"
    return line


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.grasp",
                                 description="Filter grasp candidates (GraspGroup rows) by the friction cone at both "
                                             "finger contacts on a checkpoint's Gaussians.")
    ap.add_argument("--ckpt", required=True, help="step-*.ckpt of a splatting model")
    ap.add_argument("--grasps", required=True, help=".npy (M, 17) GraspGroup rows, grasp frame")
    ap.add_argument("--camera-pose", default=None, help=".npy 4x4, grasp frame -> world")
    ap.add_argument("--transform-json", default=None, help="JSON with transform_matrix and scale (world -> scene)")
    add_object_options(ap, "the query restricts the Gaussians", "restricts the Gaussians")
    ap.add_argument("--band", type=float, default=BAND, help="contact patch depth, grasp units")
    add_grasp_options(ap)
    ap.add_argument("--out", required=True, help="output .npy: feasible rows, input frame, by score")
    ap.add_argument("--report", default=None, help="output .npz: every per-grasp output, scene frame")
    a = ap.parse_args(argv)
    check_object_options(ap, a, "optional")
    check_grasp_options(ap, a, ("band",))
    try:
        grasps = load_grasps(a.grasps)
        gripper = load_gripper_option(a.gripper)
        cam = _load_matrix(a.camera_pose, (4, 4), "camera pose") if a.camera_pose else None
        matrix, scale = load_transform_json(a.transform_json) if a.transform_json else (None, 1.0)
        scene, mlp_state = load_scene(a.ckpt)
        mask = object_mask(a, scene, mlp_state, matrix, scale)
        res = score_grasps(scene, grasps, mask, cam, matrix, scale, band=a.band, gripper=gripper,
                           **grasp_gate_kwargs(a, support_option_plane(a, scene, mask, scale)))
    except (KeyError, ValueError, OSError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    keep = (filter_grasps(grasps, res) if res.nms is None else res.nms.order).cpu().numpy()
    np.save(a.out, grasps[keep])
    if a.report:
        np.savez(a.report, grasps_scene=grasps_to_scene(grasps, cam, matrix, scale), **report_arrays(res))
    print(f"{nms_summary(int(res.feasible.sum()), len(grasps), res, len(keep), 'grasps')}; wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
