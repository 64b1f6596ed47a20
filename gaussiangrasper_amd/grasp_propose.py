"""Grasp proposals: antipodal parallel-jaw candidates from the Gaussian field itself, as GraspGroup rows in the
layout `grasp.contacts` reads, so that propose -> score -> filter runs on the device with nothing from outside the
project.  One HIP call (`gg_grasp_propose`, csrc/grasp_propose.hip) tests every seed against every oriented point of
the object in fp64; the contract is in include/gg_raster.h and PARITY.md "Grasp proposals".  This is a geometric
sampler of this project's own, not a restatement of AnyGrasp: its candidates are a different set.

    antipodal          the per-seed outputs of one gg_grasp_propose call (GraspProposals)
    choose_seeds       the points that take part, thinned to at most max_seeds
    propose_grasps     (M, 17) scene-frame rows of a model's object (model_points, choose_seeds, antipodal, compact)
    grasp_object       proposals, then grasp.contacts and grasp.filter_grasps: (rows, GraspContacts, keep)
    grasps_from_scene  scene frame -> world -> grasp frame (grasp.grasps_from_scene, handed on)
    python -m gaussiangrasper_amd.grasp_propose --ckpt IN (--object-points obj.npy | --positives ...) --out grasps.npy
"""
from __future__ import annotations

import argparse
import ctypes
import math
import sys
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (f32_rows, host_ptr, nonneg, positive, ptr as _ptr, require_hip as _require_hip,
                    stream as _stream, workspace as _ws)
from ._cli import (add_grasp_options, add_object_options, check_grasp_options, check_object_options,
                   grasp_gate_kwargs, load_scene, object_mask, report_arrays, support_option_plane)
from .frames import check_rotation, load_transform_json
from .grasp import (BAND, DEPTH_BASE, FINGER_WIDTH, GRASP_COLS, MIN_WEIGHT, MU, NMS_ROTATION, GraspContacts,
                    GraspGates, apply_gates, contacts, grasps_from_scene, limit, load_gripper_option,
                    model_points, nms_summary)

# UNVERIFIED defaults (PARITY.md "Grasp proposals"), in grasp units (metres): max_width, depth and height are
# recalled from graspnetAPI's gripper; tube_radius, min_width, clearance, min_align and num_approach are this
# project's choices
TUBE_RADIUS = 0.003
MAX_WIDTH = 0.10
MIN_WIDTH = 0.005
CLEARANCE = 0.005
DEPTH = 0.02
HEIGHT = 0.02
MIN_ALIGN = 0.0
NUM_APPROACH = 8
MAX_SEEDS = 4096
MAX_APPROACH = 64            # GG_PROPOSE_MAX_APPROACH
UP = (0.0, 0.0, 1.0)


@dataclass
class GraspProposals:
    """Per-seed outputs of one gg_grasp_propose call, device tensors; S = number of seeds, K = num_approach."""
    pair_idx: Tensor           # (S, 2) int32: the two contact points, -1 when the seed is not usable
    tube_count: Tensor         # (S,) int32: points in the seed's tube, 0 when not usable
    span: Tensor               # (S,) float32: distance between the contacts, NaN when not usable
    valid: Tensor              # (S,) bool
    rows: Tensor               # (S, K, 17) float32 GraspGroup rows, NaN for a seed that is not valid

    def compact(self) -> Tensor:
        """(M, 17) rows of the valid seeds, in seed order, then approach order."""
        return self.rows[self.valid].reshape(-1, GRASP_COLS)


# ------------------------------------------------------------------------------------------------
# device side: one gg_grasp_propose call
# ------------------------------------------------------------------------------------------------
def _check_params(tube_radius, max_width, min_width, clearance, depth, height, min_weight, min_align, up,
                  num_approach) -> Tuple[tuple, tuple, int]:
    r, w0 = nonneg("tube_radius", tube_radius), nonneg("min_width", min_width)
    c, d = nonneg("clearance", clearance), nonneg("depth", depth)
    W, h = positive("max_width", max_width), positive("height", height)
    if 2.0 * c > W:
        raise ValueError(f"clearance {c} on both sides exceeds max_width {W}")
    mw, ma = float(min_weight), float(min_align)
    if math.isnan(mw):
        raise ValueError("min_weight must not be NaN")
    if not 0.0 <= ma <= 1.0:
        raise ValueError(f"min_align must be in [0, 1], got {ma}")
    u = tuple(float(x) for x in np.asarray(up, dtype=np.float64).reshape(-1))
    if len(u) != 3 or not all(math.isfinite(x) for x in u) or not any(x != 0.0 for x in u):
        raise ValueError(f"up must be 3 finite numbers, not all zero, got {up}")
    k = int(num_approach)
    if k != num_approach or not 1 <= k <= MAX_APPROACH:
        raise ValueError(f"num_approach must be an integer in 1..{MAX_APPROACH}, got {num_approach}")
    return (r, W, w0, c, d, h, mw, ma), u, k


def antipodal(points: Tensor, normals: Tensor, weights: Tensor, seeds: Tensor, tube_radius: float = TUBE_RADIUS,
              max_width: float = MAX_WIDTH, min_width: float = MIN_WIDTH, clearance: float = CLEARANCE,
              depth: float = DEPTH, height: float = HEIGHT, min_weight: float = MIN_WEIGHT,
              min_align: float = MIN_ALIGN, up: Sequence[float] = UP,
              num_approach: int = NUM_APPROACH) -> GraspProposals:
    """Antipodal candidates of every seed against the oriented points (include/gg_raster.h gg_grasp_propose).
    points / normals (N, 3), weights (N,) float32 and seeds (S,) int32 on the HIP device (no CPU path).  Per seed:
    the farthest two points within tube_radius of the seed's normal line and max_width along it are the contacts;
    the seed is valid when they are min_width .. max_width - 2 clearance apart and both contact normals are within
    acos(min_align) of the line, and then gives num_approach rows around the closing axis, the first one
    approaching from as near -up as the axis allows.  Lengths are in the points' units.  One call; nothing waits on
    the host."""
    args, u, k = _check_params(tube_radius, max_width, min_width, clearance, depth, height, min_weight, min_align,
                               up, num_approach)
    dev = _require_hip(points, normals, weights, seeds)
    points = f32_rows(points, "points", 3)
    normals = f32_rows(normals, "normals", 3)
    weights = f32_rows(weights, "weights", None)
    if seeds.dtype != torch.int32 or seeds.ndim != 1:
        raise ValueError(f"seeds must be an int32 (S,) tensor, got {seeds.dtype} {tuple(seeds.shape)}")
    seeds = seeds.contiguous()
    n, s = points.shape[0], seeds.shape[0]
    if normals.shape[0] != n or weights.shape[0] != n:
        raise ValueError(f"points has {n} rows, normals {normals.shape[0]}, weights {weights.shape[0]}")
    lib = _lib.load()
    res = GraspProposals(
        pair_idx=torch.empty(s, 2, dtype=torch.int32, device=dev),
        tube_count=torch.empty(s, dtype=torch.int32, device=dev),
        span=torch.empty(s, dtype=torch.float32, device=dev),
        valid=torch.empty(s, dtype=torch.uint8, device=dev),
        rows=torch.empty(s, k, GRASP_COLS, dtype=torch.float32, device=dev))
    nbytes = lib.gg_grasp_propose_workspace(n, s)
    if s > 0 and nbytes == 0:
        raise ValueError(f"{n} points x {s} seeds is beyond gg_grasp_propose's limits")
    ws = _ws(nbytes, dev)
    up3 = (ctypes.c_double * 3)(*u)
    _lib.check(lib.gg_grasp_propose(n, _ptr(points), _ptr(normals), _ptr(weights), s, _ptr(seeds), *args,
                                    host_ptr(up3), k, _ptr(res.pair_idx), _ptr(res.tube_count),
                                    _ptr(res.span), _ptr(res.valid), _ptr(res.rows), _ptr(ws),
                                    ws.numel(), _stream(dev)), "gg_grasp_propose")
    res.valid = res.valid.bool()
    return res


def choose_seeds(weights: Tensor, max_seeds: int = MAX_SEEDS, seed: int = 0, min_weight: float = MIN_WEIGHT) -> Tensor:
    """int32 indices of the points with (double)w > min_weight, ascending, thinned to at most max_seeds.  With P such
    points, P <= max_seeds keeps all of them; otherwise prepare's gg_subsample picks the subset (its interface fits
    unchanged: subsample_device_indices(P, keep, seed) with keep = ceil(P / max_seeds) gives P // keep positions, a
    uniform subset by SplitMix64 keys of (seed, position), in ascending order), so between max_seeds / 2 and
    max_seeds seeds come back.  Points and normals are not looked at: a seed whose point or normal is not finite is
    simply not usable.  One read-back (P)."""
    dev = _require_hip(weights)
    if weights.ndim != 1:
        raise ValueError(f"weights must be (N,), got {tuple(weights.shape)}")
    m = int(max_seeds)
    if m != max_seeds or m < 1:
        raise ValueError(f"max_seeds must be an integer >= 1, got {max_seeds}")
    if math.isnan(float(min_weight)):
        raise ValueError("min_weight must not be NaN")
    idx = torch.nonzero(weights.double() > float(min_weight)).reshape(-1)
    p = idx.shape[0]
    if p > m:
        from .prepare import subsample_device_indices
        idx = idx[subsample_device_indices(p, -(-p // m), int(seed)).to(dev)]
    return idx.to(torch.int32)


def propose_grasps(model_or_scene, mask: Optional[Tensor] = None, max_seeds: int = MAX_SEEDS,
                   num_approach: int = NUM_APPROACH, up: Sequence[float] = UP, scale: float = 1.0,
                   tube_radius: float = TUBE_RADIUS, max_width: float = MAX_WIDTH, min_width: float = MIN_WIDTH,
                   clearance: float = CLEARANCE, depth: float = DEPTH, height: float = HEIGHT,
                   min_weight: float = MIN_WEIGHT, min_align: float = MIN_ALIGN, seed: int = 0) -> Tensor:
    """(M, 17) float32 candidates for the object `mask` selects (None: every Gaussian), on the device, in the SCENE
    frame: grasp.model_points(model, mask), choose_seeds, antipodal, then the valid seeds' rows in seed order, then
    approach order.  Lengths are given in grasp units (metres) and multiplied by `scale` (the scene's units per
    metre), as score_grasps does; `up` is a direction of the scene frame."""
    s = positive("scale", scale)
    pts, nrm, w = model_points(model_or_scene, mask)
    seeds = choose_seeds(w, max_seeds, seed, min_weight)
    res = antipodal(pts, nrm, w, seeds, nonneg("tube_radius", tube_radius) * s, float(max_width) * s,
                    nonneg("min_width", min_width) * s, nonneg("clearance", clearance) * s,
                    nonneg("depth", depth) * s, float(height) * s, min_weight, min_align, up, num_approach)
    return res.compact()


def grasp_object(model_or_scene, mask: Optional[Tensor] = None, scale: float = 1.0,
                 depth_base: float = DEPTH_BASE, finger_width: float = FINGER_WIDTH, band: float = BAND,
                 mu: float = MU, min_weight: float = MIN_WEIGHT, max_collision: Optional[float] = None,
                 gripper=None, approach: float = 0.0, max_body: Optional[float] = None,
                 max_sweep: Optional[float] = None, nms_translation: Optional[float] = None,
                 nms_rotation: float = NMS_ROTATION, nms_symmetric: bool = True, top_k: Optional[int] = None,
                 support=None, support_margin: float = 0.0, max_approach_tilt: Optional[float] = None,
                 **propose) -> Tuple[Tensor, GraspContacts, Tensor]:
    """From a model and an object mask to feasible grasps: (rows, contacts, keep), all on the device.  rows (M, 17):
    propose_grasps(model, mask, scale=scale, **propose), scene frame.  contacts: grasp.contacts of those rows, in two
    calls, because gg_grasp_contacts takes one point set for the contacts and the collision term alike while the two
    want different ones: the finger contacts, patch normals, angles and region sums come from the OBJECT's points
    (weights times mask: the fingers close on the object, not on the table under it), and collision_weight from the
    WHOLE scene's points (model_points(model, None): what the fingers must not hit is everything, the object's own
    Gaussians beside the contacts included).  feasible = the object call's friction-cone result and the scene
    call's collision_weight <= max_collision (None: no limit).  keep: filter_grasps(rows, contacts), indices of the
    feasible rows by score.  The keywords from `gripper` on are the gates of grasp.GraspGates (clearance, support
    plane, NMS; its docstring says what each does), run in that order after the contacts: their records are
    contacts.clearance, .support_clear / .support_lowest and .nms, and with NMS keep is its order[:top_k]."""
    gates = GraspGates(gripper, approach, max_body, max_sweep, nms_translation, nms_rotation, nms_symmetric, top_k,
                       support, support_margin, max_approach_tilt).check()
    rows = propose_grasps(model_or_scene, mask, scale=scale, min_weight=min_weight, **propose)
    s = float(scale)
    lengths = (nonneg("depth_base", depth_base) * s, nonneg("finger_width", finger_width) * s,
               nonneg("band", band) * s)
    mc = limit("max_collision", max_collision)
    obj = model_points(model_or_scene, mask)
    whole = obj if mask is None else model_points(model_or_scene, None)
    res = contacts(*obj, rows, *lengths, mu, min_weight, None)
    if mask is not None:
        res.collision_weight = contacts(*whole, rows, *lengths, mu, min_weight, None).collision_weight
    res.feasible = res.feasible & (res.collision_weight.double() <= mc)
    return rows, res, apply_gates(gates, res, rows, s, min_weight, lambda: (whole[0], whole[2]))


# ------------------------------------------------------------------------------------------------
# command line: from a checkpoint and an object selection to feasible grasps
# ------------------------------------------------------------------------------------------------
def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.grasp_propose",
                                 description="Propose parallel-jaw grasps on an object of a checkpoint's Gaussians "
                                             "and keep those inside the friction cone at both contacts.")
    ap.add_argument("--ckpt", required=True, help="step-*.ckpt of a splatting model")
    ap.add_argument("--transform-json", default=None, help="JSON with transform_matrix and scale (world -> scene)")
    add_object_options(ap, "the query selects the Gaussians", "selects the object's Gaussians")
    ap.add_argument("--max-seeds", type=int, default=MAX_SEEDS, help="seed points at most")
    ap.add_argument("--num-approach", type=int, default=NUM_APPROACH, help="approach directions per seed")
    ap.add_argument("--up", type=float, nargs=3, default=list(UP), metavar=("X", "Y", "Z"),
                    help="up direction, world frame; with --support-plane it only orients the fitted plane, whose "
                         "normal then is the proposer's up")
    ap.add_argument("--max-width", type=float, default=MAX_WIDTH, help="gripper opening, grasp units")
    add_grasp_options(ap)
    ap.add_argument("--out", required=True, help="output .npy: feasible rows by score, world frame (scene frame "
                                                 "without --transform-json: the two are the same then)")
    ap.add_argument("--report", default=None, help="output .npz: every candidate (scene frame) and its outputs")
    a = ap.parse_args(argv)
    check_object_options(ap, a, "required")
    check_grasp_options(ap, a)
    if a.max_seeds < 1:
        ap.error(f"--max-seeds must be >= 1, got {a.max_seeds}")
    try:
        _check_params(TUBE_RADIUS, a.max_width, MIN_WIDTH, CLEARANCE, DEPTH, HEIGHT, a.min_opacity, MIN_ALIGN, a.up,
                      a.num_approach)
    except ValueError as exc:
        ap.error(str(exc))
    try:
        gripper = load_gripper_option(a.gripper)
        matrix, scale = None, 1.0
        if a.transform_json:
            matrix, scale = load_transform_json(a.transform_json)
            if matrix.shape not in ((3, 4), (4, 4)):
                raise ValueError(f"transform_matrix must be 3x4 or 4x4, got {matrix.shape}")
            check_rotation(matrix[:3, :3], "matrix rotation")
        up = np.asarray(a.up, dtype=np.float64) if matrix is None else matrix[:3, :3] @ np.asarray(a.up)
        scene, mlp_state = load_scene(a.ckpt)
        a.support_up = up
        mask = object_mask(a, scene, mlp_state, matrix, scale)
        plane = support_option_plane(a, scene, mask, scale, up)
        if plane is not None:
            up = plane.normal                # the table's own normal, not the command line's guess
        rows, res, keep = grasp_object(scene, mask, scale=scale, gripper=gripper, max_seeds=a.max_seeds,
                                       num_approach=a.num_approach, up=up, max_width=a.max_width,
                                       **grasp_gate_kwargs(a, plane))
    except (KeyError, ValueError, OSError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    rows_np = rows.cpu().numpy()
    kept = rows_np[keep.cpu().numpy()]
    np.save(a.out, grasps_from_scene(kept, None, matrix, scale))
    if a.report:
        np.savez(a.report, grasps_scene=rows_np, **report_arrays(res))
    print(f"{nms_summary(int(res.feasible.sum()), len(rows_np), res, len(kept), 'proposed grasps')}; wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
