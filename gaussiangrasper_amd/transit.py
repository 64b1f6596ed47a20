"""Transit planning through the distance field: the exact cost-to-go over the free cells (`gg_field_route`), the
descent along it (`gg_field_descend`), the exact line of sight through the free cells (`gg_field_sight`) and greedy
string pulling of a descended path on top of it (`gg_field_shortcut`), csrc/field.hip, and the poses of a carried
gripper along the path that comes out.  The contract is in include/gg_raster.h and PARITY.md "Transit planning"; the
design, the convergence argument and the derivation of the planning pad in DESIGN.md §3.29, the line of sight and
why a pulled path is as safe as a descended one in §3.30.

    cells_of           the header's cell rule on the host in fp64
    route / descend_cells / sight / shortcut_cells   the four calls as they are
    cost_to_go         the cost field towards goal points, for a ball of `radius` kept `margin` away
    descend            the paths from start points down a cost field, called again when a path was cut
    line_of_sight      is the straight segment between the cells of two scene points clear for a ball of `radius`
    shortcut           a descended path pulled taut: the kept rows, and the kept cells padded as descend pads
    bounding_radius    the ball about the gripper's origin that holds the gripper at every orientation
    carried_spheres    spheres that cover the points of the carried object, gripper frame
    polyline_points / transit_poses    a cell path as `steps` poses, by arc length, the orientation by slerp
    plan_transit       cost field, descent, (shortcut,) poses, and field.path_clear with the real spheres as the verdict
    python -m gaussiangrasper_amd.transit --field field.npz --from POSES.npy --to POSE.npy --gripper default
                                          [--shortcut [--window W]] [...]

Out of scope: spline smoothing of the polyline (the pulled path still turns at its kept cells), orientation-aware
planning (the bounding ball is the price of a search in three dimensions), and the kinematics of the arm."""
from __future__ import annotations

import argparse
import ctypes as C
import math
import sys
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (ArrayLike, check_finite_options, host_array, positive, ptr as _ptr, require_hip as _require_hip,
                    sized_workspace, stream as _stream, to_device)
from .field import (FAR, MAX_POSES, MAX_SPHERES, DistanceField, PathClearance, cell_count, gripper_spheres,
                    interpolate, need2, path_clear, slerp_rotations, volume_args, volume_tensor)

MAX_GOALS = 1 << 24            # GG_FIELD_MAX_GOALS
MAX_ROUNDS = 4096
FIRST_CELLS = 256              # descend's first guess of the longest path, in cells
CELL_CLAMP = 2.0 ** 30         # field_cell.h FIELD_CELL_CLAMP
# DESIGN.md §3.29 "The planning pad": sqrt(3) h on the radius, and a hair for what float32 poses lose
PAD_CELLS = math.sqrt(3.0)
PAD_HAIR = 1e-6
# UNVERIFIED default (PARITY.md "Transit planning"): this project's choice, not checked on a real checkpoint
STEPS = 64


@dataclass
class CostToGo:
    cost: Tensor           # int32 [X][Y][Z]: chamfer 3-4-5 cost to the nearest goal, FAR where there is none
    need: int              # a cell is free iff dist2 >= need
    goals: np.ndarray      # (G, 3) int32 goal cells
    ignored: Tensor        # 0-dim int64: goals outside the volume or not free
    rounds: int            # rounds of relaxation the call took
    field: DistanceField   # whose dist2 the cost belongs to (stale after its next update())


@dataclass
class TransitPlan:
    poses: Tensor              # (P, steps, 12) float32 on the field's device
    clearance: PathClearance   # field.path_clear of `poses` with the real spheres: the verdict
    cost: np.ndarray           # (P,) float64 path length in scene units, chamfer 3-4-5 (cost h / 3); inf: no path
    best: int                  # the cheapest path that is planned and clear, -1 when there is none
    planned: np.ndarray        # (P,) bool: a path was found (the others hold the straight field.interpolate path)
    cells: Tensor              # (P, L, 3) int32 cell paths, `length` of each
    length: Tensor             # (P,) int32
    cost_to_go: CostToGo
    keep: Optional[Tensor] = None       # (P, L) int32 rows of `cells` the poses run through (shortcut=True only)
    count: Optional[Tensor] = None      # (P,) int32 how many of them (shortcut=True only)
    euclid: Optional[np.ndarray] = None     # (P,) float64 length of the polyline the poses follow: the start, the
    #                                         centres of the cells they run through, the goal; inf: no path


@dataclass
class Shortcut:
    keep: Tensor               # (P, L) int32 kept rows of the path, ascending; from `count` on the last one repeats
    count: Tensor              # (P,) int32 kept rows; 0 for a path of no cells (its keep rows are -1)
    blocked: Tensor            # (P,) int32 kept segments that are not clear: 0 for every path a descent produced
    cells: Tensor              # (P, L, 3) int32 the kept cells, padded as descend pads (-1 rows for no path)


# ------------------------------------------------------------------------------------------------
# host side
# ------------------------------------------------------------------------------------------------
def cells_of(field, points: ArrayLike) -> np.ndarray:
    """(N, 3) int32 cells of (N, 3) points by the header's rule in fp64: per axis the c with c h <= d < (c + 1) h,
    d = (double)p - lo (a division proposes and is clamped to +-2^30, the comparisons decide: field_cell.h step by
    step); a cell outside the volume is returned as it is.  A point that is not finite gives the row -1, -1, -1."""
    p = host_array(points, np.float64).reshape(-1, 3)
    grid = np.asarray(field.grid, np.float64)
    h = float(grid[3])
    fin = np.isfinite(p).all(1)
    d = np.where(fin[:, None], p, 0.0) - grid[:3]
    c = np.clip(np.floor(d / h), -CELL_CLAMP, CELL_CLAMP)
    c = np.where(c * h > d, c - 1.0, np.where((c + 1.0) * h <= d, c + 1.0, c))
    return np.where(fin[:, None], c, -1.0).astype(np.int32)


def cell_centres(field, cells: ArrayLike) -> np.ndarray:
    """lo + (c + 0.5) h, fp64"""
    grid = np.asarray(field.grid, np.float64)
    return grid[:3] + (np.asarray(cells, np.float64) + 0.5) * grid[3]


def bounding_radius(spheres: ArrayLike, radius: Union[float, ArrayLike]) -> float:
    """max_s |c_s| + r_s: the ball of that radius about the gripper's origin contains every sphere, and with them
    whatever they cover, at every orientation of the gripper."""
    c = np.asarray(spheres, np.float64).reshape(-1, 3)
    r = np.broadcast_to(np.asarray(radius, np.float64), (len(c),))
    if len(c) == 0 or not (np.isfinite(c).all() and np.isfinite(r).all() and (r >= 0).all()):
        raise ValueError("bounding_radius needs at least one sphere, finite centres and finite radii >= 0")
    return float((np.linalg.norm(c, axis=1) + r).max())


def carried_spheres(points_in_gripper_frame: ArrayLike, radius: float) -> np.ndarray:
    """(S, 3) float32 centres, gripper frame, whose balls of `radius` cover the points of the carried object: the
    centres of the occupied voxels of edge 2 radius / sqrt(3) (half diagonal = radius; the edge is taken 1e-4
    shorter, as field.gripper_spheres does, which is far more than the centres lose as float32).  Points that are
    not finite are left out.  ValueError beyond GG_FIELD_MAX_SPHERES."""
    p = host_array(points_in_gripper_frame, np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    edge = 2.0 * positive("radius", radius) / math.sqrt(3.0) * (1.0 - 1e-4)
    if len(p) == 0:
        return np.zeros((0, 3), np.float32)
    vox = np.unique(np.floor(p / edge).astype(np.int64), axis=0)
    if len(vox) > MAX_SPHERES:
        raise ValueError(f"{len(vox)} spheres of radius {radius} are more than {MAX_SPHERES}: use a larger radius")
    return ((vox + 0.5) * edge).astype(np.float32)


def planning_radius(spheres: ArrayLike, radius: Union[float, ArrayLike], h: float) -> float:
    """(bounding_radius + sqrt(3) h) (1 + 1e-6): a cell whose dist2 meets need2 of THIS radius holds only origins at
    which every sphere, at any orientation, meets its own need2 (DESIGN.md §3.29 "The planning pad")."""
    return (bounding_radius(spheres, radius) + PAD_CELLS * positive("h", h)) * (1.0 + PAD_HAIR)


def polyline_points(points: np.ndarray, steps: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(pts (steps, 3), seg (steps,), frac (steps,)): `steps` points at equal arc length along the polyline through
    the (K, 3) `points`, the first and last exactly its ends; seg[i] is the segment (points[seg], points[seg + 1])
    that holds pts[i], frac[i] its share of the whole length (i / (steps - 1) when the length is 0)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    steps = int(steps)
    if steps < 2 or len(p) < 2:
        raise ValueError(f"need steps >= 2 and at least two points, got {steps} and {len(p)}")
    seglen = np.linalg.norm(np.diff(p, axis=0), axis=1)
    total = float(seglen.sum())
    even = np.arange(steps) / (steps - 1.0)
    if total <= 0.0:
        return np.repeat(p[:1], steps, 0), np.zeros(steps, np.int64), even
    s = even * total
    keep = np.nonzero(seglen > 0.0)[0]                  # a point at a joint belongs to the segment that starts there,
    cum = np.concatenate([[0.0], np.cumsum(seglen[keep])])      # never to a segment of no length
    j = np.clip(np.searchsorted(cum, s, side="right") - 1, 0, len(keep) - 1)
    seg = keep[j]
    t = np.clip((s - cum[j]) / seglen[seg], 0.0, 1.0)
    pts = (1.0 - t)[:, None] * p[seg] + t[:, None] * p[seg + 1]
    pts[0], pts[-1] = p[0], p[-1]
    return pts, seg.astype(np.int64), s / total


def transit_poses(pose_from: ArrayLike, pose_to: ArrayLike, cells: ArrayLike, length: int, field,
                  steps: int = STEPS) -> np.ndarray:
    """(steps, 12) float32 poses along a cell path: the polyline from pose_from's position through the centres of the
    first `length` rows of `cells` to pose_to's position, resampled at equal arc length; the rotation by
    field.interpolate's slerp at the share of the arc passed.  The first and last pose are exactly the inputs."""
    a, b = (np.asarray(p, np.float64).reshape(-1) for p in (pose_from, pose_to))
    if a.shape != (12,) or b.shape != (12,) or not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise ValueError("a pose is 12 finite numbers: R row-major, then t")
    c = host_array(cells, np.int64).reshape(-1, 3)
    length = int(length)
    if not 1 <= length <= len(c):
        raise ValueError(f"length must be in 1..{len(c)} (the rows of cells), got {length}")
    line = np.concatenate([a[None, 9:], cell_centres(field, c[:length]), b[None, 9:]])
    pts, _, frac = polyline_points(line, steps)
    out = np.empty((len(pts), 12))
    out[:, :9] = slerp_rotations(a[:9], b[:9], frac)
    out[:, 9:] = pts
    out[0], out[-1] = a, b
    return out.astype(np.float32)


def polyline_lengths(field, starts: ArrayLike, goal: ArrayLike, cells: ArrayLike, length: ArrayLike) -> np.ndarray:
    """(P,) float64: the length, scene units, of the polyline from starts[p] through the centres of the first
    length[p] rows of cells[p] to `goal`, the line transit_poses resamples; inf where length[p] is 0."""
    s = np.asarray(starts, np.float64).reshape(-1, 3)
    g = np.asarray(goal, np.float64).reshape(1, 3)
    if len(s) == 0:
        return np.zeros(0)
    c = host_array(cells, np.int64).reshape(len(s), -1, 3)
    n = host_array(length, np.int64).reshape(-1)
    out = np.full(len(s), np.inf)
    for p in np.nonzero(n > 0)[0]:
        line = np.concatenate([s[p:p + 1], cell_centres(field, c[p, :n[p]]), g])
        out[p] = np.linalg.norm(np.diff(line, axis=0), axis=1).sum()
    return out


def best_path(planned: ArrayLike, clear: ArrayLike, rank: ArrayLike) -> int:
    """the planned and clear path of the smallest `rank` (the first of equals), -1 when there is none"""
    ok = np.asarray(planned, bool) & np.asarray(clear, bool)
    return int(np.argmin(np.where(ok, np.asarray(rank, np.float64), np.inf))) if ok.any() else -1


# ------------------------------------------------------------------------------------------------
# device side: the calls as they are
# ------------------------------------------------------------------------------------------------
def _cells_arg(cells: ArrayLike, name: str, dev) -> Tensor:
    t = to_device(cells, torch.int32, dev)
    if t.ndim != 2 or t.shape[1] != 3:
        if t.numel() == 0:
            return t.reshape(0, 3)
        raise ValueError(f"{name} must be (N, 3) cells, got {tuple(t.shape)}")
    return t


def route(dist2: Tensor, dims, need: int, goals: ArrayLike, max_rounds: int = MAX_ROUNDS,
          out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, int]:
    """(cost int32 [X][Y][Z], ignored 0-dim int64, rounds) of one gg_field_route call.  dist2 int32 [X][Y][Z] on the
    HIP device (no CPU path); goals (G, 3) int32 cells.  The call waits for the device (once per batch of rounds).
    GGError when max_rounds run out; `out`, when given, then holds upper bounds."""
    dev = _require_hip(dist2)
    d, _, shape = volume_args(dims)
    volume_tensor(dist2, "dist2", torch.int32, shape)
    need = cell_count("need", need)
    if int(max_rounds) < 1:
        raise ValueError(f"max_rounds must be >= 1, got {max_rounds}")
    g = _cells_arg(goals, "goals", dev)
    if g.shape[0] > MAX_GOALS:
        raise ValueError(f"{g.shape[0]} goals are more than {MAX_GOALS}")
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=dev)
    volume_tensor(out, "out", torch.int32, shape, dev)
    lib = _lib.load()
    ws = sized_workspace(lib.gg_field_route_workspace(d), f"{shape} cells are beyond gg_field_route's limits", dev)
    ignored = torch.zeros(1, dtype=torch.int64, device=dev)
    rounds = C.c_int(0)
    _lib.check(lib.gg_field_route(d, _ptr(dist2), need, g.shape[0], _ptr(g) if g.shape[0] else None, _ptr(out),
                                  _ptr(ignored), int(max_rounds), C.byref(rounds), _ptr(ws), ws.numel(), _stream(dev)),
               "gg_field_route")
    return out, ignored[0], int(rounds.value)


def descend_cells(dist2: Tensor, dims, need: int, cost: Tensor, starts: ArrayLike,
                  max_cells: int) -> Tuple[Tensor, Tensor]:
    """(cells (P, max_cells, 3) int32, length (P,) int32) of one gg_field_descend call; starts (P, 3) int32 cells."""
    dev = _require_hip(dist2, cost)
    d, _, shape = volume_args(dims)
    volume_tensor(dist2, "dist2", torch.int32, shape)
    volume_tensor(cost, "cost", torch.int32, shape)
    need = cell_count("need", need)
    s = _cells_arg(starts, "starts", dev)
    p, max_cells = s.shape[0], int(max_cells)
    if max_cells < 1 or p * max_cells > MAX_POSES:
        raise ValueError(f"need max_cells >= 1 and P max_cells <= {MAX_POSES}, got {p} x {max_cells}")
    cells = torch.empty(p, max_cells, 3, dtype=torch.int32, device=dev)
    length = torch.empty(p, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_field_descend(d, _ptr(dist2), need, _ptr(cost), p, _ptr(s) if p else None,
                                            max_cells, _ptr(cells), _ptr(length), _stream(dev)), "gg_field_descend")
    return cells, length


def sight(dist2: Tensor, dims, need: int, a: ArrayLike, b: ArrayLike) -> Tuple[Tensor, Tensor]:
    """(cover (S,) int32, blocked (S,) int32) of one gg_field_sight call; a, b (S, 3) int32 cells.  blocked 0: the
    segment between the two centres is clear; -1 (and cover 0): an end is outside the volume."""
    dev = _require_hip(dist2)
    d, _, shape = volume_args(dims)
    volume_tensor(dist2, "dist2", torch.int32, shape)
    need = cell_count("need", need)
    ca, cb = _cells_arg(a, "a", dev), _cells_arg(b, "b", dev)
    s = ca.shape[0]
    if cb.shape[0] != s or s > MAX_POSES:
        raise ValueError(f"a and b must hold the same number of cells, at most {MAX_POSES}: got {s} and {cb.shape[0]}")
    cover = torch.empty(s, dtype=torch.int32, device=dev)
    blocked = torch.empty(s, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_field_sight(d, _ptr(dist2), need, s, _ptr(ca) if s else None,
                                          _ptr(cb) if s else None, _ptr(cover), _ptr(blocked), _stream(dev)),
               "gg_field_sight")
    return cover, blocked


def line_of_sight(field: DistanceField, points_a: ArrayLike, points_b: ArrayLike, radius: float,
                  margin: float = 0.0) -> Tensor:
    """(S,) bool on the field's device: the straight segment between the CENTRES of the cells of points_a[s] and
    points_b[s] (scene points, (S, 3)) is clear for a ball of `radius` kept `margin` away: every cell its cover
    holds is inside the volume and has dist2 >= field.need2(radius, margin, h).  False for a point outside."""
    need = int(need2(float(radius), margin, field.h))
    _, blocked = sight(field.dist2, field.dims, need, cells_of(field, points_a), cells_of(field, points_b))
    return blocked == 0


def shortcut_cells(dist2: Tensor, dims, need: int, cells: Tensor, length: Tensor,
                   window: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(keep (P, max_cells) int32, count (P,) int32, blocked (P,) int32) of one gg_field_shortcut call; cells
    (P, max_cells, 3) int32 and length (P,) int32 as descend_cells returns them."""
    dev = _require_hip(dist2)
    d, _, shape = volume_args(dims)
    volume_tensor(dist2, "dist2", torch.int32, shape)
    need = cell_count("need", need)
    c = to_device(cells, torch.int32, dev)
    n = to_device(length, torch.int32, dev).reshape(-1)
    if c.ndim != 3 or c.shape[2] != 3 or c.shape[0] != n.shape[0]:
        raise ValueError(f"cells must be (P, max_cells, 3) and length (P,), got {tuple(c.shape)} and {tuple(n.shape)}")
    p, max_cells = c.shape[0], c.shape[1]
    if max_cells < 1 or p * max_cells > MAX_POSES:
        raise ValueError(f"need max_cells >= 1 and P max_cells <= {MAX_POSES}, got {p} x {max_cells}")
    if int(window) < 1:
        raise ValueError(f"window must be >= 1, got {window}")
    c = c.contiguous()
    keep = torch.empty(p, max_cells, dtype=torch.int32, device=dev)
    count = torch.empty(p, dtype=torch.int32, device=dev)
    blocked = torch.empty(p, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_field_shortcut(d, _ptr(dist2), need, p, max_cells, _ptr(c) if p else None,
                                             _ptr(n) if p else None, min(int(window), MAX_POSES), _ptr(keep),
                                             _ptr(count), _ptr(blocked), _stream(dev)), "gg_field_shortcut")
    return keep, count, blocked


def shortcut(ctg: CostToGo, cells: Tensor, length: Tensor, window: Optional[int] = None) -> Shortcut:
    """Greedy string pulling of the paths `descend` returned, against the free cells `ctg` was made for: from each
    kept cell the farthest cell within `window` rows (None: the whole path) whose segment is clear is kept next.
    Every point of the polyline through the kept centres then lies in a free cell of `ctg`."""
    f = ctg.field
    if window is None:
        window = max(int(cells.shape[1]), 1)
    keep, count, blocked = shortcut_cells(f.dist2, f.dims, ctg.need, cells, length, window)
    kept = torch.gather(to_device(cells, torch.int32, keep.device), 1,
                        keep.clamp(min=0).long()[:, :, None].expand(-1, -1, 3))
    return Shortcut(keep, count, blocked, torch.where(keep[:, :, None] >= 0, kept, torch.full_like(kept, -1)))


_shortcut = shortcut           # plan_transit's argument of the same name hides the function there


def cost_to_go(field: DistanceField, goal_points: ArrayLike, radius: float, margin: float = 0.0,
               max_rounds: int = MAX_ROUNDS) -> CostToGo:
    """The cost field of `field` (update() first) towards the cells of (G, 3) goal points, for a ball of `radius`
    kept `margin` away from every occupied cell: a cell is free iff dist2 >= field.need2(radius, margin, h)."""
    need = int(need2(float(radius), margin, field.h))
    goals = cells_of(field, goal_points)
    cost, ignored, rounds = route(field.dist2, field.dims, need, goals, max_rounds)
    return CostToGo(cost, need, goals, ignored, rounds, field)


def descend(ctg: CostToGo, start_points: ArrayLike, max_cells: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(cells (P, L, 3) int32, length (P,) int32, cost_at_start (P,) int32) from (P, 3) start points down `ctg`.
    L is max_cells (FIRST_CELLS when None), or the longest path when that is longer: the call is then made again
    with that much room, so no path comes back cut.  cost_at_start is FAR for a start outside the volume."""
    f = ctg.field
    starts = cells_of(f, start_points)
    dev = ctg.cost.device
    room = FIRST_CELLS if max_cells is None else int(max_cells)
    cells, length = descend_cells(f.dist2, f.dims, ctg.need, ctg.cost, starts, room)
    longest = int(length.max()) if len(starts) else 0
    if longest > room:
        cells, length = descend_cells(f.dist2, f.dims, ctg.need, ctg.cost, starts, longest)
    dims = np.asarray(f.dims, np.int64)
    inside = ((starts >= 0) & (starts < dims)).all(1)
    flat = (np.clip(starts, 0, dims - 1).astype(np.int64) * [dims[1] * dims[2], dims[2], 1]).sum(1)
    at = ctg.cost.reshape(-1)[torch.from_numpy(flat).to(dev)]
    at = torch.where(torch.from_numpy(inside).to(dev), at, torch.full_like(at, FAR))
    return cells, length, at


def plan_transit(field: DistanceField, poses_from: ArrayLike, pose_to: ArrayLike, spheres: ArrayLike,
                 radius: Union[float, ArrayLike], margin: float = 0.0, steps: int = STEPS,
                 max_rounds: int = MAX_ROUNDS, shortcut: bool = False, window: Optional[int] = None) -> TransitPlan:
    """Paths for the gripper (and what it carries: `spheres` (S, 3) of `radius`, gripper frame) from each of the
    (P, 12) poses_from to pose_to through field (update() first): ONE cost field from pose_to's cell for the ball
    of planning_radius, one descent for all P starts, transit_poses for each, and field.path_clear of those poses with
    the real spheres as the verdict.  A start from which there is no path gets the straight field.interpolate poses,
    planned False and cost inf.

    shortcut=True pulls every path taut first (`shortcut`, within `window` rows; None: the whole path): the poses
    then run through the kept cells only, `keep` and `count` say which, and `best` is the planned and clear path of
    the smallest `euclid` rather than of the smallest chamfer `cost` (which keeps its meaning).  `euclid` is filled
    either way."""
    a, b = host_array(poses_from, np.float64).reshape(-1, 12), host_array(pose_to, np.float64).reshape(-1)
    if b.shape != (12,) or not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise ValueError("poses_from is (P, 12) and pose_to (12,) finite numbers: R row-major, then t")
    sp = host_array(spheres, np.float32).reshape(-1, 3)
    ctg = cost_to_go(field, b[None, 9:], planning_radius(sp, radius, field.h), margin, max_rounds)
    cells, length, at = descend(ctg, a[:, 9:])
    n, c, at = length.cpu().numpy(), cells.cpu().numpy(), at.cpu().numpy()
    planned = n > 0
    keep = count = None
    if shortcut:
        if window is not None and int(window) < 1:
            raise ValueError(f"window must be >= 1, got {window}")
        pulled = _shortcut(ctg, cells, length, window)
        keep, count = pulled.keep, pulled.count
        n, c = count.cpu().numpy(), pulled.cells.cpu().numpy()
    poses = np.stack([transit_poses(a[i], b, c[i], n[i], field, steps) if planned[i] else interpolate(a[i], b, steps)
                      for i in range(len(a))]) if len(a) else np.zeros((0, int(steps), 12), np.float32)
    clearance = path_clear(field, poses, sp, radius, margin)
    cost = np.where(planned, at.astype(np.float64) * field.h / 3.0, np.inf)
    euclid = polyline_lengths(field, a[:, 9:], b[9:], c, n)
    best = best_path(planned, clearance.clear.cpu().numpy(), euclid if shortcut else cost)
    return TransitPlan(to_device(poses, torch.float32, field.dist2.device), clearance, cost, best, planned, cells,
                       length, ctg, keep, count, euclid)


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def main(argv: Optional[Sequence[str]] = None) -> int:
    from ._cli import add_gripper_sphere_options
    from .grasp import load_gripper_option
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.transit",
                                 description="Collision-free transit of the gripper through a saved distance field: "
                                             "from each start pose to one goal pose.")
    ap.add_argument("--field", required=True, help=".npz of python -m gaussiangrasper_amd.field (--out)")
    ap.add_argument("--from", dest="start", required=True, help=".npy (P, 12) or (12,) start poses: R row-major, then t")
    ap.add_argument("--to", required=True, help=".npy (12,) goal pose")
    add_gripper_sphere_options(ap)
    ap.add_argument("--steps", type=int, default=STEPS, help="waypoints per path")
    ap.add_argument("--carried", default=None, help=".npy (N, 3) points of the carried object, gripper frame")
    ap.add_argument("--shortcut", action="store_true", help="pull the paths taut: poses through the kept cells only")
    ap.add_argument("--window", type=int, default=None, help="with --shortcut: rows looked ahead (default: the path)")
    ap.add_argument("--out", required=True, help="output .npy (P, steps, 12) poses")
    ap.add_argument("--report", required=True, help="output .npz slack, first_hit, clear, cost, euclid, best, planned, "
                                                    "spheres; with --shortcut keep and count too")
    a = ap.parse_args(argv)
    if a.window is not None and not a.shortcut:
        ap.error("--window needs --shortcut")
    if a.window is not None and a.window < 1:
        ap.error(f"--window must be >= 1, got {a.window}")
    check_finite_options(ap, a, positive=("radius", "width"), nonneg=("margin", "depth", "height"))
    if a.steps < 2:
        ap.error(f"--steps must be >= 2, got {a.steps}")
    try:
        spheres = gripper_spheres(load_gripper_option(a.gripper), a.width, a.depth, a.height, a.radius)
        if a.carried:
            spheres = np.concatenate([spheres, carried_spheres(np.load(a.carried), a.radius)])
            if len(spheres) > MAX_SPHERES:
                raise ValueError(f"{len(spheres)} spheres with the carried object are more than {MAX_SPHERES}: "
                                 "use a larger --radius")
        start = np.asarray(np.load(a.start), np.float64)
        goal = np.asarray(np.load(a.to), np.float64).reshape(-1)
        if start.ndim not in (1, 2) or start.shape[-1] != 12 or goal.shape != (12,):
            raise ValueError(f"expected (P, 12) start poses and a (12,) goal pose, got {start.shape} and {goal.shape}")
        field = DistanceField.load(a.field)
        plan = plan_transit(field, start.reshape(-1, 12), goal, spheres, a.radius, a.margin, a.steps,
                            shortcut=a.shortcut, window=a.window)
        np.save(a.out, plan.poses.cpu().numpy())
        clear = plan.clearance.clear.cpu().numpy()
        pulled = {"keep": plan.keep.cpu().numpy(), "count": plan.count.cpu().numpy()} if a.shortcut else {}
        np.savez(a.report, slack=plan.clearance.slack.cpu().numpy(), first_hit=plan.clearance.first_hit.cpu().numpy(),
                 clear=clear, cost=plan.cost, best=np.int64(plan.best), planned=plan.planned, spheres=spheres,
                 length=plan.length.cpu().numpy(), rounds=np.int64(plan.cost_to_go.rounds), euclid=plan.euclid,
                 **pulled)
    except (KeyError, ValueError, OSError, _lib.GGError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    print(f"{int(plan.planned.sum())} of {len(plan.planned)} starts have a path, {int((plan.planned & clear).sum())} "
          f"clear; best {plan.best}"
          + (f" at {plan.cost[plan.best]:.4f} scene units" if plan.best >= 0 else "")
          + (f" ({plan.euclid[plan.best]:.4f} along {int(plan.count[plan.best])} kept cells)"
             if a.shortcut and plan.best >= 0 else "")
          + f"; {plan.cost_to_go.rounds} rounds; wrote {a.out} and {a.report}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
