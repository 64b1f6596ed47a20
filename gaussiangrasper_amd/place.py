"""Where to put an object down: the poses at which it rests on the support plane, or on whatever stands on it, without
entering anything.  The scene and the object become integer height maps over the plane's grid (`gg_height_map`) and
every (yaw, x, y) is searched exactly, a max-plus correlation of the two maps (`gg_place_search`), csrc/place.hip.
The contract is in include/gg_raster.h and PARITY.md "Placement"; the design in DESIGN.md §3.28.

    plane_frame          the plane's frame: origin under a centre, two in-plane axes by a fixed rule, the normal
    plane_grid           (grid, dims) of a box in that frame's in-plane coordinates
    yaw_frames           the object's frames, one per yaw, the pivot on the corner between cells (A/2, B/2)
    height_map           one gg_height_map call: (map, dropped)
    top_map / scene_top  the top map of points / of a model with the object left out, empty cells at the plane's level
    under_maps / object_under   the underside maps of points / of a model's object, one per yaw, grown by `dilate` cells
    object_pivot         the object's weighted centroid and its in-plane radius
    search               one gg_place_search call: PlaceSearch(rest, contact, support)
    placement_transform  the (3, 4) rigid transform of a (yaw, anchor, rest)
    propose              the anchors that pass the gates, ordered: Placements
    place_points / place_object   plane -> maps -> search -> propose, on points / on a model and an object mask
    release_paths        the gripper's descent onto every placement, as field.path_clear takes it
    python -m gaussiangrasper_amd.place --ckpt IN [selection] --out placements.npz [...]

Every decision is made on the integer outputs.  The transforms go to ops.RigidMove / edit as they are ([R | t]).

Limits.  The points are the Gaussians' MEANS: their extents are not rasterised, `dilate` and the opacity threshold are
the only allowance.  The contact box is a proxy for the support polygon, not a stability proof.

CELL 5 mm, LEVEL 1 mm, YAWS 16 over [0, pi), TOL 2 levels, MIN_CONTACT 0.1, STABILITY_MARGIN 1 cell, DILATE 1 cell,
MAX_STEP 5 levels and REGION 0.3 m are this project's choices, UNVERIFIED on a real checkpoint (PARITY.md
"Placement")."""
from __future__ import annotations

import argparse
import ctypes as C
import math
import sys
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (ArrayLike, check_finite_options, default_device, f32_rows, host_array, nonneg, positive,
                    ptr as _ptr, require_hip as _require_hip, stream as _stream, to_device)

EMPTY = -(1 << 31)             # GG_PLACE_EMPTY
MAX_LEVEL = 1 << 28            # GG_PLACE_MAX_LEVEL
MAX_DIM = 4096                 # GG_PLACE_MAX_DIM
MAX_FOOT = 128                 # GG_PLACE_MAX_FOOT
MAX_YAWS = 256                 # GG_PLACE_MAX_YAWS
# UNVERIFIED defaults (PARITY.md "Placement"): this project's choices, not checked on a real checkpoint
CELL = 0.005                   # metres: the grid's cell edge
LEVEL = 0.001                  # metres: one height level
YAWS = 16                      # over [0, pi)
TOL = 2                        # levels: a cell within this of the highest contact counts as a contact
MIN_CONTACT = 0.1              # of the object's cells
STABILITY_MARGIN = 1           # cells the contact box is shrunk by before the pivot must lie in it
DILATE = 1                     # cells the underside maps are grown by: the clearance margin
MAX_STEP = 5                   # levels above the bare plane's resting level that still count as "on the plane"
REGION = 0.3                   # metres: half edge of the searched square around the target (or the object)


@dataclass
class PlaneFrame:
    """The support plane as a frame: `o` on the plane, e0 and e1 in it, e2 = n its normal.  fp64, orthonormal."""
    o: np.ndarray
    e0: np.ndarray
    e1: np.ndarray
    e2: np.ndarray

    def rows(self) -> np.ndarray:
        """(12,): o, e0, e1, e2 — one frame as gg_height_map takes it."""
        return np.concatenate([self.o, self.e0, self.e1, self.e2])

    def coords(self, p: ArrayLike) -> np.ndarray:
        """(..., 3) points -> their (c0, c1, c2) in this frame, fp64."""
        d = np.asarray(p, np.float64) - self.o
        return np.stack([d @ self.e0, d @ self.e1, d @ self.e2], -1)


@dataclass
class PlaceSearch:
    rest: ArrayLike            # (K, I, J) int32: the level the object's frame rests at, EMPTY: invalid anchor
    contact: ArrayLike         # (K, I, J) int32: object cells within tol of the highest contact
    support: ArrayLike         # (K, I, J, 6) int32: over them sum a, sum b, min a, max a, min b, max b


@dataclass
class Placements:
    transform: np.ndarray      # (M, 3, 4) float64 [R | t]: the object's move, scene frame
    yaw: np.ndarray            # (M,) int64: index into the yaws
    anchor: np.ndarray         # (M, 2) int64: (i, j)
    rest: np.ndarray           # (M,) int64 levels
    lift: np.ndarray           # (M,) float64: (rest + 2) level, scene units along the normal
    contact_frac: np.ndarray   # (M,) float64: contact / the yaw's object cells
    score: np.ndarray          # (M,) float64: the order is by it, smaller first (distance to target, or -contact_frac)
    normal: np.ndarray         # (3,) float64: the plane's normal, the direction `lift` is along


# ------------------------------------------------------------------------------------------------
# host side (numpy, fp64)
# ------------------------------------------------------------------------------------------------
def _plane(plane) -> Tuple[np.ndarray, float]:
    """(n, offset) of a support.SupportPlane or of a pair (normal, offset), n brought to unit length."""
    n, d = (plane.normal, plane.offset) if hasattr(plane, "normal") else plane
    n = np.asarray(n, np.float64).reshape(-1)
    if n.shape != (3,) or not np.isfinite(n).all() or not float(n @ n) > 0.0 or not math.isfinite(float(d)):
        raise ValueError("a plane is a finite normal, not zero, and a finite offset")
    length = math.sqrt(float(n @ n))
    return n / length, float(d) / length


def plane_frame(plane, centre: ArrayLike) -> PlaneFrame:
    """The frame of the plane n.x + offset = 0 under `centre`: o = centre - (n.centre + offset) n; e0 = a x n / |a x n|
    with `a` the coordinate axis of the smallest |n| component (the first of equals); e1 = n x e0; e2 = n.  A pure
    function of its arguments."""
    n, d = _plane(plane)
    c = np.asarray(centre, np.float64).reshape(-1)
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError(f"centre must be three finite numbers, got {centre}")
    a = np.zeros(3)
    a[int(np.argmin(np.abs(n)))] = 1.0
    e0 = np.cross(a, n)
    e0 /= math.sqrt(float(e0 @ e0))
    e1 = np.cross(n, e0)
    e1 /= math.sqrt(float(e1 @ e1))
    return PlaneFrame(c - (float(n @ c) + d) * n, e0, e1, n)


def plane_grid(bbox_uv: Sequence[float], cell: float = CELL, level: float = LEVEL):
    """(grid, dims): lo_u, lo_v, the cell edge and the level height as float64 (4,), and the cells U, V that cover the
    box (u0, v0, u1, v1) of in-plane coordinates, int32 (2,).  ValueError beyond GG_PLACE_MAX_DIM cells per axis."""
    b = np.asarray(bbox_uv, np.float64).reshape(-1)
    h, hz = positive("cell", cell), positive("level", level)
    if b.shape != (4,) or not np.isfinite(b).all() or not (b[2] > b[0] and b[3] > b[1]):
        raise ValueError(f"bbox_uv must be finite (u0, v0, u1, v1) with u0 < u1 and v0 < v1, got {bbox_uv}")
    dims = np.maximum(1, np.ceil((b[2:] - b[:2]) / h)).astype(np.int64)
    if (dims > MAX_DIM).any():
        raise ValueError(f"{tuple(int(d) for d in dims)} cells: at most {MAX_DIM} per axis; use a larger cell or a "
                         "smaller box")
    return np.array([b[0], b[1], h, hz], np.float64), dims.astype(np.int32)


def yaw_angles(yaws=YAWS) -> np.ndarray:
    """A count K -> K angles k pi / K over [0, pi); a sequence of angles (radians) -> itself, fp64."""
    if np.ndim(yaws) == 0:
        k = int(yaws)
        if not 1 <= k <= MAX_YAWS:
            raise ValueError(f"yaws must be in 1..{MAX_YAWS}, got {yaws}")
        return np.arange(k, dtype=np.float64) * (math.pi / k)
    th = np.asarray(yaws, np.float64).reshape(-1)
    if not 1 <= len(th) <= MAX_YAWS or not np.isfinite(th).all():
        raise ValueError(f"yaws must be 1..{MAX_YAWS} finite angles")
    return th


def yaw_frames(frame: PlaneFrame, pivot: ArrayLike, yaws, A: int, B: int, h: float) -> np.ndarray:
    """(K, 4, 3) fp64: the object's frames o, e0, e1, e2 = n.  e0k = cos t e0 + sin t e1, e1k = -sin t e0 + cos t e1;
    the origin lies on the plane and is chosen so that the pivot has c0 = (A // 2) h and c1 = (B // 2) h: over the
    grid (0, 0, h, .) it sits on the corner between cells, and cell (A // 2, B // 2) starts there."""
    th = yaw_angles(yaws)
    p = np.asarray(pivot, np.float64).reshape(3)
    foot = p - float((p - frame.o) @ frame.e2) * frame.e2
    out = np.empty((len(th), 4, 3))
    for k, t in enumerate(th):
        c, s = math.cos(t), math.sin(t)
        e0, e1 = c * frame.e0 + s * frame.e1, -s * frame.e0 + c * frame.e1
        out[k] = foot - (A // 2) * float(h) * e0 - (B // 2) * float(h) * e1, e0, e1, frame.e2
    return out


def underside(frames: np.ndarray) -> np.ndarray:
    """The frames with e2 negated, as (K, 12) rows: a height map in them holds max level(-c2), the object's
    underside."""
    f = np.array(frames, np.float64, copy=True).reshape(-1, 4, 3)
    f[:, 3] = -f[:, 3]
    return f.reshape(-1, 12)


def dilate_maps(maps: np.ndarray, cells: int) -> np.ndarray:
    """Grey dilation of every [A][B] map by the flat (2 cells + 1)^2 square: the maximum over the square, the map's
    outside and EMPTY cells counting as nothing."""
    m = np.asarray(maps, np.int32)
    d = int(cells)
    if d < 0:
        raise ValueError(f"dilate must be >= 0, got {cells}")
    if d == 0:
        return m.copy()
    A, B = m.shape[-2:]
    pad = np.full(m.shape[:-2] + (A + 2 * d, B + 2 * d), EMPTY, np.int32)
    pad[..., d:d + A, d:d + B] = m
    out = m.copy()
    for da in range(2 * d + 1):
        for db in range(2 * d + 1):
            np.maximum(out, pad[..., da:da + A, db:db + B], out=out)
    return out


def placement_transform(frame: PlaneFrame, grid: ArrayLike, obj_frame: ArrayLike, anchor: Sequence[int],
                        rest: int) -> np.ndarray:
    """(3, 4) fp64 [R | t] that puts the object down at `anchor` (i, j) resting at level `rest`: a point with
    coordinates (c0, c1, c2) in obj_frame (one of yaw_frames: o, e0, e1, n) goes to
    o + (lo_u + i h + c0) e0 + (lo_v + j h + c1) e1 + (c2 + lift) n with lift = (rest + 2) hz.  Every scene point of a
    cell lies below (top + 1) hz and every object point of a cell above -(under + 1) hz, so lift >= (top + under + 2)
    hz clears them all, and at the highest contact the gap is at most 2 hz."""
    g = np.asarray(grid, np.float64).reshape(4)
    f = np.asarray(obj_frame, np.float64).reshape(4, 3)
    i, j = int(anchor[0]), int(anchor[1])
    R = np.outer(frame.e0, f[1]) + np.outer(frame.e1, f[2]) + np.outer(frame.e2, f[3])
    lift = (int(rest) + 2) * g[3]
    t = frame.o + (g[0] + i * g[2]) * frame.e0 + (g[1] + j * g[2]) * frame.e1 + lift * frame.e2 - R @ f[0]
    return np.concatenate([R, t[:, None]], 1)


def propose(found: PlaceSearch, under: ArrayLike, frame: PlaneFrame, grid: ArrayLike, obj_frames: ArrayLike,
            pivot: ArrayLike, floor: int = 0, max_step: Optional[int] = MAX_STEP, min_contact: float = MIN_CONTACT,
            stability_margin: int = STABILITY_MARGIN, target: Optional[ArrayLike] = None,
            top_k: Optional[int] = None) -> Placements:
    """The valid anchors of `found` that pass all of
        rest - free_rest[k] <= max_step levels, free_rest[k] = floor + max under[k], the value on the bare plane
            (max_step None: no limit, the object may stand on whatever stands on the plane);
        contact >= min_contact cells[k], cells[k] the object cells of yaw k;
        the pivot's cell (A // 2, B // 2) inside the contact box shrunk by stability_margin cells on every side;
    ordered by the distance of the landed pivot from `target` (a 3-D point) when given, else by descending contact
    fraction; ties by (k, i, j) ascending.  The gates are integer comparisons (contact cells[k]' >= min_contact cells[k]
    is one product in fp64); only the order by target uses the transforms.  top_k: the first so many."""
    rest, contact, support = (host_array(x, np.int64) for x in (found.rest, found.contact, found.support))
    und = host_array(under, np.int64)
    K, A, B = und.shape
    if rest.shape[:1] != (K,) or contact.shape != rest.shape or support.shape != rest.shape + (6,):
        raise ValueError(f"rest {rest.shape}, contact {contact.shape}, support {support.shape} do not belong to "
                         f"{K} maps")
    full = und != EMPTY
    cells = full.reshape(K, -1).sum(1)
    free = np.where(cells > 0, np.where(full, und, -MAX_LEVEL).reshape(K, -1).max(1) + int(floor), 0)
    keep = rest != EMPTY
    if max_step is not None:
        keep &= rest - free[:, None, None] <= int(max_step)
    keep &= contact.astype(np.float64) >= float(min_contact) * cells[:, None, None].astype(np.float64)
    m = int(stability_margin)
    keep &= (support[..., 2] + m <= A // 2) & (A // 2 <= support[..., 3] - m)
    keep &= (support[..., 4] + m <= B // 2) & (B // 2 <= support[..., 5] - m)
    k, i, j = np.nonzero(keep)                                   # (k, i, j) ascending
    r = rest[k, i, j]
    frac = contact[k, i, j] / np.maximum(cells[k], 1)
    g = np.asarray(grid, np.float64).reshape(4)
    T = np.empty((len(k), 3, 4))
    for n in range(len(k)):
        T[n] = placement_transform(frame, g, obj_frames[k[n]], (i[n], j[n]), r[n])
    if target is not None:
        tgt = np.asarray(target, np.float64).reshape(3)
        p = np.asarray(pivot, np.float64).reshape(3)
        score = np.sqrt((((T[:, :, :3] @ p + T[:, :, 3]) - tgt) ** 2).sum(1)) if len(k) else np.zeros(0)
    else:
        score = -frac
    order = np.argsort(score, kind="stable")[:top_k]
    return Placements(T[order], k[order], np.stack([i[order], j[order]], 1), r[order], (r[order] + 2) * g[3],
                      frac[order], score[order], np.array(frame.e2, np.float64))


def release_paths(placements: Placements, grasp_row: ArrayLike, lift: float, steps: int) -> np.ndarray:
    """(M, steps, 12) float32 gripper poses (R row-major, then t, as field.path_clear takes them): the grasp pose of
    `grasp_row` ((17,), grasp.load_grasps: R at 4..12, t at 13..15) carried along with the object, T_place . grasp
    pose, descending against the plane's normal from `lift` scene units above at waypoint 0 to the placement itself at
    the last one, orientation fixed."""
    g = host_array(grasp_row, np.float64).reshape(-1)
    if g.shape != (17,):
        raise ValueError(f"a grasp row is (17,), got {g.shape}")
    steps, up = int(steps), nonneg("lift", lift)
    if steps < 2:
        raise ValueError(f"steps must be >= 2, got {steps}")
    Rg, tg = g[4:13].reshape(3, 3), g[13:16]
    T = np.asarray(placements.transform, np.float64).reshape(-1, 3, 4)
    R = T[:, :, :3] @ Rg
    t = T[:, :, :3] @ tg + T[:, :, 3]
    s = up * (1.0 - np.arange(steps) / (steps - 1.0))                       # lift .. 0
    out = np.empty((len(T), steps, 12))
    out[:, :, :9] = R.reshape(-1, 1, 9)
    out[:, :, 9:] = t[:, None, :] + s[None, :, None] * np.asarray(placements.normal, np.float64).reshape(1, 1, 3)
    return np.ascontiguousarray(out.astype(np.float32))


# ------------------------------------------------------------------------------------------------
# device side: the two calls
# ------------------------------------------------------------------------------------------------
def _grid_args(grid, dims):
    g = np.asarray(grid, np.float64).reshape(-1)
    d = np.asarray(dims, np.int64).reshape(-1)
    if g.shape != (4,) or d.shape != (2,):
        raise ValueError("grid is (4,) lo_u, lo_v, cell edge, level height; dims (2,) cells")
    return (C.c_double * 4)(*g.tolist()), (C.c_int32 * 2)(*d.tolist()), (int(d[0]), int(d[1]))


def height_map(points: Tensor, weights: Optional[Tensor], frames: ArrayLike, grid, dims, min_weight: float = 0.0,
               out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(map int32 (F, U, V), dropped int64 (F,)) of one gg_height_map call.  points (N, 3) float32 and weights (N,)
    float32 or None on the HIP device (no CPU path); frames (F, 12) or (F, 4, 3) fp64 (o, e0, e1, e2).  `out`: a map to
    accumulate into; None starts from EMPTY.  Nothing waits on the host."""
    dev = _require_hip(points) if weights is None else _require_hip(points, weights)
    points = f32_rows(points, "points", 3)
    if weights is not None:
        weights = f32_rows(weights, "weights", None)
        if weights.shape[0] != points.shape[0]:
            raise ValueError(f"points has {points.shape[0]} rows, weights {weights.shape[0]}")
    fr = np.ascontiguousarray(host_array(frames, np.float64).reshape(-1, 12))
    F = fr.shape[0]
    if not 1 <= F <= MAX_YAWS:
        raise ValueError(f"need 1..{MAX_YAWS} frames, got {F}")
    if math.isnan(float(min_weight)):
        raise ValueError("min_weight must not be NaN")
    g, d, (U, V) = _grid_args(grid, dims)
    if out is None:
        out = torch.full((F, U, V), EMPTY, dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or tuple(out.shape) != (F, U, V) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous int32 {(F, U, V)} tensor on {dev}")
    frames_dev = torch.from_numpy(fr).to(dev)
    dropped = torch.empty(F, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().gg_height_map(points.shape[0], _ptr(points), _ptr(weights), float(min_weight), F,
                                         _ptr(frames_dev), g, d, _ptr(out), _ptr(dropped), _stream(dev)),
               "gg_height_map")
    return out, dropped


def search(top: ArrayLike, under: ArrayLike, tol: int = TOL, device=None) -> PlaceSearch:
    """PlaceSearch of one gg_place_search call: top int32 (U, V), under int32 (K, A, B) with A <= U, B <= V, every
    level that is not EMPTY within +-MAX_LEVEL (checked here: it is the C call's precondition).  Tensors on the HIP
    device are taken as they are; arrays are copied to `device` (default: the current one).  No CPU path."""
    if isinstance(top, Tensor) and top.device.type == "cuda":
        dev = top.device
    elif device is not None:
        dev = torch.device(device)
    else:
        dev = default_device("place")
    top, under = to_device(top, torch.int32, dev), to_device(under, torch.int32, dev)
    if top.ndim != 2 or under.ndim != 3:
        raise ValueError(f"top is (U, V) and under (K, A, B), got {tuple(top.shape)} and {tuple(under.shape)}")
    (U, V), (K, A, B) = top.shape, under.shape
    if not (1 <= U <= MAX_DIM and 1 <= V <= MAX_DIM and K <= MAX_YAWS and 1 <= A <= min(MAX_FOOT, U)
            and 1 <= B <= min(MAX_FOOT, V)):
        raise ValueError(f"top {(U, V)} (each <= {MAX_DIM}), under {(K, A, B)} (K <= {MAX_YAWS}, A, B <= {MAX_FOOT} "
                         "and no larger than the scene's map)")
    if not 0 <= int(tol) <= MAX_LEVEL:
        raise ValueError(f"tol must be in 0..{MAX_LEVEL}, got {tol}")
    for name, m in (("top", top), ("under", under)):
        if bool(((m != EMPTY) & ((m < -MAX_LEVEL) | (m > MAX_LEVEL))).any()):
            raise ValueError(f"{name} holds a level beyond +-{MAX_LEVEL}")
    I, J = U - A + 1, V - B + 1
    rest = torch.empty(K, I, J, dtype=torch.int32, device=dev)
    contact = torch.empty(K, I, J, dtype=torch.int32, device=dev)
    support = torch.empty(K, I, J, 6, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_place_search((C.c_int32 * 2)(U, V), _ptr(top), K, (C.c_int32 * 2)(A, B), _ptr(under),
                                           int(tol), _ptr(rest), _ptr(contact), _ptr(support), _stream(dev)),
               "gg_place_search")
    return PlaceSearch(rest, contact, support)


# ------------------------------------------------------------------------------------------------
# maps of a scene and of an object
# ------------------------------------------------------------------------------------------------
def top_map(points, weights, frame: PlaneFrame, grid, dims, min_weight: float = 0.0, floor: Optional[int] = 0,
            maps: Callable = height_map) -> np.ndarray:
    """The top map of points, int32 (U, V) on the host: the highest level of the points that take part (weights: the
    opacities with the object's set to 0, which leaves it out) per cell of the plane's grid.  Cells that no point fell
    in are given `floor`, the plane's own level, unless floor is None: a table is never sampled densely enough for
    every cell."""
    top = host_array(maps(points, weights, frame.rows()[None], grid, dims, min_weight)[0])[0].astype(np.int32)
    if floor is not None:
        if not -MAX_LEVEL <= int(floor) <= MAX_LEVEL:
            raise ValueError(f"floor must be within +-{MAX_LEVEL}, got {floor}")
        top = np.where(top == EMPTY, np.int32(floor), top)
    return top


def footprint_cells(radius: float, cell: float, dilate: int = DILATE) -> int:
    """The edge A = B of the underside maps of an object whose points lie within `radius` of the pivot's normal line:
    2 (ceil(radius / cell) + 1 + dilate), so that every yaw fits with `dilate` cells to spare.  ValueError beyond
    GG_PLACE_MAX_FOOT, naming the cell that would fit."""
    r, h, d = nonneg("radius", radius), positive("cell", cell), int(dilate)
    if d < 0:
        raise ValueError(f"dilate must be >= 0, got {dilate}")
    n = 2 * (int(math.ceil(r / h)) + 1 + d)
    if n > MAX_FOOT:
        room = MAX_FOOT // 2 - 1 - d
        fit = f"a cell of at least {r / room * (1.0 + 1e-9):.6g}" if room >= 1 else "a smaller dilate"
        raise ValueError(f"a footprint of {n} x {n} cells is more than {MAX_FOOT}: radius {r:.6g} at cell {h:.6g} "
                         f"needs {fit}")
    return n


def under_maps(points, weights, frame: PlaneFrame, pivot: ArrayLike, radius: float, yaws=YAWS, cell: float = CELL,
               level: float = LEVEL, dilate: int = DILATE, min_weight: float = 0.0, maps: Callable = height_map):
    """(under int32 (K, A, A) on the host, obj_frames (K, 4, 3), dropped (K,)): the object's underside per yaw over the
    grid (0, 0, cell, level) of its own frames (yaw_frames around `pivot`), each map grown by `dilate` cells
    (dilate_maps).  weights: the opacities with everything but the object set to 0.  radius: the largest in-plane
    distance of an object point from the pivot (footprint_cells sizes the maps by it)."""
    A = footprint_cells(radius, cell, dilate)
    frames = yaw_frames(frame, pivot, yaws, A, A, cell)
    und, dropped = maps(points, weights, underside(frames), np.array([0.0, 0.0, cell, level]), (A, A), min_weight)
    return dilate_maps(host_array(und), dilate), frames, host_array(dropped)


def object_pivot(points, object_weights, normal: ArrayLike, min_weight: float = 0.0) -> Tuple[np.ndarray, float]:
    """(pivot (3,), radius): the weighted centroid of the points with weight > min_weight, summed in fp64 on the host
    (the object's points are read back for it, the others are not), and the largest distance of one of them from the
    line through the pivot along `normal`."""
    n = np.asarray(normal, np.float64).reshape(3)
    ow = host_array(object_weights, np.float64).reshape(-1)
    sel = np.nonzero(ow > float(min_weight))[0]
    if isinstance(points, Tensor):
        obj = points[torch.from_numpy(sel).to(points.device)].detach().cpu().numpy().astype(np.float64)
    else:
        obj = np.asarray(points)[sel].astype(np.float64)
    fin = np.isfinite(obj).all(1)
    obj, w = obj[fin], ow[sel][fin]
    if len(obj) == 0:
        raise ValueError("the object has no point that takes part")
    pivot = (obj * w[:, None]).sum(0) / w.sum()
    d = obj - pivot
    return pivot, math.sqrt(float(np.maximum((d * d).sum(1) - (d @ n) ** 2, 0.0).max()))


def _model_weights(model_or_scene, mask: Optional[Tensor]):
    """(points, weights outside the mask, weights inside it) of a model or scene: grasp.model_points' means and
    sigmoid(opacities), split by `mask` (N,); None: everything is outside."""
    from .grasp import model_points
    pts, _, w = model_points(model_or_scene, None)
    if mask is None:
        return pts, w, torch.zeros_like(w)
    mask = mask.reshape(-1).to(device=pts.device, dtype=torch.bool)
    if mask.shape[0] != pts.shape[0]:
        raise ValueError(f"mask has {mask.shape[0]} entries for {pts.shape[0]} Gaussians")
    zero = torch.zeros_like(w)
    return pts, torch.where(mask, zero, w), torch.where(mask, w, zero)


@torch.no_grad()
def scene_top(model_or_scene, plane, bbox_uv: Sequence[float], cell: float = CELL, level: float = LEVEL,
              exclude: Optional[Tensor] = None, floor: Optional[int] = 0, centre: ArrayLike = (0.0, 0.0, 0.0),
              min_weight: float = 0.0):
    """(top int32 (U, V) on the host, frame, grid, dims): the top map of a model's Gaussians over the box bbox_uv
    (u0, v0, u1, v1) of plane_frame(plane, centre)'s in-plane coordinates, the Gaussians of `exclude` (N,) left out
    (the object).  Empty cells are given `floor`, the plane's level, unless floor is None."""
    pts, w, _ = _model_weights(model_or_scene, exclude)
    frame = plane_frame(plane, centre)
    grid, dims = plane_grid(bbox_uv, cell, level)
    return top_map(pts, w, frame, grid, dims, min_weight, floor), frame, grid, dims


@torch.no_grad()
def object_under(model_or_scene, mask: Tensor, plane, yaws=YAWS, cell: float = CELL, level: float = LEVEL,
                 dilate: int = DILATE, min_weight: float = 0.0, centre: Optional[ArrayLike] = None):
    """(under int32 (K, A, A) on the host, obj_frames (K, 4, 3), pivot (3,)): the underside maps of the Gaussians
    `mask` selects, one per yaw about their opacity-weighted centroid (object_pivot), grown by `dilate` cells.
    centre: that of the plane's frame (plane_frame; None: the pivot), which fixes the frames to the bit.
    ValueError when the footprint exceeds GG_PLACE_MAX_FOOT cells, naming the cell that would fit."""
    pts, _, w = _model_weights(model_or_scene, mask)
    n, _ = _plane(plane)
    pivot, radius = object_pivot(pts, w, n, min_weight)
    frame = plane_frame(plane, pivot if centre is None else centre)
    under, frames, _ = under_maps(pts, w, frame, pivot, radius, yaws, cell, level, dilate, min_weight)
    return under, frames, pivot


@dataclass
class PlacePlan:
    """Everything place_points made on the way: what tests, tools and a planner look at."""
    placements: Placements
    frame: PlaneFrame
    grid: np.ndarray           # (4,) lo_u, lo_v, cell, level
    dims: np.ndarray           # (2,) U, V
    top: np.ndarray            # (U, V) int32
    under: np.ndarray          # (K, A, A) int32
    obj_frames: np.ndarray     # (K, 4, 3)
    pivot: np.ndarray          # (3,)
    found: PlaceSearch


def place_points(points, scene_weights, object_weights, plane, target: Optional[ArrayLike] = None, cell: float = CELL,
                 level: float = LEVEL, yaws=YAWS, tol: int = TOL, dilate: int = DILATE, region: float = REGION,
                 min_weight: float = 0.0, floor: Optional[int] = 0, max_step: Optional[int] = MAX_STEP,
                 min_contact: float = MIN_CONTACT, stability_margin: int = STABILITY_MARGIN,
                 top_k: Optional[int] = None, maps: Callable = height_map, searcher: Callable = search) -> PlacePlan:
    """plane -> maps -> search -> propose on (N, 3) points with two weight vectors: the scene's (the object's entries
    0) and the object's (everything else 0).  The pivot is the object's weighted centroid, summed in fp64 on the host
    over the object's points (they are read back; the scene's are not).  The searched square has half edge `region`
    around the target's foot on the plane, or around the pivot's without a target.  `maps` and `searcher` are the two
    device calls; tests/place_ref.py's restatements take their place in the tests, nothing else does."""
    n, _ = _plane(plane)
    pivot, radius = object_pivot(points, object_weights, n, min_weight)
    centre = pivot if target is None else np.asarray(target, np.float64).reshape(3)
    frame = plane_frame(plane, centre)
    r = positive("region", region)
    grid, dims = plane_grid((-r, -r, r, r), cell, level)
    under, obj_frames, _ = under_maps(points, object_weights, frame, pivot, radius, yaws, cell, level, dilate,
                                      min_weight, maps)
    top = top_map(points, scene_weights, frame, grid, dims, min_weight, floor, maps)
    if under.shape[1] > top.shape[0] or under.shape[2] > top.shape[1]:
        raise ValueError(f"the object's {under.shape[1]} cells do not fit a region of {top.shape[0]}: use a larger "
                         "region")
    found = searcher(top, under, tol)
    got = propose(found, under, frame, grid, obj_frames, pivot, 0 if floor is None else floor, max_step, min_contact,
                  stability_margin, target, top_k)
    return PlacePlan(got, frame, grid, dims, top, under, obj_frames, pivot, found)


@torch.no_grad()
def place_object(model_or_scene, mask: Tensor, plane=None, target: Optional[ArrayLike] = None, **kw) -> PlacePlan:
    """place_points on a model's or scene's Gaussians: the means, sigmoid(opacities) as weights, `mask` (N,) selecting
    the object.  plane None: support.support_plane(model, mask) fits the table around the object.  Keywords:
    place_points'."""
    pts, scene_w, object_w = _model_weights(model_or_scene, mask)
    if plane is None:
        from . import support
        plane = support.support_plane(model_or_scene, mask)
    return place_points(pts, scene_w, object_w, plane, target, **kw)


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def main(argv: Optional[Sequence[str]] = None) -> int:
    from ._cli import (add_object_options, add_support_options, check_object_options, check_support_options,
                       load_scene, object_mask, support_option_plane)
    from .frames import load_transform_json
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.place",
                                 description="Poses at which the selected object rests on the support plane (or on "
                                             "what stands on it) without entering anything.")
    ap.add_argument("--ckpt", required=True, help="step-*.ckpt of a splatting model")
    ap.add_argument("--transform-json", default=None, help="JSON with transform_matrix and scale (world -> scene)")
    add_object_options(ap, "the Gaussians the query selects are the object to put down",
                       "selects the object to put down")
    add_support_options(ap, grasp=False)
    ap.add_argument("--cell", type=float, default=CELL, help="cell edge of the plane's grid, scene units")
    ap.add_argument("--level", type=float, default=LEVEL, help="height of one level, scene units")
    ap.add_argument("--yaws", type=int, default=YAWS, help="rotations about the normal that are tried, over [0, pi)")
    ap.add_argument("--region", type=float, default=REGION, help="half edge of the searched square, scene units")
    ap.add_argument("--target", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                    help="scene-frame point the placements are ordered by (default: by contact fraction)")
    ap.add_argument("--tol", type=int, default=TOL, help="levels within which a cell counts as a contact")
    ap.add_argument("--max-step", type=int, default=MAX_STEP, metavar="LEVELS",
                    help="how far above the bare plane the object may rest; negative: no limit (stacking)")
    ap.add_argument("--min-contact", type=float, default=MIN_CONTACT, help="share of the object's cells in contact")
    ap.add_argument("--stability-margin", type=int, default=STABILITY_MARGIN, help="cells the contact box is shrunk by")
    ap.add_argument("--dilate", type=int, default=DILATE, help="cells of clearance around the object")
    ap.add_argument("--min-opacity", type=float, default=0.0, help="a Gaussian takes part above it")
    ap.add_argument("--top-k", type=int, default=None, help="write the best K placements only")
    ap.add_argument("--out", required=True, help="output .npz: transform, yaw, anchor, rest, lift, contact_frac, score")
    a = ap.parse_args(argv)
    check_object_options(ap, a, "required")
    check_support_options(ap, a, grasp=False)
    check_finite_options(ap, a, positive=("cell", "level", "region"))
    if not 1 <= a.yaws <= MAX_YAWS:
        ap.error(f"--yaws must be in 1..{MAX_YAWS}, got {a.yaws}")
    if not 0 <= a.tol <= MAX_LEVEL or a.dilate < 0 or a.stability_margin < 0:
        ap.error("--tol, --dilate and --stability-margin must be >= 0")
    if not 0.0 <= a.min_contact <= 1.0 or math.isnan(a.min_opacity):
        ap.error("--min-contact must be in [0, 1] and --min-opacity not NaN")
    if a.top_k is not None and a.top_k < 1:
        ap.error(f"--top-k must be >= 1, got {a.top_k}")
    try:
        matrix, scale = load_transform_json(a.transform_json) if a.transform_json else (None, 1.0)
        scene, mlp_state = load_scene(a.ckpt)
        mask = object_mask(a, scene, mlp_state, matrix, scale)
        plane = support_option_plane(a, scene, mask, scale)
        plan = place_object(scene, mask, plane, a.target, cell=a.cell, level=a.level, yaws=a.yaws, tol=a.tol,
                            dilate=a.dilate, region=a.region, min_weight=a.min_opacity,
                            max_step=None if a.max_step < 0 else a.max_step, min_contact=a.min_contact,
                            stability_margin=a.stability_margin, top_k=a.top_k)
    except (KeyError, ValueError, OSError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    p = plan.placements
    np.savez(a.out, transform=p.transform, yaw=p.yaw, anchor=p.anchor, rest=p.rest, lift=p.lift,
             contact_frac=p.contact_frac, score=p.score, yaw_angles=yaw_angles(a.yaws), normal=plan.frame.e2,
             pivot=plan.pivot)
    valid = int((host_array(plan.found.rest) != EMPTY).sum())
    print(f"{tuple(int(d) for d in plan.dims)} cells, footprint {plan.under.shape[1]} x {plan.under.shape[2]} x "
          f"{plan.under.shape[0]} yaws: {valid} valid anchors, {len(p.yaw)} placements; wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
