"""The scene as a distance field, for the transit of the gripper: the Gaussians splatted into integer occupancy mass
(`gg_field_splat`), the exact squared Euclidean distance transform of the occupied cells (`gg_field_distance`), and
many gripper paths tested against it (`gg_field_paths`), csrc/field.hip.  The contract is in include/gg_raster.h and
PARITY.md "Distance field"; the design in DESIGN.md §3.25.

    DistanceField      the volume: .add / .remove Gaussians (a moved object: remove it, add it at the moved pose; no
                       rebuild), .update the distances, .distance() in scene units, .save / .load
    need2              the squared cell distance a sphere of `radius` plus `margin` needs: conservative
    gripper_spheres    a grasp gripper model (grasp.default_gripper, ...) at given sizes, covered by spheres
    grasp_poses        (M, 17) grasp rows as (M, 1, 12) poses
    approach_paths     the straight approach of every row from a standoff, as (M, steps, 12) poses
    interpolate        slerp plus lerp between two poses, on the host (slerp_rotations: its slerp at given fractions)
    path_clear         slack per waypoint, first hit and clear per path
    depth_pyramid      the min-depth pyramid of depth frames (gg_depth_min_pyramid)
    observe            one gg_field_observe call: which cells the frames have seen to be empty, through all of them
    DistanceField      .observe / .observe_scan / .observe_model count the views that saw each cell free, .assume_free
                       declares a box known, .update(unknown="blocked") makes what was never seen an obstacle
                       (gg_field_distance_known), .knowledge() counts the cells of each state (PARITY.md "Known free
                       space")
    python -m gaussiangrasper_amd.field --ckpt IN --bbox x0 y0 z0 x1 y1 z1 --voxel H --out field.npz [...]
        [--observe-scan DIR | --observe-transforms T.json] [--unknown blocked --min-views 2 --assume-free BOX ...]

The field is for the transit.  At the grasp pose the fingers touch the object, where a cell-conservative sphere test
rejects everything: there grasp.contacts' and grasp.clearance's exact box tests stay in charge."""
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
from ._call import (ArrayLike, check_finite_options, default_device, f32_rows, host_array, nonneg, positive,
                    ptr as _ptr, require_hip as _require_hip, sized_workspace, stream as _stream, to_device)
from .grasp import MIN_WEIGHT, check_gripper

FAR = 1 << 30                  # GG_FIELD_FAR
MAX_DIM = 1024                 # GG_FIELD_MAX_DIM
MAX_CELLS = 1 << 27            # GG_FIELD_MAX_CELLS
MAX_REACH_LIMIT = 64           # GG_FIELD_MAX_REACH
MAX_SPHERES = 1024             # GG_FIELD_MAX_SPHERES
MAX_POSES = 1 << 26            # GG_FIELD_MAX_POSES
VOTE_ONE = 1 << 16             # a weight of 1 as a vote
# UNVERIFIED defaults (PARITY.md "Distance field"): this project's choices, not checked on a real checkpoint
EXTENT = 1.0
MAX_REACH = 8
THRESHOLD = VOTE_ONE // 2      # trunc(0.5 2^16)
VOXEL = 0.01
# Known free space.  UNVERIFIED on a real scan (PARITY.md "Known free space"): this project's choices, like the 2^-20
# pixel pad of the kernel's footprint.
OBSERVE_MARGIN = 0.005         # the measured surface must lie this far beyond every point of a cell, scene units
OBSERVE_NEAR = 0.05            # a view takes no part in a cell that comes nearer to its camera plane than this
OBSERVE_MIN_VIEWS = 2          # views that must have seen a cell free before update(unknown="blocked") opens it
SEEN_MAX = 65535               # both counters saturate here
MAX_VIEWS = 1 << 20            # GG_TSDF_MAX_VIEWS
MAX_SIDE = 32768               # GG_TSDF_MAX_SIDE


@dataclass
class SplatCounts:
    """Of one gg_field_splat call: the rows that took no part and the rows max_reach cut (0-dim int64 tensors)."""
    skipped: Tensor
    truncated: Tensor


@dataclass
class PathClearance:
    slack: Tensor          # (P, W) int32: min over the spheres of dist2 - need2; < 0: too near
    first_hit: Tensor      # (P,) int32: the first waypoint with slack < 0, W when there is none
    clear: Tensor          # (P,) bool: first_hit == W


# ------------------------------------------------------------------------------------------------
# host side
# ------------------------------------------------------------------------------------------------
def field_grid(bbox_min: Sequence[float], bbox_max: Sequence[float], voxel: float = VOXEL):
    """(grid, dims): the lower corner and cell edge as float64 (4,), and the cells per axis that cover the box,
    int32 (3,).  ValueError beyond GG_FIELD_MAX_DIM per axis or GG_FIELD_MAX_CELLS in all."""
    lo, hi = np.asarray(bbox_min, np.float64).reshape(-1), np.asarray(bbox_max, np.float64).reshape(-1)
    h = positive("voxel", voxel)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()
                                                    and (hi > lo).all()):
        raise ValueError(f"bbox_min / bbox_max must be finite (3,) with min < max, got {lo} / {hi}")
    dims = np.maximum(1, np.ceil((hi - lo) / h)).astype(np.int64)
    if (dims > MAX_DIM).any() or int(dims.prod()) > MAX_CELLS:
        raise ValueError(f"{tuple(int(d) for d in dims)} cells: at most {MAX_DIM} per axis and {MAX_CELLS} in all; "
                         "use a larger voxel or a smaller box")
    return np.array([*lo, h], np.float64), dims.astype(np.int32)


def need2(radius: Union[float, ArrayLike], margin: float, h: float) -> np.ndarray:
    """floor(((radius + margin) / h + sqrt(3))^2) + 1, at most FAR, int32 (shaped like radius).  Conservative: with p
    in cell c and dist2[c] >= need2, the centres of c and of any occupied cell are further apart than radius + margin
    + sqrt(3) h, p is within sqrt(3)/2 h of the one and every point of the occupied cell's cube within sqrt(3)/2 h of
    the other, so no occupied cube meets the ball around p.  The square is nudged up by four ulps before the floor,
    so that fp64 rounding cannot land it below an integer the exact value reaches (radius + margin = 0 gives 4, not
    floor(2.9999999999999996) + 1)."""
    r = np.asarray(radius, np.float64) + float(margin)
    if not (np.isfinite(r).all() and (r >= 0).all()):
        raise ValueError("radius + margin must be finite and >= 0")
    v = np.floor((r / positive("h", h) + math.sqrt(3.0)) ** 2 * (1.0 + 2.0 ** -50)) + 1.0
    return np.minimum(v, float(FAR)).astype(np.int32)


def gripper_boxes(parts: ArrayLike, width: float, depth: float, height: float) -> np.ndarray:
    """(P, 6) bounds x_lo, x_hi, y_lo, y_hi, z_lo, z_hi of a gripper model at these sizes (gg_grasp_clearance's form:
    ((c0 + cw width) + cd depth) + ch height)."""
    g = check_gripper(parts)
    return ((g[:, :, 0] + g[:, :, 1] * float(width)) + g[:, :, 2] * float(depth)) + g[:, :, 3] * float(height)


def gripper_spheres(parts: ArrayLike, width: float, depth: float, height: float, radius: float) -> np.ndarray:
    """(S, 3) float32 sphere centres, gripper frame, whose balls of `radius` cover every box of the model that is not
    empty: each box is cut into the fewest equal sub-boxes of edge <= 2 radius / sqrt(3) per axis (half diagonal <=
    radius) and every sub-box's centre is a sphere.  The edge is taken 1e-4 shorter, which is far more than the
    centres lose when they are rounded to float32.  ValueError when that takes more than GG_FIELD_MAX_SPHERES."""
    edge = 2.0 * positive("radius", radius) / math.sqrt(3.0) * (1.0 - 1e-4)
    out = []
    for b in gripper_boxes(parts, width, depth, height):
        if not (b[0] <= b[1] and b[2] <= b[3] and b[4] <= b[5]):
            continue
        axes = []
        for a in range(3):
            lo, hi = b[2 * a], b[2 * a + 1]
            n = max(1, int(math.ceil((hi - lo) / edge)))
            while (hi - lo) / n > edge:             # the division rounded the count down
                n += 1
            axes.append(lo + (np.arange(n) + 0.5) * ((hi - lo) / n))
        out.append(np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3))
    if not out:
        raise ValueError("the gripper has no part that is not empty at these sizes")
    c = np.concatenate(out)
    if len(c) > MAX_SPHERES:
        raise ValueError(f"{len(c)} spheres of radius {radius} are more than {MAX_SPHERES}: use a larger radius")
    return c.astype(np.float32)


def grasp_poses(rows: ArrayLike) -> np.ndarray:
    """(M, 17) grasp rows (grasp.load_grasps) as (M, 1, 12) float32 poses: R row-major, then t."""
    g = host_array(rows, np.float32)
    if g.ndim != 2 or g.shape[1] != 17:
        raise ValueError(f"grasp rows are (M, 17), got {g.shape}")
    return np.ascontiguousarray(g[:, None, 4:16])


def approach_paths(rows: ArrayLike, standoff: float, steps: int) -> np.ndarray:
    """(M, steps, 12) float32: every row's straight approach, from `standoff` back along its approach axis (the first
    column of R) at waypoint 0 to the grasp pose at the last one, orientation fixed."""
    p = grasp_poses(rows)[:, 0].astype(np.float64)
    back, steps = nonneg("standoff", standoff), int(steps)
    if steps < 2:
        raise ValueError(f"steps must be >= 2, got {steps}")
    s = back * (1.0 - np.arange(steps) / (steps - 1.0))                     # standoff .. 0
    out = np.repeat(p[:, None, :], steps, 1)
    out[:, :, 9:12] = p[:, None, 9:12] - s[None, :, None] * p[:, None, 0:9:3]
    return np.ascontiguousarray(out.astype(np.float32))


def _quat(R: np.ndarray) -> np.ndarray:
    """wxyz unit quaternion of a rotation matrix (Shepperd: the largest of the four squares is the pivot)."""
    t = np.trace(R)
    d = [t, R[0, 0], R[1, 1], R[2, 2]]
    k = int(np.argmax(d))
    if k == 0:
        q = np.array([1.0 + t, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    else:
        i, j, l = k - 1, k % 3, (k + 1) % 3
        q = np.zeros(4)
        q[0] = R[l, j] - R[j, l]
        q[1 + i] = 1.0 + R[i, i] - R[j, j] - R[l, l]
        q[1 + j] = R[j, i] + R[i, j]
        q[1 + l] = R[l, i] + R[i, l]
    return q / np.linalg.norm(q)


def _rotmat(q: np.ndarray) -> np.ndarray:
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def interpolate(pose_a: ArrayLike, pose_b: ArrayLike, steps: int) -> np.ndarray:
    """(steps, 12) float32 poses from pose_a to pose_b (12 numbers each: R row-major, then t), both included: the
    rotation by slerp along the shorter arc, the translation by lerp.  fp64 on the host."""
    a, b = (np.asarray(p, np.float64).reshape(-1) for p in (pose_a, pose_b))
    steps = int(steps)
    if a.shape != (12,) or b.shape != (12,) or not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise ValueError("a pose is 12 finite numbers: R row-major, then t")
    if steps < 2:
        raise ValueError(f"steps must be >= 2, got {steps}")
    frac = np.arange(steps) / (steps - 1.0)
    out = np.empty((steps, 12))
    out[:, :9] = slerp_rotations(a[:9], b[:9], frac)
    for i, s in enumerate(frac):
        out[i, 9:] = (1.0 - s) * a[9:] + s * b[9:]
    out[0], out[-1] = a, b
    return out.astype(np.float32)


def slerp_rotations(rot_a: np.ndarray, rot_b: np.ndarray, fractions: Sequence[float]) -> np.ndarray:
    """(n, 9) float64 rotations, row-major, at `fractions` (each in 0..1) of the shorter arc from rot_a to rot_b (9
    numbers each): interpolate's slerp, for callers that bring their own fractions (transit.transit_poses)."""
    qa, qb = _quat(np.asarray(rot_a, np.float64).reshape(3, 3)), _quat(np.asarray(rot_b, np.float64).reshape(3, 3))
    dot = float(qa @ qb)
    if dot < 0.0:
        qb, dot = -qb, -dot
    theta = math.acos(min(1.0, dot))
    out = np.empty((len(fractions), 9))
    for i, s in enumerate(fractions):
        if theta < 1e-9:
            q = (1.0 - s) * qa + s * qb
        else:
            q = (math.sin((1.0 - s) * theta) * qa + math.sin(s * theta) * qb) / math.sin(theta)
        out[i] = _rotmat(q / np.linalg.norm(q)).reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------
# device side: the three calls
# ------------------------------------------------------------------------------------------------
def volume_args(dims, grid=None):
    """(c_int32[3] dims, c_double[4] grid or None, shape tuple) for the C ABI; transit.py and arm.py use these too."""
    d = host_array(dims, np.int64).reshape(-1)
    g = None if grid is None else host_array(grid, np.float64).reshape(-1)
    if d.shape != (3,) or (g is not None and g.shape != (4,)):
        raise ValueError("dims is (3,) cells" + ("" if g is None else ", grid (4,) lower corner and cell edge"))
    shape = tuple(int(v) for v in d)
    return (C.c_int32 * 3)(*shape), None if g is None else (C.c_double * 4)(*g.tolist()), shape


def volume_tensor(t: Tensor, name: str, dtype: torch.dtype, shape, dev: Optional[torch.device] = None) -> Tensor:
    """`t` after checking that it is a contiguous `dtype` tensor of `shape` (and on `dev`, when given)."""
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} {tuple(shape)} tensor, got {t.dtype} {tuple(t.shape)}")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} must be on {dev}, got {t.device}")
    return t


def cell_count(name: str, v: int) -> int:
    """A squared cell distance (`need`, `outside`) as an int in 0..FAR."""
    if not 0 <= int(v) <= FAR:
        raise ValueError(f"{name} must be in 0..{FAR}, got {v}")
    return int(v)


def pose_paths(poses: Tensor) -> Tensor:
    """`poses` contiguous, after checking that it is float32 (P, W, 12)."""
    if poses.dtype != torch.float32 or poses.ndim != 3 or poses.shape[2] != 12:
        raise ValueError(f"poses must be a float32 (P, W, 12) tensor, got {poses.dtype} {tuple(poses.shape)}")
    return poses.contiguous()


def sphere_table(spheres: Tensor, **int32_columns: Tensor):
    """(spheres, *columns) contiguous: spheres float32 (S, 3), S <= MAX_SPHERES, every named column int32 (S,)."""
    spheres = f32_rows(spheres, "spheres", 3)
    s = spheres.shape[0]
    if s > MAX_SPHERES:
        raise ValueError(f"{s} spheres are more than {MAX_SPHERES}")
    for name, t in int32_columns.items():
        if t.dtype != torch.int32 or tuple(t.shape) != (s,):
            raise ValueError(f"{name} must be an int32 ({s},) tensor, got {t.dtype} {tuple(t.shape)}")
    return (spheres, *(t.contiguous() for t in int32_columns.values()))


def splat(mass: Tensor, grid, dims, means: Tensor, rot: Tensor, scales: Tensor, weights: Tensor,
          extent: float = EXTENT, max_reach: int = MAX_REACH, min_weight: float = MIN_WEIGHT,
          sign: int = 1) -> SplatCounts:
    """One gg_field_splat call: adds sign times every row's vote into `mass` (int64 [X][Y][Z] on the HIP device, in
    place).  means (N, 3), rot (N, 9) or (N, 3, 3), scales (N, 3) activated, weights (N,): float32 on the same device
    (no CPU path).  Nothing waits on the host."""
    dev = _require_hip(mass, means, rot, scales, weights)
    d, g, shape = volume_args(dims, grid)
    volume_tensor(mass, "mass", torch.int64, shape)
    means = f32_rows(means, "means", 3)
    n = means.shape[0]
    rot = f32_rows(rot.reshape(rot.shape[0], 9) if rot.ndim == 3 else rot, "rot", 9)
    scales = f32_rows(scales, "scales", 3)
    weights = f32_rows(weights, "weights", None)
    if not (rot.shape[0] == scales.shape[0] == weights.shape[0] == n):
        raise ValueError(f"means has {n} rows, rot {rot.shape[0]}, scales {scales.shape[0]}, "
                         f"weights {weights.shape[0]}")
    if math.isnan(float(min_weight)):
        raise ValueError("min_weight must not be NaN")
    if int(sign) not in (1, -1):
        raise ValueError(f"sign must be +1 or -1, got {sign}")
    if not 0 <= int(max_reach) <= MAX_REACH_LIMIT:
        raise ValueError(f"max_reach must be in 0..{MAX_REACH_LIMIT}, got {max_reach}")
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().gg_field_splat(d, g, n, _ptr(means), _ptr(rot), _ptr(scales), _ptr(weights),
                                          nonneg("extent", extent), int(max_reach), float(min_weight), int(sign),
                                          _ptr(mass), _ptr(counts[0:]), _ptr(counts[1:]), _stream(dev)),
               "gg_field_splat")
    return SplatCounts(counts[0], counts[1])


def distance(mass: Tensor, dims, threshold: int = THRESHOLD, out: Optional[Tensor] = None) -> Tensor:
    """dist2 int32 [X][Y][Z] of `mass` (gg_field_distance): the squared distance, in cells, to the nearest cell with
    mass >= threshold; FAR everywhere when there is none."""
    dev = _require_hip(mass)
    d, _, shape = volume_args(dims)
    volume_tensor(mass, "mass", torch.int64, shape)
    if int(threshold) < 1:
        raise ValueError(f"threshold must be >= 1, got {threshold}")
    lib = _lib.load()
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=dev)
    volume_tensor(out, "out", torch.int32, shape, dev)
    ws = sized_workspace(lib.gg_field_distance_workspace(d), f"{shape} cells are beyond gg_field_distance's limits",
                         dev)
    _lib.check(lib.gg_field_distance(d, _ptr(mass), int(threshold), _ptr(out), _ptr(ws), ws.numel(), _stream(dev)),
               "gg_field_distance")
    return out


def cell_ball(h: float) -> float:
    """The radius gg_field_observe needs to cover a whole cell of edge h: half the cube's diagonal, a hair more, so
    that fp64 rounding cannot leave a corner outside: 0.5 sqrt(3) h (1 + 2^-40)."""
    return 0.5 * math.sqrt(3.0) * positive("h", h) * (1.0 + 2.0 ** -40)


def _frame_size(height: int, width: int) -> Tuple[int, int]:
    h, w = int(height), int(width)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"frames are 1..{MAX_SIDE} pixels a side, got {h} x {w}")
    return h, w


def pyramid_size(height: int, width: int) -> int:
    """S: the texels of one frame's pyramid, every level from the frame itself to 1 x 1."""
    h, w = _frame_size(height, width)
    s = 0
    while True:
        s += h * w
        if h == 1 and w == 1:
            return s
        h, w = (h + 1) // 2, (w + 1) // 2


def depth_pyramid(depth: Tensor) -> Tensor:
    """pyr float32 (V, S) of depth float32 (V, H, W) on the HIP device (gg_depth_min_pyramid): level 0 the frame
    with 0, negative and NaN as 0 ("no observation") and +inf kept, every further level the minimum of its up-to-four
    children, down to 1 x 1."""
    dev = _require_hip(depth)
    if depth.dtype != torch.float32 or depth.ndim != 3:
        raise ValueError(f"depth must be a float32 (V, H, W) tensor, got {depth.dtype} {tuple(depth.shape)}")
    depth = depth.contiguous()
    v = depth.shape[0]
    h, w = _frame_size(depth.shape[1], depth.shape[2])
    if v > MAX_VIEWS:
        raise ValueError(f"{v} frames are more than {MAX_VIEWS}")
    lib = _lib.load()
    size = int(lib.gg_depth_min_pyramid_size(h, w))
    pyr = torch.empty((v, size), dtype=torch.float32, device=dev)
    _lib.check(lib.gg_depth_min_pyramid(v, h, w, _ptr(depth), _ptr(pyr), _stream(dev)), "gg_depth_min_pyramid")
    return pyr


def camera_arrays(intrinsics: ArrayLike, w2c: ArrayLike, views: Optional[int] = None):
    """(K (V, 4), E (V, 3, 4)) float64 host arrays after the checks the device cannot make: all finite, fx, fy > 0."""
    k = host_array(intrinsics, np.float64).reshape(-1, 4)
    e = host_array(w2c, np.float64)
    e = e.reshape(-1, *e.shape[-2:])[:, :3, :] if e.ndim >= 2 and e.shape[-1] == 4 else e
    if e.ndim != 3 or e.shape[1:] != (3, 4) or e.shape[0] != k.shape[0] or (views is not None and views != k.shape[0]):
        raise ValueError(f"need (V, 4) intrinsics and (V, 3, 4) w2c for the same V"
                         f"{'' if views is None else f' = {views}'}, got {k.shape} and {e.shape}")
    if not (np.isfinite(k).all() and np.isfinite(e).all()):
        raise ValueError("intrinsics and w2c must be finite")
    if not (k[:, :2] > 0).all():
        raise ValueError("fx and fy must be > 0")
    return np.ascontiguousarray(k), np.ascontiguousarray(e)


def observe(seen: Tensor, looked: Optional[Tensor], grid, dims, pyr: Tensor, intrinsics: ArrayLike, w2c: ArrayLike,
            height: int, width: int, radius: float, margin: float = OBSERVE_MARGIN,
            near: float = OBSERVE_NEAR) -> None:
    """One gg_field_observe call: adds to seen (and looked, unless None) uint16 [X][Y][Z], in place, per cell the
    views that saw the whole ball of `radius` around its centre free by more than `margin` (that had it inside their
    image, at least `near` in front of the camera plane).  pyr (V, S): depth_pyramid's of V frames of height x width;
    intrinsics (V, 4) fx, fy, cx, cy and w2c (V, 3, 4) OpenCV world-to-camera: host arrays or tensors, taken as
    float64.  Tensors on the HIP device (no CPU path).  Nothing waits on the host."""
    dev = _require_hip(seen, pyr) if looked is None else _require_hip(seen, looked, pyr)
    d, g, shape = volume_args(dims, grid)
    volume_tensor(seen, "seen", torch.uint16, shape)
    if looked is not None:
        volume_tensor(looked, "looked", torch.uint16, shape)
    h, w = _frame_size(height, width)
    if pyr.dtype != torch.float32 or pyr.ndim != 2 or pyr.shape[1] != pyramid_size(h, w) or not pyr.is_contiguous():
        raise ValueError(f"pyr must be a contiguous float32 (V, {pyramid_size(h, w)}) tensor for {h} x {w} frames, "
                         f"got {pyr.dtype} {tuple(pyr.shape)}")
    v = pyr.shape[0]
    if v > MAX_VIEWS:
        raise ValueError(f"{v} frames are more than {MAX_VIEWS}")
    k, e = camera_arrays(intrinsics, w2c, v)
    kd, ed = torch.from_numpy(k).to(dev), torch.from_numpy(e).to(dev)
    _lib.check(_lib.load().gg_field_observe(d, g, v, h, w, _ptr(pyr), _ptr(kd), _ptr(ed), positive("radius", radius),
                                            nonneg("margin", margin), positive("near", near), _ptr(seen),
                                            _ptr(looked), _stream(dev)), "gg_field_observe")


def distance_known(mass: Tensor, seen: Tensor, dims, threshold: int = THRESHOLD,
                   min_views: int = OBSERVE_MIN_VIEWS, out: Optional[Tensor] = None) -> Tensor:
    """distance() with unknown space blocked (gg_field_distance_known): a cell seeds the transform iff mass >=
    threshold or seen < min_views."""
    dev = _require_hip(mass, seen)
    d, _, shape = volume_args(dims)
    volume_tensor(mass, "mass", torch.int64, shape)
    volume_tensor(seen, "seen", torch.uint16, shape)
    if int(threshold) < 1:
        raise ValueError(f"threshold must be >= 1, got {threshold}")
    if not 1 <= int(min_views) <= SEEN_MAX:
        raise ValueError(f"min_views must be in 1..{SEEN_MAX}, got {min_views}")
    lib = _lib.load()
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=dev)
    volume_tensor(out, "out", torch.int32, shape, dev)
    ws = sized_workspace(lib.gg_field_distance_workspace(d), f"{shape} cells are beyond gg_field_distance's limits",
                         dev)
    _lib.check(lib.gg_field_distance_known(d, _ptr(mass), int(threshold), _ptr(seen), int(min_views), _ptr(out),
                                           _ptr(ws), ws.numel(), _stream(dev)), "gg_field_distance_known")
    return out


def paths(dist2: Tensor, grid, dims, poses: Tensor, spheres: Tensor, need: Tensor,
          outside: int = FAR) -> Tuple[Tensor, Tensor]:
    """(slack (P, W) int32, first_hit (P,) int32) of one gg_field_paths call.  poses (P, W, 12) and spheres (S, 3)
    float32, need (S,) int32 in 0..FAR, dist2 int32 [X][Y][Z]: on the HIP device (no CPU path)."""
    dev = _require_hip(dist2, poses, spheres, need)
    d, g, shape = volume_args(dims, grid)
    volume_tensor(dist2, "dist2", torch.int32, shape)
    poses = pose_paths(poses)
    spheres, need = sphere_table(spheres, need=need)
    p, w = poses.shape[:2]
    if p * w > MAX_POSES:
        raise ValueError(f"{p} x {w} poses are more than {MAX_POSES}")
    slack = torch.empty(p, w, dtype=torch.int32, device=dev)
    first = torch.empty(p, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_field_paths(d, g, _ptr(dist2), p, w, _ptr(poses), spheres.shape[0], _ptr(spheres),
                                          _ptr(need), cell_count("outside", outside), _ptr(slack), _ptr(first),
                                          _stream(dev)), "gg_field_paths")
    return slack, first


# ------------------------------------------------------------------------------------------------
# the volume
# ------------------------------------------------------------------------------------------------
@torch.no_grad()
def model_gaussians(model_or_scene, mask: Optional[Tensor] = None):
    """(means, rot, scales, weights) of a model or scene as gg_field_splat takes them, built the way
    grasp.model_points builds its inputs: ops.quat_to_rotmat, exp(scales), sigmoid(opacities) times `mask`."""
    from . import ops
    means, quats = model_or_scene.means.detach(), model_or_scene.quats.detach()
    scales, opac = model_or_scene.scales.detach(), model_or_scene.opacities.detach()
    _require_hip(means, quats, scales, opac)
    rot = ops.quat_to_rotmat(quats.float()).reshape(-1, 9).contiguous()
    weights = torch.sigmoid(opac.float()).reshape(-1)
    if mask is not None:
        mask = mask.reshape(-1)
        if mask.shape[0] != weights.shape[0]:
            raise ValueError(f"mask has {mask.shape[0]} entries for {weights.shape[0]} Gaussians")
        weights = weights * mask.to(device=weights.device, dtype=torch.float32)
    return means.float().contiguous(), rot, torch.exp(scales.float()).contiguous(), weights.contiguous()


class DistanceField:
    """Occupancy mass and squared distances of the scene inside a box: `mass` int64 and `dist2` int32 [X][Y][Z] on
    the HIP device, `grid` (4,) float64 lower corner and cell edge, `dims` (3,) int32.  add / remove change the mass
    (integer votes: removing what was added restores it bit for bit), update() recomputes dist2 from it."""

    def __init__(self, bbox_min: Sequence[float], bbox_max: Sequence[float], voxel: float = VOXEL, device=None):
        self.grid, self.dims = field_grid(bbox_min, bbox_max, voxel)
        dev = default_device("field") if device is None else torch.device(device)
        shape = tuple(int(d) for d in self.dims)
        self.mass = torch.zeros(shape, dtype=torch.int64, device=dev)
        self.dist2 = torch.full(shape, FAR, dtype=torch.int32, device=dev)
        self.threshold = THRESHOLD
        self.seen: Optional[Tensor] = None       # uint16 [X][Y][Z]: views that saw the cell free; None: no observe yet
        self.looked: Optional[Tensor] = None     # uint16 [X][Y][Z]: views that had the cell in their image

    @property
    def h(self) -> float:
        return float(self.grid[3])

    def add(self, source, mask: Optional[Tensor] = None, extent: float = EXTENT, max_reach: int = MAX_REACH,
            min_weight: float = MIN_WEIGHT, sign: int = 1) -> SplatCounts:
        """Adds the votes of a model or scene (model_gaussians, times `mask`), or of a tuple (means, rot, scales,
        weights) of device tensors, to the mass.  dist2 is stale until update()."""
        if isinstance(source, (tuple, list)):
            means, rot, scales, weights = source
            if mask is not None:
                weights = weights * mask.reshape(-1).to(device=weights.device, dtype=torch.float32)
        else:
            means, rot, scales, weights = model_gaussians(source, mask)
        return splat(self.mass, self.grid, self.dims, means, rot, scales, weights, extent, max_reach, min_weight, sign)

    def remove(self, source, mask: Optional[Tensor] = None, extent: float = EXTENT, max_reach: int = MAX_REACH,
               min_weight: float = MIN_WEIGHT) -> SplatCounts:
        """add with sign -1: takes out exactly what the same call of add put in."""
        return self.add(source, mask, extent, max_reach, min_weight, sign=-1)

    def update(self, threshold: Optional[int] = None, unknown: str = "free",
               min_views: int = OBSERVE_MIN_VIEWS) -> "DistanceField":
        """dist2 from the mass.  unknown "free" (the default): a cell without mass is free, seen or not.  "blocked":
        a cell that fewer than min_views views have seen free is an obstacle too (gg_field_distance_known), so every
        reader of dist2 keeps clear of space no camera saw; it needs observe() or assume_free() first.  The robot's
        own envelope is seen by no camera: assume_free it, or "blocked" rejects every start configuration."""
        if unknown not in ("free", "blocked"):
            raise ValueError(f"unknown must be 'free' or 'blocked', got {unknown!r}")
        if threshold is not None:
            self.threshold = int(threshold)
        if unknown == "free":
            distance(self.mass, self.dims, self.threshold, out=self.dist2)
        else:
            if self.seen is None:
                raise ValueError("update(unknown='blocked') before anything was observed: call observe(), "
                                 "observe_scan(), observe_model() or assume_free() first")
            distance_known(self.mass, self.seen, self.dims, self.threshold, min_views, out=self.dist2)
        return self

    # ---- known free space ----------------------------------------------------------------------------------------
    def _counters(self) -> None:
        if self.seen is None:
            self.seen = torch.zeros_like(self.mass, dtype=torch.uint16)
            self.looked = torch.zeros_like(self.mass, dtype=torch.uint16)

    def observe(self, depth, intrinsics: ArrayLike, c2w: Optional[ArrayLike] = None, w2c: Optional[ArrayLike] = None,
                margin: float = OBSERVE_MARGIN, near: float = OBSERVE_NEAR, batch: int = 16) -> "DistanceField":
        """Counts, per cell, the frames that saw the whole cell free (self.seen) and that had it in their image
        (self.looked); both are allocated on first use, and a later call with new frames adds to them.  depth (V, H,
        W) or (H, W): along the camera's z axis in scene units (> 0 a reading, +inf free space to infinity, 0 /
        negative / NaN no reading); intrinsics (V, 4) fx, fy, cx, cy; the poses either as w2c (V, 3, 4) OpenCV
        world-to-camera or as c2w (V, 3|4, 4) nerfstudio / OpenGL camera-to-world (mesh.opencv_w2c), as the rest of the
        library passes them.  The pyramid is built per `batch` frames.  dist2 is stale until update()."""
        if (c2w is None) == (w2c is None):
            raise ValueError("give exactly one of c2w (OpenGL camera-to-world) and w2c (OpenCV world-to-camera)")
        if int(batch) < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        if w2c is None:
            from .mesh import opencv_w2c
            w2c = opencv_w2c(c2w)
        dev = self.mass.device
        d = depth.detach() if isinstance(depth, Tensor) else torch.as_tensor(np.asarray(depth))
        d = d[None] if d.ndim == 2 else d
        if d.ndim != 3:
            raise ValueError(f"depth must be (V, H, W) or (H, W), got {tuple(d.shape)}")
        k, e = camera_arrays(intrinsics, w2c, d.shape[0])
        radius, margin, near = cell_ball(self.h), nonneg("margin", margin), positive("near", near)
        h, w = _frame_size(d.shape[1], d.shape[2])
        _require_hip(self.mass)                          # before the counters exist: a refused call leaves no trace
        self._counters()
        for b0 in range(0, d.shape[0], int(batch)):
            part = d[b0:b0 + int(batch)].to(device=dev, dtype=torch.float32).contiguous()
            observe(self.seen, self.looked, self.grid, self.dims, depth_pyramid(part), k[b0:b0 + int(batch)],
                    e[b0:b0 + int(batch)], h, w, radius, margin, near)
        return self

    def observe_scan(self, scan_dir: str, depth_units_per_metre: float = 1.0, margin: float = OBSERVE_MARGIN,
                     near: float = OBSERVE_NEAR, batch: int = 16, transform=None) -> "DistanceField":
        """observe() of the raw RGB-D frames of a scan directory (mesh.scan_frames): sensor depth, the better evidence
        of the two sources.  The frames are in the scan's raw frame.  transform: (matrix, scale) of the dataparser
        (frames.load_transform_json) when the volume is in a checkpoint's frame: the poses go through
        frames.c2w_to_scene and the depth is multiplied by scale."""
        from .frames import c2w_to_scene
        from .mesh import scan_frames
        buf = []

        def flush():
            if buf:
                self.observe(np.stack([b[0] for b in buf]), np.stack([b[1] for b in buf]),
                             w2c=np.linalg.inv(np.stack([b[2] for b in buf]))[:, :3, :], margin=margin, near=near,
                             batch=batch)
                buf.clear()

        for depth, _, intr, c2w_cv in scan_frames(scan_dir, depth_units_per_metre):
            if transform is not None:
                c2w_cv, depth = c2w_to_scene(c2w_cv, *transform), depth * np.float32(transform[1])
            if buf and buf[0][0].shape != depth.shape:
                flush()
            buf.append((depth, intr, c2w_cv))
            if len(buf) == int(batch):
                flush()
        flush()
        return self

    def observe_model(self, model, cameras, downscale: float = 1.0, depth_mode: str = "median",
                      margin: float = OBSERVE_MARGIN, near: float = OBSERVE_NEAR, batch: int = 16) -> "DistanceField":
        """observe() of depth rendered from the model (mesh.render_depth) at every camera (c2w OpenGL (3|4, 4) IN THE
        MODEL'S FRAME, intrinsics fx, fy, cx, cy, height, width: what lift.scene_cameras makes of a scan's
        transforms.json and the dataparser's transform; mesh.transforms_cameras alone returns OpenCV poses in the
        scan's raw frame, which are NOT these), at 1 / downscale of its size.  RENDERED DEPTH IS EVIDENCE ONLY FROM
        CAMERAS THE MODEL WAS TRAINED ON: from anywhere else the model shows free space where it merely has no
        Gaussians, which is the assumption this state exists to remove.  Sensor depth (observe_scan) is the better
        source.  depth_mode "median" gives the depth of a real Gaussian where two surfaces share a pixel."""
        from .mesh import _scaled_intrinsics, check_depth_mode, homogeneous, render_depth
        check_depth_mode(depth_mode)
        if not float(downscale) > 0:
            raise ValueError(f"downscale must be > 0, got {downscale}")
        by_size = {}
        for c2w, K, h, w in cameras:
            Ks, hs, ws = _scaled_intrinsics(np.asarray(K, dtype=np.float64).reshape(4), int(h), int(w), downscale)
            by_size.setdefault((hs, ws), []).append((homogeneous(c2w), Ks))
        for (hs, ws), group in by_size.items():
            for b0 in range(0, len(group), int(batch)):
                part = group[b0:b0 + int(batch)]
                depth = torch.stack([render_depth(model, c, K, hs, ws, depth_mode=depth_mode)[0] for c, K in part])
                self.observe(depth, np.stack([K for _, K in part]), c2w=np.stack([c for c, _ in part]), margin=margin,
                             near=near, batch=batch)
        return self

    def assume_free(self, bbox_min: Sequence[float], bbox_max: Sequence[float]) -> "DistanceField":
        """Declares the cells whose centres lie in the closed box known free: their `seen` saturates (their mass still
        blocks them).  For the robot's own envelope, which no camera sees: without it update(unknown="blocked")
        blocks the arm's base and every start configuration with it.  This is the caller's knowledge, not the
        sensor's: the box is taken on trust."""
        lo, hi = np.asarray(bbox_min, np.float64).reshape(-1), np.asarray(bbox_max, np.float64).reshape(-1)
        if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()
                                                        and (hi >= lo).all()):
            raise ValueError(f"bbox_min / bbox_max must be finite (3,) with min <= max, got {lo} / {hi}")
        self._counters()
        inside = []
        for a in range(3):
            c = self.grid[a] + (np.arange(int(self.dims[a]), dtype=np.float64) + 0.5) * self.h
            inside.append(torch.from_numpy((c >= lo[a]) & (c <= hi[a])).to(self.seen.device))
        box = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
        self.seen.view(torch.int16).masked_fill_(box, -1)        # 0xffff: SEEN_MAX (torch has few uint16 operators)
        return self

    def knowledge(self, min_views: int = OBSERVE_MIN_VIEWS) -> dict:
        """The cells of each state as ints: occupied (mass >= threshold), free (not occupied, seen >= min_views),
        occluded (neither, but some view had the cell in its image) and unseen (no view ever had)."""
        occupied = self.mass >= self.threshold
        if self.seen is None:
            n = int(occupied.sum())
            return {"occupied": n, "free": 0, "occluded": 0, "unseen": int(occupied.numel()) - n}
        free = ~occupied & (self.seen.to(torch.int32) >= int(min_views))
        occluded = ~occupied & ~free & (self.looked.to(torch.int32) > 0)
        n, f, o = int(occupied.sum()), int(free.sum()), int(occluded.sum())
        return {"occupied": n, "free": f, "occluded": o, "unseen": int(occupied.numel()) - n - f - o}

    def distance(self) -> Tensor:
        """sqrt(dist2) h as float32, in scene units between cell centres; inf where dist2 is FAR."""
        d = torch.sqrt(self.dist2.to(torch.float64)) * self.h
        return torch.where(self.dist2 >= FAR, torch.full_like(d, math.inf), d).float()

    def save(self, path: str) -> None:
        known = {} if self.seen is None else {"seen": self.seen.cpu().numpy(), "looked": self.looked.cpu().numpy()}
        np.savez_compressed(path, mass=self.mass.cpu().numpy(), dist2=self.dist2.cpu().numpy(), grid=self.grid,
                            dims=self.dims, threshold=np.int64(self.threshold), **known)

    @classmethod
    def load(cls, path: str, device=None) -> "DistanceField":
        with np.load(path) as z:
            grid, dims = np.asarray(z["grid"], np.float64), np.asarray(z["dims"], np.int32)
            mass, dist2, thr = z["mass"], z["dist2"], int(z["threshold"])
            seen, looked = (z[n] if n in z.files else None for n in ("seen", "looked"))
        shape = tuple(int(d) for d in dims)
        if grid.shape != (4,) or dims.shape != (3,) or mass.shape != shape or dist2.shape != shape:
            raise ValueError(f"{path}: not a distance field (grid {grid.shape}, dims {dims.shape}, mass {mass.shape})")
        if (seen is None) != (looked is None) or (seen is not None and (seen.shape != shape or looked.shape != shape)):
            raise ValueError(f"{path}: seen and looked travel together, shaped like the mass")
        f = cls.__new__(cls)
        dev = default_device("field") if device is None else torch.device(device)
        f.grid, f.dims, f.threshold = grid, dims, thr
        f.mass = torch.from_numpy(mass.astype(np.int64)).to(dev)
        f.dist2 = torch.from_numpy(dist2.astype(np.int32)).to(dev)
        f.seen = None if seen is None else torch.from_numpy(seen.astype(np.uint16)).to(dev)
        f.looked = None if looked is None else torch.from_numpy(looked.astype(np.uint16)).to(dev)
        return f


def path_clear(field: DistanceField, poses: ArrayLike, spheres: ArrayLike, radius: Union[float, ArrayLike],
               margin: float = 0.0, outside: str = "free") -> PathClearance:
    """Every path's waypoints against field.dist2 (update() first): poses (P, W, 12), spheres (S, 3) gripper-frame
    centres of `radius` (one number or (S,)), kept `margin` away from every occupied cell (need2).  outside: what a
    sphere centre outside the volume counts as, "free" or "blocked"."""
    if outside not in ("free", "blocked"):
        raise ValueError(f"outside must be 'free' or 'blocked', got {outside!r}")
    dev = field.dist2.device
    sp = to_device(spheres, torch.float32, dev).reshape(-1, 3)
    need = need2(np.broadcast_to(np.asarray(radius, np.float64), (sp.shape[0],)), margin, field.h)
    p = to_device(poses, torch.float32, dev)
    slack, first = paths(field.dist2, field.grid, field.dims, p, sp, torch.from_numpy(need).to(dev),
                         FAR if outside == "free" else 0)
    return PathClearance(slack, first, first == p.shape[1])


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def main(argv: Optional[Sequence[str]] = None) -> int:
    from ._cli import (add_gripper_sphere_options, add_object_options, check_object_options, load_scene,
                       object_mask)
    from .frames import load_transform_json
    from .grasp import load_gripper_option
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.field",
                                 description="Distance field of a checkpoint's Gaussians inside a box and, with "
                                             "--paths, the clearance of gripper paths through it.")
    ap.add_argument("--ckpt", required=True, help="step-*.ckpt of a splatting model")
    ap.add_argument("--bbox", type=float, nargs=6, required=True, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="the box, scene frame")
    ap.add_argument("--voxel", type=float, default=VOXEL, help="cell edge, scene units")
    ap.add_argument("--extent", type=float, default=EXTENT, help="a Gaussian occupies its k-sigma ellipsoid")
    ap.add_argument("--max-reach", type=int, default=MAX_REACH, help="cells a Gaussian may reach from its mean's cell")
    ap.add_argument("--min-opacity", type=float, default=MIN_WEIGHT, help="a Gaussian takes part above it")
    ap.add_argument("--occupied", type=float, default=THRESHOLD / VOTE_ONE,
                    help="a cell is occupied from this much opacity mass on")
    ap.add_argument("--transform-json", default=None, help="JSON with transform_matrix and scale (world -> scene)")
    add_object_options(ap, "the selected Gaussians are LEFT OUT of the field (the object being carried)",
                       "selects the Gaussians that are left out of the field (the object being carried)")
    ap.add_argument("--out", required=True, help="output .npz: mass, dist2, grid, dims, threshold (seen, looked)")
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--observe-scan", default=None, metavar="DIR",
                     help="known free space from the raw RGB-D frames of a scan directory, brought into the checkpoint's "
                          "frame by --transform-json")
    src.add_argument("--observe-transforms", default=None, metavar="T.json",
                     help="known free space from depth rendered at the cameras of the scan's transforms.json (OpenCV "
                          "c2w, raw frame; --transform-json brings them into the checkpoint's): evidence only from "
                          "cameras the model was trained on")
    ap.add_argument("--observe-downscale", type=float, default=1.0, help="with --observe-transforms: render smaller")
    ap.add_argument("--observe-margin", type=float, default=OBSERVE_MARGIN,
                    help="the surface must lie this far beyond every point of a cell")
    ap.add_argument("--observe-near", type=float, default=OBSERVE_NEAR, help="nearest camera depth a view speaks for")
    ap.add_argument("--min-views", type=int, default=OBSERVE_MIN_VIEWS, help="views that must have seen a cell free")
    ap.add_argument("--unknown", choices=("free", "blocked"), default="free",
                    help="what a cell that was not seen free counts as")
    ap.add_argument("--assume-free", type=float, nargs=6, action="append", default=[],
                    metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="a box taken as known free (the robot's own envelope); repeatable")
    ap.add_argument("--paths", default=None, help=".npy (P, W, 12) gripper poses, scene frame: R row-major, then t")
    add_gripper_sphere_options(ap, "with --paths: ")
    ap.add_argument("--outside", choices=("free", "blocked"), default="free",
                    help="with --paths: what space outside the box counts as")
    ap.add_argument("--report", default=None, help="with --paths: output .npz slack, first_hit, clear, spheres")
    a = ap.parse_args(argv)
    check_object_options(ap, a, "optional")
    if bool(a.paths) != bool(a.gripper) or bool(a.paths) != bool(a.report):
        ap.error("--paths, --gripper and --report go together")
    check_finite_options(ap, a, positive=("voxel", "radius", "width", "observe_near", "observe_downscale"),
                         nonneg=("extent", "margin", "depth", "height", "observe_margin"))
    if not 1 <= a.min_views <= SEEN_MAX:
        ap.error(f"--min-views must be in 1..{SEEN_MAX}, got {a.min_views}")
    observed = bool(a.observe_scan or a.observe_transforms or a.assume_free)
    if a.unknown == "blocked" and not observed:
        ap.error("--unknown blocked needs --observe-scan, --observe-transforms or --assume-free")
    if not 0 <= a.max_reach <= MAX_REACH_LIMIT:
        ap.error(f"--max-reach must be in 0..{MAX_REACH_LIMIT}, got {a.max_reach}")
    if math.isnan(a.min_opacity):
        ap.error("--min-opacity must not be NaN")
    if not (math.isfinite(a.occupied) and 1 <= math.trunc(a.occupied * VOTE_ONE) < 2 ** 62):
        ap.error(f"--occupied must be at least 2^-16, got {a.occupied}")
    try:
        grid, dims = field_grid(a.bbox[:3], a.bbox[3:], a.voxel)
        spheres = poses = None
        if a.paths:
            spheres = gripper_spheres(load_gripper_option(a.gripper), a.width, a.depth, a.height, a.radius)
            poses = np.asarray(np.load(a.paths), np.float32)
            if poses.ndim != 3 or poses.shape[2] != 12:
                raise ValueError(f"{a.paths}: expected (P, W, 12) poses, got {poses.shape}")
        matrix, scale = load_transform_json(a.transform_json) if a.transform_json else (None, 1.0)
        scene, mlp_state = load_scene(a.ckpt)
        carried = object_mask(a, scene, mlp_state, matrix, scale)
        field = DistanceField(a.bbox[:3], a.bbox[3:], a.voxel)
        counts = field.add(scene, None if carried is None else ~carried.bool(), a.extent, a.max_reach, a.min_opacity)
        if a.observe_scan:
            field.observe_scan(a.observe_scan, margin=a.observe_margin, near=a.observe_near,
                               transform=(matrix, scale) if a.transform_json else None)
        if a.observe_transforms:       # OpenCV poses of the scan's raw frame -> OpenGL poses of the checkpoint's
            from .lift import scene_cameras
            field.observe_model(scene, scene_cameras(a.observe_transforms, a.transform_json)[0], a.observe_downscale,
                                margin=a.observe_margin, near=a.observe_near)
        for box in a.assume_free:
            field.assume_free(box[:3], box[3:])
        field.update(math.trunc(a.occupied * VOTE_ONE), a.unknown, a.min_views)
        field.save(a.out)
        line = (f"{tuple(int(d) for d in dims)} cells, {int((field.mass >= field.threshold).sum())} occupied; "
                f"{int(counts.skipped)} Gaussians took no part, {int(counts.truncated)} were cut by --max-reach; "
                f"wrote {a.out}")
        if observed:
            k = field.knowledge(a.min_views)
            line += (f"; known free {k['free']}, occluded {k['occluded']}, never looked at {k['unseen']} "
                     f"(unknown counts as {a.unknown})")
        if a.paths:
            res = path_clear(field, poses, spheres, a.radius, a.margin, a.outside)
            np.savez(a.report, slack=res.slack.cpu().numpy(), first_hit=res.first_hit.cpu().numpy(),
                     clear=res.clear.cpu().numpy(), spheres=spheres)
            line += f"; {int(res.clear.sum())} of {poses.shape[0]} paths clear, wrote {a.report}"
    except (KeyError, ValueError, OSError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
