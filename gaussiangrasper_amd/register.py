"""Registration of coloured point clouds: the reference's coloricp (scripts/generate_data.py:47-83, Open3D's
coloured ICP after Park, Zhou, Koltun 2017) restated.  Two HIP calls (`gg_cloud_frames` and `gg_icp_step`,
csrc/register.hip); the contract is in include/gg_raster.h and PARITY.md "Registration", the design in DESIGN.md
§3.19.

    voxel_downsample    mean position and colour per occupied voxel (torch, any device)
    cloud_frames        normals, colour gradients, neighbour counts and validity of a target cloud (IcpTarget)
    icp_step            one Gauss-Newton linearisation of a source against a target (IcpSums)
    solve_step          the 6 x 6 solve and the pose update, numpy fp64 on the host
    colored_icp         the three-scale loop (RegistrationResult)
    refine_scan_poses   frame-to-model registration of a scan's frames (ScanRefinement)
    python -m gaussiangrasper_amd.register --source a.npy --target b.npy [--init T.json] --out T.json

No GPU work falls back to the host: a missing device is an error."""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (ArrayLike, default_device, f32_rows, grid_args, host_ptr, positive, ptr as _ptr,
                    require_hip as _require_hip, sized_workspace, stream as _stream, to_device)
from .frames import homogeneous, rigid_rows
from .grid import cluster_grid

VOXEL_RADIUS = (0.02, 0.01, 0.005)     # coloricp :62
MAX_ITER = (30, 20, 10)                # coloricp :63
LAMBDA_GEOMETRIC = 0.968               # Open3D's default, recalled (PARITY.md "Registration")
RELATIVE_FITNESS = RELATIVE_RMSE = 1e-6   # coloricp :77-78
FRAME_RADIUS_FACTOR = 2.0              # normals at twice the voxel size, coloricp :71
MIN_FITNESS = 0.3                      # refine_scan_poses: this project's choices
MAX_CORRECTION = (0.05, 0.1)           # metres, radians
MAX_POINTS = 1 << 30                   # GG_REGISTER_MAX_POINTS
NUM_SUMS = 32
_TRIU = [(i, j) for i in range(6) for j in range(i, 6)]


# ------------------------------------------------------------------------------------------------
# voxel grid (torch; not the hot path)
# ------------------------------------------------------------------------------------------------
def voxel_downsample(points: Tensor, colors: Optional[Tensor], voxel: float) -> Tuple[Tensor, Optional[Tensor]]:
    """Mean position and colour of the points of every occupied voxel, in fp64, ordered by voxel key.  The voxel of
    p is floor((p - (min - voxel / 2)) / voxel) per axis, min the cloud's lower corner (Open3D's origin, recalled);
    the key is (ix ny + iy) nz + iz.  points (N, 3), colors (N, C) or None, on any device; rows with a non-finite
    coordinate are dropped.  The sums are index_add_'s, whose order on a device is not fixed: last bits may differ
    from call to call."""
    voxel = positive("voxel", voxel)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (N, 3), got {tuple(points.shape)}")
    if colors is not None and (colors.ndim != 2 or colors.shape[0] != points.shape[0]):
        raise ValueError(f"colors must be (N, C) with N = {points.shape[0]}, got {tuple(colors.shape)}")
    p = points.detach().to(torch.float64)
    keep = torch.isfinite(p).all(dim=1)
    p = p[keep]
    c = None if colors is None else colors.detach().to(torch.float64)[keep]
    if p.shape[0] == 0:
        return p, c
    lo = p.min(dim=0).values - 0.5 * voxel
    idx = torch.floor((p - lo) / voxel).to(torch.int64)
    dims = idx.max(dim=0).values + 1
    if float(dims[0]) * float(dims[1]) * float(dims[2]) >= 2.0 ** 62:
        raise ValueError(f"a voxel of {voxel} gives {dims.tolist()} cells: too many")
    key = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
    _, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    k = cnt.shape[0]
    w = cnt.to(torch.float64)[:, None]
    out_p = torch.zeros((k, 3), dtype=torch.float64, device=p.device).index_add_(0, inv, p) / w
    out_c = None
    if c is not None:
        out_c = torch.zeros((k, c.shape[1]), dtype=torch.float64, device=p.device).index_add_(0, inv, c) / w
    return out_p, out_c


# ------------------------------------------------------------------------------------------------
# device calls
# ------------------------------------------------------------------------------------------------
@dataclass
class IcpTarget:
    """A target cloud with gg_cloud_frames' outputs; N points, all on one HIP device."""
    points: Tensor             # (N, 3) float32
    intensity: Tensor          # (N,) float32
    normals: Tensor            # (N, 3) float32: NaN where valid is 0
    gradients: Tensor          # (N, 3) float32
    count: Tensor              # (N,) int32: neighbours within the radius, the point itself included
    valid: Tensor              # (N,) uint8
    radius: float


@dataclass
class IcpSums:
    """gg_icp_step's sums on the host, for M source points."""
    sums: np.ndarray                       # (32,) float64
    num_source: int
    abs_sums: Optional[np.ndarray] = None  # (32,) float64
    corr: Optional[Tensor] = None          # (M,) int32 on the device

    @property
    def jtj(self) -> np.ndarray:
        a = np.zeros((6, 6))
        for o, (i, j) in enumerate(_TRIU):
            a[i, j] = a[j, i] = self.sums[o]
        return a

    @property
    def jtr(self) -> np.ndarray:
        return np.array(self.sums[21:27])

    @property
    def inliers(self) -> int:
        return int(self.sums[27])

    @property
    def fitness(self) -> float:
        return self.sums[27] / self.num_source

    @property
    def inlier_rmse(self) -> float:
        return math.sqrt(self.sums[28] / self.sums[27]) if self.sums[27] > 0 else 0.0


class StepWorkspace:
    """gg_icp_step's workspace kept between the steps of one scale, so that the target is sorted once."""

    def __init__(self):
        self.ws: Optional[Tensor] = None
        self.key = None
        self.grid = None


def cloud_frames(points: Tensor, intensity: Tensor, radius: float, grid=None) -> IcpTarget:
    """Surface frames of `points` (N, 3) float32 with `intensity` (N,) float32 on the HIP device (gg_cloud_frames):
    per point the neighbours within `radius`, the normal of their covariance and the colour gradient in the tangent
    plane.  `grid`: (grid, dims) as cluster.cluster_grid returns (None: fitted here, which reads a sample back)."""
    radius = positive("radius", radius)
    dev = _require_hip(points, intensity)
    points = f32_rows(points, "points", 3)
    intensity = f32_rows(intensity, "intensity", None)
    n = points.shape[0]
    if intensity.shape[0] != n or not 1 <= n <= MAX_POINTS:
        raise ValueError(f"points has {n} rows (1 .. 2^30 wanted), intensity {intensity.shape[0]}")
    grid_c, dims_c = grid_args(cluster_grid(points, radius) if grid is None else grid)
    res = IcpTarget(points=points, intensity=intensity,
                    normals=torch.empty((n, 3), dtype=torch.float32, device=dev),
                    gradients=torch.empty((n, 3), dtype=torch.float32, device=dev),
                    count=torch.empty(n, dtype=torch.int32, device=dev),
                    valid=torch.empty(n, dtype=torch.uint8, device=dev), radius=radius)
    lib = _lib.load()
    ws = sized_workspace(lib.gg_cloud_frames_workspace(n, dims_c), f"{n} points on a grid of {list(dims_c)} cells is "
                         f"beyond gg_cloud_frames' limits", dev)
    _lib.check(lib.gg_cloud_frames(n, _ptr(points), _ptr(intensity), radius, host_ptr(grid_c), host_ptr(dims_c),
                                   _ptr(res.normals), _ptr(res.gradients), _ptr(res.count), _ptr(res.valid), _ptr(ws),
                                   ws.numel(), _stream(dev)), "gg_cloud_frames")
    return res


def icp_step(source: Tensor, source_intensity: Tensor, target: IcpTarget, transform: ArrayLike, max_dist: float,
             lambda_geometric: float = LAMBDA_GEOMETRIC, corr: bool = False, abs_sums: bool = False,
             grid=None, state: Optional[StepWorkspace] = None) -> IcpSums:
    """One Gauss-Newton linearisation (gg_icp_step) of `source` (M, 3) float32 with `source_intensity` (M,) float32
    against `target` under `transform` ((3, 4) or (4, 4), source to target): the 32 sums, read back.  `corr` /
    `abs_sums`: also return the correspondences (device) / the sums of absolute values.  `state`: a StepWorkspace
    shared by the steps of one target and max_dist; the target is then sorted by the first of them only."""
    max_dist = positive("max_dist", max_dist)
    lam = float(lambda_geometric)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_geometric must be in [0, 1], got {lambda_geometric}")
    dev = _require_hip(source, source_intensity, target.points)
    source = f32_rows(source, "source", 3)
    source_intensity = f32_rows(source_intensity, "source_intensity", None)
    m, n = source.shape[0], target.points.shape[0]
    if source_intensity.shape[0] != m or not 1 <= m <= MAX_POINTS:
        raise ValueError(f"source has {m} rows (1 .. 2^30 wanted), source_intensity {source_intensity.shape[0]}")
    rows = rigid_rows(transform, np.float64)
    if not np.isfinite(rows).all():
        raise ValueError("transform must be finite")
    lib = _lib.load()
    key = (id(target), max_dist)
    reuse = state is not None and state.key == key and state.ws is not None
    if reuse:
        grid_c, dims_c = state.grid
    else:
        grid_c, dims_c = grid_args(cluster_grid(target.points, max_dist, target.valid) if grid is None else grid)
    nbytes = lib.gg_icp_step_workspace(m, n, dims_c)
    reuse = reuse and 0 < nbytes <= state.ws.numel()
    ws = state.ws if reuse else sized_workspace(nbytes, f"{m} source and {n} target points on a grid of "
                                                f"{list(dims_c)} cells is beyond gg_icp_step's limits", dev)
    out = torch.empty((2 if abs_sums else 1, NUM_SUMS), dtype=torch.float64, device=dev)
    cor = torch.empty(m, dtype=torch.int32, device=dev) if corr else None
    _lib.check(lib.gg_icp_step(m, _ptr(source), _ptr(source_intensity), n, _ptr(target.points),
                               _ptr(target.intensity), _ptr(target.normals), _ptr(target.gradients),
                               _ptr(target.valid), host_ptr(grid_c), host_ptr(dims_c), host_ptr(rows), max_dist, lam,
                               1 if reuse else 0, _ptr(out[0]), _ptr(out[1]) if abs_sums else None, _ptr(cor),
                               _ptr(ws), ws.numel(), _stream(dev)), "gg_icp_step")
    if state is not None:
        state.ws, state.key, state.grid = ws, key, (grid_c, dims_c)
    host = out.cpu().numpy()
    return IcpSums(sums=host[0], num_source=m, abs_sums=host[1] if abs_sums else None, corr=cor)


# ------------------------------------------------------------------------------------------------
# host side
# ------------------------------------------------------------------------------------------------
def rodrigues(w: ArrayLike) -> np.ndarray:
    """The rotation matrix exp([w]x) of a rotation vector, fp64."""
    w = np.asarray(w, dtype=np.float64).reshape(3)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)


def solve_step(sums, transform: ArrayLike) -> Tuple[np.ndarray, bool]:
    """x = solve(J^T J, -J^T r), x = [omega, v], then T <- [Rodrigues(omega) | v] T.  `sums`: an IcpSums or its 32
    numbers.  Returns (T' (4, 4) fp64, True), or (T, False) when the system is singular or not finite."""
    s = sums if isinstance(sums, IcpSums) else IcpSums(np.asarray(sums, dtype=np.float64).reshape(NUM_SUMS), 1)
    T = homogeneous(transform)
    A, b = s.jtj, s.jtr
    if not (np.isfinite(A).all() and np.isfinite(b).all()) or np.linalg.matrix_rank(A) < 6:
        return T, False
    x = np.linalg.solve(A, -b)
    if not np.isfinite(x).all():
        return T, False
    U = np.eye(4)
    U[:3, :3] = rodrigues(x[:3])
    U[:3, 3] = x[3:]
    return U @ T, True


@dataclass
class RegistrationResult:
    transformation: np.ndarray             # (4, 4) float64, source to target
    fitness: float                         # source points with a correspondent / source points, finest scale
    inlier_rmse: float                     # root mean squared distance of those
    iterations: List[int]                  # pose updates per scale
    status: List[str] = field(default_factory=list)   # per scale: "converged", "max_iter" or "singular"


def _cloud(x: ArrayLike, dev, cols: Optional[int] = 3) -> Tensor:
    t = to_device(x, torch.float64, dev)
    if t.ndim != 2 or t.shape[1] != cols:
        raise ValueError(f"expected an (N, {cols}) array, got {tuple(t.shape)}")
    return t


def colored_icp(source: ArrayLike, source_colors: Optional[ArrayLike], target: ArrayLike,
                target_colors: Optional[ArrayLike], init: Optional[ArrayLike] = None,
                voxel_radius: Sequence[float] = VOXEL_RADIUS, max_iter: Sequence[int] = MAX_ITER,
                lambda_geometric: float = LAMBDA_GEOMETRIC, scale: float = 1.0) -> RegistrationResult:
    """The reference's coloricp: multi-scale coloured ICP of `source` (M, 3) onto `target` (N, 3), colours (., 3) in
    [0, 1], from the source-to-target guess `init` (default identity).  Per scale both clouds are voxel-downsampled
    at the voxel size, the target's frames are computed at twice that, and the pose is updated until the fitness and
    the inlier rmse both change by less than 1e-6 or max_iter updates are done; correspondences reach one voxel
    size.  `scale` multiplies the voxel sizes for clouds that are not in metres.  Without colours (both None)
    lambda_geometric must be 1: plain point-to-plane ICP.  One 32-double read-back per iteration."""
    if len(voxel_radius) != len(max_iter) or not len(voxel_radius):
        raise ValueError("voxel_radius and max_iter must have the same, non-zero length")
    scale = positive("scale", scale)
    lam = float(lambda_geometric)
    if (source_colors is None) != (target_colors is None):
        raise ValueError("give both clouds' colours or neither's")
    if source_colors is None and lam != 1.0:
        raise ValueError("registration without colours needs lambda_geometric = 1")
    dev = source.device if isinstance(source, Tensor) and source.device.type == "cuda" else default_device("register")
    src, tgt = _cloud(source, dev), _cloud(target, dev)
    src_c = None if source_colors is None else _cloud(source_colors, dev)
    tgt_c = None if target_colors is None else _cloud(target_colors, dev)
    T = np.eye(4) if init is None else homogeneous(init).copy()
    iters, status = [], []
    last = None
    for v, n_it in zip(voxel_radius, max_iter):
        v = positive("voxel_radius", v) * scale
        s, sc = voxel_downsample(src, src_c, v)
        p, pc = voxel_downsample(tgt, tgt_c, v)
        if s.shape[0] == 0 or p.shape[0] == 0:
            raise ValueError("a cloud has no finite point")
        i_s = torch.zeros(s.shape[0], device=dev) if sc is None else sc.mean(dim=1).float()
        i_p = torch.zeros(p.shape[0], device=dev) if pc is None else pc.mean(dim=1).float()
        s = s.float().contiguous()
        frames = cloud_frames(p.float().contiguous(), i_p.contiguous(), FRAME_RADIUS_FACTOR * v)
        state, prev, k = StepWorkspace(), None, 0
        while True:
            last = icp_step(s, i_s, frames, T, v, lam, state=state)
            fit, rmse = last.fitness, last.inlier_rmse
            if prev is not None and abs(prev[0] - fit) < RELATIVE_FITNESS and abs(prev[1] - rmse) < RELATIVE_RMSE:
                status.append("converged")
                break
            if k == int(n_it):
                status.append("max_iter")
                break
            prev = (fit, rmse)
            T, ok = solve_step(last, T)
            if not ok:
                status.append("singular")
                break
            k += 1
        iters.append(k)
    return RegistrationResult(transformation=T, fitness=float(last.fitness), inlier_rmse=float(last.inlier_rmse),
                              iterations=iters, status=status)


# ------------------------------------------------------------------------------------------------
# frame-to-model refinement of a scan's poses
# ------------------------------------------------------------------------------------------------
@dataclass
class ScanRefinement:
    corrections: np.ndarray        # (F, 4, 4) float64: base-frame motions; refined c2w = corrections[k] @ c2w[k]
    accepted: List[bool]
    report: List[dict]             # per frame: fitness, inlier_rmse, translation, rotation, accepted, reason


def correction_size(T: np.ndarray, centroid: np.ndarray) -> Tuple[float, float]:
    """(how far T moves `centroid`, T's rotation angle in radians)."""
    c = np.asarray(centroid, dtype=np.float64)
    moved = T[:3, :3] @ c + T[:3, 3]
    cos = min(1.0, max(-1.0, 0.5 * (float(np.trace(T[:3, :3])) - 1.0)))
    return float(np.linalg.norm(moved - c)), math.acos(cos)


def refine_scan_poses(frames: Sequence[Tuple[ArrayLike, Optional[ArrayLike]]], min_fitness: float = MIN_FITNESS,
                      max_correction: Tuple[float, float] = MAX_CORRECTION,
                      voxel_radius: Sequence[float] = VOXEL_RADIUS, max_iter: Sequence[int] = MAX_ITER,
                      lambda_geometric: float = LAMBDA_GEOMETRIC, scale: float = 1.0) -> ScanRefinement:
    """Frame-to-model registration.  `frames`: per frame (points (n, 3), colors (n, 3) in [0, 1] or None), already in
    the base frame at the poses as given.  Frame 0 is fixed; frame k is registered (colored_icp, from the identity)
    against the union of frames 0..k-1 at their refined poses, voxel-downsampled at the finest voxel size.  The
    result is accepted only if its fitness is at least min_fitness and it moves the frame's centroid by at most
    max_correction[0] (the clouds' units / scale) and turns by at most max_correction[1] radians; otherwise the frame
    keeps its pose and the report says why.  A rejected frame still joins the model, at its given pose."""
    if not len(frames):
        raise ValueError("no frames")
    dev = default_device("register")
    finest = positive("voxel_radius", min(voxel_radius)) * positive("scale", scale)
    coloured = frames[0][1] is not None
    lam = float(lambda_geometric) if coloured else 1.0
    corrections = np.tile(np.eye(4), (len(frames), 1, 1))
    accepted, report = [], []
    model_p = model_c = None
    for k, (pts, cols) in enumerate(frames):
        p = _cloud(pts, dev)
        c = _cloud(cols, dev) if coloured else None
        row = {"frame": k, "points": int(p.shape[0]), "fitness": None, "inlier_rmse": None, "translation": 0.0,
               "rotation": 0.0, "accepted": True, "reason": "fixed" if k == 0 else ""}
        if k > 0:
            ok, why = False, ""
            if p.shape[0] == 0 or model_p.shape[0] == 0:
                why = "no points"
            else:
                r = colored_icp(p, c, model_p, model_c, None, voxel_radius, max_iter, lam, scale)
                move, turn = correction_size(r.transformation, p.mean(dim=0).cpu().numpy())
                row.update(fitness=r.fitness, inlier_rmse=r.inlier_rmse, translation=move / scale, rotation=turn,
                           iterations=r.iterations, status=r.status)
                if not r.fitness >= min_fitness:
                    why = f"fitness {r.fitness:.3f} < {min_fitness}"
                elif not (move / scale <= max_correction[0] and turn <= max_correction[1]):
                    why = f"correction {move / scale:.4f} / {turn:.4f} rad beyond {tuple(max_correction)}"
                else:
                    ok = True
                    corrections[k] = r.transformation
            row.update(accepted=ok, reason=why)
            if ok:
                Tk = torch.as_tensor(corrections[k], device=dev)
                p = p @ Tk[:3, :3].T + Tk[:3, 3]
        accepted.append(bool(row["accepted"]))
        report.append(row)
        model_p = p if model_p is None else torch.cat((model_p, p))
        model_c = None if not coloured else (c if model_c is None else torch.cat((model_c, c)))
        model_p, model_c = voxel_downsample(model_p, model_c, finest)
    return ScanRefinement(corrections=corrections, accepted=accepted, report=report)


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def _load_cloud(path: str) -> Tuple[np.ndarray, np.ndarray]:
    a = np.load(path)
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError(f"{path}: expected an (N, 6) xyzrgb array, got {a.shape}")
    a = a.astype(np.float64)
    return a[:, :3], a[:, 3:]


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.register",
                                 description="Coloured ICP of one (N, 6) xyzrgb cloud onto another; writes the 4x4 "
                                             "source-to-target transform.")
    ap.add_argument("--source", required=True, help=".npy, (N, 6): x y z r g b, colours in [0, 1]")
    ap.add_argument("--target", required=True, help=".npy, (N, 6)")
    ap.add_argument("--init", default=None, help="JSON with a 4x4 (or 3x4) 'transformation': the first guess")
    ap.add_argument("--out", required=True, help="output .json: transformation, fitness, inlier_rmse, iterations")
    ap.add_argument("--voxel-radius", type=float, nargs="+", default=list(VOXEL_RADIUS))
    ap.add_argument("--max-iter", type=int, nargs="+", default=list(MAX_ITER))
    ap.add_argument("--lambda-geometric", type=float, default=LAMBDA_GEOMETRIC)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the voxel sizes (clouds not in metres)")
    a = ap.parse_args(argv)
    try:
        sp, sc = _load_cloud(a.source)
        tp, tc = _load_cloud(a.target)
        init = None
        if a.init:
            with open(a.init) as f:
                init = np.asarray(json.load(f)["transformation"], dtype=np.float64)
        r = colored_icp(sp, sc, tp, tc, init, a.voxel_radius, a.max_iter, a.lambda_geometric, a.scale)
    except (KeyError, ValueError, OSError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    with open(a.out, "w") as f:
        json.dump({"transformation": r.transformation.tolist(), "fitness": r.fitness, "inlier_rmse": r.inlier_rmse,
                   "iterations": r.iterations, "status": r.status}, f, indent=1)
    print(f"fitness {r.fitness:.4f}, inlier rmse {r.inlier_rmse:.6g}, iterations {r.iterations}; wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
