"""The support plane (the table) of a scene: a RANSAC plane fit over the Gaussians, and what the grasp layer needs of
it.  Two HIP calls (`gg_plane_consensus`, `gg_plane_classify`, csrc/support_plane.hip) test every hypothesis against
every point and label every point against one plane, exactly, in fp64; the contract is in include/gg_raster.h and
PARITY.md "Support plane".  The small linear algebra (three points to a plane, 16 sums to a least-squares plane) is
host fp64.

    draw_hypotheses     (num, 3) int32 index triples, a pure function of (count, num, seed)
    consensus           one gg_plane_consensus call: count, valid, best
    classify            one gg_plane_classify call: side, height, the 16 sums
    plane_from_triple   the plane through three points
    plane_from_moments  the least-squares plane of the 16 sums
    fit_plane           consensus -> best triple -> refits -> closing classify (SupportPlane)
    support_plane       fit_plane on a model's Gaussians, around an object mask when there is one
    above               the part of a mask that lies above the plane
    save_plane / load_plane   JSON holding normal, offset and dist
    python -m gaussiangrasper_amd.support --ckpt IN [...] --out plane.json [--labels side.npy]

dist 0.01 m, region_margin 0.25 m, 1024 hypotheses, 2 refits and min_sin2 1e-6 are this project's choices, UNVERIFIED on
a real checkpoint (PARITY.md "Support plane")."""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (ArrayLike, f32_rows, host_ptr, nonneg, positive, ptr as _ptr, require_hip as _require_hip,
                    stream as _stream, workspace as _ws)

DIST = 0.01                  # metres: half the thickness of the slab that counts as "on the plane"
REGION_MARGIN = 0.25         # metres: how far around the object's bounding box the table is looked for
NUM_HYPOTHESES = 1024
REFINE = 2
MIN_SIN2 = 1e-6              # a triple whose angle at p_a has sin^2 below this defines no plane
MAX_HYPOTHESES = 65536       # GG_PLANE_MAX_HYPOTHESES
DEGENERATE_RATIO = 1e-12     # plane_from_moments: lambda_1 <= this times lambda_2 is a line, not a plane
SIDE_BELOW, SIDE_ON, SIDE_ABOVE, SIDE_NONE = 0, 1, 2, 3


@dataclass
class SupportPlane:
    """A plane n.x + offset = 0 with |n| = 1, n pointing away from the support, and the labels of the points it was
    fitted to."""
    normal: np.ndarray           # (3,) float64
    offset: float
    dist: float                  # |n.x + offset| <= dist is "on"
    side: Optional[Tensor] = None       # (N,) uint8 device: 0 below, 1 on, 2 above, 3 takes no part
    height: Optional[Tensor] = None     # (N,) float32 device: n.x + offset, NaN for a point that is not finite
    count_on: int = 0
    count_above: int = 0
    count_below: int = 0
    rmse: float = math.nan       # sqrt(sum of height^2 over "on" / count_on)
    hypothesis_count: int = 0    # the inliers of the best hypothesis
    best: int = -1               # its index among the hypotheses
    status: str = "ok"           # "degenerate": the last refit had no plane to give, the one before it stands


# ------------------------------------------------------------------------------------------------
# host side (numpy, fp64)
# ------------------------------------------------------------------------------------------------
def draw_hypotheses(count: int, num: int, seed: int) -> np.ndarray:
    """(num, 3) int32 indices in [0, count), uniform, from np.random.default_rng(seed).  Triples with a repeated index
    are not redrawn: gg_plane_consensus marks them not valid."""
    count, num = int(count), int(num)
    if count < 1 or not 0 <= num <= MAX_HYPOTHESES:
        raise ValueError(f"need count >= 1 and 0 <= num <= {MAX_HYPOTHESES}, got {count} and {num}")
    return np.random.default_rng(int(seed)).integers(0, count, size=(num, 3), dtype=np.int32)


def _largest_positive(n: np.ndarray) -> np.ndarray:
    return -n if n[int(np.argmax(np.abs(n)))] < 0.0 else n


def plane_from_triple(p_a: ArrayLike, p_b: ArrayLike, p_c: ArrayLike) -> Tuple[np.ndarray, float]:
    """(n, d) of the plane through three points: n = (p_b - p_a) x (p_c - p_a) / |.|, its largest-magnitude component
    positive, d = -n.p_a.  ValueError for a triple that spans no plane."""
    a, b, c = (np.asarray(p, dtype=np.float64).reshape(3) for p in (p_a, p_b, p_c))
    n = np.cross(b - a, c - a)
    length = math.sqrt(float(n @ n))
    if not (math.isfinite(length) and length > 0.0):
        raise ValueError("the three points span no plane")
    n = _largest_positive(n / length)
    return n, -float(n @ a)


def plane_from_moments(sums: ArrayLike, origin: ArrayLike, prev_normal: ArrayLike,
                       prev_offset: Optional[float] = None) -> Tuple[np.ndarray, Optional[float], str]:
    """(n, d, status) of the least-squares plane of gg_plane_classify's 16 sums about `origin`: with m = sums[0],
    the centroid c = origin + sum q / m, the covariance sum q q^T - (sum q)(sum q)^T / m, n = its eigenvector of the
    smallest eigenvalue (np.linalg.eigh), signed towards prev_normal, d = -n.c, status "ok".  With m < 3 or
    lambda_1 <= 1e-12 lambda_2 (the points lie on a line) there is no plane: (prev_normal, prev_offset,
    "degenerate")."""
    s = np.asarray(sums, dtype=np.float64).reshape(16)
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    prev = np.asarray(prev_normal, dtype=np.float64).reshape(3)
    m = s[0]
    if not m >= 3.0:
        return prev, prev_offset, "degenerate"
    sq = s[4:7]
    sqq = np.array([[s[7], s[8], s[9]], [s[8], s[10], s[11]], [s[9], s[11], s[12]]])
    cov = sqq - np.outer(sq, sq) / m
    lam, vec = np.linalg.eigh(cov)
    if not (np.isfinite(lam).all() and lam[1] > DEGENERATE_RATIO * lam[2]):
        return prev, prev_offset, "degenerate"
    n = vec[:, 0] / math.sqrt(float(vec[:, 0] @ vec[:, 0]))
    if float(n @ prev) < 0.0:
        n = -n
    return n, -float(n @ (o + sq / m)), "ok"


def check_up(up: Optional[ArrayLike], max_tilt: Optional[float]) -> Tuple[Optional[np.ndarray], float]:
    """(up as (3,) float64 or None, cos^2 of max_tilt).  max_tilt: radians in [0, pi / 2], only with `up`; None: no
    tilt limit (up then only orients the normal)."""
    if up is None:
        if max_tilt is not None:
            raise ValueError("max_tilt needs up: a tilt is measured against it")
        return None, 0.0
    u = np.ascontiguousarray(np.asarray(up, dtype=np.float64).reshape(-1))
    if u.shape != (3,) or not np.isfinite(u).all() or not float(u @ u) > 0.0:
        raise ValueError(f"up must be three finite numbers, not all zero, got {up}")
    if max_tilt is None:
        return u, 0.0
    t = float(max_tilt)
    if not 0.0 <= t <= 0.5 * math.pi:
        raise ValueError(f"max_tilt must be in [0, pi / 2] radians, got {max_tilt}")
    return u, math.cos(t) ** 2


def save_plane(path: str, plane: SupportPlane) -> None:
    with open(path, "w") as f:
        json.dump({"normal": [float(v) for v in plane.normal], "offset": float(plane.offset),
                   "dist": float(plane.dist)}, f, indent=1)


def load_plane(path: str) -> SupportPlane:
    """A SupportPlane (normal, offset, dist; no labels) from save_plane's JSON.  A normal that is not of unit length
    (a file written by hand) is brought to it, and the offset with it."""
    with open(path) as f:
        try:
            d = json.load(f)
        except json.JSONDecodeError as exc:
            raise ValueError(f"{path}: not JSON: {exc}") from exc
    try:
        n = np.asarray(d["normal"], dtype=np.float64).reshape(-1)
        offset, dist = float(d["offset"]), float(d["dist"])
    except (KeyError, TypeError, ValueError) as exc:
        raise ValueError(f"{path}: a plane file holds normal, offset and dist: {exc}") from exc
    if n.shape != (3,) or not np.isfinite(n).all() or not float(n @ n) > 0.0 or not math.isfinite(offset):
        raise ValueError(f"{path}: normal must be three finite numbers, not all zero, and offset finite")
    if not (math.isfinite(dist) and dist >= 0.0):
        raise ValueError(f"{path}: dist must be finite and >= 0")
    length = math.sqrt(float(n @ n))
    if abs(length - 1.0) <= 1e-12:           # save_plane's own output: kept to the bit
        length = 1.0
    return SupportPlane(normal=n / length, offset=offset / length, dist=dist)


# ------------------------------------------------------------------------------------------------
# device side: the two calls
# ------------------------------------------------------------------------------------------------
def _points_weights(points: Tensor, weights: Optional[Tensor]):
    dev = _require_hip(points) if weights is None else _require_hip(points, weights)
    points = f32_rows(points, "points", 3)
    if weights is not None:
        weights = f32_rows(weights, "weights", None)
        if weights.shape[0] != points.shape[0]:
            raise ValueError(f"points has {points.shape[0]} rows, weights {weights.shape[0]}")
    return dev, points, weights


def consensus(points: Tensor, weights: Optional[Tensor], hyp: Tensor, dist: float, min_weight: float = 0.0,
              min_sin2: float = MIN_SIN2, up: Optional[ArrayLike] = None, max_tilt: Optional[float] = None):
    """(count int32 (H,), valid bool (H,), best int32 (2,)) of gg_plane_consensus, device tensors.  points (N, 3)
    float32 and hyp (H, 3) int32 on the HIP device (no CPU path); weights (N,) float32 or None.  Nothing waits on the
    host."""
    dev, points, weights = _points_weights(points, weights)
    if hyp.dtype != torch.int32 or hyp.ndim != 2 or hyp.shape[1] != 3 or hyp.device != dev:
        raise ValueError(f"hyp must be an int32 (H, 3) tensor on {dev}, got {hyp.dtype} {tuple(hyp.shape)}")
    hyp = hyp.contiguous()
    n, h = points.shape[0], hyp.shape[0]
    u, cos2 = check_up(up, max_tilt)
    if math.isnan(float(min_weight)) or not 0.0 <= float(min_sin2) <= 1.0:
        raise ValueError("min_weight must not be NaN and min_sin2 must be in [0, 1]")
    lib = _lib.load()
    count = torch.empty(h, dtype=torch.int32, device=dev)
    valid = torch.empty(h, dtype=torch.uint8, device=dev)
    best = torch.tensor([-1, 0], dtype=torch.int32, device=dev)
    nbytes = lib.gg_plane_consensus_workspace(n, h)
    if nbytes == 0:
        raise ValueError(f"{n} points x {h} hypotheses is beyond gg_plane_consensus' limits")
    ws = _ws(nbytes, dev)
    _lib.check(lib.gg_plane_consensus(n, _ptr(points), _ptr(weights), float(min_weight), h, _ptr(hyp),
                                      nonneg("dist", dist), float(min_sin2), host_ptr(u), cos2, _ptr(count),
                                      _ptr(valid), _ptr(best), _ptr(ws), ws.numel(), _stream(dev)),
               "gg_plane_consensus")
    return count, valid.bool(), best


def classify(points: Tensor, weights: Optional[Tensor], normal: ArrayLike, offset: float, origin: ArrayLike,
             dist: float, min_weight: float = 0.0):
    """(side uint8 (N,), height float32 (N,), sums float64 (16,)) of gg_plane_classify, device tensors.  Nothing waits
    on the host."""
    dev, points, weights = _points_weights(points, weights)
    n = points.shape[0]
    plane = np.ascontiguousarray(np.concatenate([np.asarray(normal, dtype=np.float64).reshape(3), [float(offset)]]))
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
    if math.isnan(float(min_weight)):
        raise ValueError("min_weight must not be NaN")
    lib = _lib.load()
    side = torch.empty(n, dtype=torch.uint8, device=dev)
    height = torch.empty(n, dtype=torch.float32, device=dev)
    sums = torch.empty(16, dtype=torch.float64, device=dev)
    nbytes = lib.gg_plane_classify_workspace(n)
    if nbytes == 0:
        raise ValueError(f"{n} points is beyond gg_plane_classify's limit")
    ws = _ws(nbytes, dev)
    _lib.check(lib.gg_plane_classify(n, _ptr(points), _ptr(weights), float(min_weight), host_ptr(plane),
                                     host_ptr(org), nonneg("dist", dist), _ptr(height), _ptr(side), _ptr(sums),
                                     _ptr(ws), ws.numel(), _stream(dev)), "gg_plane_classify")
    return side, height, sums


def fit_plane(points: Tensor, weights: Optional[Tensor] = None, dist: float = DIST,
              num_hypotheses: int = NUM_HYPOTHESES, up: Optional[ArrayLike] = None, max_tilt: Optional[float] = None,
              min_weight: float = 0.0, seed: int = 0, refine: int = REFINE,
              min_sin2: float = MIN_SIN2) -> SupportPlane:
    """The dominant plane of the points that take part (finite, weight > min_weight; weights None: all).
    draw_hypotheses(N, num_hypotheses, seed), consensus, the best triple's plane on the host (plane_from_triple), then
    `refine` rounds of classify -> plane_from_moments (the moments about the triple's first point, then about the last
    centroid), then a closing classify whose labels, counts and rmse are returned.  With `up` the hypotheses are held
    within max_tilt (radians; None: no limit) of it and the normal has n.up > 0; without, the normal points to the
    side with the larger summed weight, and on equality its largest-magnitude component is positive.  Read-backs: best
    with its three points (one copy of 11 numbers) and 16 doubles per classify, nothing else.  No valid hypothesis:
    ValueError."""
    dev, points, weights = _points_weights(points, weights)
    n = points.shape[0]
    refine = int(refine)
    if refine < 0:
        raise ValueError(f"refine must be >= 0, got {refine}")
    if n < 3:
        raise ValueError(f"a plane fit needs at least 3 points, got {n}")
    u, _ = check_up(up, max_tilt)
    dist = nonneg("dist", dist)
    hyp = torch.from_numpy(draw_hypotheses(n, num_hypotheses, seed)).to(dev)
    count, _, best = consensus(points, weights, hyp, dist, min_weight, min_sin2, up, max_tilt)
    if hyp.shape[0] == 0:
        raise ValueError("no hypothesis was drawn")
    tri = points[hyp[best[:1].clamp(min=0).long()].reshape(3).long()].double().reshape(9)
    back = torch.cat([best.double(), tri]).cpu().numpy()
    bi, bc = int(back[0]), int(back[1])
    if bi < 0:
        raise ValueError(f"none of the {hyp.shape[0]} hypotheses is valid (too few points take part, or every triple "
                         "is collinear or tilted beyond max_tilt)")
    p = back[2:].reshape(3, 3)
    normal, offset = plane_from_triple(p[0], p[1], p[2])
    if u is not None and float(normal @ u) != 0.0:
        if float(normal @ u) < 0.0:
            normal, offset = -normal, -offset
    origin, status = p[0].copy(), "ok"
    for _ in range(refine):
        sums = classify(points, weights, normal, offset, origin, dist, min_weight)[2].cpu().numpy()
        normal, offset, status = plane_from_moments(sums, origin, normal, offset)
        if status == "ok":
            origin = origin + sums[4:7] / sums[0]
    side, height, sums_t = classify(points, weights, normal, offset, origin, dist, min_weight)
    sums = sums_t.cpu().numpy()
    flip = False
    if u is None:
        flip = sums[14] < sums[15] or (sums[14] == sums[15] and normal[int(np.argmax(np.abs(normal)))] < 0.0)
    if flip:                       # the negated plane's h is -h exactly: relabel, do not classify again
        normal, offset = -normal, -offset
        side = torch.where(side == SIDE_BELOW, SIDE_ABOVE, torch.where(side == SIDE_ABOVE, SIDE_BELOW, side))
        side = side.to(torch.uint8)
        height = -height
        sums[[1, 2, 14, 15]] = sums[[2, 1, 15, 14]]
    on = int(sums[0])
    return SupportPlane(normal=np.asarray(normal, dtype=np.float64), offset=float(offset), dist=dist, side=side,
                        height=height, count_on=on, count_above=int(sums[1]), count_below=int(sums[2]),
                        rmse=math.sqrt(sums[3] / on) if on > 0 else math.nan, hypothesis_count=bc, best=bi,
                        status=status)


@torch.no_grad()
def support_plane(model_or_scene, mask: Optional[Tensor] = None, region_margin: float = REGION_MARGIN,
                  dist: float = DIST, scale: float = 1.0, **fit) -> SupportPlane:
    """The support plane of a model's Gaussians: fit_plane(points, weights, dist * scale, **fit) on
    grasp.model_points(model, None).  With an object `mask` (N,), only the Gaussians inside the mask's bounding box
    inflated by region_margin * scale take part in the fit (the table under the object, not the floor beside it);
    side and height are then those of EVERY Gaussian against the fitted plane (one more classify), while the counts
    and rmse stay the region's.  dist and region_margin are in metres, scale the scene's units per metre."""
    from .grasp import model_points
    s = positive("scale", scale)
    pts, _, w = model_points(model_or_scene, None)
    d = nonneg("dist", dist) * s
    if mask is None:
        return fit_plane(pts, w, d, **fit)
    mask = mask.reshape(-1).to(device=pts.device, dtype=torch.bool)
    if mask.shape[0] != pts.shape[0]:
        raise ValueError(f"mask has {mask.shape[0]} entries for {pts.shape[0]} Gaussians")
    obj = pts[mask & torch.isfinite(pts).all(dim=1)]
    if obj.shape[0] == 0:
        raise ValueError("the mask selects no Gaussian")
    m = nonneg("region_margin", region_margin) * s
    lo, hi = obj.min(dim=0).values - m, obj.max(dim=0).values + m
    idx = torch.nonzero(((pts >= lo) & (pts <= hi)).all(dim=1)).reshape(-1)
    plane = fit_plane(pts[idx].contiguous(), w[idx].contiguous(), d, **fit)
    origin = -plane.offset * plane.normal
    plane.side, plane.height, _ = classify(pts, w, plane.normal, plane.offset, origin, d, fit.get("min_weight", 0.0))
    return plane


def above(mask: Tensor, plane: SupportPlane, margin: float = 0.0) -> Tensor:
    """mask & (side == 2) & (height > margin): the selected Gaussians that lie above the plane's slab, and more than
    `margin` (scene units) above the plane itself."""
    if plane.side is None or plane.height is None:
        raise ValueError("the plane carries no labels (a loaded plane: classify the points against it first)")
    mask = mask.reshape(-1).to(device=plane.side.device, dtype=torch.bool)
    if mask.shape[0] != plane.side.shape[0]:
        raise ValueError(f"mask has {mask.shape[0]} entries, the plane's labels {plane.side.shape[0]}")
    return mask & (plane.side == SIDE_ABOVE) & (plane.height > float(margin))


def label_model(model_or_scene, plane: SupportPlane, min_weight: float = 0.0) -> SupportPlane:
    """`plane` with side and height of every Gaussian of the model (for a plane that load_plane read)."""
    from .grasp import model_points
    pts, _, w = model_points(model_or_scene, None)
    plane.side, plane.height, _ = classify(pts, w, plane.normal, plane.offset, -plane.offset * plane.normal,
                                           plane.dist, min_weight)
    return plane


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def main(argv: Optional[Sequence[str]] = None) -> int:
    from ._cli import add_object_options, check_object_options, load_scene, object_mask
    from .frames import check_rotation, load_transform_json
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.support",
                                 description="Fit the support plane (the table) of a checkpoint's Gaussians, around "
                                             "the selected object when there is a selection.")
    ap.add_argument("--ckpt", required=True, help="step-*.ckpt of a splatting model")
    ap.add_argument("--transform-json", default=None, help="JSON with transform_matrix and scale (world -> scene)")
    add_object_options(ap, "the table is looked for around the Gaussians the query selects",
                       "bounds where the table is looked for")
    ap.add_argument("--up", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                    help="up direction, world frame: orients the normal")
    ap.add_argument("--max-tilt", type=float, default=None, metavar="DEGREES",
                    help="with --up: the plane's normal is within this of it")
    ap.add_argument("--dist", type=float, default=DIST, metavar="METRES", help="half thickness of the plane's slab")
    ap.add_argument("--hypotheses", type=int, default=NUM_HYPOTHESES, help="RANSAC triples")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--min-opacity", type=float, default=0.0, help="a Gaussian takes part above it")
    ap.add_argument("--out", required=True, help="output .json: normal, offset, dist (scene frame)")
    ap.add_argument("--labels", default=None, help="output .npy: (N,) uint8 side of every Gaussian (0 below, 1 on, "
                                                   "2 above, 3 takes no part)")
    a = ap.parse_args(argv)
    check_object_options(ap, a, "optional")
    if a.max_tilt is not None and a.up is None:
        ap.error("--max-tilt needs --up")
    if a.max_tilt is not None and not 0.0 <= a.max_tilt <= 90.0:
        ap.error(f"--max-tilt must be in 0..90 degrees, got {a.max_tilt}")
    if not (math.isfinite(a.dist) and a.dist >= 0.0):
        ap.error(f"--dist must be finite and >= 0, got {a.dist}")
    if not 1 <= a.hypotheses <= MAX_HYPOTHESES:
        ap.error(f"--hypotheses must be in 1..{MAX_HYPOTHESES}, got {a.hypotheses}")
    try:
        matrix, scale = None, 1.0
        if a.transform_json:
            matrix, scale = load_transform_json(a.transform_json)
            if matrix.shape not in ((3, 4), (4, 4)):
                raise ValueError(f"transform_matrix must be 3x4 or 4x4, got {matrix.shape}")
            check_rotation(matrix[:3, :3], "matrix rotation")
        up = None
        if a.up is not None:
            up = np.asarray(a.up, dtype=np.float64) if matrix is None else matrix[:3, :3] @ np.asarray(a.up)
        scene, mlp_state = load_scene(a.ckpt)
        mask = object_mask(a, scene, mlp_state, matrix, scale)
        plane = support_plane(scene, mask, dist=a.dist, scale=scale, num_hypotheses=a.hypotheses, up=up,
                              max_tilt=None if a.max_tilt is None else math.radians(a.max_tilt),
                              min_weight=a.min_opacity, seed=a.seed)
    except (KeyError, ValueError, OSError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    save_plane(a.out, plane)
    if a.labels:
        np.save(a.labels, plane.side.cpu().numpy())
    print(f"plane n = {plane.normal.tolist()}, offset {plane.offset:.6g}: {plane.count_on} on, {plane.count_above} "
          f"above, {plane.count_below} below, rmse {plane.rmse:.3g} ({plane.status}); wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
