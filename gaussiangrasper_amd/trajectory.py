"""Arm trajectories: from a joint-space polyline to q(t) at a controller's rate, inside joint velocity and acceleration
limits.  Corners are replaced by parabolic blends small enough that the proof of clearance of the polyline still holds;
the time law is the quickest on a grid of the path (`gg_traj_time`, a backward and a forward sweep with a closed-form
linear programme per step) and `gg_traj_sample` reads it out at a fixed rate, csrc/trajectory.hip.  The contract is in
include/gg_raster.h and PARITY.md "Arm trajectories"; the proofs and the kernel's budget in DESIGN.md §3.35.

    Limits             v_max, a_max per joint; from_json / to_json / scaled(vel, acc)
    default_limits     the Franka Panda's joint limits AS RECALLED (UNVERIFIED)
    blend_fractions    the largest blend fractions that keep every sphere within delta of the polyline's sweep (host)
    time_paths / sample   the two calls as they are (no CPU path)
    plan_trajectories  routes -> Trajectory: duplicates removed, fractions proven or verified, timed, sampled
    time_plan / time_reach   durations per (from, to) of a roadmap.Plan and per (path, seed) of an arm.Reach
    python -m gaussiangrasper_amd.trajectory --arm {default,FILE.json} --waypoints W.npy|way.npz
                                             --limits {default,FILE.json} [--vel-scale V --acc-scale A] --dt 0.001
                                             --steps 16 (--delta D | --blend F --field field.npz ...) --out traj.npz

Out of scope: torque and jerk limits, Cartesian speed limits, and time-optimality of the continuous problem: the law
is the quickest for its grid."""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from . import arm as _arm
from ._call import (ArrayLike, default_device, host_ptr, nonneg, positive, ptr as _ptr, require_hip as _require_hip,
                    stream as _stream, to_device)
from .arm import MAX_JOINTS, SPHERE_RADIUS, Arm
from .field import MAX_POSES

MAX_WAYPOINTS = 64             # GG_TRAJ_MAX_WAYPOINTS
MAX_STEPS = 64                 # GG_TRAJ_MAX_STEPS
OK, NOT_FINITE, ZERO_SEGMENT, NO_DURATION = 0, 1, 2, 3      # GG_TRAJ_*
STEPS = 16                     # intervals per piece: this project's choice (PARITY.md "Arm trajectories")
DT = 1e-3
# The Franka Panda's joint limits AS RECALLED (UNVERIFIED, PARITY.md "Arm trajectories"): rad/s and rad/s^2
PANDA_V_MAX = (2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61)
PANDA_A_MAX = (15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0)


def grid_max(num_waypoints: int, steps: int) -> int:
    """GG_TRAJ_GRID(W, m)"""
    return steps * (2 * num_waypoints - 3) if num_waypoints >= 2 else 0


@dataclass
class Limits:
    """Joint velocity and acceleration limits, (J,) float64 each, finite and > 0."""
    v_max: np.ndarray
    a_max: np.ndarray

    def __post_init__(self):
        self.v_max = np.ascontiguousarray(np.asarray(self.v_max, np.float64).reshape(-1))
        self.a_max = np.ascontiguousarray(np.asarray(self.a_max, np.float64).reshape(-1))
        if self.v_max.shape != self.a_max.shape or not 1 <= len(self.v_max) <= MAX_JOINTS:
            raise ValueError(f"v_max and a_max must be (J,) with J in 1..{MAX_JOINTS}, got {self.v_max.shape} and "
                             f"{self.a_max.shape}")
        for name, v in (("v_max", self.v_max), ("a_max", self.a_max)):
            if not (np.isfinite(v).all() and (v > 0.0).all()):
                raise ValueError(f"{name}: every entry must be finite and > 0")

    @property
    def num_joints(self) -> int:
        return len(self.v_max)

    def scaled(self, vel: float = 1.0, acc: float = 1.0) -> "Limits":
        """The limits times factors in (0, 1], as MoveIt's velocity and acceleration scaling factors (recalled)."""
        for name, s in (("vel", vel), ("acc", acc)):
            if not (math.isfinite(s) and 0.0 < s <= 1.0):
                raise ValueError(f"{name} must be in (0, 1], got {s}")
        return Limits(self.v_max * float(vel), self.a_max * float(acc))

    def to_json(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump({"v_max": self.v_max.tolist(), "a_max": self.a_max.tolist()}, f)

    @classmethod
    def from_json(cls, path: str) -> "Limits":
        """Limits from a JSON file of numbers only: v_max [J], a_max [J].  ValueError naming the file and the field."""
        with open(path) as f:
            try:
                d = json.load(f)
            except json.JSONDecodeError as exc:
                raise ValueError(f"{path}: not JSON: {exc}") from exc
        try:
            if not isinstance(d, dict):
                raise ValueError("expected an object with v_max and a_max")
            return cls(np.asarray(d["v_max"], np.float64), np.asarray(d["a_max"], np.float64))
        except KeyError as exc:
            raise ValueError(f"{path}: {exc.args[0]} is missing") from exc
        except (TypeError, ValueError) as exc:
            raise ValueError(f"{path}: {exc}") from exc


def default_limits() -> Limits:
    """The Franka Panda's joint velocity and acceleration limits AS RECALLED (UNVERIFIED)."""
    return Limits(np.array(PANDA_V_MAX), np.array(PANDA_A_MAX))


def load_limits_option(text: str) -> Limits:
    return default_limits() if text == "default" else Limits.from_json(text)


# ------------------------------------------------------------------------------------------------
# host side: the blend theorem's fractions
# ------------------------------------------------------------------------------------------------
def sweep_bounds(arm: Arm, way: ArrayLike, spheres: Optional[ArrayLike] = None,
                 radius: Union[float, ArrayLike] = SPHERE_RADIUS) -> np.ndarray:
    """(n - 1,) float64: B_k = max_s sum_j |d_k[j]| reach[j][s], gg_arm_motion's sweep bound of every segment of the
    (n, J) polyline, for the arm's link spheres and the optional gripper-frame `spheres`."""
    w = np.asarray(way, np.float64).reshape(-1, arm.num_joints)
    c, f, _ = _arm._self_set(arm, spheres, radius)
    reach = _arm.reach_table(arm, c, f)                               # (J, S)
    if len(w) < 2 or reach.shape[1] == 0:
        return np.zeros(max(len(w) - 1, 0))
    return (np.abs(np.diff(w, axis=0)) @ reach).max(axis=1)


def blend_fractions(arm: Arm, way: ArrayLike, delta: float, spheres: Optional[ArrayLike] = None,
                    radius: Union[float, ArrayLike] = SPHERE_RADIUS) -> np.ndarray:
    """(n,) float64: f_k = min(1/2, 2 delta / B_{k-1}, 2 delta / B_k) at the interior waypoints of the (n, J)
    polyline, 0 at both ends.  With these no sphere centre on a blend is further than delta from its position at a
    configuration of the polyline: edges that passed arm.motion with margin >= delta and
    self_margin >= 2 delta stay proven clear."""
    delta = nonneg("delta", delta)
    B = sweep_bounds(arm, way, spheres, radius)
    n = len(B) + 1
    f = np.zeros(n)
    for k in range(1, n - 1):
        big = max(B[k - 1], B[k])
        f[k] = 0.5 if big <= 0.0 else min(0.5, 2.0 * delta / big)
    return f


# ------------------------------------------------------------------------------------------------
# device side: the two calls as they are
# ------------------------------------------------------------------------------------------------
@dataclass
class TimeLaw:
    """The inputs and outputs of one gg_traj_time call over P paths of at most W waypoints, Gmax = grid_max(W, steps)."""
    way: Tensor            # (P, W, J) float64
    length: Tensor         # (P,) int32
    blend: Tensor          # (P, W) float64
    steps: int
    count: Tensor          # (P,) int32 G, the path's intervals
    xbar: Tensor           # (P, Gmax + 1) float64 the largest (ds/dt)^2 from which the path can still be finished
    x: Tensor              # (P, Gmax + 1) float64 (ds/dt)^2 at the grid points
    u: Tensor              # (P, Gmax) float64 d2s/dt2 on the intervals
    t: Tensor              # (P, Gmax + 1) float64 the time at the grid points
    q_grid: Optional[Tensor]   # (P, Gmax + 1, J) float64, or None when not asked for
    duration: Tensor       # (P,) float64
    infeasible: Tensor     # (P,) float64 how far the chosen u fell below a lower line: rounding only
    status: Tensor         # (P,) int32 OK, NOT_FINITE, ZERO_SEGMENT, NO_DURATION


def time_paths(way: Tensor, length: Tensor, blend: Tensor, limits: Limits, steps: int = STEPS,
               q_grid: bool = True) -> TimeLaw:
    """One gg_traj_time call: way (P, W, J) float64, length (P,) int32 and blend (P, W) float64 on the HIP device (no
    CPU path)."""
    dev = _require_hip(way, length, blend)
    if way.dtype != torch.float64 or way.ndim != 3:
        raise ValueError(f"way must be a float64 (P, W, J) tensor, got {way.dtype} {tuple(way.shape)}")
    p, w, J = way.shape
    if J != limits.num_joints:
        raise ValueError(f"the limits are for {limits.num_joints} joints, the paths have {J}")
    if not 1 <= w <= MAX_WAYPOINTS:
        raise ValueError(f"a path has 1..{MAX_WAYPOINTS} waypoints, got {w}")
    if not 2 <= int(steps) <= MAX_STEPS:
        raise ValueError(f"steps must be in 2..{MAX_STEPS}, got {steps}")
    if length.dtype != torch.int32 or tuple(length.shape) != (p,):
        raise ValueError(f"length must be an int32 ({p},) tensor, got {length.dtype} {tuple(length.shape)}")
    if blend.dtype != torch.float64 or tuple(blend.shape) != (p, w):
        raise ValueError(f"blend must be a float64 ({p}, {w}) tensor, got {blend.dtype} {tuple(blend.shape)}")
    g = grid_max(w, int(steps))
    if p * (g + 1) > MAX_POSES:
        raise ValueError(f"{p} paths x {g + 1} grid points are more than {MAX_POSES}")
    way, length, blend = way.contiguous(), length.contiguous(), blend.contiguous()
    f64 = dict(dtype=torch.float64, device=dev)
    count = torch.empty(p, dtype=torch.int32, device=dev)
    status = torch.empty(p, dtype=torch.int32, device=dev)
    xbar, x, t = (torch.empty(p, g + 1, **f64) for _ in range(3))
    u = torch.empty(p, g, **f64)
    grid = torch.empty(p, g + 1, J, **f64) if q_grid else None
    duration, infeasible = torch.empty(p, **f64), torch.empty(p, **f64)
    _lib.check(_lib.load().gg_traj_time(J, p, w, _ptr(way), _ptr(length), _ptr(blend), host_ptr(limits.v_max),
                                        host_ptr(limits.a_max), int(steps), _ptr(count), _ptr(xbar), _ptr(x), _ptr(u),
                                        _ptr(t), _ptr(grid), _ptr(duration), _ptr(infeasible), _ptr(status),
                                        _stream(dev)), "gg_traj_time")
    return TimeLaw(way, length, blend, int(steps), count, xbar, x, u, t, grid, duration, infeasible, status)


@dataclass
class Samples:
    q: Tensor              # (P, K, J) float64; NaN from row num[p] on
    qd: Tensor             # (P, K, J) float64
    qdd: Tensor            # (P, K, J) float64
    num: Tensor            # (P,) int32 the samples of the whole path: the last one is at `duration`
    dt: float


def sample(law: TimeLaw, dt: float = DT, num_samples: Optional[int] = None) -> Samples:
    """One gg_traj_sample call.  num_samples None: as many as the longest path of `law` needs (this reads the
    durations back)."""
    dt = positive("dt", dt)
    p, w, J = law.way.shape
    dev = law.way.device
    if num_samples is None:
        d = law.duration[law.status == OK]
        longest = float(d.max()) if d.numel() else 0.0
        num_samples = int(math.ceil(longest / dt)) + 2
    k = int(num_samples)
    if k < 1 or p * k > MAX_POSES:
        raise ValueError(f"need num_samples >= 1 and P num_samples <= {MAX_POSES}, got {k} for {p} paths")
    q, qd, qdd = (torch.empty(p, k, J, dtype=torch.float64, device=dev) for _ in range(3))
    num = torch.empty(p, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_traj_sample(J, p, w, _ptr(law.way), _ptr(law.length), _ptr(law.blend), law.steps,
                                          _ptr(law.count), _ptr(law.x), _ptr(law.u), _ptr(law.t), _ptr(law.duration),
                                          _ptr(law.status), dt, k, _ptr(q), _ptr(qd), _ptr(qdd), _ptr(num),
                                          _stream(dev)), "gg_traj_sample")
    return Samples(q, qd, qdd, num, dt)


# ------------------------------------------------------------------------------------------------
# the task layer
# ------------------------------------------------------------------------------------------------
def dedupe(way: ArrayLike) -> np.ndarray:
    """The (n, J) waypoints without rows that repeat the row before them, and without NaN padding rows at the end."""
    w = np.asarray(way, np.float64)
    w = w.reshape(-1, w.shape[-1])
    while len(w) and np.isnan(w[-1]).all():
        w = w[:-1]
    if len(w) < 2:
        return w.copy()
    keep = np.concatenate([[True], (np.diff(w, axis=0) != 0.0).any(axis=1) | np.isnan(np.diff(w, axis=0)).any(axis=1)])
    return w[keep]


def pack_routes(routes: Sequence[ArrayLike], J: int) -> Tuple[np.ndarray, np.ndarray]:
    """(way (P, W, J) float64, length (P,) int32) of the routes after `dedupe`, W the longest; rows past a route's end are
    0 and are not read."""
    rows = [dedupe(r) for r in routes]
    for r in rows:
        if r.ndim != 2 or r.shape[1] != J or len(r) < 1:
            raise ValueError(f"a route is (n, {J}) with n >= 1, got {r.shape}")
    W = max([len(r) for r in rows] + [1])
    if W > MAX_WAYPOINTS:
        raise ValueError(f"a route of {W} waypoints is longer than {MAX_WAYPOINTS}")
    way = np.zeros((len(rows), W, J))
    for p, r in enumerate(rows):
        way[p, :len(r)] = r
    return way, np.array([len(r) for r in rows], np.int32).reshape(len(rows))


def blend_chords(way: np.ndarray, k: int, f: float, steps: int) -> np.ndarray:
    """(steps + 1, J) the grid points of the blend of fraction f about waypoint k of the (n, J) polyline, the header's
    formula."""
    dm, dp = way[k] - way[k - 1], way[k + 1] - way[k]
    tau = (np.arange(steps + 1).astype(np.float64) / np.float64(steps))[:, None]
    return ((way[k] - f * dm) + tau * ((2.0 * f) * dm)) + (tau * tau) * (f * (dp - dm))


@dataclass
class Trajectory:
    t: np.ndarray          # (K,) float64 k dt
    q: Tensor              # (P, K, J) float64; NaN from row num[p] on (the last real row is at `duration`)
    qd: Tensor             # (P, K, J) float64
    qdd: Tensor            # (P, K, J) float64
    num: Tensor            # (P,) int32
    duration: Tensor       # (P,) float64
    fractions: np.ndarray  # (P, W) float64 the blend fractions used
    verified: np.ndarray   # (P, W) bool: a fraction above the proven one that passed the chord test
    status: Tensor         # (P,) int32
    law: TimeLaw


def plan_trajectories(arm: Arm, routes: Sequence[ArrayLike], limits: Limits, field=None,
                      blend: Optional[float] = None, delta: Optional[float] = None, dt: float = DT,
                      steps: int = STEPS, verify: bool = False, num_samples: Optional[int] = None,
                      **motion_kw) -> Trajectory:
    """Time and sample the joint-space `routes` (each (n, J); consecutive duplicates and NaN padding are removed).
    delta: the corners get the proven fractions of `blend_fractions` (spheres and radius from motion_kw).  blend: the
    fraction asked for at every interior waypoint; where it exceeds the proven one (0 without delta) it needs
    verify=True and a field or a self test: the chords between consecutive grid points of every such blend, of every
    route, go into ONE arm.motion call whose margin is raised by the chords' sag bound, and a blend with a chord that is
    not ok falls back once to its proven fraction, which may be 0: a stop.  motion_kw: arm.motion's keywords."""
    J = arm.num_joints
    way, length = pack_routes(routes, J)
    P, W, _ = way.shape
    spheres, radius = motion_kw.get("spheres"), motion_kw.get("radius", SPHERE_RADIUS)
    proven = np.zeros((P, W))
    if delta is not None:
        for p in range(P):
            proven[p, :length[p]] = blend_fractions(arm, way[p, :length[p]], delta, spheres, radius)
    fractions = proven.copy()
    verified = np.zeros((P, W), bool)
    dev = default_device("trajectory") if field is None else field.dist2.device
    if blend is not None:
        want = min(max(nonneg("blend", blend), 0.0), 0.5)
        ask = [(p, k) for p in range(P) for k in range(1, length[p] - 1) if want > proven[p, k]]
        if ask:
            if not verify:
                raise ValueError("a blend above the proven fractions needs verify=True")
            if field is None and motion_kw.get("pairs") is False:
                raise ValueError("verify=True needs a field or a self test")
            c, f, r = _arm._self_set(arm, spheres, radius)
            reach = _arm.reach_table(arm, c, f)
            pts = np.stack([blend_chords(way[p], k, want, steps) for p, k in ask])           # (B, steps + 1, J)
            # a chord of parameter length D = 2 f / steps leaves its parabola by |q''| D^2 / 8 per joint
            qpp = np.stack([(way[p, k + 1] - 2.0 * way[p, k] + way[p, k - 1]) / (2.0 * want) for p, k in ask])
            sag = float((np.abs(qpp) @ reach).max() * (2.0 * want / steps) ** 2 / 8.0) if reach.shape[1] else 0.0
            kw = dict(motion_kw)
            kw["margin"] = kw.get("margin", 0.0) + sag
            kw["self_margin"] = kw.get("self_margin", 0.0) + 2.0 * sag
            mo = _arm.motion(arm, to_device(pts[:, :-1].reshape(-1, J), torch.float64, dev),
                             to_device(pts[:, 1:].reshape(-1, J), torch.float64, dev), field, **kw)
            good = mo.ok.reshape(len(ask), steps).all(dim=1).cpu().numpy()
            for (p, k), g in zip(ask, good):
                if g:
                    fractions[p, k], verified[p, k] = want, True
    law = time_paths(to_device(way, torch.float64, dev), to_device(length, torch.int32, dev),
                     to_device(fractions, torch.float64, dev), limits, steps)
    s = sample(law, dt, num_samples)
    return Trajectory(np.arange(s.q.shape[1]) * float(dt), s.q, s.qd, s.qdd, s.num, law.duration, fractions, verified,
                      law.status, law)


@dataclass
class Timed:
    duration: np.ndarray   # float64 per candidate; inf where there is no route
    best: np.ndarray       # int64 along the last axis: the quickest candidate, the lowest index of equals; -1: none
    trajectory: Optional[Trajectory]


def _timed(arm: Arm, routes: List, shape: Tuple[int, int], limits: Limits, kw) -> Timed:
    have = [i for i, r in enumerate(routes) if r is not None]
    duration = np.full(shape[0] * shape[1], np.inf)
    traj = None
    if have:
        traj = plan_trajectories(arm, [routes[i] for i in have], limits, num_samples=1, **kw)
        d = traj.duration.cpu().numpy()
        duration[have] = np.where(traj.status.cpu().numpy() == OK, d, np.inf)
    duration = duration.reshape(shape)
    best = np.where(np.isfinite(duration).any(axis=1), np.argmin(duration, axis=1), -1).astype(np.int64)
    return Timed(duration, best, traj)


def time_plan(plan, limits: Limits, arm: Optional[Arm] = None, **kw) -> Timed:
    """Durations (A, B) of a roadmap.Plan's routes and the quickest goal of every start.  Neither the Plan nor its
    order by metric length changes.  kw: plan_trajectories' keywords."""
    arm = arm if arm is not None else plan.roadmap.arm
    A, B = plan.cost.shape
    return _timed(arm, [plan.routes[a][b] for a in range(A) for b in range(B)], (A, B), limits, kw)


def time_reach(reach_result, limits: Limits, arm: Arm, **kw) -> Timed:
    """Durations (P, S) of the followed paths of an arm.Reach (every seed that follows its whole path) and the quickest
    seed of every path.  Neither the Reach nor the choice `arm.select` made changes."""
    q = reach_result.follow.q
    P, S, W, _ = q.shape
    whole = (reach_result.follow.first_fail == W).cpu().numpy()
    qh = q.cpu().numpy()
    return _timed(arm, [qh[p, s] if whole[p, s] else None for p in range(P) for s in range(S)], (P, S), limits, kw)


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def load_waypoints(path: str, J: int) -> List[np.ndarray]:
    """Routes from a .npy (n, J) or (..., n, J), or from the `waypoints` array of `roadmap plan`'s report, NaN padding
    included; routes that are all NaN (no route) are left out."""
    a = np.load(path)
    if hasattr(a, "files"):
        if "waypoints" not in a.files:
            raise ValueError(f"{path}: no array named waypoints")
        a = a["waypoints"]
    a = np.asarray(a, np.float64)
    if a.ndim < 2 or a.shape[-1] != J:
        raise ValueError(f"{path}: expected (..., n, {J}) waypoints, got {a.shape}")
    rows = [dedupe(r) for r in a.reshape(-1, a.shape[-2], J)]
    return [r for r in rows if len(r)]


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.trajectory",
                                 description="Time joint-space routes under joint limits and sample them at a fixed "
                                             "rate.")
    ap.add_argument("--arm", required=True, metavar="{default,FILE.json}", help="the arm model")
    ap.add_argument("--waypoints", required=True, help=".npy (n, J) / (..., n, J), or the .npz of roadmap plan")
    ap.add_argument("--limits", default="default", metavar="{default,FILE.json}", help="v_max and a_max per joint")
    ap.add_argument("--vel-scale", type=float, default=1.0, help="factor in (0, 1] on the velocity limits")
    ap.add_argument("--acc-scale", type=float, default=1.0, help="factor in (0, 1] on the acceleration limits")
    ap.add_argument("--dt", type=float, default=DT, help="the controller's period, seconds")
    ap.add_argument("--steps", type=int, default=STEPS, help="grid intervals per piece of the path")
    ap.add_argument("--delta", type=float, default=None, help="blend as far as keeps every sphere within this of the "
                                                              "checked polyline's sweep, metres")
    ap.add_argument("--blend", type=float, default=None, help="blend fraction asked for; verified against --field")
    ap.add_argument("--field", default=None, help=".npz of python -m gaussiangrasper_amd.field (--out)")
    ap.add_argument("--margin", type=float, default=0.0, help="clearance kept beyond the spheres (with --blend)")
    ap.add_argument("--self-margin", type=float, default=0.0, help="gap kept between the arm's own spheres")
    ap.add_argument("--motion-res", type=float, default=None, help="as python -m gaussiangrasper_amd.roadmap")
    ap.add_argument("--out", required=True, help="output .npz t, q, qd, qdd, num, duration, fractions, verified, status")
    a = ap.parse_args(argv)
    if not 2 <= a.steps <= MAX_STEPS:
        ap.error(f"--steps must be in 2..{MAX_STEPS}, got {a.steps}")
    if not (math.isfinite(a.dt) and a.dt > 0.0):
        ap.error(f"--dt must be finite and > 0, got {a.dt}")
    if a.blend is not None and not a.field and a.motion_res is None:
        ap.error("--blend needs --field or --motion-res")
    try:
        arm = _arm.load_arm_option(a.arm)
        limits = load_limits_option(a.limits).scaled(a.vel_scale, a.acc_scale)
        routes = load_waypoints(a.waypoints, arm.num_joints)
        field = None
        if a.field:
            from .field import DistanceField
            field = DistanceField.load(a.field)
        kw = {}
        if a.blend is not None:
            kw = dict(margin=a.margin, self_margin=a.self_margin, res=a.motion_res)
        tr = plan_trajectories(arm, routes, limits, field, blend=a.blend, delta=a.delta, dt=a.dt, steps=a.steps,
                               verify=a.blend is not None, **kw)
        np.savez(a.out, t=tr.t, q=tr.q.cpu().numpy(), qd=tr.qd.cpu().numpy(), qdd=tr.qdd.cpu().numpy(),
                 num=tr.num.cpu().numpy(), duration=tr.duration.cpu().numpy(), fractions=tr.fractions,
                 verified=tr.verified, status=tr.status.cpu().numpy())
    except (KeyError, ValueError, OSError, _lib.GGError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    d = tr.duration.cpu().numpy()
    ok = tr.status.cpu().numpy() == OK
    print(f"{int(ok.sum())} of {len(d)} routes timed, the longest {float(d[ok].max()) if ok.any() else 0.0:.4f} s; "
          f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
