"""Arm reachability: which gripper poses a serial arm can reach, in which joint configuration, and whether the whole
arm stays clear of the scene's distance field on the way.  Forward kinematics (`gg_arm_fk`), inverse kinematics along
pose paths by damped least squares with error-proportional damping (`gg_arm_follow`) and the arm's link spheres
against the field (`gg_arm_clear`), csrc/arm.hip.  The contract is in include/gg_raster.h and PARITY.md "Arm
reachability"; the design in DESIGN.md §3.31.

    Arm                the chain: base, fixed transforms, joints, link spheres; to_array / to_json / from_json / with_base
    default_arm        a 7-joint chain from the Franka Panda's modified DH table and limits AS RECALLED (UNVERIFIED)
    seeds              (P, S, J) start configurations: the home configuration first, the others uniform in the limits
    fk / follow / clear   the three calls as they are (no CPU path)
    select             the seed of every path: reachable, clear, smallest joint jump, lowest index
    reach              follow, clear and select for (P, W, 12) gripper pose paths -> Reach
    reach_grasps       reach on field.approach_paths of grasp rows, and a row mask for grasp.filter_grasps
    python -m gaussiangrasper_amd.arm --arm {default,FILE.json} (--grasps G.npy --standoff D --steps N | --poses P.npy)
                                      [--field field.npz --radius R --margin M] --out q.npy --report r.npz

Out of scope: self-collision, a joint-space planner between configurations, velocity and torque limits.  The spheres
cover the link models they are given and nothing more."""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass, field as _dc_field, replace
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._call import (ArrayLike, check_finite_options, default_device, host_array, host_ptr, nonneg, positive,
                    ptr as _ptr, require_hip as _require_hip, stream as _stream, to_device)
# GG_FIELD_FAR, GG_FIELD_MAX_SPHERES, GG_FIELD_MAX_POSES, and the argument checks of the calls on the volume
from .field import (FAR, MAX_POSES, MAX_SPHERES, DistanceField, approach_paths, cell_count, gripper_spheres, need2,
                    pose_paths, sphere_table, volume_args, volume_tensor)

MAX_JOINTS = 8                 # GG_ARM_MAX_JOINTS
MAX_ITER = 1024                # GG_ARM_MAX_ITER
ORTHO_TOL = 1e-9
# This project's choices (PARITY.md "Arm reachability"); none has been measured on a robot
IK_DEFAULTS = dict(tol_p=1e-4, tol_r=1e-3, L=0.1, k=1.0, lambda_min=1e-4, max_step=0.2, max_iter=100)
NUM_SEEDS = 16
SPHERE_RADIUS = 0.005          # of the optional gripper-frame spheres, as field.path_clear's command line has it

# The Franka Panda AS RECALLED (UNVERIFIED, PARITY.md "Arm reachability"): modified (Craig) DH rows a_{i-1}, d_i,
# alpha_{i-1} in quarter turns, then the flange; joint limits in radians
PANDA_DH = ((0.0, 0.333, 0), (0.0, 0.0, -1), (0.0, 0.316, 1), (0.0825, 0.0, 1), (-0.0825, 0.384, -1), (0.0, 0.0, 1),
            (0.088, 0.0, 1))
PANDA_FLANGE = 0.107           # d of the flange frame beyond joint 7
PANDA_HAND = 0.1034            # flange to the point between the fingertips, along the flange's z, as recalled
PANDA_HAND_YAW = -math.pi / 4  # the hand is mounted turned about the flange's z, as recalled
PANDA_LIMITS = ((-2.8973, 2.8973), (-1.7628, 1.7628), (-2.8973, 2.8973), (-3.0718, -0.0698), (-2.8973, 2.8973),
                (-0.0175, 3.7525), (-2.8973, 2.8973))
# link spheres [frame, x, y, z, radius]: a handful per link, centres on the link's line in its own frame, radii chosen
# by hand to hold the link's drawing as recalled
PANDA_SPHERES = (
    (0, 0.0, 0.0, 0.05, 0.11), (0, -0.07, 0.0, 0.05, 0.09),
    (1, 0.0, 0.0, -0.19, 0.09), (1, 0.0, 0.0, -0.095, 0.09), (1, 0.0, 0.0, 0.0, 0.09),
    (2, 0.0, -0.07, 0.0, 0.09), (2, 0.0, -0.14, 0.0, 0.09),
    (3, 0.0, 0.0, -0.09, 0.085), (3, 0.0, 0.0, 0.0, 0.085), (3, 0.0825, 0.0, 0.0, 0.08),
    (4, -0.0825, 0.095, 0.0, 0.075), (4, -0.0825, 0.19, 0.0, 0.07), (4, -0.0825, 0.285, 0.0, 0.07),
    (5, 0.0, 0.0, -0.06, 0.075), (5, 0.0, 0.0, 0.0, 0.075),
    (6, 0.0, 0.0, 0.0, 0.07), (6, 0.088, 0.0, 0.0, 0.065),
    (7, 0.0, 0.0, 0.06, 0.06), (7, 0.0, 0.0, 0.13, 0.06),
)

IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


def arm_doubles(num_joints: int) -> int:
    """GG_ARM_DOUBLES(J)"""
    return 12 * (num_joints + 2) + 6 * num_joints


def pose12(T: ArrayLike) -> np.ndarray:
    """A rigid transform given as 12 numbers (R row-major, then t), (3, 4) or (4, 4), as float64 (12,)."""
    a = np.asarray(T, np.float64)
    if a.shape == (12,):
        return a.copy()
    if a.shape in ((3, 4), (4, 4)):
        return np.concatenate([a[:3, :3].reshape(-1), a[:3, 3]])
    raise ValueError(f"a transform is 12 numbers (R row-major, then t), (3, 4) or (4, 4); got {a.shape}")


def _check_rotation(name: str, T: np.ndarray) -> None:
    R = T[:9].reshape(3, 3)
    if not np.isfinite(T).all():
        raise ValueError(f"{name} has an entry that is not finite")
    if not np.abs(R.T @ R - np.eye(3)).max() <= ORTHO_TOL:
        raise ValueError(f"{name}: |R^T R - I|max > {ORTHO_TOL}")


@dataclass
class Arm:
    """A serial chain of J joints.  base (12,): world from arm base; fixed (J + 1, 12): A_j from link j to joint j at
    q_j = 0, the last one from the last link to the gripper frame (R row-major, then t, each); axis (J, 3) unit
    vectors in the joint frames; lo, hi (J,); kind (J,) 0 revolute, 1 prismatic; spheres (K, 5) rows [frame, x, y,
    z, radius] with frame in 0..J + 1, the link models' cover."""
    base: np.ndarray
    fixed: np.ndarray
    axis: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    kind: np.ndarray
    spheres: np.ndarray = _dc_field(default_factory=lambda: np.zeros((0, 5)))

    @property
    def num_joints(self) -> int:
        return int(np.asarray(self.axis).reshape(-1, 3).shape[0])

    def to_array(self) -> np.ndarray:
        """The host array the C entries take (GG_ARM_DOUBLES(J) float64), after the checks they make: ValueError
        naming the field."""
        axis = np.asarray(self.axis, np.float64)
        if axis.ndim != 2 or axis.shape[1] != 3 or not 1 <= axis.shape[0] <= MAX_JOINTS:
            raise ValueError(f"axis must be (J, 3) with J in 1..{MAX_JOINTS}, got {axis.shape}")
        J = axis.shape[0]
        base = np.asarray(self.base, np.float64)
        fixed = np.asarray(self.fixed, np.float64)
        lo, hi, kind = (np.asarray(v, np.float64) for v in (self.lo, self.hi, self.kind))
        if base.shape != (12,):
            raise ValueError(f"base must be (12,), got {base.shape}")
        if fixed.shape != (J + 1, 12):
            raise ValueError(f"fixed must be ({J + 1}, 12) for {J} joints, got {fixed.shape}")
        if lo.shape != (J,) or hi.shape != (J,) or kind.shape != (J,):
            raise ValueError(f"lo, hi and kind must be ({J},), got {lo.shape}, {hi.shape}, {kind.shape}")
        _check_rotation("base", base)
        for j in range(J + 1):
            _check_rotation(f"fixed[{j}]", fixed[j])
        for j in range(J):
            if not np.isfinite(axis[j]).all():
                raise ValueError(f"axis[{j}] has an entry that is not finite")
            if not abs(float(axis[j] @ axis[j]) - 1.0) <= ORTHO_TOL:
                raise ValueError(f"axis[{j}]: the squared length is off 1 by more than {ORTHO_TOL}")
            if not (np.isfinite(lo[j]) and np.isfinite(hi[j])):
                raise ValueError(f"lo[{j}] / hi[{j}] is not finite")
            if lo[j] > hi[j]:
                raise ValueError(f"lo[{j}] > hi[{j}]")
            if kind[j] not in (0.0, 1.0):
                raise ValueError(f"kind[{j}] must be 0 (revolute) or 1 (prismatic), got {kind[j]}")
        joints = np.concatenate([axis, lo[:, None], hi[:, None], kind[:, None]], 1)
        out = np.concatenate([base, fixed.reshape(-1), joints.reshape(-1)])
        assert out.shape == (arm_doubles(J),)
        return np.ascontiguousarray(out)

    def link_spheres(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(centres (K, 3) float32, frame (K,) int32, radius (K,) float64) of the link spheres, checked."""
        s = np.asarray(self.spheres, np.float64).reshape(-1, 5)
        J = self.num_joints
        if not np.isfinite(s).all():
            raise ValueError("spheres has an entry that is not finite")
        if len(s) and not ((s[:, 0] == np.round(s[:, 0])).all() and (s[:, 0] >= 0).all() and (s[:, 0] <= J + 1).all()):
            raise ValueError(f"spheres: the frame of a sphere must be an integer in 0..{J + 1}")
        if len(s) and not (s[:, 4] >= 0).all():
            raise ValueError("spheres: a radius is negative")
        return s[:, 1:4].astype(np.float32), s[:, 0].astype(np.int32), s[:, 4].copy()

    def with_base(self, T: ArrayLike) -> "Arm":
        """A copy of the arm standing at another base pose (12 numbers, (3, 4) or (4, 4))."""
        return replace(self, base=pose12(T))

    def home(self) -> np.ndarray:
        """The middle of the limits."""
        return 0.5 * (np.asarray(self.lo, np.float64) + np.asarray(self.hi, np.float64))

    def to_json(self, path: str) -> None:
        self.to_array()
        joints = np.concatenate([np.asarray(self.axis, np.float64), np.asarray(self.lo, np.float64)[:, None],
                                 np.asarray(self.hi, np.float64)[:, None], np.asarray(self.kind, np.float64)[:, None]], 1)
        with open(path, "w") as f:
            json.dump({"base": np.asarray(self.base, np.float64).tolist(),
                       "fixed": np.asarray(self.fixed, np.float64).tolist(), "joints": joints.tolist(),
                       "spheres": np.asarray(self.spheres, np.float64).reshape(-1, 5).tolist()}, f)

    @classmethod
    def from_json(cls, path: str) -> "Arm":
        """An arm from a JSON file of numbers only: base [12], fixed [J + 1][12], joints [J][6] (axis, lo, hi, kind),
        spheres [K][5] (frame, x, y, z, radius; may be missing).  ValueError naming the file and the field."""
        with open(path) as f:
            try:
                d = json.load(f)
            except json.JSONDecodeError as exc:
                raise ValueError(f"{path}: not JSON: {exc}") from exc
        try:
            if not isinstance(d, dict):
                raise ValueError("expected an object with base, fixed, joints and spheres")
            joints = np.asarray(d["joints"], np.float64)
            if joints.ndim != 2 or joints.shape[1] != 6:
                raise ValueError(f"joints must be (J, 6): axis, lo, hi, kind; got {joints.shape}")
            arm = cls(np.asarray(d["base"], np.float64), np.asarray(d["fixed"], np.float64), joints[:, :3],
                      joints[:, 3], joints[:, 4], joints[:, 5],
                      np.asarray(d.get("spheres", []), np.float64).reshape(-1, 5))
            arm.to_array()
            arm.link_spheres()
        except KeyError as exc:
            raise ValueError(f"{path}: {exc.args[0]} is missing") from exc
        except (TypeError, ValueError) as exc:
            raise ValueError(f"{path}: {exc}") from exc
        return arm


def dh_fixed(a: float, d: float, quarter_turns: int) -> np.ndarray:
    """The modified-DH link transform Rot_x(alpha) Trans_x(a) Trans_z(d) with alpha a whole number of quarter turns
    (its sine and cosine exact), as 12 numbers; the joint then turns about z."""
    c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[quarter_turns % 4]
    return np.array([1.0, 0.0, 0.0, 0.0, c, -s, 0.0, s, c, a, -s * d, c * d])


def default_arm() -> Arm:
    """The 7-joint chain of the Franka Panda from its modified DH table and joint limits AS RECALLED (UNVERIFIED,
    PARITY.md "Arm reachability"), standing at the world's origin.  The gripper frame sits between the fingertips,
    its axes approach, closing and height: the hand's z, y and -x."""
    fixed = [dh_fixed(*row) for row in PANDA_DH]
    c, s = math.cos(PANDA_HAND_YAW), math.sin(PANDA_HAND_YAW)
    # flange (z up the hand) -> hand (yaw) -> gripper frame (columns: the hand's z, y, -x)
    hand = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    to_gripper = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    fixed.append(np.concatenate([(hand @ to_gripper).reshape(-1), [0.0, 0.0, PANDA_FLANGE + PANDA_HAND]]))
    lim = np.array(PANDA_LIMITS)
    J = len(PANDA_DH)
    return Arm(IDENTITY.copy(), np.stack(fixed), np.tile([0.0, 0.0, 1.0], (J, 1)), lim[:, 0].copy(), lim[:, 1].copy(),
               np.zeros(J), np.array(PANDA_SPHERES, np.float64))


def load_arm_option(text: str) -> Arm:
    return default_arm() if text == "default" else Arm.from_json(text)


def seeds(arm: Arm, P: int, S: int, seed: int = 0, home: Optional[ArrayLike] = None) -> np.ndarray:
    """(P, S, J) float64 start configurations: seed 0 of every path is `home` (the middle of the limits when None),
    the others uniform within the limits from np.random.default_rng(seed)."""
    P, S = int(P), int(S)
    if P < 0 or S < 1:
        raise ValueError(f"need P >= 0 and S >= 1, got {P} and {S}")
    lo, hi = np.asarray(arm.lo, np.float64), np.asarray(arm.hi, np.float64)
    h = arm.home() if home is None else np.asarray(home, np.float64).reshape(-1)
    if h.shape != lo.shape or not np.isfinite(h).all():
        raise ValueError(f"home must be {lo.shape} finite numbers")
    out = np.empty((P, S, len(lo)))
    out[:, 0] = h
    out[:, 1:] = np.random.default_rng(seed).uniform(lo, hi, size=(P, S - 1, len(lo)))
    return out


# ------------------------------------------------------------------------------------------------
# device side: the three calls as they are
# ------------------------------------------------------------------------------------------------
@dataclass
class Follow:
    q: Tensor              # (P, S, W, J) float64; NaN from a failed waypoint on
    iters: Tensor          # (P, S, W) int32 updates taken; -1 from a failed waypoint on
    resid: Tensor          # (P, S, W, 2) float64 |e_p|, |e_r| at convergence
    first_fail: Tensor     # (P, S) int32 the first failed waypoint, W when there is none


def _arm_args(arm: Union[Arm, np.ndarray], num_joints: Optional[int] = None):
    a = arm.to_array() if isinstance(arm, Arm) else np.ascontiguousarray(np.asarray(arm, np.float64).reshape(-1))
    J = arm.num_joints if isinstance(arm, Arm) else int(num_joints)
    if a.shape != (arm_doubles(J),):
        raise ValueError(f"an arm of {J} joints is {arm_doubles(J)} doubles, got {a.shape}")
    return J, a


def _q_rows(q: Tensor, J: int) -> Tensor:
    if q.dtype != torch.float64 or q.ndim != 2 or q.shape[1] != J:
        raise ValueError(f"q must be a float64 (M, {J}) tensor, got {q.dtype} {tuple(q.shape)}")
    return q.contiguous()


def fk(arm: Arm, q: Tensor) -> Tensor:
    """frames (M, J + 2, 12) float64 of one gg_arm_fk call: F_0 .. F_{J+1} of every row of q (M, J) float64 on the HIP
    device (no CPU path).  The last frame is the gripper pose.  Limits are not applied."""
    dev = _require_hip(q)
    J, a = _arm_args(arm)
    q = _q_rows(q, J)
    m = q.shape[0]
    if m > MAX_POSES:
        raise ValueError(f"{m} rows are more than {MAX_POSES}")
    frames = torch.empty(m, J + 2, 12, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().gg_arm_fk(J, host_ptr(a), m, _ptr(q), _ptr(frames), _stream(dev)), "gg_arm_fk")
    return frames


def follow(arm: Arm, poses: Tensor, seeds: Tensor, tol_p: float = IK_DEFAULTS["tol_p"],
           tol_r: float = IK_DEFAULTS["tol_r"], L: float = IK_DEFAULTS["L"], k: float = IK_DEFAULTS["k"],
           lambda_min: float = IK_DEFAULTS["lambda_min"], max_step: float = IK_DEFAULTS["max_step"],
           max_iter: int = IK_DEFAULTS["max_iter"]) -> Follow:
    """One gg_arm_follow call: poses (P, W, 12) float32 gripper poses and seeds (P, S, J) float64 on the HIP device
    (no CPU path).  Every (path, seed) follows its path on its own, each waypoint from the solution of the one before."""
    dev = _require_hip(poses, seeds)
    J, a = _arm_args(arm)
    poses = pose_paths(poses)
    p, w = poses.shape[:2]
    if seeds.dtype != torch.float64 or seeds.ndim != 3 or seeds.shape[0] != p or seeds.shape[2] != J:
        raise ValueError(f"seeds must be a float64 ({p}, S, {J}) tensor, got {seeds.dtype} {tuple(seeds.shape)}")
    s = seeds.shape[1]
    if p * s * max(w, 1) > MAX_POSES:
        raise ValueError(f"{p} paths x {s} seeds x {w} waypoints are more than {MAX_POSES}")
    if not 0 <= int(max_iter) <= MAX_ITER:
        raise ValueError(f"max_iter must be in 0..{MAX_ITER}, got {max_iter}")
    seeds = seeds.contiguous()
    q = torch.empty(p, s, w, J, dtype=torch.float64, device=dev)
    iters = torch.empty(p, s, w, dtype=torch.int32, device=dev)
    resid = torch.empty(p, s, w, 2, dtype=torch.float64, device=dev)
    first = torch.empty(p, s, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_arm_follow(J, host_ptr(a), p, w, _ptr(poses), s, _ptr(seeds), nonneg("tol_p", tol_p),
                                         nonneg("tol_r", tol_r), positive("L", L), nonneg("k", k),
                                         positive("lambda_min", lambda_min), positive("max_step", max_step),
                                         int(max_iter), _ptr(q), _ptr(iters), _ptr(resid), _ptr(first), _stream(dev)),
               "gg_arm_follow")
    return Follow(q, iters, resid, first)


def clear(arm: Arm, dist2: Tensor, grid, dims, q: Tensor, spheres: Tensor, frame: Tensor, need: Tensor,
          outside: int = FAR) -> Tuple[Tensor, Tensor]:
    """(slack (M,) int32, worst (M,) int32) of one gg_arm_clear call.  q (M, J) float64, spheres (S, 3) float32 centres,
    frame (S,) int32 in 0..J + 1 (J + 1: the gripper frame), need (S,) int32 in 0..FAR, dist2 int32 [X][Y][Z]: on the
    HIP device (no CPU path)."""
    dev = _require_hip(dist2, q, spheres, frame, need)
    J, a = _arm_args(arm)
    d, g, shape = volume_args(dims, grid)
    volume_tensor(dist2, "dist2", torch.int32, shape)
    q = _q_rows(q, J)
    spheres, frame, need = sphere_table(spheres, frame=frame, need=need)
    m = q.shape[0]
    if m > MAX_POSES:
        raise ValueError(f"{m} rows are more than {MAX_POSES}")
    slack = torch.empty(m, dtype=torch.int32, device=dev)
    worst = torch.empty(m, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_arm_clear(J, host_ptr(a), d, g, _ptr(dist2), m, _ptr(q), spheres.shape[0], _ptr(spheres),
                                        _ptr(frame), _ptr(need), cell_count("outside", outside), _ptr(slack),
                                        _ptr(worst), _stream(dev)), "gg_arm_clear")
    return slack, worst


# ------------------------------------------------------------------------------------------------
# the task layer
# ------------------------------------------------------------------------------------------------
@dataclass
class Reach:
    q: Tensor              # (P, W, J) float64 the chosen seed's configurations; NaN where no seed follows the path
    reachable: Tensor      # (P,) bool: a seed follows the whole path
    clear: Tensor          # (P,) bool: a seed follows the whole path with every slack >= 0 (the row mask)
    seed: Tensor           # (P,) int64 the chosen seed; -1 when not reachable
    slack: Tensor          # (P, W) int32 of the chosen seed (FAR without a field; INT32_MIN where q is NaN)
    worst: Tensor          # (P, W) int32 the sphere of that slack: the arm's link spheres first, then `spheres`
    jump: Tensor           # (P,) float64 max_w |q_w - q_{w-1}|inf of the chosen seed, waypoint 0 against home; inf
    follow: Follow         # the raw outputs, every seed
    slack_all: Tensor      # (P, S, W) int32
    worst_all: Tensor      # (P, S, W) int32


def select(first_fail: ArrayLike, num_waypoints: int, clear_ok: ArrayLike, jump: ArrayLike):
    """(seed (P,) int64, reachable (P,) bool, clear (P,) bool), numpy.  first_fail (P, S), clear_ok (P, S) bool (every
    slack of the seed >= 0), jump (P, S).  The chosen seed is, among those with first_fail == W and clear_ok, the one
    of the smallest jump, the lowest index of equals; when no seed is both, the same choice among those with
    first_fail == W (the path is reachable, not clear); -1 when there is none."""
    ff = np.asarray(first_fail, np.int64)
    ok = ff == int(num_waypoints)
    both = ok & np.asarray(clear_ok, bool)
    if ff.shape[1] == 0:
        none = np.zeros(len(ff), bool)
        return np.full(len(ff), -1, np.int64), none, none.copy()
    pick = np.where(both.any(1)[:, None], both, ok)
    key = np.where(pick, np.asarray(jump, np.float64), np.inf)      # a seed that follows its path has a finite jump
    seed = np.argmin(key, axis=1)                                   # the first of equals
    reachable = ok.any(1)
    return np.where(reachable, seed, -1).astype(np.int64), reachable, both.any(1)


def _sphere_set(arm: Arm, spheres, radius, margin: float, h: float):
    """centres, frames and need2 of the arm's link spheres followed by the gripper-frame `spheres` of `radius`"""
    c, f, r = arm.link_spheres()
    if spheres is not None:
        sp = host_array(spheres, np.float32).reshape(-1, 3)
        c = np.concatenate([c, sp])
        f = np.concatenate([f, np.full(len(sp), arm.num_joints + 1, np.int32)])
        r = np.concatenate([r, np.broadcast_to(np.asarray(radius, np.float64), (len(sp),))])
    if len(c) > MAX_SPHERES:
        raise ValueError(f"{len(c)} spheres with the arm's are more than {MAX_SPHERES}: use a larger radius")
    return c, f, need2(r, margin, h) if len(c) else np.zeros(0, np.int32)


def _reach(arm: Arm, poses: Tensor, field, sphere_sets, radius, margin: float, num_seeds: int, seed: int,
           home, outside: str, ik) -> Reach:
    """reach for paths whose gripper-frame spheres differ: sphere_sets is a list of (path indices, spheres or None)
    that covers every path once."""
    if outside not in ("free", "blocked"):
        raise ValueError(f"outside must be 'free' or 'blocked', got {outside!r}")
    dev = poses.device
    J = arm.num_joints
    p, w = poses.shape[:2]
    h0 = arm.home() if home is None else np.asarray(home, np.float64).reshape(-1)
    sd = to_device(seeds(arm, p, num_seeds, seed, h0), torch.float64, dev)
    fol = follow(arm, poses, sd, **ik)
    s = sd.shape[1]
    slack_all = torch.full((p, s, w), FAR, dtype=torch.int32, device=dev)
    worst_all = torch.full((p, s, w), -1, dtype=torch.int32, device=dev)
    if field is not None and p * s * w:
        for rows, sp in sphere_sets:
            c, f, need = _sphere_set(arm, sp, radius, margin, field.h)
            idx = torch.as_tensor(np.asarray(rows, np.int64), device=dev)
            sl, wo = clear(arm, field.dist2, field.grid, field.dims, fol.q[idx].reshape(-1, J),
                           to_device(c, torch.float32, dev).reshape(-1, 3), to_device(f, torch.int32, dev),
                           to_device(need, torch.int32, dev), FAR if outside == "free" else 0)
            slack_all[idx] = sl.reshape(len(idx), s, w)
            worst_all[idx] = wo.reshape(len(idx), s, w)
    jump_all = torch.zeros(p, s, dtype=torch.float64, device=dev)
    if w:
        prev = torch.cat([to_device(h0, torch.float64, dev).expand(p, s, 1, J), fol.q[:, :, :-1]], 2)
        jump_all = (fol.q - prev).abs().amax(-1).amax(-1)           # NaN for a seed that fails: never picked
    clear_ok = (slack_all >= 0).all(-1)
    pick, reachable, ok = select(fol.first_fail.cpu().numpy(), w, clear_ok.cpu().numpy(), jump_all.cpu().numpy())
    at = torch.as_tensor(np.maximum(pick, 0), device=dev)
    rows = torch.arange(p, device=dev)
    none = torch.as_tensor(pick < 0, device=dev)
    q = fol.q[rows, at]
    q = torch.where(none[:, None, None], torch.full_like(q, math.nan), q)
    jump = torch.where(none, torch.full((p,), math.inf, dtype=torch.float64, device=dev), jump_all[rows, at])
    return Reach(q, torch.as_tensor(reachable, device=dev), torch.as_tensor(ok, device=dev),
                 torch.as_tensor(pick, device=dev), slack_all[rows, at], worst_all[rows, at], jump, fol, slack_all,
                 worst_all)


def reach(arm: Arm, poses: ArrayLike, field=None, spheres: Optional[ArrayLike] = None,
          radius: Union[float, ArrayLike] = SPHERE_RADIUS, margin: float = 0.0, num_seeds: int = NUM_SEEDS,
          seed: int = 0, home: Optional[ArrayLike] = None, outside: str = "free", **ik) -> Reach:
    """Which of the (P, W, 12) gripper pose paths the arm can follow, in which configurations, and whether the whole
    arm stays clear of `field` (a field.DistanceField after update(); None: no clearance test) on the way: follow from
    num_seeds seeds per path (`seeds`), clear of every configuration with the arm's link spheres plus the optional
    gripper-frame `spheres` of `radius` (field.gripper_spheres, transit.carried_spheres), kept `margin` away, and
    `select`.  **ik: follow's parameters."""
    dev = default_device("arm") if field is None else field.dist2.device
    p = to_device(poses, torch.float32, dev)
    if p.ndim != 3 or p.shape[2] != 12:
        raise ValueError(f"poses must be (P, W, 12), got {tuple(p.shape)}")
    return _reach(arm, p, field, [(np.arange(p.shape[0]), spheres)], radius, margin, num_seeds, seed, home, outside, ik)


def reach_grasps(arm: Arm, rows: ArrayLike, standoff: float, steps: int, field=None,
                 gripper: Optional[ArrayLike] = None, radius: float = SPHERE_RADIUS, margin: float = 0.0,
                 num_seeds: int = NUM_SEEDS, seed: int = 0, home: Optional[ArrayLike] = None, outside: str = "free",
                 **ik) -> Tuple[Reach, Tensor]:
    """`reach` on the straight approach of every (M, 17) grasp row (field.approach_paths(rows, standoff, steps)), and
    the (M,) bool row mask grasp.filter_grasps accepts: the arm follows the whole approach and stays clear.  With a
    `gripper` model (grasp.default_gripper, ...) its spheres of `radius` ride on the gripper frame at each row's
    width, depth and height; leave it None when the field holds the object to be grasped, which the fingers touch at
    the last waypoint (field.py's note on the grasp pose)."""
    g = host_array(rows, np.float64)
    poses = approach_paths(g, standoff, steps)
    dev = default_device("arm") if field is None else field.dist2.device
    if gripper is None or field is None:
        sets = [(np.arange(len(g)), None)]
    else:
        sizes, inverse = np.unique(g[:, [1, 3, 2]], axis=0, return_inverse=True)       # width, depth, height
        inverse = np.asarray(inverse).reshape(-1)
        sets = [(np.nonzero(inverse == i)[0], gripper_spheres(gripper, *sizes[i], radius)) for i in range(len(sizes))]
    res = _reach(arm, to_device(poses, torch.float32, dev), field, sets, radius, margin, num_seeds, seed, home,
                 outside, ik)
    return res, res.clear


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def main(argv: Optional[Sequence[str]] = None) -> int:
    from .grasp import load_grasps
    ap = argparse.ArgumentParser(prog="python -m gaussiangrasper_amd.arm",
                                 description="Which gripper poses an arm reaches, in which joint configurations, and "
                                             "whether the whole arm stays clear of a saved distance field.")
    ap.add_argument("--arm", required=True, metavar="{default,FILE.json}", help="the arm model")
    ap.add_argument("--base", default=None, help=".npy (12,), (3, 4) or (4, 4): scene from arm base")
    ap.add_argument("--grasps", default=None, help=".npy (M, 17) grasp rows, scene frame: their straight approaches")
    ap.add_argument("--standoff", type=float, default=None, help="with --grasps: the approach starts this far back")
    ap.add_argument("--steps", type=int, default=None, help="with --grasps: waypoints per approach")
    ap.add_argument("--poses", default=None, help=".npy (P, W, 12) gripper poses, scene frame: R row-major, then t")
    ap.add_argument("--field", default=None, help=".npz of python -m gaussiangrasper_amd.field (--out)")
    ap.add_argument("--radius", type=float, default=SPHERE_RADIUS, help="radius of gripper-frame spheres (--spheres)")
    ap.add_argument("--margin", type=float, default=0.0, help="clearance kept beyond the spheres")
    ap.add_argument("--spheres", default=None, help=".npy (S, 3) further sphere centres, gripper frame")
    ap.add_argument("--seeds", type=int, default=NUM_SEEDS, help="start configurations per path")
    ap.add_argument("--seed", type=int, default=0, help="of the random start configurations")
    ap.add_argument("--max-iter", type=int, default=IK_DEFAULTS["max_iter"], help="updates per waypoint at most")
    ap.add_argument("--out", required=True, help="output .npy (P, W, J) joint configurations (NaN: not reachable)")
    ap.add_argument("--report", required=True, help="output .npz reachable, clear, seed, slack, worst, jump, "
                                                    "first_fail, iters")
    a = ap.parse_args(argv)
    if bool(a.grasps) == bool(a.poses):
        ap.error("give --grasps (with --standoff and --steps) or --poses")
    if a.grasps and (a.standoff is None or a.steps is None):
        ap.error("--grasps needs --standoff and --steps")
    if a.poses and (a.standoff is not None or a.steps is not None):
        ap.error("--standoff and --steps go with --grasps")
    if a.spheres and not a.field:
        ap.error("--spheres needs --field")
    check_finite_options(ap, a, positive=("radius",), nonneg=("margin",))
    if a.seeds < 1:
        ap.error(f"--seeds must be >= 1, got {a.seeds}")
    if not 0 <= a.max_iter <= MAX_ITER:
        ap.error(f"--max-iter must be in 0..{MAX_ITER}, got {a.max_iter}")
    try:
        arm = load_arm_option(a.arm)
        if a.base:
            arm = arm.with_base(np.load(a.base))
            arm.to_array()
        spheres = np.asarray(np.load(a.spheres), np.float32).reshape(-1, 3) if a.spheres else None
        field = DistanceField.load(a.field) if a.field else None
        kw = dict(field=field, radius=a.radius, margin=a.margin, num_seeds=a.seeds, seed=a.seed, max_iter=a.max_iter)
        if a.grasps:
            poses =approach_paths(load_grasps(a.grasps), a.standoff, a.steps)
        else:
            poses = np.asarray(np.load(a.poses), np.float32)
            if poses.ndim != 3 or poses.shape[2] != 12:
                raise ValueError(f"{a.poses}: expected (P, W, 12) poses, got {poses.shape}")
        res = reach(arm, poses, spheres=spheres, **kw)
        np.save(a.out, res.q.cpu().numpy())
        np.savez(a.report, reachable=res.reachable.cpu().numpy(), clear=res.clear.cpu().numpy(),
                 seed=res.seed.cpu().numpy(), slack=res.slack.cpu().numpy(), worst=res.worst.cpu().numpy(),
                 jump=res.jump.cpu().numpy(), first_fail=res.follow.first_fail.cpu().numpy(),
                 iters=res.follow.iters.cpu().numpy())
    except (KeyError, ValueError, OSError, _lib.GGError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    print(f"{int(res.reachable.sum())} of {poses.shape[0]} paths reachable, {int(res.clear.sum())} clear"
          + ("" if field is not None else " (no field: clearance not tested)") + f"; wrote {a.out} and {a.report}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
