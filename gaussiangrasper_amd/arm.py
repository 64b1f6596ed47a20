"""Arm reachability: which gripper poses a serial arm can reach, in which joint configuration, and whether the whole
arm stays clear of the scene's distance field on the way.  Forward kinematics (`gg_arm_fk`), inverse kinematics along
pose paths by damped least squares with error-proportional damping (`gg_arm_follow`) and the arm's link spheres
against the field (`gg_arm_clear`), the arm against itself (`gg_arm_self`) and straight joint-space moves against both
(`gg_arm_motion`), csrc/arm.hip.  The contract is in include/gg_raster.h and PARITY.md "Arm reachability"; the design
in DESIGN.md §3.31 and §3.33.

    Arm                the chain: base, fixed transforms, joints, link spheres; to_array / to_json / from_json / with_base
    default_arm        a 7-joint chain from the Franka Panda's modified DH table and limits AS RECALLED (UNVERIFIED)
    seeds              (P, S, J) start configurations: the home configuration first, the others uniform in the limits
    fk / follow / clear   the three calls as they are (no CPU path)
    select             the seed of every path: reachable, clear, smallest joint jump, lowest index
    reach_table        the bound on every sphere centre's speed per joint that gg_arm_motion samples by
    default_self_pairs which frames' spheres are tested against each other: not adjacent, not always overlapping
    self_gap / motion  the two calls as they are (no CPU path); Motion.ok is the verdict for the whole move
    reach              follow, clear and select for (P, W, 12) gripper pose paths -> Reach; motion=True also tests
                       the moves between waypoints and self-collision
    connect            a clear straight move between configurations, or one through a via configuration
    reach_grasps       reach on field.approach_paths of grasp rows, and a row mask for grasp.filter_grasps
    python -m gaussiangrasper_amd.arm --arm {default,FILE.json} (--grasps G.npy --standoff D --steps N | --poses P.npy)
                                      [--field field.npz --radius R --margin M] --out q.npy --report r.npz
                                      [--check-motion --motion-res R --self-margin M --max-samples N]
                                      [--connect-from Q.npy [--connect-roadmap {N,FILE.npz}]]

Routes through more than one intermediate configuration are roadmap.py's (a probabilistic roadmap over `motion`); when
the arm is where along them, inside joint velocity and acceleration limits, is trajectory.py's.  Out of scope: torque
limits and jerk.  The spheres cover the link models they are given and nothing more."""
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
MAX_SELF_SPHERES = 256         # GG_ARM_MAX_SELF_SPHERES
MAX_SAMPLES = 4096             # GG_ARM_MAX_SAMPLES
NUM_VIAS = 64                  # connect's via configurations, the home configuration among them: this project's choice
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
    z, radius] with frame in 0..J + 1, the link models' cover; pairs None or (J + 2, J + 2) 0 / 1, symmetric: which
    frames' spheres are tested against each other for self-collision (None: default_self_pairs(arm))."""
    base: np.ndarray
    fixed: np.ndarray
    axis: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    kind: np.ndarray
    spheres: np.ndarray = _dc_field(default_factory=lambda: np.zeros((0, 5)))
    pairs: Optional[np.ndarray] = None

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

    def pair_table(self) -> Optional[np.ndarray]:
        """`pairs` as a contiguous uint8 (J + 2, J + 2) table of 0 / 1, checked; None when it is not set."""
        if self.pairs is None:
            return None
        J = self.num_joints
        t = np.asarray(self.pairs)
        if t.shape != (J + 2, J + 2):
            raise ValueError(f"pairs must be ({J + 2}, {J + 2}) for {J} joints, got {t.shape}")
        if not np.isin(t, (0, 1)).all():
            raise ValueError("pairs: an entry is neither 0 nor 1")
        if not np.array_equal(t, t.T):
            raise ValueError("pairs is not symmetric")
        return np.ascontiguousarray(t.astype(np.uint8))

    def reach_table(self) -> np.ndarray:
        """(J, S) float64 of the link spheres: `reach_table` below."""
        c, f, _ = self.link_spheres()
        return reach_table(self, c, f)

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
        d = {"base": np.asarray(self.base, np.float64).tolist(), "fixed": np.asarray(self.fixed, np.float64).tolist(),
             "joints": joints.tolist(), "spheres": np.asarray(self.spheres, np.float64).reshape(-1, 5).tolist()}
        if self.pairs is not None:
            d["pairs"] = self.pair_table().tolist()
        with open(path, "w") as f:
            json.dump(d, f)

    @classmethod
    def from_json(cls, path: str) -> "Arm":
        """An arm from a JSON file of numbers only: base [12], fixed [J + 1][12], joints [J][6] (axis, lo, hi, kind),
        spheres [K][5] (frame, x, y, z, radius; may be missing), pairs [J + 2][J + 2] of 0 / 1 (may be missing: None).
        ValueError naming the file and the field."""
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
                      np.asarray(d.get("spheres", []), np.float64).reshape(-1, 5),
                      None if d.get("pairs") is None else np.asarray(d["pairs"]))
            arm.to_array()
            arm.link_spheres()
            arm.pair_table()
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
# host side of the motion check: the sweep bound's table and the tested frame pairs
# ------------------------------------------------------------------------------------------------
def reach_table(arm: Arm, centres: ArrayLike, frames: ArrayLike) -> np.ndarray:
    """(J, S) float64: reach[j][s] bounds the speed of sphere s's centre per unit of q_j while the prismatic joints
    are within their limits (gg_arm_motion's `reach`).  0 for j >= frame[s] (the joint does not move the sphere).  For
    a revolute joint j the centre's distance to the joint's axis is at most its distance to the joint's origin, which
    is at most |offset| + sum_{k = j+1}^{frame-1} (|t(A_k)| + [k prismatic] max(|lo_k|, |hi_k|)), with A_J and no joint
    for the gripper frame J + 1.  For a prismatic joint: 1."""
    arm.to_array()
    J = arm.num_joints
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    f = np.asarray(frames, np.int64).reshape(-1)
    fixed = np.asarray(arm.fixed, np.float64)
    kind, lo, hi = (np.asarray(v, np.float64) for v in (arm.kind, arm.lo, arm.hi))
    # step[k], k = 1..J: what lies between the origin of joint k - 1 and that of joint k (or the gripper frame, k = J)
    step = np.zeros(J + 1)
    for k in range(1, J + 1):
        step[k] = np.linalg.norm(fixed[k, 9:])
        if k < J and kind[k] == 1.0:
            step[k] += max(abs(lo[k]), abs(hi[k]))
    out = np.zeros((J, len(c)))
    off = np.linalg.norm(c, axis=1)
    for j in range(J):
        for s in range(len(c)):
            if j < f[s]:
                out[j, s] = 1.0 if kind[j] == 1.0 else off[s] + step[j + 1:f[s]].sum()
    return out


def _fk_host(arm: Arm, q: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(R (N, J + 2, 3, 3), t (N, J + 2, 3)) of the frames F_0 .. F_{J+1}, numpy; what default_self_pairs samples with
    (the device's frames come from gg_arm_fk)."""
    J = arm.num_joints
    base, fixed, axis, kind = (np.asarray(v, np.float64) for v in (arm.base, arm.fixed, arm.axis, arm.kind))
    q = np.asarray(q, np.float64).reshape(-1, J)
    N = len(q)
    R = np.broadcast_to(base[:9].reshape(3, 3), (N, 3, 3)).copy()
    t = np.broadcast_to(base[9:], (N, 3)).copy()
    Rs, ts = [R], [t]
    for j in range(J + 1):
        t = t + R @ fixed[j, 9:]
        R = R @ fixed[j, :9].reshape(3, 3)
        if j < J:
            a = axis[j]
            if kind[j] == 1.0:
                t = t + (R @ a) * q[:, j, None]
            else:
                K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
                c, s = np.cos(q[:, j])[:, None, None], np.sin(q[:, j])[:, None, None]
                R = R @ (c * np.eye(3) + (1.0 - c) * np.outer(a, a) + s * K)
        Rs.append(R)
        ts.append(t)
    return np.stack(Rs, 1), np.stack(ts, 1)


def default_self_pairs(arm: Arm, min_gap: int = 2, samples: int = 1024, seed: int = 7) -> np.ndarray:
    """(J + 2, J + 2) uint8, symmetric: the frame pairs whose spheres are tested against each other.  Frames fewer than
    `min_gap` apart are not (neighbouring links touch by construction), nor are those with a pair of spheres that
    overlaps in EVERY one of `samples` configurations: uniform in the limits from np.random.default_rng(seed), row 0
    the home configuration (the "adjacent" and "always" rules of MoveIt's setup assistant, as recalled).  Computed on
    the host."""
    J = arm.num_joints
    c, f, r = arm.link_spheres()
    lo, hi = np.asarray(arm.lo, np.float64), np.asarray(arm.hi, np.float64)
    q = np.random.default_rng(seed).uniform(lo, hi, size=(max(int(samples), 1), J))
    q[0] = arm.home()
    R, t = _fk_host(arm, q)
    w = np.einsum("nsab,sb->nsa", R[:, f], c.astype(np.float64)) + t[:, f]          # (N, S, 3)
    table = np.zeros((J + 2, J + 2), np.uint8)
    for a in range(J + 2):
        for b in range(a + int(min_gap), J + 2):
            ia, ib = np.nonzero(f == a)[0], np.nonzero(f == b)[0]
            always = False
            if len(ia) and len(ib):
                d = np.linalg.norm(w[:, ia][:, :, None] - w[:, ib][:, None, :], axis=-1)
                always = bool(((d - (r[ia][:, None] + r[ib][None, :])).min((1, 2)) < 0.0).all())
            table[a, b] = table[b, a] = 0 if always else 1
    return table


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


@dataclass
class Motion:
    """The outputs of one gg_arm_motion call over E edges (of any leading shape), and the verdict."""
    samples: Tensor        # int32 n; 0: not resolved by max_samples, or an end that is not finite
    slack: Tensor          # int32 the minimum over the samples (FAR without a field)
    slack_at: Tensor       # int32 the first sample that attains it
    worst: Tensor          # int32 the sphere of that slack: the arm's link spheres first, then `spheres`
    gap: Tensor            # float64 the smallest gap of a tested sphere pair over the samples (+inf without pairs)
    gap_at: Tensor         # int32 the first sample that attains it
    pair: Tensor           # int32 (..., 2) the pair of that gap
    ok: Tensor             # bool: (samples > 0) & (slack >= 0) & (gap >= self_margin + res)
    res: float
    self_margin: float

    def reshape(self, *shape: int) -> "Motion":
        return replace(self, **{k: getattr(self, k).reshape(*shape) for k in
                                ("samples", "slack", "slack_at", "worst", "gap", "gap_at", "ok")},
                       pair=self.pair.reshape(*shape, 2))


def _self_set(arm: Arm, spheres, radius):
    """centres, frames and radii of the arm's link spheres followed by the gripper-frame `spheres` of `radius`"""
    c, f, r = arm.link_spheres()
    if spheres is not None:
        sp = host_array(spheres, np.float32).reshape(-1, 3)
        c = np.concatenate([c, sp])
        f = np.concatenate([f, np.full(len(sp), arm.num_joints + 1, np.int32)])
        r = np.concatenate([r, np.broadcast_to(np.asarray(radius, np.float64), (len(sp),))])
    if len(c) > MAX_SELF_SPHERES:
        raise ValueError(f"{len(c)} spheres with the arm's are more than {MAX_SELF_SPHERES}: use a larger radius")
    if not (np.isfinite(r).all() and (r >= 0).all()):
        raise ValueError("radius must be finite and >= 0")
    return np.ascontiguousarray(c), np.ascontiguousarray(f), np.ascontiguousarray(r, np.float64)


def _pair_arg(arm: Arm, pairs) -> Optional[np.ndarray]:
    """the tested frame pairs of a call: False: none (no self test); None: the arm's own, default_self_pairs(arm) when
    it has none; a table: that table"""
    if pairs is False:
        return None
    if pairs is None:
        own = arm.pair_table()
        return default_self_pairs(arm) if own is None else own
    return replace(arm, pairs=np.asarray(pairs)).pair_table()


def self_gap(arm: Arm, q: Tensor, spheres: Optional[ArrayLike] = None,
             radius: Union[float, ArrayLike] = SPHERE_RADIUS, pairs=None) -> Tuple[Tensor, Tensor]:
    """(gap (M,) float64, pair (M, 2) int32) of one gg_arm_self call: the smallest gap between two spheres of frames
    that `pairs` tests (None: arm.pairs, or default_self_pairs(arm)) and the pair that attains it, for every row of q
    (M, J) float64 on the HIP device (no CPU path).  The spheres are the arm's link spheres, then the optional
    gripper-frame `spheres` of `radius`."""
    dev = _require_hip(q)
    J, a = _arm_args(arm)
    q = _q_rows(q, J)
    m = q.shape[0]
    if m > MAX_POSES:
        raise ValueError(f"{m} rows are more than {MAX_POSES}")
    table = _pair_arg(arm, pairs)
    if table is None:
        raise ValueError("self_gap needs a table of tested pairs")
    c, f, r = _self_set(arm, spheres, radius)
    ct, ft, rt = to_device(c, torch.float32, dev), to_device(f, torch.int32, dev), to_device(r, torch.float64, dev)
    gap = torch.empty(m, dtype=torch.float64, device=dev)
    pair = torch.empty(m, 2, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_arm_self(J, host_ptr(a), m, _ptr(q), len(c), _ptr(ct), _ptr(ft), _ptr(rt),
                                       host_ptr(table), _ptr(gap), _ptr(pair), _stream(dev)), "gg_arm_self")
    return gap, pair


def motion(arm: Arm, q_a: Tensor, q_b: Tensor, field=None, spheres: Optional[ArrayLike] = None,
           radius: Union[float, ArrayLike] = SPHERE_RADIUS, margin: float = 0.0, self_margin: float = 0.0,
           res: Optional[float] = None, max_samples: int = MAX_SAMPLES, pairs=None, outside: str = "free") -> Motion:
    """One gg_arm_motion call: the straight joint-space moves q_a[e] -> q_b[e] ((E, J) float64 on the HIP device, no
    CPU path) against `field` (a field.DistanceField after update(); None: no field test) and against the arm itself
    (`pairs` as self_gap takes it; False: no self test).  The edge is sampled so that no sphere centre moves more than
    `res` (None: field.h) between two samples, by the bound of reach_table; the spheres are tested at radius + res / 2
    + margin, and `ok` asks a gap of self_margin + res, which is what makes the verdict hold for the whole motion and
    not only for the samples (include/gg_raster.h).  Prismatic joints must be within their limits."""
    if outside not in ("free", "blocked"):
        raise ValueError(f"outside must be 'free' or 'blocked', got {outside!r}")
    dev = _require_hip(q_a, q_b)
    J, a = _arm_args(arm)
    q_a, q_b = _q_rows(q_a, J), _q_rows(q_b, J)
    e = q_a.shape[0]
    if q_b.shape[0] != e:
        raise ValueError(f"q_a and q_b must have as many rows, got {e} and {q_b.shape[0]}")
    if e > MAX_POSES:
        raise ValueError(f"{e} edges are more than {MAX_POSES}")
    if res is None:
        if field is None:
            raise ValueError("without a field, give res")
        res = field.h
    res, self_margin = positive("res", res), nonneg("self_margin", self_margin)
    if not 1 <= int(max_samples) <= MAX_SAMPLES:
        raise ValueError(f"max_samples must be in 1..{MAX_SAMPLES}, got {max_samples}")
    table = _pair_arg(arm, pairs)
    c, f, r = _self_set(arm, spheres, radius)
    rt = np.ascontiguousarray(reach_table(arm, c, f))
    ct, ft = to_device(c, torch.float32, dev).reshape(-1, 3), to_device(f, torch.int32, dev)
    radt, reacht = to_device(r, torch.float64, dev), to_device(rt, torch.float64, dev)
    d = g = dist2 = need = None
    if field is not None:
        d, g, shape = volume_args(field.dims, field.grid)
        dist2 = volume_tensor(field.dist2, "dist2", torch.int32, shape, dev)
        need = to_device(need2(r + 0.5 * res, margin, field.h) if len(c) else np.zeros(0, np.int32), torch.int32, dev)
    samples, slack, slack_at, worst, gap_at = (torch.empty(e, dtype=torch.int32, device=dev) for _ in range(5))
    gap = torch.empty(e, dtype=torch.float64, device=dev)
    pair = torch.empty(e, 2, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gg_arm_motion(J, host_ptr(a), d, g, _ptr(dist2), e, _ptr(q_a), _ptr(q_b), len(c), _ptr(ct),
                                         _ptr(ft), _ptr(need), FAR if outside == "free" else 0, _ptr(radt),
                                         host_ptr(table), _ptr(reacht), res, int(max_samples), _ptr(samples),
                                         _ptr(slack), _ptr(slack_at), _ptr(worst), _ptr(gap), _ptr(gap_at), _ptr(pair),
                                         _stream(dev)), "gg_arm_motion")
    ok = (samples > 0) & (slack >= 0) & (gap >= self_margin + res)
    return Motion(samples, slack, slack_at, worst, gap, gap_at, pair, ok, res, self_margin)


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
    # with motion=True (None otherwise):
    motion_ok: Optional[Tensor] = None     # (P,) bool: the chosen seed's edges are all ok and its self gaps >= self_margin
    motion_all: Optional[Tensor] = None    # (P, S) bool: the same of every seed; False for a seed that fails its path
    motion: Optional[Motion] = None        # the edges w -> w + 1 of every seed, (P, S, W - 1); NaN rows: samples 0
    gap_all: Optional[Tensor] = None       # (P, S, W) float64 gg_arm_self's gap of every configuration


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
           home, outside: str, ik, check_motion: bool = False, self_margin: float = 0.0,
           motion_res: Optional[float] = None, max_samples: int = MAX_SAMPLES) -> Reach:
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
    extra = {}
    if check_motion:
        # every edge w -> w + 1 of every seed, and every configuration's self gap; a seed that fails its path has NaN
        # rows, which come back as samples 0 and a NaN gap: not ok
        self_margin = nonneg("self_margin", self_margin)
        gap_all = torch.full((p, s, w), math.inf, dtype=torch.float64, device=dev)
        parts = []
        for rows, sp in sphere_sets:
            idx = torch.as_tensor(np.asarray(rows, np.int64), device=dev)
            qs = fol.q[idx]
            if qs.numel():
                gap_all[idx] = self_gap(arm, qs.reshape(-1, J), sp, radius)[0].reshape(len(idx), s, w)
            parts.append((idx, motion(arm, qs[:, :, :-1].reshape(-1, J), qs[:, :, 1:].reshape(-1, J), field, sp, radius,
                                      margin, self_margin, motion_res, max_samples, outside=outside)
                          .reshape(len(idx), s, max(w - 1, 0))))
        order = torch.argsort(torch.cat([i for i, _ in parts])) if parts else torch.zeros(0, dtype=torch.int64)
        edges = Motion(**{k: torch.cat([getattr(m, k) for _, m in parts])[order] for k in
                          ("samples", "slack", "slack_at", "worst", "gap", "gap_at", "pair", "ok")},
                       res=parts[0][1].res, self_margin=self_margin)
        motion_all = edges.ok.all(-1) & (gap_all >= self_margin).all(-1) & (fol.first_fail == w)
        clear_ok = clear_ok & motion_all
        extra = dict(motion_all=motion_all, motion=edges, gap_all=gap_all)
    pick, reachable, ok = select(fol.first_fail.cpu().numpy(), w, clear_ok.cpu().numpy(), jump_all.cpu().numpy())
    at = torch.as_tensor(np.maximum(pick, 0), device=dev)
    rows = torch.arange(p, device=dev)
    none = torch.as_tensor(pick < 0, device=dev)
    q = fol.q[rows, at]
    q = torch.where(none[:, None, None], torch.full_like(q, math.nan), q)
    jump = torch.where(none, torch.full((p,), math.inf, dtype=torch.float64, device=dev), jump_all[rows, at])
    if check_motion:
        extra["motion_ok"] = extra["motion_all"][rows, at] & ~none
    return Reach(q, torch.as_tensor(reachable, device=dev), torch.as_tensor(ok, device=dev),
                 torch.as_tensor(pick, device=dev), slack_all[rows, at], worst_all[rows, at], jump, fol, slack_all,
                 worst_all, **extra)


def reach(arm: Arm, poses: ArrayLike, field=None, spheres: Optional[ArrayLike] = None,
          radius: Union[float, ArrayLike] = SPHERE_RADIUS, margin: float = 0.0, num_seeds: int = NUM_SEEDS,
          seed: int = 0, home: Optional[ArrayLike] = None, outside: str = "free", motion: bool = False,
          self_margin: float = 0.0, motion_res: Optional[float] = None, max_samples: int = MAX_SAMPLES,
          **ik) -> Reach:
    """Which of the (P, W, 12) gripper pose paths the arm can follow, in which configurations, and whether the whole
    arm stays clear of `field` (a field.DistanceField after update(); None: no clearance test) on the way: follow from
    num_seeds seeds per path (`seeds`), clear of every configuration with the arm's link spheres plus the optional
    gripper-frame `spheres` of `radius` (field.gripper_spheres, transit.carried_spheres), kept `margin` away, and
    `select`.  motion=True also tests the straight joint-space move between consecutive waypoints of every seed that
    follows its path (`motion`, at motion_res: None is field.h) and every configuration's self gap against
    self_margin; `clear` then requires them too, and the result carries motion_ok, motion_all, motion and gap_all.
    With motion=False nothing of that runs and every field is what it was.  **ik: follow's parameters."""
    dev = default_device("arm") if field is None else field.dist2.device
    p = to_device(poses, torch.float32, dev)
    if p.ndim != 3 or p.shape[2] != 12:
        raise ValueError(f"poses must be (P, W, 12), got {tuple(p.shape)}")
    return _reach(arm, p, field, [(np.arange(p.shape[0]), spheres)], radius, margin, num_seeds, seed, home, outside, ik,
                  motion, self_margin, motion_res, max_samples)


def reach_grasps(arm: Arm, rows: ArrayLike, standoff: float, steps: int, field=None,
                 gripper: Optional[ArrayLike] = None, radius: float = SPHERE_RADIUS, margin: float = 0.0,
                 num_seeds: int = NUM_SEEDS, seed: int = 0, home: Optional[ArrayLike] = None, outside: str = "free",
                 motion: bool = False, self_margin: float = 0.0, motion_res: Optional[float] = None,
                 max_samples: int = MAX_SAMPLES, **ik) -> Tuple[Reach, Tensor]:
    """`reach` on the straight approach of every (M, 17) grasp row (field.approach_paths(rows, standoff, steps)), and
    the (M,) bool row mask grasp.filter_grasps accepts: the arm follows the whole approach and stays clear.  With a
    `gripper` model (grasp.default_gripper, ...) its spheres of `radius` ride on the gripper frame at each row's
    width, depth and height; leave it None when the field holds the object to be grasped, which the fingers touch at
    the last waypoint (field.py's note on the grasp pose).  motion, self_margin, motion_res, max_samples: as `reach`."""
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
                 outside, ik, motion, self_margin, motion_res, max_samples)
    return res, res.clear


@dataclass
class Connect:
    routes: list           # [A][B]: None, or the (2 or 3, J) float64 numpy waypoints of the chosen route
    via: np.ndarray        # (A, B) int64: -1 the direct move, -2 no clear route, else the row of `vias` passed through
    cost: np.ndarray       # (A, B) float64 the route's sum of |dq|inf over its moves; inf without a route
    vias: np.ndarray       # (V, J) float64 the via configurations that were tried (those not clear themselves dropped)
    motion: Motion         # the one call's edges: direct (A B, row a B + b), from -> via (A V), via -> to (V B)


def connect_select(direct_ok: ArrayLike, direct_cost: ArrayLike, leg1_ok: ArrayLike, leg1_cost: ArrayLike,
                   leg2_ok: ArrayLike, leg2_cost: ArrayLike) -> Tuple[np.ndarray, np.ndarray]:
    """(via (A, B) int64, cost (A, B) float64), numpy.  direct_* (A, B); leg1_* (A, V): from a to via v; leg2_* (V, B):
    from via v to b.  A route is clear when all of its moves are ok; its cost is the sum of its moves' costs.  Chosen
    per (a, b): the clear route of the smallest cost, the direct move before a via of the same cost, the lowest via of
    equals; via = -1 for the direct move, -2 (and cost inf) when no route is clear."""
    d_ok, d_cost = np.asarray(direct_ok, bool), np.asarray(direct_cost, np.float64)
    l1_ok, l1_cost = np.asarray(leg1_ok, bool), np.asarray(leg1_cost, np.float64)
    l2_ok, l2_cost = np.asarray(leg2_ok, bool), np.asarray(leg2_cost, np.float64)
    A, B = d_ok.shape
    via = np.full((A, B), -2, np.int64)
    cost = np.full((A, B), np.inf)
    if l1_ok.shape[1]:
        key = np.where(l1_ok[:, :, None] & l2_ok[None, :, :], l1_cost[:, :, None] + l2_cost[None, :, :], np.inf)
        best = np.argmin(key, axis=1)                               # the first of equals
        cost = np.take_along_axis(key, best[:, None, :], 1)[:, 0, :]
        via = np.where(np.isfinite(cost), best, -2)
    direct = d_ok & (d_cost <= cost)
    return np.where(direct, -1, via).astype(np.int64), np.where(direct, d_cost, cost)


def connect(arm: Arm, q_from: ArrayLike, q_to: ArrayLike, field=None, vias: Optional[ArrayLike] = None,
            num_vias: int = NUM_VIAS, seed: int = 0, spheres: Optional[ArrayLike] = None,
            radius: Union[float, ArrayLike] = SPHERE_RADIUS, margin: float = 0.0, self_margin: float = 0.0,
            res: Optional[float] = None, max_samples: int = MAX_SAMPLES, pairs=None, outside: str = "free") -> Connect:
    """A clear joint-space route from every q_from (A, J) to every q_to ((B, J), or (J,) for B = 1): the straight move,
    or from -> v -> to through one via configuration v.  vias None: the home configuration, then num_vias - 1 uniform
    in the limits from np.random.default_rng(seed).  Vias that are not clear themselves (a zero-length `motion` each)
    are dropped; every remaining move is one edge of ONE `motion` call, and `connect_select` chooses per (from, to).
    One level only: no tree, no roadmap."""
    dev = default_device("arm") if field is None else field.dist2.device
    J = arm.num_joints
    qa = host_array(q_from, np.float64).reshape(-1, J)
    qb = host_array(q_to, np.float64).reshape(-1, J)
    if vias is None:
        lo, hi = np.asarray(arm.lo, np.float64), np.asarray(arm.hi, np.float64)
        n = max(int(num_vias), 0)
        v = np.empty((n, J))
        if n:
            v[0] = arm.home()
            v[1:] = np.random.default_rng(seed).uniform(lo, hi, size=(n - 1, J))
    else:
        v = host_array(vias, np.float64).reshape(-1, J)
    kw = dict(field=field, spheres=spheres, radius=radius, margin=margin, self_margin=self_margin, res=res,
              max_samples=max_samples, pairs=pairs, outside=outside)
    if len(v):
        vt = to_device(v, torch.float64, dev)
        v = v[motion(arm, vt, vt, **kw).ok.cpu().numpy()]
    A, B, V = len(qa), len(qb), len(v)
    starts = np.concatenate([np.repeat(qa, B, 0), np.repeat(qa, V, 0), np.repeat(v, B, 0)])
    ends = np.concatenate([np.tile(qb, (A, 1)), np.tile(v, (A, 1)), np.tile(qb, (V, 1))])
    m = motion(arm, to_device(starts, torch.float64, dev), to_device(ends, torch.float64, dev), **kw)
    ok = m.ok.cpu().numpy()
    jump = np.abs(ends - starts).max(1) if J else np.zeros(len(starts))
    cut = (A * B, A * B + A * V)
    via, cost = connect_select(ok[:cut[0]].reshape(A, B), jump[:cut[0]].reshape(A, B),
                               ok[cut[0]:cut[1]].reshape(A, V), jump[cut[0]:cut[1]].reshape(A, V),
                               ok[cut[1]:].reshape(V, B), jump[cut[1]:].reshape(V, B))
    routes = [[None if via[a, b] == -2 else np.stack([qa[a], qb[b]] if via[a, b] == -1 else [qa[a], v[via[a, b]], qb[b]])
               for b in range(B)] for a in range(A)]
    return Connect(routes, via, cost, v, m)


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
    ap.add_argument("--check-motion", action="store_true",
                    help="also test the joint-space move between consecutive waypoints, and self-collision")
    ap.add_argument("--motion-res", type=float, default=None,
                    help="no sphere centre moves further than this between two samples of a move (default: the "
                         "field's cell edge)")
    ap.add_argument("--self-margin", type=float, default=0.0, help="gap kept between the arm's own spheres")
    ap.add_argument("--max-samples", type=int, default=MAX_SAMPLES, help="samples per move at most")
    ap.add_argument("--connect-from", default=None, metavar="Q.npy",
                    help=".npy (A, J) or (J,) configurations: a clear move (direct, or through one via configuration) "
                         "from each to the first configuration of every path")
    ap.add_argument("--connect-roadmap", default=None, metavar="{N,FILE.npz}",
                    help="with --connect-from: plan through a roadmap (gaussiangrasper_amd.roadmap) of N sampled "
                         "configurations, or through a saved one, in place of the one-via search; the report then has "
                         "roadmap_cost, roadmap_hops and roadmap_waypoints")
    ap.add_argument("--out", required=True, help="output .npy (P, W, J) joint configurations (NaN: not reachable)")
    ap.add_argument("--report", required=True, help="output .npz reachable, clear, seed, slack, worst, jump, "
                                                    "first_fail, iters; with --check-motion also motion_ok, samples, "
                                                    "gap, pair, slack_at; with --connect-from connect_via, "
                                                    "connect_cost, connect_waypoints")
    a = ap.parse_args(argv)
    if bool(a.grasps) == bool(a.poses):
        ap.error("give --grasps (with --standoff and --steps) or --poses")
    if a.grasps and (a.standoff is None or a.steps is None):
        ap.error("--grasps needs --standoff and --steps")
    if a.poses and (a.standoff is not None or a.steps is not None):
        ap.error("--standoff and --steps go with --grasps")
    if a.spheres and not a.field:
        ap.error("--spheres needs --field")
    check_finite_options(ap, a, positive=("radius",), nonneg=("margin", "self_margin"))
    if a.motion_res is not None and not (math.isfinite(a.motion_res) and a.motion_res > 0.0):
        ap.error(f"--motion-res must be finite and > 0, got {a.motion_res}")
    if (a.check_motion or a.connect_from) and a.motion_res is None and not a.field:
        ap.error("--check-motion and --connect-from need --field or --motion-res")
    if not 1 <= a.max_samples <= MAX_SAMPLES:
        ap.error(f"--max-samples must be in 1..{MAX_SAMPLES}, got {a.max_samples}")
    if a.connect_roadmap is not None:
        if not a.connect_from:
            ap.error("--connect-roadmap goes with --connect-from")
        if not a.connect_roadmap.endswith(".npz"):
            from .roadmap import MAX_NODES
            if not (a.connect_roadmap.isdigit() and 1 <= int(a.connect_roadmap) <= MAX_NODES):
                ap.error(f"--connect-roadmap must be a number of nodes in 1..{MAX_NODES} or a .npz file, got "
                         f"{a.connect_roadmap}")
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
        if a.check_motion:
            kw.update(motion=True, self_margin=a.self_margin, motion_res=a.motion_res, max_samples=a.max_samples)
        if a.grasps:
            poses =approach_paths(load_grasps(a.grasps), a.standoff, a.steps)
        else:
            poses = np.asarray(np.load(a.poses), np.float32)
            if poses.ndim != 3 or poses.shape[2] != 12:
                raise ValueError(f"{a.poses}: expected (P, W, 12) poses, got {poses.shape}")
        res = reach(arm, poses, spheres=spheres, **kw)
        np.save(a.out, res.q.cpu().numpy())
        report = dict(reachable=res.reachable.cpu().numpy(), clear=res.clear.cpu().numpy(),
                      seed=res.seed.cpu().numpy(), slack=res.slack.cpu().numpy(), worst=res.worst.cpu().numpy(),
                      jump=res.jump.cpu().numpy(), first_fail=res.follow.first_fail.cpu().numpy(),
                      iters=res.follow.iters.cpu().numpy())
        if a.check_motion:
            # the chosen seed's edges w -> w + 1 (the rows of paths without one are those of seed 0: samples 0)
            rows, at = torch.arange(poses.shape[0], device=res.seed.device), res.seed.clamp(min=0)
            report.update(motion_ok=res.motion_ok.cpu().numpy(),
                          **{k: getattr(res.motion, k)[rows, at].cpu().numpy()
                             for k in ("samples", "gap", "pair", "slack_at")})
        if a.connect_from:
            J = arm.num_joints
            start = np.asarray(np.load(a.connect_from), np.float64)
            if start.ndim not in (1, 2) or start.shape[-1] != J:
                raise ValueError(f"{a.connect_from}: expected ({J},) or (A, {J}) configurations, got {start.shape}")
            start = start.reshape(-1, J)
            q0 = res.q[:, 0].cpu().numpy() if poses.shape[1] else np.zeros((0, J))
            have = np.nonzero(np.isfinite(q0).all(1))[0]
        if a.connect_from and a.connect_roadmap is not None:
            from . import roadmap as _roadmap
            mkw = dict(spheres=spheres, radius=a.radius, margin=a.margin, self_margin=a.self_margin, res=a.motion_res,
                       max_samples=a.max_samples)
            if a.connect_roadmap.endswith(".npz"):
                pl = _roadmap.plan(arm, start, q0[have], field,
                                   roadmap=_roadmap.Roadmap.load(a.connect_roadmap).attach(arm, field))
            else:
                pl = _roadmap.plan(arm, start, q0[have], field, num_nodes=int(a.connect_roadmap), seed=a.seed, **mkw)
            rep = _roadmap.plan_report(pl)
            cost = np.full((len(start), len(q0)), -1, np.int64)
            hops = np.full((len(start), len(q0)), -1, np.int64)
            way = np.full((len(start), len(q0)) + rep["waypoints"].shape[2:], np.nan)
            cost[:, have], hops[:, have], way[:, have] = rep["cost"], rep["hops"], rep["waypoints"]
            report.update(roadmap_cost=cost, roadmap_hops=hops, roadmap_waypoints=way)
        elif a.connect_from:
            con = connect(arm, start, q0[have], field, seed=a.seed, spheres=spheres, radius=a.radius, margin=a.margin,
                          self_margin=a.self_margin, res=a.motion_res, max_samples=a.max_samples)
            via = np.full((len(start), len(q0)), -2, np.int64)
            cost = np.full((len(start), len(q0)), np.inf)
            way = np.full((len(start), len(q0), 3, J), np.nan)
            via[:, have], cost[:, have] = con.via, con.cost
            for i in range(len(start)):
                for k, b in enumerate(have):
                    if con.routes[i][k] is not None:
                        way[i, b, :len(con.routes[i][k])] = con.routes[i][k]
            report.update(connect_via=via, connect_cost=cost, connect_waypoints=way)
        np.savez(a.report, **report)
    except (KeyError, ValueError, OSError, _lib.GGError) as exc:
        raise SystemExit(f"error: {exc}") from exc
    print(f"{int(res.reachable.sum())} of {poses.shape[0]} paths reachable, {int(res.clear.sum())} clear"
          + ("" if field is not None else " (no field: clearance not tested)")
          + (f", {int(res.motion_ok.sum())} with every move between waypoints clear" if a.check_motion else "")
          + (f", {int((report['roadmap_hops'] >= 0).sum())} of {report['roadmap_hops'].size} connections found through "
             "the roadmap" if a.connect_from and a.connect_roadmap is not None else
             f", {int((report['connect_via'] != -2).sum())} of {report['connect_via'].size} connections found"
             if a.connect_from else "") + f"; wrote {a.out} and {a.report}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
