"""Frames on the host (numpy, fp64): homogeneous matrices, the check on rotations, the transform JSON,
and the world -> scene similarity map x -> scale (M [x, 1]) of a dataparser's transform_matrix and scale, applied
to points, directions, camera poses and rigid [R | t] rows, forwards and backwards.  edit, edit_masks, grasp,
grasp_propose and mesh hand these out under their own names; each keeps its order of floating-point operations."""
from __future__ import annotations

import json
from typing import Tuple

import numpy as np
from torch import Tensor

from ._call import ArrayLike, positive

ORTHO_TOL = 1e-4


def homogeneous(m: ArrayLike) -> np.ndarray:
    """(.., 3, 4) or (.., 4, 4) matrices as (.., 4, 4) fp64."""
    a = np.asarray(m.detach().cpu().numpy() if isinstance(m, Tensor) else m, dtype=np.float64)
    if a.shape[-2:] == (3, 4):
        a = np.concatenate([a, np.broadcast_to([0.0, 0.0, 0.0, 1.0], a.shape[:-2] + (1, 4))], axis=-2)
    if a.shape[-2:] != (4, 4):
        raise ValueError(f"expected (.., 3, 4) or (.., 4, 4) camera matrices, got {a.shape}")
    return a


def rigid_rows(transform: ArrayLike, dtype) -> np.ndarray:
    """[R | t] of a (3, 4) or (4, 4) rigid transform as 12 contiguous values of `dtype`, row-major."""
    t = transform.detach().cpu().numpy() if isinstance(transform, Tensor) else np.asarray(transform)
    if t.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"transform must be [R | t] (3, 4) or homogeneous (4, 4), got {t.shape}")
    return np.ascontiguousarray(t[:3, :], dtype=dtype).reshape(12)


def check_rotation(R: np.ndarray, what: str) -> None:
    err = np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max(initial=0.0)
    if not err <= ORTHO_TOL:
        raise ValueError(f"{what} is not orthonormal (max |R^T R - I| = {err:.3g} > {ORTHO_TOL:g})")


def load_transform_json(path_or_dict) -> Tuple[np.ndarray, float]:
    """(transform_matrix fp64 as the file has it, scale) of a nerfstudio dataparser_transforms.json (or its dict);
    the caller checks the matrix's shape."""
    if isinstance(path_or_dict, dict):
        tj = path_or_dict
    else:
        with open(path_or_dict) as f:
            tj = json.load(f)
    return np.asarray(tj["transform_matrix"], dtype=np.float64), float(tj["scale"])


# ------------------------------------------------------------------------------------------------
# the similarity map
# ------------------------------------------------------------------------------------------------
def points_to_scene(points: ArrayLike, matrix: ArrayLike, scale: float) -> np.ndarray:
    """Object points into the scene's frame (update.py:148-149): [x, 1] @ matrix[:3, :].T, times scale."""
    p = np.asarray(points, dtype=np.float64)[:, :3]
    M = np.asarray(matrix, dtype=np.float64)
    return (np.concatenate((p, np.ones((p.shape[0], 1))), axis=1) @ M[:3, :].T) * float(scale)


def points_from_scene(points: ArrayLike, matrix: ArrayLike, scale: float) -> np.ndarray:
    """Inverse of points_to_scene: scene-frame points (N, 3) back to the scan's raw frame, fp64."""
    p = np.asarray(points, dtype=np.float64)[:, :3] / float(scale)
    M = homogeneous(matrix)
    return (p - M[:3, 3]) @ np.linalg.inv(M[:3, :3]).T


def directions_from_scene(normals: ArrayLike, matrix: ArrayLike) -> np.ndarray:
    """Unit directions (N, 3) of the scene frame in the scan's raw frame (the inverse rotation, renormalised)."""
    n = np.asarray(normals, dtype=np.float64)[:, :3] @ np.linalg.inv(homogeneous(matrix)[:3, :3]).T
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)


def c2w_to_scene(c2w: ArrayLike, matrix: ArrayLike, scale: float) -> np.ndarray:
    """Camera-to-world poses (.., 3|4, 4) of the scan's raw frame in the checkpoint's frame: the same map that
    points_to_scene applies to points (x -> scale (M [x, 1])), applied to the camera centre, and M's rotation
    applied to the camera axes.  Either axis convention (the map acts on the left)."""
    a = homogeneous(c2w)
    M = homogeneous(matrix)
    out = np.array(a, dtype=np.float64)
    out[..., :3, :3] = M[:3, :3] @ a[..., :3, :3]
    out[..., :3, 3] = ((a[..., :3, 3] @ M[:3, :3].T) + M[:3, 3]) * float(scale)
    return out


def rigid_to_scene(R: np.ndarray, t: np.ndarray, cam_to_world, matrix, scale: float, inverse: bool = False):
    """Rigid rows R (N, 3, 3), t (N, 3) of a camera frame in the scene frame, M3 C3 R and
    scale (M3 (C3 t + C_t) + M_t), or with `inverse` back from it, (M3 C3)^T R and C3^T (M3^T (t / scale - M_t) - C_t).
    cam_to_world 4x4 and matrix 3x4 or 4x4 (None: identity); their rotations and every finite R must be orthonormal.
    Returns (R', t', the checked scale)."""
    C = np.eye(4) if cam_to_world is None else np.asarray(cam_to_world, dtype=np.float64)
    M = np.eye(4) if matrix is None else np.asarray(matrix, dtype=np.float64)
    if C.shape != (4, 4):
        raise ValueError(f"cam_to_world must be 4x4, got {C.shape}")
    if M.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"matrix must be 3x4 or 4x4, got {M.shape}")
    scale = positive("scale", scale)
    check_rotation(C[:3, :3], "cam_to_world rotation")
    check_rotation(M[:3, :3], "matrix rotation")
    check_rotation(R[np.isfinite(R).all(axis=(1, 2))], "grasp rotation")
    A = M[:3, :3] @ C[:3, :3]
    if inverse:
        world = (t / scale - M[:3, 3]) @ M[:3, :3]          # M3^T x as a row vector: x M3
        return A.T @ R, (world - C[:3, 3]) @ C[:3, :3], scale
    return A @ R, scale * ((t @ C[:3, :3].T + C[:3, 3]) @ M[:3, :3].T + M[:3, 3]), scale
