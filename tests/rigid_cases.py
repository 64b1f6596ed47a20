"""TEST-ONLY inputs shared by tests/test_rigid_host.py and tests/test_rigid_gpu.py: the kernels' sizes, masks and
arrays, and the pose-recovery fixture (an L-shaped coloured block on a table, four views)."""
import math

import numpy as np
import torch

from gaussiangrasper_amd.camera import ring_cameras
from gaussiangrasper_amd.constants import SH_C0
from gaussiangrasper_amd.scene import Scene

# one, two and three slab rows for chain 0 of the finish (rows of 256, 16 chains): 4096, 4097, 8449
SIZES = (1, 63, 64, 65, 255, 256, 257, 4096, 4097, 8449)
MASKS = ("null", "none", "row 0", "last row", "rows >= 4096", "every third", "bytes 1 2 255")


def make_mask(kind, n):
    """(n,) uint8 or None"""
    if kind == "null":
        return None
    m = np.zeros(n, np.uint8)
    if kind == "row 0":
        m[0] = 1
    elif kind == "last row":
        m[n - 1] = 1
    elif kind == "rows >= 4096":
        m[4096:] = 1
    elif kind == "every third":
        m[::3] = 1
    elif kind == "bytes 1 2 255":
        m[:] = np.array([1, 0, 2, 0, 255], np.uint8)[np.arange(n) % 5]
    elif kind != "none":
        raise ValueError(kind)
    return m


def pose(seed):
    """a rotation of about 20 degrees and a translation: rt (12,) fp32, qt (4,) fp32 (consistent to fp32 rounding)"""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = math.radians(20.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    rt = np.concatenate([R, rng.uniform(-0.3, 0.3, (3, 1))], axis=1).astype(np.float32).reshape(12)
    qt = np.concatenate([[math.cos(th / 2)], math.sin(th / 2) * ax]).astype(np.float32)
    return rt, qt


def real_arrays(n, seed):
    """means, quats, g_means, g_quats: fp32 normal draws"""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 4)).astype(np.float32),
            rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 4)).astype(np.float32))


def lattice_arrays(n, seed):
    """Every value a multiple of 2^-10 with magnitude below 8: a product is a multiple of 2^-20 below 64, a row's
    quaternion term a multiple of 2^-20 below 256, and a sum of fewer than 2^20 of them stays below 2^28 — 48
    significant bits, so every partial sum is exact in fp64 whatever the order."""
    rng = np.random.default_rng(seed)
    draw = lambda *s: (rng.integers(-8191, 8192, s) / 1024.0).astype(np.float32)
    return draw(n, 3), draw(n, 4), draw(n, 3), draw(n, 4)


def lattice_pose(seed):
    rng = np.random.default_rng(seed)
    draw = lambda *s: (rng.integers(-8191, 8192, s) / 1024.0).astype(np.float32)
    return draw(12), draw(4)


# ------------------------------------------------------------------------------------------------------------------
# pose recovery: an L-shaped block of 270 coloured Gaussians on a table of 300, four 72 x 96 views
# ------------------------------------------------------------------------------------------------------------------
REC_H, REC_W, REC_VIEWS = 72, 96, 4
TRUE_T = (0.02, -0.015, 0.01)
TRUE_AXIS, TRUE_DEG = (0.3, -0.8, 0.5), 4.0


def block_scene():
    """(Scene (CPU, fp32, SH degree 0), mask (570,) uint8 selecting the block)"""
    rng = np.random.default_rng(11)
    foot = rng.uniform([-0.25, -0.08, -0.2], [0.25, 0.08, -0.05], (160, 3))
    post = rng.uniform([0.09, -0.08, -0.05], [0.25, 0.08, 0.25], (110, 3))
    table = np.concatenate([rng.uniform(-0.9, 0.9, (300, 2)), np.full((300, 1), -0.2)], axis=1)   # lift_ref.two_object_scene's
    means = np.concatenate([foot, post, table]).astype(np.float32)
    scales = np.concatenate([np.full((270, 3), 0.03), np.tile([0.08, 0.08, 0.01], (300, 1))]).astype(np.float32)
    q = rng.normal(size=(270, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    quats = np.concatenate([q, np.tile([1.0, 0.0, 0.0, 0.0], (300, 1))]).astype(np.float32)
    dc = np.concatenate([(rng.random((270, 3)) - 0.5) / SH_C0, np.zeros((300, 3))]).astype(np.float32)
    n = len(means)
    sc = Scene(torch.from_numpy(means), torch.log(torch.from_numpy(scales)), torch.from_numpy(quats),
               torch.full((n, 1), 3.0), torch.from_numpy(dc)[:, None, :].contiguous(), torch.zeros(n, 1))
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[:270] = 1
    return sc, mask


def true_transform():
    """(4, 4) fp64: 4 degrees about TRUE_AXIS through the block's centroid, then TRUE_T"""
    sc, mask = block_scene()
    c = sc.means[mask.bool()].double().mean(dim=0).numpy()
    ax = np.asarray(TRUE_AXIS) / np.linalg.norm(TRUE_AXIS)
    th = math.radians(TRUE_DEG)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = c - R @ c + np.asarray(TRUE_T)
    return T


def moved_scene(T):
    """the scene with the block moved by T (4, 4) in fp64 and rounded to fp32: means R x + t, quats quat(R) (x) q; the
    colours are not turned (degree 0: nothing to turn)"""
    import rigid_ref
    from gaussiangrasper_amd.pose import rotmat_to_quat
    sc, mask = block_scene()
    qt = rotmat_to_quat(torch.from_numpy(T[:3, :3])).numpy()
    m64, q64 = rigid_ref.forward64(sc.means.numpy(), sc.quats.numpy(), mask.numpy(), T[:3, :].reshape(12), qt)
    return Scene(torch.from_numpy(m64.astype(np.float32)), sc.scales, torch.from_numpy(q64.astype(np.float32)),
                 sc.opacities, sc.colors_all, sc.feature)


def recovery_views(device="cpu"):
    return ring_cameras(REC_VIEWS, REC_H, REC_W, device=device)


def pose_errors(T_est, T_true):
    """(translation error of the block's centroid in metres, ||R_est - R_true||_F), fp64"""
    sc, mask = block_scene()
    c = sc.means[mask.bool()].double().mean(dim=0).numpy()
    A, B = np.asarray(T_est, np.float64), np.asarray(T_true, np.float64)
    dt = np.linalg.norm((A[:3, :3] @ c + A[:3, 3]) - (B[:3, :3] @ c + B[:3, 3]))
    return float(dt), float(np.linalg.norm(A[:3, :3] - B[:3, :3]))
