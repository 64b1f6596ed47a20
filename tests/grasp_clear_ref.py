"""fp64 numpy restatement of the gripper-clearance contract (include/gg_raster.h gg_grasp_clearance, PARITY.md
"Gripper clearance"), written from the contract and used by tests/test_grasp_clear_host.py and
tests/test_grasp_clear_gpu.py.  Every elementwise operation is rounded once (numpy does not contract), in the
contract's order, so every body and sweep decision is the kernel's bit for bit and the counts are equal; the sums are
taken in numpy's order, so the weights agree to rounding (exactly, when every partial sum is exact in fp64)."""
import math

import numpy as np


def part_bounds(parts, grasps):
    """(M, P, 6) bounds (x_lo, x_hi, y_lo, y_hi, z_lo, z_hi) of every part for every row:
    ((c0 + cw width) + cd depth) + ch height, in that order."""
    c = np.asarray(parts, np.float64).reshape(-1, 6, 4)
    G = np.asarray(grasps, np.float32).astype(np.float64).reshape(-1, 17)
    w, h, d = (G[:, k][:, None, None] for k in (1, 2, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        return ((c[None, :, :, 0] + c[None, :, :, 1] * w) + c[None, :, :, 2] * d) + c[None, :, :, 3] * h


def row_valid(grasps):
    G = np.asarray(grasps, np.float32).astype(np.float64).reshape(-1, 17)
    with np.errstate(invalid="ignore"):
        return np.isfinite(G).all(1) & (G[:, 1] > 0) & (G[:, 2] > 0)


def restate(points, weights, grasps, parts, approach=0.0, min_weight=0.0, max_body=math.inf, max_sweep=math.inf):
    """dict of numpy arrays: body_count, sweep_count (M, P) int64; body_weight, sweep_weight (M, P) float64, the
    fp64 sums before they are rounded; body_total, sweep_total (M,) float64; valid, clear (M,) bool."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    w = np.asarray(weights, np.float32).astype(np.float64).reshape(-1)
    G = np.asarray(grasps, np.float32).astype(np.float64).reshape(-1, 17)
    B = part_bounds(parts, grasps)
    m, P = B.shape[:2]
    with np.errstate(invalid="ignore"):
        part = np.isfinite(p).all(1) & (w > float(min_weight))
    p, w = p[part], w[part]
    valid = row_valid(grasps)
    out = dict(body_count=np.zeros((m, P), np.int64), sweep_count=np.zeros((m, P), np.int64),
               body_weight=np.zeros((m, P)), sweep_weight=np.zeros((m, P)), body_total=np.zeros(m),
               sweep_total=np.zeros(m), valid=valid, clear=np.zeros(m, bool))
    for g in np.nonzero(valid)[0]:
        R, t = G[g, 4:13], G[g, 13:16]
        d0, d1, d2 = p[:, 0] - t[0], p[:, 1] - t[1], p[:, 2] - t[2]
        u0 = (R[0] * d0 + R[3] * d1) + R[6] * d2
        u1 = (R[1] * d0 + R[4] * d1) + R[7] * d2
        u2 = (R[2] * d0 + R[5] * d1) + R[8] * d2
        tb = ts = 0.0
        for k in range(P):
            b = B[g, k]
            if not (np.isfinite(b).all() and b[0] <= b[1] and b[2] <= b[3] and b[4] <= b[5]):
                continue                                     # an empty part counts nothing, body or sweep
            yz = (u1 >= b[2]) & (u1 <= b[3]) & (u2 >= b[4]) & (u2 <= b[5])
            body = yz & (u0 >= b[0]) & (u0 <= b[1])
            sweep = yz & (u0 >= b[0] - float(approach)) & (u0 < b[0])
            out["body_count"][g, k], out["sweep_count"][g, k] = body.sum(), sweep.sum()
            out["body_weight"][g, k], out["sweep_weight"][g, k] = w[body].sum(), w[sweep].sum()
            tb += out["body_weight"][g, k]
            ts += out["sweep_weight"][g, k]
        out["body_total"][g], out["sweep_total"][g] = tb, ts
        out["clear"][g] = tb <= float(max_body) and ts <= float(max_sweep)
    return out


def slab_gripper(num_parts):
    """A model of `num_parts` boxes that split the space between the fingers along the closing axis: part k is
    x [-0.01, depth], y [(k / P - 1/2) width, ((k + 1) / P - 1/2) width], z [-height / 2, height / 2].  Disjoint up to
    faces, and every bound but x_lo depends on the row's sizes."""
    g = np.zeros((num_parts, 6, 4))
    g[:, 0, 0] = -0.01
    g[:, 1, 2] = 1.0
    g[:, 2, 1] = np.arange(num_parts) / num_parts - 0.5
    g[:, 3, 1] = (np.arange(num_parts) + 1) / num_parts - 0.5
    g[:, 4, 3], g[:, 5, 3] = -0.5, 0.5
    return g
