"""fp64 numpy restatement of the grasp-filtering contract (include/gg_raster.h gg_grasp_contacts, PARITY.md "Grasp
filtering"), written from the contract and used by tests/test_grasp_host.py and tests/test_grasp_gpu.py.  Every
elementwise operation is rounded once (numpy does not contract), in the contract's order, so the region and finger
box decisions, the contacts and the patch membership are those of the kernel bit for bit; sums are taken in numpy's
order, so normals, angles and weights agree to rounding.

Per grasp, only the points within a slab of x around the grasp centre are evaluated: the slab's half-width bounds
|p - t| over the grasp's boxes for any rotation within 1e-3 of orthonormal (every test grasp), with a wide margin,
so the slab never removes a point the exact test keeps."""
import math

import numpy as np

DEFAULTS = dict(depth_base=0.02, finger_width=0.004, band=0.003, mu=0.5, min_weight=0.0, max_collision=math.inf)


def _angle(x, b):
    c = np.array([x[1] * b[2] - x[2] * b[1], x[2] * b[0] - x[0] * b[2], x[0] * b[1] - x[1] * b[0]])
    return math.atan2(math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), (x[0] * b[0] + x[1] * b[1]) + x[2] * b[2])


def restate(points, normals, weights, grasps, **kw):
    """dict of numpy arrays: contact_idx (M, 2) int32, normals (M, 2, 3), angles (M, 2), region_count (M,),
    region_weight (M,), collision_weight (M,), feasible (M,) bool, valid (M,) bool."""
    o = dict(DEFAULTS)
    o.update(kw)
    db, fw, band = float(o["depth_base"]), float(o["finger_width"]), float(o["band"])
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    n = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
    w = np.asarray(weights, np.float32).astype(np.float64).reshape(-1)
    G = np.asarray(grasps, np.float32).astype(np.float64).reshape(-1, 17)
    m = G.shape[0]
    with np.errstate(invalid="ignore"):
        part = np.isfinite(p).all(1) & np.isfinite(n).all(1) & (w > float(o["min_weight"]))
    idx = np.nonzero(part)[0]
    order = np.argsort(p[idx, 0], kind="stable")
    sx, sidx = p[idx[order], 0], idx[order]
    out = dict(contact_idx=np.full((m, 2), -1, np.int32), normals=np.full((m, 2, 3), np.nan),
               angles=np.full((m, 2), np.nan), region_count=np.zeros(m, np.int64), region_weight=np.zeros(m),
               collision_weight=np.zeros(m), feasible=np.zeros(m, bool), valid=np.zeros(m, bool))
    lim = math.atan(float(o["mu"]))
    for g in range(m):
        row = G[g]
        if not (np.isfinite(row).all() and row[1] > 0 and row[2] > 0 and row[3] >= -db):
            continue
        R, t = row[4:13], row[13:16]
        depth, hw, hh = row[3], 0.5 * row[1], 0.5 * row[2]
        lo1, hi1 = -hw - fw, hw + fw
        r = math.sqrt(max(db, abs(depth)) ** 2 + hi1 ** 2 + hh ** 2)
        r = 1.01 * r + 1e-6 * abs(t[0]) + 1e-30
        a, b_ = np.searchsorted(sx, t[0] - r, "left"), np.searchsorted(sx, t[0] + r, "right")
        ci = np.sort(sidx[a:b_])
        P, Nn, W = p[ci], n[ci], w[ci]
        d0, d1, d2 = P[:, 0] - t[0], P[:, 1] - t[1], P[:, 2] - t[2]
        u0 = (R[0] * d0 + R[3] * d1) + R[6] * d2
        u1 = (R[1] * d0 + R[4] * d1) + R[7] * d2
        u2 = (R[2] * d0 + R[5] * d1) + R[8] * d2
        common = (u0 >= -db) & (u0 <= depth) & (np.abs(u2) <= hh)
        reg = common & (np.abs(u1) <= hw)
        fing = common & (((u1 >= lo1) & (u1 < -hw)) | ((u1 > hw) & (u1 <= hi1)))
        cnt = int(reg.sum())
        out["region_count"][g] = cnt
        out["region_weight"][g] = W[reg].sum()
        cw = W[fing].sum()
        out["collision_weight"][g] = cw
        if cnt == 0:
            continue
        ru, ri = u1[reg], ci[reg]
        yl, yr = ru.min(), ru.max()
        out["contact_idx"][g] = (ri[np.argmin(ru)], ri[np.argmax(ru)])     # first occurrence: smallest index
        b = np.array([R[1], R[4], R[7]])
        bn = (b[0] * Nn[:, 0] + b[1] * Nn[:, 1]) + b[2] * Nn[:, 2]
        tw = W[:, None] * Nn
        left, right = reg & (u1 <= yl + band), reg & (u1 >= yr - band)
        NL = (np.where(bn > 0, -1.0, 1.0)[:, None] * tw)[left].sum(0)
        NR = (np.where(bn < 0, -1.0, 1.0)[:, None] * tw)[right].sum(0)
        ll = math.sqrt((NL[0] * NL[0] + NL[1] * NL[1]) + NL[2] * NL[2])
        lr = math.sqrt((NR[0] * NR[0] + NR[1] * NR[1]) + NR[2] * NR[2])
        if not (yl < yr and ll > 0 and lr > 0):
            continue
        hl, hr = NL / ll, NR / lr
        al, ar = _angle(-hl, b), _angle(hr, b)
        out["valid"][g] = True
        out["normals"][g] = (hl, hr)
        out["angles"][g] = (al, ar)
        out["feasible"][g] = max(al, ar) <= lim and cw <= float(o["max_collision"])
    return out


def rotation(rng, n):
    """n random rotations (fp64), QR of Gaussian matrices with det +1."""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[np.linalg.det(q) < 0, :, 0] *= -1
    return q


def grasp_rows(R, t, width, height, depth, score=None, object_id=0.0):
    """(M, 17) float32 rows from rotations (M, 3, 3), translations (M, 3) and per-row or scalar sizes."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    m = R.shape[0]
    g = np.zeros((m, 17), np.float64)
    g[:, 0] = np.linspace(1.0, 0.1, m) if score is None else score
    g[:, 1], g[:, 2], g[:, 3] = width, height, depth
    g[:, 4:13] = R.reshape(m, 9)
    g[:, 13:16] = np.asarray(t, np.float64).reshape(m, 3)
    g[:, 16] = object_id
    return g.astype(np.float32)
