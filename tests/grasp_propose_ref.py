"""fp64 numpy restatement of the grasp-proposal contract (include/gg_raster.h gg_grasp_propose, PARITY.md "Grasp
proposals"), written from the contract and used by tests/test_grasp_propose_host.py and
tests/test_grasp_propose_gpu.py.  One seed at a time over all points; every elementwise operation is rounded once
(numpy evaluates each ufunc separately, so nothing is contracted), in the contract's order, so the tube membership,
the extremes and their indices, the counts and `valid` are those of the kernel bit for bit; the rows go through
sqrt, sin and cos and agree to rounding.  Independent of the library."""
import math

import numpy as np

DEFAULTS = dict(tube_radius=0.003, max_width=0.10, min_width=0.005, clearance=0.005, depth=0.02, height=0.02,
                min_weight=0.0, min_align=0.0, up=(0.0, 0.0, 1.0), num_approach=8)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def frame(b, up):
    """(a_0, c_0, fallback taken) of a unit closing axis b: the approach closest to -up, perpendicular to b."""
    v = -np.asarray(up, np.float64)
    e = v - b * _dot(b, v)
    fallback = bool(_dot(e, e) < 1e-12 * _dot(v, v))
    if fallback:
        k = int(np.argmin(np.abs(b)))                  # first occurrence: the smallest k on a tie
        v = np.zeros(3)
        v[k] = 1.0
        e = v - b * _dot(b, v)
    a0 = e / math.sqrt(_dot(e, e))
    return a0, _cross(a0, b), fallback


def restate(points, normals, weights, seeds, **kw):
    """dict of numpy arrays: pair_idx (S, 2) int32, tube_count (S,) int32, span (S,) float64, valid (S,) bool,
    rows (S, K, 17) float64, and for the tests mid (S, 3), axis (S, 3), fallback (S,) bool (NaN / False when the
    seed is not valid)."""
    o = dict(DEFAULTS)
    o.update(kw)
    r, W, w0, c = (float(o[k]) for k in ("tube_radius", "max_width", "min_width", "clearance"))
    depth, height, K = float(o["depth"]), float(o["height"]), int(o["num_approach"])
    aa = float(o["min_align"]) * float(o["min_align"])
    up = np.asarray(o["up"], np.float64)
    rr, ww, w0w0 = r * r, W * W, w0 * w0
    wc = W - 2.0 * c
    wcwc = wc * wc
    P = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    Nn = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
    w = np.asarray(weights, np.float32).astype(np.float64).reshape(-1)
    seeds = np.asarray(seeds).astype(np.int64).reshape(-1)
    n_pts, S = P.shape[0], seeds.shape[0]
    with np.errstate(invalid="ignore"):
        part = np.isfinite(P).all(1) & np.isfinite(Nn).all(1) & (w > float(o["min_weight"]))
    idx = np.nonzero(part)[0]
    Pp = P[idx]
    out = dict(pair_idx=np.full((S, 2), -1, np.int32), tube_count=np.zeros(S, np.int32), span=np.full(S, np.nan),
               valid=np.zeros(S, bool), rows=np.full((S, K, 17), np.nan), mid=np.full((S, 3), np.nan),
               axis=np.full((S, 3), np.nan), fallback=np.zeros(S, bool))
    for g in range(S):
        i = int(seeds[g])
        if not (0 <= i < n_pts and part[i]):
            continue
        p, n = P[i], Nn[i]
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        if not nn > 0.0:
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            d0, d1, d2 = Pp[:, 0] - p[0], Pp[:, 1] - p[1], Pp[:, 2] - p[2]
            s = (n[0] * d0 + n[1] * d1) + n[2] * d2
            dd = (d0 * d0 + d1 * d1) + d2 * d2
            ss = s * s
            tube = (dd * nn - ss <= rr * nn) & (ss <= ww * nn)
        st, it = s[tube], idx[tube]
        out["tube_count"][g] = len(st)
        if len(st) == 0:                                # cannot happen: the seed is in its own tube
            continue
        klo, khi = int(np.argmin(st)), int(np.argmax(st))            # first occurrence: the smallest index
        slo, shi, jlo, jhi = st[klo], st[khi], int(it[klo]), int(it[khi])
        out["pair_idx"][g] = (jlo, jhi)
        q = shi - slo
        qq = q * q
        sq = math.sqrt(nn)
        sp = q / sq
        out["span"][g] = sp

        def align(j):
            a = Nn[j]
            gj = (n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]
            mj = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
            return bool(mj > 0.0 and gj * gj >= aa * (nn * mj)), gj, mj
        al, glo, mlo = align(jlo)
        ah, ghi, mhi = align(jhi)
        if not (qq >= w0w0 * nn and qq <= wcwc * nn and al and ah):
            continue
        out["valid"][g] = True
        b = n / sq
        m = p + b * ((slo + shi) / (2.0 * sq))
        a0, c0, fb = frame(b, up)
        out["mid"][g], out["axis"][g], out["fallback"][g] = m, b, fb
        score = (abs(glo) * abs(ghi)) / (nn * math.sqrt(mlo * mhi))
        phi = (2.0 * math.pi * np.arange(K)) / K
        a = np.cos(phi)[:, None] * a0 + np.sin(phi)[:, None] * c0               # (K, 3)
        ck = np.stack([a[:, 1] * b[2] - a[:, 2] * b[1], a[:, 2] * b[0] - a[:, 0] * b[2],
                       a[:, 0] * b[1] - a[:, 1] * b[0]], 1)
        row = out["rows"][g]
        row[:, 0], row[:, 1], row[:, 2], row[:, 3] = score, sp + 2.0 * c, height, depth
        row[:, 4:13] = np.stack([a, np.broadcast_to(b, (K, 3)), ck], 2).reshape(K, 9)     # columns (a_k, b, c_k)
        row[:, 13:16] = m - (0.5 * depth) * a
        row[:, 16] = 0.0
    return out


# ------------------------------------------------------------------------------------------------
# shapes the tests share
# ------------------------------------------------------------------------------------------------
def box_faces(size, h, centre=(0.0, 0.0, 0.0)):
    """Points on the six faces of a box with sides `size` (multiples of h), on a grid of pitch h whose points sit
    h / 2 inside every edge (no point on an edge), with the outward face normals.  Opposite faces carry the same
    grid, so every point has an exact antipode.  Returns points (n, 3), normals (n, 3) float64."""
    size, centre = np.asarray(size, np.float64), np.asarray(centre, np.float64)
    pts, nrm = [], []
    for ax in range(3):
        u, v = [k for k in range(3) if k != ax]
        gu = (np.arange(int(round(size[u] / h))) + 0.5) * h - 0.5 * size[u]
        gv = (np.arange(int(round(size[v] / h))) + 0.5) * h - 0.5 * size[v]
        U, V = (a.ravel() for a in np.meshgrid(gu, gv, indexing="ij"))
        for sgn in (-1.0, 1.0):
            p = np.zeros((len(U), 3))
            p[:, ax], p[:, u], p[:, v] = sgn * 0.5 * size[ax], U, V
            nr = np.zeros((len(U), 3))
            nr[:, ax] = sgn
            pts.append(p + centre)
            nrm.append(nr)
    return np.concatenate(pts), np.concatenate(nrm)
