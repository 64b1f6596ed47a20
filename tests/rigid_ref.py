"""TEST-ONLY restatement of gg_rigid_fwd / gg_rigid_bwd (include/gg_raster.h, csrc/rigid.hip) in numpy.

Forward, a selected row (mask byte non-zero, or no mask), every fp32 input widened to fp64:
    m'_a = (float)(((R[a][0] x + R[a][1] y) + R[a][2] z) + t[a])
    q'   = (float)(qt (x) q): the Hamilton product, each component four fp64 products added left to right,
           w = w1 w2 - x1 x2 - y1 y2 - z1 z2, x = w1 x2 + x1 w2 + y1 z2 - z1 y2,
           y = w1 y2 - x1 z2 + y1 w2 + z1 x2, z = w1 z2 + x1 y2 - y1 x2 + z1 w2, rounded once.
Nothing is normalised; a row not selected is copied byte for byte.
Backward per row: v_m[b] = (float)((R[0][b] g0 + R[1][b] g1) + R[2][b] g2), v_q = (float)(conj(qt) (x) g_q); rows not
selected are copied; a missing cotangent is zeros.
Pose sums over the selected rows: v_rt[a][b] = sum g_a p_b, v_rt[a][3] = sum g_a, v_qt = sum g_q (x) conj(q), terms in
fp64, in the order of csrc/ordered_sum.h: per workgroup of 256 rows the xor butterfly of each wave (offsets 32 ... 1),
((w0 + w1) + w2) + w3 over the four waves; then 16 chains (chain c adds slab rows c, c + 16, ... from 0; the chains are
added 0, 1, ... 15); the totals rounded to fp32.

numpy does not contract, and every operation here is one IEEE fp64 operation, so the restatement's bits are the
kernel's contract."""
import math

import numpy as np

ROWS, WAVE, CHAINS = 256, 64, 16


def quat_mul(a, b):
    """Hamilton product of wxyz quaternions (..., 4), each component left to right"""
    w1, x1, y1, z1 = (a[..., k] for k in range(4))
    w2, x2, y2, z2 = (b[..., k] for k in range(4))
    return np.stack((((w1 * w2 - x1 * x2) - y1 * y2) - z1 * z2, ((w1 * x2 + x1 * w2) + y1 * z2) - z1 * y2,
                     ((w1 * y2 - x1 * z2) + y1 * w2) + z1 * x2, ((w1 * z2 + x1 * y2) - y1 * x2) + z1 * w2), -1)


def conj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def selected(n, mask):
    return np.ones(n, bool) if mask is None else np.asarray(mask) != 0


def forward64(means, quats, mask, rt, qt):
    """the forward in fp64 without the final rounding (any float dtype in, fp64 out)"""
    m, q = np.asarray(means, np.float64), np.asarray(quats, np.float64)
    rt, qt = np.asarray(rt, np.float64).reshape(3, 4), np.asarray(qt, np.float64).reshape(4)
    sel = selected(len(m), mask)
    x, y, z = m[:, 0:1], m[:, 1:2], m[:, 2:3]
    moved = ((rt[:, 0] * x + rt[:, 1] * y) + rt[:, 2] * z) + rt[:, 3]
    turned = quat_mul(qt[None], q)
    return np.where(sel[:, None], moved, m), np.where(sel[:, None], turned, q)


def forward(means, quats, mask, rt, qt):
    """fp32 in, fp32 out: the kernel's bytes"""
    means, quats = np.asarray(means, np.float32), np.asarray(quats, np.float32)
    m64, q64 = forward64(means, quats, mask, rt, qt)
    sel = selected(len(means), mask)[:, None]
    with np.errstate(all="ignore"):
        return (np.where(sel, m64.astype(np.float32), means), np.where(sel, q64.astype(np.float32), quats))


def rows64(n, mask, rt, qt, g_means, g_quats):
    """per-row backward in fp64, without the final rounding"""
    rt, qt = np.asarray(rt, np.float64).reshape(3, 4), np.asarray(qt, np.float64).reshape(4)
    sel = selected(n, mask)
    gm = np.zeros((n, 3)) if g_means is None else np.asarray(g_means, np.float64)
    gq = np.zeros((n, 4)) if g_quats is None else np.asarray(g_quats, np.float64)
    g0, g1, g2 = gm[:, 0:1], gm[:, 1:2], gm[:, 2:3]
    with np.errstate(all="ignore"):                  # a NaN cotangent in a row that is only copied
        vm = (rt[0, :3] * g0 + rt[1, :3] * g1) + rt[2, :3] * g2
        vq = quat_mul(conj(qt)[None], gq)
    return np.where(sel[:, None], vm, gm), np.where(sel[:, None], vq, gq)


def terms64(means, quats, mask, g_means, g_quats):
    """(N, 16) fp64: every row's term of the sixteen sums (zeros for rows not selected, whatever their cotangent),
    and (N, 16) the sums of the absolute products behind each term"""
    m, q = np.asarray(means, np.float64), np.asarray(quats, np.float64)
    n = len(m)
    sel = selected(n, mask)
    gm = np.zeros((n, 3)) if g_means is None else np.asarray(g_means, np.float64)
    gq = np.zeros((n, 4)) if g_quats is None else np.asarray(g_quats, np.float64)
    t, a = np.zeros((n, 16)), np.zeros((n, 16))
    with np.errstate(all="ignore"):
        for r in range(3):
            t[:, 4 * r:4 * r + 3] = gm[:, r:r + 1] * m
            t[:, 4 * r + 3] = gm[:, r]
        t[:, 12:] = quat_mul(gq, conj(q))
        a[:, :12] = np.abs(t[:, :12])
        a[:, 12:] = _abs_quat_terms(gq, q)
    t[~sel] = 0.0
    a[~sel] = 0.0
    return t, a


def _abs_quat_terms(g, q):
    """sum of |products| of every component of g (x) conj(q)"""
    ag, aq = np.abs(g), np.abs(q)
    w1, x1, y1, z1 = (ag[:, k] for k in range(4))
    w2, x2, y2, z2 = (aq[:, k] for k in range(4))
    return np.stack((w1 * w2 + x1 * x2 + y1 * y2 + z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 + z1 * y2,
                     w1 * y2 + x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 + y1 * x2 + z1 * w2), -1)


def ordered_sums(terms):
    """(N, 16) fp64 terms -> (16,) fp64 totals in the kernels' order (module docstring)"""
    n = len(terms)
    nrows = (n + ROWS - 1) // ROWS
    pad = np.zeros((nrows * ROWS, 16))
    pad[:n] = terms
    v = pad.reshape(nrows, ROWS // WAVE, WAVE, 16)
    lane = np.arange(WAVE)
    o = WAVE // 2
    while o > 0:
        v = v + v[:, :, lane ^ o, :]
        o >>= 1
    w = v[:, :, 0, :]
    slab = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]                      # (nrows, 16)
    chains = np.zeros((CHAINS, 16))
    for c in range(CHAINS):
        acc = np.zeros(16)
        for r in range(c, nrows, CHAINS):
            acc = acc + slab[r]
        chains[c] = acc
    total = chains[0].copy()
    for c in range(1, CHAINS):
        total = total + chains[c]
    return total


def backward(means, quats, mask, rt, qt, g_means, g_quats):
    """fp32 in -> dict: v_means, v_quats (fp32, the kernel's bytes), v_rt (12,), v_qt (4,) fp32 in the kernels' order,
    `exact` (16,) the exactly rounded fp64 totals (math.fsum of the terms), `abs` (16,) the sums of the absolute
    products, `count` the number of selected rows"""
    means, quats = np.asarray(means, np.float32), np.asarray(quats, np.float32)
    n = len(means)
    sel = selected(n, mask)
    vm64, vq64 = rows64(n, mask, rt, qt, g_means, g_quats)
    gm = np.zeros((n, 3), np.float32) if g_means is None else np.asarray(g_means, np.float32)
    gq = np.zeros((n, 4), np.float32) if g_quats is None else np.asarray(g_quats, np.float32)
    with np.errstate(all="ignore"):
        v_means = np.where(sel[:, None], vm64.astype(np.float32), gm)
        v_quats = np.where(sel[:, None], vq64.astype(np.float32), gq)
    t, a = terms64(means, quats, mask, g_means, g_quats)
    tot = ordered_sums(t).astype(np.float32)
    return {"v_means": v_means, "v_quats": v_quats, "v_rt": tot[:12], "v_qt": tot[12:],
            "exact": np.array([math.fsum(t[:, k]) for k in range(16)]),
            "abs": np.array([math.fsum(a[:, k]) for k in range(16)]), "count": int(sel.sum())}


def vjp64(means, quats, mask, rt, qt, g_means, g_quats):
    """the whole vector-Jacobian product in fp64 (no fp32 rounding, plain sums): v_means, v_quats, v_rt (3, 4), v_qt"""
    n = len(means)
    vm, vq = rows64(n, mask, rt, qt, g_means, g_quats)
    t, _ = terms64(means, quats, mask, g_means, g_quats)
    s = t.sum(axis=0)
    return vm, vq, s[:12].reshape(3, 4), s[12:]
