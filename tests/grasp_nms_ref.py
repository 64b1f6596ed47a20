"""fp64 numpy restatement of the grasp-NMS contract (include/gg_raster.h gg_grasp_nms, PARITY.md "Grasp NMS"), written
from the contract and used by tests/test_grasp_nms_host.py and tests/test_grasp_nms_gpu.py.  Every decision is a
comparison of fp64 sums of products of fp32 inputs, each elementwise operation rounded once (numpy does not contract)
and in the contract's order, so keep, suppressor, kept and num_kept are those of the kernel bit for bit.

restate is a plain double loop: over `order`, and for each row over the rows kept so far (that inner loop is one
numpy expression over the kept rows, in their order)."""
import numpy as np


def poses(grasps):
    """(R (M, 3, 3), t (M, 3), part (M,)) in fp64 from the fp32 rows; part: all 12 entries finite."""
    G = np.asarray(grasps, np.float32).astype(np.float64).reshape(-1, 17)
    R, t = G[:, 4:13].reshape(-1, 3, 3), G[:, 13:16]
    return R, t, np.isfinite(G[:, 4:16]).all(1)


def pair_terms(Ri, ti, Rj, tj):
    """(dd, tr, tr_s) of pose i against the poses j (leading axes broadcast), in the contract's order."""
    d0, d1, d2 = ti[..., 0] - tj[..., 0], ti[..., 1] - tj[..., 1], ti[..., 2] - tj[..., 2]
    dd = (d0 * d0 + d1 * d1) + d2 * d2
    c = [(Ri[..., 0, k] * Rj[..., 0, k] + Ri[..., 1, k] * Rj[..., 1, k]) + Ri[..., 2, k] * Rj[..., 2, k]
         for k in range(3)]
    return dd, (c[0] + c[1]) + c[2], (c[0] - c[1]) - c[2]


def near_from_terms(dd, tr, trs, translation, cos_rotation, symmetric):
    tt, bound = float(translation) * float(translation), 1.0 + 2.0 * float(cos_rotation)
    with np.errstate(invalid="ignore"):
        rot = (tr >= bound) | (trs >= bound) if symmetric else (tr >= bound)
        return (dd <= tt) & rot


def all_pairs(grasps, translation, cos_rotation, symmetric):
    """dict of (M, M) arrays: dd, tr, trs and near (False wherever a row does not take part)."""
    R, t, part = poses(grasps)
    with np.errstate(invalid="ignore", over="ignore"):
        dd, tr, trs = pair_terms(R[:, None], t[:, None], R[None], t[None])
    near = near_from_terms(dd, tr, trs, translation, cos_rotation, symmetric) & part[:, None] & part[None]
    return dict(dd=dd, tr=tr, trs=trs, near=near, part=part)


def restate(grasps, order, translation, cos_rotation, symmetric=True):
    """dict: keep (M,) bool, suppressor (M,) int32, kept (A,) int32 padded with -1, num_kept int."""
    R, t, part = poses(grasps)
    m = R.shape[0]
    order = np.asarray(order, np.int64).reshape(-1)
    keep, suppressor = np.zeros(m, bool), np.full(m, -2, np.int32)
    kept = []
    for r in order:
        if not (0 <= r < m) or not part[r]:
            continue
        if kept:
            k = np.asarray(kept)
            near = near_from_terms(*pair_terms(R[r], t[r], R[k], t[k]), translation, cos_rotation, symmetric)
            hit = np.nonzero(near)[0]
            if hit.size:
                suppressor[r] = k[hit[0]]
                continue
        keep[r], suppressor[r] = True, -1
        kept.append(int(r))
    out = np.full(order.shape[0], -1, np.int32)
    out[:len(kept)] = kept
    return dict(keep=keep, suppressor=suppressor, kept=out, num_kept=len(kept))


def clustered_rows(rng, m, clusters, spread_t=0.01, spread_r=0.15, box=0.15, twins=True):
    """m GraspGroup rows in `clusters` pose clusters: each row is its cluster's pose moved by up to spread_t and
    turned by up to about spread_r radians; with `twins`, every other row is also turned half a turn about its
    approach axis (b -> -b, c -> -c)."""
    from grasp_ref import grasp_rows, rotation
    Rc, tc = rotation(rng, clusters), rng.uniform(-box, box, size=(clusters, 3))
    which = rng.integers(0, clusters, size=m)
    small = rng.normal(size=(m, 3)) * (spread_r / 3.0)
    R = np.empty((m, 3, 3))
    for i in range(m):
        a = small[i]
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        q, _ = np.linalg.qr(np.eye(3) + K + 0.5 * K @ K)          # near exp(K): a small turn, orthonormal
        q = q * np.sign(np.diag(q))                               # the factor near the identity
        R[i] = Rc[which[i]] @ q
        if twins and i % 2:
            R[i] = R[i] * np.array([1.0, -1.0, -1.0])
    t = tc[which] + rng.uniform(-spread_t, spread_t, size=(m, 3))
    return grasp_rows(R, t, 0.05, 0.02, 0.02, score=rng.random(m))
