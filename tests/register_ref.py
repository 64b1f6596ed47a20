"""fp64 numpy restatement of the registration contract (include/gg_raster.h gg_cloud_frames / gg_icp_step and
gaussiangrasper_amd/register.py): brute-force neighbours, np.linalg.eigh, the same operation order for the moved
source points, the distances and the rows' terms.  Test infrastructure only; imports nothing from the package."""
import numpy as np

SINGULAR_REL = 2.0 ** -40


def dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross3(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1],
                     x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def sqdist(a, b):
    """(len(a), len(b)) squared distances, (dx dx + dy dy) + dz dz on b - a."""
    d = b[None, :, :] - a[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# ------------------------------------------------------------------------------------------------
# the scene of the tests
# ------------------------------------------------------------------------------------------------
def surface(n, seed):
    """n points of the test surface and their intensities, rounded to fp32 (returned as fp64)."""
    r = np.random.default_rng(seed)
    xy = r.uniform(-0.15, 0.15, (n, 2))
    z = 0.02 * np.sin(25 * xy[:, 0]) * np.cos(20 * xy[:, 1]) + 0.01 * np.sin(60 * xy[:, 0] + 1) + r.normal(0, 3e-4, n)
    inten = 0.5 + 0.25 * np.sin(40 * xy[:, 0]) + 0.25 * np.cos(35 * xy[:, 1] + 0.5)
    return np.c_[xy, z].astype(np.float32).astype(np.float64), inten.astype(np.float32).astype(np.float64)


def surface_height(x, y):
    return 0.02 * np.sin(25 * x) * np.cos(20 * y) + 0.01 * np.sin(60 * x + 1)


def surface_intensity(x, y):
    return 0.5 + 0.25 * np.sin(40 * x) + 0.25 * np.cos(35 * y + 0.5)


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    if th < 1e-15:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rigid(w, t):
    T = np.eye(4)
    T[:3, :3] = rodrigues(w)
    T[:3, 3] = t
    return T


TRUE_MOTION = rigid([0.02, -0.015, 0.03], [0.006, -0.004, 0.003])     # source frame -> target frame


def scene():
    """Target (6000) and source (3000) of the tests: the source is the surface seen from a frame moved by the
    inverse of TRUE_MOTION.  Everything fp32-representable."""
    P, I = surface(6000, 1)
    S0, Is = surface(3000, 2)
    Gi = np.linalg.inv(TRUE_MOTION)
    S = (S0 @ Gi[:3, :3].T + Gi[:3, 3]).astype(np.float32).astype(np.float64)
    return P, I, S, Is


def motion_error(T):
    """(Frobenius norm of the rotation error, length of the translation error) of T against TRUE_MOTION."""
    E = T @ np.linalg.inv(TRUE_MOTION)
    return float(np.linalg.norm(E[:3, :3] - np.eye(3))), float(np.linalg.norm((T - TRUE_MOTION)[:3, 3]))


# ------------------------------------------------------------------------------------------------
# surface frames
# ------------------------------------------------------------------------------------------------
def neighbours(P, radius, chunk=512):
    """Per point the ascending indices within the radius (itself included); none for non-finite points."""
    P = np.asarray(P, dtype=np.float64)
    fin = np.isfinite(P).all(axis=1)
    r2 = radius * radius
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, len(P), chunk):
            d2 = sqdist(P[a:a + chunk], P)
            ok = (d2 <= r2) & fin[None, :] & fin[a:a + chunk, None]
            out += [np.nonzero(row)[0] for row in ok]
    return out


def cloud_frames(P, I, radius):
    """normals (N, 3), gradients (N, 3), count (N,) int32, valid (N,) bool and the relative eigen-gap
    (l1 - l0) / l2 (N,) of every point, all fp64 and unrounded."""
    P = np.asarray(P, dtype=np.float64)
    I = np.asarray(I, dtype=np.float64)
    n = len(P)
    nrm = np.full((n, 3), np.nan)
    grad = np.zeros((n, 3))
    gap = np.zeros(n)
    nb = neighbours(P, radius)
    count = np.array([len(x) for x in nb], dtype=np.int32)
    for i, x in enumerate(nb):
        c = len(x)
        if c < 3:
            continue
        Q = P[x]
        D = Q - Q.mean(axis=0)
        w, v = np.linalg.eigh(D.T @ D)
        e = v[:, 0]
        e = e * (1.0 if e[int(np.argmax(np.abs(e)))] >= 0 else -1.0)
        nrm[i] = e
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
        if c < 4:
            continue
        o = x[x != i]
        u = P[o] - P[i]
        A = u - np.outer(u @ e, e)
        tr = float((A * A).sum())
        k = float(c - 1)
        M = A.T @ A + (k * k) * np.outer(e, e)
        rhs = A.T @ (I[o] - I[i])
        det = np.linalg.det(M)
        if det > SINGULAR_REL * (k * k) * (0.5 * tr) ** 2:
            grad[i] = np.linalg.solve(M, rhs)
    return nrm, grad, count, count >= 3, gap


# ------------------------------------------------------------------------------------------------
# one linearisation
# ------------------------------------------------------------------------------------------------
def move(T, S):
    """s = R p + t as ((r0 x + r1 y) + r2 z) + t per row."""
    T = np.asarray(T, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    return np.stack([((T[r, 0] * S[:, 0] + T[r, 1] * S[:, 1]) + T[r, 2] * S[:, 2]) + T[r, 3] for r in range(3)],
                    axis=1)


def correspondences(s, P, valid, max_dist, chunk=512):
    """(corr (M,) int64 with -1 for none, squared distance (M,)) and the two smallest squared distances per point
    (M, 2) among the usable targets (inf where there are fewer)."""
    P = np.asarray(P, dtype=np.float64)
    usable = np.asarray(valid, dtype=bool) & np.isfinite(P).all(axis=1)
    md2 = max_dist * max_dist
    corr = np.full(len(s), -1, dtype=np.int64)
    best = np.full(len(s), np.inf)
    two = np.full((len(s), 2), np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, len(s), chunk):
            d2 = sqdist(s[a:a + chunk], P)
            d2 = np.where(usable[None, :] & (d2 <= md2), d2, np.inf)
            j = np.argmin(d2, axis=1)                          # the first minimum: the smaller index on ties
            b = d2[np.arange(len(j)), j]
            hit = np.isfinite(b)
            corr[a:a + chunk] = np.where(hit, j, -1)
            best[a:a + chunk] = b
            k = min(2, d2.shape[1])
            two[a:a + chunk, :k] = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)
    return corr, best, two


def rows(s, q, n, d, i_s, i_q, lam):
    """(Jg (K, 6), rg (K,), Jp (K, 6), rp (K,), r_G, r_I) of K correspondences, weights included in J and r."""
    wg, wp = np.sqrt(lam), np.sqrt(1.0 - lam)
    r_g = dot3(s - q, n)
    Jg = np.concatenate([wg * cross3(s, n), wg * n], axis=1)
    w = (s - r_g[:, None] * n) - q
    r_i = i_s - (i_q + dot3(d, w))
    g = -(d - dot3(d, n)[:, None] * n)
    Jp = np.concatenate([wp * cross3(s, g), wp * g], axis=1)
    return Jg, wg * r_g, Jp, wp * r_i, r_g, r_i


TRIU = [(i, j) for i in range(6) for j in range(i, 6)]


def icp_sums(S, Is, P, I, normals, gradients, valid, T, max_dist, lam):
    """(sums (32,), abs_sums (32,), corr (M,)) of gg_icp_step; np.sum's pairwise order."""
    s = move(T, S)
    P = np.asarray(P, dtype=np.float64)
    corr, best, _ = correspondences(s, P, valid, max_dist)
    hit = corr >= 0
    j = corr[hit]
    sums, asum = np.zeros(32), np.zeros(32)
    if hit.any():
        Jg, rg, Jp, rp, r_g, r_i = rows(s[hit], P[j], np.asarray(normals, dtype=np.float64)[j],
                                        np.asarray(gradients, dtype=np.float64)[j],
                                        np.asarray(Is, dtype=np.float64)[hit], np.asarray(I, dtype=np.float64)[j], lam)
        for o, (a, b) in enumerate(TRIU):
            x, y = Jg[:, a] * Jg[:, b], Jp[:, a] * Jp[:, b]
            sums[o], asum[o] = (x + y).sum(), (np.abs(x) + np.abs(y)).sum()
        for a in range(6):
            x, y = Jg[:, a] * rg, Jp[:, a] * rp
            sums[21 + a], asum[21 + a] = (x + y).sum(), (np.abs(x) + np.abs(y)).sum()
        sums[27:31] = [hit.sum(), best[hit].sum(), (r_g * r_g).sum(), (r_i * r_i).sum()]
        asum[27:31] = sums[27:31]
    return sums, asum, corr


def unpack(sums):
    A = np.zeros((6, 6))
    for o, (a, b) in enumerate(TRIU):
        A[a, b] = A[b, a] = sums[o]
    return A, np.array(sums[21:27])


def solve_step(sums, T):
    """(T', ok): T' = [Rodrigues(w) | v] T with [w, v] = solve(J^T J, -J^T r)."""
    A, b = unpack(sums)
    if not (np.isfinite(A).all() and np.isfinite(b).all()) or np.linalg.matrix_rank(A) < 6:
        return T, False
    x = np.linalg.solve(A, -b)
    return rigid(x[:3], x[3:]) @ T, True


# ------------------------------------------------------------------------------------------------
# the pipeline
# ------------------------------------------------------------------------------------------------
def voxel_downsample(P, C, voxel):
    """Mean position and colour per occupied voxel, ordered by voxel key, fp64."""
    P = np.asarray(P, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    lo = P.min(axis=0) - 0.5 * voxel
    idx = np.floor((P - lo) / voxel).astype(np.int64)
    dims = idx.max(axis=0) + 1
    key = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    out_p, out_c = np.zeros((len(cnt), 3)), np.zeros((len(cnt), C.shape[1]))
    np.add.at(out_p, inv, P)
    np.add.at(out_c, inv, C)
    return out_p / cnt[:, None], out_c / cnt[:, None]


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def colored_icp(S, Sc, P, Pc, init=None, voxel_radius=(0.02, 0.01, 0.005), max_iter=(30, 20, 10), lam=0.968):
    """(T, fitness, inlier_rmse, iterations per scale): the loop of register.colored_icp with every device array
    rounded to fp32 where the package rounds it.  Sc / Pc None: no colours (lam must be 1)."""
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    iters = []
    fit = rmse = 0.0
    for v, n_it in zip(voxel_radius, max_iter):
        sc = np.zeros((len(S), 3)) if Sc is None else Sc
        pc = np.zeros((len(P), 3)) if Pc is None else Pc
        s, sc = voxel_downsample(S, sc, v)
        p, pc = voxel_downsample(P, pc, v)
        s, p = f32(s), f32(p)
        i_s, i_p = f32(sc.mean(axis=1)), f32(pc.mean(axis=1))
        nrm, grad, _, valid, _ = cloud_frames(p, i_p, 2.0 * v)
        nrm, grad = f32(nrm), f32(grad)
        prev = None
        k = 0
        while True:
            sums, _, _ = icp_sums(s, i_s, p, i_p, nrm, grad, valid, T, v, lam)
            inl = sums[27]
            fit = inl / len(s)
            rmse = float(np.sqrt(sums[28] / inl)) if inl > 0 else 0.0
            if prev is not None and abs(prev[0] - fit) < 1e-6 and abs(prev[1] - rmse) < 1e-6:
                break
            if k == n_it:
                break
            prev = (fit, rmse)
            T, ok = solve_step(sums, T)
            if not ok:
                break
            k += 1
        iters.append(k)
    return T, fit, rmse, iters
