"""numpy fp64 restatement of the arm contracts (include/gg_raster.h gg_arm_fk, gg_arm_follow, gg_arm_clear), in the
operation order the header gives, and the builders of the fixtures the arm tests share.  Every function works on a
batch of rows at once: the operations per row are the header's, one after the other.  Test infrastructure: plain."""
import functools

import numpy as np

import field_ref

FAR = 1 << 30
INT32_MIN = -(1 << 31)
LAW = dict(tol_p=1e-4, tol_r=1e-3, L=0.1, k=1.0, lambda_min=1e-4, max_step=0.2, max_iter=100)


# ------------------------------------------------------------------------------------------------
# the chain
# ------------------------------------------------------------------------------------------------
def unpack(arm, J):
    """the host array of the C entries -> base (12,), fixed (J + 1, 12), axis (J, 3), lo, hi, kind (J,)"""
    a = np.asarray(arm, np.float64).reshape(-1)
    assert a.shape == (12 * (J + 2) + 6 * J,)
    joints = a[12 * (J + 2):].reshape(J, 6)
    return a[:12], a[12:12 * (J + 2)].reshape(J + 1, 12), joints[:, :3], joints[:, 3], joints[:, 4], joints[:, 5]


def pack(base, fixed, axis, lo, hi, kind):
    J = len(axis)
    joints = np.concatenate([np.asarray(axis, np.float64).reshape(J, 3), np.asarray(lo, np.float64).reshape(J, 1),
                             np.asarray(hi, np.float64).reshape(J, 1), np.asarray(kind, np.float64).reshape(J, 1)], 1)
    return np.concatenate([np.asarray(base, np.float64).reshape(12), np.asarray(fixed, np.float64).reshape(-1),
                           joints.reshape(-1)])


def compose(T, B):
    """T B for (N, 12) and (12,) or (N, 12): (a0 b0 + a1 b1) + a2 b2, plus t"""
    T = np.asarray(T, np.float64)
    B = np.broadcast_to(np.asarray(B, np.float64), T.shape)
    out = np.empty_like(T)
    for r in range(3):
        for c in range(3):
            out[:, 3 * r + c] = (T[:, 3 * r] * B[:, c] + T[:, 3 * r + 1] * B[:, 3 + c]) + T[:, 3 * r + 2] * B[:, 6 + c]
        out[:, 9 + r] = ((T[:, 3 * r] * B[:, 9] + T[:, 3 * r + 1] * B[:, 10]) + T[:, 3 * r + 2] * B[:, 11]) + T[:, 9 + r]
    return out


def motion(kind, a, q):
    """M(q) (N, 12) of one joint"""
    q = np.asarray(q, np.float64)
    M = np.zeros((len(q), 12))
    if kind == 0.0:
        c, s = np.cos(q), np.sin(q)
        v = 1.0 - c
        M[:, 0] = c + v * (a[0] * a[0])
        M[:, 1] = (v * (a[0] * a[1])) + s * (-a[2])
        M[:, 2] = (v * (a[0] * a[2])) + s * a[1]
        M[:, 3] = (v * (a[1] * a[0])) + s * a[2]
        M[:, 4] = c + v * (a[1] * a[1])
        M[:, 5] = (v * (a[1] * a[2])) + s * (-a[0])
        M[:, 6] = (v * (a[2] * a[0])) + s * (-a[1])
        M[:, 7] = (v * (a[2] * a[1])) + s * a[0]
        M[:, 8] = c + v * (a[2] * a[2])
    else:
        M[:, 0] = M[:, 4] = M[:, 8] = 1.0
        M[:, 9], M[:, 10], M[:, 11] = q * a[0], q * a[1], q * a[2]
    return M


def fk(arm, J, q, joints=False):
    """frames (N, J + 2, 12); a row with a q that is not finite is NaN.  joints=True: also the joints' world axes
    and origins (N, J, 3) each."""
    base, fixed, axis, _, _, kind = unpack(arm, J)
    q = np.asarray(q, np.float64).reshape(-1, J)
    N = len(q)
    fin = np.isfinite(q).all(1)
    qq = np.where(fin[:, None], q, 0.0)
    frames = np.empty((N, J + 2, 12))
    zs, os_ = np.empty((N, J, 3)), np.empty((N, J, 3))
    T = np.broadcast_to(base, (N, 12)).copy()
    frames[:, 0] = T
    for j in range(J):
        T = compose(T, fixed[j])
        for k in range(3):
            zs[:, j, k] = (T[:, 3 * k] * axis[j, 0] + T[:, 3 * k + 1] * axis[j, 1]) + T[:, 3 * k + 2] * axis[j, 2]
            os_[:, j, k] = T[:, 9 + k]
        T = compose(T, motion(kind[j], axis[j], qq[:, j]))
        frames[:, j + 1] = T
    frames[:, J + 1] = compose(T, fixed[J])
    frames[~fin] = np.nan
    return (frames, zs, os_) if joints else frames


def rotvec(R):
    """(N, 3) rotation vectors of (N, 9) rotations through the quaternion: Shepperd's branches, normalised, w >= 0"""
    R = np.asarray(R, np.float64).reshape(-1, 9)
    t = (R[:, 0] + R[:, 4]) + R[:, 8]
    b0 = (t >= R[:, 0]) & (t >= R[:, 4]) & (t >= R[:, 8])
    b1 = ~b0 & (R[:, 0] >= R[:, 4]) & (R[:, 0] >= R[:, 8])
    b2 = ~b0 & ~b1 & (R[:, 4] >= R[:, 8])
    one = 1.0
    w = np.where(b0, one + t, np.where(b1, R[:, 7] - R[:, 5], np.where(b2, R[:, 2] - R[:, 6], R[:, 3] - R[:, 1])))
    x = np.where(b0, R[:, 7] - R[:, 5], np.where(b1, ((one + R[:, 0]) - R[:, 4]) - R[:, 8],
                                                 np.where(b2, R[:, 3] + R[:, 1], R[:, 6] + R[:, 2])))
    y = np.where(b0, R[:, 2] - R[:, 6], np.where(b1, R[:, 3] + R[:, 1],
                                                 np.where(b2, ((one + R[:, 4]) - R[:, 8]) - R[:, 0], R[:, 7] + R[:, 5])))
    z = np.where(b0, R[:, 3] - R[:, 1], np.where(b1, R[:, 6] + R[:, 2],
                                                 np.where(b2, R[:, 7] + R[:, 5], ((one + R[:, 8]) - R[:, 0]) - R[:, 4])))
    n = np.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    neg = w < 0.0
    w, x, y, z = np.where(neg, -w, w), np.where(neg, -x, x), np.where(neg, -y, y), np.where(neg, -z, z)
    nv = np.sqrt((x * x + y * y) + z * z)
    small = nv < 1e-12
    ang = 2.0 * np.arctan2(nv, w)
    safe = np.where(small, 1.0, nv)
    v = np.stack([x, y, z], 1)
    return np.where(small[:, None], 2.0 * v, ang[:, None] * (v / safe[:, None]))


def columns(kind, zs, os_, p, L):
    """the Jacobian's columns (N, J, 6), rotational rows times L"""
    N, J = zs.shape[:2]
    c = np.zeros((N, J, 6))
    for j in range(J):
        z = zs[:, j]
        if kind[j] == 0.0:
            d = p - os_[:, j]
            c[:, j, 0] = z[:, 1] * d[:, 2] - z[:, 2] * d[:, 1]
            c[:, j, 1] = z[:, 2] * d[:, 0] - z[:, 0] * d[:, 2]
            c[:, j, 2] = z[:, 0] * d[:, 1] - z[:, 1] * d[:, 0]
            c[:, j, 3:] = L * z
        else:
            c[:, j, :3] = z
    return c


def jacobian(arm, J, q, L=1.0):
    """(N, 6, J): the geometric Jacobian of the gripper frame, rotational rows times L"""
    frames, zs, os_ = fk(arm, J, q, joints=True)
    kind = unpack(arm, J)[5]
    return np.swapaxes(columns(kind, zs, os_, frames[:, J + 1, 9:], L), 1, 2)


def pose_error(arm, J, q, target, T=None):
    """(|e_p|, |e_r|, e_p, e_r) of the gripper frame of q (N, J) (or of the gripper poses T (N, 12) themselves) against
    target (N, 12), as step 1 forms them"""
    T = fk(arm, J, q)[:, J + 1] if T is None else T
    tgt = np.asarray(target, np.float64).reshape(-1, 12)
    e = tgt[:, 9:] - T[:, 9:]
    Re = np.empty((len(T), 9))
    for a in range(3):
        for b in range(3):
            Re[:, 3 * a + b] = (tgt[:, 3 * a] * T[:, 3 * b] + tgt[:, 3 * a + 1] * T[:, 3 * b + 1]) \
                + tgt[:, 3 * a + 2] * T[:, 3 * b + 2]
    er = rotvec(Re)
    return (np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]),
            np.sqrt((er[:, 0] * er[:, 0] + er[:, 1] * er[:, 1]) + er[:, 2] * er[:, 2]), e, er)


def follow(arm, J, poses, seeds, tol_p=1e-4, tol_r=1e-3, L=0.1, k=1.0, lambda_min=1e-4, max_step=0.2, max_iter=100,
           decisions=None):
    """(q_out (P, S, W, J), iters (P, S, W) int32, resid (P, S, W, 2), first_fail (P, S) int32).  decisions: a list
    that receives (|e_p|, |e_r|) arrays of every convergence decision made."""
    _, _, _, lo, hi, kind = unpack(arm, J)
    poses = np.asarray(poses, np.float32)
    P, W = poses.shape[:2]
    seeds = np.asarray(seeds, np.float64)
    S = seeds.shape[1]
    N = P * S
    q = seeds.reshape(N, J).copy()
    alive = np.isfinite(q).all(1)
    q = np.minimum(np.maximum(np.where(alive[:, None], q, 0.0), lo), hi)
    q_out = np.full((N, W, J), np.nan)
    iters = np.full((N, W), -1, np.int32)
    resid = np.full((N, W, 2), np.nan)
    first = np.full(N, W, np.int32)
    first[~alive] = 0
    path = np.repeat(np.arange(P), S)
    with np.errstate(all="ignore"):
        for w in range(W):
            tgt = poses[path, w].astype(np.float64)
            bad = alive & ~np.isfinite(tgt).all(1)
            first[bad] = w
            alive &= ~bad
            run = alive.copy()
            it = 0
            while run.any():
                i = np.nonzero(run)[0]
                frames, zs, os_ = fk(arm, J, q[i], joints=True)
                T = frames[:, J + 1]
                np_, nr_, e_p, er = pose_error(arm, J, None, tgt[i], T)
                fin = np.isfinite(np_) & np.isfinite(nr_)
                if decisions is not None:
                    decisions.append((np_[fin], nr_[fin]))
                conv = fin & (np_ <= tol_p) & (nr_ <= tol_r)
                fail = ~conv & (~fin | (it == max_iter))
                c = i[conv]
                q_out[c, w], iters[c, w] = q[c], it
                resid[c, w, 0], resid[c, w, 1] = np_[conv], nr_[conv]
                go = ~conv & ~fail
                e = np.concatenate([e_p, L * er], 1)
                ee = e[:, 0] * e[:, 0]
                for a in range(1, 6):
                    ee = ee + e[:, a] * e[:, a]
                lambda2 = k * ee + lambda_min * lambda_min
                col = columns(kind, zs, os_, T[:, 9:], L)
                A = np.zeros((len(i), 6, 6))
                for j in range(J):
                    for a in range(6):
                        for b in range(a + 1):
                            A[:, a, b] = A[:, a, b] + col[:, j, a] * col[:, j, b]
                for a in range(6):
                    A[:, a, a] = A[:, a, a] + lambda2
                pd = np.ones(len(i), bool)
                for a in range(6):
                    for b in range(a + 1):
                        s = A[:, a, b].copy()
                        for m in range(b):
                            s = s - A[:, a, m] * A[:, b, m]
                        if a == b:
                            pd &= s > 0.0
                            A[:, a, a] = np.sqrt(s)
                        else:
                            A[:, a, b] = s / A[:, b, b]
                y = np.empty((len(i), 6))
                for a in range(6):
                    s = e[:, a].copy()
                    for m in range(a):
                        s = s - A[:, a, m] * y[:, m]
                    y[:, a] = s / A[:, a, a]
                for a in range(5, -1, -1):
                    s = y[:, a].copy()
                    for m in range(a + 1, 6):
                        s = s - A[:, m, a] * y[:, m]
                    y[:, a] = s / A[:, a, a]
                dq = np.empty((len(i), J))
                for j in range(J):
                    s = col[:, j, 0] * y[:, 0]
                    for a in range(1, 6):
                        s = s + col[:, j, a] * y[:, a]
                    dq[:, j] = s
                dqfin = np.isfinite(dq).all(1)
                big = np.abs(np.where(dqfin[:, None], dq, 0.0)).max(1)
                fail |= go & (~pd | ~dqfin)
                go &= pd & dqfin
                over = big > max_step
                scale = np.where(over, max_step / np.where(over, big, 1.0), 1.0)
                step = np.where(over[:, None], dq * scale[:, None], dq)
                g = i[go]
                q[g] = np.minimum(np.maximum(q[g] + step[go], lo), hi)
                f = i[fail]
                first[f] = w
                alive[f] = False
                run[i[conv | fail]] = False
                it += 1
    return (q_out.reshape(P, S, W, J), iters.reshape(P, S, W), resid.reshape(P, S, W, 2), first.reshape(P, S))


def clear(arm, J, dims, grid, dist2, q, spheres, frame, need2, outside):
    """(slack (M,) int32, worst (M,) int32)"""
    q = np.asarray(q, np.float64).reshape(-1, J)
    sp = np.asarray(spheres, np.float32).reshape(-1, 3).astype(np.float64)
    frame = np.asarray(frame, np.int64).reshape(-1)
    need2 = np.asarray(need2, np.int64).reshape(-1)
    grid = np.asarray(grid, np.float64)
    dims = np.asarray(dims, np.int64)
    dist2 = np.asarray(dist2).reshape(dims)
    M, S = len(q), len(sp)
    fin = np.isfinite(q).all(1)
    slack = np.full(M, FAR, np.int64)
    worst = np.full(M, -1, np.int64)
    if S:
        centres = sphere_centres(arm, J, np.where(fin[:, None], q, 0.0), sp, frame)
        with np.errstate(all="ignore"):
            ok = np.isfinite(centres)
            cell = field_ref.cell_index(np.where(ok, centres, 0.0) - grid[:3], grid[3])
        inside = (ok & (cell >= 0) & (cell < dims)).all(2)
        cc = np.clip(cell, 0, dims - 1)
        d = np.where(inside, dist2[cc[..., 0], cc[..., 1], cc[..., 2]].astype(np.int64), int(outside))
        sl = d - need2[None, :]
        slack = sl.min(1)
        worst = np.argmax(sl == slack[:, None], axis=1)             # the lowest index that attains it
    slack[~fin], worst[~fin] = INT32_MIN, -1
    return slack.astype(np.int32), worst.astype(np.int32)


def sphere_centres(arm, J, q, spheres, frame):
    """(M, S, 3) world centres: ((R[k][0] x + R[k][1] y) + R[k][2] z) + t_k with R, t of the sphere's frame"""
    frames = fk(arm, J, q)
    T = frames[:, np.asarray(frame, np.int64)]                       # (M, S, 12)
    sp = np.asarray(spheres, np.float64)
    out = np.empty(T.shape[:2] + (3,))
    for a in range(3):
        out[..., a] = ((T[..., 3 * a] * sp[:, 0] + T[..., 3 * a + 1] * sp[:, 1]) + T[..., 3 * a + 2] * sp[:, 2]) \
            + T[..., 9 + a]
    return out


# ------------------------------------------------------------------------------------------------
# chains
# ------------------------------------------------------------------------------------------------
def matrix(T):
    """12 numbers -> 4 x 4"""
    T = np.asarray(T, np.float64)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = T[:9].reshape(3, 3), T[9:]
    return M


def twelve(M):
    return np.concatenate([M[:3, :3].reshape(-1), M[:3, 3]])


def default_chain():
    from gaussiangrasper_amd.arm import default_arm
    return default_arm().to_array(), 7


def cut_chain():
    """the default arm with its last joint frozen at 0.785: 6 joints, solutions isolated"""
    arm, J = default_chain()
    base, fixed, axis, lo, hi, kind = unpack(arm, J)
    frozen = matrix(fixed[6]) @ matrix(motion(kind[6], axis[6], np.array([0.785]))[0]) @ matrix(fixed[7])
    return pack(base, np.concatenate([fixed[:6], twelve(frozen)[None]]), axis[:6], lo[:6], hi[:6], kind[:6]), 6


def random_chain(J, seed, prismatic=()):
    """J joints about random axes with random fixed transforms (links of 0.1 to 0.3), the joints in `prismatic` sliding"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)

    def pose():
        return np.concatenate([Rotation.random(random_state=rng).as_matrix().reshape(-1), rng.uniform(-0.3, 0.3, 3)])
    axis = rng.normal(size=(J, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    kind = np.array([1.0 if j in prismatic else 0.0 for j in range(J)])
    lo = np.where(kind == 1.0, -0.2, -2.5)
    hi = np.where(kind == 1.0, 0.3, 2.0)
    return pack(pose(), np.stack([pose() for _ in range(J + 1)]), axis, lo, hi, kind), J


def in_limits(arm, J, n, rng, inset=0.25):
    """n configurations uniform in the limits, `inset` away from either end"""
    lo, hi = unpack(arm, J)[3:5]
    return rng.uniform(lo + inset, hi - inset, size=(n, J))


# ------------------------------------------------------------------------------------------------
# fixtures (built once per process)
# ------------------------------------------------------------------------------------------------
NEAR_N, NEAR_SIGMA = 65, 0.05


@functools.lru_cache(maxsize=None)
def near_fixture(which):
    """which: "cut" (6 joints) or "default" (7).  65 in-limit configurations with sigma_min(J) >= 0.05 (rotational
    rows times L = 0.1, as the law weighs them), their gripper poses as float32 (65, 1, 12), seeds within 0.2 rad of the
    truth (65, 1, J) and the restatement's outputs with every convergence decision it made."""
    arm, J = cut_chain() if which == "cut" else default_chain()
    rng = np.random.default_rng(11 if which == "cut" else 12)
    lo, hi = unpack(arm, J)[3:5]
    keep = []
    while len(keep) < NEAR_N:
        q = in_limits(arm, J, 64, rng)
        sig = np.linalg.svd(jacobian(arm, J, q, LAW["L"]), compute_uv=False)[:, -1]
        keep.extend(q[sig >= NEAR_SIGMA])
    truth = np.array(keep[:NEAR_N])
    poses = fk(arm, J, truth)[:, J + 1].astype(np.float32)[:, None, :]
    seeds = np.clip(truth + rng.uniform(-0.2, 0.2, size=truth.shape), lo, hi)[:, None, :]
    decisions = []
    out = follow(arm, J, poses, seeds, decisions=decisions, **LAW)
    return dict(arm=arm, J=J, truth=truth, poses=poses, seeds=seeds, out=out, decisions=decisions)


def near_tolerance(decisions, tol_p, tol_r, rel=1e-6):
    """how many convergence decisions were within `rel` (relative) of a tolerance"""
    n = 0
    for np_, nr_ in decisions:
        n += int((np.abs(np_ - tol_p) <= rel * tol_p).sum()) + int((np.abs(nr_ - tol_r) <= rel * tol_r).sum())
    return n


@functools.lru_cache(maxsize=None)
def random_seed_fixture():
    """16 targets x 16 seeds on the default arm: targets of in-limit configurations that at least 4 of their seeds
    (gaussiangrasper_amd.arm.seeds) reach within max_iter / 2 updates under the restatement."""
    from gaussiangrasper_amd import arm as A
    arm, J = default_chain()
    model = A.default_arm()
    rng = np.random.default_rng(21)
    cand = in_limits(arm, J, 40, rng)
    poses = fk(arm, J, cand)[:, J + 1].astype(np.float32)[:, None, :]
    seeds = A.seeds(model, len(cand), 16, seed=5)
    out = follow(arm, J, poses, seeds, **LAW)
    it = out[1][:, :, 0]
    good = ((it >= 0) & (it <= LAW["max_iter"] // 2)).sum(1) >= 4
    idx = np.nonzero(good)[0][:16]
    return dict(arm=arm, J=J, poses=poses[idx], seeds=seeds[idx], out=tuple(o[idx] for o in out),
                candidates=len(cand), good=int(good.sum()))


@functools.lru_cache(maxsize=None)
def unreachable_fixture():
    """8 targets further from the base than the summed link lengths, 4 seeds each"""
    from gaussiangrasper_amd import arm as A
    from scipy.spatial.transform import Rotation
    arm, J = default_chain()
    fixed = unpack(arm, J)[1]
    span = float(np.linalg.norm(fixed[:, 9:], axis=1).sum())
    rng = np.random.default_rng(31)
    d = rng.normal(size=(8, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    R = Rotation.random(8, random_state=rng).as_matrix().reshape(8, 9)
    poses = np.concatenate([R, d * (span + rng.uniform(0.2, 0.6, size=(8, 1)))], 1).astype(np.float32)[:, None, :]
    seeds = A.seeds(A.default_arm(), 8, 4, seed=6)
    return dict(arm=arm, J=J, span=span, poses=poses, seeds=seeds)


FIELD_DIMS = (40, 36, 44)
FIELD_H = 2.0 ** -5
FIELD_LO = (-0.613, -0.551, -0.013)


@functools.lru_cache(maxsize=None)
def field_fixture():
    """A 40 x 36 x 44 volume of h = 2^-5 about the default arm with a few occupied blocks, 257 in-limit configurations,
    the arm's link spheres and a few gripper-frame ones; `face` counts the sphere centres within 1e-9 of a cell face;
    `keep32` marks the configurations whose gripper-frame centres stay in their cells when F_{J+1} is rounded to
    float32."""
    from gaussiangrasper_amd import arm as A
    from gaussiangrasper_amd.field import need2
    arm, J = default_chain()
    model = A.default_arm()
    occ = np.zeros(FIELD_DIMS, bool)
    occ[4:9, 20:30, 10:16] = True
    occ[28:36, 5:12, 0:6] = True
    occ[18:22, 16:20, 30:40] = True
    occ[10:30, 28:33, 18:21] = True
    dist2 = edt(occ)
    grid = np.array([*FIELD_LO, FIELD_H])
    rng = np.random.default_rng(41)
    q = in_limits(arm, J, 257, rng, inset=0.05)
    c, f, r = model.link_spheres()
    gs = np.array([[0.0, 0.0, 0.0], [-0.03, 0.04, 0.0], [-0.03, -0.04, 0.0], [-0.06, 0.0, 0.0]], np.float32)
    spheres = np.concatenate([c, gs])
    frame = np.concatenate([f, np.full(len(gs), J + 1, np.int32)])
    need = need2(np.concatenate([r, np.full(len(gs), 0.01)]), 0.0, FIELD_H)
    cen = sphere_centres(arm, J, q, spheres.astype(np.float64), frame)
    t = (cen - grid[:3]) / grid[3]
    face = int((np.abs(t - np.round(t)) <= 1e-9 / grid[3]).sum())
    # the gripper-frame spheres through the float32 rounding of F_{J+1}, as gg_field_paths sees it
    T = fk(arm, J, q)[:, J + 1]
    T32 = T.astype(np.float32).astype(np.float64)
    g64 = gs.astype(np.float64)
    c32 = np.empty((len(q), len(gs), 3))
    for a in range(3):
        c32[..., a] = ((T32[:, None, 3 * a] * g64[:, 0] + T32[:, None, 3 * a + 1] * g64[:, 1])
                       + T32[:, None, 3 * a + 2] * g64[:, 2]) + T32[:, None, 9 + a]
    same = (field_ref.cell_index(c32 - grid[:3], grid[3])
            == field_ref.cell_index(cen[:, len(c):] - grid[:3], grid[3])).all((1, 2))
    return dict(arm=arm, J=J, dims=np.array(FIELD_DIMS, np.int32), grid=grid, dist2=dist2, q=q, spheres=spheres,
                frame=frame, need=need, face=face, keep32=same, gripper=gs, poses32=T.astype(np.float32),
                links=len(c))


def edt(occ):
    """exact squared Euclidean distance transform in cells, FAR when nothing is occupied (scipy)"""
    from scipy import ndimage
    if not occ.any():
        return np.full(occ.shape, FAR, np.int32)
    d = ndimage.distance_transform_edt(~occ)
    return np.minimum(np.rint(d * d), FAR).astype(np.int32)
