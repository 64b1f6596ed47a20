"""fp64 numpy restatement of the arm-trajectory contract (include/gg_raster.h "Arm trajectories"): the blended polyline's
grid, gg_traj_time's time law and gg_traj_sample's samples, in the header's operation order.  The paths of a batch are
laid out per path (a handful of numpy operations per piece) and the two passes of the law run over all paths at once,
one grid step per loop turn.  tests/test_trajectory_host.py holds this file against independent forms; the GPU tests
hold the kernels to it to the bit."""
import numpy as np

MAX_JOINTS, MAX_WAYPOINTS, MAX_STEPS = 8, 64, 64
OK, NOT_FINITE, ZERO_SEGMENT, NO_DURATION = 0, 1, 2, 3
MAX_SAMPLES = 1 << 30


def grid_max(W, m):
    """GG_TRAJ_GRID(W, m)"""
    return m * (2 * W - 3) if W >= 2 else 0


def fractions(blend_row, n):
    """f_k as the law takes them: clamped into [0, 1/2], NaN as 0, 0 at both ends."""
    f = np.fmin(np.fmax(np.asarray(blend_row, np.float64)[:n], 0.0), 0.5)
    f[0] = 0.0
    f[n - 1] = 0.0
    return f


def pieces(f, n):
    """[(kind, k, f_k, L)] in path order: kind 0 the line of segment k, kind 1 the blend about waypoint k."""
    out = []
    for k in range(n - 1):
        if k >= 1 and f[k] > 0.0:
            out.append((1, k, f[k], 2.0 * f[k]))
        L = (1.0 - f[k]) - f[k + 1]
        if L > 0.0:
            out.append((0, k, f[k], L))
    return out


class Grid:
    """One path's grid: q (G + 1, J); qp0, qp1, qpp (G, J): q' at the two ends of every interval and q''; delta (G,);
    stop (G + 1,) bool; piece (G,) the index into `pieces`."""

    def __init__(self, way, n, blend_row, m):
        w = np.asarray(way, np.float64)[:n]
        J = w.shape[1]
        self.f = fractions(blend_row, n)
        self.pieces = pieces(self.f, n)
        a = np.arange(m)
        tau = a.astype(np.float64) / np.float64(m)
        tau1 = (a + 1).astype(np.float64) / np.float64(m)
        q, qp0, qp1, qpp, delta, stop = [], [], [], [], [], []
        for kind, k, f, L in self.pieces:
            if kind == 0:
                d = w[k + 1] - w[k]
                sigma = f + tau * L
                q.append(w[k] + sigma[:, None] * d)
                qp0.append(np.broadcast_to(d, (m, J)))
                qp1.append(np.broadcast_to(d, (m, J)))
                qpp.append(np.zeros((m, J)))
                first = f == 0.0
            else:
                dm, dp = w[k] - w[k - 1], w[k + 1] - w[k]
                e = dp - dm
                qp0.append(dm + tau[:, None] * e)
                end = dm + tau1[:, None] * e
                end[m - 1] = dp
                qp1.append(end)
                qpp.append(np.broadcast_to(e / L, (m, J)))
                p0 = w[k] - f * dm
                q.append((p0 + tau[:, None] * (L * dm)) + (tau * tau)[:, None] * (f * e))
                first = False
            delta.append(np.full(m, L / np.float64(m)))
            stop.append(np.concatenate([[first], np.zeros(m - 1, bool)]))
        G = m * len(self.pieces)
        self.G, self.m = G, m
        cat = (lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape))
        self.q = np.concatenate([cat(q, (0, J)), w[n - 1:n]])
        self.qp0, self.qp1, self.qpp = cat(qp0, (0, J)), cat(qp1, (0, J)), cat(qpp, (0, J))
        self.delta = cat(delta, (0,))
        self.stop = np.concatenate([cat(stop, (0,)).astype(bool), [True]])
        self.piece = np.repeat(np.arange(len(self.pieces)), m)


def vcap(qp0, qp1, v):
    """(A,) the velocity cap of A intervals: qp0, qp1 (A, J)"""
    mx = np.fmax(np.abs(qp0), np.abs(qp1))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = v / mx
        sq = r * r
    return np.where(mx > 0.0, sq, np.inf).min(axis=1)


def rows(qp0, qp1, qpp, two, nxt, acc):
    """The rows of A intervals: (cu, cl, d, cap), each (A, 2 J + 1): the upper lines u <= cu + d x, the lower lines
    u >= cl + d x, and the caps on x; a row that is absent holds (+inf, -inf, 0, +inf)."""
    A, J = qp0.shape
    B = np.empty((A, 2 * J))
    B[:, 0::2] = qp0
    B[:, 1::2] = two[:, None] * qpp + qp1
    Aq = np.repeat(qpp, 2, axis=1)
    a2 = np.repeat(np.asarray(acc, np.float64), 2)
    nz = B != 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        c = a2 / np.abs(B)
        d = -(Aq / B)
        capv = a2 / np.abs(Aq)
    cu = np.where(nz, c, np.inf)
    cl = np.where(nz, -c, -np.inf)
    d = np.where(nz, d, 0.0)
    cap = np.where(~nz & (Aq != 0.0), capv, np.inf)
    one = np.ones((A, 1))
    cu = np.concatenate([cu, (nxt / two)[:, None]], 1)
    cl = np.concatenate([cl, 0.0 * one], 1)
    d = np.concatenate([d, (-(1.0 / two))[:, None]], 1)
    cap = np.concatenate([cap, np.inf * one], 1)
    return cu, cl, d, cap


def step_back(qp0, qp1, qpp, delta, xbar_next, v, acc):
    """xbar_i of A intervals (before the stop rule): the closed form of the header."""
    two = 2.0 * delta
    vc = vcap(qp0, qp1, v)
    cu, cl, d, cap = rows(qp0, qp1, qpp, two, np.fmin(xbar_next, vc), acc)
    dd = d[:, :, None] - d[:, None, :]                      # [lower][upper]
    with np.errstate(divide="ignore", invalid="ignore"):
        val = (cu[:, None, :] - cl[:, :, None]) / dd
    val = np.where(dd > 0.0, val, np.inf)
    best = np.fmin(np.fmin(val.min(axis=(1, 2)), cap.min(axis=1)), vc)
    return np.fmax(best, 0.0)


def step_forward(qp0, qp1, qpp, delta, x_i, xbar_next, v, acc):
    """(u_i, x_{i+1}, dt_i, low - u_i) of A intervals"""
    two = 2.0 * delta
    bound = np.fmin(xbar_next, vcap(qp0, qp1, v))
    cu, cl, d, _ = rows(qp0, qp1, qpp, two, bound, acc)
    u = (cu + d * x_i[:, None]).min(axis=1)
    low = (cl + d * x_i[:, None]).max(axis=1)
    xn = np.fmin(np.fmax(x_i + two * u, 0.0), bound)
    with np.errstate(divide="ignore"):
        dt = two / (np.sqrt(x_i) + np.sqrt(xn))
    return u, xn, dt, low - u


def path_status(way, n):
    w = np.asarray(way, np.float64)[:n]
    if not np.isfinite(w).all():
        return NOT_FINITE
    if n >= 2 and (np.diff(w, axis=0) == 0.0).all(axis=1).any():
        return ZERO_SEGMENT
    return OK


def time_law(way, length, blend, v_max, a_max, m, want_grid=True):
    """gg_traj_time: a dict of count, xbar, x, u, t, q_grid, duration, infeasible, status."""
    way = np.asarray(way, np.float64)
    P, W, J = way.shape
    v, acc = np.asarray(v_max, np.float64), np.asarray(a_max, np.float64)
    gmax = grid_max(W, m)
    nn = np.clip(np.asarray(length, np.int64), 1, W)
    status = np.array([path_status(way[p], nn[p]) for p in range(P)], np.int32).reshape(P)
    grids = [Grid(way[p], nn[p], blend[p], m) if status[p] == OK else None for p in range(P)]
    count = np.array([g.G if g else 0 for g in grids], np.int64).reshape(P)
    QP0, QP1, QPP = (np.zeros((P, gmax, J)) for _ in range(3))
    DEL = np.ones((P, gmax))
    STOP = np.zeros((P, gmax + 1), bool)
    for p, g in enumerate(grids):
        if g and g.G:
            QP0[p, :g.G], QP1[p, :g.G], QPP[p, :g.G], DEL[p, :g.G] = g.qp0, g.qp1, g.qpp, g.delta
            STOP[p, :g.G + 1] = g.stop
    xbar, x, t = (np.full((P, gmax + 1), np.nan) for _ in range(3))
    u = np.full((P, gmax), np.nan)
    ok = status == OK
    rows_ok = np.nonzero(ok)[0]
    xbar[rows_ok, count[rows_ok]] = 0.0
    for r in range(int(count.max()) if P else 0):
        act = np.nonzero(ok & (count - 1 - r >= 0))[0]
        i = count[act] - 1 - r
        xb = step_back(QP0[act, i], QP1[act, i], QPP[act, i], DEL[act, i], xbar[act, i + 1], v, acc)
        xbar[act, i] = np.where(STOP[act, i], 0.0, xb)
    x[rows_ok, 0] = 0.0
    t[rows_ok, 0] = 0.0
    worst = np.where(ok, 0.0, np.nan)
    for i in range(int(count.max()) if P else 0):
        act = np.nonzero(ok & (count > i))[0]
        ui, xn, dt, gap = step_forward(QP0[act, i], QP1[act, i], QPP[act, i], DEL[act, i], x[act, i], xbar[act, i + 1],
                                       v, acc)
        u[act, i], x[act, i + 1], t[act, i + 1] = ui, xn, t[act, i] + dt
        worst[act] = np.fmax(worst[act], gap)
    duration = np.where(ok, t[np.arange(P), count], np.nan)
    q_grid = np.full((P, gmax + 1, J), np.nan)
    for p, g in enumerate(grids):
        if g:
            q_grid[p, :g.G + 1] = g.q
    bad = ok & ~np.isfinite(duration)
    status[bad] = NO_DURATION
    gone = status != OK
    xbar[gone], x[gone], t[gone], u[gone], q_grid[gone] = np.nan, np.nan, np.nan, np.nan, np.nan
    duration[gone], worst[gone], count[gone] = np.nan, np.nan, 0
    return dict(count=count.astype(np.int32), xbar=xbar, x=x, u=u, t=t, q_grid=q_grid if want_grid else None,
                duration=duration, infeasible=worst, status=status)


def sample_count(duration, dt):
    """one more than the smallest k with k dt >= duration, the header's way"""
    r = duration / dt
    if r >= float(MAX_SAMPLES):
        return MAX_SAMPLES
    k0 = int(r)
    if float(k0) * dt < duration:
        k0 += 1
    if float(k0) * dt < duration:
        k0 += 1
    if k0 > 0 and float(k0 - 1) * dt >= duration:
        k0 -= 1
    return k0 + 1


def sample(way, length, blend, m, law, dt, K):
    """gg_traj_sample fed `law` (a dict as time_law returns, or the kernel's outputs under the same names): (q, qd,
    qdd (P, K, J), num (P,) int32)."""
    way = np.asarray(way, np.float64)
    P, W, J = way.shape
    nn = np.clip(np.asarray(length, np.int64), 1, W)
    dt = float(dt)
    q, qd, qdd = (np.full((P, K, J), np.nan) for _ in range(3))
    num = np.zeros(P, np.int32)
    for p in range(P):
        dur = float(law["duration"][p])
        if law["status"][p] != OK or not np.isfinite(dur) or dur < 0.0:
            continue
        num[p] = sample_count(dur, dt)
        ks = np.arange(min(int(num[p]), K))
        G = int(law["count"][p])
        if G == 0:
            q[p, ks], qd[p, ks], qdd[p, ks] = way[p, 0], 0.0, 0.0
            continue
        g = Grid(way[p], nn[p], blend[p], m)
        assert g.G == G
        t, x, u = law["t"][p], law["x"][p], law["u"][p]
        tt = np.fmin(ks.astype(np.float64) * dt, dur)
        i = np.clip(np.searchsorted(t[:G + 1], tt, side="right") - 1, 0, G - 1)
        tau = tt - t[i]
        root = np.sqrt(x[i])
        sd = root + u[i] * tau
        ds = np.fmin(np.fmax((root + (0.5 * u[i]) * tau) * tau, 0.0), g.delta[i])[:, None]
        qp = g.qp0[i] + ds * g.qpp[i]
        q[p, ks] = (g.q[i] + ds * g.qp0[i]) + ((0.5 * ds) * ds) * g.qpp[i]
        qd[p, ks] = qp * sd[:, None]
        qdd[p, ks] = g.qpp[i] * (sd * sd)[:, None] + qp * u[i][:, None]
    return q, qd, qdd, num


def inside(g, law_row, points=64):
    """(max_j |dq_j/dt| / v_j, max_j |d2q_j/dt2| / a_j) factors: the joint speeds and accelerations at `points` places
    inside every interval of one path, (G, points, J) each, from x_i, u_i and the interval's own piece."""
    x, u = law_row["x"][:g.G], law_row["u"][:g.G]
    lam = (np.arange(points) + 0.5) / points
    ds = lam[None, :] * g.delta[:, None]                             # (G, points)
    xs = np.fmax(x[:, None] + 2.0 * ds * u[:, None], 0.0)
    qp = g.qp0[:, None, :] + ds[:, :, None] * g.qpp[:, None, :]
    return qp * np.sqrt(xs)[:, :, None], g.qpp[:, None, :] * xs[:, :, None] + qp * u[:, None, None]


def curve(g, points=64):
    """(G, points + 1, J) q at points + 1 places of every interval, ends included"""
    lam = np.arange(points + 1) / points
    ds = (lam[None, :] * g.delta[:, None])[:, :, None]
    return (g.q[:-1, None, :] + ds * g.qp0[:, None, :]) + ((0.5 * ds) * ds) * g.qpp[:, None, :]
