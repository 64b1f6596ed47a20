"""numpy fp64 / int64 restatement of the distance-field contracts (include/gg_raster.h gg_field_splat,
gg_field_distance, gg_field_paths), in the operation order the header gives.  Test infrastructure: slow and plain."""
import numpy as np

FAR = 1 << 30
MAX_REACH = 64
INT32_MIN = -(1 << 31)
_CLAMP = float(1 << 30)


def cell_index(d, h):
    """Per element of d = p - lo (fp64, finite): the c with c h <= d < (c + 1) h, from floor(d / h) corrected by one;
    clamped to +-2^30 like the kernel's (such a cell is outside every volume)."""
    d = np.asarray(d, np.float64)
    c = np.clip(np.floor(d / h), -_CLAMP, _CLAMP)
    c = np.where(c * h > d, c - 1.0, np.where((c + 1.0) * h <= d, c + 1.0, c))
    return c.astype(np.int64)


def centre(c, lo, h):
    return lo + (np.asarray(c, np.float64) + 0.5) * h


def row_takes_part(means, rot, scales, weights, min_weight):
    m, R, s, w = (np.asarray(a, np.float32) for a in (means, rot, scales, weights))
    fin = np.isfinite(m).all(1) & np.isfinite(R.reshape(len(m), 9)).all(1) & np.isfinite(s).all(1) & np.isfinite(w)
    wd = w.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return fin & (s > 0).all(1) & (min_weight < wd) & (wd < 32768.0)


def row_reach(scales, extent, h, max_reach):
    """(reach, cut) per row: n the smallest integer >= 0 with n h >= k max_j s_j, by the comparison itself."""
    rad = float(extent) * np.asarray(scales, np.float32).max(1).astype(np.float64)
    cand = np.arange(MAX_REACH + 2, dtype=np.float64)                 # 0..65
    ge = cand[None, :] * h >= rad[:, None]
    n = np.where(ge.any(1), ge.argmax(1), MAX_REACH + 1)
    return np.minimum(max_reach, n + 1), n + 1 > max_reach


def splat(dims, grid, means, rot, scales, weights, extent=1.0, max_reach=8, min_weight=0.0, sign=1, mass=None):
    """(mass, skipped, truncated); `mass` int64 [X][Y][Z] is added to (a copy), zeros when None."""
    X, Y, Z = (int(v) for v in dims)
    lo, h = np.asarray(grid[:3], np.float64), float(grid[3])
    k = float(extent)
    out = np.zeros((X, Y, Z), np.int64) if mass is None else np.array(mass, np.int64, copy=True)
    m32 = np.asarray(means, np.float32).reshape(-1, 3)
    n_rows = len(m32)
    if n_rows == 0:
        return out, 0, 0
    R32 = np.asarray(rot, np.float32).reshape(n_rows, 3, 3)
    s32 = np.asarray(scales, np.float32).reshape(n_rows, 3)
    w32 = np.asarray(weights, np.float32).reshape(n_rows)
    ok = row_takes_part(m32, R32, s32, w32, min_weight)
    skipped = int((~ok).sum())
    idx = np.nonzero(ok)[0]
    m, R = m32[idx].astype(np.float64), R32[idx].astype(np.float64)
    s = s32[idx].astype(np.float64)
    q = np.trunc(w32[idx].astype(np.float64) * 65536.0).astype(np.int64)
    reach, cut = row_reach(s32[idx], k, h, max_reach)
    truncated = int(cut.sum())
    A = s * s
    rhs = (k * k) * ((A[:, 0] * A[:, 1]) * A[:, 2])
    c0 = np.stack([cell_index(m[:, a] - lo[a], h) for a in range(3)], 1)
    dim = np.array([X, Y, Z])
    acc = np.zeros(X * Y * Z, np.float64)                # sums of q stay far below 2^53: exact
    for r in np.unique(reach):
        rows = np.nonzero(reach == r)[0]
        o = np.arange(-r, r + 1)
        off = np.stack(np.meshgrid(o, o, o, indexing="ij"), -1).reshape(-1, 3)
        step = max(1, (1 << 20) // len(off))
        for b in range(0, len(rows), step):
            rr = rows[b:b + step]
            cell = c0[rr][:, None, :] + off[None, :, :]                       # (n, cells, 3)
            inside = ((cell >= 0) & (cell < dim)).all(-1)
            x = lo + (cell.astype(np.float64) + 0.5) * h
            d = x - m[rr][:, None, :]
            Rr = R[rr]
            u = [(Rr[:, None, 0, j] * d[..., 0] + Rr[:, None, 1, j] * d[..., 1]) + Rr[:, None, 2, j] * d[..., 2]
                 for j in range(3)]
            Ar = A[rr]
            with np.errstate(invalid="ignore", over="ignore"):
                lhs = (((u[0] * u[0]) * (Ar[:, 1] * Ar[:, 2])[:, None] + (u[1] * u[1]) * (Ar[:, 0] * Ar[:, 2])[:, None])
                       + (u[2] * u[2]) * (Ar[:, 0] * Ar[:, 1])[:, None])
                hit = lhs <= rhs[rr][:, None]
            hit |= (off == 0).all(1)[None, :]                                 # (a): the mean's own cell
            hit &= inside
            flat = (cell[..., 0] * Y + cell[..., 1]) * Z + cell[..., 2]
            votes = np.broadcast_to(q[rr][:, None], hit.shape)
            acc += np.bincount(flat[hit], weights=votes[hit].astype(np.float64), minlength=X * Y * Z)
    out += int(sign) * acc.astype(np.int64).reshape(X, Y, Z)
    return out, skipped, truncated


def min_plus(f, axis):
    """f'[c] = min_c' f[c'] + (c - c')^2 along `axis`, int64, every c' tried."""
    f = np.moveaxis(np.asarray(f, np.int64), axis, 0)
    L = f.shape[0]
    out = f.copy()
    for d in range(1, L):
        if d * d >= out.max():                    # a candidate d away is at least d^2: nothing can fall any more
            break
        out[d:] = np.minimum(out[d:], f[:-d] + d * d)
        out[:-d] = np.minimum(out[:-d], f[d:] + d * d)
    return np.moveaxis(out, 0, axis)


def distance(mass, threshold):
    """dist2 int32 [X][Y][Z]: the three passes z, y, x and the clamp."""
    f = np.where(np.asarray(mass, np.int64) >= int(threshold), 0, FAR).astype(np.int64)
    for axis in (2, 1, 0):
        f = min_plus(f, axis)
        assert f.max() < (1 << 31)
    return np.minimum(f, FAR).astype(np.int32)


def paths(dims, grid, dist2, poses, spheres, need2, outside):
    """(slack int32 [P][W], first_hit int32 [P])."""
    X, Y, Z = (int(v) for v in dims)
    lo, h = np.asarray(grid[:3], np.float64), float(grid[3])
    T32 = np.asarray(poses, np.float32)
    P, W = T32.shape[:2]
    sp = np.asarray(spheres, np.float32).reshape(-1, 3).astype(np.float64)
    need = np.asarray(need2, np.int64).reshape(-1)
    fin = np.isfinite(T32).all(-1)
    T = np.where(fin[..., None], T32, 0).astype(np.float64)
    slack = np.full((P, W), FAR, np.int64)
    dist2 = np.asarray(dist2).reshape(X, Y, Z)
    dim = (X, Y, Z)
    if len(sp):
        inside = np.ones((P, W, len(sp)), bool)
        cells = []
        for a in range(3):
            c = ((T[..., 3 * a, None] * sp[:, 0] + T[..., 3 * a + 1, None] * sp[:, 1])
                 + T[..., 3 * a + 2, None] * sp[:, 2]) + T[..., 9 + a, None]
            ok = np.isfinite(c)
            ca = cell_index(np.where(ok, c, 0.0) - lo[a], h)
            inside &= ok & (ca >= 0) & (ca < dim[a])
            cells.append(np.clip(ca, 0, dim[a] - 1))
        d = np.where(inside, dist2[cells[0], cells[1], cells[2]].astype(np.int64), int(outside))
        slack = (d - need[None, None, :]).min(-1)
    slack = np.where(fin, slack, INT32_MIN)
    hit = slack < 0
    first = np.where(hit.any(1), hit.argmax(1), W) if W else np.zeros(P, np.int64)
    return slack.astype(np.int32), first.astype(np.int32)
