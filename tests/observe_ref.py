"""numpy restatement of the known-free-space contracts (include/gg_raster.h gg_depth_min_pyramid, gg_field_observe,
gg_field_distance_known), operation for operation in the order the header gives, and the fixture the observe tests
share: a ground plane and a box, ray-cast exactly into five small pinhole frames.  Test infrastructure: slow and plain."""
import numpy as np

import field_ref

PAD = 2.0 ** -20
SAT = 65535


# ------------------------------------------------------------------------------------------------
# the entries
# ------------------------------------------------------------------------------------------------
def level_shapes(H, W):
    out, l = [], 0
    while True:
        h, w = -(-H // (1 << l)), -(-W // (1 << l))
        out.append((h, w))
        if h == 1 and w == 1:
            return out
        l += 1


def level_offsets(H, W):
    sizes = [h * w for h, w in level_shapes(H, W)]
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), int(sum(sizes))


def pyramid(depth):
    """pyr float32 [V][S] of depth [V][H][W]."""
    d = np.asarray(depth, np.float32)
    V, H, W = d.shape
    with np.errstate(invalid="ignore"):
        lev = np.where(d > 0, d, np.float32(0)).astype(np.float32)
    parts = [lev.reshape(V, -1)]
    for h, w in level_shapes(H, W)[1:]:
        pad = np.full((V, 2 * h, 2 * w), np.inf, np.float32)
        pad[:, :lev.shape[1], :lev.shape[2]] = lev
        lev = pad.reshape(V, h, 2, w, 2).min(axis=(2, 4))
        parts.append(lev.reshape(V, -1))
    return np.ascontiguousarray(np.concatenate(parts, 1))


def _axis(a, radius, zn, zf, f, cc, n):
    with np.errstate(all="ignore"):
        xl, xh = a - radius, a + radius
        ul = f * (xl / np.where(xl < 0, zn, zf)) + cc
        uh = f * (xh / np.where(xh > 0, zn, zf)) + cc
        A, B = np.floor(ul - PAD), np.floor(uh + PAD)
        ok = (A >= 0) & (B <= n - 1)
    return ok, np.where(ok, A, 0).astype(np.int64), np.where(ok, B, 0).astype(np.int64)


def choose_level(Au, Bu, Av, Bv, levels):
    """the smallest l with (B >> l) - (A >> l) <= 1 on both axes"""
    l = np.zeros(np.shape(Au), np.int64)
    for _ in range(levels):
        wide = (((Bu >> l) - (Au >> l)) > 1) | (((Bv >> l) - (Av >> l)) > 1)
        l = np.where(wide, l + 1, l)
    assert (l < levels).all()
    return l


def observe_views(dims, grid, pyr, H, W, intrinsics, w2c, radius, margin, near, levels_out=None):
    """(looked, seen) bool [V][X][Y][Z]: what every view alone says of every cell.  levels_out: a list that receives,
    per view, the level chosen for every cell (-1 where the cell was not looked at)."""
    X, Y, Z = (int(v) for v in dims)
    lo, h = np.asarray(grid[:3], np.float64), float(grid[3])
    K, E = np.asarray(intrinsics, np.float64).reshape(-1, 4), np.asarray(w2c, np.float64).reshape(-1, 3, 4)
    V = len(K)
    off, S = level_offsets(H, W)
    shapes = level_shapes(H, W)
    pyr = np.asarray(pyr, np.float32).reshape(V, S)
    idx = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    c = [lo[a] + (idx[a].astype(np.float64) + 0.5) * h for a in range(3)]
    looked, seen = np.zeros((V, X, Y, Z), bool), np.zeros((V, X, Y, Z), bool)
    wl = np.array([s[1] for s in shapes], np.int64)
    for v in range(V):
        with np.errstate(all="ignore"):
            p = [((E[v, r, 0] * c[0] + E[v, r, 1] * c[1]) + E[v, r, 2] * c[2]) + E[v, r, 3] for r in range(3)]
            zn, zf = p[2] - radius, p[2] + radius
            part = zn >= near
        oku, Au, Bu = _axis(p[0], radius, zn, zf, K[v, 0], K[v, 2], W)
        okv, Av, Bv = _axis(p[1], radius, zn, zf, K[v, 1], K[v, 3], H)
        lk = part & oku & okv
        Au, Bu, Av, Bv = (np.where(lk, t, 0) for t in (Au, Bu, Av, Bv))
        l = choose_level(Au, Bu, Av, Bv, len(shapes))
        if levels_out is not None:
            levels_out.append(np.where(lk, l, -1))
        m = np.full((X, Y, Z), np.inf, np.float32)
        for yy in (Av >> l, Bv >> l):
            for xx in (Au >> l, Bu >> l):
                m = np.minimum(m, pyr[v][off[l] + yy * wl[l] + xx])
        with np.errstate(invalid="ignore"):
            free = m.astype(np.float64) > zf + margin
        looked[v], seen[v] = lk, lk & free
    return looked, seen


def accumulate(old, per_view):
    """min(65535, old + count) as uint16"""
    return np.minimum(SAT, np.asarray(old, np.int64) + per_view.sum(0)).astype(np.uint16)


def observe(dims, grid, pyr, H, W, intrinsics, w2c, radius, margin, near, seen=None, looked=None):
    """(seen, looked) uint16 [X][Y][Z] after one gg_field_observe call; None starts from zeros."""
    shape = tuple(int(v) for v in dims)
    lk, sn = observe_views(dims, grid, pyr, H, W, intrinsics, w2c, radius, margin, near)
    z = np.zeros(shape, np.uint16)
    return accumulate(z if seen is None else seen, sn), accumulate(z if looked is None else looked, lk)


def distance_known(mass, threshold, seen, min_views):
    """gg_field_distance_known: field_ref's transform from the seeds mass >= threshold or seen < min_views"""
    seed = (np.asarray(mass, np.int64) >= int(threshold)) | (np.asarray(seen, np.int64) < int(min_views))
    return field_ref.distance(seed.astype(np.int64), 1)


def cell_ball(h):
    return 0.5 * np.sqrt(3.0) * h * (1.0 + 2.0 ** -40)


# ------------------------------------------------------------------------------------------------
# the fixture
# ------------------------------------------------------------------------------------------------
BOX_LO, BOX_HI = np.array([-0.1, -0.1, 0.0]), np.array([0.1, 0.1, 0.2])
FH, FW = 37, 53
FK = (40.0, 41.0, 26.3, 18.1)
EYES = ((0.9, 0.2, 0.8), (-0.7, 0.6, 0.9), (0.1, -1.0, 0.5), (0.2, 0.1, 1.6), (0.3, 0.3, 0.25))
TARGET = (0.0, 0.0, 0.1)
LO, CELL, DIMS = (-0.4, -0.4, -0.1), 2.0 ** -5, (13, 9, 21)
GRID = np.array([*LO, CELL])
MARGIN, NEAR = 0.004, 0.05
RADIUS = cell_ball(CELL)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """OpenCV world-to-camera (3, 4): z forward from eye to target, x right, y down"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, (-R @ eye)[:, None]], 1)


def ray_depth(E, K, H, W):
    """exact z-depth of the plane z = 0 and the box through every pixel's centre ray; +inf where it hits nothing"""
    R, t = E[:, :3], E[:, 3]
    eye = -R.T @ t
    v, u = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    dc = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1)      # camera ray with z = 1
    dw = dc @ R                                                                     # R^T dc, per pixel
    best = np.full((H, W), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = -eye[2] / dw[..., 2]
        best = np.where((s > 0) & np.isfinite(s), s, best)
        t0, t1 = (BOX_LO - eye) / dw, (BOX_HI - eye) / dw
        tn, tf = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
        hit = (tn <= tf) & (tf > 0)
        best = np.where(hit, np.minimum(best, np.maximum(tn, 0.0)), best)
    return best.astype(np.float32)


def fixture():
    """dict: depth [5][37][53] (holes punched), raw = the same, K [5][4], E [5][3][4]"""
    K = np.tile(np.array(FK, np.float64), (len(EYES), 1))
    E = np.stack([look_at(e, TARGET) for e in EYES])
    depth = np.stack([ray_depth(E[v], K[v], FH, FW) for v in range(len(EYES))])
    depth[1, 12:16, 20:30] = 0.0                     # a 4 x 10 block of missing readings
    depth[3, 20, 25] = np.nan
    return {"depth": depth, "K": K, "E": E}


def solid(points):
    """inside the box or below the plane (closed)"""
    p = np.asarray(points, np.float64)
    return (p[..., 2] <= 0.0) | ((p >= BOX_LO) & (p <= BOX_HI)).all(-1)


def centres(dims=DIMS, grid=GRID):
    idx = np.stack(np.meshgrid(*[np.arange(int(d)) for d in dims], indexing="ij"), -1)
    return grid[:3] + (idx.astype(np.float64) + 0.5) * grid[3]
