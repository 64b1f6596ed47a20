"""numpy fp64 / int64 restatement of the placement contracts (include/gg_raster.h gg_height_map, gg_place_search), in
the operation order the header gives, of place.placement_transform, and the scene the placement tests share.  Test
infrastructure: slow and plain; nothing here is imported by the package."""
import numpy as np

from field_ref import cell_index

EMPTY = -(1 << 31)
MAX_LEVEL = 1 << 28
MAX_DIM, MAX_FOOT, MAX_YAWS = 4096, 128, 256
INVALID_SUPPORT = (0, 0, -1, -1, -1, -1)


# ------------------------------------------------------------------------------------------------
# gg_height_map
# ------------------------------------------------------------------------------------------------
def takes_part(points, weights, min_weight):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    ok = np.isfinite(p).all(1)
    if weights is not None:
        with np.errstate(invalid="ignore"):
            ok &= float(min_weight) < np.asarray(weights, np.float32).astype(np.float64)
    return ok


def frame_coords(points, frame):
    """(N, 3) fp64 c of fp32 points in one frame (12,): d = p - o, c_a = (d0 e_a0 + d1 e_a1) + d2 e_a2"""
    f = np.asarray(frame, np.float64).reshape(4, 3)
    d = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64) - f[0]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(d[:, 0] * f[a, 0] + d[:, 1] * f[a, 1]) + d[:, 2] * f[a, 2] for a in (1, 2, 3)], 1)


def cells_levels(points, frame, grid):
    """(a, b, z, finite) per point in one frame: the cell by field_ref.cell_index, the level by the same rule clamped
    to +-MAX_LEVEL; where `finite` is false the other three are 0"""
    lo_u, lo_v, h, hz = (float(v) for v in grid)
    c = frame_coords(points, frame)
    with np.errstate(invalid="ignore", over="ignore"):
        du, dv = c[:, 0] - lo_u, c[:, 1] - lo_v
    fin = np.isfinite(du) & np.isfinite(dv) & np.isfinite(c[:, 2])
    du, dv, c2 = (np.where(fin, v, 0.0) for v in (du, dv, c[:, 2]))
    return cell_index(du, h), cell_index(dv, h), np.clip(cell_index(c2, hz), -MAX_LEVEL, MAX_LEVEL), fin


def height_map(points, weights, frames, grid, dims, min_weight=0.0, out=None):
    """(map int32 [F][U][V], dropped int64 [F]); `out` is added to (a copy), EMPTY when None.  The argument order is
    place.height_map's, so that it can stand in for it."""
    U, V = (int(v) for v in dims)
    fr = np.asarray(frames, np.float64).reshape(-1, 12)
    F = len(fr)
    m = np.full((F, U, V), EMPTY, np.int32) if out is None else np.array(out, np.int32, copy=True)
    p = np.asarray(points, np.float32).reshape(-1, 3)
    part = takes_part(p, weights, min_weight)
    dropped = np.zeros(F, np.int64)
    for f in range(F):
        a, b, z, fin = cells_levels(p, fr[f], grid)
        land = part & fin & (a >= 0) & (a < U) & (b >= 0) & (b < V)
        dropped[f] = len(p) - int(land.sum())
        np.maximum.at(m[f], (a[land], b[land]), z[land].astype(np.int32))
    return m, dropped


# ------------------------------------------------------------------------------------------------
# gg_place_search
# ------------------------------------------------------------------------------------------------
def _by_anchor(top, under_k, I, J, tols):
    """few anchors under a large object: a loop over the anchors, the object's cells at once"""
    A, B = under_k.shape
    full = under_k != EMPTY
    aa, bb = np.nonzero(full)
    out = []
    for i in range(I):
        for j in range(J):
            t = top[i:i + A, j:j + B][full]
            if (t == EMPTY).any():
                out.append(None)
                continue
            s = t + under_k[full]
            row = []
            for tol in tols:
                c = s >= s.max() - int(tol)
                a, b = aa[c], bb[c]
                row.append((s.max(), c.sum(), a.sum(), b.sum(), a.min(), a.max(), b.min(), b.max()))
            out.append(row)
    return out


def search_many(top, under, tols):
    """[search(top, under, tol) for tol in tols], the first sweep shared: (rest int32 [K][I][J], contact int32
    [K][I][J], support int32 [K][I][J][6]) each, in int64.  Many anchors: a loop over the object's cells, every anchor
    at once; few anchors: a loop over the anchors, every cell at once."""
    top, under = np.asarray(top, np.int64), np.asarray(under, np.int64)
    (U, V), (K, A, B) = top.shape, under.shape
    I, J = U - A + 1, V - B + 1
    res = [(np.full((K, I, J), EMPTY, np.int64), np.zeros((K, I, J), np.int64),
            np.tile(np.array(INVALID_SUPPORT, np.int64), (K, I, J, 1))) for _ in tols]
    for k in range(K):
        cells = np.argwhere(under[k] != EMPTY)
        if len(cells) == 0:
            continue
        if I * J <= 64 and len(cells) > I * J:
            for n, row in enumerate(_by_anchor(top, under[k], I, J, tols)):
                for (rest, contact, support), v in zip(res, row or ()):
                    rest[k, n // J, n % J], contact[k, n // J, n % J], support[k, n // J, n % J] = v[0], v[1], v[2:]
            continue
        best = np.full((I, J), np.iinfo(np.int64).min)
        bad = np.zeros((I, J), bool)
        for a, b in cells:
            t = top[a:a + I, b:b + J]
            bad |= t == EMPTY
            np.maximum(best, t + under[k, a, b], out=best)
        ok = ~bad
        for (rest, contact, support), tol in zip(res, tols):
            thr = best - int(tol)
            cnt, sa, sb = (np.zeros((I, J), np.int64) for _ in range(3))
            amin, bmin = np.full((I, J), 1 << 20), np.full((I, J), 1 << 20)
            amax, bmax = np.full((I, J), -1), np.full((I, J), -1)
            for a, b in cells:
                c = (top[a:a + I, b:b + J] + under[k, a, b] >= thr) & ok
                cnt += c
                sa += c * a
                sb += c * b
                np.minimum(amin, np.where(c, a, 1 << 20), out=amin)
                np.maximum(amax, np.where(c, a, -1), out=amax)
                np.minimum(bmin, np.where(c, b, 1 << 20), out=bmin)
                np.maximum(bmax, np.where(c, b, -1), out=bmax)
            rest[k][ok] = best[ok]
            contact[k][ok] = cnt[ok]
            support[k][ok] = np.stack([sa, sb, amin, amax, bmin, bmax], -1)[ok]
    return [tuple(x.astype(np.int32) for x in r) for r in res]


def search(top, under, tol):
    return search_many(top, under, (tol,))[0]


def search_brute(top, under, tol):
    """the same by a triple loop over yaw and anchor, for one small case"""
    top, under = np.asarray(top, np.int64), np.asarray(under, np.int64)
    (U, V), (K, A, B) = top.shape, under.shape
    I, J = U - A + 1, V - B + 1
    rest = np.full((K, I, J), EMPTY, np.int64)
    contact = np.zeros((K, I, J), np.int64)
    support = np.tile(np.array(INVALID_SUPPORT, np.int64), (K, I, J, 1))
    for k in range(K):
        for i in range(I):
            for j in range(J):
                s = [(int(top[i + a, j + b]), int(under[k, a, b]), a, b) for a in range(A) for b in range(B)
                     if under[k, a, b] != EMPTY]
                if not s or any(t == EMPTY for t, _, _, _ in s):
                    continue
                r = max(t + u for t, u, _, _ in s)
                hit = [(a, b) for t, u, a, b in s if t + u >= r - tol]
                aa, bb = [a for a, _ in hit], [b for _, b in hit]
                rest[k, i, j], contact[k, i, j] = r, len(hit)
                support[k, i, j] = sum(aa), sum(bb), min(aa), max(aa), min(bb), max(bb)
    return rest.astype(np.int32), contact.astype(np.int32), support.astype(np.int32)


def searcher(top, under, tol):
    """search as place.search returns it (a stand-in for it in place.place_points)"""
    from gaussiangrasper_amd.place import PlaceSearch
    return PlaceSearch(*search(top, under, tol))


# ------------------------------------------------------------------------------------------------
# the transform
# ------------------------------------------------------------------------------------------------
def placement_transform(o, e0, e1, n, grid, obj_frame, anchor, rest):
    """(3, 4): x -> o + (lo_u + i h + c0) e0 + (lo_v + j h + c1) e1 + (c2 + (rest + 2) hz) n, c the coordinates of x in
    obj_frame (o_k, e0_k, e1_k, n)"""
    lo_u, lo_v, h, hz = (float(v) for v in grid)
    f = np.asarray(obj_frame, np.float64).reshape(4, 3)
    R = np.outer(e0, f[1]) + np.outer(e1, f[2]) + np.outer(n, f[3])
    t = o + (lo_u + anchor[0] * h) * e0 + (lo_v + anchor[1] * h) * e1 + (int(rest) + 2) * hz * n - R @ f[0]
    return np.concatenate([R, t[:, None]], 1)


# ------------------------------------------------------------------------------------------------
# the scene the tests share
# ------------------------------------------------------------------------------------------------
CELL, LEVEL = 2.0 ** -7, 2.0 ** -10
TABLE, OBSTACLE, OBJECT = 0, 1, 2


def place_scene():
    """A table, an obstacle and an object over plane_ref's tilted plane, default_rng(5), rounded to fp32:
    20 000 table points over [-0.3, 0.3]^2 with 0.5 mm of normal noise, 1500 points in a 10 x 8 x 6 cm block standing
    at (0.12, 0.05) of the plane's (t1, t2) coordinates, and an L-shaped object of 900 points (12 x 4 cm and 4 x 8 cm
    arms, 5 cm tall) lying at (-0.15, -0.1), turned by 0.4 rad.  Returns (points (22400, 3) float32, kind (22400,),
    (normal, offset))."""
    import plane_ref
    rng = np.random.default_rng(5)
    t1, t2, n = plane_ref.table_frame()
    o = -plane_ref.TRUE_OFFSET * n

    def at(u, v, z):
        return o + np.asarray(u)[:, None] * t1 + np.asarray(v)[:, None] * t2 + np.asarray(z)[:, None] * n
    table = at(rng.uniform(-0.3, 0.3, 20000), rng.uniform(-0.3, 0.3, 20000), rng.normal(0.0, 0.0005, 20000))
    block = at(0.12 + rng.uniform(-0.05, 0.05, 1500), 0.05 + rng.uniform(-0.04, 0.04, 1500),
               rng.uniform(0.0, 0.06, 1500))
    arm = rng.random(900) < 0.6
    x = np.where(arm, rng.uniform(-0.06, 0.06, 900), rng.uniform(-0.06, -0.02, 900))
    y = np.where(arm, rng.uniform(-0.02, 0.02, 900), rng.uniform(0.02, 0.10, 900))
    c, s = np.cos(0.4), np.sin(0.4)
    obj = at(-0.15 + c * x - s * y, -0.1 + s * x + c * y, rng.uniform(0.002, 0.05, 900))
    pts = np.concatenate([table, block, obj]).astype(np.float32)
    kind = np.repeat([TABLE, OBSTACLE, OBJECT], [20000, 1500, 900])
    return pts, kind, (plane_ref.TRUE_NORMAL.copy(), plane_ref.TRUE_OFFSET)


_PLAN = {}


def reference_plan(**kw):
    """place.place_points on place_scene() through the restatements (computed once per set of keywords and shared;
    callers do not change it)"""
    key = tuple(sorted(kw.items()))
    if key not in _PLAN:
        from gaussiangrasper_amd import place
        pts, kind, plane = place_scene()
        w = np.ones(len(pts), np.float32)
        args = dict(cell=CELL, level=LEVEL, yaws=5, region=0.28, maps=height_map, searcher=searcher)
        args.update(kw)
        _PLAN[key] = place.place_points(pts, np.where(kind == OBJECT, 0, w).astype(np.float32),
                                        np.where(kind == OBJECT, w, 0).astype(np.float32), plane, **args)
    return _PLAN[key]


def clearance(plan, pts, kind, placement):
    """Of one placement of a plan: (gap in levels, skipped share).  The object's points are moved by the transform in
    fp64; a point must clear (top[cell] + 1) hz of the scene cell it lands in (every scene point of the cell lies below
    that), and gap is the smallest height above it over the points, in levels.  Points within 1e-9 of a cell edge
    (or outside the grid: there are none when the footprint holds the object) are left out and counted."""
    T = plan.placements.transform[placement]
    x = pts[kind == OBJECT].astype(np.float64) @ T[:, :3].T + T[:, 3]
    c = plan.frame.coords(x)
    lo_u, lo_v, h, hz = plan.grid
    fu, fv = (c[:, 0] - lo_u) / h, (c[:, 1] - lo_v) / h
    edge = (np.abs(fu - np.round(fu)) * h < 1e-9) | (np.abs(fv - np.round(fv)) * h < 1e-9)
    a, b = np.floor(fu).astype(np.int64), np.floor(fv).astype(np.int64)
    inside = (a >= 0) & (a < plan.dims[0]) & (b >= 0) & (b < plan.dims[1])
    use = ~edge & inside
    need = (plan.top[a[use], b[use]].astype(np.float64) + 1.0) * hz
    gaps = c[use, 2] - need
    return float(gaps.min() / hz), float(1.0 - use.mean())
