"""fp64 numpy restatement of the support plane: gg_plane_consensus and gg_plane_classify in the contract's operation
order (include/gg_raster.h), support.plane_from_moments, support.fit_plane and grasp.plane_clear, and the two scenes
the tests share.  Test infrastructure: nothing here is imported by the package."""
import math

import numpy as np

TRUE_NORMAL = np.array([0.05, -0.03, 1.0]) / math.sqrt(0.05 ** 2 + 0.03 ** 2 + 1.0)
TRUE_OFFSET = -0.2


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
def table_frame():
    """(t1, t2, n): an orthonormal frame whose third axis is the table's normal."""
    n = TRUE_NORMAL
    t1 = np.cross([0.0, 1.0, 0.0], n)
    t1 /= np.linalg.norm(t1)
    return t1, np.cross(n, t1), n


def table_scene():
    """The table scene, default_rng(7), rounded to fp32: 3000 table points on the plane with normal ~ (0.05, -0.03, 1)
    and offset -0.2 over [-0.4, 0.4]^2 with 1 mm normal noise, 1200 points on the faces of an 8 x 6 x 5 cm box standing
    on it, 800 on a vertical wall at x = 0.4, 500 uniform clutter points.  Returns (points (5500, 3) float32, outward
    normals (5500, 3) float64, kind (5500,): 0 table, 1 box, 2 wall, 3 clutter)."""
    rng = np.random.default_rng(7)
    t1, t2, n = table_frame()

    def on_plane(xy):
        z = (-TRUE_OFFSET - n[0] * xy[:, 0] - n[1] * xy[:, 1]) / n[2]
        return np.column_stack([xy, z])
    table = on_plane(rng.uniform(-0.4, 0.4, (3000, 2))) + rng.normal(0.0, 0.001, (3000, 1)) * n
    half = np.array([0.04, 0.03, 0.025])
    face = rng.integers(0, 6, 1200)
    u = rng.uniform(-1.0, 1.0, (1200, 3)) * half
    ax, sign = face // 2, (face % 2) * 2.0 - 1.0
    u[np.arange(1200), ax] = sign * half[ax]
    foot = on_plane(np.zeros((1, 2)))[0]
    box = foot + u[:, :1] * t1 + u[:, 1:2] * t2 + (u[:, 2:] + half[2]) * n
    nb = np.zeros((1200, 3))
    nb[np.arange(1200), ax] = sign
    box_n = nb[:, :1] * t1 + nb[:, 1:2] * t2 + nb[:, 2:] * n
    wall = np.column_stack([np.full(800, 0.4), rng.uniform(-0.4, 0.4, 800), rng.uniform(0.15, 0.6, 800)])
    clutter = np.column_stack([rng.uniform(-0.4, 0.4, (500, 2)), rng.uniform(0.05, 0.6, 500)])
    pts = np.concatenate([table, box, wall, clutter]).astype(np.float32)
    nrm = np.concatenate([np.tile(n, (3000, 1)), box_n, np.tile([-1.0, 0.0, 0.0], (800, 1)),
                          np.tile([0.0, 0.0, 1.0], (500, 1))])
    kind = np.repeat([0, 1, 2, 3], [3000, 1200, 800, 500])
    return pts, nrm, kind


def lattice_scene(n, seed):
    """(points (n, 3) float32, weights (n,) float32): coordinates multiples of 2^-7 in [-1, 1], so that every product
    of the contract is exact in fp64; about half the points lie on the plane z = 0 and a quarter exactly 2^-5 off it;
    weights in {0.25, 0.5, 1}."""
    rng = np.random.default_rng(seed)
    p = rng.integers(-128, 129, (n, 3)).astype(np.float64)
    r = rng.random(n)
    p[r < 0.5, 2] = 0.0
    p[(r >= 0.5) & (r < 0.75), 2] = rng.choice([-4.0, 4.0], int(((r >= 0.5) & (r < 0.75)).sum()))
    w = rng.choice([0.25, 0.5, 1.0], n)
    return (p / 128.0).astype(np.float32), w.astype(np.float32)


def lattice_hypotheses(points, h, seed):
    """(h, 3) int32 triples over the points: uniform, repeats and all; every fourth one, when the scene has three
    such points, among the points with z = 0, so that many hypotheses are that plane, with a quarter of the scene
    exactly 2^-5 from it."""
    rng = np.random.default_rng(seed)
    n = len(points)
    hyp = rng.integers(0, max(n, 1), (h, 3)).astype(np.int32)
    flat = np.nonzero(np.asarray(points)[:, 2] == 0.0)[0] if n else np.zeros(0, np.int64)
    if len(flat) >= 3:
        hyp[3::4] = flat[rng.integers(0, len(flat), (len(hyp[3::4]), 3))]
    return hyp


# ------------------------------------------------------------------------------------------------
# gg_plane_consensus
# ------------------------------------------------------------------------------------------------
def takes_part(points, weights, min_weight):
    p = np.asarray(points, np.float32)
    fin = np.isfinite(p).all(axis=1) if len(p) else np.zeros(0, bool)
    if weights is None:
        return fin
    return fin & (np.asarray(weights, np.float32).astype(np.float64) > float(min_weight))


def consensus(points, weights, min_weight, hyp, dist, min_sin2, up=None, cos2_tilt=0.0):
    """dict(count int32 (H,), valid uint8 (H,), best int32 (2,), gap: the smallest |s s - (dist dist) nn| / nn over
    the (valid hypothesis, point taking part) pairs that are not exactly on the limit, on_limit: how many are)."""
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    hyp = np.asarray(hyp, np.int32).reshape(-1, 3)
    N, H = len(p32), len(hyp)
    part = takes_part(p32, weights, min_weight)
    p = p32.astype(np.float64)
    count, valid = np.zeros(H, np.int32), np.zeros(H, np.uint8)
    gap, on_limit = math.inf, 0
    dd = float(dist) * float(dist)
    u = None if up is None else np.asarray(up, np.float64)
    with np.errstate(all="ignore"):
        for h in range(H):
            a, b, c = (int(v) for v in hyp[h])
            if min(a, b, c) < 0 or max(a, b, c) >= N or a == b or a == c or b == c:
                continue
            if not (part[a] and part[b] and part[c]):
                continue
            e1, e2 = p[b] - p[a], p[c] - p[a]
            n0 = e1[1] * e2[2] - e1[2] * e2[1]
            n1 = e1[2] * e2[0] - e1[0] * e2[2]
            n2 = e1[0] * e2[1] - e1[1] * e2[0]
            nn = (n0 * n0 + n1 * n1) + n2 * n2
            ee1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]
            ee2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]
            if not (np.isfinite(nn) and nn > float(min_sin2) * (ee1 * ee2)):
                continue
            if u is not None:
                g = (n0 * u[0] + n1 * u[1]) + n2 * u[2]
                uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
                if not g * g >= float(cos2_tilt) * (nn * uu):
                    continue
            valid[h] = 1
            d = p[part] - p[a]
            s = (n0 * d[:, 0] + n1 * d[:, 1]) + n2 * d[:, 2]
            ss, lim = s * s, dd * nn
            count[h] = int((ss <= lim).sum())
            on_limit += int((ss == lim).sum())
            off = np.abs(ss - lim)[ss != lim]
            if len(off):
                gap = min(gap, float(off.min()) / nn)
    best = np.array([-1, 0], np.int32)
    if valid.any():
        c = np.where(valid == 1, count, -1)
        best[:] = (int(np.argmax(c)), int(c.max()))                # argmax: the first, i.e. smallest, index
    return dict(count=count, valid=valid, best=best, gap=gap, on_limit=on_limit)


# ------------------------------------------------------------------------------------------------
# gg_plane_classify
# ------------------------------------------------------------------------------------------------
def _seq(x):
    """sum in index order (np.sum adds pairwise)"""
    t = 0.0
    for v in np.asarray(x, np.float64).ravel():
        t += v
    return t


def classify(points, weights, min_weight, plane, origin, dist, order="pairwise"):
    """dict(height float32 (N,), side uint8 (N,), sums float64 (16,), abs_sums: the sums of the terms' absolute
    values, terms: how many terms the longest sum has, h: fp64 heights).  order: "pairwise" (np.sum) or "sequential"
    (index order): two of the orders a fixed-order sum may take."""
    add = np.sum if order == "pairwise" else _seq
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    N = len(p32)
    part = takes_part(p32, weights, min_weight)
    fin = np.isfinite(p32).all(axis=1) if N else np.zeros(0, bool)
    p = p32.astype(np.float64)
    n, d, o = np.asarray(plane[:3], np.float64), float(plane[3]), np.asarray(origin, np.float64)
    w = np.ones(N) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        h = ((n[0] * p[:, 0] + n[1] * p[:, 1]) + n[2] * p[:, 2]) + d
    height = np.where(fin, h, np.nan).astype(np.float32)
    side = np.full(N, 3, np.uint8)
    dist = float(dist)
    side[part & (h < -dist)] = 0
    side[part & (h >= -dist) & (h <= dist)] = 1
    side[part & (h > dist)] = 2
    on, ab, be = side == 1, side == 2, side == 0
    q = p[on] - o
    terms = [np.ones(int(on.sum())), np.ones(int(ab.sum())), np.ones(int(be.sum())), h[on] * h[on],
             q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2], q[:, 1] * q[:, 1],
             q[:, 1] * q[:, 2], q[:, 2] * q[:, 2], w[on], w[ab], w[be]]
    sums = np.array([float(add(t)) if len(t) else 0.0 for t in terms])
    abs_sums = np.array([float(np.abs(t).sum()) if len(t) else 0.0 for t in terms])
    return dict(height=height, side=side, sums=sums, abs_sums=abs_sums, terms=max(len(t) for t in terms), h=h)


# ------------------------------------------------------------------------------------------------
# host linear algebra and the whole fit
# ------------------------------------------------------------------------------------------------
def plane_from_triple(a, b, c):
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    n = np.cross(b - a, c - a)
    n = n / math.sqrt(float(n @ n))
    if n[int(np.argmax(np.abs(n)))] < 0.0:
        n = -n
    return n, -float(n @ a)


def plane_from_moments(sums, origin, prev_normal, prev_offset=None):
    s, o, prev = np.asarray(sums, np.float64), np.asarray(origin, np.float64), np.asarray(prev_normal, np.float64)
    m = s[0]
    if not m >= 3.0:
        return prev, prev_offset, "degenerate"
    sq = s[4:7]
    sqq = np.array([[s[7], s[8], s[9]], [s[8], s[10], s[11]], [s[9], s[11], s[12]]])
    lam, vec = np.linalg.eigh(sqq - np.outer(sq, sq) / m)
    if not (np.isfinite(lam).all() and lam[1] > 1e-12 * lam[2]):
        return prev, prev_offset, "degenerate"
    n = vec[:, 0] / math.sqrt(float(vec[:, 0] @ vec[:, 0]))
    if float(n @ prev) < 0.0:
        n = -n
    return n, -float(n @ (o + sq / m)), "ok"


def fit_plane(points, weights=None, dist=0.01, num_hypotheses=1024, up=None, max_tilt=None, min_weight=0.0, seed=0,
              refine=2, min_sin2=1e-6, order="pairwise"):
    """support.fit_plane, step by step.  dict(normal, offset, side, height, counts (on, above, below), rmse,
    hypothesis_count, best, status, planes: every (normal, offset) a classify ran against, consensus: the consensus
    record)."""
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    hyp = np.random.default_rng(int(seed)).integers(0, len(p32), size=(int(num_hypotheses), 3), dtype=np.int32)
    u = None if up is None else np.asarray(up, np.float64)
    cos2 = 0.0 if (u is None or max_tilt is None) else math.cos(float(max_tilt)) ** 2
    con = consensus(p32, weights, min_weight, hyp, dist, min_sin2, u, cos2)
    bi, bc = int(con["best"][0]), int(con["best"][1])
    if bi < 0:
        raise ValueError("no valid hypothesis")
    tri = p32[hyp[bi]].astype(np.float64)
    normal, offset = plane_from_triple(*tri)
    if u is not None and float(normal @ u) < 0.0:
        normal, offset = -normal, -offset
    origin, status, planes = tri[0].copy(), "ok", []
    for _ in range(int(refine)):
        planes.append((normal, offset))
        sums = classify(p32, weights, min_weight, [*normal, offset], origin, dist, order)["sums"]
        normal, offset, status = plane_from_moments(sums, origin, normal, offset)
        if status == "ok":
            origin = origin + sums[4:7] / sums[0]
    planes.append((normal, offset))
    cl = classify(p32, weights, min_weight, [*normal, offset], origin, dist, order)
    sums, side, height = cl["sums"].copy(), cl["side"].copy(), cl["height"].copy()
    if u is None and (sums[14] < sums[15] or (sums[14] == sums[15] and normal[int(np.argmax(np.abs(normal)))] < 0)):
        normal, offset = -normal, -offset
        side = np.where(cl["side"] == 0, 2, np.where(cl["side"] == 2, 0, cl["side"])).astype(np.uint8)
        height = -height
        sums[[1, 2, 14, 15]] = sums[[2, 1, 15, 14]]
    on = int(sums[0])
    return dict(normal=normal, offset=offset, side=side, height=height,
                counts=(on, int(sums[1]), int(sums[2])), rmse=math.sqrt(sums[3] / on) if on else math.nan,
                hypothesis_count=bc, best=bi, status=status, planes=planes, consensus=con)


def order_difference(points, **kw):
    """max |difference| over the normal's components and the offset between fit_plane with the moments summed
    pairwise and summed in index order: what the order of a sum alone does to the fitted plane."""
    a, b = fit_plane(points, order="pairwise", **kw), fit_plane(points, order="sequential", **kw)
    return max(float(np.abs(a["normal"] - b["normal"]).max()), abs(a["offset"] - b["offset"]))


# ------------------------------------------------------------------------------------------------
# grasp.plane_clear
# ------------------------------------------------------------------------------------------------
def plane_clear(rows, gripper, normal, offset, approach=0.0, margin=0.0):
    """(clear bool (M,), lowest float64 (M,)): the 8 corners of every part that is not empty, one by one, at t and at
    t - approach a."""
    g = np.asarray(rows, np.float32).astype(np.float64).reshape(-1, 17)
    parts = np.asarray(gripper, np.float64)
    n = np.asarray(normal, np.float64)
    lowest = np.full(len(g), np.inf)
    for m, row in enumerate(g):
        width, height, depth = row[1], row[2], row[3]
        R, t = row[4:13].reshape(3, 3), row[13:16]
        for c in parts:
            b = ((c[:, 0] + c[:, 1] * width) + c[:, 2] * depth) + c[:, 3] * height
            if not (np.isfinite(b).all() and b[0] <= b[1] and b[2] <= b[3] and b[4] <= b[5]):
                continue
            for start in (t, t - float(approach) * R[:, 0]):
                for x in (b[0], b[1]):
                    for y in (b[2], b[3]):
                        for z in (b[4], b[5]):
                            v = float(n @ (start + R @ np.array([x, y, z]))) + float(offset)
                            lowest[m] = v if math.isnan(v) else min(lowest[m], v)
    with np.errstate(invalid="ignore"):
        clear = np.isfinite(g).all(axis=1) & (lowest >= float(margin))
    return clear, lowest


def random_rotations(m, rng):
    """(m, 3, 3) proper rotations from normalised Gaussian quaternions."""
    q = rng.normal(size=(m, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def clear_rows(m, seed):
    """(m, 17) float32 rows over the table scene's plane: random rotations, t at a height uniform in [-0.05, 0.15]
    over the plane, widths 2..8 cm, height 2 cm, depth 2..4 cm."""
    rng = np.random.default_rng(seed)
    t1, t2, n = table_frame()
    R = random_rotations(m, rng)
    xy = rng.uniform(-0.3, 0.3, (m, 2))
    foot = -TRUE_OFFSET * n                                          # a point of the plane
    t = foot + xy[:, :1] * t1 + xy[:, 1:] * t2 + rng.uniform(-0.05, 0.15, (m, 1)) * n
    g = np.zeros((m, 17))
    g[:, 0] = rng.random(m)
    g[:, 1], g[:, 2], g[:, 3] = rng.uniform(0.02, 0.08, m), 0.02, rng.uniform(0.02, 0.04, m)
    g[:, 4:13], g[:, 13:16] = R.reshape(m, 9), t
    return g.astype(np.float32)
