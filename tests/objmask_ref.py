"""Host restatement of gg_object_masks (include/gg_raster.h; the reference's scripts/project_hull.py :83-121), numpy and
pure Python: the projection in the contract's operation order, truncation, the drop rule, the exact integer monotone
chain hull, the closed-hull fill by per-pixel half-plane tests (not by row intervals, the kernel's formulation),
naive k x k dilation with cv2's anchor, and the boxes.  Test infrastructure: never imported by the package."""
import json
import os

import numpy as np

LIM = 2.0 ** 30


def transform_points(points, T):
    """q_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3, fp64, per row."""
    p = np.asarray(points, np.float64)
    T = np.asarray(T, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def project(q, K, E):
    """(ix, iy, kept): int32 truncated pixels of the kept points, the kept flags of all points."""
    q = np.asarray(q, np.float64)
    E = np.asarray(E, np.float64)
    fx, fy, cx, cy = (float(k) for k in K)
    c = transform_points(q, E)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = ((fx * c[:, 0]) + (cx * c[:, 2])) / c[:, 2]
        v = ((fy * c[:, 1]) + (cy * c[:, 2])) / c[:, 2]
        kept = (c[:, 2] > 0) & (np.abs(u) < LIM) & (np.abs(v) < LIM)
    return u[kept].astype(np.int32), v[kept].astype(np.int32), kept


def project_literal(points, K, E):
    """The reference's own expression (project_points_3d_to_2d :21-34, :91-92): (K @ (E @ P_h.T)[:3])[:2] / [2],
    then astype(np.int32).  E is 4 x 4."""
    Km = np.array([[K[0], 0.0, K[2]], [0.0, K[1], K[3]], [0.0, 0.0, 1.0]])
    ph = np.hstack([points, np.ones((points.shape[0], 1))])
    h = Km @ (E @ ph.T)[:3]
    uv = (h[:2, :] / h[2, :]).T
    return uv, uv.astype(np.int32)


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(xy):
    """Andrew's monotone chain on integer points (Python ints: exact).  Counter-clockwise in (x, y) without collinear
    vertices; [] for no point, [p] for one, [p, q] for a segment."""
    pts = sorted(set((int(x), int(y)) for x, y in xy))
    if len(pts) <= 2:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    hull = lower[:-1] + upper[:-1]
    return hull


def fill(hull, h, w):
    """bool (h, w): pixel (row y, col x) is set iff (x, y) lies in the closed hull (half-plane tests, int64)."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    if not hull:
        return np.zeros((h, w), bool)
    if len(hull) == 1:
        return (xs == hull[0][0]) & (ys == hull[0][1])
    if len(hull) == 2:
        (ax, ay), (bx, by) = hull
        on = (np.int64(bx - ax) * (ys - ay) - np.int64(by - ay) * (xs - ax)) == 0
        return on & (xs >= min(ax, bx)) & (xs <= max(ax, bx)) & (ys >= min(ay, by)) & (ys <= max(ay, by))
    m = np.ones((h, w), bool)
    for i in range(len(hull)):
        (ax, ay), (bx, by) = hull[i], hull[(i + 1) % len(hull)]
        m &= (np.int64(bx - ax) * (ys - ay) - np.int64(by - ay) * (xs - ax)) >= 0
    return m


def dilate(mask, k):
    """cv2.dilate with a k x k ones kernel, anchor (k // 2, k // 2), outside pixels contributing nothing."""
    if k <= 1:
        return mask.copy()
    h, w = mask.shape
    a = k // 2
    out = np.zeros_like(mask)
    for dy in range(k):
        for dx in range(k):
            sy, sx = dy - a, dx - a              # dst(y, x) |= src(y + sy, x + sx)
            y0, y1 = max(0, -sy), min(h, h - sy)
            x0, x1 = max(0, -sx), min(w, w - sx)
            if y0 < y1 and x0 < x1:
                out[y0:y1, x0:x1] |= mask[y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out


def box(mask):
    """(rmin, rmax, cmin, cmax), (centre row, centre col); -1 / NaN when empty (center1, :101-102)."""
    r, c = np.where(mask)
    if r.size == 0:
        return np.array([-1, -1, -1, -1], np.int32), np.array([np.nan, np.nan])
    b = np.array([r.min(), r.max(), c.min(), c.max()], np.int32)
    return b, np.array([0.5 * (int(b[1]) + int(b[0])), 0.5 * (int(b[3]) + int(b[2]))])


def object_masks(points, T, intrinsics, w2c, h, w, k=0):
    """The whole contract: before, after, union (V, h, w) bool, boxes (V, 3, 4) int32, centres (V, 3, 2), dropped
    (V, 2) int32."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    V = len(intrinsics)
    qa = transform_points(points, T)
    out = {"before": np.zeros((V, h, w), bool), "after": np.zeros((V, h, w), bool), "union": np.zeros((V, h, w), bool),
           "boxes": np.zeros((V, 3, 4), np.int32), "centres": np.zeros((V, 3, 2)), "dropped": np.zeros((V, 2), np.int32)}
    for v in range(V):
        masks = []
        for pose, q in enumerate((points, qa)):
            ix, iy, kept = project(q, intrinsics[v], w2c[v])
            out["dropped"][v, pose] = int((~kept).sum())
            masks.append(dilate(fill(convex_hull(zip(ix, iy)), h, w), k))
        masks.append(masks[0] | masks[1])
        for m, name in enumerate(("before", "after", "union")):
            out[name][v] = masks[m]
            out["boxes"][v, m], out["centres"][v, m] = box(masks[m])
    return out


# ------------------------------------------------------------------------------------------------
# synthetic scans
# ------------------------------------------------------------------------------------------------
def rodrigues(r):
    r = np.asarray(r, np.float64)
    t = np.linalg.norm(r)
    if t == 0:
        return np.eye(3)
    k = r / t
    Km = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * Km + (1 - np.cos(t)) * Km @ Km


def look_at_c2w(eye, target):
    """OpenCV camera-to-world (x right, y down, z forward) looking from eye at target."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


def ring(n, radius=0.6, height=0.3, seed=0, target=(0.0, 0.0, 0.0)):
    """n camera-to-world matrices around target, jittered."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        a = 2 * np.pi * i / max(n, 1) + 0.1 * rng.normal()
        eye = np.array([radius * np.cos(a), radius * np.sin(a), height + 0.05 * rng.normal()])
        out.append(look_at_c2w(eye, np.asarray(target) + 0.02 * rng.normal(size=3)))
    return np.array(out)


def write_transforms(path, c2w, h, w, fx, fy, cx, cy, ext=".png", overrides=None):
    meta = {"w": w, "h": h, "fl_x": fx, "fl_y": fy, "cx": cx, "cy": cy, "frames": []}
    for i, T in enumerate(c2w):
        fr = {"file_path": f"images/frame_{i:04d}{ext}", "transform_matrix": np.asarray(T).tolist()}
        fr.update((overrides or {}).get(i, {}))
        meta["frames"].append(fr)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(meta, f)
    return meta
