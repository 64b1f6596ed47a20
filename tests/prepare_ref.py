"""Host restatements of scene preparation (gaussiangrasper_amd.prepare), in the operation order of include/gg_raster.h
(gg_backproject, gg_depth_normals, gg_knn), fp64 numpy: numpy neither contracts nor reorders elementwise operations,
so these give the kernels' bits.  Plus the reference's literal formulas (scripts/generate_data.py) and COLMAP text
readers restated from the dataparser's colmap_utils, for the host tests.  No GPU code here."""
import numpy as np


def backproject(depth, mask, rgb, intr, c2w, d_lo=0.001, d_hi=1.2, z_lo=-0.3, z_hi=-0.1):
    """(points (M, 3) fp64, colors (M, 3) uint8) in frame-major, row-major order."""
    pts, cols = [], []
    for f in range(depth.shape[0]):
        d = depth[f]
        h, w = d.shape
        u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        fx, fy, cx, cy = intr[f]
        with np.errstate(invalid="ignore"):
            keep = (mask[f] != 0) & (d > d_lo) & (d < d_hi)
        T = c2w[f]
        with np.errstate(invalid="ignore", over="ignore"):
            X = ((u - cx) * d) / fx
            Y = ((v - cy) * d) / fy
            Z = d
            p = [((T[k, 0] * X + T[k, 1] * Y) + T[k, 2] * Z) + T[k, 3] for k in range(3)]
            keep &= (p[2] > z_lo) & (p[2] < z_hi)
        pts.append(np.stack([p[0][keep], p[1][keep], p[2][keep]], axis=1))
        cols.append(rgb[f][keep])
    return np.concatenate(pts).reshape(-1, 3), np.concatenate(cols).reshape(-1, 3).astype(np.uint8)


def backproject_literal(depth, mask, rgb, fx, fy, cx, cy, c2w):
    """depth_image_to_point_cloud + merge_point_clouds as the reference writes them (np.dot, / after *)."""
    height, width = depth.shape
    u, v = np.meshgrid(np.arange(width), np.arange(height))
    Z = depth
    X = (u - cx) * Z / fx
    Y = (v - cy) * Z / fy
    m = mask * (depth > 0.001) * (depth < 1.2)
    m = m > 0
    pc = np.dstack((X, Y, Z))[m]
    color = rgb[m]
    Tp = np.hstack((pc, np.ones((pc.shape[0], 1)))).T
    mat = np.dot(c2w, Tp).T[:, :3]
    z = (mat[:, 2] > -0.3) * (mat[:, 2] < -0.1)
    return mat[z], color[z]


def _grad(d):
    """np.gradient(d) (rows, columns), edge_order 1, written out."""
    gv = np.empty_like(d)
    gu = np.empty_like(d)
    gv[1:-1] = (d[2:] - d[:-2]) / 2.0
    gv[0] = d[1] - d[0]
    gv[-1] = d[-1] - d[-2]
    gu[:, 1:-1] = (d[:, 2:] - d[:, :-2]) / 2.0
    gu[:, 0] = d[:, 1] - d[:, 0]
    gu[:, -1] = d[:, -1] - d[:, -2]
    return gv, gu


def normals(depth, intr, c2w):
    """(F, H, W, 3) fp64 in gg_depth_normals' order."""
    out = np.empty(depth.shape + (3,))
    for f in range(depth.shape[0]):
        d = np.where(depth[f] < 0.01, 1e-5, depth[f])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            gv, gu = _grad(d)
            a = -(gu * (intr[f][0] / d))
            b = -(gv * (intr[f][1] / d))
            c = np.ones_like(d)
            nrm = np.sqrt((a * a + b * b) + c * c)
            n = [a / nrm, b / nrm, c / nrm]
        bad = ~(np.isfinite(n[0]) & np.isfinite(n[1]) & np.isfinite(n[2]))
        n[0] = np.where(bad, 0.0, n[0])
        n[1] = np.where(bad, 0.0, n[1])
        n[2] = np.where(bad, 1.0, n[2])
        R = c2w[f]
        for k in range(3):
            out[f, ..., k] = (R[k, 0] * n[0] + R[k, 1] * n[1]) + R[k, 2] * n[2]
    return out


def normals_literal(depth, fx, fy, c2w):
    """cal_normal as the reference writes it (np.gradient, np.linalg.norm, np.dot), any H x W."""
    depth = depth.copy()
    depth[depth < 0.01] = 1e-5
    dz_dv, dz_du = np.gradient(depth)
    dz_dx = dz_du * (fx / depth)
    dz_dy = dz_dv * (fy / depth)
    nc = np.dstack((-dz_dx, -dz_dy, np.ones_like(depth)))
    nu = nc / np.linalg.norm(nc, axis=2, keepdims=True)
    nu[~np.isfinite(nu).all(2)] = [0, 0, 1]
    h, w = depth.shape
    return np.dot(c2w[:3, :3], nu.reshape(-1, 3).T).T.reshape((h, w, 3))


def knn(points, k=3, chunk=512, index=False):
    """Brute force: per point the k smallest (sqrt(((dx dx + dy dy) + dz dz)) fp64, index) over j != i, the distance
    rounded to fp32.  Returns (dist (N, k) float32, sorted fp64 squared distances (N, k)) and, with `index`, the
    indices (N, k) int64 of the k smallest (squared distance, index) pairs in that order: gg_knn's tie rule."""
    x = np.asarray(points, dtype=np.float32).astype(np.float64)
    n = x.shape[0]
    d_out = np.empty((n, k), np.float32)
    s_out = np.empty((n, k))
    i_out = np.empty((n, k), np.int64)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        dx = x[a:b, None, 0] - x[None, :, 0]
        dy = x[a:b, None, 1] - x[None, :, 1]
        dz = x[a:b, None, 2] - x[None, :, 2]
        s = (dx * dx + dy * dy) + dz * dz
        s[np.arange(b - a), np.arange(a, b)] = np.inf
        part = np.sort(np.partition(s, k - 1, axis=1)[:, :k], axis=1)
        s_out[a:b] = part
        d_out[a:b] = np.sqrt(part).astype(np.float32)
        if index:
            # every pair up to the k-th distance (all of its ties), sorted by (row, squared distance, index)
            rr, cc = np.nonzero(s <= part[:, k - 1:k])
            order = np.lexsort((cc, s[rr, cc], rr))
            rr, cc = rr[order], cc[order]
            first = np.searchsorted(rr, np.arange(b - a))
            i_out[a:b] = cc[first[:, None] + np.arange(k)]
    return (d_out, s_out, i_out) if index else (d_out, s_out)


def qvec2rotmat(q):
    """colmap_utils.qvec2rotmat"""
    return np.array([
        [1 - 2 * q[2] ** 2 - 2 * q[3] ** 2, 2 * q[1] * q[2] - 2 * q[0] * q[3], 2 * q[3] * q[1] + 2 * q[0] * q[2]],
        [2 * q[1] * q[2] + 2 * q[0] * q[3], 1 - 2 * q[1] ** 2 - 2 * q[3] ** 2, 2 * q[2] * q[3] - 2 * q[0] * q[1]],
        [2 * q[3] * q[1] - 2 * q[0] * q[2], 2 * q[2] * q[3] + 2 * q[0] * q[1], 1 - 2 * q[1] ** 2 - 2 * q[2] ** 2]])


def read_cameras_text(path):
    """colmap_utils.read_cameras_text: {id: (model, width, height, params)}"""
    out = {}
    for line in open(path):
        line = line.strip()
        if line and line[0] != "#":
            e = line.split()
            out[int(e[0])] = (e[1], int(e[2]), int(e[3]), np.array(tuple(map(float, e[4:]))))
    return out


def read_images_text(path):
    """colmap_utils.read_images_text: {id: (qvec, tvec, camera_id, name, xys)}"""
    out = {}
    with open(path) as f:
        while True:
            line = f.readline()
            if not line:
                break
            line = line.strip()
            if line and line[0] != "#":
                e = line.split()
                elems = f.readline().split()
                xys = np.column_stack([tuple(map(float, elems[0::3])), tuple(map(float, elems[1::3]))])
                out[int(e[0])] = (np.array(tuple(map(float, e[1:5]))), np.array(tuple(map(float, e[5:8]))),
                                  int(e[8]), e[9], xys)
    return out


def read_points3D_text(path):
    """colmap_utils.read_points3D_text: {id: (xyz, rgb)}"""
    out = {}
    for line in open(path):
        line = line.strip()
        if line and line[0] != "#":
            e = line.split()
            out[int(e[0])] = (np.array(tuple(map(float, e[1:4]))), np.array(tuple(map(int, e[4:7]))))
    return out


def rodrigues(v):
    v = np.asarray(v, dtype=np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def random_pose(rng, t_scale=0.1):
    T = np.eye(4)
    T[:3, :3] = rodrigues(rng.normal(size=3))
    T[:3, 3] = rng.normal(size=3) * t_scale
    return T


def write_scan(root, n_frames=3, h=24, w=32, seed=0, mask_png=False, units=1.0):
    """A synthetic scan directory: transforms.json, images/*.png, depths/*.npy, boundary_mask/*.npy|png.  Cameras
    look down -z from above a table at z = -0.2, so most pixels pass the workspace window."""
    import json
    import os
    from PIL import Image
    rng = np.random.default_rng(seed)
    for d in ("images", "depths", "boundary_mask"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    fx = fy = 0.9 * w
    meta = {"fl_x": fx, "fl_y": fy, "cx": w / 2 - 0.3, "cy": h / 2 + 0.2, "w": w, "h": h, "camera_model": "OPENCV",
            "k1": -0.05, "k2": 0.06, "p1": -0.0007, "p2": 0.0006, "frames": []}
    for i in range(n_frames):
        stem = f"frame_{i:04d}"
        T = np.eye(4)
        T[:3, :3] = rodrigues(rng.normal(size=3) * 0.1) @ np.diag([1.0, -1.0, -1.0])   # optical axis -z
        T[:3, 3] = [rng.normal() * 0.02, rng.normal() * 0.02, 0.3]
        meta["frames"].append({"file_path": f"images/{stem}.png", "transform_matrix": T.tolist()})
        depth = 0.5 + 0.02 * rng.normal(size=(h, w))
        depth[rng.random((h, w)) < 0.05] = 0.0
        np.save(os.path.join(root, "depths", stem + ".npy"), depth * units)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "images",
                                                                                          stem + ".png"))
        m = (rng.random((h, w)) > 0.1).astype(np.uint8) * 255
        if mask_png:
            Image.fromarray(m).save(os.path.join(root, "boundary_mask", stem + ".png"))
        else:
            np.save(os.path.join(root, "boundary_mask", stem + ".npy"), m)
    with open(os.path.join(root, "transforms.json"), "w") as f:
        json.dump(meta, f)
    return meta
