"""numpy fp32 restatement of the mesh-export contract (include/gg_raster.h, gg_tsdf_*): the same operations in the same
order, so the kernels are held to it bit for bit.  Also the analytic scenes the tests share: ray-cast depth maps of
spheres, cameras looking at the origin, and mesh topology checks."""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]], dtype=np.int64)
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


# ------------------------------------------------------------------------------------------------
# the marching-tetrahedra table
# ------------------------------------------------------------------------------------------------
def _corner(t, n):
    c = [0, 0, 0]
    for s in range(min(n, 3)):
        c[PERMS[t][s]] = 1
    return np.array(c, dtype=np.int64)


def _cid(c):
    return int(c[0]) * 4 + int(c[1]) * 2 + int(c[2])


def _edge_code(t, a, b):
    lo, hi = min(a, b), max(a, b)
    cl, ch = _corner(t, lo), _corner(t, hi)
    d = [q for q in range(7) if (DIRS[q] == ch - cl).all()][0]
    return _cid(cl) * 8 + d


def _orient(t, edges, w):
    cw = _corner(t, w)
    m = np.array([_corner(t, a) + _corner(t, b) - 2 * cw for a, b in edges], dtype=np.int64)
    return int(round(np.linalg.det(m.astype(np.float64))))


def make_table():
    """(corner (6, 4), ntri (6, 16), edge (6, 16, 2, 3)): corner ids (ox << 2 | oy << 1 | oz) of each Kuhn
    tetrahedron and, per inside-case, its triangles as edge codes (lower corner id * 8 + direction)."""
    corner = np.zeros((6, 4), np.int64)
    ntri = np.zeros((6, 16), np.int64)
    edge = np.zeros((6, 16, 2, 3), np.int64)
    for t in range(6):
        for n in range(4):
            corner[t, n] = _cid(_corner(t, n))
        for cs in range(16):
            ins = [n for n in range(4) if (cs >> n) & 1]
            outs = [n for n in range(4) if not (cs >> n) & 1]
            tris = []
            if len(ins) in (1, 3):
                a = ins[0] if len(ins) == 1 else outs[0]
                o = outs if len(ins) == 1 else ins
                tris.append(([(a, o[0]), (a, o[1]), (a, o[2])], a, 1 if len(ins) == 1 else -1))
            elif len(ins) == 2:
                p, q = ins
                r, s = outs
                tris.append(([(p, r), (p, s), (q, s)], p, 1))
                tris.append(([(p, r), (q, s), (q, r)], q, 1))
            ntri[t, cs] = len(tris)
            for k, (e, w, sign) in enumerate(tris):
                if sign * _orient(t, e, w) < 0:
                    e = [e[0], e[2], e[1]]
                edge[t, cs, k] = [_edge_code(t, a, b) for a, b in e]
    return corner, ntri, edge


TABLE = make_table()


def _corner_offset(dims, cid):
    X, Y, Z = dims
    return (((cid >> 2) & 1) * Y + ((cid >> 1) & 1)) * Z + (cid & 1)


# ------------------------------------------------------------------------------------------------
# integration
# ------------------------------------------------------------------------------------------------
def lattice(dims, grid):
    """fp32 coordinates x, y, z of every point, flattened in C order."""
    X, Y, Z = dims
    g = np.asarray(grid, dtype=f32)
    ax = [g[a] + np.arange(n, dtype=f32) * g[3 + a] for a, n in enumerate((X, Y, Z))]
    x, y, z = np.meshgrid(ax[0], ax[1], ax[2], indexing="ij")
    return x.ravel(), y.ravel(), z.ravel()


def new_volume(dims, color=False):
    """tsdf 1, weight 0 (and colour 0, colour weight 0): what TSDFVolume starts from."""
    P = int(np.prod(dims))
    vol = {"tsdf": np.ones(P, f32), "weight": np.zeros(P, f32)}
    if color:
        vol["color"] = np.zeros((P, 3), f32)
        vol["color_weight"] = np.zeros(P, f32)
    return vol


def integrate(vol, dims, grid, trunc, depth, intrinsics, w2c, rgb=None):
    """gg_tsdf_integrate on a dict of flat fp32 arrays (updated in place and returned)."""
    depth = np.asarray(depth, dtype=f32)
    V, H, W = depth.shape
    K = np.asarray(intrinsics, dtype=f32).reshape(V, 4)
    E = np.asarray(w2c, dtype=f32).reshape(V, 3, 4)
    tr = f32(trunc)
    x, y, z = lattice(dims, grid)
    T, Wt = vol["tsdf"].copy(), vol["weight"].copy()
    if rgb is not None:
        rgb = np.asarray(rgb, dtype=f32).reshape(V, H, W, 3)
        C, Kw = vol["color"].copy(), vol["color_weight"].copy()
    with np.errstate(all="ignore"):
        for v in range(V):
            e = E[v]
            c2 = ((e[2, 0] * x + e[2, 1] * y) + e[2, 2] * z) + e[2, 3]
            c0 = ((e[0, 0] * x + e[0, 1] * y) + e[0, 2] * z) + e[0, 3]
            c1 = ((e[1, 0] * x + e[1, 1] * y) + e[1, 2] * z) + e[1, 3]
            ok = c2 > 0
            u = (K[v, 0] * c0) / c2 + K[v, 2]
            vv = (K[v, 1] * c1) / c2 + K[v, 3]
            ok &= (u >= 0) & (u < f32(W)) & (vv >= 0) & (vv < f32(H))
            col = np.where(ok, u, 0).astype(np.int64)
            row = np.where(ok, vv, 0).astype(np.int64)
            d = np.where(ok, depth[v][row, col], f32(0))
            ok &= d > 0
            dist = d - c2
            ok &= dist >= -tr
            obs = np.minimum(f32(1), dist / tr)
            Wn = Wt + f32(1)
            T = np.where(ok, (T * Wt + obs) / Wn, T)
            Wt = np.where(ok, Wn, Wt)
            if rgb is not None:
                okc = ok & (np.abs(dist) < tr)
                Kn = Kw + f32(1)
                px = rgb[v][row, col]
                C = np.where(okc[:, None], (C * Kw[:, None] + px) / Kn[:, None], C)
                Kw = np.where(okc, Kn, Kw)
    vol["tsdf"], vol["weight"] = T.astype(f32), Wt.astype(f32)
    if rgb is not None:
        vol["color"], vol["color_weight"] = C.astype(f32), Kw.astype(f32)
    return vol


# ------------------------------------------------------------------------------------------------
# extraction
# ------------------------------------------------------------------------------------------------
def _gradient(T3, grid):
    """(X, Y, Z, 3) fp32 TSDF gradient: central differences inside, one-sided at the borders."""
    g = np.asarray(grid, dtype=f32)
    out = np.zeros(T3.shape + (3,), f32)
    for a in range(3):
        n = T3.shape[a]
        if n < 2:
            continue
        s = g[3 + a]
        Tm = np.moveaxis(T3, a, 0)
        G = np.moveaxis(out[..., a], a, 0)
        G[0] = (Tm[1] - Tm[0]) / s
        G[n - 1] = (Tm[n - 1] - Tm[n - 2]) / s
        if n > 2:
            G[1:n - 1] = (Tm[2:] - Tm[:-2]) / (f32(2) * s)
    return out


def extract(dims, grid, tsdf, weight, color=None):
    """gg_tsdf_mesh_count + gg_tsdf_mesh_emit: (vertices (Nv, 3), normals (Nv, 3), colors (Nv, 3) or None,
    faces (Nf, 3) int32)."""
    X, Y, Z = (int(d) for d in dims)
    P = X * Y * Z
    g = np.asarray(grid, dtype=f32)
    T = np.asarray(tsdf, dtype=f32).reshape(P)
    Wt = np.asarray(weight, dtype=f32).reshape(P)
    corner, ntri, edge = TABLE
    ii, jj, kk = np.meshgrid(np.arange(max(X - 1, 0)), np.arange(max(Y - 1, 0)), np.arange(max(Z - 1, 0)),
                             indexing="ij")
    cell = ((ii * Y + jj) * Z + kk).ravel()
    offs = np.array([_corner_offset(dims, c) for c in range(8)], dtype=np.int64)
    Tc = T[cell[:, None] + offs[None, :]]                                  # (cells, 8)
    obs = (Wt[cell[:, None] + offs[None, :]] > 0).all(axis=1)
    inside = Tc < 0
    mask = np.zeros(P, np.int64)
    tris = []                                                             # (key, codes (n, 3), cell)
    for t in range(6):
        cs = sum(inside[:, corner[t, n]].astype(np.int64) << n for n in range(4))
        for s in range(2):
            sel = obs & (ntri[t, cs] > s)
            c = cell[sel]
            codes = edge[t, cs[sel], s]                                   # (m, 3)
            for e in range(3):
                q = c + offs[codes[:, e] >> 3]
                np.bitwise_or.at(mask, q, 1 << (codes[:, e] & 7))
            tris.append((c * 12 + t * 2 + s, codes, c))
    counts = np.array([bin(m).count("1") for m in range(128)], np.int64)
    vbase = np.concatenate(([0], np.cumsum(counts[mask])[:-1])) if P else np.zeros(0, np.int64)
    nv = int(counts[mask].sum())

    def vid(q, d):
        return vbase[q] + counts[mask[q] & ((1 << d) - 1)]

    keys = np.concatenate([k for k, _, _ in tris]) if tris else np.zeros(0, np.int64)
    fv = []
    for _, codes, c in tris:
        cols = []
        for e in range(3):
            q = c + offs[codes[:, e] >> 3]
            cols.append(vid(q, codes[:, e] & 7))
        fv.append(np.stack(cols, axis=1) if len(c) else np.zeros((0, 3), np.int64))
    faces = np.concatenate(fv) if fv else np.zeros((0, 3), np.int64)
    faces = faces[np.argsort(keys, kind="stable")].astype(np.int32)

    T3 = T.reshape(X, Y, Z)
    grad = _gradient(T3, g).reshape(P, 3)
    verts = np.zeros((nv, 3), f32)
    nrms = np.zeros((nv, 3), f32)
    cols_out = np.zeros((nv, 3), f32) if color is not None else None
    C = None if color is None else np.asarray(color, dtype=f32).reshape(P, 3)
    stride = np.array([Y * Z, Z, 1], dtype=np.int64)
    pidx = np.arange(P)
    ia = np.stack([pidx // (Y * Z), (pidx // Z) % Y, pidx % Z], axis=1)
    with np.errstate(all="ignore"):
        for d in range(7):
            p = np.nonzero((mask >> d) & 1)[0]
            if len(p) == 0:
                continue
            q = p + (DIRS[d] * stride).sum()
            Ta, Tb = T[p], T[q]
            t = Ta / (Ta - Tb)
            ids = vid(p, d)
            n = np.zeros((len(p), 3), f32)
            for a in range(3):
                fa = ia[p, a].astype(f32)
                gc = fa + t if DIRS[d, a] else fa
                verts[ids, a] = g[a] + gc * g[3 + a]
                n[:, a] = grad[p, a] + t * (grad[q, a] - grad[p, a])
            ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            nrms[ids] = np.where(ln[:, None] > 0, n / ln[:, None], f32(0))
            if C is not None:
                for a in range(3):
                    ca, cb = C[p, a], C[q, a]
                    cols_out[ids, a] = ca + t * (cb - ca)
    return verts, nrms, cols_out, faces


# ------------------------------------------------------------------------------------------------
# analytic scenes and mesh checks (shared by the host and GPU tests)
# ------------------------------------------------------------------------------------------------
def look_at_w2c(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """(3, 4) fp64 world-to-camera, OpenCV axes (x right, y down, z forward), camera at eye looking at target."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    zc = target - eye
    zc /= np.linalg.norm(zc)
    if abs(float(np.dot(zc, up))) > 0.99:
        up = np.array([0.0, 1.0, 0.0])
    xc = np.cross(zc, up)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    R = np.stack([xc, yc, zc])
    return np.concatenate([R, (-R @ eye)[:, None]], axis=1)


def sphere_cameras(n, radius):
    """n cameras on a Fibonacci sphere of the given radius, looking at the origin: w2c (n, 3, 4) fp64."""
    out = []
    for i in range(n):
        zc = 1.0 - 2.0 * (i + 0.5) / n
        r = math.sqrt(max(0.0, 1.0 - zc * zc))
        ph = i * math.pi * (3.0 - math.sqrt(5.0))
        out.append(look_at_w2c(radius * np.array([r * math.cos(ph), r * math.sin(ph), zc])))
    return np.stack(out)


def raycast_spheres(w2c, K, H, W, spheres):
    """Projective depth (z) of the nearest of `spheres` [(centre, radius), ...] through every pixel centre; +inf
    where a ray misses them all.  fp64 then fp32."""
    R, t = w2c[:, :3], w2c[:, 3]
    eye = -R.T @ t
    u, v = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    dc = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], axis=-1)   # z = 1 per unit s
    dw = dc @ R                                                                         # world direction
    best = np.full((H, W), np.inf)
    for c, r in spheres:
        oc = eye - np.asarray(c, np.float64)
        a = (dw * dw).sum(-1)
        b = 2.0 * (dw @ oc)
        cc = float(oc @ oc) - r * r
        disc = b * b - 4 * a * cc
        s = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2 * a)
        hit = (disc >= 0) & (s > 0)
        best = np.where(hit & (s < best), s, best)
    return best.astype(np.float32)


def check_closed_manifold(faces, num_vertices):
    """Every directed edge occurs exactly once and its reverse exactly once; every vertex is used.  Returns the
    Euler characteristic V - E + F."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = e[:, 0] * num_vertices + e[:, 1]
    rkey = e[:, 1] * num_vertices + e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    assert (cnt == 1).all(), f"{int((cnt > 1).sum())} directed edges occur more than once"
    assert np.isin(rkey, uniq).all(), f"{int((~np.isin(rkey, uniq)).sum())} edges have no reverse (boundary)"
    assert np.unique(f).size == num_vertices, "orphan vertices"
    return num_vertices - len(uniq) // 2 + len(f)


def face_normals(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
