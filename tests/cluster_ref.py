"""fp64 numpy restatement of the object-instance contract (include/gg_raster.h gg_cluster_dbscan / gg_cluster_stats,
PARITY.md "Object instances"), and the clouds the cluster tests share.

restate: candidate pairs from cKDTree.query_pairs at a slightly widened radius, every candidate re-tested exactly as
the contract writes it ((dx dx + dy dy) + dz dz <= eps eps in fp64, dx the fp64 difference of the fp32 coordinates);
components of the core points from scipy.sparse.csgraph.connected_components; clusters numbered in ascending order
of their smallest core index; border points take the smallest number among their core neighbours."""
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


def restate(points, eps, min_points, active=None):
    """dict(labels int32 (N,), core bool (N,), neighbor_count int32 (N,), num_clusters int, near int): `near` is
    the number of pairs with |d - eps| < 1e-9 eps, where another rounding could decide otherwise."""
    p = np.ascontiguousarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(p)
    act = np.isfinite(p).all(axis=1)
    if active is not None:
        act &= np.asarray(active).reshape(-1) != 0
    idx = np.nonzero(act)[0]
    q = p[idx]
    m = len(q)
    eps = float(eps)
    if m:
        pairs = cKDTree(q).query_pairs(eps * (1.0 + 1e-6), output_type="ndarray")
    else:
        pairs = np.zeros((0, 2), np.int64)
    d = q[pairs[:, 0]] - q[pairs[:, 1]]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    near = int((np.abs(np.sqrt(d2) - eps) < 1e-9 * eps).sum())
    pairs = pairs[d2 <= eps * eps]
    a, b = pairs[:, 0], pairs[:, 1]
    cnt = 1 + np.bincount(a, minlength=m) + np.bincount(b, minlength=m)
    core = cnt >= min_points
    cc = core[a] & core[b]
    ncomp, comp = connected_components(coo_matrix((np.ones(cc.sum(), np.int8), (a[cc], b[cc])), shape=(m, m)),
                                       directed=False)
    # smallest core index of every component that has a core point; numbered in that order
    first = np.full(ncomp, m, np.int64)
    np.minimum.at(first, comp[core], np.nonzero(core)[0])
    order = np.argsort(first, kind="stable")
    k = int((first < m).sum())
    number = np.full(ncomp, -1, np.int64)
    number[order[:k]] = np.arange(k)
    big = np.iinfo(np.int64).max
    lab = np.where(core, number[comp], big)
    for u, v in ((a, b), (b, a)):                      # u core, v not: v is a border point of u's cluster
        sel = core[u] & ~core[v]
        np.minimum.at(lab, v[sel], number[comp[u[sel]]])
    lab[lab == big] = -1
    out = dict(labels=np.full(n, -1, np.int32), core=np.zeros(n, bool), neighbor_count=np.zeros(n, np.int32),
               num_clusters=k, near=near)
    out["labels"][idx] = lab
    out["core"][idx] = core
    out["neighbor_count"][idx] = cnt
    return out


def restate_stats(points, weights, labels, num_clusters):
    """Per cluster: count, weight (math.fsum: correctly rounded), centroid, bbox, and the summation bounds
    weight_bound = M 2^-52 sum|w| and centroid_bound = M 2^-52 (sum|w x| + |c| sum|w|) / W  (M members)."""
    p32 = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    p, w = p32.astype(np.float64), np.ascontiguousarray(weights, np.float32).astype(np.float64)
    k = int(num_clusters)
    out = dict(count=np.zeros(k, np.int64), weight=np.zeros(k), centroid=np.zeros((k, 3)),
               bbox=np.zeros((k, 6), np.float32), weight_bound=np.zeros(k), centroid_bound=np.zeros((k, 3)))
    order = np.argsort(labels, kind="stable")
    lo = np.searchsorted(labels[order], np.arange(k), "left")
    hi = np.searchsorted(labels[order], np.arange(k), "right")
    for c in range(k):
        mem = order[lo[c]:hi[c]]
        m = len(mem)
        W = math.fsum(w[mem])
        out["count"][c], out["weight"][c] = m, W
        out["weight_bound"][c] = m * 2.0 ** -52 * math.fsum(np.abs(w[mem]))
        for ax in range(3):
            t = w[mem] * p[mem, ax]
            cen = math.fsum(t) / W
            out["centroid"][c, ax] = cen
            out["centroid_bound"][c, ax] = (m * 2.0 ** -52 * (math.fsum(np.abs(t)) + abs(cen) * math.fsum(np.abs(w[mem])))
                                            / W + 2.0 ** -51 * abs(cen))
        out["bbox"][c, :3], out["bbox"][c, 3:] = p32[mem].min(axis=0), p32[mem].max(axis=0)
    return out


# ------------------------------------------------------------------------------------------------
# clouds
# ------------------------------------------------------------------------------------------------
def blobs(seed, n, num_blobs=6, sigma=0.03, noise=0.15, box=1.0):
    """Gaussian blobs in a box plus uniform noise, float32, in random index order."""
    rng = np.random.default_rng(seed)
    nn = int(noise * n)
    centres = rng.uniform(0.15 * box, 0.85 * box, size=(num_blobs, 3))
    which = rng.integers(0, num_blobs, n - nn)
    p = np.concatenate([centres[which] + rng.normal(scale=sigma, size=(n - nn, 3)),
                        rng.uniform(0.0, box, size=(nn, 3))])
    return p[rng.permutation(n)].astype(np.float32)


def blobs_without_ties(seed, n, eps, min_points, **kw):
    """blobs(...) of the first seed at or after `seed` (in steps of 1000) whose cloud has no pair within 1e-9 eps of
    eps, and its restatement: the comparison against another implementation then needs to exclude no point."""
    for s in range(seed, seed + 20_000, 1000):
        p = blobs(s, n, **kw)
        ref = restate(p, eps, min_points)
        if ref["near"] == 0:
            return p, ref
    raise AssertionError("no cloud without near-eps pairs found")


def lattice(seed=0, side=12, fill=0.6, spacing=0.25):
    """A partly filled cubic lattice: every coordinate a multiple of `spacing`, so that with eps == spacing the
    axis neighbours sit exactly on the boundary and every product of the test is exact."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.random(len(g)) < fill]
    return (g[rng.permutation(len(g))] * spacing).astype(np.float32)


def with_duplicates(seed, n, **kw):
    """blobs with a third of the rows repeated two to four times."""
    rng = np.random.default_rng(seed + 7)
    p = blobs(seed, n, **kw)
    src = rng.choice(n, n // 3, replace=False)
    rep = np.repeat(src, rng.integers(1, 4, len(src)))
    q = np.concatenate([p, p[rep]])
    return q[rng.permutation(len(q))]


def helix(n, step, radius=50.0, rise=1.0, phase=0.0, z0=0.0):
    """n points along a helix at arc spacing `step`; consecutive turns are 2 pi rise apart."""
    t = np.arange(n) * (step / math.hypot(radius, rise))
    return np.stack([radius * np.cos(t + phase), radius * np.sin(t + phase), z0 + rise * t], 1).astype(np.float32)
