"""The memory contract of the geometry and task entry points that predate the sentinel habit (grasp, kNN, prepare,
cluster, ICP, TSDF, object masks, hull edit, clip query, image and geometry losses), one test per family, every call
through ctypes on a sentinel arena (tests/arena.py).  The training path's entries (view chain, projection, binning,
blend, MLP, cosine loss) are held the same way by tests/test_memory_contract_core_gpu.py, which imports this file's
helpers.

  * every device array at exactly the smallest alignment include/gg_raster.h and the entry point's GG_REQUIRE allow
    (byte arrays at odd addresses), followed by a guard;
  * the workspace exactly the queried number of bytes, inside the arena, full of garbage; every call made twice with
    different garbage: outputs PARITY.md calls deterministic are byte-equal, the others within their bound both times;
  * outputs held to the restatement under the criterion of the family's present GPU test (no new tolerance); rows the
    header says are not written still hold the sentinel;
  * guards and inputs unchanged (Arena.check);
  * the empty call the header defines returns its status and writes nothing but what the header says it writes;
  * a pointer one step below its alignment is refused before any launch: non-zero status, gg_last_error() naming the
    argument, nothing written.  No call here hands a kernel a pointer the header forbids."""
import ctypes
import re

import numpy as np
import pytest
import torch

from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = ctypes.c_void_p
F32, F64, I32, I64, U8 = np.float32, np.float64, np.int32, np.int64, np.uint8


def _lib():
    from gaussiangrasper_amd import _lib
    return _lib.load()


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _err():
    return _lib().gg_last_error().decode("utf-8", "replace")


def _ptrs(ar, shift=None):
    """name -> c_void_p of the region (None -> NULL), moved by shift[name] bytes"""
    def p(name, plus=0):
        if name is None:
            return P(None)
        return P(ar.address(name) + plus + (shift or {}).get(name, 0))
    return p


def _carve(ar, role, align, **arrays):
    for name, a in arrays.items():
        if a is not None:
            ar.carve(name, a, align, role)


def _refused(ar, status, word):
    """non-zero status, the message names `word` as a whole name (`normals` is not named by `normals_out`), and
    nothing was written"""
    msg = _err()
    assert status != 0 and re.search(r"(?<![A-Za-z0-9_])" + re.escape(word) + r"(?![A-Za-z0-9_])", msg), \
        (status, word, msg)
    ar.untouched()


def _same_bytes(a, b, keys):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _is_sentinel(ar, name, a):
    return np.array_equal(np.ascontiguousarray(a).view(U8).reshape(-1),
                          np.full(a.nbytes, ar.sentinel, U8))


def _grid_args(grid, dims):
    return (ctypes.c_double * 4)(*[float(v) for v in grid]), (ctypes.c_int32 * 3)(*[int(v) for v in dims])


# ------------------------------------------------------------------------------------------------
# gg_grasp_contacts
# ------------------------------------------------------------------------------------------------
CONTACT_OUTS = ("contact_idx", "normals_out", "angles", "region_count", "region_weight", "collision_weight", "feasible")


def contacts_call(p, nr, w, g, seed, shift=None, **kw):
    import grasp_ref
    lib = _lib()
    o = dict(grasp_ref.DEFAULTS, **kw)
    n, m = len(p), len(g)
    need = lib.gg_grasp_contacts_workspace(n, m)
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, points=np.asarray(p, F32), normals=np.asarray(nr, F32), weights=np.asarray(w, F32),
           grasps=np.asarray(g, F32).reshape(m, 17))
    _carve(ar, "out", 4, contact_idx=np.empty((m, 2), I32), normals_out=np.empty((m, 2, 3), F32),
           angles=np.empty((m, 2), F32), region_count=np.empty(m, I32), region_weight=np.empty(m, F32),
           collision_weight=np.empty(m, F32))
    ar.carve("feasible", np.empty(m, U8), 1, "out")
    ar.carve("ws", need, 256, "ws")
    q = _ptrs(ar, shift)
    st = lib.gg_grasp_contacts(n, q("points"), q("normals"), q("weights"), m, q("grasps"), o["depth_base"],
                               o["finger_width"], o["band"], o["mu"], o["min_weight"], o["max_collision"],
                               *[q(k) for k in CONTACT_OUTS], q("ws"), need, _stream())
    return ar, st, need


@pytest.mark.parametrize("n,m", [(1, 1), (513, 257), (5000, 600)])
def test_grasp_contacts(n, m):
    import grasp_ref
    import test_grasp_gpu as G
    rng = np.random.default_rng(1000 * n + m)
    p, nr, w = G.scene(rng, n)
    if n == 1:
        p[0] = 0.0
    g = G.candidates(rng, m, p)
    kw = dict(mu=0.7, max_collision=2.0)
    ref = grasp_ref.restate(p, nr, w, g, **kw)
    runs = []
    for seed in (1, 2):
        ar, st, need = contacts_call(p, nr, w, g, seed, **kw)
        assert st == 0 and need > 0 and need % 256 == 0, _err()
        out = ar.check()
        got = dict(out, normals=out["normals_out"])
        G.check(got, ref)
        runs.append(out)
    _same_bytes(runs[0], runs[1], CONTACT_OUTS)
    if n >= 513:
        assert (ref["region_count"] > 0).any()
    # num_grasps == 0 does nothing
    ar, st, need = contacts_call(p, nr, w, g[:0], 3, **kw)
    assert st == 0 and need == 0
    ar.untouched()
    if n == 513:
        for name in ("points", "normals", "weights", "grasps") + CONTACT_OUTS[:-1]:
            ar, st, _ = contacts_call(p, nr, w, g, 4, shift={name: 2}, **kw)
            _refused(ar, st, name)
        ar, st, _ = contacts_call(p, nr, w, g, 4, shift={"ws": 128}, **kw)
        _refused(ar, st, "ws")


# ------------------------------------------------------------------------------------------------
# gg_grasp_propose
# ------------------------------------------------------------------------------------------------
PROPOSE_OUTS = ("pair_idx", "tube_count", "span", "valid", "rows")


def propose_call(p, nr, w, seeds, seed, shift=None, **kw):
    import grasp_propose_ref
    lib = _lib()
    o = dict(grasp_propose_ref.DEFAULTS, **kw)
    n, s, k = len(p), len(seeds), int(o["num_approach"])
    need = lib.gg_grasp_propose_workspace(n, s)
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, points=np.asarray(p, F32), normals=np.asarray(nr, F32), weights=np.asarray(w, F32),
           seeds=np.asarray(seeds, I32))
    _carve(ar, "out", 4, pair_idx=np.empty((s, 2), I32), tube_count=np.empty(s, I32), span=np.empty(s, F32))
    ar.carve("valid", np.empty(s, U8), 1, "out")
    ar.carve("rows", np.empty((s, k, 17), F32), 4, "out")
    ar.carve("ws", need, 256, "ws")
    q = _ptrs(ar, shift)
    up = (ctypes.c_double * 3)(*o["up"])
    st = lib.gg_grasp_propose(n, q("points"), q("normals"), q("weights"), s, q("seeds"), o["tube_radius"],
                              o["max_width"], o["min_width"], o["clearance"], o["depth"], o["height"], o["min_weight"],
                              o["min_align"], ctypes.cast(up, P), k, *[q(x) for x in PROPOSE_OUTS], q("ws"), need,
                              _stream())
    return ar, st, need


@pytest.mark.parametrize("n,s,k", [(1, 1, 1), (513, 65, 8), (1000, 257, 3)])
def test_grasp_propose(n, s, k):
    import grasp_propose_ref
    import test_grasp_propose_gpu as G
    rng = np.random.default_rng(100 * n + 10 * s + k)
    p, nr, w = G.scene(rng, n)
    seeds = G.some_seeds(rng, s, n)
    kw = dict(num_approach=k, tube_radius=0.02, up=(0.1, -0.2, 1.0), min_align=0.3)
    ref = grasp_propose_ref.restate(p, nr, w, seeds, **kw)
    runs = []
    for seed in (1, 2):
        ar, st, need = propose_call(p, nr, w, seeds, seed, **kw)
        assert st == 0 and need > 0 and need % 256 == 0, _err()
        out = ar.check()
        G.check(out, ref)
        runs.append(out)
    _same_bytes(runs[0], runs[1], PROPOSE_OUTS)
    if n >= 513:
        assert ref["valid"].any() and not ref["valid"].all() and ref["tube_count"].max() > 2
    ar, st, need = propose_call(p, nr, w, seeds[:0], 3, **kw)          # num_seeds == 0 does nothing
    assert st == 0 and need == 0
    ar.untouched()
    if n == 513:
        for name in ("points", "normals", "weights", "seeds", "pair_idx", "tube_count", "span", "rows"):
            ar, st, _ = propose_call(p, nr, w, seeds, 4, shift={name: 2}, **kw)
            _refused(ar, st, name)
        ar, st, _ = propose_call(p, nr, w, seeds, 4, shift={"ws": 128}, **kw)
        _refused(ar, st, "ws")


# ------------------------------------------------------------------------------------------------
# gg_knn
# ------------------------------------------------------------------------------------------------
def knn_call(x, k, grid, dims, seed, shift=None):
    lib = _lib()
    n = len(x)
    gc, dc = _grid_args(grid, dims)
    need = lib.gg_knn_workspace(n, dc)
    ar = Arena(DEV, seed)
    ar.carve("points", np.asarray(x, F32), 4, "in")
    ar.carve("dist", np.empty((n, k), F32), 4, "out")
    ar.carve("idx", np.empty((n, k), I64), 8, "out")
    ar.carve("ws", need, 256, "ws")
    q = _ptrs(ar, shift)
    st = lib.gg_knn(n, q("points"), k, gc, dc, q("dist"), q("idx"), q("ws"), need, _stream())
    return ar, st, need


@pytest.mark.parametrize("n", [1, 5, 257, 3000])
def test_knn(n):
    import prepare_ref
    from gaussiangrasper_amd.grid import knn_grid
    x = np.random.default_rng(40 + n).random((n, 3)).astype(F32)
    grids = {"fitted": knn_grid(torch.from_numpy(x)), "one cell": ((0.0, 0.0, 0.0, 1.0), (1, 1, 1))}
    if n == 1:                                         # k < num_points is the contract: refused, nothing written
        for grid, dims in grids.values():
            ar, st, need = knn_call(x, 3, grid, dims, 1)
            assert need > 0
            _refused(ar, st, "num_points")
        return
    ref_d, ref_s, ref_i = prepare_ref.knn(x, 3, index=True)
    assert (ref_s[:, 0] > 0.0).all()                   # no duplicates: every index is pinned
    runs = []
    for name, (grid, dims) in grids.items():
        for seed in (1, 2):
            ar, st, need = knn_call(x, 3, grid, dims, seed)
            assert st == 0 and need > 0 and need % 256 == 0, (name, _err())
            out = ar.check()
            assert np.array_equal(_bits(out["dist"]), _bits(ref_d)), name
            assert np.array_equal(out["idx"], ref_i), name
            runs.append(out)
    for r in runs[1:]:
        _same_bytes(runs[0], r, ("dist", "idx"))
    if n == 257:
        grid, dims = grids["fitted"]
        for name, step in (("points", 2), ("dist", 2), ("idx", 4)):
            ar, st, _ = knn_call(x, 3, grid, dims, 3, shift={name: step})
            _refused(ar, st, name)
        ar, st, _ = knn_call(x, 3, grid, dims, 3, shift={"ws": 128})
        _refused(ar, st, "ws")


# ------------------------------------------------------------------------------------------------
# gg_backproject, gg_subsample, gg_depth_normals
# ------------------------------------------------------------------------------------------------
def backproject_call(depth, mask, rgb, intr, c2w, seed, shift=None, window=(0.001, 1.2, -0.3, -0.1)):
    lib = _lib()
    f, h, w = depth.shape
    need = lib.gg_backproject_workspace(f, h, w)
    ar = Arena(DEV, seed)
    ar.carve("depth", np.asarray(depth, F64), 8, "in")
    ar.carve("mask", np.asarray(mask, U8), 1, "in")
    ar.carve("rgb", np.asarray(rgb, U8), 1, "in")
    ar.carve("intrinsics", np.asarray(intr, F64), 8, "in")
    ar.carve("c2w", np.asarray(c2w, F64), 8, "in")
    ar.carve("points", np.empty((f * h * w, 3), F64), 8, "out")
    ar.carve("colors", np.empty((f * h * w, 3), U8), 1, "out")
    ar.carve("count", np.empty(1, I64), 8, "out")
    ar.carve("ws", need, 256, "ws")
    q = _ptrs(ar, shift)
    st = lib.gg_backproject(f, h, w, q("depth"), q("mask"), q("rgb"), q("intrinsics"), q("c2w"), *window, q("points"),
                            q("colors"), q("count"), q("ws"), need, _stream())
    return ar, st, need


def test_backproject():
    import prepare_ref
    import test_prepare_gpu as G
    depth, mask, rgb, intr, c2w = (a[:2] for a in G._frames(0, 4, 13, 17))
    rp, rc = prepare_ref.backproject(depth, mask, rgb, intr, c2w)
    m = len(rp)
    assert 0 < m < depth.size
    runs = []
    for seed in (1, 2):
        ar, st, need = backproject_call(depth, mask, rgb, intr, c2w, seed)
        assert st == 0 and need > 0 and need % 256 == 0, _err()
        out = ar.check()
        assert out["count"][0] == m
        assert np.array_equal(_bits(out["points"][:m]), _bits(rp)) and np.array_equal(out["colors"][:m], rc)
        # rows past the count are not written
        assert _is_sentinel(ar, "points", out["points"][m:]) and _is_sentinel(ar, "colors", out["colors"][m:])
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("points", "colors", "count"))
    # num_frames == 0 writes the count, 0, and nothing else
    ar, st, need = backproject_call(depth[:0], mask[:0], rgb[:0], intr[:0], c2w[:0], 3)
    assert st == 0, _err()
    out = ar.check()
    assert out["count"][0] == 0 and out["points"].size == 0
    for name in ("depth", "intrinsics", "c2w", "points", "count"):
        ar, st, _ = backproject_call(depth, mask, rgb, intr, c2w, 4, shift={name: 4})
        _refused(ar, st, name)
    ar, st, _ = backproject_call(depth, mask, rgb, intr, c2w, 4, shift={"ws": 128})
    _refused(ar, st, "ws")


def subsample_call(pts, cols, keep, law_seed, seed, shift=None):
    lib = _lib()
    num = len(pts)
    m = num // keep
    need = lib.gg_subsample_workspace(num)
    ar = Arena(DEV, seed)
    ar.carve("points", np.asarray(pts, F64), 8, "in")
    ar.carve("colors", np.asarray(cols, U8), 1, "in")
    ar.carve("out_points", np.empty((m, 3), F64), 8, "out")
    ar.carve("out_colors", np.empty((m, 3), U8), 1, "out")
    ar.carve("out_index", np.empty(m, I64), 8, "out")
    ar.carve("ws", need, 256, "ws")
    q = _ptrs(ar, shift)
    st = lib.gg_subsample(num, keep, law_seed, q("points"), q("colors"), q("out_points"), q("out_colors"),
                          q("out_index"), q("ws"), need, _stream())
    return ar, st, need


def test_subsample():
    from gaussiangrasper_amd.prepare import subsample_indices
    rng = np.random.default_rng(2)
    pts, cols = rng.normal(size=(1000, 3)), rng.integers(0, 256, (1000, 3), dtype=U8)
    ref = subsample_indices(1000, 8, 12345)
    assert len(ref) == 125
    runs = []
    for seed in (1, 2):
        ar, st, need = subsample_call(pts, cols, 8, 12345, seed)
        assert st == 0 and need > 0 and need % 256 == 0, _err()
        out = ar.check()
        assert np.array_equal(out["out_index"], ref)
        assert np.array_equal(_bits(out["out_points"]), _bits(pts[ref])) and np.array_equal(out["out_colors"], cols[ref])
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("out_points", "out_colors", "out_index"))
    ar, st, _ = subsample_call(pts[:7], cols[:7], 8, 1, 3)             # m == 0 does nothing
    assert st == 0
    ar.untouched()
    for name in ("points", "out_points", "out_index"):
        ar, st, _ = subsample_call(pts, cols, 8, 12345, 4, shift={name: 4})
        _refused(ar, st, name)
    ar, st, _ = subsample_call(pts, cols, 8, 12345, 4, shift={"ws": 128})
    _refused(ar, st, "ws")


def normals_call(depth, intr, c2w, seed, shift=None):
    lib = _lib()
    f, h, w = depth.shape
    ar = Arena(DEV, seed)
    ar.carve("depth", np.asarray(depth, F64), 8, "in")
    ar.carve("intrinsics", np.asarray(intr, F64), 8, "in")
    ar.carve("c2w", np.asarray(c2w, F64), 8, "in")
    ar.carve("normals", np.empty((f, h, w, 3), F64), 8, "out")
    q = _ptrs(ar, shift)
    st = lib.gg_depth_normals(f, h, w, q("depth"), q("intrinsics"), q("c2w"), q("normals"), _stream())
    return ar, st


def test_depth_normals():
    import prepare_ref
    rng = np.random.default_rng(3)
    f, h, w = 2, 13, 17
    d = 0.4 + 0.1 * rng.random((f, h, w))
    d[rng.random((f, h, w)) < 0.05] = 0.0
    d[0, 0, 0], d[0, -1, -1], d[-1, 0, -1], d[-1, -1, 0] = 0.00999, np.nan, np.inf, -np.inf
    intr = np.array([[385.86 + i, 385.38, w / 2, h / 2] for i in range(f)])
    c2w = np.array([prepare_ref.random_pose(rng) for _ in range(f)])
    ref = prepare_ref.normals(d, intr, c2w)
    runs = []
    for seed in (1, 2):
        ar, st = normals_call(d, intr, c2w, seed)
        assert st == 0, _err()
        out = ar.check()
        assert np.array_equal(_bits(out["normals"]), _bits(ref))
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("normals",))
    ar, st = normals_call(d[:0], intr[:0], c2w[:0], 3)                 # num_frames == 0 does nothing
    assert st == 0
    ar.untouched()
    for name in ("depth", "intrinsics", "c2w", "normals"):
        ar, st = normals_call(d, intr, c2w, 4, shift={name: 4})
        _refused(ar, st, name)


# ------------------------------------------------------------------------------------------------
# gg_cluster_dbscan, gg_cluster_stats
# ------------------------------------------------------------------------------------------------
def dbscan_call(p, active, eps, mp, grid, dims, seed, shift=None):
    lib = _lib()
    n = len(p)
    gc, dc = _grid_args(grid, dims)
    need = lib.gg_cluster_workspace(n, dc)
    ar = Arena(DEV, seed)
    ar.carve("points", np.asarray(p, F32), 4, "in")
    if active is not None:
        ar.carve("active", np.asarray(active, U8), 1, "in")
    ar.carve("labels", np.empty(n, I32), 4, "out")
    ar.carve("core", np.empty(n, U8), 1, "out")
    ar.carve("neighbor_count", np.empty(n, I32), 4, "out")
    ar.carve("num_clusters", np.empty(1, I32), 4, "out")
    ar.carve("ws", need, 256, "ws")
    q = _ptrs(ar, shift)
    st = lib.gg_cluster_dbscan(n, q("points"), q("active" if active is not None else None), float(eps), int(mp), gc,
                               dc, q("labels"), q("core"), q("neighbor_count"), q("num_clusters"), q("ws"), need,
                               _stream())
    return ar, st, need


def stats_call(p, w, labels, k, seed, shift=None):
    lib = _lib()
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, points=np.asarray(p, F32), weights=np.asarray(w, F32), labels=np.asarray(labels, I32))
    _carve(ar, "out", 8, count=np.empty(k, I64), weight=np.empty(k, F64), centroid=np.empty((k, 3), F64))
    ar.carve("bbox", np.empty((k, 6), F32), 4, "out")
    q = _ptrs(ar, shift)
    st = lib.gg_cluster_stats(len(p), q("points"), q("weights"), q("labels"), k, q("count"), q("weight"),
                              q("centroid"), q("bbox"), _stream())
    return ar, st


@pytest.mark.parametrize("n", [1, 257, 3000])
def test_cluster(n):
    import cluster_ref
    from gaussiangrasper_amd.grid import cluster_grid
    rng = np.random.default_rng(n)
    if n == 1:
        p, eps, mp = np.float32([[0.25, -0.5, 0.125]]), 0.03, 1
    else:
        p, eps, mp = cluster_ref.blobs(16, n), (0.03 if n == 3000 else 0.06), (5 if n == 3000 else 3)
    act = rng.random(n) < 0.7 if n > 1 else np.ones(1, bool)
    for active in (None, act.astype(U8) * 7):
        ref = cluster_ref.restate(p, eps, mp, None if active is None else act)
        grid, dims = cluster_grid(torch.from_numpy(p), eps, None if active is None else torch.from_numpy(act))
        runs = []
        for seed in (1, 2):
            ar, st, need = dbscan_call(p, active, eps, mp, grid, dims, seed)
            assert st == 0 and need > 0 and need % 256 == 0, _err()
            out = ar.check()
            assert np.array_equal(out["neighbor_count"], ref["neighbor_count"])
            assert np.array_equal(out["core"], np.asarray(ref["core"]).astype(U8))
            assert out["num_clusters"][0] == ref["num_clusters"]
            assert np.array_equal(out["labels"], ref["labels"])
            runs.append(out)
        _same_bytes(runs[0], runs[1], ("labels", "core", "neighbor_count", "num_clusters"))
        if n == 3000:
            assert ref["num_clusters"] > 1 and (ref["labels"] < 0).any()
    # statistics of the last labelling (the active subset)
    k = int(ref["num_clusters"])
    assert k >= 1
    w = rng.uniform(0.01, 1.0, n).astype(F32)
    rs = cluster_ref.restate_stats(p, w, ref["labels"], k)
    runs = []
    for seed in (1, 2):
        ar, st = stats_call(p, w, ref["labels"], k, seed)
        assert st == 0, _err()
        out = ar.check()
        assert np.array_equal(out["count"], rs["count"]) and np.array_equal(_bits(out["bbox"]), _bits(rs["bbox"].astype(F32)))
        assert (np.abs(out["weight"] - rs["weight"]) <= rs["weight_bound"]).all()
        assert (np.abs(out["centroid"] - rs["centroid"]) <= rs["centroid_bound"]).all()
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("count", "bbox"))
    # the empty calls: num_points == 0, num_clusters == 0
    ar, st, _ = dbscan_call(p[:0], None, eps, mp, grid, dims, 3)
    assert st == 0
    ar.untouched()
    ar, st = stats_call(p, w, ref["labels"], 0, 3)
    assert st == 0
    ar.untouched()
    if n == 257:
        for name in ("points", "labels", "neighbor_count", "num_clusters"):
            ar, st, _ = dbscan_call(p, active, eps, mp, grid, dims, 4, shift={name: 2})
            _refused(ar, st, name)
        ar, st, _ = dbscan_call(p, active, eps, mp, grid, dims, 4, shift={"ws": 128})
        _refused(ar, st, "ws")
        for name, step in (("points", 2), ("weights", 2), ("labels", 2), ("count", 4), ("weight", 4), ("centroid", 4),
                           ("bbox", 2)):
            ar, st = stats_call(p, w, ref["labels"], k, 4, shift={name: step})
            _refused(ar, st, name)


# ------------------------------------------------------------------------------------------------
# gg_cloud_frames, gg_icp_step
# ------------------------------------------------------------------------------------------------
def frames_call(pts, inten, radius, grid, dims, seed, shift=None, n=None):
    lib = _lib()
    n = len(pts) if n is None else n
    gc, dc = _grid_args(grid, dims)
    need = lib.gg_cloud_frames_workspace(len(pts), dc)
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, points=np.asarray(pts, F32), intensity=np.asarray(inten, F32))
    _carve(ar, "out", 4, normals=np.empty((len(pts), 3), F32), gradients=np.empty((len(pts), 3), F32),
           count=np.empty(len(pts), I32))
    ar.carve("valid", np.empty(len(pts), U8), 1, "out")
    ar.carve("ws", need, 256, "ws")
    q = _ptrs(ar, shift)
    st = lib.gg_cloud_frames(n, q("points"), q("intensity"), float(radius), gc, dc, q("normals"), q("gradients"),
                             q("count"), q("valid"), q("ws"), need, _stream())
    return ar, st, need


def step_call(S, Is, tgt, T, max_dist, lam, grid, dims, seed, extra=True, shift=None, m=None):
    lib = _lib()
    m = len(S) if m is None else m
    gc, dc = _grid_args(grid, dims)
    need = lib.gg_icp_step_workspace(len(S), len(tgt["points"]), dc)
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, source=np.asarray(S, F32), source_intensity=np.asarray(Is, F32),
           points=np.asarray(tgt["points"], F32), intensity=np.asarray(tgt["intensity"], F32),
           normals=np.asarray(tgt["normals"], F32), gradients=np.asarray(tgt["gradients"], F32))
    ar.carve("valid", np.asarray(tgt["valid"], U8), 1, "in")
    ar.carve("sums", np.empty(32, F64), 8, "out")
    if extra:
        ar.carve("abs_sums", np.empty(32, F64), 8, "out")
        ar.carve("corr", np.empty(len(S), I32), 4, "out")
    ar.carve("ws", need, 256, "ws")
    q = _ptrs(ar, shift)
    tf = (ctypes.c_double * 12)(*np.asarray(T, F64)[:3, :4].reshape(-1))
    st = lib.gg_icp_step(m, q("source"), q("source_intensity"), len(tgt["points"]), q("points"), q("intensity"),
                         q("normals"), q("gradients"), q("valid"), gc, dc, ctypes.cast(tf, P), float(max_dist),
                         float(lam), 0, q("sums"), q("abs_sums" if extra else None), q("corr" if extra else None),
                         q("ws"), need, _stream())
    return ar, st, need


@pytest.mark.parametrize("n", [257, 3000])
def test_registration(n):
    import register_ref as R
    from gaussiangrasper_amd.grid import cluster_grid
    radius, max_dist, lam = (0.05, 0.03, 0.968) if n == 257 else (0.02, 0.01, 0.968)
    pts, inten = R.surface(n, 1)
    rn, rg, rc, rv, gap = R.cloud_frames(pts, inten, radius)
    grid, dims = cluster_grid(torch.from_numpy(pts.astype(F32)), radius)
    clear = rv & (gap >= 1e-2)
    assert rv.sum() > n // 2 and (rv & ~clear).sum() <= 0.01 * n
    size = np.linalg.norm(rg, axis=1)
    bound = 1e-5 * size + 1e-6 * size.max(initial=0.0)
    runs = []
    for seed in (1, 2):
        ar, st, need = frames_call(pts, inten, radius, grid, dims, seed)
        assert st == 0 and need > 0 and need % 256 == 0, _err()
        out = ar.check()
        nrm, grad = out["normals"].astype(F64), out["gradients"].astype(F64)
        assert np.array_equal(out["count"], rc) and np.array_equal(out["valid"], rv.astype(U8))
        assert np.isnan(nrm[~rv]).all() and (grad[~rv] == 0).all()
        assert np.allclose(np.linalg.norm(nrm[rv], axis=1), 1.0, rtol=0, atol=1e-6)
        assert np.abs(nrm[clear] - rn[clear]).max(initial=0.0) <= 1e-6
        assert (np.abs(grad - rg).max(axis=1)[clear] <= bound[clear]).all()
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("count", "valid"))
    ar, st, _ = frames_call(pts, inten, radius, grid, dims, 3, n=0)     # num_points >= 1 is the contract
    _refused(ar, st, "num_points")
    if n == 257:
        for name in ("points", "intensity", "normals", "gradients", "count"):
            ar, st, _ = frames_call(pts, inten, radius, grid, dims, 4, shift={name: 2})
            _refused(ar, st, name)
        ar, st, _ = frames_call(pts, inten, radius, grid, dims, 4, shift={"ws": 128})
        _refused(ar, st, "ws")

    # one linearisation against this target, with the restatement's frames rounded to fp32
    _, _, S, Is = R.scene()
    S, Is = S[:300], Is[:300]
    tgt = dict(points=R.f32(pts), intensity=R.f32(inten), normals=R.f32(rn), gradients=R.f32(rg), valid=rv)
    T = R.TRUE_MOTION @ R.rigid([0.004, -0.003, 0.006], [0.0012, -0.0008, 0.0006])
    rs, ra, rcorr = R.icp_sums(S, Is, tgt["points"], tgt["intensity"], tgt["normals"], tgt["gradients"], rv, T,
                               max_dist, lam)
    assert (rcorr >= 0).sum() > 30
    sgrid, sdims = cluster_grid(torch.from_numpy(tgt["points"].astype(F32)), max_dist)
    runs = {True: [], False: []}
    for extra in (True, False):
        for seed in (1, 2):
            ar, st, need = step_call(S, Is, tgt, T, max_dist, lam, sgrid, sdims, seed, extra)
            assert st == 0 and need > 0 and need % 256 == 0, _err()
            out = ar.check()
            sums = out["sums"]
            asum = out["abs_sums"] if extra else ra
            b = len(S) * 2.0 ** -52 * asum
            assert sums[27] == rs[27] == (rcorr >= 0).sum() and sums[31] == 0
            assert (np.abs(sums - rs) <= b).all()
            if extra:
                assert np.array_equal(out["corr"], rcorr) and (np.abs(asum - ra) <= b).all()
            runs[extra].append(out)
    _same_bytes(runs[True][0], runs[True][1], ("sums", "abs_sums", "corr"))
    _same_bytes(runs[False][0], runs[False][1], ("sums",))
    ar, st, _ = step_call(S, Is, tgt, T, max_dist, lam, sgrid, sdims, 3, m=0)   # num_source >= 1 is the contract
    _refused(ar, st, "num_source")
    if n == 257:
        for name, step in (("source", 2), ("source_intensity", 2), ("points", 2), ("intensity", 2), ("normals", 2),
                           ("gradients", 2), ("corr", 2), ("sums", 4), ("abs_sums", 4)):
            ar, st, _ = step_call(S, Is, tgt, T, max_dist, lam, sgrid, sdims, 4, shift={name: step})
            _refused(ar, st, name)
        ar, st, _ = step_call(S, Is, tgt, T, max_dist, lam, sgrid, sdims, 4, shift={"ws": 128})
        _refused(ar, st, "ws")


# ------------------------------------------------------------------------------------------------
# gg_tsdf_integrate, gg_tsdf_mesh_count, gg_tsdf_mesh_emit
# ------------------------------------------------------------------------------------------------
TSDF_BOX = ((-0.7, -0.65, -0.6), (0.7, 0.6, 0.6))
TSDF_TRUNC = 0.5


def tsdf_frames(seed, views=3, H=24, W=32):
    """depth of a sphere from three cameras around it, with misses (+inf), 0 and NaN pixels, and colour"""
    import tsdf_ref as R
    rng = np.random.default_rng(seed)
    E = R.sphere_cameras(views, 1.1)
    K = np.array([[25.0 + 1.5 * v, 26.0 - 0.5 * v, 15.7, 12.2] for v in range(views)])
    depth = np.stack([R.raycast_spheres(E[v], K[v], H, W, [((0.05, -0.02, 0.0), 0.45)]) for v in range(views)])
    depth[rng.random(depth.shape) < 0.03] = 0.0
    depth[rng.random(depth.shape) < 0.03] = np.nan
    rgb = rng.random(depth.shape + (3,)).astype(F32)
    return depth.astype(F32), K.astype(F32), np.asarray(E, F64).astype(F32), rgb


def tsdf_grid(dims):
    lo, hi = (np.asarray(a, F64) for a in TSDF_BOX)
    return np.concatenate([lo.astype(F32), ((hi - lo) / np.asarray(dims)).astype(F32)]).astype(F32)


def _host(a, ctype):
    return (ctype * len(a))(*[a_.item() for a_ in np.asarray(a).reshape(-1)])


def integrate_call(dims, grid, vol, depth, K, E, rgb, seed, shift=None, views=None):
    lib = _lib()
    V, H, W = depth.shape
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, depth=depth, rgb=rgb, intrinsics=K, w2c=E)
    _carve(ar, "inout", 4, tsdf=vol["tsdf"], weight=vol["weight"], color=vol.get("color"),
           color_weight=vol.get("color_weight"))
    q = _ptrs(ar, shift)
    c = rgb is not None
    st = lib.gg_tsdf_integrate(_host(dims, ctypes.c_int32), _host(grid, ctypes.c_float), TSDF_TRUNC,
                               V if views is None else views, H, W, q("depth"), q("rgb" if c else None),
                               q("intrinsics"), q("w2c"), q("tsdf"), q("weight"), q("color" if c else None),
                               q("color_weight" if c else None), _stream())
    return ar, st


def mesh_arena(dims, vol, color, nv, nf, seed):
    lib = _lib()
    need = lib.gg_tsdf_mesh_workspace(_host(dims, ctypes.c_int32))
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, tsdf=vol["tsdf"], weight=vol["weight"], color=vol["color"] if color else None)
    ar.carve("counts", np.empty(2, I64), 8, "out")
    for tag, v, f in (("", nv, nf), ("_short", max(nv - 1, 0), max(nf - 1, 0))):
        _carve(ar, "out", 4, **{"vertices" + tag: np.empty((v, 3), F32), "normals" + tag: np.empty((v, 3), F32),
                                "faces" + tag: np.empty((f, 3), I32)})
        if color:
            ar.carve("colors" + tag, np.empty((v, 3), F32), 4, "out")
    ar.carve("ws", need, 256, "ws")
    return ar, need


def count_call(ar, need, dims, shift=None):
    q = _ptrs(ar, shift)
    return _lib().gg_tsdf_mesh_count(_host(dims, ctypes.c_int32), q("tsdf"), q("weight"), q("counts"), q("ws"), need,
                                     _stream())


def emit_call(ar, need, dims, grid, color, nv, nf, tag="", shift=None):
    q = _ptrs(ar, shift)
    return _lib().gg_tsdf_mesh_emit(_host(dims, ctypes.c_int32), _host(grid, ctypes.c_float), q("tsdf"),
                                    q("color" if color else None), nv, nf, q("vertices" + tag), q("normals" + tag),
                                    q("colors" + tag if color else None), q("faces" + tag), q("ws"), need, _stream())


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("dims", [(5, 9, 11), (9, 17, 13)])
def test_tsdf(dims, color):
    import tsdf_ref as R
    depth, K, E, rgb = tsdf_frames(dims[0])
    if not color:
        rgb = None
    grid = tsdf_grid(dims)
    keys = ("tsdf", "weight") + (("color", "color_weight") if color else ())
    ref = R.integrate(R.new_volume(dims, color), dims, grid, TSDF_TRUNC, depth, K, E, rgb)
    assert (ref["weight"] == 0).any() and (ref["weight"] > 0).any()
    runs = []
    for seed in (1, 2):
        ar, st = integrate_call(dims, grid, R.new_volume(dims, color), depth, K, E, rgb, seed)
        assert st == 0, _err()
        out = ar.check()
        for k in keys:
            assert np.array_equal(_bits(out[k]), _bits(ref[k].reshape(out[k].shape))), k
        runs.append(out)
    _same_bytes(runs[0], runs[1], keys)
    ar, st = integrate_call(dims, grid, R.new_volume(dims, color), depth, K, E, rgb, 3, views=0)   # num_views == 0
    assert st == 0
    ar.untouched()
    if dims[0] == 5:
        for name in ("depth", "intrinsics", "w2c", "tsdf", "weight") + (("rgb", "color", "color_weight") if color else ()):
            ar, st = integrate_call(dims, grid, R.new_volume(dims, color), depth, K, E, rgb, 4, shift={name: 2})
            _refused(ar, st, name)

    # the mesh of that volume: capacities exactly the counts
    v, nr, c, f = R.extract(dims, grid, ref["tsdf"], ref["weight"], ref["color"] if color else None)
    nv, nf = len(v), len(f)
    assert nv > 8 and nf > 8
    runs = []
    for seed in (1, 2):
        ar, need = mesh_arena(dims, ref, color, nv, nf, seed)
        assert need > 0 and need % 256 == 0
        assert count_call(ar, need, dims) == 0, _err()
        out = ar.check()
        assert out["counts"].tolist() == [nv, nf]
        ws_after_count = out["ws"].copy()
        ar.rebase()
        assert emit_call(ar, need, dims, grid, color, nv, nf) == 0, _err()
        out = ar.check()
        assert out["ws"].tobytes() == ws_after_count.tobytes()                    # emit only reads it
        assert np.array_equal(_bits(out["vertices"]), _bits(v)) and np.array_equal(_bits(out["normals"]), _bits(nr))
        assert np.array_equal(out["faces"], f)
        if color:
            assert np.array_equal(_bits(out["colors"]), _bits(c))
        for k in out:
            if k.endswith("_short"):
                assert _is_sentinel(ar, k, out[k]), k
        # capacities one less: one row less is written, the rows before it are the same
        ar.rebase()
        assert emit_call(ar, need, dims, grid, color, nv - 1, nf - 1, "_short") == 0, _err()
        short = ar.check()
        for k in ("vertices", "normals", "faces") + (("colors",) if color else ()):
            assert short[k].tobytes() == out[k].tobytes(), k
            rows = (nf if k == "faces" else nv) - 1
            assert short[k + "_short"].tobytes() == out[k][:rows].tobytes(), k
        # capacities 0: nothing is launched
        ar.rebase()
        assert emit_call(ar, need, dims, grid, color, 0, 0) == 0, _err()
        ar.untouched()
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("counts", "vertices", "normals", "faces") + (("colors",) if color else ()))
    if dims[0] == 5:
        ar, need = mesh_arena(dims, ref, color, nv, nf, 4)
        for name, step in (("tsdf", 2), ("weight", 2), ("counts", 4), ("ws", 128)):
            _refused(ar, count_call(ar, need, dims, shift={name: step}), name)
        for name in ("tsdf", "vertices", "normals", "faces") + (("color", "colors") if color else ()):
            _refused(ar, emit_call(ar, need, dims, grid, color, nv, nf, shift={name: 2}), name)
        _refused(ar, emit_call(ar, need, dims, grid, color, nv, nf, shift={"ws": 128}), "ws")


# ------------------------------------------------------------------------------------------------
# gg_object_masks
# ------------------------------------------------------------------------------------------------
def objmask_call(pts, T, intr, w2c, h, w, k, mask_align, seed, shift=None, views=None, max_rows=4096):
    lib = _lib()
    V = len(intr)
    need = lib.gg_object_masks_workspace(V, max_rows)
    ar = Arena(DEV, seed)
    _carve(ar, "in", 8, points=np.asarray(pts, F64), intrinsics=np.asarray(intr, F64),
           w2c=np.asarray(w2c, F64)[:, :3, :4])
    _carve(ar, "out", mask_align, before=np.empty((V, h, w), U8), after=np.empty((V, h, w), U8),
           union_mask=np.empty((V, h, w), U8))
    ar.carve("boxes", np.empty((V, 3, 4), I32), 4, "out")
    ar.carve("centres", np.empty((V, 3, 2), F64), 8, "out")
    ar.carve("dropped", np.empty((V, 2), I32), 4, "out")
    ar.carve("ws", need, 256, "ws")
    q = _ptrs(ar, shift)
    tf = (ctypes.c_double * 12)(*np.asarray(T, F64)[:3, :4].reshape(-1))
    st = lib.gg_object_masks(len(pts), q("points"), ctypes.cast(tf, P), V if views is None else views,
                             q("intrinsics"), q("w2c"), h, w, k, max_rows, q("before"), q("after"), q("union_mask"),
                             q("boxes"), q("centres"), q("dropped"), q("ws"), need, _stream())
    return ar, st, need


OBJMASK_OUTS = ("before", "after", "union_mask", "boxes", "centres", "dropped")


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("h,w,mask_align", [(24, 32, 1), (24, 32, 4), (23, 29, 1)])
def test_object_masks(h, w, mask_align, k):
    import objmask_ref as R
    import test_objmask_gpu as G
    rng = np.random.default_rng(10 + k)
    pts = G._blob(rng, 400)
    T = G._motion()
    intr, w2c = G._cams(3, h, w, seed=k)
    ref = R.object_masks(pts, T, intr, w2c, h, w, k)
    assert ref["union"].any() and not ref["union"].all()
    runs = []
    for seed in (1, 2):
        ar, st, need = objmask_call(pts, T, intr, w2c, h, w, k, mask_align, seed)
        assert st == 0 and need > 0 and need % 256 == 0, _err()
        for name in ("before", "after", "union_mask"):          # the byte branch and the word branch of the writer
            assert ar.address(name) % (2 * mask_align) == mask_align
        out = ar.check()
        for name, r in (("before", "before"), ("after", "after"), ("union_mask", "union")):
            assert np.array_equal(out[name], ref[r].astype(U8)), name
        assert np.array_equal(out["boxes"], ref["boxes"]) and np.array_equal(out["dropped"], ref["dropped"])
        c = out["centres"]
        assert np.array_equal(np.isnan(c), np.isnan(ref["centres"]))
        assert np.array_equal(np.nan_to_num(c, nan=-7.0), np.nan_to_num(ref["centres"], nan=-7.0))
        runs.append(out)
    _same_bytes(runs[0], runs[1], OBJMASK_OUTS)
    ar, st, _ = objmask_call(pts, T, intr[:0], w2c[:0], h, w, k, mask_align, 3)     # num_views == 0 does nothing
    assert st == 0, _err()
    ar.untouched()
    if (h, mask_align, k) == (24, 1, 0):
        for name, step in (("points", 4), ("intrinsics", 4), ("w2c", 4), ("centres", 4), ("boxes", 2), ("dropped", 2),
                           ("ws", 128)):
            ar, st, _ = objmask_call(pts, T, intr, w2c, h, w, k, mask_align, 4, shift={name: step})
            _refused(ar, st, name)


# ------------------------------------------------------------------------------------------------
# gg_hull_edit
# ------------------------------------------------------------------------------------------------
def hull_call(means, quats, planes, rt, seed, shift=None, tol=0.0):
    lib = _lib()
    n = len(means)
    ar = Arena(DEV, seed)
    ar.carve("means", np.asarray(means, F32), 4, "inout")
    ar.carve("quats", np.asarray(quats, F32), 16, "inout")
    ar.carve("planes", np.asarray(planes, F64), 8, "in")
    ar.carve("mask", np.empty(n, U8), 1, "out")
    ar.carve("count_out", np.empty(1, I64), 8, "out")
    q = _ptrs(ar, shift)
    r = None if rt is None else ctypes.cast((ctypes.c_float * 12)(*np.asarray(rt, F32).reshape(-1)), P)
    st = lib.gg_hull_edit(n, q("means"), q("quats"), len(planes), q("planes"), tol, r, q("mask"), q("count_out"),
                          _stream())
    return ar, st


@pytest.mark.parametrize("n", [1, 257, 1025])
def test_hull_edit(n):
    import test_scene_edit_gpu as G
    from gaussiangrasper_amd import ops
    planes = G.sphere_planes(12, 0.6, 1)
    means, quats = (t.numpy() for t in G.cloud(n, seed=n + 7))
    means[0] = 0.0                                                     # inside
    if n >= 257:
        means[5], means[6, 1] = np.nan, np.inf
    rt = G.random_rt(12)
    sel = G.mask_ref(means, planes, 0.0).astype(bool)
    assert sel[0] and (n == 1 or 0 < sel.sum() < n)
    rq = ops.quat_to_rotmat(torch.from_numpy(quats).to(DEV)).detach().cpu().numpy().reshape(-1, 9)
    want_m, want_q = means.copy(), quats.copy()
    want_m[sel] = G.f32_move_means(means[sel], rt)
    want_q[sel] = G.f32_shepperd(G.f32_product(rt, rq[sel]))[0]
    runs = []
    for seed in (1, 2):
        ar, st = hull_call(means, quats, planes, rt, seed)
        assert st == 0, _err()
        assert ar.address("quats") % 32 == 16 and ar.address("mask") % 2 == 1
        out = ar.check()
        assert np.array_equal(out["mask"], sel.astype(U8)) and out["count_out"][0] == sel.sum()
        # selected rows: the stated arithmetic; rows not selected: never written, NaN rows included
        assert np.array_equal(_bits(out["means"]), _bits(want_m)) and np.array_equal(_bits(out["quats"]), _bits(want_q))
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("means", "quats", "mask", "count_out"))
    # select only: means and quats are inputs
    ar, st = hull_call(means, quats, planes, None, 3)
    assert st == 0, _err()
    out = ar.check()
    assert np.array_equal(out["mask"], sel.astype(U8)) and out["count_out"][0] == sel.sum()
    assert np.array_equal(_bits(out["means"]), _bits(means)) and np.array_equal(_bits(out["quats"]), _bits(quats))
    # num_points == 0 zeroes the count and writes nothing else
    ar, st = hull_call(means[:0], quats[:0], planes, rt, 3)
    assert st == 0, _err()
    assert ar.check()["count_out"][0] == 0
    if n == 257:
        for name, step in (("count_out", 4), ("quats", 8), ("means", 2), ("planes", 4)):
            ar, st = hull_call(means, quats, planes, rt, 4, shift={name: step})
            _refused(ar, st, name)


# ------------------------------------------------------------------------------------------------
# gg_clip_query
# ------------------------------------------------------------------------------------------------
def clip_call(x, w, qn, n_pos, tau, seed, shift=None):
    lib = _lib()
    rows, d = x.shape
    c, nq = w[2].shape[0], len(qn)
    need = lib.gg_clip_query_workspace(d, 128, c, nq)
    ar = Arena(DEV, seed)
    ar.carve("x", np.asarray(x, F32), 16, "in")
    _carve(ar, "in", 4, w1=w[0], b1=w[1], w2=w[2], b2=w[3], queries=np.asarray(qn, F32))
    _carve(ar, "out", 4, sims=np.empty((rows, nq), F32), relevancy=np.empty((rows, n_pos), F32))
    ar.carve("ws", need, 16, "ws")
    q = _ptrs(ar, shift)
    st = lib.gg_clip_query(rows, d, 128, c, q("x"), q("w1"), q("b1"), q("w2"), q("b2"), nq, n_pos, q("queries"), tau,
                           q("sims"), q("relevancy"), q("ws"), need, _stream())
    return ar, st, need


@pytest.mark.parametrize("rows", [1, 65, 300])
def test_clip_query(rows):
    import test_clip_query_gpu as G
    w = G.make_mlp(32, 96, seed=32 + 96)
    g = torch.Generator().manual_seed(7 + rows)
    x = torch.randn(rows, 32, generator=g)
    qs = torch.randn(3, 96, generator=g)
    qn = (qs / qs.norm(dim=1, keepdim=True)).contiguous()
    wn = [t.numpy() for t in w]
    ref_s = G.ref_sims(x, w, qs)
    ref_r = G.ref_rel(ref_s, 1, 10.0)
    runs = []
    for seed in (1, 2):
        ar, st, need = clip_call(x.numpy(), wn, qn.numpy(), 1, 10.0, seed)
        assert st == 0 and need > 0, _err()
        assert ar.address("x") % 32 == 16 and all(ar.address(k) % 8 == 4 for k in ("w1", "b1", "w2", "b2", "queries"))
        out = ar.check()
        assert np.abs(out["sims"].astype(F64) - ref_s).max() <= 2e-5
        assert np.abs(out["relevancy"].astype(F64) - ref_r).max() <= 1e-4
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("sims", "relevancy"))
    ar, st, _ = clip_call(x.numpy()[:0], wn, qn.numpy(), 1, 10.0, 3)   # num_rows == 0 does nothing
    assert st == 0
    ar.untouched()
    if rows == 65:
        for name, step in (("x", 8), ("w1", 2), ("b1", 2), ("w2", 2), ("b2", 2), ("queries", 2), ("sims", 2),
                           ("relevancy", 2)):
            ar, st, _ = clip_call(x.numpy(), wn, qn.numpy(), 1, 10.0, 4, shift={name: step})
            _refused(ar, st, name)
        ar, st, _ = clip_call(x.numpy(), wn, qn.numpy(), 1, 10.0, 4, shift={"ws": 8})
        _refused(ar, st, "workspace")


# ------------------------------------------------------------------------------------------------
# gg_image_loss_fwd / bwd, gg_geom_loss_fwd / bwd
# ------------------------------------------------------------------------------------------------
def image_arena(rgb, gt, valid, stride, seed):
    lib = _lib()
    h, w = gt.shape[:2]
    need = lib.gg_image_loss_workspace(h, w)
    wide = np.full((h, w, stride), 0.25, F32)
    wide[..., :3] = rgb
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, rgb=wide, gt=np.asarray(gt, F32), v_main=np.array([1.7], F32))
    if valid is not None:
        ar.carve("valid", np.asarray(valid, U8), 1, "in")
    _carve(ar, "out", 4, out3=np.empty(3, F32), v_rgb=np.empty((h, w, 3), F32))
    ar.carve("ws", need, 256, "ws")
    return ar, need


def image_fwd(ar, need, h, w, stride, valid, lam, shift=None):
    q = _ptrs(ar, shift)
    return _lib().gg_image_loss_fwd(h, w, q("rgb"), stride, q("gt"), q("valid" if valid is not None else None), lam,
                                    q("out3"), q("ws"), need, _stream())


def image_bwd(ar, need, h, w, stride, valid, lam, shift=None):
    q = _ptrs(ar, shift)
    return _lib().gg_image_loss_bwd(h, w, q("rgb"), stride, q("gt"), q("valid" if valid is not None else None), lam,
                                    q("v_main"), q("ws"), need, q("v_rgb"), _stream())


@pytest.mark.parametrize("h,w,masked,stride", [(11, 11, False, 3), (27, 16, True, 7)])
def test_image_loss(oracle, h, w, masked, stride):
    import test_image_loss as G
    rgb, gt, valid = G._images(h, w, 9, F32, masked)
    lam = 0.2
    ref = oracle.image_loss_fwd(rgb, gt, valid, lam)
    v_ref = oracle.image_loss_bwd(rgb, gt, valid, lam, 1.7)
    runs = []
    for seed in (1, 2):
        ar, need = image_arena(rgb, gt, valid, stride, seed)
        assert need > 0 and need % 256 == 0
        assert image_fwd(ar, need, h, w, stride, valid, lam) == 0, _err()
        out = ar.check()                                       # rgb and gt are inputs: unchanged
        np.testing.assert_allclose(out["out3"], ref, rtol=2e-6, atol=1e-7)
        assert _is_sentinel(ar, "v_rgb", out["v_rgb"])
        ws_fwd = out["ws"].copy()
        ar.rebase()
        assert image_bwd(ar, need, h, w, stride, valid, lam) == 0, _err()
        out = ar.check()
        assert out["ws"].tobytes() == ws_fwd.tobytes()         # the backward reads the forward's workspace in place
        assert np.array_equal(_bits(out["v_rgb"]), _bits(np.asarray(v_ref, F32).reshape(h, w, 3)))
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("out3", "v_rgb"))
    if masked:
        ar, need = image_arena(rgb, gt, valid, stride, 4)
        for name, step in (("rgb", 2), ("gt", 2), ("out3", 2), ("ws", 128)):
            _refused(ar, image_fwd(ar, need, h, w, stride, valid, lam, shift={name: step}), name)
        for name, step in (("rgb", 2), ("gt", 2), ("v_main", 2), ("v_rgb", 2), ("ws", 128)):
            _refused(ar, image_bwd(ar, need, h, w, stride, valid, lam, shift={name: step}), name)


def geom_arena(depth, gt_depth, normal, gt_normal, mask, seed):
    """the plugin route's layout: depth and normal are channels 3 and 4..6 of one (H, W, 7) image, the ground-truth
    normal is channel-major"""
    lib = _lib()
    h, w = gt_depth.shape
    need = lib.gg_geom_loss_workspace()
    tail = np.full((h, w, 7), -3.0, F32)
    tail[..., 3:4], tail[..., 4:7] = depth, normal
    ar = Arena(DEV, seed)
    _carve(ar, "in", 4, tail=tail, gt_depth=np.asarray(gt_depth, F32), gt_normal=np.asarray(gt_normal, F32),
           v_depth_loss=np.array([1.3], F32), v_normal_loss=np.array([0.7], F32))
    ar.carve("mask", np.asarray(mask, U8), 1, "in")
    _carve(ar, "out", 4, out3=np.empty(3, F32), v_depth=np.empty(h * w, F32), v_normal=np.empty((h * w, 3), F32))
    ar.carve("ws", need, 256, "ws")
    return ar, need


def geom_fwd(ar, need, hw, shift=None):
    """shift: region names, and "depth" / "normal" for the two pointers into the (H, W, 7) image"""
    q, s = _ptrs(ar, shift), shift or {}
    return _lib().gg_geom_loss_fwd(hw, q("tail", 12 + s.get("depth", 0)), 7, q("gt_depth"), 1,
                                   q("tail", 16 + s.get("normal", 0)), 7, 1, q("gt_normal"), 1, hw, q("mask"),
                                   q("out3"), q("ws"), need, _stream())


def geom_bwd(ar, need, hw, shift=None):
    q, s = _ptrs(ar, shift), shift or {}
    return _lib().gg_geom_loss_bwd(hw, q("tail", 12 + s.get("depth", 0)), 7, q("gt_depth"), 1,
                                   q("tail", 16 + s.get("normal", 0)), 7, 1, q("gt_normal"), 1, hw, q("mask"),
                                   q("v_depth_loss"), q("v_normal_loss"), q("ws"), need, q("v_depth"), q("v_normal"),
                                   _stream())


def test_geom_loss(oracle):
    import test_image_loss as G
    h, w = 23, 31
    depth, gt_depth, normal, gt_normal, mask = G._geom_inputs(h, w, 4)
    ref = oracle.geom_loss_fwd(depth, gt_depth, normal, gt_normal, mask)
    vd, vn = oracle.geom_loss_bwd(depth, gt_depth, normal, gt_normal, mask, 1.3, 0.7)
    runs = []
    for seed in (1, 2):
        ar, need = geom_arena(depth, gt_depth, normal, gt_normal, mask, seed)
        assert need > 0
        assert geom_fwd(ar, need, h * w) == 0, _err()
        out = ar.check()
        np.testing.assert_allclose(out["out3"][:2], ref[:2], rtol=2e-6, atol=1e-7)
        assert out["out3"][2] == mask.sum()
        ws_fwd = out["ws"].copy()
        ar.rebase()
        assert geom_bwd(ar, need, h * w) == 0, _err()
        out = ar.check()
        assert out["ws"].tobytes() == ws_fwd.tobytes()
        assert np.array_equal(_bits(out["v_depth"]), _bits(np.asarray(vd, F32).reshape(-1)))
        assert np.array_equal(_bits(out["v_normal"]), _bits(np.asarray(vn, F32).reshape(-1, 3)))
        runs.append(out)
    _same_bytes(runs[0], runs[1], ("out3", "v_depth", "v_normal"))
    ar, need = geom_arena(depth, gt_depth, normal, gt_normal, mask, 4)
    for name in ("depth", "gt_depth", "normal", "gt_normal", "out3", "ws"):
        _refused(ar, geom_fwd(ar, need, h * w, shift={name: 128 if name == "ws" else 2}), name)
    for name in ("depth", "gt_depth", "normal", "gt_normal", "v_depth_loss", "v_normal_loss", "v_depth", "v_normal",
                 "ws"):
        _refused(ar, geom_bwd(ar, need, h * w, shift={name: 128 if name == "ws" else 2}), name)
