"""GPU checks of scene preparation (gaussiangrasper_amd.prepare on gg_backproject, gg_subsample, gg_depth_normals and
gg_knn): bit-exact against the host restatements of tests/prepare_ref.py — back-projection with holes, NaN, inf and
pixels exactly on every window bound, in any batching; the subsample law; normal maps with edges, clamped and
non-finite depths on non-square frames; kNN distances on uniform, clustered, tied, duplicated, outlier, identical,
planar and minimal clouds, every index reproducing its distance; a worst-case time guard; the plugin's device kNN;
and the command-line tool end to end, twice, byte for byte."""
import ctypes
import functools
import os
import time

import numpy as np
import pytest
import torch

import prepare_ref as R

gpu = pytest.mark.gpu


def _frames(seed, f=4, h=37, w=53):
    rng = np.random.default_rng(seed)
    depth = 0.5 + 0.1 * rng.normal(size=(f, h, w))
    depth[rng.random((f, h, w)) < 0.05] = 0.0
    depth[0, 1, 2], depth[1, 3, 4], depth[2, 5, 6] = np.nan, np.inf, -np.inf
    mask = (rng.random((f, h, w)) > 0.1).astype(np.uint8) * rng.integers(1, 256, (f, h, w)).astype(np.uint8)
    rgb = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
    intr = np.array([[0.9 * w + i, 0.85 * w, w / 2 - 0.3, h / 2 + 0.2] for i in range(f)])
    T = np.array([np.eye(4)] * f)
    for i in range(f):
        T[i, :3, :3] = R.rodrigues(rng.normal(size=3) * 0.3) @ np.diag([1.0, -1.0, -1.0])
        T[i, :3, 3] = [0.02 * i, -0.02, 0.3]
    # pixels whose base-frame z lands exactly on z_lo / z_hi: with this axis-aligned pose z = -d exactly
    T[3, :3, :3] = np.diag([1.0, -1.0, -1.0])
    T[3, :3, 3] = [0.01, -0.01, 0.0]
    depth[3, 0, 0:4] = [0.3, 0.1, np.nextafter(0.3, 0.0), np.nextafter(0.1, 1.0)]   # on the bounds, just inside
    mask[3, 0, 0:4] = 1
    assert (((T[3, 2, 2] * depth[3, 0, :2]) + T[3, 2, 3]) == np.array([-0.3, -0.1])).all()
    return depth, mask, rgb, intr, T


def _bits(a, dt=np.uint64):
    return np.ascontiguousarray(a).view(dt)


@gpu
def test_backprojection_bit_exact_and_batch_invariant():
    from gaussiangrasper_amd.prepare import backproject_frames
    depth, mask, rgb, intr, T = _frames(0)
    rp, rc = R.backproject(depth, mask, rgb, intr, T)
    assert 0 < rp.shape[0] < depth.size
    for batch in (1, 3, 4):
        ps, cs = [], []
        for b in range(0, 4, batch):
            p, c = backproject_frames(depth[b:b + batch], mask[b:b + batch], rgb[b:b + batch], intr[b:b + batch],
                                      T[b:b + batch])
            ps.append(p.cpu().numpy())
            cs.append(c.cpu().numpy())
        p, c = np.concatenate(ps), np.concatenate(cs)
        assert p.shape == rp.shape, batch
        assert np.array_equal(_bits(p), _bits(rp)) and np.array_equal(c, rc), batch
    # the z window is strict
    p3, _ = R.backproject(depth[3:], mask[3:], rgb[3:], intr[3:], T[3:])
    assert not np.isin(p3[:, 2], [-0.3, -0.1]).any()
    assert np.isin([-np.nextafter(0.3, 0.0), -np.nextafter(0.1, 1.0)], p3[:, 2]).all()


@gpu
def test_backprojection_depth_bounds_are_strict():
    """Pixels exactly on d_lo / d_hi, and one step inside, on the axis-aligned frame (z = -d) with a depth range
    inside the z window, so that only the depth test decides them."""
    from gaussiangrasper_amd.prepare import backproject_frames
    depth, mask, rgb, intr, T = _frames(0)
    depth, mask, rgb, intr, T = depth[3:], mask[3:], rgb[3:], intr[3:], T[3:]
    lo, hi = 0.15, 0.25
    inside = [np.nextafter(lo, 1.0), np.nextafter(hi, 0.0)]
    depth[0, 1, 0:4] = [lo, hi] + inside
    mask[0, 1, 0:4] = 1
    rp, rc = R.backproject(depth, mask, rgb, intr, T, d_lo=lo, d_hi=hi)
    assert not np.isin(rp[:, 2], [-lo, -hi]).any() and np.isin(-np.array(inside), rp[:, 2]).all()
    # inclusive bounds would keep two more rows: the pin is not vacuous
    wide, _ = R.backproject(depth, mask, rgb, intr, T, d_lo=np.nextafter(lo, 0.0), d_hi=np.nextafter(hi, 1.0))
    assert wide.shape[0] == rp.shape[0] + 2
    p, c = backproject_frames(depth, mask, rgb, intr, T, depth_range=(lo, hi))
    p, c = p.cpu().numpy(), c.cpu().numpy()
    assert p.shape == rp.shape and np.array_equal(_bits(p), _bits(rp)) and np.array_equal(c, rc)


@gpu
def test_backprojection_empty_gives_zero_rows():
    from gaussiangrasper_amd.prepare import backproject_frames
    depth, mask, rgb, intr, T = _frames(1)
    p, c = backproject_frames(depth, np.zeros_like(mask), rgb, intr, T)
    assert tuple(p.shape) == (0, 3) and tuple(c.shape) == (0, 3)
    p, c = backproject_frames(depth, mask, rgb, intr, T, z_range=(5.0, 6.0))
    assert p.shape[0] == 0


@gpu
def test_subsample_is_the_host_law_and_repeatable():
    from gaussiangrasper_amd.prepare import subsample, subsample_device_indices, subsample_indices
    rng = np.random.default_rng(2)
    for num, keep, seed in ((100003, 8, 0), (5000, 1, 3), (7, 8, 1), (8, 8, 2), (2_000_001, 8, 12345)):
        pts = torch.from_numpy(rng.normal(size=(num, 3))).cuda()
        cols = torch.from_numpy(rng.integers(0, 256, (num, 3), dtype=np.uint8)).cuda()
        a = subsample(pts, cols, keep, seed)
        b = subsample(pts, cols, keep, seed)
        ref = subsample_indices(num, keep, seed)
        ia = a[2].cpu().numpy()
        assert np.array_equal(ia, ref), (num, keep)
        assert np.array_equal(ia, b[2].cpu().numpy())
        assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(pts.cpu().numpy()[ref]))
        assert np.array_equal(a[1].cpu().numpy(), cols.cpu().numpy()[ref])
        assert np.array_equal(subsample_device_indices(num, keep, seed).cpu().numpy(), ref)


@gpu
def test_normals_bit_exact():
    from gaussiangrasper_amd.prepare import depth_normals
    rng = np.random.default_rng(3)
    for f, h, w in ((2, 37, 53), (1, 2, 2), (1, 2, 9), (3, 11, 3), (1, 480, 640)):
        d = 0.4 + 0.1 * rng.random((f, h, w))
        d[rng.random((f, h, w)) < 0.05] = 0.0             # clamped to 1e-5
        d[0, 0, 0] = 0.00999
        d[0, -1, -1] = np.nan
        d[-1, 0, -1] = np.inf
        d[-1, -1, 0] = -np.inf
        intr = np.array([[385.86 + i, 385.38, w / 2, h / 2] for i in range(f)])
        T = np.array([R.random_pose(rng) for _ in range(f)])
        got = depth_normals(d, intr, T).cpu().numpy()
        ref = R.normals(d, intr, T)
        assert got.shape == (f, h, w, 3) and got.dtype == np.float64
        assert np.array_equal(_bits(got), _bits(ref)), (f, h, w)


def _clouds():
    rng = np.random.default_rng(4)
    out = {}
    out["uniform"] = rng.random((20000, 3))
    th, ph = rng.random(30000) * 2 * np.pi, np.arccos(1 - 2 * rng.random(30000))
    c = rng.normal(size=(5, 3))
    out["clustered surface"] = (c[rng.integers(0, 5, 30000)] + 0.1 * np.stack([np.sin(ph) * np.cos(th),
                                                                            np.sin(ph) * np.sin(th), np.cos(ph)], 1))
    g = np.arange(22) * 0.25
    out["lattice ties"] = np.stack(np.meshgrid(g, g, g), -1).reshape(-1, 3)
    u = rng.random((10000, 3))
    out["duplicates"] = np.concatenate([u, u[::50], u[::97], u[:3]])
    out["far outliers"] = np.concatenate([rng.random((20000, 3)), rng.normal(size=(20, 3)) * 1e4])
    out["all identical"] = np.tile([[0.25, -1.5, 3.0]], (3000, 1))
    p = rng.random((20000, 3))
    p[:, 2] = -0.2
    out["planar"] = p
    out["N = 4"] = rng.random((4, 3))
    out["line"] = np.stack([rng.random(5000), np.zeros(5000), np.zeros(5000)], 1)
    return {k: v.astype(np.float32) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _knn_ref(name):
    """(cloud, fp32 distances, fp64 squared distances, indices by the tie rule) of a cloud of _clouds() for k = 8 (3
    for N = 4), brute force, computed once per process and read-only; the first k columns are the answer for k."""
    x = _clouds()[name]
    out = (x,) + R.knn(x, 8 if x.shape[0] > 8 else 3, index=True)
    for a in out:
        a.setflags(write=False)
    return out


def _check_knn(name, k, dist, idx, what):
    """dist: the reference's bits.  idx: a neighbour set that reproduces its distances and, for every point without
    a neighbour at distance 0, exactly the k smallest (squared distance, index) pairs."""
    x, ref_d, ref_s, ref_i = _knn_ref(name)
    n = x.shape[0]
    assert dist.dtype == np.float32 and idx.dtype == np.int64 and dist.shape == idx.shape == (n, k)
    assert np.array_equal(dist.view(np.uint32), ref_d[:, :k].view(np.uint32)), (name, k, what)
    assert ((idx >= 0) & (idx < n)).all() and (idx != np.arange(n)[:, None]).all()
    assert all(len(set(r)) == k for r in idx[:: max(1, n // 2000)])
    xd = x.astype(np.float64)
    d = xd[idx] - xd[:, None, :]
    again = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)
    assert np.array_equal(again.view(np.uint32), dist.view(np.uint32)), (name, k, what)
    apart = ref_s[:, 0] > 0.0
    assert np.array_equal(idx[apart], ref_i[apart, :k]), (name, k, what)
    return int(apart.sum())


@gpu
@pytest.mark.parametrize("name", list(_clouds()))
def test_knn_bit_exact(name):
    from gaussiangrasper_amd.prepare import knn_distances
    x = _clouds()[name]
    ks = (3, 1, 8) if x.shape[0] > 8 else (3,)
    for k in ks:
        dist, idx = knn_distances(torch.from_numpy(x).cuda(), k)
        apart = _check_knn(name, k, dist.cpu().numpy(), idx.cpu().numpy(), "fitted grid")
        if name == "lattice ties":                         # every neighbour shell is a tie: the rule decides them all
            ref_s = _knn_ref(name)[2]
            assert apart == x.shape[0] and (ref_s[:, 0] == ref_s[:, 1]).all()


def _knn_on_grid(x, k, grid, dims):
    """gg_knn on a caller's grid (lower corner and cell edge, cells per axis) -> (dist, idx) as numpy"""
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = x.shape[0]
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    grid_c, dims_c = (ctypes.c_double * 4)(*grid), (ctypes.c_int32 * 3)(*dims)
    need = lib.gg_knn_workspace(n, dims_c)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dist = torch.full((n, k), -1.0, dtype=torch.float32, device="cuda")
    idx = torch.full((n, k), -1, dtype=torch.int64, device="cuda")
    P = ctypes.c_void_p
    st = lib.gg_knn(n, P(xd.data_ptr()), k, grid_c, dims_c, P(dist.data_ptr()), P(idx.data_ptr()), P(ws.data_ptr()),
                    need, P(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.gg_last_error()
    torch.cuda.synchronize()
    return dist.cpu().numpy(), idx.cpu().numpy()


# "any grid gives the same result" (include/gg_raster.h): cloud, (lower corner, cell edge), cells per axis
HOSTILE_GRIDS = {
    # every point of the 22^3 lattice lies exactly on a cell face: the search's face bound b is 0
    "cell faces": ("lattice ties", (0.0, 0.0, 0.0, 0.25), (22, 22, 22)),
    # one cell, and a grid that misses the cloud (everything clamped into one corner cell): the quadratic walk,
    # 10 648^2 = 1.1e8 distances
    "one cell": ("lattice ties", (0.0, 0.0, 0.0, 1.0), (1, 1, 1)),
    "misses the cloud": ("lattice ties", (50.0, 50.0, 50.0, 0.001), (40, 30, 20)),
    # flat: one column of 4096 thin cells, a lattice layer in every 128th of them
    "flat": ("lattice ties", (0.0, 0.0, 0.0, 1.0 / 512.0), (1, 1, 4096)),
    # 128 x 128 x 65 = 1 064 960 cells are 1040 tile sums: pp_scan_single_kernel carries across its first 1024;
    # the upper half of the unit cube is clamped into the top layer
    "scan carry": ("uniform", (0.0, 0.0, 0.0, 1.0 / 128.0), (128, 128, 65)),
}


@gpu
@pytest.mark.parametrize("grid_name", list(HOSTILE_GRIDS))
def test_knn_on_any_grid(grid_name):
    from gaussiangrasper_amd.prepare import knn_distances
    name, grid, dims = HOSTILE_GRIDS[grid_name]
    x, _, ref_s, _ = _knn_ref(name)
    assert (ref_s[:, 0] > 0.0).all()                           # no zero distances: the indices are pinned everywhere
    if grid_name == "scan carry":
        assert -(-dims[0] * dims[1] * dims[2] // 1024) > 1024 and (x[:, 2] > 65.0 / 128.0).sum() > 5000
    for k in (1, 3, 8):
        dist, idx = _knn_on_grid(x, k, grid, dims)
        assert _check_knn(name, k, dist, idx, grid_name) == x.shape[0]
        fit_d, fit_i = knn_distances(torch.from_numpy(x).cuda(), k)
        assert np.array_equal(dist.view(np.uint32), fit_d.cpu().numpy().view(np.uint32))
        assert np.array_equal(idx, fit_i.cpu().numpy())


@gpu
def test_knn_worst_cases_have_a_bounded_time():
    from gaussiangrasper_amd.prepare import knn_distances
    rng = np.random.default_rng(5)
    th, z = rng.random(1_000_000) * 2 * np.pi, rng.random(1_000_000)
    bulk = np.stack([np.cos(th), np.sin(th), z], 1)
    clouds = {"outliers": np.concatenate([bulk, rng.normal(size=(100, 3)) * 1e3]).astype(np.float32),
              "1 % outliers": np.concatenate([bulk, rng.normal(size=(10_000, 3)) * 1e3]).astype(np.float32),
              "identical": np.zeros((1_000_000, 3), np.float32)}
    for name, x in clouds.items():
        xt = torch.from_numpy(x).cuda()
        knn_distances(xt[:1000], 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dist, _ = knn_distances(xt, 3)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert dt < 10.0, (name, dt)
        if name == "identical":
            assert (dist == 0).all()
        else:
            far = dist[-100:].cpu().numpy()
            ref, _ = R.knn(x[-100:], 3)   # the last 100 outliers among themselves bound their distances from above
            assert (far <= ref).all()


@gpu
def test_plugin_device_knn_returns_the_reference_types():
    from gaussiangrasper_amd.plugin import make_fused_model_class
    from gaussiangrasper_amd.scene import make_scene
    from gaussiangrasper_amd.stub import StubGaussianSplattingModel
    model = make_fused_model_class(StubGaussianSplattingModel, device_knn=True)(make_scene(5000, feature_dim=32))
    model = model.to("cuda:0")
    d, i = model.k_nearest_sklearn(model.means.data, 3)
    assert isinstance(d, np.ndarray) and isinstance(i, np.ndarray)
    assert d.dtype == np.float32 and i.dtype == np.float32 and d.shape == i.shape == (5000, 3)
    ref, _ = R.knn(model.means.data.cpu().numpy(), 3)
    assert np.array_equal(d.view(np.uint32), ref.view(np.uint32))
    d2, _ = model.k_nearest_sklearn(model.means.data.cpu(), 3)        # a host tensor is moved to the device
    assert np.array_equal(d2, d)


@gpu
def test_cli_end_to_end_twice_byte_identical(tmp_path):
    from gaussiangrasper_amd.prepare import depth_normals, main
    scan = tmp_path / "scan"
    meta = R.write_scan(str(scan), n_frames=5, h=30, w=41, seed=6, units=1000.0)
    (scan / "boundary_mask" / "frame_0002.npy").unlink()
    from PIL import Image
    Image.fromarray(np.full((30, 41, 3), 255, np.uint8)).save(scan / "boundary_mask" / "frame_0002.png")
    outs = []
    for run, batch in (("a", 2), ("b", 5)):
        out = tmp_path / run
        assert main(["--scan", str(scan), "--out", str(out), "--depth-units-per-metre", "1000", "--seed", "9",
                     "--frames-per-batch", str(batch), "--normal-vis"]) == 0
        outs.append(out)
    files = sorted(os.path.relpath(os.path.join(d, f), outs[0]) for d, _, fs in os.walk(outs[0]) for f in fs)
    assert len(files) == 3 + 2 * 5
    for f in files:
        assert (outs[0] / f).read_bytes() == (outs[1] / f).read_bytes(), f
    sp = outs[0] / "colmap" / "sparse" / "0"
    cams = R.read_cameras_text(str(sp / "cameras.txt"))
    assert cams[1][:3] == ("OPENCV", 41, 30)
    ims = R.read_images_text(str(sp / "images.txt"))
    for i, fr in enumerate(meta["frames"]):
        T = np.array(fr["transform_matrix"])
        q, t, _, name, _ = ims[i + 1]
        assert name == os.path.basename(fr["file_path"])
        assert np.abs(R.qvec2rotmat(q) - T[:3, :3]).max() <= 1e-12 and np.abs(t - T[:3, 3]).max() <= 1e-12
    pts = R.read_points3D_text(str(sp / "points3D.txt"))
    # the seed cloud is the host restatement's rows, subsampled by the host law
    depth = np.stack([np.load(scan / "depths" / f"frame_{i:04d}.npy") / 1000.0 for i in range(5)])
    mask = np.stack([np.load(scan / "boundary_mask" / f"frame_{i:04d}.npy") if i != 2 else np.ones((30, 41))
                     for i in range(5)])
    rgb = np.stack([np.asarray(Image.open(scan / "images" / f"frame_{i:04d}.png").convert("RGB")) for i in range(5)])
    intr = np.array([[meta["fl_x"], meta["fl_y"], meta["cx"], meta["cy"]]] * 5)
    T = np.array([fr["transform_matrix"] for fr in meta["frames"]])
    rp, rc = R.backproject(depth, mask, rgb, intr, T)
    from gaussiangrasper_amd.prepare import subsample_indices
    sel = subsample_indices(rp.shape[0], 8, 9)
    assert len(pts) == len(sel) > 0
    assert np.allclose(np.array([pts[i + 1][0] for i in range(len(sel))]), rp[sel], atol=5e-7, rtol=0)
    assert np.array_equal(np.array([pts[i + 1][1] for i in range(len(sel))]), rc[sel].astype(int))
    for i in range(5):
        n = np.load(outs[0] / "normals" / f"frame_{i:04d}.npy")
        assert n.dtype == np.float64 and n.shape == (30, 41, 3)
        assert np.array_equal(n, depth_normals(depth[i], intr[i], T[i]).cpu().numpy()[0])
    assert main(["--scan", str(scan), "--out", str(outs[0])]) == 2          # refuses to overwrite
    assert main(["--scan", str(scan), "--out", str(outs[0]), "--depth-units-per-metre", "1000", "--seed", "9",
                 "--normal-vis", "--force"]) == 0
    assert (outs[0] / "colmap" / "sparse" / "0" / "points3D.txt").read_bytes() == \
        (outs[1] / "colmap" / "sparse" / "0" / "points3D.txt").read_bytes()


@gpu
def test_cli_per_frame_intrinsics_get_their_own_camera(tmp_path):
    from gaussiangrasper_amd.prepare import main
    import json
    scan = tmp_path / "scan"
    meta = R.write_scan(str(scan), n_frames=3, h=20, w=26, seed=8)
    meta["frames"][1]["fl_x"] = meta["fl_x"] * 1.1                  # frame 1 overrides fx
    (scan / "transforms.json").write_text(json.dumps(meta))
    assert main(["--scan", str(scan), "--out", str(tmp_path / "o")]) == 0
    sp = tmp_path / "o" / "colmap" / "sparse" / "0"
    cams = R.read_cameras_text(str(sp / "cameras.txt"))
    assert sorted(cams) == [1, 2] and cams[2][3][0] == meta["fl_x"] * 1.1 and cams[1][3][0] == meta["fl_x"]
    ims = R.read_images_text(str(sp / "images.txt"))
    assert [ims[i][2] for i in (1, 2, 3)] == [1, 2, 1]
