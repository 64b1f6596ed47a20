"""No-GPU checks of the distance field (gaussiangrasper_amd.field, gg_field_*): the restatement (tests/field_ref.py)
of the distance transform against scipy and against brute force, of the splat against an independent form of the
ellipsoid test, need2's conservative bound and gripper_spheres' cover as properties, the host helpers that build
poses, the C entries' argument validation and the workspace query."""
import ctypes
import math
import threading

import numpy as np
import pytest
import torch

import field_ref as ref
from grasp_ref import grasp_rows, rotation

D = ctypes.c_double
FAR = ref.FAR
EDT_DIMS = [(1, 1, 1), (1, 1, 17), (17, 1, 1), (3, 5, 7), (33, 17, 65), (64, 64, 64), (1024, 2, 2)]
DENSITIES = [0.0, 0.002, 0.05, 0.5, 1.0]


# ------------------------------------------------------------------------------------------------
# the distance transform's restatement
# ------------------------------------------------------------------------------------------------
def _brute(occ):
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in occ.shape], indexing="ij"), -1).reshape(-1, 3)
    src = idx[occ.reshape(-1)]
    if not len(src):
        return np.full(occ.shape, FAR, np.int64)
    d = ((idx[:, None, :] - src[None, :, :]) ** 2).sum(-1)
    return d.min(1).reshape(occ.shape)


@pytest.mark.parametrize("dims", EDT_DIMS)
def test_restatement_edt_against_scipy_and_brute_force(dims):
    from scipy.ndimage import distance_transform_edt
    rng = np.random.default_rng(sum(dims))
    for density in DENSITIES:
        occ = rng.random(dims) < density if 0.0 < density < 1.0 else np.full(dims, density == 1.0)
        got = ref.distance(np.where(occ, 7, 6), threshold=7)
        assert got.dtype == np.int32
        if not occ.any():
            assert (got == FAR).all()
            continue
        want = np.rint(distance_transform_edt(~occ) ** 2).astype(np.int64)
        assert np.array_equal(got, want), (dims, density)
        if occ.size <= 2500:
            assert np.array_equal(got, _brute(occ)), (dims, density)


def test_empty_volume_is_far_everywhere_and_the_far_corner():
    assert (ref.distance(np.zeros((5, 4, 3), np.int64), 1) == FAR).all()
    m = np.zeros((1024, 2, 2), np.int64)
    m[0, 0, 0] = 1
    d = ref.distance(m, 1)
    assert d[1023, 1, 1] == 1023 ** 2 + 2 and d[0, 0, 0] == 0 and d[1023, 0, 0] == 1023 ** 2
    assert FAR + 2 * 1023 ** 2 < 2 ** 31


# ------------------------------------------------------------------------------------------------
# the splat's restatement against sum (u_j / s_j)^2 <= k^2
# ------------------------------------------------------------------------------------------------
def test_splat_restatement_against_the_form_with_division():
    rng = np.random.default_rng(11)
    dims, grid = (16, 14, 18), np.array([-0.07, 0.01, 0.3, 0.01])
    n, k = 48, 1.5
    lo, h = grid[:3], grid[3]
    means = (lo + rng.uniform(-1.0, np.array(dims) + 1.0, size=(n, 3)) * h).astype(np.float32)   # some outside
    R = rotation(rng, n).astype(np.float32)
    s = (rng.uniform(0.3, 2.5, size=(n, 3)) * h).astype(np.float32)
    w = rng.uniform(0.05, 1.0, n).astype(np.float32)
    got, skipped, truncated = ref.splat(dims, grid, means, R, s, w, extent=k, max_reach=8)
    assert skipped == 0 and truncated == 0
    cells = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    x = lo + (cells + 0.5) * h
    want = np.zeros(len(cells), np.int64)
    closest = math.inf
    for i in range(n):
        u = (x - means[i].astype(np.float64)) @ R[i].astype(np.float64)          # u_j = column j . d
        val = ((u / s[i].astype(np.float64)) ** 2).sum(1)
        own = (ref.cell_index(means[i].astype(np.float64)[None, :] - lo, h) == cells).all(1)
        closest = min(closest, np.abs(val[~own] - k * k).min() / (k * k))
        want[(val <= k * k) | own] += int(np.trunc(float(w[i]) * 65536.0))
    assert closest > 1e-9                         # no (row, cell) pair had to be set aside
    assert np.array_equal(got.reshape(-1), want)
    assert (got > 0).sum() > 500
    # a call with sign -1 on the same rows restores the zeros; max_reach 0 leaves the means' own cells only
    back, _, _ = ref.splat(dims, grid, means, R, s, w, extent=k, max_reach=8, sign=-1, mass=got)
    assert not back.any()
    own_only, _, cut = ref.splat(dims, grid, means, R, s, w, extent=k, max_reach=0)
    assert cut == n and (own_only > 0).sum() <= n


def test_splat_restatement_rows_reach_and_boundary_lattice():
    h = 0.125
    grid, dims = np.array([0.0, 0.0, 0.0, h]), (24, 24, 24)
    eye = np.eye(3, dtype=np.float32)[None]
    c = np.float32([[12.5 * h] * 3])              # a cell centre
    got, sk, tr = ref.splat(dims, grid, c, eye, np.float32([[5 * h] * 3]), np.float32([1.0]), extent=1.0, max_reach=8)
    assert (sk, tr) == (0, 0)
    ii = np.stack(np.meshgrid(*[np.arange(24)] * 3, indexing="ij"), -1) - 12
    assert np.array_equal(got != 0, (ii ** 2).sum(-1) <= 25)           # (3, 4, 0), (5, 0, 0): on the boundary, counted
    assert got[15, 16, 12] == 65536 and got[17, 12, 12] == 65536 and got[16, 16, 12] == 0
    # reach: n h >= k smax decided by the comparison; a row is cut iff n + 1 > max_reach
    s = np.float32([[h, h, 2 * h], [h, h, 2 * h + 2 ** -10], [0.5 * h] * 3])
    reach, cut = ref.row_reach(s, 1.0, h, 3)
    assert reach.tolist() == [3, 3, 2] and cut.tolist() == [False, True, False]
    assert ref.row_reach(s, 0.0, h, 8)[0].tolist() == [1, 1, 1]
    # rows that take no part
    m = np.zeros((6, 3), np.float32) + 1.0
    sc = np.full((6, 3), h, np.float32)
    w = np.float32([0.5, 0.5, 0.5, 0.0, 32768.0, 0.5])
    m[0, 1], sc[1, 2], sc[2, 0] = np.nan, 0.0, -h
    assert ref.row_takes_part(m, np.repeat(eye, 6, 0), sc, w, 0.0).tolist() == [False] * 5 + [True]
    # a mean on a cell face belongs to the upper cell
    assert ref.cell_index(np.array([0.0, h, 3 * h, -h, np.nextafter(h, 0)]), h).tolist() == [0, 1, 3, -1, 0]


# ------------------------------------------------------------------------------------------------
# need2 and the sphere cover
# ------------------------------------------------------------------------------------------------
def test_need2_is_conservative_on_random_cases():
    from gaussiangrasper_amd.field import need2
    rng = np.random.default_rng(5)
    n = 200_000
    h = rng.uniform(0.002, 0.05, n)
    rho = rng.uniform(0.0, 24.0, n) * h               # against offsets of up to 16 cells per axis: both outcomes common
    radius = rho * rng.random(n)
    need = np.array([need2(r, m, hh) for r, m, hh in zip(radius[:2000], (rho - radius)[:2000], h[:2000])])
    need = np.concatenate([need, np.floor(((radius[2000:] + (rho - radius)[2000:]) / h[2000:] + math.sqrt(3.0)) ** 2)
                           .astype(np.int64) + 1])
    p = rng.random((n, 3)) * h[:, None]                                   # a point of cell (0, 0, 0)
    delta = rng.integers(-16, 17, size=(n, 3))
    dist2 = (delta ** 2).sum(1)
    lo, hi = delta * h[:, None], (delta + 1) * h[:, None]
    gap = np.sqrt((np.maximum(0.0, np.maximum(lo - p, p - hi)) ** 2).sum(1))   # point to the occupied cell's cube
    passes = dist2 >= need
    assert passes.sum() > 20_000 and (~passes).sum() > 20_000
    assert int((passes & (gap <= radius + (rho - radius))).sum()) == 0
    assert need2(0.0, 0.0, 0.01) == 4 and need2(1e9, 0.0, 0.01) == FAR
    assert need2([0.0, 0.01], 0.0, 0.01).tolist() == [4, 8]
    with pytest.raises(ValueError):
        need2(-1.0, 0.0, 0.01)
    with pytest.raises(ValueError):
        need2(0.01, 0.0, 0.0)


def test_gripper_spheres_cover_every_box():
    from gaussiangrasper_amd.field import gripper_boxes, gripper_spheres
    from gaussiangrasper_amd.grasp import box_part, default_gripper
    rng = np.random.default_rng(6)
    wrist = box_part((-0.12, -0.064), (-0.03, 0.03), (-0.02, 0.02))
    for parts, radius in ((default_gripper(), 0.004), (default_gripper(), 0.01),
                          (np.concatenate([default_gripper(), wrist[None]]), 0.006)):
        w, d, hgt = 0.07, 0.025, 0.02
        c = gripper_spheres(parts, w, d, hgt, radius)
        assert c.dtype == np.float32 and c.ndim == 2 and c.shape[1] == 3 and len(c) <= 1024
        for b in gripper_boxes(parts, w, d, hgt):
            corners = np.stack(np.meshgrid(b[0:2], b[2:4], b[4:6], indexing="ij"), -1).reshape(-1, 3)
            pts = np.concatenate([b[0::2] + rng.random((4000, 3)) * (b[1::2] - b[0::2]), corners])
            near = np.sqrt(((pts[:, None, :] - c[None].astype(np.float64)) ** 2).sum(-1)).min(1)
            assert near.max() <= radius
    with pytest.raises(ValueError, match="larger radius"):
        gripper_spheres(default_gripper(), 0.08, 0.02, 0.02, 0.0005)
    with pytest.raises(ValueError):
        gripper_spheres(default_gripper(), 0.08, 0.02, 0.02, 0.0)


def test_poses_paths_and_interpolation():
    from gaussiangrasper_amd.field import approach_paths, grasp_poses, interpolate
    rng = np.random.default_rng(8)
    R = rotation(rng, 5)
    t = rng.uniform(-0.2, 0.2, size=(5, 3))
    rows = grasp_rows(R, t, 0.05, 0.02, 0.01)
    P = grasp_poses(rows)
    assert P.shape == (5, 1, 12) and P.dtype == np.float32
    assert np.array_equal(P[:, 0, :9], rows[:, 4:13]) and np.array_equal(P[:, 0, 9:], rows[:, 13:16])
    A = approach_paths(rows, 0.1, 6)
    assert A.shape == (5, 6, 12) and np.array_equal(A[:, -1], P[:, 0])
    assert np.array_equal(A[:, :, :9], np.repeat(P[:, :, :9], 6, 1))
    assert np.allclose(A[:, 0, 9:], t - 0.1 * R[:, :, 0], atol=1e-6)
    assert np.allclose(np.diff(A[:, :, 9:], axis=1), 0.02 * R[:, None, :, 0], atol=1e-6)
    with pytest.raises(ValueError):
        approach_paths(rows, 0.1, 1)
    a, b = P[0, 0], P[1, 0]
    path = interpolate(a, b, 9)
    assert path.shape == (9, 12) and np.array_equal(path[0], a) and np.array_equal(path[-1], b)
    Rs = path[:, :9].reshape(-1, 3, 3).astype(np.float64)
    assert np.allclose(Rs @ Rs.transpose(0, 2, 1), np.eye(3), atol=1e-6)
    assert np.allclose(np.linalg.det(Rs), 1, atol=1e-6)
    ang = np.arccos(np.clip((np.trace(Rs[:-1].transpose(0, 2, 1) @ Rs[1:], axis1=1, axis2=2) - 1) / 2, -1, 1))
    total = math.acos(max(-1.0, min(1.0, (np.trace(Rs[0].T @ Rs[-1]) - 1) / 2)))
    assert np.allclose(ang, total / 8, atol=1e-5)                  # equal steps along the shorter arc
    assert np.allclose(np.diff(path[:, 9:], axis=0), (b[9:] - a[9:]) / 8, atol=1e-6)
    half_turn = np.concatenate([np.diag([1.0, -1.0, -1.0]).reshape(-1), [0, 0, 0]])
    H = interpolate(np.concatenate([np.eye(3).reshape(-1), [0, 0, 0]]), half_turn, 3)
    assert np.allclose(np.abs(H[1, :9].reshape(3, 3)), [[1, 0, 0], [0, 0, 1], [0, 1, 0]], atol=1e-6)
    with pytest.raises(ValueError):
        interpolate(a[:11], b, 4)


def test_field_grid_and_limits():
    from gaussiangrasper_amd.field import field_grid
    grid, dims = field_grid([0, 0, 0], [1.0, 0.5, 0.255], 0.01)
    assert grid.tolist() == [0, 0, 0, 0.01] and dims.tolist() == [100, 50, 26] and dims.dtype == np.int32
    for bad in (([0, 0, 0], [11, 1, 1], 0.01), ([0, 0, 0], [6, 6, 6], 0.01), ([0, 0, 0], [1, 1, 0], 0.01),
                ([0, 0, 0], [1, 1, 1], 0.0), ([0, 0, math.nan], [1, 1, 1], 0.01)):
        with pytest.raises(ValueError):
            field_grid(*bad)


# ------------------------------------------------------------------------------------------------
# the C entries
# ------------------------------------------------------------------------------------------------
def _call_on_thread(fn, cases):
    got = []

    def run():
        for args in cases:
            got.append(fn(args))
    t = threading.Thread(target=run)        # gg_last_error is per thread: the message does not outlive the test
    t.start()
    t.join()
    return got


def _dims(*d):
    return (ctypes.c_int32 * 3)(*d)


def _grid(*g):
    return (D * 4)(*g)


def _p(a):
    return None if a is None else ctypes.cast(a, ctypes.c_void_p)


def test_field_argument_validation_without_a_gpu():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = ctypes.c_void_p(0)
    f = ctypes.c_void_p(1 << 20)        # never dereferenced: every call below fails validation first
    odd = ctypes.c_void_p((1 << 20) + 4)
    ok_dims, ok_grid = _dims(32, 32, 32), _grid(0, 0, 0, 0.01)

    def splat(dims=ok_dims, grid=ok_grid, rows=10, ins=(f, f, f, f), extent=1.0, max_reach=8, min_weight=0.0, sign=1,
              outs=(f, f, f)):
        return (_p(dims), _p(grid), rows, *ins, D(extent), max_reach, D(min_weight), sign, *outs, n)
    cases = [
        (splat(dims=_dims(0, 4, 4)), b"dims"),
        (splat(dims=_dims(4, 1025, 4)), b"dims"),
        (splat(dims=_dims(1024, 1024, 129)), b"GG_FIELD_MAX_CELLS"),
        (splat(dims=None), b"dims"),
        (splat(grid=None), b"grid"),
        (splat(grid=_grid(0, 0, 0, 0.0)), b"h finite and > 0"),
        (splat(grid=_grid(0, 0, 0, -0.01)), b"h finite and > 0"),
        (splat(grid=_grid(0, 0, 0, math.nan)), b"h finite and > 0"),
        (splat(grid=_grid(0, math.inf, 0, 0.01)), b"grid"),
        (splat(rows=-1), b"num_rows"),
        (splat(extent=-0.5), b"extent"),
        (splat(extent=math.nan), b"extent"),
        (splat(extent=math.inf), b"extent"),
        (splat(max_reach=65), b"max_reach"),
        (splat(max_reach=-1), b"max_reach"),
        (splat(min_weight=math.nan), b"min_weight"),
        (splat(sign=0), b"sign"),
        (splat(sign=2), b"sign"),
        (splat(ins=(n, f, f, f)), b"null pointer"),
        (splat(ins=(f, f, f, n)), b"null pointer"),
        (splat(outs=(n, f, f)), b"null pointer"),
        (splat(outs=(f, f, n)), b"null pointer"),
        (splat(ins=(f, ctypes.c_void_p((1 << 20) + 2), f, f)), b"misaligned"),
        (splat(outs=(odd, f, f)), b"misaligned"),
        (splat(outs=(f, odd, f)), b"misaligned"),
    ]
    got = _call_on_thread(lambda a: (lib.gg_field_splat(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_field_splat") and want in msg, msg
    assert lib.gg_field_splat(*splat(rows=0, ins=(n,) * 4, outs=(n,) * 3)) == 0         # no rows: nothing to do

    need = lib.gg_field_distance_workspace(ok_dims)

    def dist(dims=ok_dims, mass=f, threshold=1, out=f, ws=f, ws_bytes=1 << 30):
        return (_p(dims), mass, threshold, out, ws, ctypes.c_size_t(ws_bytes), n)
    cases = [
        (dist(dims=_dims(4, 4, 0)), b"dims"),
        (dist(dims=_dims(1025, 1, 1)), b"dims"),
        (dist(dims=_dims(512, 512, 513)), b"GG_FIELD_MAX_CELLS"),
        (dist(threshold=0), b"threshold"),
        (dist(threshold=-5), b"threshold"),
        (dist(mass=n), b"null pointer"),
        (dist(out=n), b"null pointer"),
        (dist(mass=odd), b"misaligned"),
        (dist(out=ctypes.c_void_p((1 << 20) + 2)), b"misaligned"),
        (dist(ws=n), b"ws"),
        (dist(ws=ctypes.c_void_p((1 << 20) + 16)), b"ws"),
    ]
    got = _call_on_thread(lambda a: (lib.gg_field_distance(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_field_distance") and want in msg, msg
    for st, msg in _call_on_thread(lambda a: (lib.gg_field_distance(*a), lib.gg_last_error()),
                                   [dist(ws_bytes=need - 1), dist(ws_bytes=0)]):
        assert st == -3 and b"workspace" in msg

    def paths(dims=ok_dims, grid=ok_grid, dist2=f, P=3, W=5, poses=f, S=7, spheres=f, need2=f, outside=ref.FAR,
              outs=(f, f)):
        return (_p(dims), _p(grid), dist2, P, W, poses, S, spheres, need2, outside, *outs, n)
    cases = [
        (paths(dims=_dims(0, 1, 1)), b"dims"),
        (paths(grid=None), b"grid"),
        (paths(grid=_grid(0, 0, 0, 0.0)), b"h finite and > 0"),
        (paths(P=-1), b"num_paths"),
        (paths(W=-1), b"num_waypoints"),
        (paths(P=1 << 14, W=(1 << 12) + 1), b"GG_FIELD_MAX_POSES"),
        (paths(S=1025), b"num_spheres"),
        (paths(S=-1), b"num_spheres"),
        (paths(outside=-1), b"outside"),
        (paths(outside=ref.FAR + 1), b"outside"),
        (paths(dist2=n), b"null pointer"),
        (paths(poses=n), b"null pointer"),
        (paths(outs=(n, f)), b"null pointer"),
        (paths(outs=(f, n)), b"null pointer"),
        (paths(spheres=n), b"null pointer"),
        (paths(need2=n), b"null pointer"),
        (paths(poses=ctypes.c_void_p((1 << 20) + 1)), b"misaligned"),
        (paths(outs=(f, ctypes.c_void_p((1 << 20) + 2))), b"misaligned"),
    ]
    got = _call_on_thread(lambda a: (lib.gg_field_paths(*a), lib.gg_last_error()), [c[0] for c in cases])
    for (st, msg), (_, want) in zip(got, cases):
        assert st == -1 and msg.startswith(b"gg_field_paths") and want in msg, msg
    # no paths or no waypoints: nothing to do, null pointers accepted
    assert lib.gg_field_paths(*paths(P=0, dist2=n, poses=n, spheres=n, need2=n, outs=(n, n))) == 0
    assert lib.gg_field_paths(*paths(W=0, dist2=n, poses=n, spheres=n, need2=n, outs=(n, n))) == 0


def test_field_distance_workspace_query():
    from gaussiangrasper_amd import _lib
    ws = _lib.load().gg_field_distance_workspace
    for bad in ((0, 1, 1), (1, 1, 1025), (-3, 4, 4), (1024, 1024, 129), (512, 513, 512)):
        assert ws(_dims(*bad)) == 0
    assert ws(None) == 0
    sizes = [ws(_dims(*d)) for d in ((1, 1, 1), (3, 5, 7), (33, 17, 65), (64, 64, 64), (128, 128, 128), (1024, 2, 2),
                                      (512, 512, 512))]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert sizes[:5] == sorted(sizes[:5]) and sizes[-1] == max(sizes) and sizes[-1] <= 1 << 30
    assert ws(_dims(8, 8, 9)) >= ws(_dims(8, 8, 8)) and ws(_dims(9, 8, 8)) >= ws(_dims(8, 8, 8))


def test_the_calls_refuse_host_tensors_and_bad_arguments():
    from gaussiangrasper_amd import field
    mass = torch.zeros(4, 4, 4, dtype=torch.int64)
    rows = (torch.zeros(2, 3), torch.zeros(2, 9), torch.ones(2, 3), torch.ones(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        field.splat(mass, [0, 0, 0, 0.01], [4, 4, 4], *rows)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        field.distance(mass, [4, 4, 4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        field.paths(torch.zeros(4, 4, 4, dtype=torch.int32), [0, 0, 0, 0.01], [4, 4, 4], torch.zeros(1, 1, 12),
                    torch.zeros(1, 3), torch.zeros(1, dtype=torch.int32))
    assert field.THRESHOLD == math.trunc(0.5 * 2 ** 16) and field.EXTENT == 1.0 and field.MAX_REACH == 8
    from gaussiangrasper_amd.grasp import MIN_WEIGHT
    assert field.MIN_WEIGHT == MIN_WEIGHT and field.VOXEL == 0.01


def test_cli_argument_errors(tmp_path):
    from gaussiangrasper_amd import field
    base = ["--ckpt", str(tmp_path / "none.ckpt"), "--bbox", "0", "0", "0", "1", "1", "1", "--out",
            str(tmp_path / "f.npz")]
    np.save(tmp_path / "p.npy", np.zeros((2, 3, 12), np.float32))
    for extra in (["--paths", str(tmp_path / "p.npy")], ["--gripper", "default"], ["--voxel", "0"],
                  ["--voxel", "nan"], ["--extent", "-1"], ["--max-reach", "65"], ["--occupied", "0"],
                  ["--min-opacity", "nan"], ["--outside", "maybe"], ["--threshold", "0.5"]):
        with pytest.raises(SystemExit) as e:
            field.main(base + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit, match="error"):                 # 10^9 cells
        field.main(base + ["--voxel", "0.001"])
    with pytest.raises(SystemExit, match="error"):                 # valid options: on to the checkpoint
        field.main(base + ["--voxel", "0.05"])
    assert not (tmp_path / "f.npz").exists()
