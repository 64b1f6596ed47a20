"""No-GPU checks of the registration: the numpy restatement (tests/register_ref.py) against independent statements
(a KD-tree, central differences, a plane with a linear intensity), the host side of gaussiangrasper_amd.register,
and the C ABI's argument checks."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import register_ref as R


@pytest.fixture(scope="module")
def scene():
    P, I, S, Is = R.scene()
    nrm, grad, count, valid, gap = R.cloud_frames(P, I, 0.02)
    return dict(P=P, I=I, S=S, Is=Is, nrm=nrm, grad=grad, count=count, valid=valid, gap=gap)


def test_scene_is_the_one_the_bounds_were_reasoned_for(scene):
    assert scene["count"].min() >= 21 and scene["count"].max() <= 106
    assert scene["valid"].all() and (scene["gap"] >= 1e-2).all()


def test_correspondences_equal_a_kd_tree(scene):
    from scipy.spatial import cKDTree
    s = R.move(np.eye(4), scene["S"])
    corr, best, two = R.correspondences(s, scene["P"], scene["valid"], 0.01)
    dist, j = cKDTree(scene["P"]).query(s, k=1, distance_upper_bound=0.01)
    hit = np.isfinite(dist)
    clear = two[:, 0] != two[:, 1]                   # wherever the two nearest distances differ
    assert clear.sum() > 0.99 * len(s)
    assert ((corr >= 0) == hit)[clear].all()
    assert (corr[hit & clear] == j[hit & clear]).all()
    assert np.allclose(np.sqrt(best[hit]), dist[hit], rtol=1e-12)


def test_jacobian_rows_equal_central_differences(scene):
    lam = 0.968
    s = R.move(np.eye(4), scene["S"])
    corr, _, _ = R.correspondences(s, scene["P"], scene["valid"], 0.01)
    hit = np.nonzero(corr >= 0)[0][:200]
    j = corr[hit]
    q, n, d = scene["P"][j], scene["nrm"][j], scene["grad"][j]
    i_s, i_q = scene["Is"][hit], scene["I"][j]
    Jg, _, Jp, _, _, _ = R.rows(s[hit], q, n, d, i_s, i_q, lam)

    def residuals(x):
        moved = s[hit] @ R.rodrigues(x[:3]).T + x[3:]
        _, rg, _, rp, _, _ = R.rows(moved, q, n, d, i_s, i_q, lam)
        return rg, rp

    h = 1e-6
    for a in range(6):
        e = np.zeros(6)
        e[a] = h
        (gp, pp), (gm, pm) = residuals(e), residuals(-e)
        # residuals are at most quadratic in x over this step: the central difference is exact to O(h^2) |s|
        assert np.abs((gp - gm) / (2 * h) - Jg[:, a]).max() < 1e-8
        assert np.abs((pp - pm) / (2 * h) - Jp[:, a]).max() < 1e-6 * max(1.0, np.abs(d).max())


def test_gradient_on_a_plane_is_the_tangential_part():
    rng = np.random.default_rng(3)
    n = np.array([0.2, -0.3, 0.9])
    n /= np.linalg.norm(n)
    t1 = np.cross(n, [1.0, 0, 0])
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(n, t1)
    uv = rng.uniform(-0.05, 0.05, (400, 2))
    P = uv[:, :1] * t1 + uv[:, 1:] * t2
    a, c = np.array([1.5, -2.0, 0.7]), 0.4
    nrm, grad, count, valid, _ = R.cloud_frames(P, P @ a + c, 0.02)
    full = count >= 4
    assert full.sum() > 300
    want = a - (a @ n) * n
    assert np.abs(grad[full] - want).max() < 1e-10
    assert np.abs(np.abs(nrm[full] @ n) - 1.0).max() < 1e-12


def test_voxel_downsample_law():
    from gaussiangrasper_amd.register import voxel_downsample
    # lower corner (0, 0, 0), voxel 1: the origin is (-0.5, -0.5, -0.5), so voxel i covers [i - 0.5, i + 0.5)
    P = np.array([[0.0, 0.0, 0.0], [0.4, 0.0, 0.0], [0.6, 0.0, 0.0], [1.4, 0.2, 0.0], [0.0, 2.6, 0.3],
                  [0.1, 3.4, 0.0], [np.nan, 0.0, 0.0]])
    C = np.arange(21, dtype=np.float64).reshape(7, 3)
    p, c = voxel_downsample(torch.tensor(P), torch.tensor(C), 1.0)
    # voxels by key (ix ny + iy) nz + iz: (0,0,0) <- rows 0, 1; (0,3,0) <- rows 4, 5; (1,0,0) <- rows 2, 3
    assert p.shape == (3, 3)
    assert np.allclose(p.numpy(), [P[[0, 1]].mean(0), P[[4, 5]].mean(0), P[[2, 3]].mean(0)], rtol=0, atol=1e-15)
    assert np.allclose(c.numpy(), [C[[0, 1]].mean(0), C[[4, 5]].mean(0), C[[2, 3]].mean(0)], rtol=0, atol=1e-15)
    rp, rc = R.voxel_downsample(P[:6], C[:6], 1.0)
    assert np.allclose(p.numpy(), rp, rtol=0, atol=1e-15) and np.allclose(c.numpy(), rc, rtol=0, atol=1e-15)
    p2, c2 = voxel_downsample(torch.tensor(P[:6]), None, 1.0)
    assert c2 is None and torch.equal(p2, p)
    with pytest.raises(ValueError):
        voxel_downsample(torch.tensor(P), None, 0.0)


def test_solve_step_of_an_aligned_pair_is_the_identity(scene):
    from gaussiangrasper_amd.register import IcpSums, rodrigues, solve_step
    sel = np.arange(0, 6000, 3)
    sums, _, corr = R.icp_sums(scene["P"][sel], scene["I"][sel], scene["P"], scene["I"], scene["nrm"], scene["grad"],
                               scene["valid"], np.eye(4), 0.01, 0.968)
    assert (corr == sel).all() and sums[27] == len(sel) and (sums[21:27] == 0).all()
    T, ok = solve_step(IcpSums(sums, len(sel)), np.eye(4))
    assert ok and np.array_equal(T, np.eye(4))
    T, ok = solve_step(np.zeros(32), R.TRUE_MOTION)            # no correspondences: singular, unchanged
    assert not ok and np.array_equal(T, R.TRUE_MOTION)
    bad = sums.copy()
    bad[3] = np.nan
    assert not solve_step(bad, np.eye(4))[1]
    # the update is [Rodrigues(w) | v] on the left, and the package's step equals the restatement's
    sums, _, _ = R.icp_sums(scene["S"], scene["Is"], scene["P"], scene["I"], scene["nrm"], scene["grad"],
                            scene["valid"], np.eye(4), 0.02, 0.968)
    T, ok = solve_step(sums, np.eye(4))
    Tr, okr = R.solve_step(sums, np.eye(4))
    assert ok and okr and np.allclose(T, Tr, rtol=0, atol=1e-14)
    w = np.array([0.3, -0.2, 0.5])
    assert np.allclose(rodrigues(w), R.rodrigues(w), rtol=0, atol=1e-15)
    assert np.allclose(rodrigues(1e-10 * w), R.rodrigues(1e-10 * w), rtol=0, atol=1e-18)


def test_three_scale_restatement_converges(scene):
    """Converged means: the pose is resolved well below the scale of the finest correspondences.  The bounds are a
    tenth of the finest voxel (0.5 mm) in translation and the rotation that moves the scene's edge (0.15 m from the
    centre) by as much, 0.5 mm / 0.15 m = 3.3e-3, as a Frobenius norm sqrt(2) times that; the start is 7.8 mm and
    5.5e-2 away."""
    rot0, tr0 = R.motion_error(np.eye(4))
    assert rot0 > 5e-2 and tr0 > 7e-3
    col = lambda i: np.repeat(i[:, None], 3, axis=1)
    T, fit, rmse, iters = R.colored_icp(scene["S"], col(scene["Is"]), scene["P"], col(scene["I"]))
    rot, tr = R.motion_error(T)
    print(f"restatement, lambda 0.968: rotation {rot:.3e}, translation {tr:.3e} m, fitness {fit:.4f}, "
          f"rmse {rmse:.3e}, iterations {iters}")
    assert tr < 5e-4 and rot < np.sqrt(2) * 5e-4 / 0.15
    assert fit > 0.9 and len(iters) == 3
    T, fit, rmse, iters = R.colored_icp(scene["S"], None, scene["P"], None, lam=1.0)
    rot, tr = R.motion_error(T)
    print(f"restatement, lambda 1: rotation {rot:.3e}, translation {tr:.3e} m, iterations {iters}")
    assert tr < 5e-4 and rot < np.sqrt(2) * 5e-4 / 0.15


def test_refine_poses_is_off_by_default():
    from gaussiangrasper_amd import prepare
    sig = inspect.signature(prepare.prepare_scene)
    assert sig.parameters["refine_poses"].default is False and sig.parameters["refine_options"].default is None
    # every parameter the function had keeps its place and default
    names = list(sig.parameters)
    assert names[:10] == ["scan_dir", "out_dir", "keep", "seed", "depth_units_per_metre", "depth_range", "z_range",
                          "frames_per_batch", "normal_vis", "force"]


def test_refine_poses_flag_reaches_prepare_scene(monkeypatch, tmp_path):
    from gaussiangrasper_amd import prepare
    seen = []

    def fake(scan, out, **kw):
        seen.append(kw)
        return {"frames": 0, "width": 0, "height": 0, "points": 0, "seed_points": 0, "out_dir": str(tmp_path),
                "read_s": 0.0, "gpu_s": 0.0, "write_s": 0.0}

    monkeypatch.setattr(prepare, "prepare_scene", fake)
    assert prepare.main(["--scan", str(tmp_path)]) == 0 and prepare.main(["--scan", str(tmp_path), "--refine-poses"]) == 0
    assert [kw["refine_poses"] for kw in seen] == [False, True]


def test_abi_surface_and_argument_checks():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    for name in ("gg_cloud_frames_workspace", "gg_cloud_frames", "gg_icp_step_workspace", "gg_icp_step"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.gg_prof_name(48) == b"gg_cloud_frames(all launches)"
    assert lib.gg_prof_name(49) == b"gg_icp_step(all launches)"
    dims = (ctypes.c_int32 * 3)(4, 4, 4)
    grid = (ctypes.c_double * 4)(0.0, 0.0, 0.0, 0.1)
    small, big = lib.gg_cloud_frames_workspace(100, dims), lib.gg_cloud_frames_workspace(100000, dims)
    assert 0 < small < big and lib.gg_cloud_frames_workspace(0, dims) == 0
    assert 0 < lib.gg_icp_step_workspace(1, 100, dims) < lib.gg_icp_step_workspace(100000, 100, dims)
    assert lib.gg_icp_step_workspace(0, 100, dims) == 0 and lib.gg_icp_step_workspace(1, 0, dims) == 0
    assert lib.gg_icp_step_workspace(1, 1, (ctypes.c_int32 * 3)(0, 1, 1)) == 0
    n = ctypes.c_void_p(0)
    P = ctypes.cast(grid, ctypes.c_void_p)
    D = ctypes.cast(dims, ctypes.c_void_p)
    assert lib.gg_cloud_frames(0, n, n, 0.1, P, D, n, n, n, n, n, 0, n) == -1 and b"num_points" in lib.gg_last_error()
    assert lib.gg_cloud_frames(4, n, n, 0.0, P, D, n, n, n, n, n, 0, n) == -1 and b"radius" in lib.gg_last_error()
    assert lib.gg_cloud_frames(4, n, n, 0.1, P, D, n, n, n, n, n, 0, n) == -1 and b"null" in lib.gg_last_error()
    args = [n, n, n, n, n, P, D, n]
    assert lib.gg_icp_step(4, n, n, 4, *args, 0.0, 0.5, 0, n, n, n, n, 0, n) == -1 and b"max_dist" in lib.gg_last_error()
    assert lib.gg_icp_step(4, n, n, 4, *args, 0.1, 1.5, 0, n, n, n, n, 0, n) == -1 and b"lambda" in lib.gg_last_error()
    assert lib.gg_icp_step(4, n, n, 4, *args, 0.1, float("nan"), 0, n, n, n, n, 0, n) == -1
    assert lib.gg_icp_step(0, n, n, 4, *args, 0.1, 0.5, 0, n, n, n, n, 0, n) == -1 and b"num_source" in lib.gg_last_error()


def test_colored_icp_argument_checks():
    from gaussiangrasper_amd.register import colored_icp
    P = np.zeros((4, 3))
    with pytest.raises(ValueError):
        colored_icp(P, None, P, None)                          # no colours needs lambda_geometric = 1
    with pytest.raises(ValueError):
        colored_icp(P, P, P, None)
    with pytest.raises(ValueError):
        colored_icp(P, P, P, P, voxel_radius=(0.02, 0.01), max_iter=(5,))
