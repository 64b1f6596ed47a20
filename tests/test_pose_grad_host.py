"""No-GPU checks of the camera-pose gradient: the float64 reference the GPU tests hold the pose VJP
to (tests/pose_grad_ref.py) reproduces the oracle's projection backward, the stand-in camera optimizer's exponential
maps, and the new C-ABI entries' host-side argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import pose_grad_ref as ref
from gaussiangrasper_amd.camera import ring_cameras
from gaussiangrasper_amd.scene import make_scene

F64 = np.float64


def _scene(n=300, h=48, w=64, spread=1.0, seed=3):
    sc = make_scene(n, feature_dim=4, config_index=seed)
    v = ring_cameras(3, h, w)[1]
    means = sc.means.numpy().astype(F64) * spread
    scales = sc.scales.exp().numpy().astype(F64) * (12.0 if spread <= 1.0 else 80.0)   # beyond the FOV: wide ones
    quats = sc.quats.numpy().astype(F64) * 1.3          # un-normalised: the q / |q| VJP
    return v, means, scales, quats


@pytest.mark.parametrize("spread", [1.0, 2.5])
def test_fp64_reference_reproduces_the_oracle_backward(oracle, spread):
    """autograd through pose_grad_ref.project == oracle.project_bwd (fp64) for means, scales and quaternions: the
    restatement, the conic cotangent convention and the FOV clamp rule are the oracle's (spread 2.5 puts Gaussians
    beyond the clamp)"""
    v, means, scales, quats = _scene(n=300 if spread <= 1.0 else 1500, spread=spread)
    vm, pm = v.viewmat[:3].numpy().astype(F64), v.projmat.numpy().astype(F64)
    xys, depths, radii, conics, _nth, _ = oracle.project_fwd(means, scales, 1.0, quats, vm, pm, v.fx, v.fy, v.cx, v.cy,
                                                           v.height, v.width, v.tile_bounds, dtype=F64)
    vis = radii > 0
    assert vis.sum() > 50
    t = means @ vm[:, :3].T + vm[:, 3]
    lim = 1.3 * 0.5 * v.width / v.fx
    if spread > 1.0:
        limy = 1.3 * 0.5 * v.height / v.fy
        clamped = (np.abs(t[vis, 0] / t[vis, 2]) > lim) | (np.abs(t[vis, 1] / t[vis, 2]) > limy)
        assert clamped.sum() > 5, clamped.sum()     # the clamp is exercised
    rng = np.random.default_rng(1)
    n = len(means)
    v_xy, v_depth, v_conic = rng.standard_normal((n, 2)), rng.standard_normal(n), rng.standard_normal((n, 3))
    om, os_, oq = oracle.project_bwd(means, scales, 1.0, quats, vm, pm, v.fx, v.fy, v.cx, v.cy, v.height, v.width, radii,
                                     conics, v_xy, v_depth, v_conic, dtype=F64)
    g = ref.pose_grads(means, scales, 1.0, quats, vm, pm, v.fx, v.fy, v.cx, v.cy, v.height, v.width, vis, v_xy,
                       v_depth, v_conic)
    # the reference's own conics equal the oracle's (same forward)
    _, _, con = ref.project(torch.tensor(means), torch.tensor(scales), 1.0, torch.tensor(quats), torch.tensor(vm),
                            torch.tensor(pm), v.fx, v.fy, v.cx, v.cy, v.height, v.width)
    assert np.abs(con.numpy()[vis] - conics[vis]).max() <= 1e-12 * np.abs(conics[vis]).max()
    for name, want in (("means", om), ("scales", os_), ("quats", oq)):
        got = g[name].numpy()
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err < 1e-12, (name, err)
    # the camera's gradient: the sums over the Gaussians of their contributions, finite
    assert torch.isfinite(g["v_viewmat"]).all() and torch.isfinite(g["v_projmat"]).all()
    assert (g["abs_viewmat"] > 0).all() and (g["v_projmat"][2] == 0).all()


def test_fp64_reference_camera_gradient_matches_finite_differences():
    """the viewmat / full_proj gradients of the reference against central differences of its own loss"""
    v, means, scales, quats = _scene(n=60, spread=1.0)
    vm, pm = v.viewmat[:3].double(), v.projmat.double()
    rng = np.random.default_rng(2)
    n = len(means)
    v_xy, v_depth, v_conic = (torch.tensor(rng.standard_normal(s)) for s in ((n, 2), (n,), (n, 3)))
    vis = torch.ones(n, dtype=torch.bool)
    g = ref.pose_grads(means, scales, 1.0, quats, vm, pm, v.fx, v.fy, v.cx, v.cy, v.height, v.width, vis, v_xy,
                       v_depth, v_conic)
    T = lambda a: torch.tensor(a)

    def loss(vm_, pm_):
        xys, d, c = ref.project(T(means), T(scales), 1.0, T(quats), vm_, pm_, v.fx, v.fy, v.cx, v.cy, v.height,
                                v.width)
        return float(ref.cotangent_loss(xys, d, c, v_xy, v_depth, v_conic))
    eps = 1e-6
    for r in range(3):
        for c in range(4):
            a, b = vm.clone(), vm.clone()
            a[r, c] += eps
            b[r, c] -= eps
            fd = (loss(a, pm) - loss(b, pm)) / (2 * eps)
            assert abs(fd - float(g["v_viewmat"][r, c])) <= 1e-5 * float(g["abs_viewmat"][r, c]) + 1e-6, (r, c)
    for r in (0, 1, 3):
        for c in range(4):
            a, b = pm.clone(), pm.clone()
            a[r, c] += eps
            b[r, c] -= eps
            fd = (loss(vm, a) - loss(vm, b)) / (2 * eps)
            assert abs(fd - float(g["v_projmat"][r, c])) <= 1e-5 * float(g["abs_projmat"][r, c]) + 1e-6, (r, c)


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_stand_in_camera_optimizer_exponential_map(mode):
    from gaussiangrasper_amd.pose import exp_map, homogeneous
    from gaussiangrasper_amd.stub import StubCameraOptimizer, StubCameras, StubPoseCameraOptimizer
    opt = StubPoseCameraOptimizer(4, mode)
    eye = torch.eye(4)[:3]
    assert torch.equal(opt([0, 1, 2, 3]), eye.expand(4, 3, 4))          # identity at zero
    g = torch.Generator().manual_seed(0)
    for scale in (1e-5, 1e-3, 0.3, 2.0):
        tan = torch.randn(64, 6, generator=g, dtype=torch.float64) * scale
        T = exp_map(tan, mode)
        R = T[:, :, :3]
        assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(64, 3, 3), atol=1e-12)
        assert torch.allclose(torch.linalg.det(R), torch.ones(64, dtype=torch.float64), atol=1e-12)
        # the rotation vector is the axis (fixed by R) and the angle
        w = tan[:, 3:]
        assert torch.allclose((R @ w[:, :, None])[:, :, 0], w, atol=1e-12)
        if mode == "SO3xR3":
            assert torch.equal(T[:, :, 3], tan[:, :3])
    # a gradient at exactly zero (the camera optimizer starts there)
    tan = torch.zeros(1, 6, dtype=torch.float64, requires_grad=True)
    (exp_map(tan, mode) * torch.arange(12, dtype=torch.float64).reshape(1, 3, 4)).sum().backward()
    assert torch.isfinite(tan.grad).all() and (tan.grad != 0).all()
    # apply_to_camera: c2w @ adj for the camera's row, param group "camera_opt"
    cam = StubCameras(torch.eye(4), 50.0, 50.0, 16.0, 12.0, 24, 32)
    cam.metadata = {"cam_idx": 2}
    with torch.no_grad():
        opt.pose_adjustment[2] = torch.tensor([0.1, -0.2, 0.3, 0.05, 0.1, -0.02])
    before = cam.camera_to_worlds.clone()
    opt.apply_to_camera(cam)
    want = torch.bmm(before, homogeneous(exp_map(opt.pose_adjustment[[2]].detach(), mode)))
    assert torch.allclose(cam.camera_to_worlds, want)
    groups = {}
    opt.get_param_groups(groups)
    assert groups == {"camera_opt": [opt.pose_adjustment]}
    assert StubCameraOptimizer().apply_to_camera(cam) is None           # the "off" stand-in stays as it was


def test_pose_abi_symbols_and_host_argument_checks():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gg_pose_grad_workspace", "gg_view_bwd_pose", "gg_project_pose_bwd"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.gg_pose_grad_workspace(0) >= 96 and lib.gg_pose_grad_workspace(1_000_000) == 96 * 3907
    assert lib.gg_prof_name(40) == b"view_bwd_pose_kernel" and lib.gg_prof_name(42) == b"pose_finish_kernel"
    n = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(4096)           # never dereferenced: every call below is refused before a launch
    ws_ok = lib.gg_pose_grad_workspace(1000)

    def pose_bwd(N, means=fake, out=fake, ws=fake, ws_bytes=ws_ok, xs=2, cs=3):
        return lib.gg_project_pose_bwd(N, means, fake, 1.0, fake, fake, fake, 50.0, 50.0, 24, 32, fake, fake, fake, xs,
                                       fake, fake, cs, out, fake, ws, ws_bytes, n)
    assert pose_bwd(-1) == -1 and b"num_points" in lib.gg_last_error()
    assert pose_bwd(1000, out=n) == -1 and b"null" in lib.gg_last_error()
    assert pose_bwd(0, out=n) == -1                                  # N == 0 writes zeros: it needs the outputs
    assert pose_bwd(1000, means=n) == -1 and b"null" in lib.gg_last_error()
    assert pose_bwd(1000, ws=n) == -3 and b"gg_pose_grad_workspace" in lib.gg_last_error()
    assert pose_bwd(1000, ws_bytes=ws_ok - 4) == -3
    assert pose_bwd(1000, ws=ctypes.c_void_p(4100)) == -3            # not 16-byte aligned
    assert pose_bwd(1000, xs=1) == -1 and pose_bwd(1000, cs=2) == -1

    def view_bwd_pose(N, rec=fake, stride=16, out=fake, ws=fake, ws_bytes=ws_ok):
        return lib.gg_view_bwd_pose(N, rec, stride, fake, fake, fake, 1.0, fake, fake, fake, fake, fake, fake, 50.0,
                                    50.0, 24, 32, fake, fake, fake, fake, fake, fake, fake, out, fake, ws, ws_bytes, n)
    assert view_bwd_pose(-1) == -1
    assert view_bwd_pose(1000, stride=12) == -1 and b"13" in lib.gg_last_error()
    assert view_bwd_pose(1000, out=n) == -1
    assert view_bwd_pose(1000, rec=n) == -1 and b"null" in lib.gg_last_error()
    assert view_bwd_pose(1000, ws_bytes=16) == -3
    assert view_bwd_pose(1000, rec=ctypes.c_void_p(4100)) == -1     # 16-float records must be 16-byte aligned
