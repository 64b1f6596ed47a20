"""Camera pose gradients on the MI355X: the pose VJP of csrc/project.hip against the float64
reference (tests/pose_grad_ref.py), the world-versus-camera identity through the whole plugin-route forward and
backward, the untouched default path, determinism, the plugin class with the stand-in camera optimizer, and pose
recovery with pose.refine_camera."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pose_grad_ref as ref
from gaussiangrasper_amd.camera import ring_cameras
from gaussiangrasper_amd.scene import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ptr(t, offset_floats=0):
    return C.c_void_p(t.data_ptr() + 4 * offset_floats)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _flip(dev, dtype=torch.float32):
    return torch.diag(torch.tensor([1.0, -1.0, -1.0], device=dev, dtype=dtype))


def _viewmat(c2w):
    """plugin.get_outputs' world -> camera matrix (gsplat convention), differentiable: (3, 4) or (4, 4) c2w -> (4, 4)"""
    R = c2w[:3, :3] @ _flip(c2w.device, c2w.dtype)
    R_inv = R.T
    top = torch.cat((R_inv, -R_inv @ c2w[:3, 3:4]), dim=1)
    last = torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=c2w.device, dtype=c2w.dtype)
    return torch.cat((top, last), dim=0)


def _c2w_of(view):
    w2c = view.viewmat.detach().cpu()
    c2w = torch.eye(4)
    c2w[:3, :3] = w2c[:3, :3].T @ _flip("cpu")
    c2w[:3, 3] = view.cam_pos.detach().cpu()
    return c2w.to(DEV)


def _projmat(view):
    """projmat alone (view.projmat is projmat @ viewmat), as camera.view_from_c2w forms it"""
    from gaussiangrasper_amd.camera import projection_matrix
    f32 = np.float32
    fovx = 2 * math.atan(float(f32(view.width) / (f32(2.0) * f32(view.fx))))
    fovy = 2 * math.atan(float(f32(view.height) / (f32(2.0) * f32(view.fy))))
    return projection_matrix(0.001, 1000, fovx, fovy).to(DEV)


# ------------------------------------------------------------------------------------------------------------------
# the kernels against the float64 reference
# ------------------------------------------------------------------------------------------------------------------
def _kernel_case(n, h, w, spread, smul, seed, zero_rows=None):
    from gaussiangrasper_amd import _lib, ops as P
    lib = _lib.load()
    sc = make_scene(n, feature_dim=4, config_index=seed)
    v = ring_cameras(3, h, w, device=DEV)[1]
    means = (sc.means * spread).to(DEV).contiguous()
    scales = (sc.scales.exp() * smul).to(DEV).contiguous()
    quats = sc.quats.to(DEV).contiguous()
    vm, pm = v.viewmat[:3].contiguous(), v.projmat.contiguous()
    with torch.no_grad():
        xys, depths, radii, conics, nth, _ = P.ProjectGaussians.apply(means, scales, 1, quats, vm, pm, v.fx, v.fy, v.cx,
                                                                      v.cy, h, w, v.tile_bounds)
    g = torch.Generator(device="cpu").manual_seed(seed)
    rec = torch.randn(n, 16, generator=g).to(DEV)                 # the pair backward's 16-float records
    if zero_rows is not None:
        rec[zero_rows] = 0.0                                      # no cotangent: these Gaussians add 0 to every sum
    v_depth = rec[:, 9].contiguous()
    return lib, v, means, scales, quats, vm, pm, radii, conics, rec, v_depth


def _pose_bwd(lib, n, v, means, scales, quats, vm, pm, radii, conics, rec, v_depth):
    out_v, out_p = torch.full((12,), float("nan"), device=DEV), torch.full((16,), float("nan"), device=DEV)
    ws = torch.empty(max(lib.gg_pose_grad_workspace(n), 256), dtype=torch.uint8, device=DEV)
    st = lib.gg_project_pose_bwd(n, _ptr(means), _ptr(scales), 1.0, _ptr(quats), _ptr(vm), _ptr(pm), v.fx, v.fy,
                                 v.height, v.width, _ptr(radii), _ptr(conics), _ptr(rec), 16, _ptr(v_depth),
                                 _ptr(rec, 2), 16, _ptr(out_v), _ptr(out_p), _ptr(ws), ws.numel(), _stream())
    assert st == 0, lib.gg_last_error()
    return out_v, out_p


def _view_bwd(lib, pose, n, v, means, scales, quats, vm, pm, radii, conics, rec):
    """gg_view_bwd (pose False) or gg_view_bwd_pose on fresh gradient buffers holding a known non-zero start"""
    g = torch.Generator(device="cpu").manual_seed(99)
    sinks = [torch.randn(n, k, generator=g).to(DEV) for k in (3, 3, 4, 1)]
    v_rgb = torch.empty(n, 3, device=DEV)
    mask = torch.randint(0, 8, (n,), generator=g, dtype=torch.uint8).to(DEV)
    axis = torch.argmin(scales, dim=1).to(torch.int32)
    opac = torch.rand(n, generator=g).to(DEV)
    args = [n, _ptr(rec), 16, _ptr(mask), _ptr(means), _ptr(scales), 1.0, _ptr(quats), _ptr(quats), _ptr(opac),
            _ptr(axis), _ptr(vm), _ptr(pm), v.fx, v.fy, v.height, v.width, _ptr(radii), _ptr(conics), _ptr(v_rgb)]
    args += [_ptr(s) for s in sinks]
    if not pose:
        assert lib.gg_view_bwd(*args, _stream()) == 0, lib.gg_last_error()
        return [v_rgb] + sinks, None, None
    out_v, out_p = torch.full((12,), float("nan"), device=DEV), torch.full((16,), float("nan"), device=DEV)
    ws = torch.empty(max(lib.gg_pose_grad_workspace(n), 256), dtype=torch.uint8, device=DEV)
    st = lib.gg_view_bwd_pose(*args, _ptr(out_v), _ptr(out_p), _ptr(ws), ws.numel(), _stream())
    assert st == 0, lib.gg_last_error()
    return [v_rgb] + sinks, out_v, out_p


@pytest.mark.parametrize("n,h,w,spread,smul", [(7, 45, 70, 1.0, 20.0), (300, 48, 64, 1.0, 12.0),
                                               (200, 32, 48, 2.5, 80.0), (150, 16, 32, 1.0, 12.0),
                                               (400, 32, 32, 2.5, 80.0), (300_000, 600, 800, 2.0, 3.0)])
def test_pose_kernels_against_the_fp64_reference(n, h, w, spread, smul):
    """gg_project_pose_bwd and gg_view_bwd_pose against autograd through the float64 restatement, per entry within
    1e-5 of the sum of the Gaussians' absolute contributions; the two entries give the same bits (shared device code,
    same reduction); gg_view_bwd_pose's per-Gaussian gradients are gg_view_bwd's, bit for bit"""
    lib, v, means, scales, quats, vm, pm, radii, conics, rec, v_depth = _kernel_case(n, h, w, spread, smul, seed=n % 97)
    vis = radii > 0
    assert int(vis.sum()) > 0
    got_v, got_p = _pose_bwd(lib, n, v, means, scales, quats, vm, pm, radii, conics, rec, v_depth)
    outs_pose, gv, gp = _view_bwd(lib, True, n, v, means, scales, quats, vm, pm, radii, conics, rec)
    outs_plain, _, _ = _view_bwd(lib, False, n, v, means, scales, quats, vm, pm, radii, conics, rec)
    torch.cuda.synchronize()
    assert torch.equal(gv, got_v) and torch.equal(gp, got_p)
    for a, b in zip(outs_pose, outs_plain):
        assert torch.equal(a, b)
    if spread > 1.0:       # Gaussians beyond the FOV clamp are part of the sums
        t = means @ vm[:, :3].T + vm[:, 3]
        lim = 1.3 * 0.5 * w / v.fx
        assert int(((t[:, 0] / t[:, 2]).abs() > lim)[vis].sum()) > 0
    want = ref.pose_grads(means, scales, 1.0, quats, vm, pm, v.fx, v.fy, v.cx, v.cy, h, w, vis, rec[:, 0:2], v_depth,
                          rec[:, 2:5])
    for got, key in ((got_v.reshape(3, 4), "viewmat"), (got_p.reshape(4, 4), "projmat")):
        err = (got.double() - want["v_" + key]).abs()
        bound = 1e-5 * want["abs_" + key] + 1e-30
        assert (err <= bound).all(), (key, err.max().item(), (err / bound).max().item())
    assert (got_p.reshape(4, 4)[2] == 0).all()


# pose_finish_kernel takes the slab's rows (256 Gaussians each) 12 x GG_POSE_FIN_ROWS = 2016 to a round
FIRST_ROUND = 2016 * 256


@pytest.mark.parametrize("planted", ["second round", "first round"])
def test_pose_finish_past_its_first_round(planted):
    """N = 516 096 + 3000 on the smallest image: 2028 slab rows, the last 12 of them in pose_finish_kernel's second
    round.  1e-5 of the absolute sum would not notice a few lost rows among 2000, so the cotangents are planted: with
    those of the first 516 096 Gaussians zero, every non-zero row is in the second round and the bound is 1e-5 of
    those rows' own absolute sum; the complement (the last 3000 zero) pins the first round's 12-way unroll with all
    twelve rows of every lane live."""
    n, h, w, spread, smul = FIRST_ROUND + 3000, 16, 32, 1.0, 12.0
    live = slice(FIRST_ROUND, n) if planted == "second round" else slice(0, FIRST_ROUND)
    dead = slice(0, FIRST_ROUND) if planted == "second round" else slice(FIRST_ROUND, n)
    lib, v, means, scales, quats, vm, pm, radii, conics, rec, v_depth = _kernel_case(n, h, w, spread, smul, seed=11,
                                                                                     zero_rows=dead)
    vis = radii > 0
    rows = torch.zeros((n + 255) // 256 * 256, dtype=torch.bool, device=DEV)
    rows[:n] = vis
    rows[dead] = False
    rows = rows.reshape(-1, 256).any(dim=1)                       # slab rows that hold a visible, live Gaussian
    print(f"pose finish, {planted}: {int(vis[live].sum())} visible live Gaussians in {int(rows.sum())} slab rows of "
          f"{rows.numel()}")
    assert not rec[dead].any() and not v_depth[dead].any()
    if planted == "second round":
        assert int(vis[live].sum()) > 100 and not rows[:2016].any() and rows[2016:].any()
    else:                                                         # each of the 12 loads of a lane has live rows
        assert rows[:2016].reshape(12, 168).any(dim=1).all() and not rows[2016:].any()
    got_v, got_p = _pose_bwd(lib, n, v, means, scales, quats, vm, pm, radii, conics, rec, v_depth)
    again_v, again_p = _pose_bwd(lib, n, v, means, scales, quats, vm, pm, radii, conics, rec, v_depth)
    _, gv, gp = _view_bwd(lib, True, n, v, means, scales, quats, vm, pm, radii, conics, rec)
    torch.cuda.synchronize()
    assert torch.equal(gv, got_v) and torch.equal(gp, got_p)                   # the two entries: the same bits
    assert torch.equal(again_v, got_v) and torch.equal(again_p, got_p)         # two calls: the same bits
    want = ref.pose_grads(means, scales, 1.0, quats, vm, pm, v.fx, v.fy, v.cx, v.cy, h, w, vis, rec[:, 0:2], v_depth,
                          rec[:, 2:5])
    for got, key in ((got_v.reshape(3, 4), "viewmat"), (got_p.reshape(4, 4), "projmat")):
        err = (got.double() - want["v_" + key]).abs()
        bound = 1e-5 * want["abs_" + key] + 1e-30
        print(f"pose finish, {planted}, {key}: worst error {(err / bound).max().item():.3e} of its bound")
        assert (err <= bound).all(), (key, err.max().item(), (err / bound).max().item())
        assert want["abs_" + key].max() > 0
    assert (got_p.reshape(4, 4)[2] == 0).all()


def test_pose_entries_write_zeros_for_no_gaussians():
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    out_v, out_p = torch.full((12,), 7.0, device=DEV), torch.full((16,), 7.0, device=DEV)
    z = C.c_void_p(0)
    assert lib.gg_project_pose_bwd(0, z, z, 1.0, z, z, z, 1.0, 1.0, 8, 8, z, z, z, 2, z, z, 3, _ptr(out_v), _ptr(out_p),
                                   z, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert (out_v == 0).all() and (out_p == 0).all()


# ------------------------------------------------------------------------------------------------------------------
# the world-versus-camera identity through ViewGeometry + the fused blend, both backward branches
# ------------------------------------------------------------------------------------------------------------------
def _quat_mul(a, b):
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack((w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2), -1)


def _render(P, means, log_scales, quats, opac, colors, feature, c2w, projmat, view, h, w):
    from gaussiangrasper_amd.pipeline import fused_images
    vm4 = _viewmat(c2w)
    full_proj = projmat @ vm4
    P.clear_bin_cache()
    xys, depths, radii, conics, nth, op, tail, normals, packed = P.ViewGeometry.apply(
        means, log_scales, quats, opac, colors, c2w[:3, 3].detach(), vm4[:3, :], full_proj, view.fx, view.fy, view.cx,
        view.cy, h, w, view.tile_bounds, 4)
    return fused_images(P, xys, depths, radii, conics, nth, op, h, w, feature, None, normals, tail=tail, packed=packed)


def _scene_on_gpu(n, seed):
    sc = make_scene(n, feature_dim=32, config_index=seed).to(DEV)
    sc.scales.data.add_(1.0)
    return sc


@pytest.mark.parametrize("branch", ["fast", "fallback"])
@pytest.mark.parametrize("motion", ["translation", "rotation"])
def test_world_versus_camera_identity(branch, motion):
    """Moving the camera by delta renders what moving every Gaussian by -delta renders, so the gradient of a loss
    with respect to a world-frame camera translation is -sum_i dL/d means_i; for a rotation w about the world origin
    it is the gradient with respect to -w of the means and quaternions rotated by -w (normal cotangent zero: the
    normal image is world-frame).  The camera side runs ViewGeometry's fast branch (gradient sinks, gg_view_bwd_pose)
    or its fallback (gg_project_pose_bwd); the world side is plain autograd through the fallback"""
    from gaussiangrasper_amd import ops as P
    n, h, w = 30000, 120, 160
    view = ring_cameras(4, h, w, device=DEV)[1]
    c2w0, projmat = _c2w_of(view), _projmat(view)
    g = torch.Generator(device="cpu").manual_seed(3)
    prev = P.set_deterministic_backward(True)
    try:
        # camera side
        sc = _scene_on_gpu(n, 7)
        params = [sc.means, sc.scales, sc.quats, sc.opacities, sc.colors_all]
        for p_ in params + [sc.feature]:
            p_.requires_grad_(True)
        bufs = [torch.zeros_like(p_) for p_ in params]
        if branch == "fast":
            for p_, b in zip(params, bufs):
                P.register_grad_sink(p_, b)
        tan = torch.zeros(3, device=DEV, requires_grad=True)
        if motion == "translation":
            c2w = torch.cat((c2w0[:3, :3], c2w0[:3, 3:4] + tan[:, None]), dim=1)
        else:
            from gaussiangrasper_amd.pose import exp_map_so3xr3
            Rw = exp_map_so3xr3(torch.cat((torch.zeros(3, device=DEV), tan))[None])[0, :, :3]
            c2w = Rw @ c2w0[:3, :]
        calls = {}
        from gaussiangrasper_amd import _lib
        lib = _lib.load()
        real = {k: getattr(lib, k) for k in ("gg_view_bwd", "gg_view_bwd_pose", "gg_project_pose_bwd")}
        try:
            for k, f in real.items():
                setattr(lib, k, (lambda f_, k_: (lambda *a: (calls.__setitem__(k_, calls.get(k_, 0) + 1), f_(*a))[1]))(f, k))
            imgs = _render(P, sc.means, sc.scales, sc.quats, sc.opacities, sc.colors_all, sc.feature, c2w, projmat, view,
                           h, w)
            cots = [torch.randn(o.shape, generator=g).to(DEV) for o in imgs]
            if motion == "rotation":
                cots[3].zero_()
            torch.autograd.backward(list(imgs), cots)
            torch.cuda.synchronize()
        finally:
            for k, f in real.items():
                setattr(lib, k, f)
            P.clear_grad_sinks()
        if branch == "fast":
            assert calls == {"gg_view_bwd_pose": 1}, calls
            g_means = bufs[0]
        else:
            assert calls == {"gg_project_pose_bwd": 1}, calls
            g_means = sc.means.grad
        cam_grad = tan.grad.double()
        # world side
        sc2 = _scene_on_gpu(n, 7)
        wt = torch.zeros(3, device=DEV, requires_grad=True)
        if motion == "translation":
            means = sc2.means - wt
            quats = sc2.quats
        else:        # rotated by -w to first order (the gradient at w = 0): p - w x p, [1, -w / 2] (x) q
            means = sc2.means - torch.linalg.cross(wt.expand_as(sc2.means), sc2.means)
            quats = _quat_mul(torch.cat((torch.ones(1, device=DEV), -0.5 * wt))[None], sc2.quats)
        imgs2 = _render(P, means, sc2.scales, quats, sc2.opacities, sc2.colors_all, sc2.feature, c2w0[:3, :], projmat,
                        view, h, w)
        for a, b in zip(imgs, imgs2):
            assert torch.allclose(a.detach(), b.detach(), atol=1e-5)   # the same render (the motions are zero)
        torch.autograd.backward(list(imgs2), cots)
        world_grad = wt.grad.double()
    finally:
        P.set_deterministic_backward(prev)
    if motion == "translation":
        # the same identity against the means' own gradient
        assert torch.allclose(cam_grad, -g_means.double().sum(0), rtol=1e-4, atol=1e-4 * g_means.abs().sum().item())
        scale = g_means.double().abs().sum(0)
    else:
        scale = torch.full((3,), (g_means.double().abs() * sc.means.detach().double().abs().max()).sum().item(),
                           device=DEV)
    err = (cam_grad - world_grad).abs()
    assert cam_grad.abs().max() > 0
    assert (err <= 1e-4 * scale + 1e-6).all(), (motion, branch, cam_grad.tolist(), world_grad.tolist())


# ------------------------------------------------------------------------------------------------------------------
# the default path, determinism
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [True, False])
def test_default_path_launch_and_determinism(deterministic, monkeypatch):
    """pose not requiring grad: gg_view_bwd is the launch taken (no pose launch).  With the pose: two runs give the
    same v_viewmat / v_full_proj bits — through the whole chain under the deterministic blend backward, from the same
    blend cotangents (ViewGeometry's fallback fed directly) in the default mode"""
    from gaussiangrasper_amd import _lib, ops as P
    lib = _lib.load()
    calls = {}
    for k in ("gg_view_bwd", "gg_view_bwd_pose", "gg_project_pose_bwd"):
        f = getattr(lib, k)
        monkeypatch.setattr(lib, k, (lambda f_, k_: (lambda *a: (calls.__setitem__(k_, calls.get(k_, 0) + 1),
                                                                   f_(*a))[1]))(f, k), raising=False)
    n, h, w = 20000, 96, 128
    view = ring_cameras(4, h, w, device=DEV)[2]
    c2w0, projmat = _c2w_of(view), _projmat(view)
    prev = P.set_deterministic_backward(deterministic)
    try:
        sc = _scene_on_gpu(n, 9)
        params = [sc.means, sc.scales, sc.quats, sc.opacities, sc.colors_all]
        for p_ in params + [sc.feature]:
            p_.requires_grad_(True)
        results = []
        for pose in (False, True, True):
            bufs = [torch.zeros_like(p_) for p_ in params]
            for p_, b in zip(params, bufs):
                P.register_grad_sink(p_, b)
            c2w = c2w0[:3, :].clone().requires_grad_(pose)
            calls.clear()
            imgs = _render(P, sc.means, sc.scales, sc.quats, sc.opacities, sc.colors_all, sc.feature, c2w, projmat, view,
                           h, w)
            gen = torch.Generator(device="cpu").manual_seed(4)
            torch.autograd.backward(list(imgs), [torch.randn(o.shape, generator=gen).to(DEV) for o in imgs])
            torch.cuda.synchronize()
            P.clear_grad_sinks()
            assert calls == ({"gg_view_bwd_pose": 1} if pose else {"gg_view_bwd": 1}), calls
            if pose:
                results.append(c2w.grad.clone())
        if deterministic:
            assert torch.equal(results[0], results[1]) and results[0].abs().max() > 0
        # the fallback fed the same cotangents twice (any blend mode): same bits
        outs = []
        for _ in range(2):
            vm4 = _viewmat(c2w0).detach().requires_grad_(True)
            fp = (projmat @ vm4).detach().requires_grad_(True)
            xys, depths, radii, conics, nth, op, tail, normals, packed = P.ViewGeometry.apply(
                sc.means, sc.scales, sc.quats, sc.opacities, sc.colors_all, c2w0[:3, 3], vm4[:3, :], fp, view.fx,
                view.fy, view.cx, view.cy, h, w, view.tile_bounds, 4)
            gen = torch.Generator(device="cpu").manual_seed(5)
            torch.autograd.backward([xys, depths, conics, tail], [torch.randn(t_.shape, generator=gen).to(DEV)
                                                                  for t_ in (xys, depths, conics, tail)])
            outs.append((vm4.grad.clone(), fp.grad.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert (outs[0][0][3] == 0).all() and outs[0][0].abs().max() > 0 and (outs[0][1][2] == 0).all()
    finally:
        P.set_deterministic_backward(prev)
        P.clear_grad_sinks()


# ------------------------------------------------------------------------------------------------------------------
# the public interface
# ------------------------------------------------------------------------------------------------------------------
def _pose_model(n, seed, mode="SO3xR3", num_cameras=4):
    import types
    from gaussiangrasper_amd.plugin import make_fused_model_class
    from gaussiangrasper_amd.stub import StubGaussianSplattingModel, StubPoseCameraOptimizer, default_config
    sc = make_scene(n, feature_dim=32, config_index=seed)
    sc.scales.add_(1.0)
    cfg = default_config(camera_optimizer=types.SimpleNamespace(mode=mode))
    m = make_fused_model_class(StubGaussianSplattingModel)(sc, config=cfg)
    m.camera_optimizer = StubPoseCameraOptimizer(num_cameras, mode)
    return m.to(DEV)


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_plugin_training_view_reaches_the_pose_adjustment(mode):
    """the plugin class with the stand-in camera optimizer: after one training view the camera's row of
    pose_adjustment has a finite, non-zero gradient and the other rows zero (None without the pose VJP)"""
    from gaussiangrasper_amd import ops as P
    from gaussiangrasper_amd.stub import StubCameras
    h, w = 96, 128
    m = _pose_model(20000, 4, mode)
    m.train()
    view = ring_cameras(4, h, w)[2]
    cam = StubCameras.from_view(view, device=DEV, cam_idx=2)
    P.clear_bin_cache()
    out = m(cam)
    loss = out["rgb"].square().mean() + out["depth"].mean() + out["feature"].abs().mean()
    loss.backward()
    g = m.camera_optimizer.pose_adjustment.grad
    assert g is not None
    assert torch.isfinite(g).all() and (g[2] != 0).any()
    assert (g[[0, 1, 3]] == 0).all()
    groups = m.get_param_groups()
    assert groups["camera_opt"] == [m.camera_optimizer.pose_adjustment]


def test_refine_camera_recovers_a_perturbed_pose():
    """render a frame from a true pose, start 1 cm and 1 degree away: refine_camera (Gaussians frozen, deterministic
    backward) cuts the translation and rotation errors by at least 10x within its fixed number of steps"""
    from gaussiangrasper_amd import ops as P
    from gaussiangrasper_amd.pose import refine_camera, exp_map_so3xr3
    from gaussiangrasper_amd.stub import StubCameras
    h, w = 120, 160
    m = _pose_model(40000, 6)
    with torch.no_grad():
        m.scales.add_(1.5)                # a smoother field: a basin wider than a degree of rotation
    view = ring_cameras(4, h, w)[1]
    cam = StubCameras.from_view(view, device=DEV)
    prev = P.set_deterministic_backward(True)
    try:
        m.eval()
        with torch.no_grad():
            P.clear_bin_cache()
            out = m.get_outputs(cam)
            rgb, depth = out["rgb"].detach().clone(), out["depth"].detach().clone()
        true_c2w = cam.camera_to_worlds.detach().clone()
        axis = torch.tensor([0.3, -0.8, 0.5], device=DEV)
        axis = axis / axis.norm()
        pert = torch.cat((torch.tensor([0.006, -0.005, 0.006], device=DEV), axis * math.radians(1.0)))[None]
        adj = exp_map_so3xr3(pert)
        start = true_c2w.clone()
        start[0, :, :3] = true_c2w[0, :, :3] @ adj[0, :, :3]
        start[0, :, 3] = true_c2w[0, :, 3] + true_c2w[0, :, :3] @ adj[0, :, 3]
        cam.camera_to_worlds = start.clone()
        valid = depth.reshape(h, w) < 5.0
        c2w, losses = refine_camera(m, cam, rgb, depth=depth, valid=valid, steps=100)
    finally:
        P.set_deterministic_backward(prev)

    def errors(c):
        dt = (c[0, :, 3] - true_c2w[0, :, 3]).norm().item()
        dR = c[0, :, :3].T @ true_c2w[0, :, :3]
        ang = math.acos(max(-1.0, min(1.0, (dR.trace().item() - 1) / 2)))
        return dt, ang
    t0, r0 = errors(start)
    t1, r1 = errors(c2w)
    print(f"refine_camera: translation {t0:.2e} -> {t1:.2e}, rotation {math.degrees(r0):.3f} -> "
          f"{math.degrees(r1):.4f} deg, loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert 0 < len(losses) <= 100 and min(losses) < losses[0]
    assert torch.equal(cam.camera_to_worlds, start)              # the camera is left as it was
    assert all(p.requires_grad for p in m.parameters()) and not m.training
    assert t1 <= t0 / 10 and r1 <= r0 / 10, (t0, t1, r0, r1)
