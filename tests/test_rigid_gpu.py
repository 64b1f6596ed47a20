"""Object pose refinement on the MI355X: gg_rigid_fwd / gg_rigid_bwd against the numpy restatement
(tests/rigid_ref.py) bit for bit, the ordered pose sums, the entry points' memory contract, and the chain on top:
ops.RigidMove + ViewGeometry against the camera-side pose gradient, the plugin hook, and pose.refine_object recovering
a slipped block on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import rigid_cases as cases
import rigid_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _fwd(lib, means, quats, mask, rt, qt):
    n = len(means)
    d = [_dev(a) for a in (means, quats, mask, rt, qt)]
    out_m = torch.full((n, 3), float("nan"), device=DEV)
    out_q = torch.full((n, 4), float("nan"), device=DEV)
    st = lib.gg_rigid_fwd(n, *[_ptr(t) for t in d], _ptr(out_m), _ptr(out_q), _stream())
    assert st == 0, lib.gg_last_error()
    return out_m.cpu().numpy(), out_q.cpu().numpy()


def _bwd(lib, means, quats, mask, rt, qt, g_m, g_q, rows=True, ws_fill=0):
    n = len(means)
    d = [_dev(a) for a in (means, quats, mask, rt, qt, g_m, g_q)]
    v_m = torch.full((n, 3), float("nan"), device=DEV) if rows else None
    v_q = torch.full((n, 4), float("nan"), device=DEV) if rows else None
    v_rt, v_qt = torch.full((12,), float("nan"), device=DEV), torch.full((4,), float("nan"), device=DEV)
    ws = torch.full((max(lib.gg_rigid_bwd_workspace(n), 256),), ws_fill, dtype=torch.uint8, device=DEV)
    st = lib.gg_rigid_bwd(n, *[_ptr(t) for t in d], _ptr(v_m), _ptr(v_q), _ptr(v_rt), _ptr(v_qt), _ptr(ws), ws.numel(),
                          _stream())
    assert st == 0, lib.gg_last_error()
    torch.cuda.synchronize()
    return (None if v_m is None else v_m.cpu().numpy(), None if v_q is None else v_q.cpu().numpy(),
            v_rt.cpu().numpy(), v_qt.cpu().numpy())


@pytest.mark.parametrize("n", cases.SIZES)
def test_kernels_equal_the_restatement(n):
    """every mask at this size.  Forward and per-row backward: the restatement's bits.  The sixteen sums: on lattice
    inputs (every order exact) the restatement's bits; on real inputs within M 2^-52 sum|products| + 2^-24 |s| of the
    exact sum (PARITY.md's bound for reordered fp64 sums plus the one fp32 rounding; M products).  Two calls on
    different workspace garbage: the same bytes.  The pose-only call: the full call's sums."""
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    for mi, kind in enumerate(cases.MASKS):
        mask = cases.make_mask(kind, n)
        for lattice in (True, False):
            seed = 100 * n + 2 * mi + lattice
            means, quats, g_m, g_q = (cases.lattice_arrays if lattice else cases.real_arrays)(n, seed)
            rt, qt = cases.lattice_pose(seed) if lattice else cases.pose(seed)
            what = (n, kind, "lattice" if lattice else "real")
            got_m, got_q = _fwd(lib, means, quats, mask, rt, qt)
            want_m, want_q = ref.forward(means, quats, mask, rt, qt)
            assert np.array_equal(_bits(got_m), _bits(want_m)), what
            assert np.array_equal(_bits(got_q), _bits(want_q)), what
            want = ref.backward(means, quats, mask, rt, qt, g_m, g_q)
            v_m, v_q, v_rt, v_qt = _bwd(lib, means, quats, mask, rt, qt, g_m, g_q, ws_fill=0xFF)
            assert np.array_equal(_bits(v_m), _bits(want["v_means"])), what
            assert np.array_equal(_bits(v_q), _bits(want["v_quats"])), what
            got = np.concatenate([v_rt, v_qt])
            if lattice:
                assert np.array_equal(_bits(got), _bits(np.concatenate([want["v_rt"], want["v_qt"]]))), what
                assert np.array_equal(got.astype(np.float64), want["exact"].astype(np.float32).astype(np.float64)), what
            else:
                m_terms = want["count"] * np.array([1.0] * 12 + [4.0] * 4)
                bound = m_terms * 2.0 ** -52 * want["abs"] + 2.0 ** -24 * np.abs(want["exact"])
                err = np.abs(got.astype(np.float64) - want["exact"])
                assert (err <= bound).all(), (what, (err / np.maximum(bound, 1e-300)).max())
            if want["count"] == 0:
                assert not got.any(), what
            _, _, rt2, qt2 = _bwd(lib, means, quats, mask, rt, qt, g_m, g_q, ws_fill=0x5A)
            assert np.array_equal(_bits(rt2), _bits(v_rt)) and np.array_equal(_bits(qt2), _bits(v_qt)), what
            m3, q3, rt3, qt3 = _bwd(lib, means, quats, mask, rt, qt, g_m, g_q, rows=False, ws_fill=0x11)
            assert m3 is None and q3 is None
            assert np.array_equal(_bits(rt3), _bits(v_rt)) and np.array_equal(_bits(qt3), _bits(v_qt)), what


def test_missing_cotangents_and_nan_in_unselected_rows():
    """g_means or g_quats NULL is zeros; a NaN / inf cotangent in a row that is not selected is copied to that row's
    output and stays out of the sums"""
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = 4097
    means, quats, g_m, g_q = cases.real_arrays(n, 3)
    rt, qt = cases.pose(3)
    mask = cases.make_mask("every third", n)
    g_m[1], g_q[2], g_m[4094] = np.nan, np.inf, -np.inf                  # rows 1, 2 and 4094: not selected
    assert not mask[[1, 2, 4094]].any()
    want = ref.backward(means, quats, mask, rt, qt, g_m, g_q)
    v_m, v_q, v_rt, v_qt = _bwd(lib, means, quats, mask, rt, qt, g_m, g_q)
    assert np.isfinite(v_rt).all() and np.isfinite(v_qt).all()
    assert np.array_equal(_bits(v_m), _bits(want["v_means"])) and np.array_equal(_bits(v_q), _bits(want["v_quats"]))
    assert np.isnan(v_m[1]).all() and np.isinf(v_q[2]).all()
    for gm, gq in ((None, g_q), (g_m, None), (None, None)):
        want = ref.backward(means, quats, mask, rt, qt, gm, gq)
        v_m, v_q, v_rt, v_qt = _bwd(lib, means, quats, mask, rt, qt, gm, gq)
        assert np.array_equal(_bits(v_m), _bits(want["v_means"])) and np.array_equal(_bits(v_q), _bits(want["v_quats"]))
        got = np.concatenate([v_rt, v_qt]).astype(np.float64)
        m_terms = want["count"] * np.array([1.0] * 12 + [4.0] * 4)
        assert (np.abs(got - want["exact"]) <= m_terms * 2.0 ** -52 * want["abs"] + 2.0 ** -24 * np.abs(want["exact"])).all()
        if gm is None:
            assert not v_rt.any()
        if gq is None:
            assert not v_qt.any()


def test_memory_contract_in_a_sentinel_arena():
    """every array at exactly its stated alignment between guards: the calls write their outputs and nothing else,
    a misaligned quats is refused with nothing written, and the empty backward writes sixteen zeros only"""
    from arena import Arena
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    n = 4097
    means, quats, g_m, g_q = cases.real_arrays(n, 9)
    rt, qt = cases.pose(9)
    mask = cases.make_mask("bytes 1 2 255", n)

    def arena(seed):
        a = Arena(DEV, seed)
        a.carve("means", means, 4, "in").carve("quats", quats, 16, "in").carve("mask", mask, 1, "in")
        a.carve("rt", rt, 4, "in").carve("qt", qt, 4, "in").carve("g_means", g_m, 4, "in")
        a.carve("g_quats", g_q, 16, "in")
        a.carve("means_out", means, 4, "out").carve("quats_out", quats, 16, "out")
        a.carve("v_means", means, 4, "out").carve("v_quats", quats, 16, "out")
        a.carve("v_rt", rt, 4, "out").carve("v_qt", qt, 4, "out")
        a.carve("ws", int(lib.gg_rigid_bwd_workspace(n)), 256, "ws")
        return a

    def fwd_args(a, quats_ptr=None):
        return [n, a.ptr("means"), quats_ptr or a.ptr("quats"), a.ptr("mask"), a.ptr("rt"), a.ptr("qt"),
                a.ptr("means_out"), a.ptr("quats_out"), _stream()]

    def bwd_args(a, count=n, quats_ptr=None):
        return [count, a.ptr("means"), quats_ptr or a.ptr("quats"), a.ptr("mask"), a.ptr("rt"), a.ptr("qt"),
                a.ptr("g_means"), a.ptr("g_quats"), a.ptr("v_means"), a.ptr("v_quats"), a.ptr("v_rt"), a.ptr("v_qt"),
                a.ptr("ws"), a.nbytes("ws"), _stream()]

    a = arena(1)
    assert lib.gg_rigid_fwd(*fwd_args(a)) == 0, lib.gg_last_error()
    out = a.check()
    want_m, want_q = ref.forward(means, quats, mask, rt, qt)
    assert np.array_equal(_bits(out["means_out"]), _bits(want_m)) and np.array_equal(_bits(out["quats_out"]), _bits(want_q))
    for k in ("v_means", "v_quats", "v_rt", "v_qt"):
        assert np.array_equal(out[k].view(np.uint8), a.sentinel_like(k).view(np.uint8)), k
    a.rebase()
    assert lib.gg_rigid_bwd(*bwd_args(a)) == 0, lib.gg_last_error()
    out = a.check()
    want = ref.backward(means, quats, mask, rt, qt, g_m, g_q)
    assert np.array_equal(_bits(out["v_means"]), _bits(want["v_means"]))
    assert np.array_equal(_bits(out["v_quats"]), _bits(want["v_quats"]))
    assert np.array_equal(_bits(out["means_out"]), _bits(want_m))          # the forward's outputs: not touched again
    first = (out["v_rt"].copy(), out["v_qt"].copy())
    b = arena(2)                                                           # other workspace garbage: the same bytes
    assert lib.gg_rigid_bwd(*bwd_args(b)) == 0, lib.gg_last_error()
    out_b = b.check()
    assert np.array_equal(_bits(out_b["v_rt"]), _bits(first[0])) and np.array_equal(_bits(out_b["v_qt"]), _bits(first[1]))
    # refused: quats four bytes off its alignment
    c = arena(3)
    off = C.c_void_p(c.address("quats") + 4)
    assert lib.gg_rigid_fwd(*fwd_args(c, off)) == -1 and b"quats misaligned" in lib.gg_last_error()
    assert lib.gg_rigid_bwd(*bwd_args(c, quats_ptr=off)) == -1 and b"quats misaligned" in lib.gg_last_error()
    assert c.untouched()
    # empty: sixteen zeros and nothing else
    assert lib.gg_rigid_fwd(0, *fwd_args(c)[1:]) == 0
    assert c.untouched()
    assert lib.gg_rigid_bwd(*bwd_args(c, count=0)) == 0, lib.gg_last_error()
    out_c = c.check()
    assert not out_c["v_rt"].any() and not out_c["v_qt"].any()
    for k in ("means_out", "quats_out", "v_means", "v_quats"):
        assert np.array_equal(out_c[k].view(np.uint8), c.sentinel_like(k).view(np.uint8)), k
    assert np.array_equal(out_c["ws"], c.before("ws"))


# ------------------------------------------------------------------------------------------------------------------
# the chain: RigidMove + ViewGeometry + the fused blend
# ------------------------------------------------------------------------------------------------------------------
def _chain_grad(P, n, h, w, side, seed_cot=3, frozen=False):
    """d loss / d delta at delta = 0 of a random-cotangent loss (normal cotangent zero: the normal image is
    world-frame).  side "world": every Gaussian moved by object_transform(delta) through RigidMove, the camera fixed;
    side "camera": the camera moved, c2w = object_transform(delta) c2w0.  Also the means' own gradient (world side,
    not frozen)."""
    from test_pose_grad_gpu import _c2w_of, _projmat, _render, _scene_on_gpu
    from gaussiangrasper_amd.camera import ring_cameras
    from gaussiangrasper_amd.pose import object_transform
    view = ring_cameras(4, h, w, device=DEV)[1]
    c2w0, projmat = _c2w_of(view), _projmat(view)
    sc = _scene_on_gpu(n, 7)
    delta = torch.zeros(6, device=DEV, requires_grad=True)
    rt, qt = object_transform(delta)
    if side == "world":
        sc.means.requires_grad_(not frozen)
        means, quats = P.RigidMove(sc.means, sc.quats, None, rt, qt)
        c2w = c2w0[:3, :]
    else:
        means, quats = sc.means, sc.quats
        c2w = rt @ c2w0
    imgs = _render(P, means, sc.scales, quats, sc.opacities, sc.colors_all, sc.feature, c2w, projmat, view, h, w)
    g = torch.Generator(device="cpu").manual_seed(seed_cot)
    cots = [torch.randn(o.shape, generator=g).to(DEV) for o in imgs]
    cots[3].zero_()
    torch.autograd.backward(list(imgs), cots)
    torch.cuda.synchronize()
    return delta.grad.clone(), sc.means.grad, sc.means.detach(), [i.detach() for i in imgs]


def test_world_against_camera():
    """moving every Gaussian by D renders what moving the camera by D^-1 renders, so at D = identity the gradient with
    respect to delta through RigidMove + ViewGeometry is minus the camera-side gradient of the existing pose VJP.
    Scene, sizes and bar of test_pose_grad_gpu.py::test_world_versus_camera_identity"""
    from gaussiangrasper_amd import ops as P
    n, h, w = 30000, 120, 160
    prev = P.set_deterministic_backward(True)
    try:
        world, g_means, means, imgs_w = _chain_grad(P, n, h, w, "world")
        cam, _, _, imgs_c = _chain_grad(P, n, h, w, "camera")
    finally:
        P.set_deterministic_backward(prev)
    for a, b in zip(imgs_w, imgs_c):
        assert torch.allclose(a, b, atol=1e-5)                     # the same render: both motions are zero
    t_scale = g_means.double().abs().sum(0)
    r_scale = torch.full((3,), (g_means.double().abs() * means.double().abs().max()).sum().item(), device=DEV)
    scale = torch.cat((t_scale, r_scale))
    err = (world.double() + cam.double()).abs()
    print("world against camera: d/d delta", world.tolist(), "camera side", cam.tolist(),
          "worst error / bound", (err / (1e-4 * scale + 1e-6)).max().item())
    assert world.abs().min() > 0
    # the translation part is the means' own gradient, summed
    assert torch.allclose(world[:3].double(), g_means.double().sum(0), rtol=1e-4, atol=1e-4 * g_means.abs().sum().item())
    assert (err <= 1e-4 * scale + 1e-6).all(), (world.tolist(), cam.tolist())


def test_same_bits_twice():
    """two runs under the deterministic blend backward, Gaussians frozen (the pose-only rigid backward): the same
    delta.grad bits"""
    from gaussiangrasper_amd import ops as P
    prev = P.set_deterministic_backward(True)
    try:
        a, none, _, _ = _chain_grad(P, 30000, 120, 160, "world", frozen=True)
        b, _, _, _ = _chain_grad(P, 30000, 120, 160, "world", frozen=True)
    finally:
        P.set_deterministic_backward(prev)
    assert none is None and a.abs().min() > 0
    assert torch.equal(a, b)


def _spy(monkeypatch, lib, calls):
    for k in ("gg_rigid_fwd", "gg_rigid_bwd"):
        f = getattr(lib, k)
        monkeypatch.setattr(lib, k, (lambda f_, k_: (lambda *a: (calls.__setitem__(k_, calls.get(k_, 0) + 1),
                                                                   f_(*a))[1]))(f, k), raising=False)


def test_plugin_hook_off_and_identity(monkeypatch):
    """object_pose None: no gg_rigid_* call; an identity pose on a subset: one gg_rigid_fwd, and the same image bytes"""
    from test_pose_grad_gpu import _pose_model
    from gaussiangrasper_amd import _lib, ops as P
    from gaussiangrasper_amd.camera import ring_cameras
    from gaussiangrasper_amd.stub import StubCameras
    lib = _lib.load()
    calls = {}
    _spy(monkeypatch, lib, calls)
    m = _pose_model(20000, 4)
    m.eval()
    assert m.object_pose is None
    cam = StubCameras.from_view(ring_cameras(4, 96, 128)[2], device=DEV)

    def images():
        out = m.get_outputs(cam)
        return {k: out[k].clone() for k in ("rgb", "depth", "feature", "normal")}
    with torch.no_grad():
        P.clear_bin_cache()
        off = images()
        assert calls == {}
        mask = torch.zeros(m.means.shape[0], dtype=torch.uint8, device=DEV)
        mask[::3] = 1
        m.object_pose = (mask, torch.eye(4, device=DEV)[:3], torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV))
        P.clear_bin_cache()
        on = images()
        assert calls == {"gg_rigid_fwd": 1}, calls
        m.object_pose = None
        P.clear_bin_cache()
        again = images()
        assert calls == {"gg_rigid_fwd": 1}, calls
    for k in off:
        assert torch.equal(off[k], on[k]) and torch.equal(off[k], again[k]), k
        assert off[k].abs().max() > 0


def test_refine_object_recovers_a_slipped_block_on_the_device():
    """tests/test_rigid_host.py's fixture and bar on the device, through the plugin model and its hook: frames rendered
    with the block at its true place, the model holding it 2.7 cm and 4 degrees away; 40 evaluations, both errors
    down by at least 10x"""
    from gaussiangrasper_amd import ops as P
    from gaussiangrasper_amd.plugin import make_fused_model_class
    from gaussiangrasper_amd.pose import refine_object
    from gaussiangrasper_amd.scene import Scene
    from gaussiangrasper_amd.stub import StubCameras, StubGaussianSplattingModel, default_config

    def model_of(sc):
        n = sc.means.shape[0]
        colors = torch.zeros(n, 25, 3)
        colors[:, 0] = sc.colors_all[:, 0]
        full = Scene(sc.means, sc.scales, sc.quats, sc.opacities, colors, torch.zeros(n, 32))
        return make_fused_model_class(StubGaussianSplattingModel)(full, config=default_config()).to(DEV)

    sc, mask = cases.block_scene()
    T_true = cases.true_transform()
    cams = [StubCameras.from_view(v, device=DEV) for v in cases.recovery_views()]
    prev = P.set_deterministic_backward(True)
    try:
        truth = model_of(cases.moved_scene(T_true)).eval()
        with torch.no_grad():
            frames = []
            for cam in cams:
                P.clear_bin_cache()
                out = truth.get_outputs(cam)
                frames.append((out["rgb"].detach().clone(), out["depth"].detach().clone()))
        m = model_of(sc)
        m.train()
        before = (m.means.detach().clone(), m.quats.detach().clone())
        T, losses = refine_object(m, mask.to(DEV), cams, [f[0] for f in frames], depths=[f[1] for f in frames], steps=40)
    finally:
        P.set_deterministic_backward(prev)
    t0, r0 = cases.pose_errors(np.eye(4), T_true)
    t1, r1 = cases.pose_errors(T.double().cpu().numpy(), T_true)
    print(f"refine_object on the device: translation {1e3 * t0:.2f} -> {1e3 * t1:.4f} mm, ||R - R_true||_F {r0:.3e} -> "
          f"{r1:.3e}, loss {losses[0]:.3e} -> {min(losses):.3e} in {len(losses)} evaluations")
    assert 0 < len(losses) <= 40 and min(losses) < losses[0]
    assert m.object_pose is None and m.training and all(p.requires_grad for p in m.parameters())
    assert torch.equal(m.means.detach(), before[0]) and torch.equal(m.quats.detach(), before[1])
    assert t1 <= t0 / 10 and r1 <= r0 / 10, (t0, t1, r0, r1)


def test_cli_refines_the_reported_pose_change(tmp_path):
    """python -m gaussiangrasper_amd.edit --refine-transforms on a synthetic checkpoint: the arm reports a pose change,
    the block slipped 2.7 cm and 4 degrees on top of it, the frames (8-bit PNGs, depth .npy in the scan's metres, the
    scan's frame 1 / 0.8 of the checkpoint's) show where it really is.  This is a test of the plumbing — cameras,
    frames, depth units, the composed transform written through the exact move — so the bar is only that both errors
    at least halve against the unrefined edit: a mis-read camera or depth scale pulls the fit away instead."""
    pytest.importorskip("scipy")
    import json
    from PIL import Image
    from gaussiangrasper_amd import edit, interop, ops as P
    from gaussiangrasper_amd.pipeline import render_view
    from gaussiangrasper_amd.pose import rotmat_to_quat
    from gaussiangrasper_amd.scene import Scene
    sc, _ = cases.block_scene()
    n = sc.means.shape[0]
    colors = torch.zeros(n, 25, 3)
    colors[:, 0] = sc.colors_all[:, 0]
    full = Scene(sc.means, sc.scales, sc.quats, sc.opacities, colors, torch.zeros(n, 32))
    ck = tmp_path / "step-000029999.ckpt"
    torch.save({"step": 29999, "pipeline": interop.state_dict_from_scene(full, {"layers.0.weight": torch.randn(128, 32)}),
                "optimizers": {}, "schedulers": {}, "scalers": {}}, ck)
    scale = 0.8
    (tmp_path / "transform.json").write_text(json.dumps({"transform_matrix": np.eye(4).tolist(), "scale": scale}))
    obj = sc.means[:270].double().numpy() / scale                      # the block's points in the scan's frame
    np.save(tmp_path / "obj.npy", obj)
    pose_from, pose_to = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.1, 0.06, 0.0, 0.0, 0.0, 0.25]
    base = np.eye(4)
    base[:3] = edit.compose_transform(np.eye(4), scale, pose_from, pose_to).astype(np.float64)
    planes = edit.hull_planes(edit.filter_object_points(edit.object_points_to_scene(obj, np.eye(4), scale)))
    mask, count = edit.select_and_move(sc.means.to(DEV).contiguous(), None, planes)
    mask = mask.cpu().numpy()
    assert int(count.item()) > 200
    # the truth: the slip of rigid_cases about the moved centroid, on the left of the reported motion
    c = base[:3, :3] @ sc.means[torch.from_numpy(mask != 0)].double().mean(dim=0).numpy() + base[:3, 3]
    slip = cases.true_transform()
    slip[:3, 3] = c - slip[:3, :3] @ c + np.asarray(cases.TRUE_T)
    T_true = slip @ base
    qt = rotmat_to_quat(torch.from_numpy(T_true[:3, :3])).numpy()
    m64, q64 = ref.forward64(sc.means.numpy(), sc.quats.numpy(), mask, T_true[:3].reshape(12), qt)
    truth = Scene(torch.from_numpy(m64.astype(np.float32)), full.scales, torch.from_numpy(q64.astype(np.float32)),
                  full.opacities, full.colors_all, full.feature).to(DEV)
    views = cases.recovery_views(DEV)
    frames = []
    (tmp_path / "after" / "images").mkdir(parents=True)
    (tmp_path / "after" / "depths").mkdir()
    for k, v in enumerate(views):
        with torch.no_grad():
            P.clear_bin_cache()
            out = render_view(truth, v, P, sh_degree_to_use=4, channels=("rgb", "depth"))
        rgb = (out["rgb"].clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
        Image.fromarray(rgb).save(tmp_path / "after" / "images" / f"frame_{k:05d}.png")
        np.save(tmp_path / "after" / "depths" / f"frame_{k:05d}.npy", out["depth"][..., 0].cpu().numpy() / scale)
        c2w = np.eye(4)
        c2w[:3, :3] = v.viewmat[:3, :3].T.double().cpu().numpy()      # OpenCV axes: the operators' world -> camera, inverted
        c2w[:3, 3] = v.cam_pos.double().cpu().numpy() / scale
        frames.append({"file_path": f"images/frame_{k:05d}.png", "transform_matrix": c2w.tolist()})
    v0 = views[0]
    (tmp_path / "after" / "transforms.json").write_text(json.dumps(
        {"fl_x": v0.fx, "fl_y": v0.fy, "cx": v0.cx, "cy": v0.cy, "w": v0.width, "h": v0.height, "frames": frames}))
    common = ["--ckpt", str(ck), "--object-points", str(tmp_path / "obj.npy"), "--transform-json",
              str(tmp_path / "transform.json"), "--pose-from", *map(str, pose_from), "--pose-to", *map(str, pose_to)]
    plain, refined = tmp_path / "plain.ckpt", tmp_path / "refined.ckpt"
    assert edit.main(common + ["--out", str(plain)]) == 0
    assert edit.main(common + ["--out", str(refined), "--refine-transforms", str(tmp_path / "after" / "transforms.json"),
                               "--refine-depth", str(tmp_path / "after" / "depths"), "--refine-steps", "40"]) == 0
    sel = mask != 0

    def errors(path):
        got = torch.load(path, weights_only=True)["pipeline"][interop.MODEL_PREFIX + "means"].double().numpy()
        d = got[sel] - m64[sel]
        centred = d - d.mean(axis=0)
        return float(np.linalg.norm(d.mean(axis=0))), float(np.sqrt((centred ** 2).sum(axis=1).mean()))
    t0, r0 = errors(plain)
    t1, r1 = errors(refined)
    print(f"edit --refine-transforms: centroid error {1e3 * t0:.2f} -> {1e3 * t1:.3f} mm, residual after the centroid "
          f"(rotation) {1e3 * r0:.2f} -> {1e3 * r1:.3f} mm rms")
    got = torch.load(refined, weights_only=True)["pipeline"][interop.MODEL_PREFIX + "means"].numpy()
    assert np.array_equal(got[~sel], sc.means.numpy()[~sel])          # the rest of the scene: not touched
    assert abs(t0 - 0.0269) < 2e-3
    assert t1 <= t0 / 2 and r1 <= r0 / 2, (t0, t1, r0, r1)
    with pytest.raises(SystemExit):
        edit.main(common + ["--out", str(plain), "--refine-steps", "3"])


def test_edit_model_refines_then_moves():
    """edit.edit_model(..., refine=...): the hull's Gaussians are re-localised against the frames (the plugin model
    and its hook), then moved by the composed transform through the exact path.  The host fixture with a reported
    motion underneath the slip; the fixture's 10x bar, on the moved means themselves"""
    from gaussiangrasper_amd import edit, ops as P
    from gaussiangrasper_amd.plugin import make_fused_model_class
    from gaussiangrasper_amd.pose import rotmat_to_quat
    from gaussiangrasper_amd.scene import Scene
    from gaussiangrasper_amd.stub import StubCameras, StubGaussianSplattingModel, default_config

    def model_of(means, quats, sc):
        n = means.shape[0]
        colors = torch.zeros(n, 25, 3)
        colors[:, 0] = sc.colors_all[:, 0]
        full = Scene(means, sc.scales, quats, sc.opacities, colors, torch.zeros(n, 32))
        return make_fused_model_class(StubGaussianSplattingModel)(full, config=default_config()).to(DEV)

    sc, _ = cases.block_scene()
    lo, hi = np.array([-0.3, -0.12, -0.195]), np.array([0.3, 0.12, 0.3])         # the block, not the table under it
    planes = np.concatenate([np.concatenate([np.eye(3), -hi[:, None]], axis=1),
                             np.concatenate([-np.eye(3), lo[:, None]], axis=1)])
    base = np.eye(4)
    base[:3] = edit.compose_transform(np.eye(4), 1.0, [0.0] * 6, [0.1, 0.06, 0.0, 0.0, 0.0, 0.25]).astype(np.float64)
    mask, count = edit.select_and_move(sc.means.to(DEV).contiguous(), None, planes)
    mask = mask.cpu().numpy()
    sel = mask != 0
    assert 200 < int(count.item()) <= 270 and not sel[270:].any()
    c = base[:3, :3] @ sc.means[torch.from_numpy(sel)].double().mean(dim=0).numpy() + base[:3, 3]
    slip = cases.true_transform()
    slip[:3, 3] = c - slip[:3, :3] @ c + np.asarray(cases.TRUE_T)
    T_true = slip @ base
    m64, q64 = ref.forward64(sc.means.numpy(), sc.quats.numpy(), mask, T_true[:3].reshape(12),
                             rotmat_to_quat(torch.from_numpy(T_true[:3, :3])).numpy())
    cams = [StubCameras.from_view(v, device=DEV) for v in cases.recovery_views()]
    truth = model_of(torch.from_numpy(m64.astype(np.float32)), torch.from_numpy(q64.astype(np.float32)), sc).eval()
    frames = []
    with torch.no_grad():
        for cam in cams:
            P.clear_bin_cache()
            out = truth.get_outputs(cam)
            frames.append((out["rgb"].detach().clone(), out["depth"].detach().clone()))

    def errors(model):
        d = model.means.detach().double().cpu().numpy()[sel] - m64[sel]
        centred = d - d.mean(axis=0)
        return float(np.linalg.norm(d.mean(axis=0))), float(np.sqrt((centred ** 2).sum(axis=1).mean()))
    plain, refined = model_of(sc.means, sc.quats, sc), model_of(sc.means, sc.quats, sc)
    assert edit.edit_model(plain, planes, base[:3]) == int(count.item())
    n_sel = edit.edit_model(refined, planes, base[:3], refine=dict(cameras=cams, rgbs=[f[0] for f in frames],
                                                                   depths=[f[1] for f in frames], steps=40))
    assert n_sel == int(count.item()) and refined.object_pose is None
    t0, r0 = errors(plain)
    t1, r1 = errors(refined)
    print(f"edit_model(refine=): centroid error {1e3 * t0:.2f} -> {1e3 * t1:.3f} mm, residual after the centroid "
          f"{1e3 * r0:.2f} -> {1e3 * r1:.3f} mm rms")
    assert torch.equal(refined.means.detach()[270:].cpu(), sc.means[270:])
    assert t1 <= t0 / 10 and r1 <= r0 / 10, (t0, t1, r0, r1)
