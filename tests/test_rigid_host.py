"""Object pose refinement without a GPU: the restatement of the rigid-move kernels
(tests/rigid_ref.py) against fp64 autograd and central differences, pose.object_transform, the CPU route of
ops.RigidMove, the entry points' argument checks, and pose.refine_object recovering a slipped block through the CPU
oracle's renderer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rigid_cases as cases
import rigid_ref as ref


def _quat_mul_t(a, b):
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack((w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2), -1)


def _composite64(means, quats, mask, rt, qt):
    """an independent fp64 torch statement: matrix product, broadcast quaternion product, where()"""
    rt = rt.reshape(3, 4)
    moved = means @ rt[:, :3].T + rt[:, 3]
    turned = _quat_mul_t(qt[None].expand_as(quats), quats)
    sel = torch.ones(len(means), dtype=torch.bool) if mask is None else torch.from_numpy(np.asarray(mask) != 0)
    return torch.where(sel[:, None], moved, means), torch.where(sel[:, None], turned, quats)


@pytest.mark.parametrize("kind", ["null", "every third", "none"])
def test_restated_vjp_equals_fp64_autograd_and_central_differences(kind):
    n = 37
    means, quats, g_m, g_q = [a.astype(np.float64) for a in cases.real_arrays(n, 5)]
    rt, qt = [a.astype(np.float64) for a in cases.pose(5)]
    mask = cases.make_mask(kind, n)
    leaves = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (means, quats, rt, qt)]
    out_m, out_q = _composite64(leaves[0], leaves[1], mask, leaves[2], leaves[3])
    want_m, want_q = ref.forward64(means, quats, mask, rt, qt)
    assert np.abs(out_m.detach().numpy() - want_m).max() <= 1e-12
    assert np.abs(out_q.detach().numpy() - want_q).max() <= 1e-12
    loss = (out_m * torch.from_numpy(g_m)).sum() + (out_q * torch.from_numpy(g_q)).sum()
    loss.backward()
    got = ref.vjp64(means, quats, mask, rt, qt, g_m, g_q)
    for g, leaf, name in zip(got, leaves, ("v_means", "v_quats", "v_rt", "v_qt")):
        err = np.abs(g.reshape(leaf.shape) - leaf.grad.numpy()).max()
        assert err <= 1e-12 * max(1.0, np.abs(leaf.grad.numpy()).max()), (name, err)

    # central differences of the same loss in the pose's sixteen numbers and in a few rows
    def f(m_, q_, rt_, qt_):
        a, b = ref.forward64(m_, q_, mask, rt_, qt_)
        return float((a * g_m).sum() + (b * g_q).sum())
    h = 1e-6
    for k in range(12):
        e = np.zeros(12)
        e[k] = h
        fd = (f(means, quats, rt + e, qt) - f(means, quats, rt - e, qt)) / (2 * h)
        assert abs(fd - got[2].reshape(12)[k]) <= 1e-7 * max(1.0, abs(fd)), ("rt", k)
    for k in range(4):
        e = np.zeros(4)
        e[k] = h
        fd = (f(means, quats, rt, qt + e) - f(means, quats, rt, qt - e)) / (2 * h)
        assert abs(fd - got[3][k]) <= 1e-7 * max(1.0, abs(fd)), ("qt", k)
    for row in (0, 3, n - 1):
        for k in range(3):
            e = np.zeros_like(means)
            e[row, k] = h
            fd = (f(means + e, quats, rt, qt) - f(means - e, quats, rt, qt)) / (2 * h)
            assert abs(fd - got[0][row, k]) <= 1e-7 * max(1.0, abs(fd))
        for k in range(4):
            e = np.zeros_like(quats)
            e[row, k] = h
            fd = (f(means, quats + e, rt, qt) - f(means, quats - e, rt, qt)) / (2 * h)
            assert abs(fd - got[1][row, k]) <= 1e-7 * max(1.0, abs(fd))


def test_ordered_sums_are_exact_on_the_lattice_and_ignore_unselected_rows():
    n = 8449
    means, quats, g_m, g_q = cases.lattice_arrays(n, 2)
    mask = cases.make_mask("every third", n)
    g_m[1] = np.nan                                       # rows 1 and 2 are not selected
    g_q[2] = np.inf
    rt, qt = cases.lattice_pose(2)
    out = ref.backward(means, quats, mask, rt, qt, g_m, g_q)
    got = np.concatenate([out["v_rt"], out["v_qt"]]).astype(np.float64)
    assert np.isfinite(got).all()
    assert np.array_equal(got, out["exact"].astype(np.float32).astype(np.float64))
    assert out["count"] == len(range(0, n, 3))


def test_object_transform_rotation_quaternion_composition_and_gradient_at_zero():
    from oracle_ops import quat_to_rotmat_torch
    from gaussiangrasper_amd.pose import object_transform, rotmat_to_quat
    delta = torch.tensor([0.02, -0.015, 0.01, 0.3, -0.8, 0.5], dtype=torch.float64)
    delta[3:] *= math.radians(40.0) / delta[3:].norm()
    rt, qt = object_transform(delta)
    assert (quat_to_rotmat_torch(qt) - rt[:, :3]).abs().max() <= 1e-12
    assert (rt[:, 3] - delta[:3]).abs().max() == 0
    assert abs(qt.norm().item() - 1) <= 1e-15
    # below the series' threshold too
    rt_s, qt_s = object_transform(delta * 1e-4)
    assert (quat_to_rotmat_torch(qt_s) - rt_s[:, :3]).abs().max() <= 1e-12
    # about a centre, on the left of a base: T x = R (B x - c) + c + t
    base = torch.eye(4, dtype=torch.float64)
    base[:3, :] = object_transform(torch.tensor([0.3, 0.1, -0.2, 1.1, 0.4, -0.7], dtype=torch.float64))[0]
    centre = torch.tensor([0.4, -0.2, 0.1], dtype=torch.float64)
    rt_c, qt_c = object_transform(delta, base=base, centre=centre)
    x = torch.tensor([[0.3, 0.5, -0.1], [1.0, -2.0, 0.7]], dtype=torch.float64)
    bx = x @ base[:3, :3].T + base[:3, 3]
    want = (bx - centre) @ rt[:, :3].T + centre + delta[:3]
    assert (x @ rt_c[:, :3].T + rt_c[:, 3] - want).abs().max() <= 1e-12
    assert (quat_to_rotmat_torch(qt_c) - rt_c[:, :3]).abs().max() <= 1e-12
    assert (quat_to_rotmat_torch(rotmat_to_quat(base[:3, :3])) - base[:3, :3]).abs().max() <= 1e-12
    # rotmat_to_quat's other branches: half turns about each axis and near them
    for axis in range(3):
        w = torch.zeros(6, dtype=torch.float64)
        w[3 + axis] = math.pi - 1e-3
        w[3 + (axis + 1) % 3] = 0.2
        R = object_transform(w)[0][:, :3]
        assert (quat_to_rotmat_torch(rotmat_to_quat(R)) - R).abs().max() <= 1e-12
    # the gradient at delta = 0: finite, and the central difference's
    g = torch.Generator().manual_seed(1)
    c_rt, c_qt = torch.randn(3, 4, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)

    def f(d):
        a, b = object_transform(d, base=base, centre=centre)
        return (a * c_rt).sum() + (b * c_qt).sum()
    zero = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    f(zero).backward()
    assert torch.isfinite(zero.grad).all() and zero.grad.abs().min() > 0
    for k in range(6):
        e = torch.zeros(6, dtype=torch.float64)
        e[k] = 1e-6
        fd = (f(e) - f(-e)).item() / 2e-6
        assert abs(fd - zero.grad[k].item()) <= 1e-8 * max(1.0, abs(fd)), (k, fd, zero.grad[k].item())
    with pytest.raises(ValueError):
        object_transform(delta, mode="nope")


@pytest.mark.parametrize("kind", ["null", "bytes 1 2 255", "none"])
def test_cpu_route_of_rigid_move_equals_the_restatement(kind):
    from gaussiangrasper_amd import ops as P
    n = 300
    means, quats, g_m, g_q = cases.real_arrays(n, 8)
    rt, qt = cases.pose(8)
    mask = cases.make_mask(kind, n)
    leaves = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (means, quats, rt, qt)]
    out_m, out_q = P.RigidMove(leaves[0], leaves[1], None if mask is None else torch.from_numpy(mask), leaves[2],
                               leaves[3])
    want_m, want_q = ref.forward(means, quats, mask, rt, qt)
    assert out_m.dtype == torch.float32 and out_q.dtype == torch.float32
    assert np.array_equal(out_m.detach().numpy().view(np.uint32), want_m.view(np.uint32))
    assert np.array_equal(out_q.detach().numpy().view(np.uint32), want_q.view(np.uint32))
    torch.autograd.backward([out_m, out_q], [torch.from_numpy(g_m), torch.from_numpy(g_q)])
    want = ref.backward(means, quats, mask, rt, qt, g_m, g_q)
    # autograd's fp32 sums are unordered: n 2^-24 of the absolute sums; the rows are one rounding each
    assert np.abs(leaves[0].grad.numpy() - want["v_means"]).max() <= 2.0 ** -22 * np.abs(want["v_means"]).max()
    assert np.abs(leaves[1].grad.numpy() - want["v_quats"]).max() <= 2.0 ** -22 * np.abs(want["v_quats"]).max()
    got = np.concatenate([leaves[2].grad.numpy().reshape(12), leaves[3].grad.numpy()]).astype(np.float64)
    assert (np.abs(got - want["exact"]) <= n * 2.0 ** -24 * want["abs"] + 1e-30).all()


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """validation runs on the host before anything is launched; gg_last_error names the array"""
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    z, p4, p16 = C.c_void_p(0), C.c_void_p(0x1004), C.c_void_p(0x1010)
    assert lib.gg_rigid_bwd_workspace(-1) == 0
    assert lib.gg_rigid_bwd_workspace(0) == 256 and lib.gg_rigid_bwd_workspace(256) == 256
    assert lib.gg_rigid_bwd_workspace(257) == 256 and lib.gg_rigid_bwd_workspace(3 * 256) == 512
    assert lib.gg_rigid_fwd(-1, z, z, z, z, z, z, z, z) == -1 and b"num_points" in lib.gg_last_error()
    assert lib.gg_rigid_fwd(0, z, z, z, z, z, z, z, z) == 0
    for bad, name in ((1, b"means"), (2, b"quats"), (4, b"rt"), (5, b"qt"), (6, b"means_out"), (7, b"quats_out")):
        args = [4, p16, p16, z, p4, p4, p16, p16, z]
        args[bad] = z
        assert lib.gg_rigid_fwd(*args) == -1 and name in lib.gg_last_error(), name
    assert lib.gg_rigid_fwd(4, p16, p4, z, p4, p4, p16, p16, z) == -1 and b"quats misaligned" in lib.gg_last_error()
    assert lib.gg_rigid_fwd(4, p16, p16, z, p4, p4, p16, p4, z) == -1 and b"quats_out misaligned" in lib.gg_last_error()
    assert lib.gg_rigid_fwd(4, C.c_void_p(0x1002), p16, z, p4, p4, p16, p16, z) == -1 \
        and b"means misaligned" in lib.gg_last_error()
    ws = C.c_void_p(0x1100)
    ok = [4, p16, p16, z, p4, p4, p4, p16, p4, p16, p4, p4, ws, 256, z]
    for bad, name in ((1, b"means"), (2, b"quats"), (4, b"rt"), (5, b"qt"), (10, b"v_rt"), (11, b"v_qt")):
        args = list(ok)
        args[bad] = z
        assert lib.gg_rigid_bwd(*args) == -1 and name in lib.gg_last_error(), name
    for bad, name in ((7, b"g_quats"), (9, b"v_quats"), (2, b"quats")):
        args = list(ok)
        args[bad] = p4
        assert lib.gg_rigid_bwd(*args) == -1 and name + b" misaligned" in lib.gg_last_error(), name
    args = list(ok)
    args[12] = C.c_void_p(0x1010)
    assert lib.gg_rigid_bwd(*args) == -1 and b"ws" in lib.gg_last_error()
    args = list(ok)
    args[13] = 128
    assert lib.gg_rigid_bwd(*args) == -3 and b"workspace too small" in lib.gg_last_error()
    assert lib.gg_prof_name(53) == b""                   # no profiling id was added: the bench times with events


def test_plugin_model_has_the_hook_switched_off():
    from gaussiangrasper_amd.plugin import make_fused_model_class
    from gaussiangrasper_amd.stub import StubGaussianSplattingModel
    assert make_fused_model_class(StubGaussianSplattingModel).object_pose is None


def _oracle_render(sc, views):
    import oracle_ops
    from gaussiangrasper_amd.pipeline import render_view

    def render(means, quats, k):
        from gaussiangrasper_amd.scene import Scene
        s = Scene(means, sc.scales, quats, sc.opacities, sc.colors_all, sc.feature)
        return render_view(s, views[k], oracle_ops, sh_degree_to_use=0, channels=("rgb", "depth"))
    return render


def test_refine_object_recovers_a_slipped_block_through_the_cpu_oracle():
    """the L-shaped coloured block on its table, four 72 x 96 views rendered with the block at its true place
    (2.7 cm and 4 degrees from where the scene has it); from the identity, within 40 evaluations of the rgb + depth
    loss, both errors fall by at least 10x (the bar of test_refine_camera_recovers_a_perturbed_pose)"""
    from gaussiangrasper_amd.pose import refine_object
    sc, mask = cases.block_scene()
    views = cases.recovery_views()
    T_true = cases.true_transform()
    truth = cases.moved_scene(T_true)
    render_true = _oracle_render(truth, views)
    with torch.no_grad():
        frames = [render_true(truth.means, truth.quats, k) for k in range(len(views))]
    rgbs = [f["rgb"].detach() for f in frames]
    depths = [f["depth"].detach() for f in frames]
    T, losses = refine_object(_oracle_render(sc, views), mask, [None] * len(views), rgbs, depths=depths, steps=40,
                              means=sc.means, quats=sc.quats)
    t0, r0 = cases.pose_errors(np.eye(4), T_true)
    t1, r1 = cases.pose_errors(T.double().numpy(), T_true)
    print(f"refine_object on the CPU oracle: translation {1e3 * t0:.2f} -> {1e3 * t1:.4f} mm, "
          f"||R - R_true||_F {r0:.3e} -> {r1:.3e}, loss {losses[0]:.3e} -> {losses[-1]:.3e} in {len(losses)} evaluations")
    assert 0 < len(losses) <= 40 and min(losses) < losses[0]
    assert abs(t0 - 0.0269) < 1e-3 and r0 > 0.09
    assert t1 <= t0 / 10 and r1 <= r0 / 10, (t0, t1, r0, r1)
