"""The host side of the operators (gaussiangrasper_amd/ops.py): which C entry points a training step calls, in which
order, on each route through the operators, and the one branch of the deferred SH gradient that the parity tests do
not reach (views of a step that use different SH degrees)."""
import numpy as np
import pytest
import torch

from gaussiangrasper_amd.camera import ring_cameras
from gaussiangrasper_amd.pipeline import backward_view, fused_images, render_view, seeded_cotangents
from gaussiangrasper_amd.scene import make_scene

N, H, W, VIEWS, FEATURE_DIM = 3000, 48, 64, 3, 32


def _gg(names):
    return ["gg_" + n for n in names.split()]


# Recorded on the parent of the change that introduced ops.GradSink (commit 92e4167, "Pin fused Adam and the row
# kernels on ragged, unaligned layouts") and never on the code under test: one list per view of the step.
EXPECTED_CALLS = {
    "node-deferred": [
        _gg("blend_workspace view_fwd shade_tail_fwd bin_sort_workspace bin_sort blend_workspace "
            "blend_fwd_pair_packed blend_bwd_pair view_bwd"),
        _gg("blend_workspace view_fwd shade_tail_fwd bin_sort_workspace bin_sort_dev_ex blend_workspace "
            "blend_fwd_pair_packed blend_bwd_pair view_bwd"),
        _gg("blend_workspace view_fwd shade_tail_fwd bin_sort_workspace bin_sort_dev_ex blend_workspace "
            "blend_fwd_pair_packed blend_bwd_pair view_bwd sh_bwd_multi"),
    ],
    "node-immediate": [
        _gg("blend_workspace view_fwd shade_tail_fwd bin_sort_workspace bin_sort blend_workspace "
            "blend_fwd_pair_packed blend_bwd_pair view_bwd sh_bwd_multi"),
        _gg("blend_workspace view_fwd shade_tail_fwd bin_sort_workspace bin_sort_dev_ex blend_workspace "
            "blend_fwd_pair_packed blend_bwd_pair view_bwd sh_bwd_multi"),
        _gg("blend_workspace view_fwd shade_tail_fwd bin_sort_workspace bin_sort_dev_ex blend_workspace "
            "blend_fwd_pair_packed blend_bwd_pair view_bwd sh_bwd_multi"),
    ],
    "chain-deferred": [
        _gg("activate_fwd project_count_workspace project_fwd_count shade_tail_fwd bin_sort_workspace bin_sort "
            "blend_workspace blend_fwd_pair_fast blend_bwd_pair shade_tail_bwd_split project_bwd_ex "
            "activate_bwd_ex"),
        _gg("activate_fwd project_count_workspace project_fwd_count shade_tail_fwd bin_sort_workspace "
            "bin_sort_dev_ex blend_workspace blend_fwd_pair_fast blend_bwd_pair shade_tail_bwd_split "
            "project_bwd_ex activate_bwd_ex"),
        _gg("activate_fwd project_count_workspace project_fwd_count shade_tail_fwd bin_sort_workspace "
            "bin_sort_dev_ex blend_workspace blend_fwd_pair_fast blend_bwd_pair shade_tail_bwd_split sh_bwd_multi "
            "project_bwd_ex activate_bwd_ex"),
    ],
    "shim": [
        _gg("quat_to_rotmat_fwd project_count_workspace project_fwd_count sh_fwd bin_sort_workspace bin_sort "
            "blend_workspace blend_fwd blend_workspace blend_fwd blend_workspace blend_fwd blend_workspace "
            "blend_fwd blend_bwd blend_bwd blend_bwd blend_bwd sh_bwd project_bwd_ex quat_to_rotmat_bwd"),
        _gg("quat_to_rotmat_fwd project_count_workspace project_fwd_count sh_fwd bin_sort_workspace "
            "bin_sort_dev_ex blend_workspace blend_fwd blend_workspace blend_fwd blend_workspace blend_fwd "
            "blend_workspace blend_fwd blend_bwd blend_bwd blend_bwd blend_bwd sh_bwd project_bwd_ex "
            "quat_to_rotmat_bwd"),
        _gg("quat_to_rotmat_fwd project_count_workspace project_fwd_count sh_fwd bin_sort_workspace "
            "bin_sort_dev_ex blend_workspace blend_fwd blend_workspace blend_fwd blend_workspace blend_fwd "
            "blend_workspace blend_fwd blend_bwd blend_bwd blend_bwd blend_bwd sh_bwd project_bwd_ex "
            "quat_to_rotmat_bwd"),
    ],
}


def _record_step(route):
    """Ordered names of every gg_* entry point called during one three-view step on `route`, one list per view (the
    last one includes what the end of the step enqueues)."""
    from gaussiangrasper_amd import _lib, ops as P
    from gaussiangrasper_amd.dist import GradBucket
    dev = torch.device("cuda:0")
    lib = _lib.load()
    names = [k for k in _lib.SIGNATURES if k.startswith("gg_")]
    real = {k: getattr(lib, k) for k in names}
    calls = []

    def recorder(name, fn):
        def call(*a):
            calls.append(name)
            return fn(*a)
        return call

    sc = make_scene(N, feature_dim=FEATURE_DIM, config_index=5).to(dev)
    sc.scales.data.add_(1.2)               # bigger splats at this tiny resolution: no empty tile list
    for p_ in sc.params():
        p_.requires_grad_(True)
    views = ring_cameras(VIEWS, H, W, device=dev)
    per_view = []
    prev_hint, prev_exact, prev_det = P._capacity_hint, P.set_exact_forward(False), P.set_deterministic_backward(False)
    P._capacity_hint = {}                  # the first view sizes its lists exactly, the later ones speculatively
    P.clear_bin_cache()
    P.clear_grad_sinks()
    bucket = None
    if route != "shim":
        bucket = GradBucket(sc.params())
        bucket.enable_direct(P, defer_sh=(route != "node-immediate"))
        bucket.zero_()
    for k in names:
        setattr(lib, k, recorder(k, real[k]))
    try:
        for k, v in enumerate(views):
            if bucket is not None and k == VIEWS - 1:
                bucket.arm()
            cam = v.cam_pos.to(dev).reshape(-1)[:3]
            if route == "shim":
                out = render_view(sc, v, P, fused=False)
                backward_view(out, seeded_cotangents(out, seed=k))
            else:
                packed = None
                if route.startswith("node"):
                    xys, depths, radii, conics, nth, opac, tail, normals, packed = P.ViewGeometry.apply(
                        sc.means, sc.scales, sc.quats, sc.opacities, sc.colors_all, cam, v.viewmat[:3, :], v.projmat,
                        v.fx, v.fy, v.cx, v.cy, H, W, v.tile_bounds, 4)
                else:
                    scales_e, quats_n, opac, viewdirs, normals = P.ActivateGaussians.apply(
                        sc.means, sc.scales, sc.quats, sc.opacities, cam)
                    xys, depths, radii, conics, nth, _ = P.ProjectGaussians.apply(
                        sc.means, scales_e, 1, quats_n, v.viewmat[:3, :], v.projmat, v.fx, v.fy, v.cx, v.cy, H, W,
                        v.tile_bounds)
                    tail = P.ShadeTail.apply(4, viewdirs, sc.colors_all, depths, normals)
                out = fused_images(P, xys, depths, radii, conics, nth, opac, H, W, sc.feature, None, normals,
                                   tail=tail, packed=packed)
                g = torch.Generator(device="cpu").manual_seed(5 + k)
                torch.autograd.backward(list(out), [torch.randn(o.shape, generator=g).to(dev) for o in out])
            assert P.last_num_intersects() > 0
            if bucket is not None and k == VIEWS - 1:
                bucket.finish()
            per_view.append(calls[:])
            del calls[:]
        torch.cuda.synchronize()
    finally:
        for k in names:
            setattr(lib, k, real[k])
        P.clear_grad_sinks()
        P.clear_bin_cache()
        P._capacity_hint = prev_hint
        P.set_exact_forward(prev_exact)
        P.set_deterministic_backward(prev_det)
    if bucket is not None:
        grads = bucket.gathered()
        assert bool(torch.isfinite(grads).all()) and float(grads.abs().sum()) > 0
    return per_view


ROUTES = ("node-deferred", "node-immediate", "chain-deferred", "shim")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_entry_point_sequence_of_a_three_view_step(route):
    """One three-view step (N = 3000, 48 x 64, feature_dim 32; the second and third view bin speculatively) calls the
    same C entry points in the same order as the recorded ones, on
      node-deferred   ViewGeometry + rasterize_segments, GradBucket.enable_direct(ops, defer_sh=True), armed before
                      the last view;
      node-immediate  the same with enable_direct(ops): immediate sinks, `defer is None`;
      chain-deferred  ActivateGaussians -> ProjectGaussians -> ShadeTail -> rasterize_segments, deferred sinks;
      shim            pipeline.render_view(fused=False), no sinks."""
    assert _record_step(route) == EXPECTED_CALLS[route]


def _unit(rng, n):
    v = rng.standard_normal((n, 3)).astype(np.float32)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["ShadeTail", "SphericalHarmonics"])
@pytest.mark.parametrize("n", [70, 3000])
def test_deferred_sh_gradient_with_mixed_degrees_flushes_what_is_kept_first(n, op):
    """Three views of a step with degrees_to_use 4, 3, 3 (K = 25) into one sink with `defer`: the second view cannot
    join the first one's expansion (gg_sh_bwd_multi takes one degree), so it expands the first — one notification —
    and the step's last view expands views two and three — the second notification.  The buffer is bit-identical to
    the immediate sink's."""
    from gaussiangrasper_amd import ops as P
    dev = torch.device("cuda:0")
    k, degrees = 25, (4, 3, 3)
    rng = np.random.default_rng(n)
    t = lambda a: torch.from_numpy(a).to(dev)
    coeffs = (rng.standard_normal((n, k, 3)) * 0.6).astype(np.float32)
    depths, normals = rng.uniform(0.5, 9.0, n).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    dirs = [t(_unit(rng, n)) for _ in degrees]
    recs = [t(rng.standard_normal((n, 13)).astype(np.float32)) for _ in degrees]

    def run(deferred):
        sh = t(coeffs).requires_grad_(True)
        buf = torch.full((n, k, 3), 0.375, device=dev)
        fired, state = [], {"more": True}
        P.clear_grad_sinks()
        P.register_grad_sink(sh, buf, lambda p: fired.append(p), defer=(lambda: state["more"]) if deferred else None)
        try:
            for v, deg in enumerate(degrees):
                state["more"] = v < len(degrees) - 1
                if op == "ShadeTail":
                    P.ShadeTail.apply(deg, dirs[v], sh, t(depths), t(normals)).backward(recs[v][:, 6:])
                else:
                    P.SphericalHarmonics.apply(deg, dirs[v], sh).backward(recs[v][:, 6:9])
                if deferred:
                    assert len(fired) == (0, 1, 2)[v]
        finally:
            P.clear_grad_sinks()
        assert sh.grad is None and all(p is sh for p in fired)
        return buf.cpu().numpy(), len(fired)

    want, fired_immediate = run(False)
    got, fired_deferred = run(True)
    assert fired_immediate == 3 and fired_deferred == 2
    assert np.abs(want - 0.375).sum() > 0
    np.testing.assert_array_equal(got, want)
