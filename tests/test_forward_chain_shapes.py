"""The SH forward beside a blend kernel (ops.ShadeTail's `one_wave`; profiles/forward_chain_overlap.txt): the build with
one-wave workgroups against the 256-thread build, one plugin-route view through the opted-in path against the default
one, and which of the two the plugin's model class launches.  Everything a forward kernel writes is compared bit for
bit: the shape changes which workgroup computes a Gaussian, never an operation or a summation order."""
import numpy as np
import pytest
import torch

from gaussiangrasper_amd import _lib, ops as P
from gaussiangrasper_amd._call import ptr as _ptr, stream as _stream, workspace as _workspace
from gaussiangrasper_amd.camera import ring_cameras
from gaussiangrasper_amd.constants import CLIP_THRESH_DEFAULT, num_sh_bases
from gaussiangrasper_amd.scene import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.numpy().view(np.uint8 if t.dtype == torch.uint8 else np.uint32 if t.element_size() == 4 else np.uint64)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: not bit-equal"


def _scene(n, h, w, case="plain", sh_degree=4, seed_cfg=1):
    sc = make_scene(n, feature_dim=32, sh_degree=sh_degree, config_index=seed_cfg).to(DEV)
    sc.scales.data.add_(1.2)                     # bigger splats at these tiny resolutions
    view = ring_cameras(3, h, w, device=DEV)[1]
    if case != "plain":
        # behind the camera: every Gaussian is culled by the near plane
        back = view.cam_pos.reshape(-1)[:3] * 3.0
        keep = sc.means.data[-1].clone()
        sc.means.data[:] = back + 0.01 * sc.means.data
        if case == "last_visible":               # ... but the last one, alone in the last workgroup
            sc.means.data[-1] = 0.1 * keep
    return sc, view


def _view_fwd(sc, view, h, w):
    """gg_view_fwd on fresh, poisoned outputs"""
    lib = _lib.load()
    n = sc.means.shape[0]
    f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    o = {"scales": f(n, 3), "quats_n": f(n, 4), "opac": f(n, 1), "viewdirs": f(n, 3), "normals": f(n, 3), "axis": i32(n),
         "xys": f(n, 2), "depths": f(n), "radii": i32(n), "conics": f(n, 3), "num_tiles_hit": i32(n),
         "total": torch.full((1,), -1, dtype=torch.int64, device=DEV)}
    blocks = max((n + 255) // 256, 1)
    assert lib.gg_view_fwd_workspace(n) == 12 * blocks
    o["parts"] = i32(3 * blocks)
    o["records"] = _workspace(lib.gg_blend_workspace(n), DEV)
    o["records"].zero_()
    tb = view.tile_bounds
    cam = view.cam_pos.to(DEV).reshape(-1)[:3].contiguous()
    vm, pm = view.viewmat[:3, :].contiguous(), view.projmat.contiguous()
    args = (n, _ptr(sc.means), _ptr(sc.scales), _ptr(sc.quats), _ptr(sc.opacities), _ptr(cam), _ptr(vm), _ptr(pm),
            view.fx, view.fy, view.cx, view.cy, h, w, int(tb[0]), int(tb[1]), CLIP_THRESH_DEFAULT,
            _ptr(o["scales"]), _ptr(o["quats_n"]), _ptr(o["opac"]), _ptr(o["viewdirs"]), _ptr(o["normals"]),
            _ptr(o["axis"]), _ptr(o["xys"]), _ptr(o["depths"]), _ptr(o["radii"]), _ptr(o["conics"]),
            _ptr(o["num_tiles_hit"]), _ptr(o["total"]), _ptr(o["parts"]), o["parts"].numel() * 4, _ptr(o["records"]),
            o["records"].numel())
    _lib.check(lib.gg_view_fwd(*args, _stream(DEV)), "gg_view_fwd")
    torch.cuda.synchronize()
    return o


CASES = [(n, "plain") for n in (1, 63, 64, 65, 255, 257, 1000)] + [(1000, "all_culled"), (1000, "last_visible")]


@pytest.mark.parametrize("h,w", [(48, 64), (17, 33)])
@pytest.mark.parametrize("deg", [0, 4])
@pytest.mark.parametrize("n,case", CASES)
def test_one_wave_sh_forward_matches_the_256_thread_build(n, case, deg, h, w):
    """gg_shade_tail_fwd_ex(one_wave=1) against gg_shade_tail_fwd: the (N, 7) colour | depth | normal array and the clamp
    mask, bit for bit; K = 1 (64 rows per wave) and K = 25 (32 rows per wave)."""
    lib = _lib.load()
    sc, view = _scene(n, h, w, case, sh_degree=deg)
    geo = _view_fwd(sc, view, h, w)
    k = num_sh_bases(deg)
    assert sc.colors_all.shape[1] == k
    outs = []
    for one_wave in (None, 0, 1):
        tail = torch.full((n, 7), float("nan"), dtype=torch.float32, device=DEV)
        mask = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
        args = (n, k, deg, _ptr(geo["viewdirs"]), _ptr(sc.colors_all), _ptr(geo["depths"]), _ptr(geo["normals"]),
                _ptr(tail), _ptr(mask))
        if one_wave is None:
            _lib.check(lib.gg_shade_tail_fwd(*args, _stream(DEV)), "gg_shade_tail_fwd")
        else:
            _lib.check(lib.gg_shade_tail_fwd_ex(*args, one_wave, _stream(DEV)), "gg_shade_tail_fwd_ex")
        torch.cuda.synchronize()
        outs.append((tail, mask))
    assert not bool(torch.isnan(outs[0][0][:, :3]).any()) and int(outs[0][1].max()) <= 7
    for (tail, mask), tag in zip(outs[1:], ("four waves", "one wave")):
        _same_bits(tail, outs[0][0], f"{tag}: tail")
        _same_bits(mask, outs[0][1], f"{tag}: clamp mask")


def _render(sc, view, h, w, beside, seed=3):
    """one plugin-route view forward and backward (ViewGeometry + rasterize_segments through pipeline.fused_images)"""
    from gaussiangrasper_amd.pipeline import fused_images
    leaves = [p.detach().clone().requires_grad_(True) for p in sc.params()]
    means, scales, quats, opacities, colors_all, feature = leaves
    cam = view.cam_pos.to(DEV).reshape(-1)[:3]
    xys, depths, radii, conics, nth, opac, tail, normals, packed = P.ViewGeometry.apply(
        means, scales, quats, opacities, colors_all, cam, view.viewmat[:3, :], view.projmat, view.fx, view.fy,
        view.cx, view.cy, h, w, view.tile_bounds, 4, beside)
    out = fused_images(P, xys, depths, radii, conics, nth, opac, h, w, feature, None, normals, tail=tail, packed=packed)
    saved = out[0].grad_fn.saved_tensors
    final_T, final_idx = saved[5], saved[6]
    assert final_T.shape == (h, w) and final_idx.dtype == torch.int32
    g = torch.Generator(device="cpu").manual_seed(seed)
    torch.autograd.backward(list(out), [torch.randn(o.shape, generator=g).to(DEV) for o in out])
    torch.cuda.synchronize()
    return [o.detach() for o in out], final_T, final_idx, [p.grad for p in leaves]


@pytest.mark.parametrize("capacity", ["hinted", "too small"])
def test_plugin_route_view_through_the_new_path(capacity):
    """2 000 Gaussians, 160 x 96, forward and backward: images, final_T and final_idx of the opted-in path bit-equal to
    the default path's; parameter gradients within the pair-backward tests' tolerance (tests/test_gpu_parity.py:
    rtol 5e-5 + 1e-6 max|g| — what two runs of the float atomics differ by is far inside it).  `too small`: the
    capacity hint is forced below the count, so the speculative lists are truncated and Binning.resolve bins again with
    the exact size (the re-bin behind the one-wave SH forward)."""
    from test_gpu_parity import assert_close
    h, w, n = 96, 160, 2000
    sc, view = _scene(n, h, w)
    prev_hint = dict(P._capacity_hint)
    stats0 = dict(P.bin_cache_stats)
    try:
        P.clear_bin_cache()
        P._capacity_hint.clear()
        ref = _render(sc, view, h, w, False)          # (also leaves a capacity hint: the next view bins speculatively)
        count = P.last_num_intersects()
        assert count > 0 and P._capacity_hint[torch.device(DEV).index] >= count
        if capacity == "too small":
            P._capacity_hint[torch.device(DEV).index] = max(count // 2, 1)
        P.clear_bin_cache()
        lib, calls = _lib.load(), []
        real = lib.gg_shade_tail_fwd_ex
        lib.gg_shade_tail_fwd_ex = lambda *a: calls.append(a[-2]) or real(*a)
        try:
            got = _render(sc, view, h, w, True)
        finally:
            lib.gg_shade_tail_fwd_ex = real
        assert calls == [1], "the opted-in view launches the one-wave SH forward, once"
        assert P.last_num_intersects() == count
        rebinned = P.bin_cache_stats["rebinned"] - stats0["rebinned"]
        assert rebinned == (1 if capacity == "too small" else 0)
    finally:
        P._capacity_hint.clear()
        P._capacity_hint.update(prev_hint)
        P.clear_bin_cache()
    for a, b, name in zip(got[0], ref[0], ("feature", "rgb", "depth", "normal")):
        _same_bits(a, b, f"image {name}")
    _same_bits(got[1], ref[1], "final_T")
    _same_bits(got[2], ref[2], "final_idx")
    for a, b, name in zip(got[3], ref[3], ("means", "scales", "quats", "opacities", "colors_all", "feature")):
        assert a is not None and b is not None, name
        assert_close(a.cpu().numpy(), b.cpu().numpy(), f"forward chain grad.{name}", rtol=5e-5, atol_frac=1e-6)


def test_plugin_model_launches_one_wave_sh_forward_in_training_mode_only():
    """plugin.fused_view through the model class: a training view calls gg_shade_tail_fwd_ex(one_wave=1), a render-only
    (eval) view gg_shade_tail_fwd, and both give the same images bit for bit."""
    from gaussiangrasper_amd.plugin import make_fused_model_class
    from gaussiangrasper_amd.stub import StubCameras, StubGaussianSplattingModel
    h, w = 96, 160
    sc, view = _scene(2000, h, w)
    model = make_fused_model_class(StubGaussianSplattingModel)(sc)
    cam = StubCameras.from_view(view, device=DEV)
    lib, calls = _lib.load(), []
    real = {k: getattr(lib, k) for k in ("gg_shade_tail_fwd", "gg_shade_tail_fwd_ex")}
    lib.gg_shade_tail_fwd = lambda *a: calls.append("plain") or real["gg_shade_tail_fwd"](*a)
    lib.gg_shade_tail_fwd_ex = lambda *a: calls.append(("ex", a[-2])) or real["gg_shade_tail_fwd_ex"](*a)
    outs = {}
    try:
        for mode in ("train", "eval"):
            getattr(model, mode)()
            P.clear_bin_cache()
            out = model(cam)
            torch.cuda.synchronize()
            outs[mode] = {k: out[k].detach().clone() for k in ("rgb", "feature", "depth", "normal")}
    finally:
        for k, fn in real.items():
            setattr(lib, k, fn)
        P.clear_bin_cache()
    assert calls == [("ex", 1), "plain"]
    for k in outs["train"]:
        _same_bits(outs["train"][k], outs["eval"][k], f"image {k}")
