#!/usr/bin/env python3
"""Cost of the camera-pose gradient (a measurement tool, not part of the product).

  kernels   at the bench scene (1 M Gaussians, 1600 x 1200): gg_view_bwd (view_bwd_kernel) against gg_view_bwd_pose
            (view_bwd_pose_kernel + pose_finish_kernel) and the pose-only pass gg_project_pose_bwd, on the same
            per-Gaussian records; the library's event brackets give the per-launch means (run it under
            `rocprofv3 --kernel-trace --stats` for the profiler's view of the same launches)
  iteration one training view through the plugin class (stub model, gradient sinks on the Gaussian parameters so the
            backward is the one-kernel branch): forward, an L1 rgb + depth loss, backward — with the camera
            optimizer off and in SO3xR3 mode

Prints one JSON object.  Usage: python tools/pose_grad_bench.py [--points 1000000] [--reps 50]"""
import argparse
import ctypes as C
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "shim")]
import torch  # noqa: E402

from gaussiangrasper_amd import _lib, ops as P  # noqa: E402
from gaussiangrasper_amd.camera import ring_cameras  # noqa: E402
from gaussiangrasper_amd.scene import make_scene  # noqa: E402

DEV = "cuda:0"
K_VIEW_BWD, K_VIEW_BWD_POSE, K_POSE_BWD, K_POSE_FINISH = 29, 40, 41, 42


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def kernels(lib, n, h, w, reps):
    sc = make_scene(n, feature_dim=4, config_index=0)
    v = ring_cameras(8, h, w, device=DEV)[0]
    means, scales = sc.means.to(DEV), sc.scales.exp().to(DEV)
    quats = sc.quats.to(DEV).contiguous()
    vm, pm = v.viewmat[:3].contiguous(), v.projmat.contiguous()
    with torch.no_grad():
        _, _, radii, conics, _, _ = P.ProjectGaussians.apply(means, scales, 1, quats, vm, pm, v.fx, v.fy, v.cx, v.cy, h,
                                                             w, v.tile_bounds)
    rec = torch.randn(n, 16, device=DEV) * 1e-3
    v_depth = rec[:, 9].contiguous()
    mask = torch.randint(0, 8, (n,), dtype=torch.uint8, device=DEV)
    axis = torch.argmin(scales, 1).to(torch.int32)
    opac = torch.rand(n, device=DEV)
    sinks = [torch.zeros(n, k, device=DEV) for k in (3, 3, 4, 1)]
    v_rgb = torch.empty(n, 3, device=DEV)
    out_v, out_p = torch.empty(12, device=DEV), torch.empty(16, device=DEV)
    ws = torch.empty(lib.gg_pose_grad_workspace(n), dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    args = [n, ptr(rec), 16, ptr(mask), ptr(means), ptr(scales), 1.0, ptr(quats), ptr(quats), ptr(opac), ptr(axis),
            ptr(vm), ptr(pm), v.fx, v.fy, h, w, ptr(radii), ptr(conics), ptr(v_rgb)] + [ptr(s) for s in sinks]
    calls = {
        "view_bwd": lambda: lib.gg_view_bwd(*args, st),
        "view_bwd_pose": lambda: lib.gg_view_bwd_pose(*args, ptr(out_v), ptr(out_p), ptr(ws), ws.numel(), st),
        "project_pose_bwd": lambda: lib.gg_project_pose_bwd(
            n, ptr(means), ptr(scales), 1.0, ptr(quats), ptr(vm), ptr(pm), v.fx, v.fy, h, w, ptr(radii), ptr(conics),
            ptr(rec), 16, ptr(v_depth), ptr(rec, 2), 16, ptr(out_v), ptr(out_p), ptr(ws), ws.numel(), st),
    }
    for f in calls.values():            # warm-up
        assert f() == 0, lib.gg_last_error()
    torch.cuda.synchronize()
    lib.gg_prof_reset()
    lib.gg_prof_enable(1)
    for _ in range(reps):               # interleaved: the same clocks and caches for all three
        for f in calls.values():
            assert f() == 0
    torch.cuda.synchronize()
    lib.gg_prof_enable(0)
    res = {}
    for kid, name in ((K_VIEW_BWD, "view_bwd_kernel"), (K_VIEW_BWD_POSE, "view_bwd_pose_kernel"),
                      (K_POSE_BWD, "project_pose_bwd_kernel"), (K_POSE_FINISH, "pose_finish_kernel")):
        cnt, ms = C.c_int(0), C.c_double(0.0)
        lib.gg_prof_get(kid, C.byref(cnt), C.byref(ms))
        res[name + "_us"] = round(1e3 * ms.value / max(cnt.value, 1), 2)
    lib.gg_prof_reset()
    res["visible"] = int((radii > 0).sum())
    res["slab_rows"] = (n + 255) // 256
    return res


def iteration(n, h, w, reps):
    from gaussiangrasper_amd.plugin import make_fused_model_class
    from gaussiangrasper_amd.stub import (StubCameras, StubGaussianSplattingModel, StubPoseCameraOptimizer,
                                          default_config)
    out = {}
    views = ring_cameras(8, h, w)
    for mode in ("off", "SO3xR3"):
        cfg = default_config(camera_optimizer=types.SimpleNamespace(mode=mode))
        m = make_fused_model_class(StubGaussianSplattingModel)(make_scene(n, feature_dim=32, config_index=0),
                                                                config=cfg).to(DEV)
        if mode != "off":
            m.camera_optimizer = StubPoseCameraOptimizer(len(views), mode, device=DEV)
        m.train()
        params = [m.means, m.scales, m.quats, m.opacities, m.colors_all]
        for p_ in params:
            P.register_grad_sink(p_, torch.zeros_like(p_))
        cams = [StubCameras.from_view(v, device=DEV, cam_idx=i) for i, v in enumerate(views)]
        rgb_t = torch.rand(h, w, 3, device=DEV)
        times = []
        for k in range(reps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            cam = cams[k % len(cams)]
            cam.camera_to_worlds = cam.camera_to_worlds.detach()
            a.record()
            o = m(cam)
            loss = (o["rgb"] - rgb_t).abs().mean() + o["depth"].mean() * 1e-3
            loss.backward()
            b.record()
            torch.cuda.synchronize()
            if k >= 3:
                times.append(a.elapsed_time(b))
        P.clear_grad_sinks()
        times.sort()
        out[f"view_ms_camopt_{mode}"] = round(times[len(times) // 2], 3)
        if mode != "off":
            g = m.camera_optimizer.pose_adjustment.grad
            out["pose_grad_rows_nonzero"] = int((g != 0).any(1).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-iteration", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    res = {"points": a.points, "image": [a.height, a.width]}
    res.update(kernels(lib, a.points, a.height, a.width, a.reps))
    if not a.skip_iteration:
        res.update(iteration(a.points, a.height, a.width, max(a.reps // 5, 5)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
