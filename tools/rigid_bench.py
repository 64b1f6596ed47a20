"""GPU time of the rigid-move operator (gg_rigid_fwd + gg_rigid_bwd, csrc/rigid.hip) and of one evaluation of
pose.refine_object.

    python tools/rigid_bench.py [--reps 10] [--points 1000000] [--height 1200] [--width 1600] [--out profiles/rigid_bench.json]

rows[0..2]   N rows with 1 %, 10 % and 100 % of them selected (a seeded random mask).  A figure is a forward and a
             backward through autograd with dense random cotangents:
               kernels_full / kernels_pose_only      ops.RigidMove (means and quats requiring gradients / frozen);
               composite_full / composite_pose_only  ops.rigid_move_torch, the same formulas as torch operations;
               abi_full / abi_pose_only              the two C entries alone, no autograd around them.
rows[3]      one evaluation of refine_object's loss (rgb + depth, one view) on the plugin model at N Gaussians and
             height x width, the Gaussians inside a ball of radius 0.4 selected, split with device events recorded
             around the two gg_rigid_* calls: rigid_fwd | render_fwd (get_outputs + loss) | render_bwd | rigid_bwd; and
             the same split of one refine_camera evaluation on the same model (no rigid move: ViewGeometry's pose
             branch instead of its fallback, which a RigidMove output — no leaf with a sink — takes).

Every figure is the median [min, max] of --reps device-event timings after 3 warm-up calls.  There is no in-library
profiling id for these kernels: the figures are event timings around the calls."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiangrasper_amd import _lib, ops  # noqa: E402
from gaussiangrasper_amd.camera import ring_cameras  # noqa: E402
from gaussiangrasper_amd.pose import exp_map, homogeneous, object_transform  # noqa: E402
from gaussiangrasper_amd.scene import make_scene  # noqa: E402

WARMUP = 3


def stats(ts):
    return {"ms_median": round(float(np.median(ts)), 4), "ms_min": round(float(np.min(ts)), 4),
            "ms_max": round(float(np.max(ts)), 4)}


def timed(fn, reps):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return stats(ts)


def operator_rows(n, reps, dev):
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(5)
    means, quats = torch.randn(n, 3, generator=g).to(dev), torch.randn(n, 4, generator=g).to(dev)
    g_m, g_q = torch.randn(n, 3, generator=g).to(dev), torch.randn(n, 4, generator=g).to(dev)
    rt0, qt0 = object_transform(torch.tensor([0.02, -0.015, 0.01, 0.02, -0.05, 0.03]))
    rt0, qt0 = rt0.to(dev), qt0.to(dev)
    order = torch.randperm(n, generator=g)
    ws = torch.empty(max(lib.gg_rigid_bwd_workspace(n), 256), dtype=torch.uint8, device=dev)
    out_m, out_q, v_m, v_q = (torch.empty_like(t) for t in (means, quats, means, quats))
    v_pose = torch.empty(16, device=dev)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rows = []
    for frac in (0.01, 0.1, 1.0):
        mask = torch.zeros(n, dtype=torch.uint8)
        mask[order[:int(round(frac * n))]] = 1
        mask = mask.to(dev)

        def through(move, full):
            def run():
                m = means.detach().requires_grad_(full)
                q = quats.detach().requires_grad_(full)
                rt, qt = rt0.detach().requires_grad_(True), qt0.detach().requires_grad_(True)
                a, b = move(m, q, mask, rt, qt)
                torch.autograd.backward([a, b], [g_m, g_q])
                return rt.grad, qt.grad
            return run

        def abi(full):
            def run():
                _lib.check(lib.gg_rigid_fwd(n, p(means), p(quats), p(mask), p(rt0), p(qt0), p(out_m), p(out_q), stream()),
                           "gg_rigid_fwd")
                _lib.check(lib.gg_rigid_bwd(n, p(means), p(quats), p(mask), p(rt0), p(qt0), p(g_m), p(g_q),
                                            p(v_m if full else None), p(v_q if full else None), p(v_pose),
                                            C.c_void_p(v_pose.data_ptr() + 48), p(ws), ws.numel(), stream()),
                           "gg_rigid_bwd")
            return run
        # the two routes compute the same pose gradient (the composite's sums are unordered fp32)
        k_rt, k_qt = through(ops.RigidMove, False)()
        c_rt, c_qt = through(ops.rigid_move_torch, False)()
        scale = float(k_rt.abs().max())
        assert float((k_rt - c_rt).abs().max()) <= 1e-3 * scale and float((k_qt - c_qt).abs().max()) <= 1e-3 * scale
        row = {"what": "ops.RigidMove forward + backward against the torch composite, same GPU", "N": n,
               "selected": int(mask.sum()), "fraction": frac}
        for name, fn in (("kernels_full", through(ops.RigidMove, True)),
                         ("kernels_pose_only", through(ops.RigidMove, False)),
                         ("composite_full", through(ops.rigid_move_torch, True)),
                         ("composite_pose_only", through(ops.rigid_move_torch, False)),
                         ("abi_full", abi(True)), ("abi_pose_only", abi(False))):
            row[name] = timed(fn, reps)
        row["composite_over_kernels_full"] = round(row["composite_full"]["ms_median"] / row["kernels_full"]["ms_median"], 2)
        row["composite_over_kernels_pose_only"] = round(row["composite_pose_only"]["ms_median"] /
                                                        row["kernels_pose_only"]["ms_median"], 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def evaluation_row(n, h, w, reps, dev):
    from gaussiangrasper_amd.plugin import make_fused_model_class
    from gaussiangrasper_amd.stub import StubCameras, StubGaussianSplattingModel
    lib = _lib.load()
    sc = make_scene(n, feature_dim=32, config_index=3)
    model = make_fused_model_class(StubGaussianSplattingModel)(sc).to(dev).eval()
    for prm in model.parameters():
        prm.requires_grad_(False)
    cam = StubCameras.from_view(ring_cameras(8, h, w)[0], device=dev)
    base_c2w = cam.camera_to_worlds.detach().clone()
    mask = (model.means.detach().norm(dim=1) < 0.4).to(torch.uint8)
    centre = model.means.detach()[mask.bool()].mean(dim=0)
    with torch.no_grad():
        rt, qt = object_transform(torch.tensor([0.02, -0.015, 0.01, 0.02, -0.05, 0.03], device=dev), None, centre)
        model.object_pose = (mask, rt, qt)
        ops.clear_bin_cache()
        out = model.get_outputs(cam)
        rgb, depth = out["rgb"].clone(), out["depth"].clone()
        model.object_pose = None
    marks = {}
    real = {k: getattr(lib, k) for k in ("gg_rigid_fwd", "gg_rigid_bwd")}

    def bracket(name):
        def call(*args):
            marks[name + "0"].record()
            st = real[name](*args)
            marks[name + "1"].record()
            return st
        return call

    def loss_of(out):
        return ((out["rgb"] - rgb) ** 2).sum(-1).mean() + ((out["depth"] - depth) ** 2).mean()

    def one(kind):
        for k in ("start", "fwd_done", "end", "gg_rigid_fwd0", "gg_rigid_fwd1", "gg_rigid_bwd0", "gg_rigid_bwd1"):
            marks[k] = torch.cuda.Event(enable_timing=True)
        delta = torch.zeros(6, device=dev, requires_grad=True)
        ops.clear_bin_cache()
        marks["start"].record()
        if kind == "object":
            model.object_pose = (mask, *object_transform(delta, None, centre))
        else:
            cam.camera_to_worlds = torch.bmm(base_c2w, homogeneous(exp_map(delta[None])))
        loss = loss_of(model.get_outputs(cam))
        marks["fwd_done"].record()
        loss.backward()
        marks["end"].record()
        marks["end"].synchronize()
        model.object_pose = None
        cam.camera_to_worlds = base_c2w
        assert delta.grad is not None and bool(torch.isfinite(delta.grad).all())
        el = lambda a, b: marks[a].elapsed_time(marks[b])
        if kind == "object":
            return {"rigid_fwd": el("gg_rigid_fwd0", "gg_rigid_fwd1"), "render_fwd": el("gg_rigid_fwd1", "fwd_done"),
                    "render_bwd": el("fwd_done", "gg_rigid_bwd0"), "rigid_bwd": el("gg_rigid_bwd0", "gg_rigid_bwd1"),
                    "total": el("start", "end")}
        return {"render_fwd": el("start", "fwd_done"), "render_bwd": el("fwd_done", "end"), "total": el("start", "end")}

    try:
        for k in real:
            setattr(lib, k, bracket(k))
        row = {"what": "one evaluation of pose.refine_object's loss (one view, rgb + depth) on the plugin "
                       "model, and one of pose.refine_camera's on the same model",
               "N": n, "height": h, "width": w, "selected": int(mask.sum())}
        for kind in ("object", "camera"):
            for _ in range(WARMUP):
                one(kind)
            runs = [one(kind) for _ in range(reps)]
            row["refine_" + kind + "_evaluation"] = {k: stats([r[k] for r in runs]) for k in runs[0]}
    finally:
        for k, f in real.items():
            setattr(lib, k, f)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rigid_bench needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = operator_rows(a.points, a.reps, dev)
    rows.append(evaluation_row(a.points, a.height, a.width, a.reps, dev))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARMUP, "rows": rows}, f,
                      indent=1)


if __name__ == "__main__":
    main()
