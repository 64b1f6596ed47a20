"""GPU time of one `ops.blend_votes` call (gg_blend_votes: record packing + the vote walk) at the headline scene —
1 M synthetic Gaussians (config 3), 1600x1200 — with L = 2 and L = 8 labels, next to the only route to the same sums
before the entry existed: `ops.NDRasterizeGaussians` forward plus backward over L channels with a one-hot cotangent,
reading `v_colors` (float atomics, geometry gradients paid for as well).

    python tools/lift_bench.py [--reps 10] [--points 1000000] [--height 1200] [--width 1600] [--out profiles/lift_bench.json]

Every figure is the median [min, max] of --reps device-event timings after 3 warm-up calls.  Projection and binning
are outside both timed windows (both routes share them: the tile lists are cached on the projected tensors).  Labels:
a seeded image of 48x48-pixel blocks (a segmenter's masks are piecewise constant: most 8x8 quadrants see one label,
the blocks' borders two to four) and, as the worst case for the per-label wave reductions, a per-pixel random image.
`walk_ms` is the in-library bracket of the vote kernel alone (GG_K_BLEND_VOTES), from a separate pass with the
hipEvent hooks on.  The votes of the timed call are compared with the backward's v_colors before anything is timed."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiangrasper_amd import _lib, lift, ops  # noqa: E402
from gaussiangrasper_amd.camera import ring_cameras  # noqa: E402
from gaussiangrasper_amd.scene import make_scene  # noqa: E402

WARMUP = 3
GG_K_BLEND_VOTES = 14


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
    return {"ms_median": round(float(np.median(ts)), 4), "ms_min": round(float(np.min(ts)), 4),
            "ms_max": round(float(np.max(ts)), 4)}


def walk_ms(lib, fn, reps):
    """median of the in-library bracket of the vote walk alone"""
    lib.gg_prof_enable(1)
    ts = []
    for _ in range(reps):
        lib.gg_prof_reset()
        fn()
        torch.cuda.synchronize()
        n, ms = ctypes.c_int(0), ctypes.c_double(0.0)
        lib.gg_prof_get(GG_K_BLEND_VOTES, ctypes.byref(n), ctypes.byref(ms))
        ts.append(ms.value / max(n.value, 1))
    lib.gg_prof_enable(0)
    lib.gg_prof_reset()
    return round(float(np.median(ts)), 4)


def label_image(kind, h, w, L, seed):
    rng = np.random.default_rng(seed)
    if kind == "blocks":
        small = rng.integers(0, L, ((h + 47) // 48, (w + 47) // 48))
        return np.kron(small, np.ones((48, 48), np.int64))[:h, :w].astype(np.uint8)
    return rng.integers(0, L, (h, w)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lift_bench needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    n, h, w = a.points, a.height, a.width
    sc = make_scene(n, feature_dim=1, config_index=3).to(dev)
    v = ring_cameras(8, h, w, device=dev)[0]
    with torch.no_grad():      # the projection as lift.project_view runs it
        geo = ops.ProjectGaussians.apply(sc.means.contiguous(), torch.exp(sc.scales), 1,
                                         sc.quats / sc.quats.norm(dim=-1, keepdim=True), v.viewmat[:3, :], v.projmat,
                                         v.fx, v.fy, v.cx, v.cy, h, w, v.tile_bounds)
    proj = (*geo[:5], torch.sigmoid(sc.opacities).reshape(-1, 1).contiguous())
    xys, depths, radii, conics, nth, op = proj
    bins = ops.bin_and_sort_gaussians(xys, depths, radii, nth, h, w)
    rows = []
    for L in (2, 8):
        for kind in ("blocks", "random"):
            lab_np = label_image(kind, h, w, L, 100 + L)
            lab = torch.from_numpy(lab_np).to(dev)
            votes = torch.zeros(n, L, dtype=torch.int64, device=dev)
            colors = torch.rand(n, L, device=dev, requires_grad=True)
            bg = torch.zeros(L, device=dev)
            onehot = torch.nn.functional.one_hot(lab.long(), L).float().contiguous()

            def vote():
                ops.blend_votes(*proj, h, w, lab, votes)

            def route():
                colors.grad = None
                img = ops.NDRasterizeGaussians.apply(xys, depths, radii, conics, nth, colors, op, h, w, bg)
                img.backward(onehot)
                return colors.grad

            # same sums first: the backward's bar against the oracle plus the truncation over the tile box
            vote()
            got = lift.weights(votes).cpu().numpy()
            ref = route().double().cpu().numpy()
            tol = 5e-5 * np.abs(ref) + 1e-6 * np.abs(ref).max() + nth.cpu().numpy()[:, None] * 256 * 2.0 ** -24
            assert (np.abs(got - ref) <= tol).all(), "votes and the backward's v_colors disagree"
            row = {"what": "ops.blend_votes against NDRasterizeGaussians forward + backward (one-hot cotangent)",
                   "N": n, "height": h, "width": w, "L": L, "labels": kind, "num_intersects": int(bins.num_intersects),
                   "blend_votes": timed(vote, a.reps), "walk_ms": walk_ms(lib, vote, a.reps),
                   "forward_backward": timed(route, a.reps)}
            row["speedup"] = round(row["forward_backward"]["ms_median"] / row["blend_votes"]["ms_median"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARMUP, "rows": rows}, f,
                      indent=1)


if __name__ == "__main__":
    main()
