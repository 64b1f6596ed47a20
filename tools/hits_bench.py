"""GPU time of one `ops.blend_hits` call (gg_blend_hits: record packing + the hit walk) at the lift_bench scene — 1 M
synthetic Gaussians (config 3), 1600x1200 — in its two builds: hit only (full=False: a pixel leaves at its hit) and
full (top_idx, top_vis, count: the walk goes to the forward's stop).  Next to them, on the same tile lists:

    blend_votes_one_label   `ops.blend_votes` with one label everywhere: the same walk with atomics
    render_depth_segments   the `ops.rasterize_segments` call of mesh.render_depth (rgb | z, 1): the route that
                            depth_mode="median" takes the depth away from

    python tools/hits_bench.py [--reps 10] [--points 1000000] [--height 1200] [--width 1600] [--out profiles/hits_bench.json]

Every figure is the median [min, max] of --reps device-event timings after 3 warm-up calls.  Projection and binning
are outside every timed window (the tile lists are cached on the projected tensors).  The entry has no in-library
profiling id, so the figures include the record-packing pass, as blend_votes' do.  Before anything is timed the two
builds' hit_idx are compared, and the hits with the forward's final_T (a pixel has a hit iff final_T <= t_hit)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiangrasper_amd import ops  # noqa: E402
from gaussiangrasper_amd.camera import ring_cameras  # noqa: E402
from gaussiangrasper_amd.scene import make_scene  # noqa: E402

WARMUP = 3
T_HIT = 0.5


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "hits_bench needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
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
        lab = torch.zeros(h, w, dtype=torch.uint8, device=dev)
        votes = torch.zeros(n, 1, dtype=torch.int64, device=dev)
        rgbs = torch.rand(n, 3, device=dev)
        zw = torch.stack([depths, torch.ones_like(depths)], dim=1).contiguous()
        segs = [(rgbs, torch.zeros(3, device=dev)), (zw, torch.zeros(2, device=dev))]

        def hit_only():
            return ops.blend_hits(*proj, h, w, T_HIT, full=False)

        def full():
            return ops.blend_hits(*proj, h, w, T_HIT, full=True)

        def vote():
            ops.blend_votes(*proj, h, w, lab, votes)

        def segments():
            return ops.rasterize_segments(xys, depths, radii, conics, nth, op, h, w, segs)

        # the same hits from both builds, and a hit exactly where the forward's final_T is <= t_hit
        hit, top, vis, cnt = full()
        assert torch.equal(hit_only()[0], hit), "the two builds disagree on hit_idx"
        bg = torch.zeros(1, device=dev)
        img = ops.NDRasterizeGaussians.apply(xys, depths, radii, conics, nth, torch.ones(n, 1, device=dev), op, h, w, bg)
        final_T = 1.0 - img[..., 0]          # to fp32 rounding: used away from the threshold only
        clear = (final_T - T_HIT).abs() > 1e-4
        assert torch.equal((hit >= 0)[clear], (final_T <= T_HIT)[clear]), "hits disagree with the forward's final_T"
        row = {"what": "ops.blend_hits (hit only / full) against ops.blend_votes with one label and against "
                       "render_depth's rasterize_segments call, same tile lists",
               "N": n, "height": h, "width": w, "t_hit": T_HIT, "num_intersects": int(bins.num_intersects),
               "pixels_with_hit": int((hit >= 0).sum()), "mean_blended_per_pixel": round(float(cnt.float().mean()), 2),
               "blend_hits_hit_only": timed(hit_only, a.reps), "blend_hits_full": timed(full, a.reps),
               "blend_votes_one_label": timed(vote, a.reps), "render_depth_segments": timed(segments, a.reps)}
        row["hit_only_over_votes"] = round(row["blend_hits_hit_only"]["ms_median"] /
                                           row["blend_votes_one_label"]["ms_median"], 3)
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARMUP, "rows": [row]}, f,
                      indent=1)


if __name__ == "__main__":
    main()
