"""GPU time of the scene-update masks (gaussiangrasper_amd.edit_masks.object_masks -> gg_object_masks): 200 views of
640 x 480, M = 20 000 and 200 000 object points, dilation k = 0 and 5, against the numpy restatement of
tests/objmask_ref.py on one host core (timed on a few views and scaled to 200: it costs the same per view).

    python tools/objmask_bench.py [--reps 50] [--host-views 4] [--out profiles/objmask_bench.json]

Object: an anisotropic Gaussian blob (sigma 0.02 m x 0.6 / 1.4 per axis) at the origin; cameras: a jittered ring at
0.6 m looking at it (fx = 576 px), so the object's hull covers a few hundred pixels across in every view (the row
`union_pixels_per_view` says how many).  Each timed call is the whole call as a user
makes it: six launches, one status read-back, one stream synchronisation.  Median of --reps CUDA-event timings
after 5 warm-up calls; every result is checked once against the restatement on the host-timed views."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import objmask_ref as R  # noqa: E402
from gaussiangrasper_amd.edit_masks import motion, object_masks  # noqa: E402

H, W, V = 480, 640, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-views", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "objmask_bench needs the GPU"
    c2w = R.ring(V, seed=1)
    intr = np.array([[0.9 * W, 0.9 * W, W / 2, H / 2]] * V)
    w2c = np.array([np.linalg.inv(T)[:3] for T in c2w])
    T = motion([0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.08, -0.03, 0.02, 0.0, 0.0, 0.4])
    K, E = torch.as_tensor(intr).cuda(), torch.as_tensor(w2c).cuda()
    rows = []
    for m in (20_000, 200_000):
        pts = np.random.default_rng(m).normal(scale=0.02, size=(m, 3)) * np.array([1.0, 0.6, 1.4])
        P = torch.as_tensor(pts).cuda()
        for k in (0, 5):
            for _ in range(5):
                out = object_masks(P, T, K, E, H, W, dilate=k)
            torch.cuda.synchronize()
            ts, walls = [], []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                out = object_masks(P, T, K, E, H, W, dilate=k)
                e1.record()
                e1.synchronize()
                walls.append(time.perf_counter() - t0)
                ts.append(e0.elapsed_time(e1))
            hv = a.host_views
            t0 = time.perf_counter()
            ref = R.object_masks(pts, T, intr[:hv], w2c[:hv], H, W, k)
            host_s = (time.perf_counter() - t0) * V / hv
            same = all(np.array_equal(getattr(out, n)[:hv].cpu().numpy(), ref[n]) for n in ("before", "after", "union"))
            same = same and np.array_equal(out.boxes[:hv].cpu().numpy(), ref["boxes"])
            med = float(np.median(ts))
            row = {"what": "gg_object_masks", "views": V, "height": H, "width": W, "M": m, "dilate": k,
                   "gpu_ms_median": round(med, 4), "gpu_ms_min": round(float(np.min(ts)), 4),
                   "wall_ms_median": round(1e3 * float(np.median(walls)), 4),
                   "views_per_s": round(V / (med * 1e-3), 1),
                   "mask_bytes_written": 3 * V * H * W,
                   "mask_gb_per_s": round(3 * V * H * W / (med * 1e-3) / 1e9, 1),
                   "union_pixels_per_view": round(float(out.union.sum().item()) / V, 1),
                   "host_numpy_1core_s_200_views": round(host_s, 3), "host_views_timed": hv,
                   "speedup_vs_host": round(host_s / (med * 1e-3), 1), "bit_equal_on_host_views": bool(same)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
