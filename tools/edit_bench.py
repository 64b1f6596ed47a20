"""GPU time of one scene-update launch (gaussiangrasper_amd.edit.select_and_move -> gg_hull_edit) at 1 M and 5 M
Gaussians with hulls of ~100 and ~1000 facets, and — where scipy is present — the host route the reference takes
(scipy Delaunay of the object points, then find_simplex over every mean) for comparison.

    python tools/edit_bench.py [--reps 50] [--out profiles/edit_bench.json]

Scene: make_scene-style means in [-1, 1]^2 x [-0.5, 0.5]; object: points on a sphere of radius 0.12 at the origin
(~0.1 % of the Gaussians inside, as for a grasped object).  The timed call moves the selection by the identity, so
every repetition selects the same rows and does the full work (select + move).  Median of --reps CUDA-event timings
after 5 warm-up launches."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiangrasper_amd.edit import select_and_move  # noqa: E402


def sphere_points(m, radius, seed):
    p = np.random.default_rng(seed).normal(size=(m, 3))
    return radius * p / np.linalg.norm(p, axis=1, keepdims=True)


def planes_for(obj):
    """Qhull half-spaces where scipy is present (a points-on-sphere hull has 2m - 4 facets), else the m tangent planes
    at the points"""
    try:
        from gaussiangrasper_amd.edit import hull_planes
        return hull_planes(obj), "qhull"
    except ImportError:
        r = np.linalg.norm(obj, axis=1, keepdims=True)
        return np.concatenate([obj / r, -r], axis=1), "tangent"


def time_gpu(means, quats, planes, reps):
    eye = np.eye(3, 4, dtype=np.float32)
    pl = torch.from_numpy(planes).cuda()
    for _ in range(5):
        select_and_move(means, quats, pl, eye)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _, count = select_and_move(means, quats, pl, eye)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), int(count.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the scipy find_simplex comparison")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "edit_bench needs the GPU"
    rows = []
    for n in (1_000_000, 5_000_000):
        g = torch.Generator().manual_seed(n)
        means = ((torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 1.0, 0.5])).cuda()
        quats = torch.randn(n, 4, generator=g).cuda()
        for m in (52, 502):
            obj = sphere_points(m, 0.12, m)
            planes, kind = planes_for(obj)
            med, best, count = time_gpu(means, quats, planes, a.reps)
            row = {"what": "gg_hull_edit select+move", "N": n, "F": int(planes.shape[0]), "hull": kind,
                   "selected": count, "gpu_ms_median": round(med, 4), "gpu_ms_min": round(best, 4),
                   "gb_per_s_min_traffic": round(n * 13 / (med * 1e-3) / 1e9, 1)}
            if not a.no_host and n == 1_000_000:
                try:
                    from scipy.spatial import Delaunay
                    x = means.cpu().numpy()
                    t0 = time.perf_counter()
                    tri = Delaunay(obj)
                    t1 = time.perf_counter()
                    host = tri.find_simplex(x) >= 0
                    t2 = time.perf_counter()
                    row.update(host_delaunay_s=round(t1 - t0, 4), host_find_simplex_s=round(t2 - t1, 4),
                               host_selected=int(host.sum()))
                except ImportError:
                    pass
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
