"""GPU time of the three distance-field calls (gaussiangrasper_amd.field on gg_field_splat, gg_field_distance and
gg_field_paths) at sizes a planner would use:

    splat     1 M synthetic Gaussians into 256^3 cells of 1 cm (log-normal scales around 6 mm, 0.2 % of them 4-12 cm)
    distance  the transform at 128^3 and 256^3 of that scene, next to scipy.ndimage.distance_transform_edt on the host
              (one host run each; the results are compared first)
    paths     4096 paths x 64 waypoints x 32 spheres, next to a torch restatement (fp64 centres, cell rule, gather, min)
              on the same GPU (the results are compared first)

    python tools/field_bench.py [--reps 10] [--rows 1000000] [--out profiles/field_bench.json]

Every GPU figure is the median [min, max] of --reps device-event timings after 3 warm-up calls."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiangrasper_amd import field  # noqa: E402

WARMUP = 3


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


def synthetic_rows(n, side, dev, seed=0):
    """means on noisy sheets (a scan's surfaces), random rotations, log-normal scales, opacities in (0.05, 1)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = torch.rand(n, 3, generator=g) * side
    sheet = torch.randint(0, 3, (n,), generator=g)
    level = torch.randint(1, 8, (n,), generator=g).float() * (side / 8.0)
    m[torch.arange(n), sheet] = level + 0.004 * torch.randn(n, generator=g)
    q = torch.randn(n, 4, generator=g)
    s = 0.006 * torch.exp(0.5 * torch.randn(n, 3, generator=g))
    big = torch.rand(n, generator=g) < 0.002
    s[big] = 0.04 + 0.08 * torch.rand(int(big.sum()), 3, generator=g)
    w = 0.05 + 0.95 * torch.rand(n, generator=g)
    from gaussiangrasper_amd import ops
    rot = ops.quat_to_rotmat(q.to(dev)).reshape(n, 9).contiguous()
    return m.to(dev).contiguous(), rot, s.to(dev).contiguous(), w.to(dev).contiguous()


def torch_paths(dist2, grid, dims, poses, spheres, need, outside):
    """the contract of gg_field_paths in torch operations on the device"""
    P, W = poses.shape[:2]
    T, sp = poses.double(), spheres.double()
    lo = torch.as_tensor(grid[:3], dtype=torch.float64, device=poses.device)
    h = float(grid[3])
    fin = torch.isfinite(poses).all(-1)
    inside = torch.ones(P, W, sp.shape[0], dtype=torch.bool, device=poses.device)
    flat = torch.zeros(P, W, sp.shape[0], dtype=torch.int64, device=poses.device)
    for a in range(3):
        c = (T[..., 3 * a, None] * sp[:, 0] + T[..., 3 * a + 1, None] * sp[:, 1]) + T[..., 3 * a + 2, None] * sp[:, 2]
        c = c + T[..., 9 + a, None]
        d = c - lo[a]
        k = torch.floor(d / h).clamp(-2.0 ** 30, 2.0 ** 30)
        k = torch.where(k * h > d, k - 1.0, torch.where((k + 1.0) * h <= d, k + 1.0, k)).long()
        inside &= torch.isfinite(c) & (k >= 0) & (k < int(dims[a]))
        flat = flat * int(dims[a]) + k.clamp(0, int(dims[a]) - 1)
    dd = torch.where(inside, dist2.reshape(-1)[flat].long(), torch.full_like(flat, int(outside)))
    slack = (dd - need.long()).min(-1).values
    slack = torch.where(fin, slack, torch.full_like(slack, -(1 << 31))).int()
    hit = slack < 0
    first = torch.where(hit.any(1), hit.int().argmax(1), torch.full((P,), W, device=poses.device)).int()
    return slack, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default="profiles/field_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "field_bench needs the GPU"
    from scipy.ndimage import distance_transform_edt
    dev = torch.device("cuda", torch.cuda.current_device())
    side = 2.56
    rows_out = []
    rows = synthetic_rows(a.rows, side, dev)
    fields = {}
    for cells in (256, 128):
        f = field.DistanceField([0.0] * 3, [side] * 3, side / cells, device=dev)
        counts = f.add(rows)
        fields[cells] = f
        if cells == 256:
            reach = np.minimum(field.MAX_REACH, np.ceil(rows[2].max(1).values.cpu().numpy() / f.h) + 1)
            mass = f.mass.clone()
            f.remove(rows)
            assert not bool(f.mass.any()), "+1 then -1 did not restore the zeros"
            f.add(rows)
            assert torch.equal(f.mass, mass), "two builds of the same rows differ"

            def splat():
                field.splat(f.mass, f.grid, f.dims, *rows)
            t = timed(splat, a.reps)
            f.mass.copy_(mass)
            row = {"what": "field.splat (gg_field_splat), mass of 1 cm cells", "rows": a.rows, "cells": [cells] * 3,
                   "extent": field.EXTENT, "max_reach": field.MAX_REACH, "skipped": int(counts.skipped),
                   "truncated": int(counts.truncated), "rows_walked_by_their_wave": int((reach > 2).sum()),
                   "cells_with_mass": int((mass != 0).sum()), "splat": t,
                   "rows_per_second": round(a.rows / (t["ms_median"] * 1e-3))}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
    for cells in (128, 256):
        f = fields[cells]
        f.update()
        occ = (f.mass >= f.threshold).cpu().numpy()
        t0 = time.perf_counter()
        want = np.rint(distance_transform_edt(~occ) ** 2).astype(np.int64)
        host_s = time.perf_counter() - t0
        assert np.array_equal(f.dist2.cpu().numpy().astype(np.int64), want), "dist2 differs from scipy's"
        t = timed(lambda: f.update(), a.reps)
        row = {"what": "field.distance (gg_field_distance) against scipy.ndimage.distance_transform_edt on the host",
               "cells": [cells] * 3, "occupied": int(occ.sum()), "max_dist2": int(want.max()), "distance": t,
               "scipy_host_seconds": round(host_s, 3), "speedup": round(host_s * 1e3 / t["ms_median"], 1)}
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    # paths through the 256^3 field: random poses inside the box, 32 spheres of a 1 cm gripper lattice
    f = fields[256]
    P, W, S = 4096, 64, 32
    g = torch.Generator(device="cpu").manual_seed(1)
    from gaussiangrasper_amd import ops
    R = ops.quat_to_rotmat(torch.randn(P * W, 4, generator=g).to(dev)).reshape(P, W, 9)
    tr = (torch.rand(P, W, 3, generator=g) * (side + 0.2) - 0.1).to(dev)
    poses = torch.cat([R, tr], -1).contiguous()
    spheres = ((torch.rand(S, 3, generator=g) - 0.5) * 0.12).to(dev)
    need = torch.from_numpy(field.need2(np.full(S, 0.01), 0.005, f.h)).to(dev)
    got = field.paths(f.dist2, f.grid, f.dims, poses, spheres, need, field.FAR)
    want = torch_paths(f.dist2, f.grid, f.dims, poses, spheres, need, field.FAR)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "paths differ from the torch restatement"
    row = {"what": "field.paths (gg_field_paths) against a torch gather restatement on the same GPU",
           "paths": P, "waypoints": W, "spheres": S, "paths_hit": int((got[1] < W).sum()),
           "paths_call": timed(lambda: field.paths(f.dist2, f.grid, f.dims, poses, spheres, need, field.FAR), a.reps),
           "torch": timed(lambda: torch_paths(f.dist2, f.grid, f.dims, poses, spheres, need, field.FAR), a.reps)}
    row["speedup"] = round(row["torch"]["ms_median"] / row["paths_call"]["ms_median"], 1)
    rows_out.append(row)
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARMUP, "rows": rows_out}, fh,
                      indent=1)


if __name__ == "__main__":
    main()
