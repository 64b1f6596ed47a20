"""GPU time of the two placement calls (gaussiangrasper_amd.place on gg_height_map and gg_place_search) at the sizes of
a table-top scene:

    height_map  1 M points into a 256 x 256 map, for 1 frame and for 16 frames in one call
    search      a 256 x 256 scene map, a 64 x 64 footprint about 60 % full, 16 yaws, tol 2; next to it a torch
                restatement on the same GPU (a running torch.maximum over shifted slices, then the count and the sums
                the same way) and the numpy restatement of tests/place_ref.py on one core (one run; --no-host skips it).
                The results are compared first.

    python tools/place_bench.py [--reps 10] [--points 1000000] [--out profiles/place_bench.json]

Every GPU figure is the median [min, max] of --reps device-event timings after 3 warm-up calls."""
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
from gaussiangrasper_amd import place  # noqa: E402

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


def torch_search(top, under, tol):
    """the contract of gg_place_search in torch operations on the device: per yaw a loop over the object's cells, every
    anchor at once (int32; EMPTY scene cells are tracked apart)"""
    (U, V), (K, A, B) = top.shape, under.shape
    I, J = U - A + 1, V - B + 1
    E = place.EMPTY
    rest = torch.full((K, I, J), E, dtype=torch.int32, device=top.device)
    contact = torch.zeros((K, I, J), dtype=torch.int32, device=top.device)
    support = torch.tensor([0, 0, -1, -1, -1, -1], dtype=torch.int32, device=top.device).repeat(K, I, J, 1)
    hole = top == E
    host = under.cpu().numpy()
    for k in range(K):
        cells = np.argwhere(host[k] != E)
        if len(cells) == 0:
            continue
        best = torch.full((I, J), E, dtype=torch.int32, device=top.device)
        bad = torch.zeros((I, J), dtype=torch.bool, device=top.device)
        for a, b in cells:
            bad |= hole[a:a + I, b:b + J]
            best = torch.maximum(best, top[a:a + I, b:b + J] + int(host[k, a, b]))
        thr = best - int(tol)
        acc = torch.zeros((3, I, J), dtype=torch.int32, device=top.device)
        lo = torch.full((2, I, J), 1 << 20, dtype=torch.int32, device=top.device)
        hi = torch.full((2, I, J), -1, dtype=torch.int32, device=top.device)
        for a, b in cells:
            c = top[a:a + I, b:b + J] + int(host[k, a, b]) >= thr
            ci = c.int()
            acc[0] += ci
            acc[1] += ci * int(a)
            acc[2] += ci * int(b)
            for axis, v in ((0, int(a)), (1, int(b))):
                lo[axis] = torch.where(c, lo[axis].clamp(max=v), lo[axis])
                hi[axis] = torch.where(c, hi[axis].clamp(min=v), hi[axis])
        ok = ~bad
        rest[k] = torch.where(ok, best, rest[k])
        contact[k] = torch.where(ok, acc[0], contact[k])
        sup = torch.stack([acc[1], acc[2], lo[0], hi[0], lo[1], hi[1]], -1)
        support[k] = torch.where(ok[..., None], sup, support[k])
    return rest, contact, support


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement's run")
    ap.add_argument("--out", default="profiles/place_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "place_bench needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    rows_out = []
    # height maps: a noisy table with a few boxes on it, seen in frames turned about the normal
    g = torch.Generator(device="cpu").manual_seed(0)
    n, side, cell, level = a.points, 1.28, 0.005, 0.001
    pts = torch.rand(n, 3, generator=g) * torch.tensor([side, side, 0.0]) + torch.tensor([0.0, 0.0, 0.001]) * \
        torch.randn(n, 1, generator=g)
    box = torch.rand(n, generator=g) < 0.2
    pts[box, 2] += torch.randint(1, 6, (int(box.sum()),), generator=g).float() * 0.03
    pts = pts.to(dev).contiguous()
    w = (0.05 + 0.95 * torch.rand(n, generator=g)).to(dev)
    frame = place.plane_frame(((0.0, 0.0, 1.0), 0.0), (side / 2, side / 2, 0.0))
    grid, dims = place.plane_grid((-side / 2, -side / 2, side / 2, side / 2), cell, level)
    for F in (1, 16):
        frames = place.yaw_frames(frame, frame.o, F, 0, 0, cell)
        m, dropped = place.height_map(pts, w, frames, grid, dims, 0.1)
        again, _ = place.height_map(pts, w, frames, grid, dims, 0.1)
        assert torch.equal(m, again), "two height maps of the same points differ"
        out = torch.empty_like(m)

        def call():
            out.fill_(place.EMPTY)
            place.height_map(pts, w, frames, grid, dims, 0.1, out=out)
        t = timed(call, a.reps)
        row = {"what": "place.height_map (gg_height_map; the map's fill and the frames' upload are inside)",
               "points": n, "frames": F, "cells": [int(d) for d in dims], "filled": int((m != place.EMPTY).sum()),
               "dropped": [int(d) for d in dropped.cpu()][:4], "height_map": t,
               "point_frames_per_second": round(n * F / (t["ms_median"] * 1e-3))}
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    # the search
    rng = np.random.default_rng(1)
    U = V = 256
    A = B = 64
    K = 16
    top = rng.integers(0, 4, size=(U, V)).astype(np.int32)
    for _ in range(12):                                               # boxes on the table
        i, j = rng.integers(0, U - 30), rng.integers(0, V - 30)
        top[i:i + rng.integers(8, 30), j:j + rng.integers(8, 30)] = rng.integers(20, 200)
    ii, jj = np.meshgrid(np.arange(A) - A / 2 + 0.5, np.arange(B) - B / 2 + 0.5, indexing="ij")
    under = np.full((K, A, B), place.EMPTY, np.int32)
    for k in range(K):                                        # an ellipse of about 60 % of the footprint, turned
        t = k * np.pi / K
        x, y = np.cos(t) * ii + np.sin(t) * jj, -np.sin(t) * ii + np.cos(t) * jj
        inside = (x / 31.5) ** 2 + (y / 24.5) ** 2 <= 1.0
        under[k][inside] = (-3 - rng.integers(0, 3, size=int(inside.sum()))).astype(np.int32)
    top_d, under_d = torch.from_numpy(top).to(dev), torch.from_numpy(under).to(dev)
    got = place.search(top_d, under_d, place.TOL)
    want = torch_search(top_d, under_d, place.TOL)
    for name, x, y in zip(("rest", "contact", "support"), (got.rest, got.contact, got.support), want):
        assert torch.equal(x, y), f"{name} differs from the torch restatement"
    cells = int((under != place.EMPTY).sum())
    I, J = U - A + 1, V - B + 1
    row = {"what": "place.search (gg_place_search) against a torch restatement on the same GPU and numpy on one core",
           "scene": [U, V], "footprint": [A, B], "yaws": K, "tol": place.TOL, "object_cells": cells,
           "fill": round(cells / (K * A * B), 3), "anchor_cell_pairs": I * J * cells,
           "search": timed(lambda: place.search(top_d, under_d, place.TOL), a.reps),
           "torch": timed(lambda: torch_search(top_d, under_d, place.TOL), max(1, a.reps // 5))}
    row["pairs_per_second_both_sweeps"] = round(2 * I * J * cells / (row["search"]["ms_median"] * 1e-3))
    row["speedup_over_torch"] = round(row["torch"]["ms_median"] / row["search"]["ms_median"], 1)
    if not a.no_host:
        import place_ref
        t0 = time.perf_counter()
        host = place_ref.search(top, under, place.TOL)
        row["numpy_one_core_seconds"] = round(time.perf_counter() - t0, 2)
        for name, x, y in zip(("rest", "contact", "support"), (got.rest, got.contact, got.support), host):
            assert np.array_equal(x.cpu().numpy(), y), f"{name} differs from the numpy restatement"
        row["speedup_over_numpy"] = round(row["numpy_one_core_seconds"] * 1e3 / row["search"]["ms_median"], 1)
    rows_out.append(row)
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARMUP, "rows": rows_out}, fh,
                      indent=1)


if __name__ == "__main__":
    main()
