"""GPU time of transit planning (gaussiangrasper_amd.transit on gg_field_route and gg_field_descend) on a synthetic
cluttered table, the same scene at 128^3 and 256^3 cells:

    route      the cost field from one goal for a ball of 6 cm, and the rounds it took; next to a torch restatement
               on the same GPU (whole-volume Jacobi sweeps of shifted slices until the costs stop changing; the
               results are compared first) and, at 128^3, next to scipy's Dijkstra on the host (tests/route_ref.py;
               one host run, compared too)
    descend    4096 starts down that cost field
    plan       transit.plan_transit end to end: 8 start poses, the default gripper as spheres, 64 waypoints

    python tools/route_bench.py [--reps 10] [--out profiles/route_bench.json]

Every GPU figure is the median [min, max] of --reps device-event timings after 3 warm-up calls; the torch sweeps are
timed --torch-reps times after one warm-up call (they take seconds)."""
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
from gaussiangrasper_amd import field, transit  # noqa: E402

WARMUP = 3
SIDE = 2.56
MOVES = [(m, m // 9 - 1, (m // 3) % 3 - 1, m % 3 - 1) for m in range(27) if m != 13]


def timed(fn, reps, warmup=WARMUP):
    for _ in range(warmup):
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


def cluttered_table(cells, dev, seed=0):
    """A DistanceField of SIDE^3 with a table slab and 60 boxes standing on it, some reaching the top; the occupancy
    is written straight into the mass (one vote per occupied cell)"""
    f = field.DistanceField([0.0] * 3, [SIDE] * 3, SIDE / cells, device=dev)
    c = (torch.arange(cells, device=dev, dtype=torch.float64) + 0.5) * f.h
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    occ = z < 0.2
    rng = np.random.default_rng(seed)
    for _ in range(60):
        cx, cy = rng.uniform(0.2, SIDE - 0.2, 2)
        wx, wy = rng.uniform(0.05, 0.25, 2)
        if abs(cx - 0.3) < 0.3 + wx and abs(cy - 0.3) < 0.3 + wy:    # 30 cm around the goal stay open
            continue
        top = SIDE if rng.random() < 0.3 else rng.uniform(0.4, 1.6)
        occ |= ((x - cx).abs() < wx) & ((y - cy).abs() < wy) & (z < top)
    f.mass.copy_(occ.to(torch.int64) * field.VOTE_ONE)
    return f.update()


def _shifted(a, dx, dy, dz, fill):
    """out[c] = a[c + d], `fill` where c + d is outside"""
    out = torch.full_like(a, fill)
    X, Y, Z = a.shape
    sx, tx = slice(max(0, -dx), X - max(0, dx)), slice(max(0, dx), X - max(0, -dx))
    sy, ty = slice(max(0, -dy), Y - max(0, dy)), slice(max(0, dy), Y - max(0, -dy))
    sz, tz = slice(max(0, -dz), Z - max(0, dz)), slice(max(0, dz), Z - max(0, -dz))
    out[sx, sy, sz] = a[tx, ty, tz]
    return out


def torch_allowed(dist2, need):
    free = dist2 >= need
    out = []
    for m, dx, dy, dz in MOVES:
        ok = free.clone()
        for ex in {0, dx}:
            for ey in {0, dy}:
                for ez in {0, dz}:
                    if (ex, ey, ez) != (0, 0, 0):
                        ok &= _shifted(free, ex, ey, ez, False)
        out.append(ok)
    return free, out


def torch_route(free, allowed, goal, check_every=8):
    """the contract of gg_field_route in whole-volume torch sweeps -> (cost, sweeps)"""
    far = field.FAR
    cost = torch.full(free.shape, far, dtype=torch.int32, device=free.device)
    if bool(free[tuple(goal)]):
        cost[tuple(goal)] = 0
    sweeps = 0
    while True:
        before = cost
        for _ in range(check_every):
            new = cost
            for (m, dx, dy, dz), ok in zip(MOVES, allowed):
                w = 2 + (dx != 0) + (dy != 0) + (dz != 0)
                new = torch.minimum(new, torch.where(ok, _shifted(cost, dx, dy, dz, far) + w, far))
            cost = new
            sweeps += 1
        if torch.equal(cost, before):
            return cost, sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--cells", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default="profiles/route_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "route_bench needs the GPU"
    import route_ref
    from gaussiangrasper_amd.grasp import default_gripper
    dev = torch.device("cuda", torch.cuda.current_device())
    rows_out = []
    goal_point = np.array([[0.3, 0.3, 0.7]])
    for cells in a.cells:
        f = cluttered_table(cells, dev)
        ctg = transit.cost_to_go(f, goal_point, 0.06)
        goal = ctg.goals[0]
        assert int(ctg.ignored) == 0, "the goal is not free"
        free, allowed = torch_allowed(f.dist2, ctg.need)
        want, sweeps = torch_route(free, allowed, goal)
        assert torch.equal(ctg.cost, want), "cost differs from the torch restatement"
        reach = ctg.cost < field.FAR
        row = {"what": "transit.cost_to_go (gg_field_route) against whole-volume torch Jacobi sweeps on the same GPU",
               "cells": [cells] * 3, "need": ctg.need, "free_cells": int(free.sum()), "reached_cells": int(reach.sum()),
               "max_cost": int(ctg.cost[reach].max()), "rounds": ctg.rounds, "torch_sweeps": sweeps,
               "route": timed(lambda: transit.route(f.dist2, f.dims, ctg.need, ctg.goals, out=ctg.cost), a.reps),
               "torch": timed(lambda: torch_route(free, allowed, goal), a.torch_reps, warmup=1),
               "torch_reps": a.torch_reps}
        row["speedup_over_torch"] = round(row["torch"]["ms_median"] / row["route"]["ms_median"], 1)
        if cells <= 128:
            d = f.dist2.cpu().numpy()
            t0 = time.perf_counter()
            host, _ = route_ref.route(d, ctg.need, ctg.goals)
            row["scipy_host_seconds"] = round(time.perf_counter() - t0, 3)
            assert np.array_equal(ctg.cost.cpu().numpy(), host), "cost differs from scipy's Dijkstra"
            row["speedup_over_scipy"] = round(row["scipy_host_seconds"] * 1e3 / row["route"]["ms_median"], 1)
        del allowed, want
        rows_out.append(row)
        print(json.dumps(row), flush=True)
        # the descent: 4096 starts among the reached cells
        rng = np.random.default_rng(1)
        idx = torch.nonzero(reach).cpu().numpy()
        starts = idx[rng.choice(len(idx), 4096, replace=len(idx) < 4096)].astype(np.int32)
        _, length = transit.descend_cells(f.dist2, f.dims, ctg.need, ctg.cost, starts, 1)
        room = int(length.max())
        st = torch.from_numpy(starts).to(dev)
        row = {"what": "transit.descend_cells (gg_field_descend)", "cells": [cells] * 3, "paths": 4096,
               "longest_path_cells": room, "mean_path_cells": round(float(length.float().mean()), 1),
               "descend": timed(lambda: transit.descend_cells(f.dist2, f.dims, ctg.need, ctg.cost, st, room), a.reps)}
        rows_out.append(row)
        print(json.dumps(row), flush=True)
        # end to end
        spheres = field.gripper_spheres(default_gripper(), 0.08, 0.02, 0.02, 0.01)
        eye = np.eye(3).reshape(-1)
        goal_p = np.concatenate([eye, goal_point[0]]).astype(np.float32)
        # 8 starts the gripper's ball can stand at, in the half of the table away from the goal
        ball = transit.cost_to_go(f, goal_point, transit.planning_radius(spheres, 0.01, f.h))
        far_half = torch.nonzero((ball.cost < field.FAR)[cells // 2:, cells // 2:]).cpu().numpy() + [cells // 2, cells // 2, 0]
        assert len(far_half) >= 8, "the gripper's ball reaches no cell of the far half of the table"
        at = transit.cell_centres(f, far_half[rng.choice(len(far_half), 8, replace=False)])
        starts_p = np.stack([np.concatenate([eye, t]) for t in at]).astype(np.float32)
        plan = transit.plan_transit(f, starts_p, goal_p, spheres, 0.01)
        wall0 = time.perf_counter()
        t = timed(lambda: transit.plan_transit(f, starts_p, goal_p, spheres, 0.01), a.reps)
        row = {"what": "transit.plan_transit end to end (cost field, descent, host poses, field.path_clear)",
               "cells": [cells] * 3, "starts": 8, "waypoints": transit.STEPS, "spheres": int(len(spheres)),
               "planned": int(plan.planned.sum()), "clear": int(plan.clearance.clear.sum()), "best": plan.best,
               "rounds": plan.cost_to_go.rounds, "plan": t,
               "host_wall_seconds_per_call": round((time.perf_counter() - wall0) / (a.reps + WARMUP), 4)}
        assert bool((plan.clearance.clear.cpu().numpy() | ~plan.planned).all()), "a planned path is not clear"
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARMUP, "rows": rows_out}, fh,
                      indent=1)


if __name__ == "__main__":
    main()
