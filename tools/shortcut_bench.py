"""GPU time of the line of sight and of string pulling (gg_field_sight, gg_field_shortcut, and
transit.plan_transit with them) on tools/route_bench.py's synthetic cluttered table at 128^3 and 256^3 cells:

    shortcut   the descended paths of 8 and of 4096 starts pulled taut over their whole length; the path statistics
               (cells in, anchors out, the pulled polyline against the chamfer cost); for the 8 paths at 128^3 next
               to the numpy restatement on the host that walks (tests/shortcut_ref.py shortcut_by_walk; one host
               run, the results compared first)
    sight      1 M random segments, the whole cover of each
    plan       transit.plan_transit end to end with and without shortcut=True: 8 start poses, the default gripper as
               spheres, 64 waypoints (route_bench's setting, whose recorded times are the parent's yardstick)

    python tools/shortcut_bench.py [--reps 10] [--out profiles/shortcut_bench.json]

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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaussiangrasper_amd import field, transit  # noqa: E402
from route_bench import WARMUP, cluttered_table, timed  # noqa: E402


def path_stats(f, cells, length, keep, count, cost_at):
    """cells in, anchors out, and the pulled polyline through the kept centres against the chamfer cost"""
    c, n, k, m = cells.cpu().numpy(), length.cpu().numpy(), keep.cpu().numpy(), count.cpu().numpy()
    cost = cost_at.cpu().numpy().astype(np.float64) / 3.0                    # in cells
    pulled = np.array([np.linalg.norm(np.diff(c[p][k[p, :m[p]]].astype(np.float64), axis=0), axis=1).sum()
                       for p in range(len(n))])
    moving = cost > 0
    return {"cells_in_mean": round(float(n.mean()), 1), "cells_in_max": int(n.max()),
            "anchors_out_mean": round(float(m.mean()), 2), "anchors_out_max": int(m.max()),
            "euclid_over_chamfer_mean": round(float((pulled[moving] / cost[moving]).mean()), 4),
            "euclid_over_chamfer_min": round(float((pulled[moving] / cost[moving]).min()), 4),
            "euclid_over_chamfer_max": round(float((pulled[moving] / cost[moving]).max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cells", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--segments", type=int, default=1 << 20)
    ap.add_argument("--out", default="profiles/shortcut_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "shortcut_bench needs the GPU"
    import shortcut_ref
    from gaussiangrasper_amd.grasp import default_gripper
    dev = torch.device("cuda", torch.cuda.current_device())
    rows_out = []
    goal_point = np.array([[0.3, 0.3, 0.7]])
    for cells in a.cells:
        f = cluttered_table(cells, dev)
        ctg = transit.cost_to_go(f, goal_point, 0.06)
        assert int(ctg.ignored) == 0, "the goal is not free"
        reach = ctg.cost < field.FAR
        rng = np.random.default_rng(1)
        idx = torch.nonzero(reach).cpu().numpy()
        starts = idx[rng.choice(len(idx), 4096, replace=len(idx) < 4096)].astype(np.int32)
        at = ctg.cost[tuple(torch.from_numpy(starts.astype(np.int64)).to(dev).T)]
        _, length = transit.descend_cells(f.dist2, f.dims, ctg.need, ctg.cost, starts, 1)
        room = int(length.max())
        path, length = transit.descend_cells(f.dist2, f.dims, ctg.need, ctg.cost, starts, room)
        for paths in (8, 4096):
            c, n = path[:paths].contiguous(), length[:paths].contiguous()
            keep, count, blocked = transit.shortcut_cells(f.dist2, f.dims, ctg.need, c, n, room)
            assert int(blocked.sum()) == 0, "a kept segment of a descended path is not clear"
            row = {"what": "transit.shortcut_cells (gg_field_shortcut), window = the whole path", "cells": [cells] * 3,
                   "paths": paths, "max_cells": room, **path_stats(f, c, n, keep, count, at[:paths]),
                   "shortcut": timed(lambda: transit.shortcut_cells(f.dist2, f.dims, ctg.need, c, n, room), a.reps)}
            if paths == 8 and cells <= 128:
                d = f.dist2.cpu().numpy()
                t0 = time.perf_counter()
                host = shortcut_ref.shortcut_by_walk(d, ctg.need, c.cpu().numpy(), n.cpu().numpy(), room)
                row["numpy_host_seconds"] = round(time.perf_counter() - t0, 3)
                assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((keep, count, blocked), host)), \
                    "the kernel differs from the restatement"
                row["speedup_over_numpy"] = round(row["numpy_host_seconds"] * 1e3 / row["shortcut"]["ms_median"], 1)
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        # sight: random segments across the volume
        sa = torch.from_numpy(rng.integers(0, cells, size=(a.segments, 3)).astype(np.int32)).to(dev)
        sb = torch.from_numpy(rng.integers(0, cells, size=(a.segments, 3)).astype(np.int32)).to(dev)
        cover, blk = transit.sight(f.dist2, f.dims, ctg.need, sa, sb)
        row = {"what": "transit.sight (gg_field_sight), random segments, the whole cover", "cells": [cells] * 3,
               "segments": a.segments, "cover_mean": round(float(cover.float().mean()), 1),
               "cover_max": int(cover.max()), "clear": int((blk == 0).sum()),
               "sight": timed(lambda: transit.sight(f.dist2, f.dims, ctg.need, sa, sb), a.reps)}
        row["cells_per_second"] = round(float(cover.sum()) / (row["sight"]["ms_median"] * 1e-3), 0)
        rows_out.append(row)
        print(json.dumps(row), flush=True)
        del sa, sb, cover, blk
        # end to end, route_bench's setting
        spheres = field.gripper_spheres(default_gripper(), 0.08, 0.02, 0.02, 0.01)
        eye = np.eye(3).reshape(-1)
        goal_p = np.concatenate([eye, goal_point[0]]).astype(np.float32)
        ball = transit.cost_to_go(f, goal_point, transit.planning_radius(spheres, 0.01, f.h))
        far_half = torch.nonzero((ball.cost < field.FAR)[cells // 2:, cells // 2:]).cpu().numpy() + [cells // 2, cells // 2, 0]
        assert len(far_half) >= 8, "the gripper's ball reaches no cell of the far half of the table"
        pos = transit.cell_centres(f, far_half[rng.choice(len(far_half), 8, replace=False)])
        starts_p = np.stack([np.concatenate([eye, t]) for t in pos]).astype(np.float32)
        row = {"what": "transit.plan_transit end to end (cost field, descent, [shortcut,] host poses, "
                       "field.path_clear)", "cells": [cells] * 3, "starts": 8, "waypoints": transit.STEPS,
               "spheres": int(len(spheres))}
        for name, pull in (("plain", False), ("shortcut", True)):
            plan = transit.plan_transit(f, starts_p, goal_p, spheres, 0.01, shortcut=pull)
            assert bool((plan.clearance.clear.cpu().numpy() | ~plan.planned).all()), "a planned path is not clear"
            wall0 = time.perf_counter()
            t = timed(lambda: transit.plan_transit(f, starts_p, goal_p, spheres, 0.01, shortcut=pull), a.reps)
            row[name] = {"planned": int(plan.planned.sum()), "clear": int(plan.clearance.clear.sum()),
                         "best": plan.best, "plan": t, "euclid_mean": round(float(plan.euclid[plan.planned].mean()), 4),
                         "cost_mean": round(float(plan.cost[plan.planned].mean()), 4),
                         "min_slack": int(plan.clearance.slack.min()),
                         "host_wall_seconds_per_call": round((time.perf_counter() - wall0) / (a.reps + WARMUP), 4)}
            if pull:
                row[name]["cells_in_mean"] = round(float(plan.length.float().mean()), 1)
                row[name]["anchors_out_mean"] = round(float(plan.count.float().mean()), 2)
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARMUP, "rows": rows_out}, fh,
                      indent=1)


if __name__ == "__main__":
    main()
