"""GPU time of arm reachability (gg_arm_follow, gg_arm_clear, gg_arm_fk through gaussiangrasper_amd.arm) on the default
arm:

    follow   4096 paths x 16 seeds x 4 waypoints: the gripper poses of configurations that drift by 0.03 rad per
             waypoint, from arm.seeds (the home configuration and 15 random ones); how many (path, seed) pairs follow
             their whole path and the updates they took
    clear    262 144 configurations x 64 spheres (the arm's link spheres and gripper-frame ones up to 64) in the
             256^3 field of tools/route_bench.py's cluttered table, the arm standing in the corner that table keeps open
    fk       the frames of those 262 144 configurations

    python tools/arm_bench.py [--reps 10] [--out profiles/arm_bench.json]

Every GPU figure is the median [min, max] of --reps device-event timings after 3 warm-up calls.  There is no earlier
implementation to compare with."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaussiangrasper_amd import arm as A, field  # noqa: E402
from route_bench import WARMUP, cluttered_table, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--waypoints", type=int, default=4)
    ap.add_argument("--configurations", type=int, default=1 << 18)
    ap.add_argument("--spheres", type=int, default=64)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--out", default="profiles/arm_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "arm_bench needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    model = A.default_arm()
    J = model.num_joints
    rng = np.random.default_rng(0)
    rows = []

    # follow: paths the arm can follow, so that the time is that of useful work
    q0 = rng.uniform(model.lo + 0.4, model.hi - 0.4, size=(a.paths, J))
    drift = 0.03 * np.arange(a.waypoints)[None, :, None] * rng.choice([-1.0, 1.0], size=(a.paths, 1, J))
    qs = torch.from_numpy((q0[:, None, :] + drift).reshape(-1, J)).to(dev)
    poses = A.fk(model, qs)[:, J + 1].float().reshape(a.paths, a.waypoints, 12).contiguous()
    seeds = torch.from_numpy(A.seeds(model, a.paths, a.seeds, seed=1)).to(dev)
    fol = A.follow(model, poses, seeds)
    whole = fol.first_fail == a.waypoints
    it = fol.iters[fol.iters >= 0].double()
    row = {"what": "arm.follow (gg_arm_follow), default arm, default law", "paths": a.paths, "seeds": a.seeds,
           "waypoints": a.waypoints, "pairs_following_the_whole_path": int(whole.sum()),
           "paths_with_such_a_seed": int(whole.any(1).sum()), "updates_mean": round(float(it.mean()), 2),
           "updates_max": int(it.max()), "follow": timed(lambda: A.follow(model, poses, seeds), a.reps)}
    row["pair_waypoints_per_second"] = round(a.paths * a.seeds * a.waypoints / (row["follow"]["ms_median"] * 1e-3), 0)
    rows.append(row)
    print(json.dumps(row), flush=True)

    # clear and fk
    f = cluttered_table(a.cells, dev)
    stood = model.with_base(np.concatenate([np.eye(3).reshape(-1), [0.3, 0.3, 0.35]]))
    c, fr, r = stood.link_spheres()
    extra = max(a.spheres - len(c), 0)
    g = rng.uniform(-0.06, 0.06, size=(extra, 3)).astype(np.float32)
    centres = torch.from_numpy(np.concatenate([c, g])[:a.spheres]).to(dev)
    frame = torch.from_numpy(np.concatenate([fr, np.full(extra, J + 1, np.int32)])[:a.spheres]).to(dev)
    need = torch.from_numpy(field.need2(np.concatenate([r, np.full(extra, 0.01)])[:a.spheres], 0.0, f.h)).to(dev)
    q = torch.from_numpy(rng.uniform(model.lo, model.hi, size=(a.configurations, J))).to(dev)
    slack, worst = A.clear(stood, f.dist2, f.grid, f.dims, q, centres, frame, need)
    row = {"what": "arm.clear (gg_arm_clear), default arm in the cluttered table", "cells": [a.cells] * 3,
           "configurations": a.configurations, "spheres": int(centres.shape[0]), "clear": int((slack >= 0).sum()),
           "clear_call": timed(lambda: A.clear(stood, f.dist2, f.grid, f.dims, q, centres, frame, need), a.reps)}
    row["sphere_tests_per_second"] = round(a.configurations * int(centres.shape[0])
                                           / (row["clear_call"]["ms_median"] * 1e-3), 0)
    rows.append(row)
    print(json.dumps(row), flush=True)
    row = {"what": "arm.fk (gg_arm_fk), default arm", "configurations": a.configurations,
           "fk": timed(lambda: A.fk(stood, q), a.reps)}
    rows.append(row)
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARMUP, "rows": rows}, fh,
                      indent=1)


if __name__ == "__main__":
    main()
