"""GPU time of the arm's motion test (gg_arm_motion through gaussiangrasper_amd.arm.motion) on the default arm, against
the only route there was before it: the samples expanded in torch, arm.clear on all of them, arm.fk plus torch pair
distances for the gaps.

    short    the edges w -> w + 1 of tools/arm_bench.py's follow run (4096 paths x 16 seeds x 4 waypoints: 196 608
             edges, those of failed seeds NaN), in the 256^3 field of tools/route_bench.py's cluttered table
    long     4096 edges between configurations uniform in the limits, cut to n of about 100 to 300 samples

    python tools/arm_motion_bench.py [--reps 10] [--out profiles/arm_motion_bench.json]

Every GPU figure is the median [min, max] of --reps device-event timings after 3 warm-up calls.  The two routes must
agree: samples, slack, slack_at and worst exactly, gap within 1e-12.  (gap_at and pair are the first of equals in each
route's own arithmetic; the default arm has sphere pairs at a constant distance, shoulder to elbow, whose gap is the
smallest at every sample of many edges, so the share of edges on which the routes name the same sample is reported, not
required.)"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaussiangrasper_amd import arm as A, field  # noqa: E402
from route_bench import WARMUP, cluttered_table, timed  # noqa: E402

INT32_MIN = -(1 << 31)


def torch_motion(model, f, q_a, q_b, centres, frame, need, radius, reach, table, res, max_samples, chunk):
    """the contract of gg_arm_motion from arm.clear, arm.fk and torch, `chunk` edges at a time"""
    dev = q_a.device
    E, J = q_a.shape
    S = centres.shape[0]
    dq = q_b - q_a
    b = torch.zeros(E, S, dtype=torch.float64, device=dev)
    for j in range(J):                                              # j ascending onto 0.0
        b = b + dq[:, j].abs()[:, None] * reach[j][None, :]
    B = b.amax(1)
    fin = torch.isfinite(q_a).all(1) & torch.isfinite(q_b).all(1)
    resolved = fin & ~(B > float(max_samples) * res)
    Bs = torch.where(resolved, B, torch.zeros_like(B))
    n = torch.ceil(Bs / res).clamp(1, max_samples).long()
    n = n + ((n.double() * res < Bs) & (n < max_samples)).long()
    n = n - ((n > 1) & ((n - 1).double() * res >= Bs)).long()
    n = torch.where(resolved, n, torch.zeros_like(n))
    fr = frame.long()
    s_idx, t_idx = torch.triu_indices(S, S, 1, device=dev)
    on = torch.as_tensor(table, device=dev)[fr[s_idx], fr[t_idx]] != 0
    s_idx, t_idx = s_idx[on], t_idx[on]
    rsum = radius[s_idx] + radius[t_idx]
    cx, cy, cz = (centres[:, a].double()[None, :] for a in range(3))
    out = dict(samples=n.int(), slack=torch.full((E,), INT32_MIN, dtype=torch.int32, device=dev),
               slack_at=torch.full((E,), -1, dtype=torch.int32, device=dev),
               worst=torch.full((E,), -1, dtype=torch.int32, device=dev),
               gap=torch.full((E,), float("nan"), dtype=torch.float64, device=dev),
               gap_at=torch.full((E,), -1, dtype=torch.int32, device=dev))
    for lo in range(0, E, chunk):
        rows = torch.nonzero(resolved[lo:lo + chunk])[:, 0] + lo
        if not len(rows):
            continue
        nn = n[rows]
        m = int(nn.max()) + 1
        i = torch.arange(m, device=dev)
        q = q_a[rows, None, :] + (i[None, :].double() / nn[:, None].double())[:, :, None] * dq[rows, None, :]
        q[torch.arange(len(rows), device=dev), nn] = q_b[rows]
        valid = i[None, :] <= nn[:, None]
        flat = q.reshape(-1, J)
        sl, wo = A.clear(model, f.dist2, f.grid, f.dims, flat, centres, frame, need)
        key = sl.reshape(len(rows), m).long() * 8192 + i[None, :]    # the smallest slack, then the first sample
        key = torch.where(valid, key, torch.full_like(key, 1 << 62)).amin(1)
        at = key - torch.div(key, 8192, rounding_mode="floor") * 8192
        out["slack"][rows] = torch.div(key, 8192, rounding_mode="floor").int()
        out["slack_at"][rows] = at.int()
        out["worst"][rows] = wo.reshape(len(rows), m)[torch.arange(len(rows), device=dev), at]
        T = A.fk(model, flat)[:, fr]                                # (N, S, 12)
        cen = torch.stack([((T[..., 3 * a] * cx + T[..., 3 * a + 1] * cy) + T[..., 3 * a + 2] * cz) + T[..., 9 + a]
                           for a in range(3)], -1)
        d = cen[:, s_idx] - cen[:, t_idx]
        g = torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) - rsum[None, :]
        g = g.amin(1).reshape(len(rows), m)
        g = torch.where(valid, g, torch.full_like(g, float("inf")))
        best = g.amin(1)
        out["gap"][rows] = best
        first = torch.where(g == best[:, None], i[None, :], torch.full_like(i, m)[None, :]).amin(1)
        out["gap_at"][rows] = first.int()
    return out


def compare(m, t):
    same = {k: bool(torch.equal(getattr(m, k), t[k])) for k in ("samples", "slack", "slack_at", "worst")}
    fin = torch.isfinite(t["gap"])
    same["gap_nan_alike"] = bool(torch.equal(torch.isnan(m.gap), torch.isnan(t["gap"])))
    dev = float((m.gap[fin] - t["gap"][fin]).abs().max()) if bool(fin.any()) else 0.0
    same["gap_max_abs_difference"] = dev
    same["gap_at_same_share"] = round(float((m.gap_at == t["gap_at"]).double().mean()), 4)
    ok = all(v for k, v in same.items() if isinstance(v, bool)) and dev <= 1e-12
    return ok, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--waypoints", type=int, default=4)
    ap.add_argument("--long-edges", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--out", default="profiles/arm_motion_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "arm_motion_bench needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    f = cluttered_table(a.cells, dev)
    model = A.default_arm().with_base(np.concatenate([np.eye(3).reshape(-1), [0.3, 0.3, 0.35]]))
    J = model.num_joints
    c, fr, r = model.link_spheres()
    table = A.default_self_pairs(model)
    res = f.h
    centres, frame = torch.from_numpy(c).to(dev), torch.from_numpy(fr).to(dev)
    need = torch.from_numpy(field.need2(r + 0.5 * res, 0.0, f.h)).to(dev)
    radius = torch.from_numpy(r).to(dev)
    reach = torch.from_numpy(model.reach_table()).to(dev)
    rows = []

    def measure(what, q_a, q_b, chunk, extra):
        def run():
            return A.motion(model, q_a, q_b, f, pairs=table)

        def ref():
            return torch_motion(model, f, q_a, q_b, centres, frame, need, radius, reach, table, res, A.MAX_SAMPLES,
                                chunk)
        m, t = run(), ref()
        ok, same = compare(m, t)
        n = m.samples.long()
        row = {"what": what, "cells": [a.cells] * 3, "res": res, "edges": int(q_a.shape[0]), "spheres": len(c),
               "tested_pairs": int(sum(table[fr[s], fr[u]] for s in range(len(c)) for u in range(s + 1, len(c)))),
               "resolved_edges": int((n > 0).sum()), "samples_total": int((n + (n > 0).long()).sum()),
               "samples_per_edge": [int(n[n > 0].min()), float(n[n > 0].double().mean().round()), int(n.max())],
               "ok_edges": int(m.ok.sum()), **extra, "routes_agree": ok, "agreement": same,
               "motion": timed(run, a.reps), "torch_route": timed(ref, a.torch_reps, 1)}
        row["speedup"] = round(row["torch_route"]["ms_median"] / row["motion"]["ms_median"], 1)
        row["samples_per_second"] = round(row["samples_total"] / (row["motion"]["ms_median"] * 1e-3), 0)
        rows.append(row)
        print(json.dumps(row), flush=True)
        assert ok, same

    # short: the edges of arm_bench's follow run
    q0 = rng.uniform(model.lo + 0.4, model.hi - 0.4, size=(a.paths, J))
    drift = 0.03 * np.arange(a.waypoints)[None, :, None] * rng.choice([-1.0, 1.0], size=(a.paths, 1, J))
    qs = torch.from_numpy((q0[:, None, :] + drift).reshape(-1, J)).to(dev)
    poses = A.fk(model, qs)[:, J + 1].float().reshape(a.paths, a.waypoints, 12).contiguous()
    fol = A.follow(model, poses, torch.from_numpy(A.seeds(model, a.paths, a.seeds, seed=1)).to(dev))
    q_a = fol.q[:, :, :-1].reshape(-1, J).contiguous()
    q_b = fol.q[:, :, 1:].reshape(-1, J).contiguous()
    measure("arm.motion (gg_arm_motion), the edges of a follow run", q_a, q_b, 16384,
            {"paths": a.paths, "seeds": a.seeds, "waypoints": a.waypoints})

    # long: uniform in the limits, cut so that n is about 100 to 300
    lo, hi = np.asarray(model.lo), np.asarray(model.hi)
    start = rng.uniform(lo, hi, size=(a.long_edges, J))
    end = rng.uniform(lo, hi, size=(a.long_edges, J))
    B = (np.abs(end - start)[:, :, None] * model.reach_table()[None]).sum(1).max(1)
    end = start + (end - start) * (rng.uniform(100.0, 300.0, size=a.long_edges) * res / B)[:, None]
    measure("arm.motion (gg_arm_motion), long edges", torch.from_numpy(start).to(dev), torch.from_numpy(end).to(dev),
            a.chunk, {})
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch_reps": a.torch_reps,
                       "warmup": WARMUP, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
