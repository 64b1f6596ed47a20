"""GPU time of the arm roadmap (gaussiangrasper_amd.roadmap) on the default arm in the 256^3 field of
tools/route_bench.py's cluttered table: every stage of `build` on its own, then `route` for 256 goal sets and `descend`.
Each new kernel is measured against the route there was before it for the same result:

    neighbours   chunked fp64 pairwise distances in torch (the header's operation order) plus torch.topk; compared on
                 the rows where torch's unspecified tie order cannot matter (no two of the k + 1 smallest are equal)
    route        a torch pull relaxation: gather and amin over the degree-padded rows, run to a fixed point; the
                 results must be equal.  scipy's Dijkstra on the host is recorded beside it as a CPU figure.

    python tools/roadmap_bench.py [--reps 10] [--out profiles/roadmap_bench.json]

Every GPU figure is the median [min, max] of --reps device-event timings after 3 warm-up calls; `spread` is (max -
min) / median of the kernel's own timings.  No time is asserted."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaussiangrasper_amd import arm as A, roadmap as R  # noqa: E402
from route_bench import WARMUP, cluttered_table, timed  # noqa: E402

FAR = R.FAR


def torch_neighbours(nodes, metric, valid, k, chunk):
    """the k nearest valid nodes of every node but itself: d2 in the header's order, then torch.topk"""
    N, J = nodes.shape
    m = torch.as_tensor(metric, device=nodes.device)
    idx = torch.empty(N, k, dtype=torch.int64, device=nodes.device)
    d2 = torch.empty(N, k, dtype=torch.float64, device=nodes.device)
    off = torch.where(valid != 0, 0.0, float("inf")).double()
    for lo in range(0, N, chunk):
        q = nodes[lo:lo + chunk]
        e = m[0] * (q[:, None, 0] - nodes[None, :, 0])
        d = e * e
        for j in range(1, J):
            e = m[j] * (q[:, None, j] - nodes[None, :, j])
            d = d + e * e
        d = d + off[None, :]
        rows = torch.arange(q.shape[0], device=nodes.device)
        d[rows, rows + lo] = float("inf")
        d2[lo:lo + chunk], idx[lo:lo + chunk] = torch.topk(d, k, dim=1, largest=False, sorted=True)
    return idx, d2


def torch_route(offsets, targets, weights, goals, N, chunk):
    """pull relaxation over the degree-padded rows to a fixed point; (cost (Q, N) int32, rounds)"""
    dev = targets.device
    deg = (offsets[1:] - offsets[:-1]).long()
    D = max(int(deg.max()), 1)
    col = torch.arange(D, device=dev)[None, :]
    at = (offsets[:-1].long()[:, None] + col).clamp(max=max(targets.shape[0] - 1, 0))
    live = col < deg[:, None]
    tpad = torch.where(live, targets[at].long(), torch.zeros_like(at))
    wpad = torch.where(live, weights[at], torch.full_like(at, FAR, dtype=torch.int32))
    Q = len(goals)
    cost = torch.full((Q, N), FAR, dtype=torch.int32, device=dev)
    cost[torch.arange(Q, device=dev), torch.as_tensor(goals, device=dev)] = 0
    rounds = 0
    while True:
        rounds += 1
        changed = False
        for lo in range(0, Q, chunk):
            c = cost[lo:lo + chunk]
            new = torch.minimum(c, (c[:, tpad].long() + wpad[None].long()).amin(2).clamp(max=FAR).int())
            changed = changed or bool((new != c).any())
            cost[lo:lo + chunk] = new
        if not changed:
            return cost, rounds


def spread(t):
    return round((t["ms_max"] - t["ms_min"]) / t["ms_median"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=16384)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--out", default="profiles/roadmap_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "roadmap_bench needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    f = cluttered_table(a.cells, dev)
    model = A.default_arm().with_base(np.concatenate([np.eye(3).reshape(-1), [0.3, 0.3, 0.35]]))
    J = model.num_joints
    rows = []

    def record(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    # the stages of build, each on its own
    nodes = R.sample_nodes(model, a.nodes, 0)
    nt = torch.from_numpy(nodes).to(dev)
    metric = R.default_metric(model)
    own = A.motion(model, nt, nt, f)
    valid = own.ok.to(torch.uint8)
    record({"what": "build: the node test (arm.motion, zero-length moves)", "nodes": a.nodes, "cells": [a.cells] * 3,
            "res": f.h, "valid_nodes": int(valid.sum()), "time": timed(lambda: A.motion(model, nt, nt, f), a.reps)})

    idx, d2 = R.neighbours(nt, a.k, metric, valid=valid)
    t_idx, t_d2 = torch_neighbours(nt, metric, valid, a.k + 1, 1024)
    clean = (t_d2[:, 1:] > t_d2[:, :-1]).all(1) & torch.isfinite(t_d2).all(1)     # no tie among the k + 1 smallest
    agree = bool(torch.equal(idx[clean].long(), t_idx[clean][:, :a.k])) and bool(torch.equal(d2[clean], t_d2[clean][:, :a.k]))
    t_new = timed(lambda: R.neighbours(nt, a.k, metric, valid=valid), a.reps)
    t_old = timed(lambda: torch_neighbours(nt, metric, valid, a.k, 1024), a.torch_reps, 1)
    record({"what": "build: neighbours (gg_roadmap_neighbours), every node against all", "nodes": a.nodes, "k": a.k,
            "joints": J, "rows_compared": int(clean.sum()), "rows_with_ties_left_out": int((~clean).sum()),
            "routes_agree": agree, "neighbours": t_new, "spread": spread(t_new), "torch_route": t_old,
            "speedup": round(t_old["ms_median"] / t_new["ms_median"], 1)})
    assert agree

    hidx = idx.cpu().numpy()
    hidx[valid.cpu().numpy() == 0] = -1
    ea, eb = R.candidate_pairs(np.arange(a.nodes), hidx, a.nodes)
    qa, qb = torch.from_numpy(nodes[ea]).to(dev), torch.from_numpy(nodes[eb]).to(dev)
    m = A.motion(model, qa, qb, f)
    n = m.samples.long()
    record({"what": "build: the edge test (arm.motion, one call)", "edges": len(ea), "resolved_edges": int((n > 0).sum()),
            "ok_edges": int(m.ok.sum()), "samples_total": int((n + (n > 0).long()).sum()),
            "samples_per_edge": [int(n[n > 0].min()), float(n[n > 0].double().mean().round()), int(n.max())],
            "time": timed(lambda: A.motion(model, qa, qb, f), a.reps)})

    ed2 = R.metric_d2(nodes[ea], nodes[eb], metric)
    w = R.edge_weights(ed2, R.UNIT)
    ok = m.ok.cpu().numpy() & (w <= R.MAX_WEIGHT)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        offsets, targets, weights = R.assemble(a.nodes, ea, eb, ok, w)
        ts.append((time.perf_counter() - t0) * 1e3)
    record({"what": "build: assemble (numpy on the host, a CPU figure)", "directed_edges": int(len(targets)),
            "max_degree": int(np.diff(offsets).max()), "dropped_as_too_long": int((m.ok.cpu().numpy() & ~ok).sum()),
            "ms_median": round(float(np.median(ts)), 3), "ms_min": round(float(np.min(ts)), 3),
            "ms_max": round(float(np.max(ts)), 3)})

    # route for Q goal sets, one goal each, and descend
    rng = np.random.default_rng(1)
    live = np.nonzero(np.diff(offsets) > 0)[0]
    goals = rng.choice(live, a.queries, replace=False)
    sets = [[int(g)] for g in goals]
    cost, ignored, rounds = R.route_csr(offsets, targets, weights, R.MAX_WEIGHT, sets, device=dev)
    ot, tt, wt = (torch.from_numpy(x).to(dev) for x in (offsets, targets, weights))
    t_cost, t_rounds = torch_route(ot, tt, wt, goals, a.nodes, 32)
    same = bool(torch.equal(cost, t_cost))
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    graph = csr_matrix((weights.astype(np.float64), targets, offsets), shape=(a.nodes, a.nodes))
    t0 = time.perf_counter()
    dj = dijkstra(graph.T.tocsr(), directed=True, indices=goals)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    same_cpu = bool(np.array_equal(np.where(np.isfinite(dj), dj, FAR).astype(np.int32), cost.cpu().numpy()))
    t_new = timed(lambda: R.route_csr(offsets, targets, weights, R.MAX_WEIGHT, sets, device=dev), a.reps)
    t_old = timed(lambda: torch_route(ot, tt, wt, goals, a.nodes, 32), a.torch_reps, 1)
    record({"what": "route (gg_roadmap_route): cost-to-go for Q goal sets, uploads included", "nodes": a.nodes,
            "directed_edges": int(len(targets)), "queries": a.queries, "rounds": rounds, "ignored": ignored,
            "reachable_share": round(float((cost < FAR).double().mean()), 4), "routes_agree": same,
            "scipy_agrees": same_cpu, "route": t_new, "spread": spread(t_new), "torch_route": t_old,
            "torch_rounds": t_rounds, "speedup": round(t_old["ms_median"] / t_new["ms_median"], 1),
            "scipy_dijkstra_cpu_ms": round(cpu_ms, 1)})
    assert same and same_cpu

    query = rng.integers(0, a.queries, a.paths).astype(np.int32)
    starts = rng.choice(live, a.paths).astype(np.int32)
    path, length = R.descend_csr(offsets, targets, weights, R.MAX_WEIGHT, cost, query, starts, 64)
    record({"what": "descend (gg_roadmap_descend)", "paths": a.paths, "max_nodes": 64,
            "found": int((length > 0).sum()), "nodes_per_path": [int(length[length > 0].min()),
                                                                 round(float(length[length > 0].double().mean()), 1),
                                                                 int(length.max())],
            "time": timed(lambda: R.descend_csr(offsets, targets, weights, R.MAX_WEIGHT, cost, query, starts, 64),
                          a.reps)})
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch_reps": a.torch_reps,
                       "warmup": WARMUP, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
