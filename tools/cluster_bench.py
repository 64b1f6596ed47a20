"""GPU time of one DBSCAN call (gaussiangrasper_amd.cluster.dbscan -> gg_cluster_dbscan) at 100 k, 1 M and 3 M active
points, against sklearn.cluster.DBSCAN on 16 host threads in the same run, with gg_knn (k = 3) at the same N as a
plausibility yardstick: that is one grid sort plus one search, this is one sort plus three searches.

    python tools/cluster_bench.py [--reps 10] [--sizes 100000 1000000 3000000] [--timeout 1100]
                                  [--out profiles/cluster_bench.json]

The cloud: balls of uniform density (about 16 points within eps of each point) plus 5 % uniform speckle, in random
index order.  Device times are per launch sequence as the library's own event pairs record them (gg_prof: one pair
around all launches of a call, so the host side of the Python call is not in them): median and minimum of --reps calls
after 2 warm-up calls, the grid fitted once outside.  The inputs (12 bytes a point) and the workspace (about 45 bytes
a point) stay in the Infinity Cache between repetitions up to about 4 M points.  sklearn runs once per size.  The
measurement runs in one child process under its own time limit."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GG_K_KNN, GG_K_CLUSTER, GG_K_CLUSTER_STATS = 38, 46, 47
NEIGHBOURS, MIN_POINTS, PER_BALL, BALL_RADIUS, SPECKLE = 16, 8, 5000, 0.05, 0.05


def make_cloud(n, seed):
    """(points float32 (n, 3), eps): balls of PER_BALL points of uniform density, NEIGHBOURS per eps-ball"""
    rng = np.random.default_rng(seed)
    ns = int(SPECKLE * n)
    balls = max(1, (n - ns) // PER_BALL)
    side = 0.25 * balls ** (1.0 / 3.0) + 2 * BALL_RADIUS            # room for the balls at a fifth of the volume
    centres = rng.uniform(BALL_RADIUS, side - BALL_RADIUS, size=(balls, 3))
    which = rng.integers(0, balls, n - ns)
    d = rng.normal(size=(n - ns, 3))
    d *= (BALL_RADIUS * rng.random(n - ns) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    p = np.concatenate([centres[which] + d, rng.uniform(0.0, side, size=(ns, 3))])
    eps = BALL_RADIUS * (NEIGHBOURS / ((n - ns) / balls)) ** (1.0 / 3.0)
    return p[rng.permutation(n)].astype(np.float32), float(eps)


def prof_times(lib, kernel_id, fn, reps, warmup=2):
    """median / min ms of `reps` calls of fn as gg_prof's event pair of kernel_id records each"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    prev = lib.gg_prof_enable(1)
    try:
        for _ in range(reps):
            lib.gg_prof_reset()
            fn()
            torch.cuda.synchronize()
            launches, ms = ctypes.c_int(0), ctypes.c_double(0.0)
            lib.gg_prof_get(kernel_id, ctypes.byref(launches), ctypes.byref(ms))
            assert launches.value == 1, launches.value
            ts.append(ms.value)
    finally:
        lib.gg_prof_reset()
        lib.gg_prof_enable(prev)
    return float(np.median(ts)), float(np.min(ts))


def child(a):
    import torch
    from sklearn.cluster import DBSCAN
    from gaussiangrasper_amd import _lib, cluster
    from gaussiangrasper_amd.prepare import knn_distances
    assert torch.cuda.is_available(), "cluster_bench needs the GPU"
    lib = _lib.load()
    rows = []
    for n in a.sizes:
        p_host, eps = make_cloud(n, seed=n)
        p = torch.from_numpy(p_host).cuda()
        w = torch.ones(n, device="cuda")
        grid = cluster.cluster_grid(p, eps)
        cl = cluster.dbscan(p, eps, MIN_POINTS, grid=grid)
        d_med, d_min = prof_times(lib, GG_K_CLUSTER, lambda: cluster.dbscan(p, eps, MIN_POINTS, grid=grid), a.reps)
        s_med, s_min = prof_times(lib, GG_K_CLUSTER_STATS, lambda: cluster.cluster_stats(p, w, cl), a.reps)
        k_med, k_min = prof_times(lib, GG_K_KNN, lambda: knn_distances(p, 3), a.reps)
        t0 = time.perf_counter()
        sk = DBSCAN(eps=eps, min_samples=MIN_POINTS, n_jobs=16).fit(p_host.astype(np.float64))
        sk_s = time.perf_counter() - t0
        labels = cl.labels.cpu().numpy()
        row = {"N": n, "eps": eps, "min_points": MIN_POINTS, "grid_dims": [int(x) for x in grid[1]],
               "grid_cell": float(grid[0][3]), "num_clusters": cl.num_clusters,
               "mean_neighbor_count": round(float(cl.neighbor_count.float().mean()), 2),
               "core_points": int(cl.core.sum()), "noise_points": int((labels < 0).sum()),
               "dbscan_ms_median": round(d_med, 4), "dbscan_ms_min": round(d_min, 4),
               "stats_ms_median": round(s_med, 4), "stats_ms_min": round(s_min, 4),
               "knn3_ms_median": round(k_med, 4), "knn3_ms_min": round(k_min, 4),
               "dbscan_over_knn3": round(d_med / k_med, 2),
               "sklearn_16_threads_s": round(sk_s, 2), "speedup_over_sklearn": round(sk_s * 1e3 / d_med, 1),
               "labels_differing_from_sklearn": int((labels != sk.labels_).sum()),
               "timing": "gg_prof event pair around all launches of one call; inputs and workspace "
                         "Infinity-Cache resident across repetitions below about 4 M points"}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del p, w, cl
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}, f, indent=1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000, 3_000_000])
    ap.add_argument("--timeout", type=int, default=1100, help="seconds the measuring child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--sizes",
           *[str(s) for s in a.sizes]] + (["--out", a.out] if a.out else [])
    try:
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"cluster_bench: the measuring process exceeded {a.timeout} s and was ended", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
