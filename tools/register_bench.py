"""GPU time of one gg_icp_step and of one three-scale register.colored_icp at a 300 k-point target and a 30 k-point
source, against scipy's cKDTree plus numpy on the host (step and full run) and a chunked torch restatement of the
step on the same GPU.

    python tools/register_bench.py [--reps 10] [--target 300000] [--source 30000] [--timeout 1100]
                                   [--out profiles/register_bench.json]

The scene: the tests' surface law on a 1 m x 1 m patch, the source moved by the tests' motion.  The step is timed
at the finest scale's setting (max_dist 5 mm, frames at 1 cm) on the full clouds, as the library's own event pair
records it (gg_prof: the sort, the step kernel and the finishing workgroup; the host side of the Python call is not
in it), median and minimum of --reps calls after 2 warm-up calls; `step_resorted` sorts the target in every call,
`step_sorted_once` reuses the sort as colored_icp's loop does.  The full run is wall time, read-backs included.  The
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

GG_K_CLOUD_FRAMES, GG_K_ICP_STEP = 48, 49
MOTION_W, MOTION_T = (0.02, -0.015, 0.03), (0.006, -0.004, 0.003)


def surface(n, seed, half=0.5):
    r = np.random.default_rng(seed)
    xy = r.uniform(-half, half, (n, 2))
    z = 0.02 * np.sin(25 * xy[:, 0]) * np.cos(20 * xy[:, 1]) + 0.01 * np.sin(60 * xy[:, 0] + 1) + r.normal(0, 3e-4, n)
    i = 0.5 + 0.25 * np.sin(40 * xy[:, 0]) + 0.25 * np.cos(35 * xy[:, 1] + 0.5)
    return np.c_[xy, z].astype(np.float32), i.astype(np.float32)


def prof_times(lib, kernel_id, fn, reps, warmup=2):
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
    return round(float(np.median(ts)), 4), round(float(np.min(ts)), 4)


def rows_sums(xp, s, q, n, d, i_s, i_q, dist2, lam):
    """the 32 sums from matched rows; xp is numpy or torch"""
    cross = lambda a, b: xp.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                   a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    wg, wp = lam ** 0.5, (1.0 - lam) ** 0.5
    rg = ((s - q) * n).sum(1)
    ri = i_s - (i_q + (d * ((s - rg[:, None] * n) - q)).sum(1))
    g = -(d - (d * n).sum(1)[:, None] * n)
    J = xp.concatenate([xp.concatenate([wg * cross(s, n), wg * n], 1), xp.concatenate([wp * cross(s, g), wp * g], 1)])
    r = xp.concatenate([wg * rg, wp * ri])
    A, b = J.T @ J, J.T @ r
    iu = np.triu_indices(6)
    return A[iu[0], iu[1]], b, len(s), dist2.sum(), (rg * rg).sum(), (ri * ri).sum()


def host_step(tree, S, Is, P, I, nrm, grad, T, max_dist, lam):
    s = S.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    dist, j = tree.query(s, distance_upper_bound=max_dist, workers=16)
    ok = np.isfinite(dist)
    j = j[ok]
    return rows_sums(np, s[ok], P[j].astype(np.float64), nrm[j].astype(np.float64), grad[j].astype(np.float64),
                     Is[ok].astype(np.float64), I[j].astype(np.float64), dist[ok] ** 2, lam)


def torch_step(S, Is, P, I, nrm, grad, T, max_dist, lam, chunk=1024):
    import torch
    Tt = torch.as_tensor(T, device=S.device)
    s = S.double() @ Tt[:3, :3].T + Tt[:3, 3]
    Pd = P.double()
    best, idx = [], []
    for a in range(0, s.shape[0], chunk):
        d = Pd[None, :, :] - s[a:a + chunk, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        b, j = d2.min(dim=1)
        best.append(b)
        idx.append(j)
    best, j = torch.cat(best), torch.cat(idx)
    ok = best <= max_dist * max_dist
    j = j[ok]
    return rows_sums(torch, s[ok], Pd[j], nrm[j].double(), grad[j].double(), Is[ok].double(), I[j].double(), best[ok],
                     lam)


def host_frames(P, I, radius):
    from scipy.spatial import cKDTree
    P = P.astype(np.float64)
    nb = cKDTree(P).query_ball_point(P, radius, workers=16)
    nrm, grad = np.full((len(P), 3), np.nan), np.zeros((len(P), 3))
    for i, x in enumerate(nb):
        if len(x) < 3:
            continue
        D = P[x] - P[x].mean(0)
        e = np.linalg.eigh(D.T @ D)[1][:, 0]
        nrm[i] = e
        if len(x) >= 4:
            o = [k for k in x if k != i]
            u = P[o] - P[i]
            A = np.vstack([u - np.outer(u @ e, e), (len(x) - 1) * e])
            try:
                grad[i] = np.linalg.solve(A.T @ A, A.T @ np.r_[I[o] - I[i], 0.0])
            except np.linalg.LinAlgError:
                pass
    return nrm, grad


def host_downsample(P, C, v):
    lo = P.min(0) - 0.5 * v
    idx = np.floor((P - lo) / v).astype(np.int64)
    dims = idx.max(0) + 1
    _, inv, cnt = np.unique((idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2], return_inverse=True,
                            return_counts=True)
    return (np.stack([np.bincount(inv, P[:, k]) for k in range(3)], 1) / cnt[:, None],
            np.bincount(inv, C) / cnt)


def host_run(S, Is, P, I, lam, voxels=(0.02, 0.01, 0.005), iters=(30, 20, 10)):
    """the three-scale loop on the host: cKDTree, numpy, np.linalg; (T, iterations)"""
    from scipy.spatial import cKDTree
    from gaussiangrasper_amd.register import solve_step
    T, done = np.eye(4), []
    for v, n_it in zip(voxels, iters):
        s, i_s = host_downsample(S.astype(np.float64), Is.astype(np.float64), v)
        p, i_p = host_downsample(P.astype(np.float64), I.astype(np.float64), v)
        nrm, grad = host_frames(p, i_p, 2 * v)
        keep = np.isfinite(nrm[:, 0])
        p, i_p, nrm, grad = p[keep], i_p[keep], nrm[keep], grad[keep]
        tree = cKDTree(p)
        prev, k = None, 0
        while True:
            u, b, inl, d2, _, _ = host_step(tree, s, i_s, p, i_p, nrm, grad, T, v, lam)
            fit, rmse = inl / len(s), float(np.sqrt(d2 / max(inl, 1)))
            if (prev is not None and abs(prev[0] - fit) < 1e-6 and abs(prev[1] - rmse) < 1e-6) or k == n_it:
                break
            prev = (fit, rmse)
            T, ok = solve_step(np.r_[u, b, inl, d2, 0, 0, 0], T)
            if not ok:
                break
            k += 1
        done.append(k)
    return T, done


def child(a):
    import torch
    from scipy.spatial import cKDTree
    from gaussiangrasper_amd import _lib, register
    from gaussiangrasper_amd.cluster import cluster_grid
    assert torch.cuda.is_available(), "register_bench needs the GPU"
    lib = _lib.load()
    lam = register.LAMBDA_GEOMETRIC
    P, I = surface(a.target, 1)
    S0, Is = surface(a.source, 2)
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = register.rodrigues(MOTION_W), MOTION_T
    Gi = np.linalg.inv(G)
    S = (S0.astype(np.float64) @ Gi[:3, :3].T + Gi[:3, 3]).astype(np.float32)
    dP, dI, dS, dIs = (torch.from_numpy(x).cuda() for x in (P, I, S, Is))
    md, fr = 0.005, 0.01
    grid_f = cluster_grid(dP, fr)
    f_med, f_min = prof_times(lib, GG_K_CLOUD_FRAMES, lambda: register.cloud_frames(dP, dI, fr, grid=grid_f), a.reps)
    tgt = register.cloud_frames(dP, dI, fr, grid=grid_f)
    grid_s = cluster_grid(dP, md, tgt.valid)
    r_med, r_min = prof_times(lib, GG_K_ICP_STEP, lambda: register.icp_step(dS, dIs, tgt, G, md, lam, grid=grid_s),
                              a.reps)
    st = register.StepWorkspace()
    o_med, o_min = prof_times(lib, GG_K_ICP_STEP,
                              lambda: register.icp_step(dS, dIs, tgt, G, md, lam, grid=grid_s, state=st), a.reps)
    gpu = register.icp_step(dS, dIs, tgt, G, md, lam, grid=grid_s)
    nrm, grad = tgt.normals.cpu().numpy(), tgt.gradients.cpu().numpy()
    valid = tgt.valid.cpu().numpy().astype(bool)
    tree = cKDTree(P[valid].astype(np.float64))
    hs = []
    for _ in range(3):
        t0 = time.perf_counter()
        h = host_step(tree, S, Is, P[valid], I[valid], nrm[valid], grad[valid], G, md, lam)
        hs.append((time.perf_counter() - t0) * 1e3)
    vt = tgt.valid.bool()
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = torch_step(dS, dIs, dP[vt], dI[vt], tgt.normals[vt], tgt.gradients[vt], G, md, lam)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    col = lambda x: x[:, None].expand(-1, 3)
    register.colored_icp(dS, col(dIs), dP, col(dI))                       # warm-up
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = register.colored_icp(dS, col(dIs), dP, col(dI))
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    Th, it_h = host_run(S, Is, P, I, lam)
    host_run_s = time.perf_counter() - t0
    err = lambda T: (float(np.linalg.norm((T @ Gi)[:3, :3] - np.eye(3))), float(np.linalg.norm((T - G)[:3, 3])))
    row = {"target": a.target, "source": a.source, "valid_targets": int(valid.sum()), "max_dist": md,
           "frame_radius": fr, "mean_neighbours": round(float(tgt.count.float().mean()), 1),
           "inliers": gpu.inliers, "host_inliers": int(h[2]), "torch_inliers": int(t[2]),
           "frames_ms_median": f_med, "frames_ms_min": f_min,
           "step_resorted_ms_median": r_med, "step_resorted_ms_min": r_min,
           "step_sorted_once_ms_median": o_med, "step_sorted_once_ms_min": o_min,
           "host_step_ms_median": round(float(np.median(hs)), 2), "host_tree_build": "not included",
           "torch_step_ms_median": round(float(np.median(ts)), 2),
           "step_speedup_over_host": round(float(np.median(hs)) / o_med, 1),
           "step_speedup_over_torch": round(float(np.median(ts)) / o_med, 1),
           "run_ms_median": round(float(np.median(runs)), 2), "run_ms_min": round(float(np.min(runs)), 2),
           "run_iterations": res.iterations, "run_status": res.status, "run_fitness": res.fitness,
           "run_error_rot_trans": err(res.transformation),
           "host_run_s": round(host_run_s, 2), "host_run_iterations": it_h, "host_run_error_rot_trans": err(Th),
           "run_speedup_over_host": round(host_run_s * 1e3 / float(np.median(runs)), 1),
           "timing": "frames / step: gg_prof event pair around all launches of one call; run: wall time of "
                     "register.colored_icp with its read-backs; host: cKDTree (16 workers) + numpy"}
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": [row]}, f, indent=1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--target", type=int, default=300_000)
    ap.add_argument("--source", type=int, default=30_000)
    ap.add_argument("--timeout", type=int, default=1100, help="seconds the measuring child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--target", str(a.target),
           "--source", str(a.source)] + (["--out", a.out] if a.out else [])
    try:
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"register_bench: the measuring process exceeded {a.timeout} s and was ended", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
