"""Time of one plane-consensus call (gaussiangrasper_amd.support.consensus -> gg_plane_consensus) and of one whole
support.fit_plane (hypotheses, consensus, two refits, closing classify, every read-back included) at 1 M points x 1024
hypotheses and at 5 M x 4096, against
  * a torch restatement of the consensus on the same GPU: fp64, the contract's operation order, the hypotheses in
    chunks so that a chunk's (hypotheses x points) temporaries stay under 512 MiB each;
  * the numpy restatement on one core, timed over --numpy-hypotheses hypotheses and scaled to all of them (recorded as
    an extrapolation: the loop is one hypothesis after the other, so its time is proportional to their number).

    python tools/support_plane_bench.py [--reps 10] [--torch-reps 3] [--out profiles/support_plane_bench.json]

Scene: a noisy tilted table (55 % of the points), a box on it, a wall and uniform clutter, the proportions of the
tests' table scene.  Wall-clock times around a device synchronisation, after 3 warm-up calls; median, minimum and
maximum of --reps calls.  With --kernels, gg_prof's device time of the launches is recorded too (a separate set of
calls).  Each row records whether the routes agree on every count."""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussiangrasper_amd import support  # noqa: E402

DIST, MIN_SIN2 = 0.004, support.MIN_SIN2
UP, MAX_TILT = (0.0, 0.0, 1.0), math.radians(20.0)
NORMAL = np.array([0.05, -0.03, 1.0]) / math.sqrt(0.05 ** 2 + 0.03 ** 2 + 1.0)


def make_scene(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    nt, nb, nw = int(0.55 * n), int(0.2 * n), int(0.15 * n)
    xy = rng.uniform(-0.4, 0.4, (nt, 2))
    z = (0.2 - NORMAL[0] * xy[:, 0] - NORMAL[1] * xy[:, 1]) / NORMAL[2]
    table = np.column_stack([xy, z]) + rng.normal(0.0, 0.001, (nt, 1)) * NORMAL
    box = np.column_stack([rng.uniform(-0.04, 0.04, nb), rng.uniform(-0.03, 0.03, nb), rng.uniform(0.2, 0.25, nb)])
    wall = np.column_stack([np.full(nw, 0.4), rng.uniform(-0.4, 0.4, nw), rng.uniform(0.15, 0.6, nw)])
    nc = n - nt - nb - nw
    clutter = np.column_stack([rng.uniform(-0.4, 0.4, (nc, 2)), rng.uniform(0.05, 0.6, nc)])
    return np.concatenate([table, box, wall, clutter]).astype(np.float32)


def numpy_counts(p32: np.ndarray, hyp: np.ndarray) -> np.ndarray:
    p = p32.astype(np.float64)
    cos2, dd = math.cos(MAX_TILT) ** 2, DIST * DIST
    out = np.zeros(len(hyp), np.int32)
    for h, (a, b, c) in enumerate(hyp):
        if a == b or a == c or b == c:
            continue
        e1, e2 = p[b] - p[a], p[c] - p[a]
        n0 = e1[1] * e2[2] - e1[2] * e2[1]
        n1 = e1[2] * e2[0] - e1[0] * e2[2]
        n2 = e1[0] * e2[1] - e1[1] * e2[0]
        nn = (n0 * n0 + n1 * n1) + n2 * n2
        if not nn > MIN_SIN2 * (float(e1 @ e1) * float(e2 @ e2)) or not n2 * n2 >= cos2 * nn:
            continue
        d = p - p[a]
        s = (n0 * d[:, 0] + n1 * d[:, 1]) + n2 * d[:, 2]
        out[h] = int((s * s <= dd * nn).sum())
    return out


@torch.no_grad()
def torch_counts(pts: torch.Tensor, hyp: torch.Tensor) -> torch.Tensor:
    p = pts.double()
    n = p.shape[0]
    chunk = max(1, (1 << 26) // n)
    cos2, dd = math.cos(MAX_TILT) ** 2, DIST * DIST
    a, b, c = (p[hyp[:, k].long()] for k in range(3))
    e1, e2 = b - a, c - a
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    nn = (nx * nx + ny * ny) + nz * nz
    ee = ((e1 * e1)[:, 0] + (e1 * e1)[:, 1] + (e1 * e1)[:, 2]) * ((e2 * e2)[:, 0] + (e2 * e2)[:, 1] + (e2 * e2)[:, 2])
    distinct = (hyp[:, 0] != hyp[:, 1]) & (hyp[:, 0] != hyp[:, 2]) & (hyp[:, 1] != hyp[:, 2])
    valid = distinct & (nn > MIN_SIN2 * ee) & (nz * nz >= cos2 * nn)
    out = torch.zeros(hyp.shape[0], dtype=torch.int32, device=pts.device)
    for s0 in range(0, hyp.shape[0], chunk):
        sl = slice(s0, s0 + chunk)
        s = nx[sl, None] * (p[None, :, 0] - a[sl, None, 0])
        s += ny[sl, None] * (p[None, :, 1] - a[sl, None, 1])
        s += nz[sl, None] * (p[None, :, 2] - a[sl, None, 2])
        out[sl] = ((s * s <= (dd * nn[sl])[:, None]).sum(dim=1) * valid[sl]).int()
    return out


def wall_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(ts)), 4), "min": round(float(np.min(ts)), 4),
            "max": round(float(np.max(ts)), 4), "reps": reps}


def kernel_ms(fn, reps):
    """gg_prof's device time of the support-plane launches, per call of fn"""
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    lib.gg_prof_enable(1)
    lib.gg_prof_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    n, ms = ctypes.c_int(0), ctypes.c_double(0.0)
    lib.gg_prof_get(52, ctypes.byref(n), ctypes.byref(ms))
    lib.gg_prof_enable(0)
    return round(ms.value / max(reps, 1), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--numpy-hypotheses", type=int, default=16)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "support_plane_bench needs the GPU"
    rows = []
    for n, h in ((1_000_000, 1024), (5_000_000, 4096)):
        p_np = make_scene(n, seed=n)
        pts = torch.from_numpy(p_np).cuda()
        hyp_np = support.draw_hypotheses(n, h, 0)
        hyp = torch.from_numpy(hyp_np).cuda()

        def one_consensus():
            return support.consensus(pts, None, hyp, DIST, 0.0, MIN_SIN2, UP, MAX_TILT)

        def one_fit():
            return support.fit_plane(pts, None, DIST, h, UP, MAX_TILT)
        count = one_consensus()[0]
        fit = one_fit()
        t_count = torch_counts(pts, hyp)
        row = {"points": n, "hypotheses": h, "best_count": int(count.max()),
               "fit_angle_deg": round(math.degrees(math.acos(min(1.0, float(fit.normal @ NORMAL)))), 5),
               "fit_on_above_below": [fit.count_on, fit.count_above, fit.count_below],
               "consensus_ms": wall_ms(one_consensus, a.reps), "fit_plane_ms": wall_ms(one_fit, a.reps),
               "torch_consensus_ms": wall_ms(lambda: torch_counts(pts, hyp), a.torch_reps, 1),
               "torch_agrees": bool(torch.equal(count, t_count))}
        if a.kernels:
            row["consensus_kernels_ms"] = kernel_ms(one_consensus, a.reps)
            row["fit_plane_kernels_ms"] = kernel_ms(one_fit, a.reps)
        if not a.skip_numpy:
            k = min(a.numpy_hypotheses, h)
            first = np.nonzero(count.cpu().numpy() > 0)[0][:k]          # valid ones: an invalid one costs nothing
            t0 = time.perf_counter()
            n_count = numpy_counts(p_np, hyp_np[first])
            dt = (time.perf_counter() - t0) * 1e3
            valid = int((count > 0).sum())
            row["numpy_one_core_ms_extrapolated"] = round(dt / max(len(first), 1) * valid, 1)
            row["numpy_timed_hypotheses"] = int(len(first))
            row["numpy_agrees"] = bool(np.array_equal(count.cpu().numpy()[first], n_count))
        row["speedup_over_torch_median"] = round(row["torch_consensus_ms"]["median"] / row["consensus_ms"]["median"], 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pts, hyp, count, t_count, fit
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "dist": DIST, "min_sin2": MIN_SIN2,
                       "max_tilt_deg": 20.0, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
