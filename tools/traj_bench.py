"""GPU time of the arm trajectory kernels (gaussiangrasper_amd.trajectory) on the default arm's limits: gg_traj_time for
4096 and 65 536 random paths of 2, 4 and 8 waypoints at m = 16 with every corner blended by 1/4, and gg_traj_sample
at 1 kHz.  The baselines compute the same law for the same paths:

    torch    batched over the paths on the same GPU, one group of launches per grid step (the geometry of the grid is
             prepared beforehand and not timed); its x and duration must agree with the kernel's to 1e-9
    numpy    the restatement of tests/trajectory_ref.py on the host, for the first 64 paths

    python tools/traj_bench.py [--reps 10] [--out profiles/traj_bench.json]

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gaussiangrasper_amd import arm as A, trajectory as T  # noqa: E402
from route_bench import WARMUP, timed  # noqa: E402

STEPS = 16
FRACTION = 0.25
INF = float("inf")


def random_paths(P, n, seed):
    """P zigzags of n waypoints inside the default arm's limits"""
    arm = A.default_arm()
    lo, hi = np.asarray(arm.lo), np.asarray(arm.hi)
    return np.random.default_rng(seed).uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), size=(P, n, len(lo)))


def uniform_grid(way, f, m):
    """The grid of paths that all have the same pieces (every interior fraction f > 0, f < 1/2): qp0, qp1, qpp
    (G, P, J), delta (G,), stop (G + 1,), the header's formulas"""
    P, n, J = way.shape
    tau = (np.arange(m) / m)[:, None, None]
    tau1 = (np.arange(1, m + 1) / m)[:, None, None]
    qp0, qp1, qpp, delta, stop = [], [], [], [], []
    for k in range(n - 1):
        fk = f if k >= 1 else 0.0
        fn = f if k + 1 <= n - 2 else 0.0
        d = way[:, k + 1] - way[:, k]
        if k >= 1:
            dm = way[:, k] - way[:, k - 1]
            e = d - dm
            qp0.append(dm + tau * e)
            end = dm + tau1 * e
            end[m - 1] = d
            qp1.append(end)
            qpp.append(np.broadcast_to(e / (2.0 * fk), (m, P, J)))
            delta.append(np.full(m, 2.0 * fk / m))
            stop.append(np.zeros(m, bool))
        L = (1.0 - fk) - fn
        qp0.append(np.broadcast_to(d, (m, P, J)))
        qp1.append(np.broadcast_to(d, (m, P, J)))
        qpp.append(np.zeros((m, P, J)))
        delta.append(np.full(m, L / m))
        stop.append(np.concatenate([[k == 0], np.zeros(m - 1, bool)]))
    return (np.concatenate(qp0), np.concatenate(qp1), np.concatenate(qpp), np.concatenate(delta),
            np.concatenate(stop + [[True]]))


def torch_law(qp0, qp1, qpp, delta, stop, v, a):
    """(x (G + 1, P), duration (P,)): the law of include/gg_raster.h batched over the paths, a loop over the grid"""
    G, P, J = qp0.shape
    dev = qp0.device
    a2 = a.repeat_interleave(2)

    def rows(i, nxt):
        two = 2.0 * delta[i]
        mx = torch.maximum(qp0[i].abs(), qp1[i].abs())
        r = v / mx
        vc = torch.where(mx > 0, r * r, torch.full_like(r, INF)).amin(1)
        nxt = torch.minimum(nxt, vc)
        B = torch.stack([qp0[i], two * qpp[i] + qp1[i]], 2).reshape(P, 2 * J)
        Aq = qpp[i].repeat_interleave(2, dim=1)
        nz = B != 0
        c = a2 / B.abs()
        cu = torch.where(nz, c, torch.full_like(c, INF))
        d = torch.where(nz, -(Aq / B), torch.zeros_like(c))
        cap = torch.where(~nz & (Aq != 0), a2 / Aq.abs(), torch.full_like(c, INF)).amin(1)
        one = torch.ones(P, 1, dtype=torch.float64, device=dev)
        cu = torch.cat([cu, (nxt / two)[:, None]], 1)
        cl = torch.cat([-torch.where(nz, c, torch.full_like(c, INF)), 0.0 * one], 1)
        d = torch.cat([d, -(1.0 / two) * one], 1)
        return cu, cl, d, torch.minimum(cap, vc), nxt, two

    xbar = torch.zeros(G + 1, P, dtype=torch.float64, device=dev)
    for i in range(G - 1, -1, -1):
        cu, cl, d, cap, _, _ = rows(i, xbar[i + 1])
        dd = d[:, :, None] - d[:, None, :]
        val = torch.where(dd > 0, (cu[:, None, :] - cl[:, :, None]) / dd, torch.full_like(dd, INF))
        xbar[i] = 0.0 if stop[i] else torch.minimum(val.amin((1, 2)), cap).clamp(min=0.0)
    x = torch.zeros(G + 1, P, dtype=torch.float64, device=dev)
    t = torch.zeros(P, dtype=torch.float64, device=dev)
    for i in range(G):
        cu, cl, d, _, bound, two = rows(i, xbar[i + 1])
        u = (cu + d * x[i][:, None]).amin(1)
        x[i + 1] = torch.minimum((x[i] + two * u).clamp(min=0.0), bound)
        t = t + two / (x[i].sqrt() + x[i + 1].sqrt())
    return x, t


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("traj_bench measures on a HIP device; none is available")
    import trajectory_ref as ref
    dev = torch.device("cuda")
    lim = T.default_limits()
    v, acc = torch.as_tensor(lim.v_max, device=dev), torch.as_tensor(lim.a_max, device=dev)
    rows = []
    for P in (4096, 65536):
        for n in (2, 4, 8):
            way = random_paths(P, n, 100 + n)
            blend = np.full((P, n), FRACTION)
            wt, lt, bt = (torch.as_tensor(way, device=dev), torch.full((P,), n, dtype=torch.int32, device=dev),
                          torch.as_tensor(blend, device=dev))
            law = T.time_paths(wt, lt, bt, lim, STEPS)
            G = int(law.count[0])
            own = timed(lambda: T.time_paths(wt, lt, bt, lim, STEPS), a.reps)
            bare = timed(lambda: T.time_paths(wt, lt, bt, lim, STEPS, q_grid=False), a.reps)
            geo = [torch.as_tensor(np.ascontiguousarray(g), device=dev) for g in uniform_grid(way, FRACTION, STEPS)[:3]]
            _, _, _, delta, stop = uniform_grid(way[:1], FRACTION, STEPS)
            x, dur = torch_law(*geo, delta.tolist(), stop.tolist(), v, acc)
            err_x = float((x.T - law.x[:, :G + 1]).abs().max() / law.x[:, :G + 1].abs().max())
            err_t = float(((dur - law.duration).abs() / law.duration).max())
            base = timed(lambda: torch_law(*geo, delta.tolist(), stop.tolist(), v, acc), a.torch_reps, warmup=1)
            t0 = time.perf_counter()
            host = ref.time_law(way[:64], [n] * 64, blend[:64], lim.v_max, lim.a_max, STEPS)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(host["x"], law.x[:64].cpu().numpy(), equal_nan=True)
            dt = 1e-3
            K = int(np.ceil(float(law.duration.max()) / dt)) + 2
            fits = P * K <= T.MAX_POSES
            smp = timed(lambda: T.sample(law, dt, K), a.reps) if fits else None
            row = {"what": "gg_traj_time, a wave per path", "paths": P, "waypoints": n, "steps": STEPS,
                   "fraction": FRACTION, "intervals": G, "time": own, "time_without_q_grid": bare,
                   "spread": round((own["ms_max"] - own["ms_min"]) / own["ms_median"], 3),
                   "torch_batched": base, "speedup_over_torch": round(base["ms_median"] / own["ms_median"], 1),
                   "torch_x_rel_err": err_x, "torch_duration_rel_err": err_t, "agree_1e-9": err_x <= 1e-9 and err_t <= 1e-9,
                   "numpy_64_paths_ms": round(host_ms, 2), "numpy_equals_kernel_bits": True,
                   "duration_s_median": round(float(law.duration.median()), 4),
                   "sample_1khz": smp, "samples_per_path": K if fits else None}
            rows.append(row)
            print(json.dumps(row))
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch_reps": a.torch_reps, "warmup": WARMUP,
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
