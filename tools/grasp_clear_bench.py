"""GPU time of one gripper-clearance call (gaussiangrasper_amd.grasp.clearance -> gg_grasp_clearance) with the default
gripper and a 5 cm approach, against a chunked torch fp64 restatement of the same contract on the same GPU, and beside
gg_grasp_contacts on the same points and rows (the yardstick DESIGN.md §3.20 names), at two shapes:

    1 M points x 1024 grasps
    1 M points x 8192 grasps

    python tools/grasp_clear_bench.py [--reps 20] [--torch-reps 3] [--out profiles/grasp_clear_bench.json]

Scene, grasps and timing are those of tools/grasp_bench.py (its make_points, make_grasps and median_ms): an object of
50 k points on a sphere on a table of uniform points, grasps centred on object points; median and minimum of --reps
CUDA-event timings after 3 warm-up calls, the inputs resident in the Infinity Cache between repetitions.  Each row
records how many grasps the two routes disagree on (any count, or clear)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grasp_bench import make_grasps, make_points, median_ms  # noqa: E402

from gaussiangrasper_amd.grasp import clearance, contacts, default_gripper  # noqa: E402

APPROACH, MAX_BODY, MAX_SWEEP = 0.05, 0.5, 0.5


@torch.no_grad()
def torch_route(p, w, g, parts, approach=APPROACH, max_body=MAX_BODY, max_sweep=MAX_SWEEP, pairs=1 << 24):
    """The contract in torch ops, fp64, grasps in chunks of at most `pairs` point-grasp pairs."""
    n, m = p.shape[0], g.shape[0]
    p64, w64 = p.double(), w.double()
    part = torch.isfinite(p).all(1) & (w64 > 0.0)
    G = g.double()
    c = torch.as_tensor(parts, dtype=torch.float64, device=p.device)                    # (P, 6, 4)
    out = {k: [] for k in ("body_count", "sweep_count", "clear")}
    step = max(1, pairs // max(n, 1))
    for s in range(0, m, step):
        gc = G[s:s + step]
        R, t = gc[:, 4:13].reshape(-1, 3, 3), gc[:, 13:16]
        u = torch.matmul(p64[None] - t[:, None], R)                                     # (g, n, 3)
        wd, h, d = (gc[:, k][:, None, None] for k in (1, 2, 3))
        B = ((c[None, :, :, 0] + c[None, :, :, 1] * wd) + c[None, :, :, 2] * d) + c[None, :, :, 3] * h   # (g, P, 6)
        ok = torch.isfinite(gc).all(1) & (gc[:, 1] > 0) & (gc[:, 2] > 0)
        bc, sc, tb, ts = [], [], 0.0, 0.0
        for k in range(c.shape[0]):
            b = B[:, k, :, None]                                                        # (g, 6, 1)
            full = ok & torch.isfinite(B[:, k]).all(1) & (B[:, k, 0::2] <= B[:, k, 1::2]).all(1)
            yz = (part[None] & full[:, None] & (u[..., 1] >= b[:, 2]) & (u[..., 1] <= b[:, 3]) &
                  (u[..., 2] >= b[:, 4]) & (u[..., 2] <= b[:, 5]))
            body = yz & (u[..., 0] >= b[:, 0]) & (u[..., 0] <= b[:, 1])
            sweep = yz & (u[..., 0] >= b[:, 0] - approach) & (u[..., 0] < b[:, 0])
            bc.append(body.sum(1))
            sc.append(sweep.sum(1))
            tb = tb + torch.where(body, w64[None], 0.0).sum(1)
            ts = ts + torch.where(sweep, w64[None], 0.0).sum(1)
        out["body_count"].append(torch.stack(bc, 1))
        out["sweep_count"].append(torch.stack(sc, 1))
        out["clear"].append(ok & (tb <= max_body) & (ts <= max_sweep))
    return {k: torch.cat(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "grasp_clear_bench needs the GPU"
    parts = default_gripper()
    kw = dict(approach=APPROACH, max_body=MAX_BODY, max_sweep=MAX_SWEEP)
    rows = []
    for n, m in ((1_000_000, 1024), (1_000_000, 8192)):
        p, nr, w, obj_p, obj_n = make_points(n, 50_000, seed=n)
        g = make_grasps(m, obj_p, obj_n, seed=m)
        fused = clearance(p, w, g, parts, **kw)
        ref = torch_route(p, w, g, parts)
        torch.cuda.synchronize()
        mism = int(((fused.body_count != ref["body_count"]).any(1) | (fused.sweep_count != ref["sweep_count"]).any(1)
                    | (fused.clear != ref["clear"])).sum())
        f_med, f_min = median_ms(lambda: clearance(p, w, g, parts, **kw), a.reps)
        c_med, c_min = median_ms(lambda: contacts(p, nr, w, g), a.reps)
        t_med, t_min = median_ms(lambda: torch_route(p, w, g, parts), a.torch_reps, warmup=1)
        row = {"N": n, "M": m, "parts": int(parts.shape[0]), "approach": APPROACH,
               "fused_ms_median": round(f_med, 4), "fused_ms_min": round(f_min, 4),
               "contacts_ms_median": round(c_med, 4), "contacts_ms_min": round(c_min, 4),
               "torch_ms_median": round(t_med, 3), "torch_ms_min": round(t_min, 3),
               "speedup_median": round(t_med / f_med, 1), "pair_tests_per_s": f"{n * m / (f_med * 1e-3):.3e}",
               "grasps_with_body_points": int((fused.body_count.sum(1) > 0).sum()),
               "grasps_with_sweep_points": int((fused.sweep_count.sum(1) > 0).sum()),
               "clear": int(fused.clear.sum()), "grasps_differing_from_torch": mism,
               "residency": "inputs Infinity-Cache resident across repetitions (16 B/point), not L2"}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del p, nr, w, g, fused, ref
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
