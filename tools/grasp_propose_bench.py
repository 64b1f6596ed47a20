"""GPU time of one grasp-proposal call (gaussiangrasper_amd.grasp_propose.antipodal -> gg_grasp_propose) against a
chunked torch fp64 restatement of the same search on the same GPU, at two shapes:

    100 k points x 4096 seeds     a selected object only (a sphere of radius 4 cm, radial normals)
    1 M points x 16384 seeds      the same object among 900 k points of a table-top scene, no mask

    python tools/grasp_propose_bench.py [--reps 20] [--torch-reps 3] [--timeout 900] [--out profiles/grasp_propose_bench.json]

The measurement runs in one child process under its own time limit; the parent only starts it and passes its output
on.  Median and minimum of --reps hipEvent timings after 3 warm-up calls; the inputs (28 bytes a point) stay in the
Infinity Cache between repetitions.  The torch route forms fp64 offsets for a chunk of seeds at a time (at most 16 M
seed-point pairs, 384 MB per chunk), so it is timed with one warm-up call and fewer repetitions.  Each row records how
many seeds the two routes disagree on (contacts, counts, validity): ties in torch's min / max may pick another index,
so a few are expected at most."""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, W, W0, C = 0.003, 0.10, 0.005, 0.005


def make_points(n, n_obj, seed):
    import torch
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_obj, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m = n - n_obj
    p = np.concatenate([0.04 * d, rng.uniform([-0.5, -0.5, -0.1], [0.5, 0.5, 0.3], size=(m, 3))])
    nr = np.concatenate([d, rng.normal(size=(m, 3))])
    perm = rng.permutation(n)                     # Gaussians come in no spatial order
    w = rng.uniform(0.0, 1.0, size=n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    return t(p[perm]), t(nr[perm]), t(w)


def torch_route(p, nr, w, seeds, pairs=1 << 24):
    """The search and the validity test in torch ops, fp64, seeds in chunks of at most `pairs` seed-point pairs."""
    import torch
    with torch.no_grad():
        n = p.shape[0]
        p64, n64 = p.double(), nr.double()
        part = torch.isfinite(p).all(1) & torch.isfinite(nr).all(1) & (w.double() > 0.0)
        sd = seeds.long()
        out = {k: [] for k in ("pair_idx", "tube_count", "valid")}
        step = max(1, pairs // max(n, 1))
        wc = W - 2.0 * C
        for s0 in range(0, sd.shape[0], step):
            i = sd[s0:s0 + step]
            ps, ns = p64[i], n64[i]
            nn = (ns * ns).sum(1)
            d = p64[None] - ps[:, None]                                          # (s, n, 3)
            s = torch.matmul(d, ns[:, :, None])[..., 0]
            dd = (d * d).sum(-1)
            ss = s * s
            tube = part[None] & (dd * nn[:, None] - ss <= (R * R) * nn[:, None]) & (ss <= (W * W) * nn[:, None])
            slo, jlo = torch.where(tube, s, math.inf).min(1)
            shi, jhi = torch.where(tube, s, -math.inf).max(1)
            q = shi - slo
            usable = part[i] & (nn > 0)
            mlo, mhi = (n64[jlo] * n64[jlo]).sum(1), (n64[jhi] * n64[jhi]).sum(1)
            ok = usable & (q * q >= (W0 * W0) * nn) & (q * q <= (wc * wc) * nn) & (mlo > 0) & (mhi > 0)
            out["pair_idx"].append(torch.where(usable[:, None], torch.stack([jlo, jhi], 1), -1))
            out["tube_count"].append(torch.where(usable, tube.sum(1), 0))
            out["valid"].append(ok)
        return {k: torch.cat(v) for k, v in out.items()}


def median_ms(fn, reps, warmup=3):
    import torch
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
    return float(np.median(ts)), float(np.min(ts))


def child(a):
    import torch
    from gaussiangrasper_amd.grasp import contacts
    from gaussiangrasper_amd.grasp_propose import antipodal
    assert torch.cuda.is_available(), "grasp_propose_bench needs the GPU"
    rows = []
    for name, n, s in (("object", 100_000, 4096), ("scene", 1_000_000, 16384)):
        p, nr, w = make_points(n, 100_000, seed=n)
        # exactly s seeds, ascending (choose_seeds would thin to a divisor of the point count)
        pick = np.sort(np.random.default_rng(s).choice(n, size=s, replace=False))
        seeds = torch.from_numpy(pick.astype(np.int32)).cuda()
        kw = dict(tube_radius=R, max_width=W, min_width=W0, clearance=C)
        fused = antipodal(p, nr, w, seeds, **kw)
        ref = torch_route(p, nr, w, seeds)
        torch.cuda.synchronize()
        mism = int(((fused.pair_idx != ref["pair_idx"]).any(1) | (fused.tube_count != ref["tube_count"])
                    | (fused.valid != ref["valid"])).sum())
        f_med, f_min = median_ms(lambda: antipodal(p, nr, w, seeds, **kw), a.reps)
        t_med, t_min = median_ms(lambda: torch_route(p, nr, w, seeds), a.torch_reps, warmup=1)
        row = {"shape": name, "N": n, "S": int(seeds.shape[0]), "K": 8, "fused_ms_median": round(f_med, 4),
               "fused_ms_min": round(f_min, 4), "torch_ms_median": round(t_med, 3), "torch_ms_min": round(t_min, 3),
               "speedup_median": round(t_med / f_med, 1),
               "pair_tests_per_s": f"{n * int(seeds.shape[0]) / (f_med * 1e-3):.3e}",
               "valid_seeds": int(fused.valid.sum()),
               "mean_tube_count": round(float(fused.tube_count.float().mean()), 1),
               "seeds_differing_from_torch": mism,
               "residency": "inputs Infinity-Cache resident across repetitions (28 B/point), not L2"}
        if name == "object":           # the share of a whole grasp_object call: the filter on the proposed rows
            cand = fused.compact()
            c_med, _ = median_ms(lambda: contacts(p, nr, w, cand), a.reps)
            row.update(proposed_rows=int(cand.shape[0]), contacts_ms_median=round(c_med, 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del p, nr, w, seeds, fused, ref
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch_reps": a.torch_reps,
                       "rows": rows}, f, indent=1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds the measuring child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--torch-reps",
           str(a.torch_reps)] + (["--out", a.out] if a.out else [])
    try:
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"grasp_propose_bench: the measuring process exceeded {a.timeout} s and was ended", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
