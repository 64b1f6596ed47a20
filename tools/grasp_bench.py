"""GPU time of one grasp-filtering call (gaussiangrasper_amd.grasp.contacts -> gg_grasp_contacts) against a chunked
torch restatement of the same contract, at three shapes:

    1 M points x 1024 grasps   the whole scene, no mask
    50 k points x 1024 grasps  a selected object only
    5 M points x 256 grasps    a large scene

    python tools/grasp_bench.py [--reps 20] [--torch-reps 3] [--out profiles/grasp_bench.json]

Scene: an object of 50 k points on a sphere of radius 0.05 m at the origin (radial normals) on a table of uniform
points in [-0.5, 0.5]^2 x [-0.1, 0.3] (random normals); weights uniform in (0, 1).  Grasps: centred on object points,
pushed out along the normal by up to 1 cm, random rotations, width 2-8 cm, height 2 cm, depth 2 cm.  Median and
minimum of --reps CUDA-event timings after 3 warm-up calls; the inputs (28 bytes a point: 28 MB at 1 M, 140 MB at 5 M)
stay in the 256 MiB Infinity Cache between repetitions and are read from there, not from L2 (4 MiB per XCD).  The
torch route forms fp64 local coordinates for a chunk of grasps at a time (at most 16 M point-grasp pairs, 384 MB per
chunk), so it is timed with the same warm-up, fewer repetitions.  Each row records how many grasps the two routes
disagree on (contacts, counts, feasibility): ties in torch's min / max may pick another index, so a few are expected
at most."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiangrasper_amd.grasp import BAND, DEPTH_BASE, FINGER_WIDTH, MU, contacts  # noqa: E402


def make_points(n, n_obj, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_obj, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    obj_p, obj_n = 0.05 * d, d
    m = n - n_obj
    bg_p = rng.uniform([-0.5, -0.5, -0.1], [0.5, 0.5, 0.3], size=(m, 3))
    bg_n = rng.normal(size=(m, 3))
    p = np.concatenate([obj_p, bg_p])
    nr = np.concatenate([obj_n, bg_n])
    perm = rng.permutation(n)                     # Gaussians come in no spatial order
    w = rng.uniform(0.0, 1.0, size=n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    return t(p[perm]), t(nr[perm]), t(w), obj_p, obj_n


def make_grasps(m, obj_p, obj_n, seed):
    rng = np.random.default_rng(seed)
    k = rng.choice(len(obj_p), size=m)
    c = obj_p[k] + obj_n[k] * rng.uniform(0.0, 0.01, size=(m, 1))
    q, r = np.linalg.qr(rng.normal(size=(m, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[np.linalg.det(q) < 0, :, 0] *= -1
    g = np.zeros((m, 17))
    g[:, 0] = rng.random(m)
    g[:, 1], g[:, 2], g[:, 3] = rng.uniform(0.02, 0.08, m), 0.02, 0.02
    g[:, 4:13] = q.reshape(m, 9)
    g[:, 13:16] = c
    return torch.from_numpy(g.astype(np.float32)).cuda()


@torch.no_grad()
def torch_route(p, nr, w, g, db=DEPTH_BASE, fw=FINGER_WIDTH, band=BAND, mu=MU, pairs=1 << 24):
    """The contract in torch ops, fp64, grasps in chunks of at most `pairs` point-grasp pairs."""
    n, m = p.shape[0], g.shape[0]
    p64, n64, w64 = p.double(), nr.double(), w.double()
    part = torch.isfinite(p).all(1) & torch.isfinite(nr).all(1) & (w64 > 0.0)
    G = g.double()
    out = {k: [] for k in ("contact_idx", "region_count", "feasible")}
    step = max(1, pairs // max(n, 1))
    lim = math.atan(mu)
    for s in range(0, m, step):
        gc = G[s:s + step]
        R, t = gc[:, 4:13].reshape(-1, 3, 3), gc[:, 13:16]
        u = torch.matmul(p64[None] - t[:, None], R)                          # (g, n, 3): u_j = sum_k d_k R[k][j]
        hw, hh, depth = 0.5 * gc[:, 1:2], 0.5 * gc[:, 2:3], gc[:, 3:4]
        u0, u1, u2 = u[..., 0], u[..., 1], u[..., 2]
        common = part[None] & (u0 >= -db) & (u0 <= depth) & (u2.abs() <= hh)
        reg = common & (u1.abs() <= hw)
        fing = common & (((u1 >= -hw - fw) & (u1 < -hw)) | ((u1 > hw) & (u1 <= hw + fw)))
        cnt = reg.sum(1)
        cw = torch.where(fing, w64[None], 0.0).sum(1)
        yl, il = torch.where(reg, u1, math.inf).min(1)
        yr, ir = torch.where(reg, u1, -math.inf).max(1)
        b = R[:, :, 1]
        bn = torch.matmul(n64[None], b[:, :, None])[..., 0]
        wn = w64[None, :, None] * n64[None]
        left = reg & (u1 <= (yl + band)[:, None])
        right = reg & (u1 >= (yr - band)[:, None])
        NL = (torch.where(bn > 0, -1.0, 1.0)[..., None] * wn * left[..., None]).sum(1)
        NR = (torch.where(bn < 0, -1.0, 1.0)[..., None] * wn * right[..., None]).sum(1)
        ll, lr = NL.norm(dim=1), NR.norm(dim=1)
        valid = (cnt > 0) & (yl < yr) & (ll > 0) & (lr > 0)

        def ang(x):
            return torch.atan2(torch.linalg.cross(x, b).norm(dim=1), (x * b).sum(1))
        al, ar = ang(-NL / ll[:, None]), ang(NR / lr[:, None])
        ok = (gc[:, 1] > 0) & (gc[:, 2] > 0) & (gc[:, 3] >= -db) & torch.isfinite(gc).all(1)
        out["feasible"].append(ok & valid & (torch.maximum(al, ar) <= lim))
        out["region_count"].append(torch.where(ok, cnt, 0))
        ci = torch.stack([il, ir], 1)
        out["contact_idx"].append(torch.where((ok & (cnt > 0))[:, None], ci, -1))
    return {k: torch.cat(v) for k, v in out.items()}


def median_ms(fn, reps, warmup=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "grasp_bench needs the GPU"
    rows = []
    for name, n, m in (("scene", 1_000_000, 1024), ("object", 50_000, 1024), ("large", 5_000_000, 256)):
        p, nr, w, obj_p, obj_n = make_points(n, 50_000, seed=n)
        g = make_grasps(m, obj_p, obj_n, seed=m)
        fused = contacts(p, nr, w, g)
        ref = torch_route(p, nr, w, g)
        torch.cuda.synchronize()
        mism = int(((fused.contact_idx != ref["contact_idx"]).any(1) | (fused.region_count != ref["region_count"])
                    | (fused.feasible != ref["feasible"])).sum())
        f_med, f_min = median_ms(lambda: contacts(p, nr, w, g), a.reps)
        t_med, t_min = median_ms(lambda: torch_route(p, nr, w, g), a.torch_reps, warmup=1)
        row = {"shape": name, "N": n, "M": m, "fused_ms_median": round(f_med, 4), "fused_ms_min": round(f_min, 4),
               "torch_ms_median": round(t_med, 3), "torch_ms_min": round(t_min, 3),
               "speedup_median": round(t_med / f_med, 1), "pair_tests_per_s": f"{n * m * 2 / (f_med * 1e-3):.3e}",
               "grasps_with_points": int((fused.region_count > 0).sum()),
               "feasible": int(fused.feasible.sum()), "grasps_differing_from_torch": mism,
               "residency": "inputs Infinity-Cache resident across repetitions (28 B/point), not L2"}
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
