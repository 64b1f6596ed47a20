"""Scene preparation timings (gaussiangrasper_amd.prepare) on the GPU against the host routes the reference takes:

    frames     back-projection + normal maps of 200 synthetic 640x480 frames, device time (no file I/O, frames already
               on the device, batches of 16), against a numpy restatement of the reference's per-frame steps
               (depth_image_to_point_cloud + merge_point_clouds, cal_normal without its file writes)
    knn        exact 3-NN (gg_knn) of 0.25 / 1 / 3 M surface-like points against sklearn NearestNeighbors(4) fit +
               kneighbors in the same process (k_nearest_sklearn); the distances are compared bit for bit
    worst      1 M points + 100 far outliers, 1 M points + 1 % far outliers, and 1 M identical points
    cli        python -m gaussiangrasper_amd.prepare on a synthetic 200-frame 640x480 scan, its own breakdown

    python tools/prepare_bench.py [--out profiles/prepare_bench.json] [--skip-host] [--skip-cli]

Surface-like points: a table plane with 0.5 mm noise and five spheres of radius 3-8 cm on it (the seed clouds of
a tabletop scan).  GPU times: median of 5 calls after a warm-up, host clock around a device synchronise.  Host times:
one call each (the reference runs them once per model construction)."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prepare_ref as R  # noqa: E402
from gaussiangrasper_amd.prepare import backproject_frames, depth_normals, knn_distances  # noqa: E402


def gpu_time(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def surface_points(n, seed):
    rng = np.random.default_rng(seed)
    n_t = n // 2
    table = np.stack([rng.uniform(-0.4, 0.4, n_t), rng.uniform(-0.3, 0.3, n_t), -0.2 + 0.0005 * rng.normal(size=n_t)], 1)
    k = n - n_t
    c = np.stack([rng.uniform(-0.3, 0.3, 5), rng.uniform(-0.2, 0.2, 5), np.zeros(5)], 1)
    r = rng.uniform(0.03, 0.08, 5)
    c[:, 2] = -0.2 + r
    which = rng.integers(0, 5, k)
    d = rng.normal(size=(k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([table, c[which] + r[which, None] * d]).astype(np.float32)


def synthetic_frames(f, h, w, seed):
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:h, 0:w]
    depth = np.empty((f, h, w))
    T = np.empty((f, 4, 4))
    for i in range(f):
        depth[i] = 0.45 + 0.05 * np.sin(u / 40.0 + i) * np.cos(v / 30.0) + 0.001 * rng.normal(size=(h, w))
        T[i] = np.eye(4)
        T[i, :3, :3] = R.rodrigues(rng.normal(size=3) * 0.1) @ np.diag([1.0, -1.0, -1.0])
        T[i, :3, 3] = [rng.normal() * 0.02, rng.normal() * 0.02, 0.25]
    depth[rng.random((f, h, w)) < 0.02] = 0.0
    mask = (rng.random((f, h, w)) > 0.05).astype(np.uint8)
    rgb = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
    intr = np.array([[385.86016845703125, 385.3817443847656, 325.68145751953125, 243.561767578125]] * f)
    return depth, mask, rgb, intr, T


def bench_frames(skip_host):
    F, H, W, B = 200, 480, 640, 16
    depth, mask, rgb, intr, T = synthetic_frames(F, H, W, 0)
    dd, dm, dr = torch.from_numpy(depth).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(rgb).cuda()
    n_pts = [0]

    def run():
        n_pts[0] = 0
        for b in range(0, F, B):
            p, _ = backproject_frames(dd[b:b + B], dm[b:b + B], dr[b:b + B], intr[b:b + B], T[b:b + B])
            depth_normals(dd[b:b + B], intr[b:b + B], T[b:b + B])
            n_pts[0] += p.shape[0]
    med, mn = gpu_time(run, reps=5)
    row = {"what": "backprojection + normals, 200 x 640x480, device", "gpu_ms_median": med * 1e3,
           "gpu_ms_min": mn * 1e3, "points": n_pts[0]}
    if not skip_host:
        t0 = time.perf_counter()
        for i in range(F):
            R.backproject_literal(depth[i], mask[i], rgb[i], *intr[i], T[i])
            R.normals_literal(depth[i], intr[i][0], intr[i][1], T[i])
        row["numpy_ms"] = (time.perf_counter() - t0) * 1e3
        row["speedup"] = row["numpy_ms"] / row["gpu_ms_median"]
    return row


def bench_knn(n, skip_host, x=None, label=None):
    x = surface_points(n, n) if x is None else x
    xt = torch.from_numpy(x).cuda()
    out = {}

    def run():
        out["d"] = knn_distances(xt, 3)[0]
    med, mn = gpu_time(run)
    row = {"what": label or f"knn k=3, {n} surface-like points", "n": int(x.shape[0]), "gpu_ms_median": med * 1e3,
           "gpu_ms_min": mn * 1e3}
    if not skip_host:
        try:
            from sklearn.neighbors import NearestNeighbors
        except ImportError:
            row["sklearn"] = "not installed here"
            return row
        t0 = time.perf_counter()
        m = NearestNeighbors(n_neighbors=4, algorithm="auto", metric="euclidean").fit(x)
        t1 = time.perf_counter()
        ref = m.kneighbors(x)[0][:, 1:].astype(np.float32)
        t2 = time.perf_counter()
        row.update(sklearn_fit_s=t1 - t0, sklearn_query_s=t2 - t1, sklearn_ms=(t2 - t0) * 1e3,
                   speedup=(t2 - t0) * 1e3 / row["gpu_ms_median"],
                   bit_equal=bool(np.array_equal(out["d"].cpu().numpy().view(np.uint32), ref.view(np.uint32))))
    return row


def bench_cli():
    tmp = tempfile.mkdtemp(prefix="gg_prepare_bench_")
    try:
        scan = os.path.join(tmp, "scan")
        from PIL import Image
        depth, mask, rgb, intr, T = synthetic_frames(200, 480, 640, 1)
        v, u = np.mgrid[0:480, 0:640]
        smooth = np.stack([u % 256, v % 256, (u + v) % 256], -1).astype(np.uint8)
        meta = {"fl_x": intr[0, 0], "fl_y": intr[0, 1], "cx": intr[0, 2], "cy": intr[0, 3], "w": 640, "h": 480,
                "k1": -0.055006977170705795, "k2": 0.06818309426307678, "p1": -0.0007415282307192683,
                "p2": 0.0006959497695788741, "frames": []}
        for d in ("images", "depths", "boundary_mask"):
            os.makedirs(os.path.join(scan, d))
        for i in range(200):
            stem = f"images_{i + 1:04d}"
            meta["frames"].append({"file_path": f"images/{stem}.png", "transform_matrix": T[i].tolist()})
            np.save(os.path.join(scan, "depths", stem + ".npy"), np.round(depth[i] * 1000).astype(np.uint16))
            Image.fromarray(smooth).save(os.path.join(scan, "images", stem + ".png"), compress_level=1)
            np.save(os.path.join(scan, "boundary_mask", stem + ".npy"), mask[i])
        with open(os.path.join(scan, "transforms.json"), "w") as f:
            json.dump(meta, f)
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-m", "gaussiangrasper_amd.prepare", "--scan", scan, "--out",
                            os.path.join(tmp, "out"), "--depth-units-per-metre", "1000"], cwd=ROOT,
                           capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        return {"what": "CLI, 200 x 640x480 scan (uint16 mm depth, npy masks)", "wall_s": wall,
                "stdout": r.stdout.replace(tmp, "<tmp>").strip().splitlines()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-cli", action="store_true")
    a = ap.parse_args()
    rows = [bench_frames(a.skip_host)]
    print(json.dumps(rows[-1]), flush=True)
    for n in (250_000, 1_000_000, 3_000_000):
        rows.append(bench_knn(n, a.skip_host))
        print(json.dumps(rows[-1]), flush=True)
    rng = np.random.default_rng(7)
    x = np.concatenate([surface_points(1_000_000, 1), (rng.normal(size=(100, 3)) * 1e3).astype(np.float32)])
    rows.append(bench_knn(0, True, x, "worst case: 1 M surface-like points + 100 far outliers (|x| ~ 1e3 m)"))
    print(json.dumps(rows[-1]), flush=True)
    x = np.concatenate([surface_points(1_000_000, 1), (rng.normal(size=(10_000, 3)) * 1e3).astype(np.float32)])
    rows.append(bench_knn(0, True, x, "worst case: 1 M surface-like points + 1 % far outliers (10 000, |x| ~ 1e3 m)"))
    print(json.dumps(rows[-1]), flush=True)
    rows.append(bench_knn(0, True, np.zeros((1_000_000, 3), np.float32), "worst case: 1 M identical points"))
    print(json.dumps(rows[-1]), flush=True)
    if not a.skip_cli:
        rows.append(bench_cli())
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
