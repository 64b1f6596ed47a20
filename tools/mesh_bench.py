"""GPU time of mesh export (gaussiangrasper_amd.mesh.TSDFVolume -> gg_tsdf_integrate, gg_tsdf_mesh_count /
gg_tsdf_mesh_emit) at 128^3 and 256^3 lattice points with 50 and 200 depth frames of 640 x 480, through the library's
profiling ids (GG_K_TSDF_INTEGRATE, GG_K_TSDF_MESH).  Comparison lines: a torch restatement of the reference
exporter's fusion (batches of 10 frames, every voxel projected into every frame of the batch, ray-distance SDF,
nearest grid_sample, weights capped at 1) on the same GPU, and the numpy extraction restatement (tests/tsdf_ref.py)
on one host core at 128^3.

    python tools/mesh_bench.py [--reps 10] [--out profiles/mesh_bench.json]

Scene: a sphere of radius 0.5 at the origin in the reference's default box [-1, 1]^3, exact ray-cast depth from
cameras on a Fibonacci sphere of radius 2 looking at it (fx = 576 px), so every frame sees the whole box.  Times are
means over --reps calls after 2 warm-up calls; the extraction time covers both of its calls (the count read-back in
between is host time, reported as wall time)."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsdf_ref as R  # noqa: E402
from gaussiangrasper_amd import _lib  # noqa: E402
from gaussiangrasper_amd.mesh import TSDFVolume  # noqa: E402

H, W = 480, 640
K_INTEGRATE, K_MESH = 43, 44     # gg_raster.h GG_K_TSDF_INTEGRATE / GG_K_TSDF_MESH


def frames(V):
    K = np.array([0.9 * W, 0.9 * W, W / 2, H / 2])
    E = R.sphere_cameras(V, 2.0)
    depth = np.stack([R.raycast_spheres(e, K, H, W, [((0.0, 0.0, 0.0), 0.5)]) for e in E])
    return torch.from_numpy(depth).cuda(), np.tile(K, (V, 1)), E


def prof_ms(lib, kid):
    n, ms = ctypes.c_int(0), ctypes.c_double(0.0)
    lib.gg_prof_get(kid, ctypes.byref(n), ctypes.byref(ms))
    return n.value, ms.value


def torch_reference_style(depth, K, E, n, trunc, batch=10):
    """The reference exporter's fusion rule, restated in torch: per batch of frames, every voxel into every frame;
    sdf = depth - |c|; nearest sample at align_corners=False; voxels with sdf < -trunc or no depth skipped; running
    blend with the total weight capped at 1."""
    dev = depth.device
    vs = 2.0 / n
    ax = -1.0 + torch.arange(n, device=dev, dtype=torch.float32) * vs
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)
    ph = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)
    tsdf = -torch.ones(pts.shape[0], device=dev)
    wts = torch.zeros(pts.shape[0], device=dev)
    Et = torch.as_tensor(E, dtype=torch.float32, device=dev)
    Kt = torch.as_tensor(K, dtype=torch.float32, device=dev)
    V, h, w = depth.shape
    for b0 in range(0, V, batch):
        e, k, d = Et[b0:b0 + batch], Kt[b0:b0 + batch], depth[b0:b0 + batch]
        c = torch.einsum("brc,pc->bpr", e, ph)                                   # (B, P, 3)
        z = c[..., 2].clamp_min(1e-6)
        u = k[:, None, 0] * c[..., 0] / z + k[:, None, 2]
        v = k[:, None, 1] * c[..., 1] / z + k[:, None, 3]
        grid = torch.stack([2 * u / w - 1, 2 * v / h - 1], dim=-1)[:, :, None, :]
        dd = torch.nn.functional.grid_sample(torch.nan_to_num(d, posinf=0.0)[:, None], grid, mode="nearest",
                                             align_corners=False)[:, 0, :, 0]
        sdf = dd - c.norm(dim=-1)
        ok = (dd > 0) & (sdf >= -trunc) & (grid.abs() <= 1).all(dim=-1)[..., 0]
        val = (sdf / trunc).clamp(-1.0, 1.0)
        for i in range(c.shape[0]):
            m = ok[i]
            nw = wts[m] + 1.0
            tsdf[m] = (tsdf[m] * wts[m] + val[i][m]) / nw
            wts[m] = nw.clamp(max=1.0)
    return tsdf, wts


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_bench needs the GPU"
    lib = _lib.load()
    rows = []
    cache = {V: frames(V) for V in (50, 200)}
    for n in (128, 256):
        for V in (50, 200):
            depth, K, E = cache[V]
            vol = TSDFVolume((-1.0,) * 3, (1.0,) * 3, n)

            def integrate():
                vol.tsdf.fill_(1.0)
                vol.weight.zero_()
                vol.integrate_w2c(depth, K, E)
            lib.gg_prof_enable(1)
            integrate()
            lib.gg_prof_reset()
            wall_i = timed(integrate, a.reps)
            cnt, ms_i = prof_ms(lib, K_INTEGRATE)
            lib.gg_prof_reset()
            mesh = None

            def extract():
                nonlocal mesh
                mesh = vol.extract()
            wall_m = timed(extract, a.reps)
            cnt_m, ms_m = prof_ms(lib, K_MESH)
            lib.gg_prof_enable(0)
            updates = n ** 3 * V
            row = {"what": "tsdf mesh export", "points": n, "views": V, "height": H, "width": W,
                   "integrate_gpu_ms": round(ms_i / max(cnt, 1), 4),
                   "integrate_wall_ms": round(1e3 * wall_i, 4),
                   "voxel_view_updates_per_s": round(updates / (ms_i / max(cnt, 1) * 1e-3), 1),
                   "extract_gpu_ms": round(ms_m / max(cnt_m // 2, 1), 4),          # two bracketed calls per extract
                   "extract_wall_ms": round(1e3 * wall_m, 4),
                   "vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0])}
            torch.cuda.synchronize()
            t_ref = timed(lambda: torch_reference_style(depth, K, E, n, vol.truncation), 1 if n == 256 else 2)
            row["torch_reference_style_integrate_ms"] = round(1e3 * t_ref, 2)
            row["speedup_vs_torch_reference_style"] = round(t_ref / (row["integrate_gpu_ms"] * 1e-3), 1)
            if n == 128 and V == 50:
                T, Wt = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
                t0 = time.perf_counter()
                v, _, _, f = R.extract(vol.dims, vol.grid, T, Wt)
                row["host_numpy_1core_extract_s"] = round(time.perf_counter() - t0, 3)
                m = mesh.numpy()
                row["extract_bit_equal_to_numpy"] = bool(np.array_equal(m.vertices.view(np.uint32),
                                                                         v.view(np.uint32))
                                                          and np.array_equal(m.faces, f))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
