"""Time of one grasp-NMS call (gaussiangrasper_amd.grasp.nms -> gg_grasp_nms, order construction and the read-back of
the kept count included) at 4096 and 32 768 active proposer-like rows, against
  * a torch restatement on the same GPU: the fp64 near matrix in chunks of rows, copied to the host, and the greedy
    walk there over the copied matrix (one row OR per kept row);
  * the numpy restatement on one core: a loop over the order, each row against the rows kept so far.

    python tools/grasp_nms_bench.py [--reps 20] [--torch-reps 3] [--out profiles/grasp_nms_bench.json]

Rows: seeds on the faces of an 8 x 6 x 5 cm box, the closing axis the face normal, the centre on the box's mid-plane,
8 approach directions around the closing axis per seed, random scores: neighbouring seeds and antipodal seeds give
near-copies, as gg_grasp_propose's output does.  Wall-clock times around a device synchronisation, after 3 warm-up
calls; median, minimum and maximum of --reps calls.  With --kernels, gg_prof's time of the three launches together
is recorded too (a separate set of calls).  Each row records whether the three routes agree on keep."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussiangrasper_amd import grasp  # noqa: E402

TRANSLATION, ROTATION = grasp.NMS_TRANSLATION, grasp.NMS_ROTATION
SIZE = np.array([0.08, 0.06, 0.05])


def make_rows(m: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    s = -(-m // 8)
    ax = rng.integers(0, 3, s)
    sign = rng.choice([-1.0, 1.0], s)
    p = rng.uniform(-0.5, 0.5, size=(s, 3)) * SIZE
    p[np.arange(s), ax] = 0.0                                 # the grasp centre: the seed on the mid-plane
    b = np.zeros((s, 3))
    b[np.arange(s), ax] = sign
    u = np.zeros((s, 3))
    u[np.arange(s), (ax + 1) % 3] = 1.0
    v = np.cross(b, u)
    ang = (np.arange(8) * (2 * math.pi / 8))[None, :, None] + rng.uniform(0, 0.05, size=(s, 1, 1))
    a = np.cos(ang) * u[:, None] + np.sin(ang) * v[:, None]   # (s, 8, 3) approach
    bb = np.broadcast_to(b[:, None], a.shape)
    R = np.stack([a, bb, np.cross(a, bb)], axis=-1)           # columns a, b, c
    g = np.zeros((s * 8, 17), np.float32)
    g[:, 0] = rng.random(s * 8)
    g[:, 1:4] = (0.07, 0.02, 0.02)
    g[:, 4:13] = R.reshape(-1, 9)
    g[:, 13:16] = np.repeat(p, 8, axis=0)
    return g[:m]


def near_numpy(R, t, i, js, tt, bound):
    d = t[i] - t[js]
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    c = [(R[i, 0, k] * R[js, 0, k] + R[i, 1, k] * R[js, 1, k]) + R[i, 2, k] * R[js, 2, k] for k in range(3)]
    return (dd <= tt) & (((c[0] + c[1]) + c[2] >= bound) | ((c[0] - c[1]) - c[2] >= bound))


def numpy_route(g: np.ndarray, order: np.ndarray) -> np.ndarray:
    G = g.astype(np.float64)
    R, t = G[:, 4:13].reshape(-1, 3, 3), G[:, 13:16]
    tt, bound = TRANSLATION * TRANSLATION, 1.0 + 2.0 * math.cos(ROTATION)
    keep, kept = np.zeros(len(g), bool), []
    for r in order:
        if kept and near_numpy(R, t, r, np.asarray(kept), tt, bound).any():
            continue
        keep[r] = True
        kept.append(r)
    return keep


@torch.no_grad()
def torch_route(g: torch.Tensor, order: torch.Tensor, chunk: int = 2048) -> np.ndarray:
    G = g.double()[order.long()]
    R, t = G[:, 4:13].reshape(-1, 3, 3), G[:, 13:16]
    tt, bound = TRANSLATION * TRANSLATION, 1.0 + 2.0 * math.cos(ROTATION)
    blocks = []
    for s in range(0, G.shape[0], chunk):
        d = t[s:s + chunk, None] - t[None]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        c = [(R[s:s + chunk, None, 0, k] * R[None, :, 0, k] + R[s:s + chunk, None, 1, k] * R[None, :, 1, k])
             + R[s:s + chunk, None, 2, k] * R[None, :, 2, k] for k in range(3)]
        blocks.append((dd <= tt) & (((c[0] + c[1]) + c[2] >= bound) | ((c[0] - c[1]) - c[2] >= bound)))
    near = torch.cat(blocks).cpu().numpy()
    removed = np.zeros(G.shape[0], bool)
    keep = np.zeros(g.shape[0], bool)
    rows = order.cpu().numpy()
    for p in range(G.shape[0]):
        if not removed[p]:
            keep[rows[p]] = True
            removed |= near[p]
    return keep


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
    """gg_prof's device time of gg_grasp_nms' launches, per call"""
    import ctypes
    from gaussiangrasper_amd import _lib
    lib = _lib.load()
    lib.gg_prof_enable(1)
    lib.gg_prof_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    n, ms = ctypes.c_int(0), ctypes.c_double(0.0)
    lib.gg_prof_get(51, ctypes.byref(n), ctypes.byref(ms))
    lib.gg_prof_enable(0)
    return round(ms.value / max(n.value, 1), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "grasp_nms_bench needs the GPU"
    rows = []
    for m in (4096, 32768):
        g_np = make_rows(m, seed=m)
        g = torch.from_numpy(g_np).cuda()

        def fused():
            return grasp.nms(g, None, max_candidates=m)
        rec = fused()
        order = grasp.nms_order(g, None, m)
        keep = rec.keep.cpu().numpy()
        t_keep = torch_route(g, order)
        row = {"active_rows": m, "kept": int(keep.sum()), "workspace_MiB": round(m * ((m + 63) // 64) * 8 / 2 ** 20, 1),
               "fused_ms": wall_ms(fused, a.reps), "torch_ms": wall_ms(lambda: torch_route(g, order), a.torch_reps, 1),
               "torch_agrees": bool(np.array_equal(keep, t_keep))}
        if a.kernels:
            row["fused_kernels_ms"] = kernel_ms(fused, a.reps)
        if not a.skip_numpy:
            t0 = time.perf_counter()
            n_keep = numpy_route(g_np, order.cpu().numpy())
            row["numpy_one_core_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["numpy_agrees"] = bool(np.array_equal(keep, n_keep))
        row["speedup_over_torch_median"] = round(row["torch_ms"]["median"] / row["fused_ms"]["median"], 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del g, rec
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "translation": TRANSLATION, "rotation": ROTATION,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
