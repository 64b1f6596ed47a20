"""GPU time of known free space (gaussiangrasper_amd.field on gg_depth_min_pyramid, gg_field_observe and
gg_field_distance_known) at the size of a scan:

    pyramid   the min-depth pyramids of 200 frames of 640 x 480
    observe   those frames into 128^3 and 256^3 cells of a synthetic table scene (a floor, a table slab and a box on it
              inside 2.56 m, ray-cast exactly from a ring of cameras), next to a torch restatement of the same rule,
              chunked by view, on the same GPU (the counts are compared first); and how many (brick, view) pairs the
              brick cull skips, from a torch restatement of the kernel's brick test
    update    DistanceField.update(unknown="blocked") against update()

    python tools/observe_bench.py [--reps 10] [--views 200] [--out profiles/observe_bench.json]

Every GPU figure is the median [min, max] of --reps device-event timings after 3 warm-up calls (the torch restatement:
of --torch-reps after one).  `observe` and `pyramid` time the Python call: its host checks and, for observe, the upload of
the intrinsics and poses are inside.  `observe_kernel` and `pyramid_kernels` are the library's own event brackets around
the launches alone (GG_K_FIELD_OBSERVE, GG_K_DEPTH_PYRAMID), from a separate pass of --reps calls."""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiangrasper_amd import _lib, field  # noqa: E402

WARMUP = 3
SIDE = 2.56
H, W = 480, 640
K = (525.0, 525.0, 319.5, 239.5)
BOXES = (((0.4, 0.4, 0.75), (2.16, 2.16, 0.8)), ((1.0, 1.1, 0.8), (1.3, 1.5, 1.05)))      # table slab, box on it
K_PYRAMID, K_OBSERVE = 54, 55     # gg_raster.h GG_K_DEPTH_PYRAMID / GG_K_FIELD_OBSERVE
BRICK = (4, 8, 8)                  # csrc/field_observe.hip FO_BX, FO_BY, FO_BZ
TOL, SANE = 1e-9, 2.0 ** 24        # FO_TOL, FO_SANE


def timed(fn, reps, warmup=WARMUP):
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
    return {"ms_median": round(float(np.median(ts)), 4), "ms_min": round(float(np.min(ts)), 4),
            "ms_max": round(float(np.max(ts)), 4)}


def bracketed(kid, fn, reps):
    """the library's own event bracket of kernel id `kid`, one reading per call of fn"""
    lib = _lib.load()
    fn()
    torch.cuda.synchronize()
    lib.gg_prof_enable(1)
    ts = []
    try:
        for _ in range(reps):
            lib.gg_prof_reset()
            fn()
            torch.cuda.synchronize()
            n, ms = ctypes.c_int(0), ctypes.c_double(0.0)
            lib.gg_prof_get(kid, ctypes.byref(n), ctypes.byref(ms))
            assert n.value == 1, f"kernel id {kid}: {n.value} brackets in one call"
            ts.append(ms.value)
    finally:
        lib.gg_prof_reset()
        lib.gg_prof_enable(0)
    return {"ms_median": round(float(np.median(ts)), 4), "ms_min": round(float(np.min(ts)), 4),
            "ms_max": round(float(np.max(ts)), 4)}


def look_at(eye, target):
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, (0.0, 0.0, 1.0))
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return np.concatenate([R, (-R @ eye)[:, None]], 1)


def cameras(n):
    """a ring of cameras at two heights around the table, looking at it: OpenCV world-to-camera (n, 3, 4)"""
    out = []
    for i in range(n):
        a = 2.0 * math.pi * i / n
        r, z = (1.9, 1.5) if i % 2 else (2.4, 2.1)
        eye = np.array([SIDE / 2 + r * math.cos(a), SIDE / 2 + r * math.sin(a), z])
        out.append(look_at(eye, np.array([SIDE / 2, SIDE / 2, 0.8])))
    return np.stack(out)


def ray_depth(E, dev):
    """(V, H, W) float32 z-depth of the floor z = 0 and the boxes through every pixel's centre; +inf where nothing is"""
    E = torch.as_tensor(E, dtype=torch.float64, device=dev)
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64) + 0.5,
                          torch.arange(W, device=dev, dtype=torch.float64) + 0.5, indexing="ij")
    dc = torch.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], torch.ones_like(u)], -1)
    out = []
    for e in E:
        R, eye = e[:, :3], -e[:, :3].T @ e[:, 3]
        dw = dc @ R
        s = -eye[2] / dw[..., 2]
        best = torch.where((s > 0) & torch.isfinite(s), s, torch.full_like(s, math.inf))
        for lo, hi in BOXES:
            t0 = (torch.tensor(lo, dtype=torch.float64, device=dev) - eye) / dw
            t1 = (torch.tensor(hi, dtype=torch.float64, device=dev) - eye) / dw
            tn, tf = torch.minimum(t0, t1).max(-1).values, torch.maximum(t0, t1).min(-1).values
            best = torch.where((tn <= tf) & (tf > 0), torch.minimum(best, tn.clamp_min(0.0)), best)
        out.append(best.float())
    return torch.stack(out)


def level_table(h, w):
    shapes = []
    while True:
        shapes.append((h, w))
        if h == 1 and w == 1:
            break
        h, w = (h + 1) // 2, (w + 1) // 2
    off = np.concatenate([[0], np.cumsum([a * b for a, b in shapes])[:-1]])
    return shapes, off


def torch_observe(seen, looked, grid, dims, pyr, Kd, Ed, radius, margin, near):
    """the contract of gg_field_observe in torch operations on the device, a view at a time"""
    dev = pyr.device
    shapes, off = level_table(H, W)
    offs = torch.as_tensor(off, device=dev)
    wl = torch.as_tensor([s[1] for s in shapes], device=dev)
    ax = [float(grid[a]) + (torch.arange(int(dims[a]), device=dev, dtype=torch.float64) + 0.5) * float(grid[3])
          for a in range(3)]
    c = [ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]]
    ns, nl = torch.zeros_like(seen, dtype=torch.int32), torch.zeros_like(seen, dtype=torch.int32)
    pad = 2.0 ** -20

    def axis(a, zn, zf, f, cc, n):
        xl, xh = a - radius, a + radius
        ul = f * (xl / torch.where(xl < 0, zn, zf)) + cc
        uh = f * (xh / torch.where(xh > 0, zn, zf)) + cc
        A, B = torch.floor(ul - pad), torch.floor(uh + pad)
        ok = (A >= 0) & (B <= n - 1)
        return ok, torch.where(ok, A, 0.0).long(), torch.where(ok, B, 0.0).long()

    for v in range(pyr.shape[0]):
        e, k = Ed[v], Kd[v]
        p = [((e[r, 0] * c[0] + e[r, 1] * c[1]) + e[r, 2] * c[2]) + e[r, 3] for r in range(3)]
        zn, zf = p[2] - radius, p[2] + radius
        oku, Au, Bu = axis(p[0], zn, zf, k[0], k[2], W)
        okv, Av, Bv = axis(p[1], zn, zf, k[1], k[3], H)
        lk = (zn >= near) & oku & okv
        Au, Bu, Av, Bv = (torch.where(lk, t, 0) for t in (Au, Bu, Av, Bv))
        l = torch.zeros_like(Au)
        for _ in range(len(shapes)):
            l = l + ((((Bu >> l) - (Au >> l)) > 1) | (((Bv >> l) - (Av >> l)) > 1)).long()
        m = None
        for yy in (Av >> l, Bv >> l):
            for xx in (Au >> l, Bu >> l):
                t = pyr[v][offs[l] + yy * wl[l] + xx]
                m = t if m is None else torch.minimum(m, t)
        nl += lk.int()
        ns += (lk & (m.double() > zf + margin)).int()
    to16 = lambda old, n: (old.to(torch.int32) + n).clamp_max(65535).to(torch.uint16)
    return to16(seen, ns), to16(looked, nl)


def culled_pairs(grid, dims, Kd, Ed, radius, near):
    """(brick, view) pairs gg_field_observe's brick test skips: fo_brick_sees of csrc/field_observe.hip in torch"""
    dev = Ed.device
    lo_hi = []
    for a in range(3):
        first = torch.arange(0, int(dims[a]), BRICK[a], device=dev)
        last = torch.clamp(first + BRICK[a], max=int(dims[a])) - 1
        centre = lambda i: float(grid[a]) + (i.double() + 0.5) * float(grid[3])
        lo_hi.append((centre(first), centre(last)))
    shape = [len(lo_hi[a][0]) for a in range(3)]
    skipped = 0
    for v in range(Ed.shape[0]):
        e, k = Ed[v], Kd[v]
        fx, fy, cx, cy = (float(t) for t in k)
        if not (0 < fx <= SANE and 0 < fy <= SANE and abs(cx) <= SANE and abs(cy) <= SANE):
            continue
        pmax = [torch.maximum(lo_hi[a][0].abs(), lo_hi[a][1].abs()) for a in range(3)]
        bc = lambda t, a: t.reshape([-1 if b == a else 1 for b in range(3)])
        B = [((e[r, 0].abs() * bc(pmax[0], 0) + e[r, 1].abs() * bc(pmax[1], 1)) + e[r, 2].abs() * bc(pmax[2], 2))
             + e[r, 3].abs() for r in range(3)]
        mu = TOL * (fx * B[0] + (abs(cx) + W) * B[2])
        mv = TOL * (fy * B[1] + (abs(cy) + H) * B[2])
        tests = [torch.ones(shape, dtype=torch.bool, device=dev) for _ in range(5)]
        for corner in range(8):
            q = [bc(lo_hi[a][(corner >> (2 - a)) & 1], a) for a in range(3)]
            cc = [((e[r, 0] * q[0] + e[r, 1] * q[1]) + e[r, 2] * q[2]) + e[r, 3] for r in range(3)]
            tests[0] &= cc[2] - radius < near - TOL * ((B[2] + radius) + near)
            tests[1] &= fx * cc[0] + cx * cc[2] < -mu
            tests[2] &= fx * cc[0] + (cx - W) * cc[2] > mu
            tests[3] &= fy * cc[1] + cy * cc[2] < -mv
            tests[4] &= fy * cc[1] + (cy - H) * cc[2] > mv
        skipped += int((tests[0] | tests[1] | tests[2] | tests[3] | tests[4]).sum())
    return skipped, int(np.prod(shape)) * int(Ed.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--out", default="profiles/observe_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "observe_bench needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    E = cameras(a.views)
    Kh = np.tile(np.array(K), (a.views, 1))
    depth = ray_depth(E, dev)
    Kd, Ed = torch.from_numpy(Kh).to(dev), torch.from_numpy(E).to(dev)
    rows = []
    pyr = field.depth_pyramid(depth)
    t = timed(lambda: field.depth_pyramid(depth), a.reps)
    row = {"what": "field.depth_pyramid (gg_depth_min_pyramid)", "frames": a.views, "height": H, "width": W,
           "texels_per_frame": int(pyr.shape[1]), "pixels_without_a_reading": int((pyr[:, :H * W] == 0).sum()),
           "pixels_at_infinity": int(torch.isinf(pyr[:, :H * W]).sum()), "pyramid": t,
           "pyramid_kernels": bracketed(K_PYRAMID, lambda: field.depth_pyramid(depth), a.reps),
           "GB_per_second_read_and_written": round((depth.numel() + pyr.numel()) * 4 / (t["ms_median"] * 1e-3) / 1e9, 1)}
    rows.append(row)
    print(json.dumps(row), flush=True)
    for cells in (128, 256):
        f = field.DistanceField([0.0] * 3, [SIDE] * 3, SIDE / cells, device=dev)
        radius = field.cell_ball(f.h)
        args = (f.grid, f.dims, pyr, Kh, E, H, W, radius, field.OBSERVE_MARGIN, field.OBSERVE_NEAR)
        seen, looked = torch.zeros_like(f.mass, dtype=torch.uint16), torch.zeros_like(f.mass, dtype=torch.uint16)
        field.observe(seen, looked, *args)
        zero = torch.zeros_like(seen)
        want = torch_observe(zero, zero, f.grid, f.dims, pyr, Kd, Ed, radius, field.OBSERVE_MARGIN, field.OBSERVE_NEAR)
        same = bool((seen.view(torch.int16) == want[0].view(torch.int16)).all()) and \
            bool((looked.view(torch.int16) == want[1].view(torch.int16)).all())
        assert same, "the kernel's counts differ from the torch restatement's"
        skipped, pairs = culled_pairs(f.grid, f.dims, Kd, Ed, radius, field.OBSERVE_NEAR)
        scratch, scratch2 = torch.zeros_like(seen), torch.zeros_like(seen)
        t_k = timed(lambda: field.observe(scratch, scratch2, *args), a.reps)
        t_kernel = bracketed(K_OBSERVE, lambda: field.observe(scratch, scratch2, *args), a.reps)
        t_t = timed(lambda: torch_observe(zero, zero, f.grid, f.dims, pyr, Kd, Ed, radius, field.OBSERVE_MARGIN,
                                          field.OBSERVE_NEAR), a.torch_reps, warmup=1)
        s32, l32 = seen.to(torch.int32), looked.to(torch.int32)
        row = {"what": "field.observe (gg_field_observe) against a torch restatement, a view at a time, on the same GPU",
               "cells": [cells] * 3, "views": a.views, "radius": radius, "margin": field.OBSERVE_MARGIN,
               "near": field.OBSERVE_NEAR, "counts_agree": same,
               "cells_seen_by_min_views": int((s32 >= field.OBSERVE_MIN_VIEWS).sum()),
               "cells_looked_at": int((l32 > 0).sum()), "cell_views_looked_at": int(l32.sum()),
               "cell_views_seen_free": int(s32.sum()), "brick_view_pairs": pairs, "brick_view_pairs_culled": skipped,
               "observe": t_k, "observe_kernel": t_kernel, "torch": t_t, "torch_reps": a.torch_reps,
               "speedup": round(t_t["ms_median"] / t_k["ms_median"], 1),
               "cell_views_per_second": round(cells ** 3 * a.views / (t_kernel["ms_median"] * 1e-3))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        # the table's Gaussians stand in as occupied cells on its surfaces
        idx = [torch.arange(cells, device=dev, dtype=torch.float64).add(0.5).mul(f.h)] * 3
        x, y, z = idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]
        occ = (z < f.h) | torch.zeros_like(f.mass, dtype=torch.bool)
        for lo, hi in BOXES:
            occ |= (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
        f.mass[occ] = field.VOTE_ONE
        f.seen, f.looked = seen, looked
        t_free = timed(lambda: f.update(), a.reps)
        free_zero = int((f.dist2 == 0).sum())
        t_blocked = timed(lambda: f.update(unknown="blocked"), a.reps)
        row = {"what": "DistanceField.update(unknown='blocked') (gg_field_distance_known) against update() "
                       "(gg_field_distance)", "cells": [cells] * 3, "min_views": field.OBSERVE_MIN_VIEWS,
               "knowledge": f.knowledge(), "seed_cells_free": free_zero, "seed_cells_blocked": int((f.dist2 == 0).sum()),
               "update": t_free, "update_blocked": t_blocked}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARMUP, "rows": rows}, fh,
                      indent=1)


if __name__ == "__main__":
    main()
