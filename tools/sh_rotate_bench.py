"""GPU time of the SH rotation of moved Gaussians (gaussiangrasper_amd.sh_rotation -> gg_sh_rotate) at 5 M rows with
K = 16 and K = 25 bases and 1 %, 10 % and 100 % of the rows selected, next to the torch restatement on the same GPU
(`sh[mask.bool(), lo:hi] = einsum(D_l, ...)` per band: a gather, a product and a scatter per band), and of the scene
update with and without it (gg_hull_edit + gg_sh_rotate against gg_hull_edit alone, at tools/edit_bench.py's shapes).

    python tools/sh_rotate_bench.py [--reps 10] [--out profiles/sh_rotate_bench.json]

Every figure is the median [min, max] of --reps device-event timings after 3 warm-up calls; the selected rows are a
seeded uniform draw (the scan of the mask is the same wherever they lie; a grasped object's rows are as scattered).
The bands are built on the host once, outside the timed window (their cost is reported as host_bands_ms).  The
kernel is not a throughput hot spot and no time is promised for it: the figures say what the opt-in costs."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edit_bench import planes_for, sphere_points  # noqa: E402
from gaussiangrasper_amd import sh_rotation  # noqa: E402
from gaussiangrasper_amd.edit import rotvec_to_matrix, select_and_move  # noqa: E402

WARMUP = 3


def timed(fn, reps):
    for _ in range(WARMUP):
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


def torch_rotate(sh, sel, bands_dev):
    """the torch restatement: per band a gather of the selected rows, a product, a scatter"""
    for l, D in enumerate(bands_dev, start=1):
        lo, hi = l * l, (l + 1) * (l + 1)
        sh[sel, lo:hi] = torch.einsum("ab,nbc->nac", D, sh[sel, lo:hi])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sh_rotate_bench needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    R = rotvec_to_matrix([0.9, -1.3, 0.6])
    t0 = time.perf_counter()
    bands = sh_rotation.rotation_bands(R)
    host_bands_ms = (time.perf_counter() - t0) * 1e3
    rows = []
    n = a.rows
    for k in (16, 25):
        deg = sh_rotation.NUM_BASES.index(k)
        packed = sh_rotation.pack_bands(bands, k)
        bands_dev = [torch.from_numpy(D.astype(np.float32)).to(dev) for D in bands[:deg]]
        g = torch.Generator().manual_seed(k)
        sh = torch.randn(n, k, 3, generator=g).to(dev)
        for frac in (0.01, 0.1, 1.0):
            mask = (torch.rand(n, generator=g) < frac).to(torch.uint8).to(dev)
            sel = mask.bool()
            selected = int(mask.sum().item())
            row = {"what": "gg_sh_rotate", "N": n, "K": k, "selected": selected, "fraction": frac,
                   "hip": timed(lambda: sh_rotation.launch(sh, mask, packed, dev), a.reps),
                   "torch": timed(lambda: torch_rotate(sh, sel, bands_dev), a.reps),
                   # least traffic: the mask once, the selected rows past band 0 in and out
                   "min_bytes": n + selected * 3 * (k - 1) * 4 * 2}
            row["hip_gb_per_s_min_traffic"] = round(row["min_bytes"] / (row["hip"]["ms_median"] * 1e-3) / 1e9, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del sh
    # the scene update with and without the rotation, at edit_bench's shapes (identity move: every repetition selects
    # the same rows; the rotation's launch is issued as select_and_move(sh=) issues it)
    eye = np.eye(3, 4, dtype=np.float32)
    packed = sh_rotation.pack_bands(bands, 25)
    for n in (1_000_000, 5_000_000):
        g = torch.Generator().manual_seed(n)
        means = ((torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 1.0, 0.5])).to(dev)
        quats = torch.randn(n, 4, generator=g).to(dev)
        sh = torch.randn(n, 25, 3, generator=g).to(dev)
        for m in (52, 502):
            planes, kind = planes_for(sphere_points(m, 0.12, m))
            pl = torch.from_numpy(planes).to(dev)

            def edit_only():
                return select_and_move(means, quats, pl, eye)

            def edit_and_rotate():
                mask, count = select_and_move(means, quats, pl, eye)
                sh_rotation.launch(sh, mask, packed, dev)
                return mask, count
            _, count = edit_only()
            row = {"what": "gg_hull_edit with and without gg_sh_rotate", "N": n, "K": 25, "F": int(planes.shape[0]),
                   "hull": kind, "selected": int(count.item()), "hull_edit": timed(edit_only, a.reps),
                   "hull_edit_and_sh_rotate": timed(edit_and_rotate, a.reps)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del means, quats, sh
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARMUP,
                       "host_bands_ms": round(host_bands_ms, 3), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
