#!/usr/bin/env python3
"""Language query (gaussiangrasper_amd.query, gg_clip_query) against the chain it replaces, one JSON line per shape:
  1600x1200, 32 -> 128 -> 512, Q = 4 (1 positive + 3 canonical negatives): the render.sh view;
  1920x1080, 128 -> 128 -> 512, Q = 4: BASELINE config 5's feature width.
`fused_ms`: query.relevancy (weight packing, W2^T q, the query kernel) timed with torch events, and the query kernel
bracket alone from the in-library hipEvents (GG_K_QUERY); `unfused_ms`: mlp_forward -> F.normalize -> @ q^T ->
softmax over (positive, negative) pairs -> min, timed the same way.  Peak device memory beyond the inputs for each.
`--out PATH` also writes the lines to PATH.
Roofline: the fused kernel's fp16 matrix work (four fp16 products per fp32 multiply-add, two-piece operands) against
2.5 PFLOP/s and its HBM bytes against 8 TB/s; the larger fraction names the bound."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "shim")]
import torch
import torch.nn.functional as F

from gaussiangrasper_amd import _lib, query
from gaussiangrasper_amd.mlp import MLP, mlp_forward

F16_PEAK_TFLOPS = 2500.0   # MI355X_MICROARCH.md: fp16 MFMA, dense
HBM_PEAK_GBS = 8000.0
GG_K_QUERY = 33
dev = "cuda:0"


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def peak_beyond(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def run(h, w, cin, cout=512, n_pos=1, n_neg=3, reps=10):
    lib = _lib.load()
    torch.manual_seed(0)
    m = MLP(cin, cout, [128]).to(dev)
    x = torch.randn(h, w, cin, device=dev)
    pos, neg = torch.randn(n_pos, cout), torch.randn(n_neg, cout)
    wts = (m.layers[0].weight, m.layers[0].bias, m.layers[2].weight, m.layers[2].bias)
    qn = F.normalize(torch.cat([pos, neg]).to(dev), dim=-1)

    def fused():
        return query.relevancy(x, m, pos, neg)

    def unfused():
        with torch.no_grad():
            s = F.normalize(mlp_forward(x, *wts), dim=-1) @ qn.T
            pair = torch.stack([s[..., :n_pos, None].expand(*s.shape[:-1], n_pos, n_neg),
                                s[..., None, n_pos:].expand(*s.shape[:-1], n_pos, n_neg)], -1)
            return torch.softmax(10.0 * pair, dim=-1)[..., 0].min(dim=-1).values

    fused_ms, r = timed(fused, reps)
    lib.gg_prof_reset()
    lib.gg_prof_enable(1)
    for _ in range(reps):
        fused()
    torch.cuda.synchronize()
    lib.gg_prof_enable(0)
    n, tot = ctypes.c_int(0), ctypes.c_double(0.0)
    lib.gg_prof_get(GG_K_QUERY, ctypes.byref(n), ctypes.byref(tot))
    unfused_ms, r_ref = timed(unfused, reps)
    err = float((r - r_ref).abs().max())
    fused_mib, unfused_mib = peak_beyond(fused), peak_beyond(unfused)
    rows = h * w
    f16_flops = 4 * 2.0 * rows * (cin * 128 + 128 * cout)
    hbm_bytes = rows * (cin + n_pos) * 4
    k_ms = tot.value / max(n.value, 1)
    mfma = f16_flops / (k_ms * 1e-3) / 1e12 / F16_PEAK_TFLOPS
    hbm = hbm_bytes / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
    return {
        "workload": f"{w}x{h} pixels, {cin}->128->{cout} fea_up, Q = {n_pos + n_neg} ({n_pos} positive + {n_neg} "
                    f"negatives), relevancy out",
        "fused_ms": fused_ms, "fused_kernel_bracket_ms": k_ms,
        "unfused_ms": unfused_ms, "fused_over_unfused": fused_ms / unfused_ms,
        "peak_mib_beyond_inputs": {"fused": fused_mib, "unfused": unfused_mib},
        "max_abs_diff_vs_unfused": err,
        "roofline": {"bound": "mfma_f16" if mfma >= hbm else "hbm",
                     "mfma_f16": {"achieved_tflops": f16_flops / (k_ms * 1e-3) / 1e12, "peak": F16_PEAK_TFLOPS,
                                  "frac": mfma},
                     "hbm": {"achieved_gbs": hbm_bytes / (k_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "frac": hbm}},
    }


if __name__ == "__main__":
    lines = [run(1200, 1600, 32), run(1080, 1920, 128)]
    for line in lines:
        print(json.dumps(line))
    if "--out" in sys.argv:                  # the same lines to a file, e.g. profiles/query_bench.json
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)
