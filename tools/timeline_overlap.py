#!/usr/bin/env python3
"""How much of the forward chain runs beside a blend kernel of the other stream: the timeline of a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 bench.py --gpus 1 --steps 6 --warmup 2
    python tools/timeline_overlap.py OUT/**/*_kernel_trace.csv [--skip-views 17]

Reads the per-dispatch start / end stamps (one row per dispatch: Kernel_Name, Start_Timestamp, End_Timestamp and
Stream_Id, or Queue_Id where the trace has no stream column) and looks at the PIPELINED steps only: the dispatches of the
two streams that carry the most blend kernels (dist.train_step_pipelined's; the probe view and whatever else runs on
the default stream is left out), after the first --skip-views views (warm-up).  It prints

  * per kernel name: launches, mean duration, workgroup size and registers as the trace reports them, and the share of
    the kernel's time during which a blend kernel of the OTHER stream was in flight (and of any stream but itself);
  * per view (a view = one pair forward; the window is cut into views at the pair forwards' starts): the time with no
    blend kernel in flight, mean / min / max, and which kernels ran in that time;
  * the time with no kernel in flight at all.

What counts as "pipelined" is up to the caller: trace a PLAIN bench.py run (no --full: its profiled steps run the same
kernels sequentially and would be mixed in if they shared the two streams) and pass as --skip-views the views of the
warm-up (warm-up steps x views per step, + 1 for the view in flight at the cut).

Measurement tool only; it inspects stamps, nothing else."""
import argparse
import bisect
import csv
import glob
import sys
from collections import defaultdict

BLEND = ("blend2_", "blend_fwd", "blend_bwd")


def short(name: str) -> str:
    name = name.strip().strip('"')
    if name.startswith("void "):
        name = name[5:]
    depth, out = 0, []
    for ch in name:                      # cut the argument list, keep template arguments
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            break
        out.append(ch)
    s = "".join(out)
    return s if len(s) <= 60 else s[:57] + "..."


def is_blend(name: str) -> bool:
    return name.startswith(BLEND)


def merge(iv):
    """union of intervals as a sorted list of disjoint (start, end)"""
    out = []
    for a, b in sorted(iv):
        if out and a <= out[-1][1]:
            if b > out[-1][1]:
                out[-1][1] = b
        else:
            out.append([a, b])
    return out


def covered(a, b, union, starts=None):
    """length of [a, b) inside the disjoint sorted intervals `union`"""
    if starts is None:
        starts = [u[0] for u in union]
    i = max(bisect.bisect_right(starts, a) - 1, 0)
    tot = 0
    while i < len(union) and union[i][0] < b:
        lo, hi = max(a, union[i][0]), min(b, union[i][1])
        if hi > lo:
            tot += hi - lo
        i += 1
    return tot


def complement(union, a, b):
    out, cur = [], a
    for lo, hi in union:
        if hi <= a or lo >= b:
            continue
        if lo > cur:
            out.append([cur, lo])
        cur = max(cur, hi)
    if cur < b:
        out.append([cur, b])
    return out


def read(paths):
    rows = []
    for pat in paths:
        for path in (glob.glob(pat, recursive=True) or [pat]):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    name = r.get("Kernel_Name")
                    if not name:
                        continue
                    stream = r.get("Stream_Id")
                    if stream in (None, ""):
                        stream = r.get("Queue_Id", "0")
                    wg = r.get("Workgroup_Size_X") or r.get("Workgroup_Size")
                    rows.append({"name": short(name), "stream": (r.get("Agent_Id", ""), stream),
                                 "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"]),
                                 "wg": wg or "?", "vgpr": r.get("VGPR_Count") or r.get("Arch_VGPR_Count") or "?",
                                 "lds": r.get("LDS_Block_Size") or "?"})
    rows.sort(key=lambda r: r["t0"])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace", nargs="+", help="kernel-trace CSV file(s) or glob(s)")
    ap.add_argument("--skip-views", type=int, default=0, help="leave out the first views of the pipelined streams")
    ap.add_argument("--forward-mark", default="blend2_fwd", help="prefix of the kernel that starts a view window")
    a = ap.parse_args()
    rows = read(a.trace)
    if not rows:
        print("no kernel dispatches in", a.trace)
        return 1
    per_stream = defaultdict(int)
    for r in rows:
        if is_blend(r["name"]):
            per_stream[r["stream"]] += 1
    pipe = sorted(per_stream, key=per_stream.get, reverse=True)[:2]
    if len(pipe) < 2:
        print("the blend kernels ran on one stream only: not a pipelined run", dict(per_stream))
        return 1
    rows = [r for r in rows if r["stream"] in pipe]
    marks = [r["t0"] for r in rows if r["name"].startswith(a.forward_mark)]
    if len(marks) <= a.skip_views + 1:
        print("fewer views than --skip-views")
        return 1
    w0, w1 = marks[a.skip_views], marks[-1]          # whole view windows only: [first kept forward, last forward)
    marks = marks[a.skip_views:]
    rows = [r for r in rows if r["t1"] > w0 and r["t0"] < w1]
    for r in rows:
        r["t0"], r["t1"] = max(r["t0"], w0), min(r["t1"], w1)
    nviews = len(marks) - 1
    blend_by_stream = {s: merge([(r["t0"], r["t1"]) for r in rows if r["stream"] == s and is_blend(r["name"])])
                       for s in pipe}
    other = {pipe[0]: blend_by_stream[pipe[1]], pipe[1]: blend_by_stream[pipe[0]]}
    other_starts = {s: [u[0] for u in other[s]] for s in pipe}
    any_blend = merge([tuple(u) for s in pipe for u in blend_by_stream[s]])
    any_kernel = merge([(r["t0"], r["t1"]) for r in rows])
    no_blend = complement(any_blend, w0, w1)
    nb_starts = [u[0] for u in no_blend]

    print("window: %d views of the two pipelined streams %s, %.3f ms, %.4f ms per view" %
          (nviews, [s[1] for s in pipe], (w1 - w0) / 1e6, (w1 - w0) / 1e6 / nviews))
    # ---- per kernel
    agg = defaultdict(lambda: {"n": 0, "dur": 0, "beside": 0, "alone": 0, "wg": set(), "vgpr": set(), "lds": set()})
    for r in rows:
        g = agg[r["name"]]
        d = r["t1"] - r["t0"]
        g["n"] += 1
        g["dur"] += d
        g["beside"] += covered(r["t0"], r["t1"], other[r["stream"]], other_starts[r["stream"]])
        g["alone"] += covered(r["t0"], r["t1"], no_blend, nb_starts)
        g["wg"].add(r["wg"]); g["vgpr"].add(r["vgpr"]); g["lds"].add(r["lds"])
    print()
    print("%-60s %6s %9s %9s %8s %8s %6s %6s %7s" % ("kernel", "calls", "mean us", "us/view", "beside", "no blend",
                                                      "wg", "vgpr", "lds"))
    print("%-60s %6s %9s %9s %8s %8s" % ("", "", "", "", "other's", "at all"))
    for name, g in sorted(agg.items(), key=lambda kv: -kv[1]["dur"]):
        print("%-60s %6d %9.1f %9.1f %7.1f%% %7.1f%% %6s %6s %7s" % (
            name, g["n"], g["dur"] / g["n"] / 1e3, g["dur"] / nviews / 1e3, 100.0 * g["beside"] / max(g["dur"], 1),
            100.0 * g["alone"] / max(g["dur"], 1), "/".join(sorted(g["wg"])), "/".join(sorted(g["vgpr"])),
            "/".join(sorted(g["lds"]))))
    chain = [n for n in agg if not is_blend(n)]
    fwd_chain = [n for n in chain if any(k in n for k in ("view_fwd", "sh_fwd", "db_", "radix_", "emit_kernel",
                                                           "tile_bins", "count_finish"))]
    for label, names in (("forward chain (view_fwd, count, SH forward, binning)", fwd_chain),
                         ("binning only (db_*, radix_*, emit, tile_bins)",
                          [n for n in fwd_chain if not any(k in n for k in ("view_fwd", "sh_fwd", "count_finish"))])):
        dur = sum(agg[n]["dur"] for n in names)
        bes = sum(agg[n]["beside"] for n in names)
        print("%-60s %6s %9s %9.1f %7.1f%%" % (label, "", "", dur / nviews / 1e3, 100.0 * bes / max(dur, 1)))
    # ---- per view: time without a blend kernel, and what ran then
    per_view = [covered(marks[i], marks[i + 1], no_blend, nb_starts) for i in range(nviews)]
    print()
    print("time with no blend kernel in flight, per view: mean %.1f us, min %.1f, max %.1f (%.1f %% of the window)" %
          (sum(per_view) / nviews / 1e3, min(per_view) / 1e3, max(per_view) / 1e3,
           100.0 * sum(per_view) / (w1 - w0)))
    print("  kernels running in that time (us per view; they may overlap each other):")
    for name, g in sorted(agg.items(), key=lambda kv: -kv[1]["alone"]):
        if g["alone"] * 200 >= sum(per_view) and not is_blend(name):
            print("    %-60s %8.1f" % (name, g["alone"] / nviews / 1e3))
    idle = (w1 - w0) - sum(u[1] - u[0] for u in any_kernel)
    print("GPU fully idle (no kernel of either stream in flight): %.1f us per view (%.1f %% of the window)" %
          (idle / nviews / 1e3, 100.0 * idle / (w1 - w0)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
