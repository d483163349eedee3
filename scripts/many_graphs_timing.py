#!/usr/bin/env python3
"""What sgo_optimize_gn_many costs against the loop it replaces (NOTES.md section 51).

For n in {1, 16, 64, 256, 512} DISTINCT 600 / 620 graphs (seed = index) and for one mix of sizes from 100 to 6000 poses, each in
its own context: the whole-call time of
    many   sgo_optimize_gn_many(ctxs, n, 20, 0.0, stats, res, &launches)
    loop   for i: sgo_optimize_gn_until(ctxs[i], 20, 0.0, stats[i], &why)             (the route of the commit before)
on the same contexts of the same process, through ctypes with every output preallocated (no Python work per graph inside the
timed window beyond the loop's own call).  gain_tol 0: every graph runs its 20 iterations.  Before every timed call each context
gets its starting poses back (sgo_set_poses, outside the window), so both legs do the same work; the legs alternate, one
warm-up pair first, and the median, minimum and maximum of the repetitions are reported (host clock around calls that end in a
device synchronisation).  The legs' final poses are compared bit for bit once per case.

Writes one JSON document (--out, default profiles/many_graphs_timing.json) and a markdown table for NOTES.md (--md, default
stdout).  The one timing condition: at n = 64 the call must not be slower than the loop (median against median); exit code 1
with a line saying so otherwise.
Usage: python scripts/many_graphs_timing.py [--reps 15] [--max-n 512] [--out FILE] [--md FILE]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ARGS = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparse_gslam_amd import capi, synth  # noqa: E402

ITERS = 20
NS = (1, 16, 64, 256, 512)
# the mix: two graphs of every size, closures growing with the size (all on the single-launch path; the largest ones keep their
# right-hand side in global memory, so the call takes two launches)
MIX_SIZES = (100, 200, 400, 600, 800, 1000, 1500, 2000, 3000, 4000, 5000, 6000)


def arg(name, default):
    return type(default)(ARGS[ARGS.index(name) + 1]) if name in ARGS else default


def stats_of(ts):
    ts = sorted(ts)
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), reps=len(ts))


def measure(name, graphs, reps):
    L = capi.lib()
    n = len(graphs)
    opts = []
    for g in graphs:
        o = capi.Optimizer(0)
        o.set_graph(*g.arrays())
        opts.append(o)
    paths = [o.solver_description().split(":")[0].split(";")[0] for o in opts]
    handles = (C.c_void_p * n)(*[o._h for o in opts])
    stats = [capi.Stats() for _ in range(n)]
    sp = (C.POINTER(capi.Stats) * n)(*[C.pointer(s) for s in stats])
    res = (capi.ManyResult * n)()
    launches, why = C.c_int32(0), C.c_int32(0)

    def reset():
        for o, g in zip(opts, graphs):
            o.set_poses(g.poses)

    def many():
        t = time.perf_counter()
        rc = L.sgo_optimize_gn_many(handles, n, ITERS, 0.0, sp, res, C.byref(launches))
        dt = 1e3 * (time.perf_counter() - t)
        assert rc >= 0, (rc, L.sgo_last_error(handles[0]))
        return dt

    def loop():
        per = []
        t = time.perf_counter()
        for i in range(n):
            t1 = time.perf_counter()
            rc = L.sgo_optimize_gn_until(handles[i], ITERS, 0.0, sp[i], C.byref(why))
            per.append(1e3 * (time.perf_counter() - t1))
            assert rc >= 0, (i, rc, L.sgo_last_error(handles[i]))
        return 1e3 * (time.perf_counter() - t), max(per)

    # warm-up pair, and the results against each other
    reset()
    many()
    P = [o.get_poses() for o in opts]
    in_launch = sum(r.in_launch for r in res)
    reset()
    loop()
    same = all(np.array_equal(p.view(np.uint64), o.get_poses().view(np.uint64)) for p, o in zip(P, opts))
    tm, tl, slowest = [], [], []
    for _ in range(reps):
        reset()
        tm.append(many())
        reset()
        a, b = loop()
        tl.append(a)
        slowest.append(b)
    row = dict(case=name, n=n, iters=ITERS, paths=sorted(set(paths)), in_launch=in_launch, launches=launches.value, same_bits=bool(same),
               many=stats_of(tm), loop=stats_of(tl), slowest_single_call=stats_of(slowest), workspace_bytes=opts[0].many_workspace_bytes())
    row["speedup_median"] = round(row["loop"]["median_ms"] / row["many"]["median_ms"], 3)
    for o in opts:
        o.close()
    print(json.dumps(row), flush=True)
    return row


def main():
    reps = arg("--reps", 15)
    max_n = arg("--max-n", NS[-1])
    out = arg("--out", os.path.join(ROOT, "profiles", "many_graphs_timing.json"))
    md = arg("--md", "")
    pool = [synth.manhattan(600, 620, seed=1 + k, info_mode="full", phi=10.0) for k in range(min(max_n, NS[-1]))]
    rows = []
    for n in NS:
        if n <= max_n:
            rows.append(measure(f"{n} x 600/620", pool[:n], max(5, min(reps, 1280 // n))))
    mix = [synth.manhattan(V, V - 1 + min(8 + V // 100, 40), seed=100 + 2 * k + j, info_mode="full", phi=10.0)
           for k, V in enumerate(MIX_SIZES) for j in (0, 1)]
    rows.append(measure(f"mix of {len(mix)}: {MIX_SIZES[0]} .. {MIX_SIZES[-1]} poses", mix, reps))
    doc = dict(script="scripts/many_graphs_timing.py", iters=ITERS, gain_tol=0.0, rows=rows)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    lines = ["| graphs | in the launch / launches | one call: median (min .. max) ms | the loop: median (min .. max) ms | loop / call | slowest single call of the loop, median ms | same bits |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        m, lo = r["many"], r["loop"]
        lines.append(f"| {r['case']} | {r['in_launch']} / {r['launches']} | {m['median_ms']:.3f} ({m['min_ms']:.3f} .. {m['max_ms']:.3f}) | "
                     f"{lo['median_ms']:.3f} ({lo['min_ms']:.3f} .. {lo['max_ms']:.3f}) | {r['speedup_median']:.2f} | "
                     f"{r['slowest_single_call']['median_ms']:.3f} | {'yes' if r['same_bits'] else 'NO'} |")
    text = "\n".join(lines) + "\n"
    if md:
        with open(md, "w") as f:
            f.write(text)
    else:
        print(text)
    r64 = [r for r in rows if r["n"] == 64 and r["case"].startswith("64 x")]
    if r64 and r64[0]["many"]["median_ms"] > r64[0]["loop"]["median_ms"]:
        print(f"FINDING: at n = 64 the one call ({r64[0]['many']['median_ms']} ms) is slower than the loop it replaces ({r64[0]['loop']['median_ms']} ms)")
        return 1
    if not all(r["same_bits"] for r in rows):
        print("FINDING: the call's poses differ from the loop's")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
