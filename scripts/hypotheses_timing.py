#!/usr/bin/env python3
"""What sgo_optimize_gn_hypotheses costs against the host loop it replaces (NOTES.md section 38): per graph and per number of
hypotheses B the whole-call time of the call (history and poses read back, no per-edge values) and of the loop { zero rows;
sgo_set_poses; sgo_optimize_gn_until; sgo_get_poses; the rows again } over the same hypotheses -- leave-one-out masks over the graph's
closures, repeated to make B rows, 20 iterations each (gain_tol 0: no hypothesis ends early) --, beside sgo_optimize_gn(20) and
sgo_optimize_gn_until(20, 0.0) of the same process.  Host clock around calls that end in a synchronise, one warm-up call, median of
15; one JSON line per figure.
With --loop the call itself is left out and nothing newer than sgo_optimize_gn_until is used: run that with --root pointing at a
checkout (built) of the commit to compare against, alternating with this one in one session.
At B = 1 the call is also timed with the history alone read back: what it costs beside the bare sgo_optimize_gn_until, which returns
no poses either.  --max-b N leaves the larger Bs out.
With --mfront the multifrontal leg runs instead (NOTES.md section 41): on 2 500 / 3 400 and C3s, for B = 16, 64, 256 and gain_tol 0 and
1e-6, the call on the batched route -- sgo_set_hypotheses_workspace(--budget-gib, default 16) -- against the same call on the
sequential route of the same context (a grant of 0), with the bytes one hypothesis takes and the chunk the grant gives; fewer
repetitions at the large Bs (640 / B, at least 3).
Usage: python scripts/hypotheses_timing.py [--loop | --mfront] [--root DIR] [--reps 15] [--round N] [--max-b N] [--budget-gib G]"""
import json
import os
import sys
import time

import numpy as np

ARGS = sys.argv[1:]
ROOT = ARGS[ARGS.index("--root") + 1] if "--root" in ARGS else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparse_gslam_amd import capi, synth  # noqa: E402

# (name, graph, Optimizer options, the Bs measured): the two single-launch graphs up to 512 hypotheses, C3s -- the sequential route,
# a full multifrontal call per hypothesis and no batching to show -- up to 64
GRAPHS = [("600/620", lambda: synth.manhattan(600, 620, seed=3, info_mode="full", phi=10.0), {}, (1, 2, 8, 64, 256, 512)),
          ("1000/1030", lambda: synth.manhattan(1000, 1030, seed=3, info_mode="full", phi=10.0), {}, (1, 2, 8, 64, 256, 512)),
          ("C3s", lambda: synth.config("C3s"), {}, (1, 2, 8, 64))]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps):
    fn()   # warm-up
    ts, r = [], None
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        ts.append(1e3 * (time.perf_counter() - t))
    ts.sort()
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), reps=reps), r


def host_loop(opt, g, masks):
    resident = g.poses
    zero = np.zeros((1, 6))
    done = []
    for off in masks:
        ids = np.flatnonzero(off).astype(np.int32)
        if ids.size:
            opt.set_edge_information(ids, np.repeat(zero, ids.size, axis=0))
        opt.set_poses(resident)
        done.append(opt.optimize_until(20, 0.0)[0])
        opt.get_poses()
        if ids.size:
            opt.set_edge_information(ids, g.info[ids])
    opt.set_poses(resident)
    return done


MFRONT_GRAPHS = [("2500/3400", lambda: synth.manhattan(2500, 3400, seed=31, info_mode="full", phi=10.0)),
                 ("C3s", lambda: synth.config("C3s"))]


def mfront_leg(reps, rnd, max_b):
    budget = int(float(ARGS[ARGS.index("--budget-gib") + 1]) * 2 ** 30) if "--budget-gib" in ARGS else 16 << 30
    for name, make in MFRONT_GRAPHS:
        g = make()
        clo = np.arange(g.V - 1, g.E)
        with capi.Optimizer(0) as opt:
            opt.set_graph(*g.arrays())
            path = opt.solver_description().split(":")[0]
            per = opt.hypotheses_bytes(20, False)
            emit(graph=name, path=path, round=rnd, what="bytes per hypothesis", bytes=per, V=int(g.V), E=int(g.E))
            t, r = timed(lambda: (opt.set_poses(g.poses), opt.optimize_until(20, 0.0))[1], reps)
            emit(graph=name, path=path, round=rnd, what="until(20, 0.0)", done=r[0], **t)
            opt.set_poses(g.poses)   # every hypothesis starts from the graph's own poses, not from the optimum the call above left
            for tol in (0.0, 1e-6):
                for B in [b for b in (16, 64, 256) if b <= max_b]:
                    masks = np.zeros((B, g.E), dtype=np.uint8)
                    masks[np.arange(B), clo[np.arange(B) % clo.size]] = 1
                    n = max(3, min(reps, 640 // B))
                    row = {}
                    for route, grant in (("batched", budget), ("sequential", 0)):
                        opt.set_hypotheses_workspace(grant)
                        t, r = timed(lambda: opt.optimize_hypotheses(masks, 20, tol, want=("hist", "poses")), n)
                        row[route] = t["median_ms"]
                        emit(graph=name, path=path, round=rnd, what="hypotheses", B=B, gain_tol=tol, grant=grant,
                             chunk=capi.hypotheses_chunk(per, grant, B), route=int(r["route"]), done_min=int(r["iters_done"].min()),
                             done_mean=float(r["iters_done"].mean()), **t)
                    emit(graph=name, path=path, round=rnd, what="sequential / batched", B=B, gain_tol=tol,
                         ratio=round(row["sequential"] / row["batched"], 2))


def main():
    loop_only = "--loop" in ARGS
    reps = int(ARGS[ARGS.index("--reps") + 1]) if "--reps" in ARGS else 15
    rnd = int(ARGS[ARGS.index("--round") + 1]) if "--round" in ARGS else 0
    max_b = int(ARGS[ARGS.index("--max-b") + 1]) if "--max-b" in ARGS else 1 << 30
    if "--mfront" in ARGS:
        return mfront_leg(reps, rnd, max_b)
    lib = "loop-only library" if loop_only else "this library"
    for name, make, opts, Bs in GRAPHS:
        g = make()
        clo = np.arange(g.V - 1, g.E)
        with capi.Optimizer(0, **opts) as opt:
            opt.set_graph(*g.arrays())
            path = opt.solver_description().split(":")[0]

            def reset_then(fn):
                opt.set_poses(g.poses)
                return fn()

            t, r = timed(lambda: reset_then(lambda: opt.optimize(20)), reps)
            emit(graph=name, path=path, lib=lib, round=rnd, what="gn(20)", done=r[0], **t)
            t, r = timed(lambda: reset_then(lambda: opt.optimize_until(20, 0.0)), reps)
            emit(graph=name, path=path, lib=lib, round=rnd, what="until(20, 0.0)", done=r[0], **t)
            for B in [b for b in Bs if b <= max_b]:
                masks = np.zeros((B, g.E), dtype=np.uint8)
                masks[np.arange(B), clo[np.arange(B) % clo.size]] = 1
                if not loop_only:
                    t, r = timed(lambda: opt.optimize_hypotheses(masks, 20, 0.0, want=("hist", "poses")), reps)
                    emit(graph=name, path=path, lib=lib, round=rnd, what="hypotheses", B=B, route=int(r["route"]),
                         done_min=int(r["iters_done"].min()), **t)
                    if B == 1:
                        t, r = timed(lambda: opt.optimize_hypotheses(masks, 20, 0.0, want=("hist",)), reps)
                        emit(graph=name, path=path, lib=lib, round=rnd, what="hypotheses, history only", B=B, route=int(r["route"]),
                             done_min=int(r["iters_done"].min()), **t)
                t, r = timed(lambda: host_loop(opt, g, masks), reps)
                emit(graph=name, path=path, lib=lib, round=rnd, what="host loop", B=B, done_min=int(min(r)), **t)


if __name__ == "__main__":
    main()
