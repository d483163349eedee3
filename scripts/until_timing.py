#!/usr/bin/env python3
"""What sgo_optimize_gn_until saves and what until-mode costs (NOTES.md section 37), on the library of this checkout: per graph the
whole-call times of sgo_optimize_gn(20), sgo_optimize_gn_until(20, 0.0) (never stops: the cost of the mode), sgo_optimize_gn_until(20,
tol) with the k* it stops at, and sgo_optimize_gn(k*) (on the multifrontal path the difference of the last two is the tail of
launches that exit at once after the stop); then the reference's flow on the mid-size path, per closure sgo_update_graph_se2 +
optimise, with and without the stop.  Host clock around calls that end in a synchronise, the poses put back before every call, one
warm-up call, medians; every measurement twice ("round"), so that the run-to-run spread is on the page.  One JSON line per figure.
With --plain only sgo_optimize_gn(20) is timed: run that from a checkout of the commit to compare against, alternating with this one.
Usage: python scripts/until_timing.py [--plain] [--tol 1e-6] [--skip-c4]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_gslam_amd import capi, synth  # noqa: E402

GRAPHS = [("600/620", lambda: synth.manhattan(600, 620, seed=3, info_mode="full", phi=10.0), {}, 15),
          ("2500/3400", lambda: synth.manhattan(2500, 3400, seed=31, info_mode="full", phi=10.0), {}, 15),
          ("3000/12000", lambda: synth.manhattan(3000, 12000, seed=7, info_mode="full", phi=10.0), {"direct_rows": 0}, 9),
          ("C3s", lambda: synth.config("C3s"), {}, 15),
          ("C4", lambda: synth.config("C4"), {}, 5)]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(opt, poses, fn, reps):
    opt.set_poses(poses)
    fn()   # warm-up
    ts, r = [], None
    for _ in range(reps):
        opt.set_poses(poses)
        t = time.perf_counter()
        r = fn()
        ts.append(1e3 * (time.perf_counter() - t))
    ts.sort()
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), reps=reps), r


def per_graph(plain_only, tol, skip_c4):
    for name, make, opts, reps in GRAPHS:
        if skip_c4 and name == "C4":
            continue
        g = make()
        with capi.Optimizer(0, **opts) as opt:
            opt.set_graph(*g.arrays())
            path = opt.solver_description().split(":")[0]
            for rnd in range(2):
                t, r = timed(opt, g.poses, lambda: opt.optimize(20), reps)
                emit(graph=name, path=path, what="gn(20)", round=rnd, done=r[0], **t)
                if plain_only:
                    continue
                t, r = timed(opt, g.poses, lambda: opt.optimize_until(20, 0.0), reps)
                emit(graph=name, path=path, what="until(20, 0.0)", round=rnd, done=r[0], **t)
                t, r = timed(opt, g.poses, lambda: opt.optimize_until(20, tol), reps)
                k = r[0]
                emit(graph=name, path=path, what=f"until(20, {tol:g})", round=rnd, done=k, stop_reason=r[2], **t)
                t, r = timed(opt, g.poses, lambda: opt.optimize(k), reps)
                emit(graph=name, path=path, what="gn(k*)", round=rnd, done=r[0], **t)


def closure_flow(tol, closures=8, chain=25):
    base, steps, gg = synth.append_session(5489, 7629, closures, chain, seed=3, info_mode="full", phi=0.75)
    for mode in ("gn(20)", f"until(20, {tol:g})"):
        with capi.Optimizer(0) as opt:
            opt.set_graph(*base.arrays())
            opt.optimize(20)
            P, E_res, lat, done = opt.get_poses(), base.E, [], []
            for k in range(1, len(steps) + 1):
                parts = [base] + steps[:k]
                cat = lambda key: np.concatenate([getattr(p, key) if hasattr(p, key) else p[key] for p in parts])   # noqa: E731
                V = steps[k - 1]["V"]
                fixed = np.zeros(V, dtype=bool)
                fixed[: base.V] = base.fixed
                P0 = np.empty((V, 3))
                P0[: P.shape[0]] = P
                synth.chain_init(P0, gg.meas[: gg.V - 1], P.shape[0], V - 1)
                ei = cat("ei")
                t0 = time.perf_counter()
                opt.update_graph(P0, fixed, ei, cat("ej"), cat("meas"), cat("info"), cat("phi"), E_res)
                t1 = time.perf_counter()
                d = opt.optimize(20)[0] if mode == "gn(20)" else opt.optimize_until(20, tol)[0]
                t2 = time.perf_counter()
                lat.append((1e3 * (t1 - t0), 1e3 * (t2 - t1)))
                done.append(d)
                P, E_res = opt.get_poses(), ei.size
            path = opt.solver_description().split(":")[0]
        lat = lat[1:]   # (the first closure warms up)
        emit(what="closure flow", mode=mode, path=path, update_ms_median=round(sorted(a for a, _ in lat)[len(lat) // 2], 3),
             optimize_ms_median=round(sorted(b for _, b in lat)[len(lat) // 2], 3), iterations=done)


def main():
    args = sys.argv[1:]
    tol = float(args[args.index("--tol") + 1]) if "--tol" in args else 1e-6
    per_graph("--plain" in args, tol, "--skip-c4" in args)
    if "--plain" not in args:
        closure_flow(tol)


if __name__ == "__main__":
    main()
