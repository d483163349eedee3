#!/usr/bin/env python3
"""What Powell's dogleg costs beside Levenberg-Marquardt and Gauss-Newton (NOTES.md section 47), on the library of this checkout: per
graph the whole-call times of sgo_optimize_dogleg(8) and sgo_optimize_dogleg_pcg(8) beside sgo_optimize_lm(8) / sgo_optimize_lm_pcg(8)
and sgo_optimize_gn(8) from the same start, their trials, solves and host synchronisations, and the chi2 histories.  Graphs:
300 / 400 and 2500 / 3400 without kernels from tests/test_gpu_lm.py's perturbed starts, C3s and C2 from their own starts, C4 from the
dead-reckoned one (DCS: the no-op).
What one rejected trial costs: the first iteration alone, once from delta_0 = 1e4 (q trials, one solve) and once from the delta its
accepted trial ran with (one trial, one solve); the difference over q - 1 is a rejected trial with its share of the extra round.
Host clock around calls that end in a synchronise, the poses put back before every call, one warm-up call, medians.  One JSON line
per figure.
Usage: python scripts/dogleg_timing.py [--skip-large]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_gslam_amd import capi, synth  # noqa: E402

ITERS = 8


def perturbed(g, sigma, seed=1):
    rng = np.random.default_rng(seed)
    P = g.poses.copy()
    P[1:, 2] += rng.normal(0.0, sigma, g.V - 1)
    P[1:, :2] += rng.normal(0.0, sigma, (g.V - 1, 2))
    return P


def no_kernels(g):
    g.phi[:] = -1.0
    return g


GRAPHS = [("300/400, sigma = 2.0", lambda: no_kernels(synth.manhattan(300, 400, seed=2, info_mode="full")), 2.0, 15),
          ("2500/3400, sigma = 1.0", lambda: no_kernels(synth.manhattan(2500, 3400, seed=31, info_mode="full")), 1.0, 15),
          ("C3s", lambda: synth.config("C3s"), 0.0, 15),
          ("C2", lambda: synth.config("C2"), 0.0, 5),
          ("C4 odom", lambda: synth.config("C4", init="odom"), 0.0, 3)]


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


def short(v, digits=6):
    return [float(f"{x:.{digits}g}") for x in v]


def report(opt, name, path, what, start, fn, reps, per):
    t, (rc, st) = timed(opt, start, fn, reps)
    if rc < 0:
        emit(graph=name, path=path, what=what, refused=opt.last_error())
        return None
    extra = {k: st[k] for k in ("trials", "step_kind", "solves", "sync_rounds", "stop_reason") if k in st}
    if "delta" in st:
        extra["delta"] = short(st["delta"], 4)
    if "pcg_iters" in st:
        extra["pcg_iters"] = [int(v) for v in st["pcg_iters"][:ITERS]]
    n = max(per(st), 1)
    emit(graph=name, path=path, what=what, done=rc, ms_per_unit=round(t["median_ms"] / n, 4), units=n, robust_chi2=short(st["robust_chi2"]),
         **extra, **t)
    return st


def main():
    for name, make, sigma, reps in GRAPHS:
        if "--skip-large" in sys.argv and name.startswith("C4"):
            continue
        g = make()
        start = perturbed(g, sigma) if sigma > 0 else g.poses
        with capi.Optimizer(0) as opt:
            opt.set_graph(*g.arrays())
            path = opt.solver_description().split(":")[0]
            factor = report(opt, name, path, f"dogleg({ITERS})", start, lambda: opt.optimize_dogleg(ITERS), reps, lambda st: st["solves"])
            report(opt, name, path, f"dogleg_pcg({ITERS})", start, lambda: opt.optimize_dogleg_pcg(ITERS), reps, lambda st: st["solves"])
            if factor is not None:
                report(opt, name, path, f"lm({ITERS})", start, lambda: opt.optimize_lm(ITERS), reps, lambda st: st["trials_total"])
            report(opt, name, path, f"lm_pcg({ITERS})", start, lambda: opt.optimize_lm_pcg(ITERS), reps, lambda st: st["trials_total"])
            report(opt, name, path, f"gn({ITERS})", start, lambda: opt.optimize(ITERS), reps, lambda st: ITERS)
            # one rejected trial: the first iteration from delta_0 = 1e4 and from the delta its accepted trial ran with
            for route, fn in (("dogleg", opt.optimize_dogleg), ("dogleg_pcg", opt.optimize_dogleg_pcg)):
                opt.set_poses(start)
                rc, st = fn(1)
                if rc != 1 or st["trials"][0] < 2:
                    continue
                q = st["trials"][0]
                accepted_at = 1e4 * 0.5 ** (q - 1)
                ta, _ = timed(opt, start, lambda: fn(1), reps)
                tb, (_, sb) = timed(opt, start, lambda: fn(1, accepted_at), reps)
                emit(graph=name, path=path, what=f"{route}(1): one rejected trial", trials=q, rounds=st["sync_rounds"], ms_with_rejections=ta["median_ms"],
                     ms_without=tb["median_ms"], trials_without=sb["trials"], ms_per_rejected_trial=round((ta["median_ms"] - tb["median_ms"]) / (q - 1), 4))


if __name__ == "__main__":
    main()
