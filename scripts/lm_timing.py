#!/usr/bin/env python3
"""What a Levenberg-Marquardt attempt costs beside a Gauss-Newton iteration (NOTES.md section 45), on the library of this checkout:
per graph the whole-call time of sgo_optimize_lm(8) over its trials (one attempt = one trial: elements, factorisation of
H + lambda I, substitution, trial poses, chi2, decision) beside sgo_optimize_gn(8) over its iterations on the same graph from the
same start, the host synchronisations per LM call (sync_rounds), and both chi2 histories.  Graphs: 2500 / 3400 without kernels from
tests/test_gpu_lm.py's perturbed start (resident multifrontal plan), C3s from its own start, and the 150 000-pose dead-reckoned
graph of scripts/odom_sizes.py on which undamped Gauss-Newton blows up -- if the multifrontal analysis admits it; a refusal is
reported as such.  Host clock around calls that end in a synchronise, the poses put back before every call, one warm-up call,
medians.  One JSON line per figure.
Usage: python scripts/lm_timing.py [--skip-large]"""
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


GRAPHS = [("2500/3400, sigma = 1.0", lambda: no_kernels(synth.manhattan(2500, 3400, seed=31, info_mode="full")), 1.0, 15),
          ("C3s", lambda: synth.config("C3s"), 0.0, 15),
          ("150000/900000 odom, full, phi = 10", lambda: synth.manhattan(150000, 900000, seed=10, init="odom", info_mode="full", phi=10.0), 0.0, 3)]


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


def main():
    for name, make, sigma, reps in GRAPHS:
        if "--skip-large" in sys.argv and name.startswith("150000"):
            continue
        g = make()
        start = perturbed(g, sigma) if sigma > 0 else g.poses
        with capi.Optimizer(0) as opt:
            opt.set_graph(*g.arrays())
            path = opt.solver_description().split(":")[0]
            opt.set_poses(start)
            rc, st = opt.optimize_lm(ITERS)
            if rc < 0:
                emit(graph=name, path=path, what="lm", refused=opt.last_error())
                t, r = timed(opt, start, lambda: opt.optimize(ITERS), reps)
                emit(graph=name, path=path, what=f"gn({ITERS})", done=r[0], robust_chi2=[float(f"{v:.6g}") for v in r[1]["robust_chi2"]], **t)
                continue
            t, r = timed(opt, start, lambda: opt.optimize_lm(ITERS), reps)
            st = r[1]
            emit(graph=name, path=path, what=f"lm({ITERS})", done=r[0], trials=st["trials"], sync_rounds=st["sync_rounds"],
                 stop_reason=st["stop_reason"], ms_per_attempt=round(t["median_ms"] / max(st["trials_total"], 1), 4),
                 robust_chi2=[float(f"{v:.6g}") for v in st["robust_chi2"]], lam=[float(f"{v:.4g}") for v in st["lam"]], **t)
            t, r = timed(opt, start, lambda: opt.optimize(ITERS), reps)
            emit(graph=name, path=path, what=f"gn({ITERS})", done=r[0], ms_per_iteration=round(t["median_ms"] / ITERS, 4),
                 robust_chi2=[float(f"{v:.6g}") for v in r[1]["robust_chi2"]], **t)


if __name__ == "__main__":
    main()
