#!/usr/bin/env python3
"""What a Levenberg-Marquardt attempt costs beside a Gauss-Newton iteration (NOTES.md sections 45 and 46), on the library of this
checkout: per graph the whole-call time of sgo_optimize_lm(8) over its trials (one attempt = one trial: elements, factorisation of
H + lambda I, substitution, trial poses, chi2, decision) beside sgo_optimize_gn(8) over its iterations on the same graph from the
same start, the host synchronisations per LM call (sync_rounds), and both chi2 histories.  Graphs: 2500 / 3400 without kernels from
tests/test_gpu_lm.py's perturbed start (resident multifrontal plan), C3s from its own start, and the graphs the multifrontal
analysis refuses, which take sgo_optimize_lm_pcg (one trial: linearisation, the hierarchy refreshed for H + lambda I, a cold PCG
solve, trial poses, chi2, decision; PCG iterations per trial from sgo_lm_pcg_trace): C2, C4 from the dead-reckoned start, and the two
graphs of scripts/odom_sizes.py on which undamped Gauss-Newton blows up (150 000 / 900 000 and 200 000 / 2 000 000, full
information, phi = 10).  A library without sgo_optimize_lm_pcg (the parent commit's) reports the refusal and the Gauss-Newton
figures.  Host clock around calls that end in a synchronise, the poses put back before every call, one warm-up call, medians.  One
JSON line per figure.
--profile (PCG-route graphs only): one sgo_optimize_lm_pcg(8) on a profiling context, the per-kernel event times summed into what the
hierarchy's refresh (amg_update's kernels), the linearisation and the rest cost per trial.
Usage: python scripts/lm_timing.py [--skip-large] [--pcg-only] [--profile]"""
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
          ("C2", lambda: synth.config("C2"), 0.0, 7),
          ("C4 odom", lambda: synth.config("C4", init="odom"), 0.0, 3),
          ("150000/900000 odom, full, phi = 10", lambda: synth.manhattan(150000, 900000, seed=10, init="odom", info_mode="full", phi=10.0), 0.0, 3),
          ("200000/2000000 odom, full, phi = 10", lambda: synth.manhattan(200000, 2000000, seed=7, init="odom", info_mode="full", phi=10.0), 0.0, 3)]
FACTOR_ROUTE = 2   # the first graphs take sgo_optimize_lm; the rest are refused by it


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


# amg_update's kernels by their profile names (sgo_kernels.hip: kKernelNames), with or without " @level0"
REFRESH = ("k_positions0", "k_centres", "k_galerkin", "k_level_dinv", "k_gj_step", "k_p_values", "k_block_products", "k_ptilde_values")


def profile_refresh(name, g, start):
    with capi.Optimizer(0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(start)
        opt.optimize_lm_pcg(ITERS)   # warm-up
        opt.set_poses(start)
        opt.profile_reset()
        rc, st = opt.optimize_lm_pcg(ITERS)
        prof = opt.kernel_profile()
    n = max(st["trials_total"], 1)
    refresh = sum(v["ms"] for k, v in prof.items() if k.startswith(REFRESH))
    lin = sum(v["ms"] for k, v in prof.items() if k.startswith(("k_linearize", "k_finalize")))
    total = sum(v["ms"] for v in prof.values())
    emit(graph=name, what=f"lm_pcg({ITERS}) profile", trials=st["trials"], pcg_iterations=pcg_iterations(prof), event_ms_per_trial=round(total / n, 4),
         refresh_ms_per_trial=round(refresh / n, 4), linearize_finalize_ms_per_trial=round(lin / n, 4),
         refresh_launches_per_trial=round(sum(v["launches"] for k, v in prof.items() if k.startswith(REFRESH)) / n, 1))


def pcg_iterations(prof):
    return int(prof.get("k_update_p", {}).get("launches", 0))   # one k_update_p per PCG iteration


def main():
    for k, (name, make, sigma, reps) in enumerate(GRAPHS):
        if "--skip-large" in sys.argv and name[:6] in ("150000", "200000"):
            continue
        if "--pcg-only" in sys.argv and k < FACTOR_ROUTE:
            continue
        g = make()
        start = perturbed(g, sigma) if sigma > 0 else g.poses
        if "--profile" in sys.argv:
            if k >= FACTOR_ROUTE:
                profile_refresh(name, g, start)
            continue
        with capi.Optimizer(0) as opt:
            opt.set_graph(*g.arrays())
            path = opt.solver_description().split(":")[0]
            opt.set_poses(start)
            rc, st = opt.optimize_lm(ITERS)
            if rc < 0:
                emit(graph=name, path=path, what="lm", refused=opt.last_error())
                if hasattr(opt, "optimize_lm_pcg"):
                    t, r = timed(opt, start, lambda: opt.optimize_lm_pcg(ITERS), reps)
                    st = r[1]
                    its, how = opt.lm_pcg_trace()
                    emit(graph=name, path=path, what=f"lm_pcg({ITERS})", done=r[0], trials=st["trials"], stop_reason=st["stop_reason"],
                         ms_per_trial=round(t["median_ms"] / max(st["trials_total"], 1), 4), pcg_iters=its.tolist(), solve_stop=how.tolist(),
                         robust_chi2=[float(f"{v:.6g}") for v in st["robust_chi2"]], lam=[float(f"{v:.4g}") for v in st["lam"]], **t)
                t, r = timed(opt, start, lambda: opt.optimize(ITERS), reps)
                emit(graph=name, path=path, what=f"gn({ITERS})", done=r[0], ms_per_iteration=round(t["median_ms"] / ITERS, 4),
                     pcg_iters=[int(v) for v in r[1]["pcg_iters"][:ITERS]], robust_chi2=[float(f"{v:.6g}") for v in r[1]["robust_chi2"]], **t)
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
