#!/usr/bin/env python3
"""bench.py -- edge-Jacobians/s per Gauss-Newton iteration on a synthetic SE(2) pose graph.

    python bench.py --gpus N --steps K --warmup W [--config C4] [--iters 20] [--dump-outputs DIR] [--full]

A *step* is one ``optimize(20)`` call of the hot path (what the reference runs per accepted loop
closure: src/sparse_gslam/src/submap_loop_closer.cpp:286-287) from the same initial poses, i.e.
20 x { chi2, linearise + assemble, PCG solve, pose update } over all E edges.  ``value`` =
steps x iters x E / time = edge-Jacobian evaluations per second per GN iteration, with the graph
(structure + edge arrays) already resident in HBM when the timed region starts; the only upload in
the timed region is the 24*V-byte pose reset at the start of each step.

N > 1: launched by ``python -m torch.distributed.run``; one rank per GPU, libsgo's own RCCL communicator.  Every rank
marshals the same graph; in row-owner mode (graphs with spatially local closures, C4) a rank holds the Hessian blocks
and edge operands of its own contiguous range of rows only, does all level-0 work for these rows and exchanges boundary
rows + partial dot products in small all-gather packets; graphs whose rows are mostly boundary
rows (random closures) keep every rank's copy whole and all-reduce the product vectors.  Total work is fixed =>
"scaling": "strong".

A plain run sets up, warms up, times the K steps and prints the line: `value`, `ms_per_step` and what the last timed step
returned (chi2, PCG iterations, per-iteration times).  --dump-outputs DIR also writes what that step's caller receives:
DIR/poses.npy (the optimised poses), DIR/chi2.npy and DIR/robust_chi2.npy (every iterate), float64; the inputs are the
seeded generator's, the same in every run with the same arguments.

--full adds everything else the line has carried: `set_graph_ms` (median of 11 set-ups) and the set-up-inclusive figures,
`final_chi2_rel_err_vs_oracle` (the committed CPU-oracle fixture), `roofline` (median-based, recomputable from profiles/:
DESIGN.md section 4), `cpu_baseline`, `value_init_odom` (BASELINE.md's literal dead-reckoned start), `reference_usage_session`
(the reference's flow at its own graph size: the single-launch direct path) and `incremental_session` (the reference's flow
at the bench workload's size: sgo_update_graph_se2 per closure against a fresh sgo_set_graph_se2).  --no-roofline and
--no-cpu-baseline leave parts of it out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec ...
HBM_COPY_GBS = 6290.0  # ... and the copy rate measured there (frac_of_measured_copy)


def cpu_baseline(g, iters: int, config: str = ""):
    """CPU restatement of g2o's GN (not g2o itself: g2o / Eigen are not in the image) on the host cores, the three
    variants of SURVEY.md section 8(d), each on a BOUNDED sample of the workload:
    A  single thread, sparse direct LDL^T (the reference's solver class) on the sub-graph of the first 30 000
       poses -- the direct solver's cost is super-linear in the graph size (fill-in), so the rate on the sample
       is an UPPER bound of the rate on the full graph (`full_graph`: the full-size figure, read from the committed
       golden fixture's 'seconds' -- measured once while scripts/make_golden_large.py generated it);
    B  single thread, block-Jacobi PCG on the FULL graph: linearise + assemble, then a bounded number of PCG
       iterations; block-Jacobi PCG needs thousands of iterations per solve on these graphs (7 764 on C2, more
       than 20 000 on C4, profiles/r01_bj_c4_bench.json), so the figure is seconds per PCG iteration and the
       rate it bounds;
    C  the same on all host cores (OpenMP).
    `value` is variant A's rate (the fastest CPU path on graphs it can factorise)."""
    from oracle import c_oracle

    # ---- variant A on the WHOLE workload, on this box (round 6): symbolic analysis + two numeric
    # factorisations of the full graph in a CHILD process (a fresh interpreter that never touches the GPU), so that a graph whose
    # factorisation does not fit the budget can be given up: the child is killed at the limit and the line falls back to the
    # 30 000-pose sample below, saying so.
    full_here, full_why = None, None
    if g.V > 30_000 and g.meta.get("p_random", 0.0) == 0.0 and g.V <= 200_000 and config:
        import subprocess
        limit = float(os.environ.get("SGO_BENCH_CPU_FULL_LIMIT_S", "300"))
        code = ("import sys, json, time; sys.path.insert(0, %r)\n"
                "from oracle import c_oracle\nfrom sparse_gslam_amd import synth\n"
                "g = synth.config(%r)\nt = time.time()\n"
                "_, st = c_oracle.gauss_newton(*g.arrays(), iters=3, solver='direct')\n"
                "print(json.dumps(dict(seconds=[float(x) for x in st['seconds']], wall=time.time() - t, V=int(g.V), E=int(g.E), "
                "chi2=[float(x) for x in st['chi2']])))\n") % (ROOT, config)
        t0 = time.time()
        print(f"[bench] cpu baseline: variant A on the full graph in a child process (limit {limit:.0f} s)", file=sys.stderr, flush=True)
        try:
            r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=limit)
            if r.returncode == 0:
                full_here = json.loads(r.stdout.strip().splitlines()[-1])
            else:
                full_why = f"the full-graph run failed (exit {r.returncode}): {r.stderr.strip()[-200:]}"
        except subprocess.TimeoutExpired:
            full_why = f"the full-graph factorisation did not finish within {limit:.0f} s on this box (child killed)"
        print(f"[bench] cpu baseline, full graph: {time.time() - t0:.1f} s ({'ok' if full_here else full_why})", file=sys.stderr, flush=True)
    Vs = min(g.V, 30_000)
    keep = (g.ei < Vs) & (g.ej < Vs)
    args = (g.poses[:Vs], g.fixed[:Vs], g.ei[keep], g.ej[keep], g.meas[keep], g.info[keep], g.phi[keep])
    Es = int(keep.sum())
    _, st = c_oracle.gauss_newton(*args, iters=3, solver="direct")
    med = float(np.median(st["seconds"][1:]))   # iteration 0 also pays the symbolic analysis (once per optimize())
    # the FULL graph through the same solver: not timed here (13 min of CPU), read from the committed fixture the golden run left
    # (tests/golden/<config>_direct.npz 'seconds': per-iteration times of scripts/make_golden_large.py on the build container's cores)
    full = None
    gpath = os.path.join(ROOT, "tests", "golden", f"{config}_direct.npz")
    if config and Vs < g.V and os.path.exists(gpath):
        gf = np.load(gpath)
        if "seconds" in gf.files and gf["seconds"].size > 2:
            sec = float(np.median(gf["seconds"][1:]))
            full = {"V": g.V, "E": g.E, "seconds_per_gn_iter_median": sec, "value": g.E / sec, "unit": "edge-Jacobians/s per GN iter",
                    "source": os.path.relpath(gpath, ROOT) + "['seconds'] (measured when the fixture was generated, on the build "
                              "container's host, not on this box)"}
    try:
        ncores = len(os.sched_getaffinity(0))
    except AttributeError:
        ncores = os.cpu_count() or 1
    k_needed = 20000 if g.V >= 100_000 else 7764

    def timed(threads, maxit):
        r = c_oracle.pcg_timing(*g.arrays(), threads=threads, pcg_tol=1e-8, pcg_maxit=maxit)
        return r, r["seconds_pcg"] / max(r["pcg_iters"], 1)

    def entry(threads, r, per_it, extra=None):
        d = dict(threads=threads, seconds_linearize=r["seconds_linearize"], pcg_iterations_timed=r["pcg_iters"],
                 converged_within_sample=r["converged"], seconds_per_pcg_iteration=per_it,
                 sample=f"full graph, {r['pcg_iters']} PCG iterations",
                 rate_bound=dict(value=g.E / (r["seconds_linearize"] + k_needed * per_it), unit="edge-Jacobians/s per GN iter",
                                 assumes_pcg_iterations=k_needed,
                                 note="block-Jacobi PCG iterations per solve measured on the GPU path with the same "
                                      "preconditioner (lower bound where it did not converge)"))
        if extra:
            d.update(extra)
        return d

    variants = {}
    r, per_it = timed(1, 60)
    variants["B_pcg_1_thread"] = entry(1, r, per_it)
    # variant C: OpenMP over the host cores; a 3n-vector problem of this size stops scaling well before hundreds of
    # threads (and a container may see more cores than its quota grants), so a short sweep picks the thread count
    sweep = {}
    for th in sorted({t for t in (4, 8, 16, 32, 64, 128, ncores) if t <= ncores}):
        _, p_it = timed(th, 20)
        sweep[th] = p_it
    best = min(sweep, key=sweep.get)
    r, per_it = timed(best, 200)
    variants["C_pcg_openmp"] = entry(best, r, per_it, dict(host_cores=ncores, seconds_per_pcg_iteration_by_threads=sweep))
    if full_here:
        sec = float(np.median(full_here["seconds"][1:]))
        return dict(value=g.E / sec, unit="edge-Jacobians/s per GN iter", cores=1, kind="port", host_cores=ncores,
                    sample_V=g.V, sample_E=g.E, workload_V=g.V, workload_E=g.E,
                    sample=f"variant A on the WHOLE workload, timed on this box: CPU restatement of g2o GN (not g2o itself: g2o/Eigen "
                           f"are not in the image), single-thread C++ oracle, sparse direct LDL^T + min-degree ordering, all {g.V} poses / "
                           f"{g.E} edges, three Gauss-Newton iterations in a child process; value = E / median of iterations 2-3 "
                           f"(numeric factorisation + solve: {sec:.2f} s; iteration 1 with the symbolic analysis "
                           f"{full_here['seconds'][0]:.2f} s; whole child {full_here['wall']:.1f} s)",
                    seconds_per_gn_iter=[float(x) for x in full_here["seconds"]],
                    sample_30k=dict(V=Vs, E=Es, value=Es / med, note="the same solver on the first 30 000 poses (what rounds 1-5 reported as value)"),
                    full_graph=full, variants=variants)
    return dict(value=Es / med, unit="edge-Jacobians/s per GN iter", cores=1, kind="port", host_cores=ncores,
                sample_V=Vs, sample_E=Es, workload_V=g.V, workload_E=g.E, full_graph_here=full_why,
                sample=f"variant A: CPU restatement of g2o GN (not g2o itself: g2o/Eigen are not in the image): "
                       f"single-thread C++ oracle, sparse direct LDL^T + min-degree ordering, on the "
                       f"first {Vs} poses / {Es} edges of the workload (NOT the whole workload: sample_V / sample_E; the direct "
                       f"solver's cost is super-linear in the size, so this rate is an upper bound of the full graph's), median "
                       f"of GN iterations 2-3 (numeric factorisation + solve; symbolic analysis excluded)",
                full_graph=full, variants=variants)


def golden_rel_err(config, iters, st):
    """Relative error of the final chi2 against the committed CPU-oracle fixture of this workload
    (tests/golden/<config>_{direct,pcg}.npz: sparse direct LDL^T, or the oracle's PCG for graphs with random
    closures), None when there is no fixture for (config, iters)."""
    for kind in ("direct", "pcg"):
        path = os.path.join(ROOT, "tests", "golden", f"{config}_{kind}.npz")
        if os.path.exists(path):
            f = np.load(path)
            if int(f["iters"]) == iters:
                ref = float(f["chi2"][-1])
                return {"value": abs(st["chi2"][-1] - ref) / ref, "reference": f"{config}_{kind}.npz (CPU oracle, {kind})",
                        "bound": 1e-6}
    return None


def reference_usage_session(device: int, V: int = 1000, closures: int = 30):
    """The reference's own usage pattern at the reference's own size (slc.cpp:205-288): the graph grows along the
    trajectory and after every accepted closure the WHOLE graph is re-initialised and optimised with optimize(20).
    Latency per closure of libsgo (set_graph + optimize(20) + read-back; such graphs take the single-launch direct
    path) and of the CPU oracle (analysis + 20 x sparse LDL^T, one thread) on the same graphs."""
    from oracle import c_oracle
    from sparse_gslam_amd import capi, synth
    g = synth.manhattan(V, V - 1 + closures, seed=1, info_mode="full", init="odom", phi=10.0)
    odo, clo = np.arange(V - 1), np.arange(V - 1, g.E)
    clo = clo[np.argsort(np.maximum(g.ei[clo], g.ej[clo]))]
    pg, pc = g.poses.copy(), g.poses.copy()
    tg, tc, worst = [], [], 0.0
    desc = ""
    with capi.Optimizer(device) as opt:
        for k, c in enumerate(clo):
            last = int(max(g.ei[c], g.ej[c]))
            edges = np.concatenate([odo[:last], clo[: k + 1]])
            edges = edges[(g.ei[edges] <= last) & (g.ej[edges] <= last)]
            sl = slice(0, last + 1)
            a = lambda P: (P[sl], g.fixed[sl], g.ei[edges], g.ej[edges], g.meas[edges], g.info[edges], g.phi[edges])  # noqa: E731
            t = time.perf_counter()
            opt.set_graph(*a(pg))
            done, st = opt.optimize(20)
            pg[sl] = opt.get_poses()
            tg.append(time.perf_counter() - t)
            desc = opt.solver_description().split(":")[0]
            t = time.perf_counter()
            P, ost = c_oracle.gauss_newton(*a(pc), iters=20)
            pc[sl] = P
            tc.append(time.perf_counter() - t)
            if ost["chi2"][-1] > 1e-9:
                worst = max(worst, abs(st["chi2"][-1] - ost["chi2"][-1]) / ost["chi2"][-1])
    tg, tc = 1e3 * np.array(tg[1:]), 1e3 * np.array(tc[1:])      # the first call carries one-time initialisation
    return {"workload": f"manhattan chain of {V} poses, {closures} closures found along the way; optimize(20) after each",
            "solver": desc, "closures_timed": int(tg.size), "ms_per_closure_median": float(np.median(tg)),
            "ms_per_closure_mean": float(tg.mean()), "cpu_oracle_ms_per_closure_median": float(np.median(tc)),
            "cpu_oracle_ms_per_closure_mean": float(tc.mean()), "cpu_oracle_threads": 1,
            "final_chi2_rel_err_vs_oracle_max": worst}


def midsize_usage_session(device: int, name: str = "C3s", last_n: int = 25):
    """The same flow at the size of the reference's LARGEST graphs (mit-killian: 5 489 keyframe poses / 7 629 edges, C3s): the
    last `last_n` accepted closures of the run -- the graph up to each closure's later endpoint is re-initialised and optimised
    with optimize(20), as slc.cpp:286-287 does.  Such graphs take the multifrontal path: per closure the
    symbolic analysis + upload (sgo_set_graph_se2), 20 numeric factorisations + solves, the read-back; the CPU oracle beside it
    (its own analysis + 20 x sparse LDL^T, one thread)."""
    from oracle import c_oracle
    from sparse_gslam_amd import capi, synth
    g = synth.config(name)
    V = g.V
    odo, clo = np.arange(V - 1), np.arange(V - 1, g.E)
    clo = clo[np.argsort(np.maximum(g.ei[clo], g.ej[clo]), kind="stable")]
    pg, pc = g.poses.copy(), g.poses.copy()
    tg, tc, ts, worst, desc = [], [], [], 0.0, ""
    with capi.Optimizer(device) as opt:
        for k in range(len(clo) - last_n - 1, len(clo)):
            c = clo[k]
            last = int(max(g.ei[c], g.ej[c]))
            edges = np.concatenate([odo[:last], clo[: k + 1]])
            edges = edges[(g.ei[edges] <= last) & (g.ej[edges] <= last)]
            sl = slice(0, last + 1)
            a = lambda P: (P[sl], g.fixed[sl], g.ei[edges], g.ej[edges], g.meas[edges], g.info[edges], g.phi[edges])  # noqa: E731
            t = time.perf_counter()
            opt.set_graph(*a(pg))
            t1 = time.perf_counter()
            done, st = opt.optimize(20)
            pg[sl] = opt.get_poses()
            tg.append(time.perf_counter() - t)
            ts.append(t1 - t)
            desc = opt.solver_description().split(":")[0]
            t = time.perf_counter()
            P, ost = c_oracle.gauss_newton(*a(pc), iters=20)
            pc[sl] = P
            tc.append(time.perf_counter() - t)
            worst = max(worst, abs(st["chi2"][-1] - ost["chi2"][-1]) / ost["chi2"][-1])
    tg, tc, ts = 1e3 * np.array(tg[1:]), 1e3 * np.array(tc[1:]), 1e3 * np.array(ts[1:])   # the first call carries one-time initialisation
    return {"workload": f"{name}: the last {last_n} closures of the run (graphs of {int(max(g.ei[clo[-last_n]], g.ej[clo[-last_n]])) + 1} "
                        f"to {V} poses), sgo_set_graph_se2 + optimize(20) + read-back after each",
            "solver": desc, "closures_timed": int(tg.size), "ms_per_closure_median": float(np.median(tg)),
            "set_graph_ms_median": float(np.median(ts)), "cpu_oracle_ms_per_closure_median": float(np.median(tc)),
            "cpu_oracle_threads": 1, "final_chi2_rel_err_vs_oracle_max": worst}


def incremental_session(device: int, V: int, E: int, seed: int, steps: int = 12, chain: int = 25, iters: int = 20, compare: bool = True):
    """The reference's usage pattern at the BENCH workload's size (slc.cpp:205-226, :272-287): a resident graph of V poses /
    E edges, then `steps` accepted loop closures, each appending `chain` new poses with their odometry edges and one
    closure, re-initialising and running optimize(iters).  Through sgo_update_graph_se2 (the resident level-0 structure and
    multigrid hierarchy are kept, the appended part is an overlay: sparse_gslam_amd/csrc/sgo_overlay.h) against a fresh
    sgo_set_graph_se2 of the same arrays from the same initial poses on a second context: set-up and optimize() times, PCG
    iterations, and the worst relative chi2 difference over all iterates of all steps (bound 1e-6)."""
    from sparse_gslam_amd import capi, synth
    base, app, g = synth.append_session(V, E, steps, chain, seed)
    odom_meas = g.meas[: g.V - 1]
    arrs = [base.ei, base.ej, base.meas, base.info, base.phi]
    # The grown graph's arrays are allocated ONCE at their final size and filled in place, as a C++ caller's containers grow: up to
    # round 5 this loop made them anew per closure (np.concatenate: ~100 MB mapped and unmapped), and the driver's work behind the
    # munmap of a process with device queues landed on the next submission -- single updates of 15-35 ms, half of them in some runs
    # (scripts/update_outlier_probe.py).
    names = ("ei", "ej", "meas", "info", "phi")
    e_max = base.E + sum(len(a["ei"]) for a in app)
    bufs = [np.empty((e_max,) + x.shape[1:], dtype=x.dtype) for x in arrs]
    for b_, x in zip(bufs, arrs):
        b_[: base.E] = x
    pbuf, fbuf, ne = np.empty((app[-1]["V"], 3)), np.zeros(app[-1]["V"], dtype=bool), base.E
    fbuf[0] = True
    t_up, t_opt, t_set, t_fopt, its, fits, worst, descs = [], [], [], [], [], [], 0.0, []
    with capi.Optimizer(device) as inc, capi.Optimizer(device) as fresh:
        inc.set_graph(*base.arrays())
        d, st = inc.optimize(iters)
        P = inc.get_poses()
        E_res = base.E
        for k, a in enumerate(app):
            k_new = len(a["ei"])
            for b_, n in zip(bufs, names):
                b_[ne: ne + k_new] = a[n]
            ne += k_new
            arrs = [b_[:ne] for b_ in bufs]
            P0, fixed = pbuf[: a["V"]], fbuf[: a["V"]]
            P0[: P.shape[0]] = P
            synth.chain_init(P0, odom_meas, P.shape[0], a["V"] - 1)
            t = time.perf_counter()
            inc.update_graph(P0, fixed, *arrs, E_res)
            t1 = time.perf_counter()
            d, st = inc.optimize(iters)
            t2 = time.perf_counter()
            P = inc.get_poses()
            descs.append(inc.solver_description().split("; last update: ")[-1])
            t_up.append(1e3 * (t1 - t)); t_opt.append(1e3 * (t2 - t1)); its.append(float(np.mean(st["pcg_iters"])))
            if not compare:
                E_res = arrs[0].size
                continue
            t = time.perf_counter()
            fresh.set_graph(P0, fixed, *arrs)
            t1 = time.perf_counter()
            df, sf = fresh.optimize(iters)
            t2 = time.perf_counter()
            t_set.append(1e3 * (t1 - t)); t_fopt.append(1e3 * (t2 - t1)); fits.append(float(np.mean(sf["pcg_iters"])))
            if d == iters == df:
                worst = max(worst, max(abs(x - y) / y for x, y in zip(st["chi2"], sf["chi2"])),
                            max(abs(x - y) / y for x, y in zip(st["robust_chi2"], sf["robust_chi2"])))
            else:
                worst = float("nan")
            E_res = arrs[0].size
    med = lambda v: float(np.median(v)) if len(v) else None   # noqa: E731
    if not compare:
        return {"update_ms": [round(x, 3) for x in t_up], "optimize_ms_median": med(t_opt), "pcg_iters_per_gn_iter": its, "updates": descs}
    return {"workload": f"append_session(V={V}, E={E}, seed={seed}): {steps} closures, each {chain} new poses + odometry + 1 closure, "
                        f"optimize({iters}) after each",
            "update_ms_median": med(t_up), "update_ms_min_max": [float(min(t_up)), float(max(t_up))],
            # (both definitions, ADVICE round 5: the sum of the medians -- what rounds 4-5 reported -- and the median of the
            # per-closure sums; they differ when single updates are outliers, which the in-place arrays removed at the source:
            # update_ms_min_max)
            "optimize_ms_median": med(t_opt), "setup_plus_optimize_ms": med(t_up) + med(t_opt),
            "setup_plus_optimize_ms_median_of_sums": med([a + b for a, b in zip(t_up, t_opt)]),
            "fresh_setup_plus_optimize_ms_median_of_sums": med([a + b for a, b in zip(t_set, t_fopt)]),
            "pcg_iters_per_gn_iter": its,
            "fresh_set_graph_ms_median": med(t_set), "fresh_optimize_ms_median": med(t_fopt),
            "fresh_setup_plus_optimize_ms": med(t_set) + med(t_fopt), "fresh_pcg_iters_per_gn_iter": fits,
            "max_rel_chi2_diff_vs_fresh_setup": worst, "bound": 1e-6, "updates": descs}


def dump_outputs(path: str, poses, st):
    """What a caller of the timed path receives from the last timed step, as float64 .npy files: the optimised poses
    (sgo_get_poses, V x 3) and the chi2 / robust chi2 of every iterate of that optimize() call.  At most 24 MB (C5's 1M
    poses)."""
    os.makedirs(path, exist_ok=True)
    for name, a in (("poses", poses), ("chi2", st["chi2"]), ("robust_chi2", st["robust_chi2"])):
        np.save(os.path.join(path, name + ".npy"), np.asarray(a, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="C4")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--solver", default=None, help="pcg | amg (default: library default)")
    ap.add_argument("--tol", type=float, default=None)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: set-up time, the oracle fixture's chi2, the "
                         "dead-reckoned start, the roofline leg, the CPU baseline and the usage sessions")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (poses, chi2, robust chi2) as DIR/<name>.npy, float64")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline and usage sessions")
    ap.add_argument("--no-roofline", action="store_true", help="--full without the roofline leg, dead-reckoned start and incremental session")
    ap.add_argument("--transport", choices=("rccl", "host"), default="rccl",
                    help="N > 1 only.  rccl: one rank per GPU, libsgo's own RCCL communicator (the measured configuration).  host: the "
                         "same launcher, rendezvous, sharding, MAX-reduce and JSON with libsgo's caller-supplied transport "
                         "(sgo_comm_init_host + gloo) -- rank processes may then SHARE a GPU (rank r uses device r mod the number of "
                         "devices), which is how the --gpus N code path runs end to end on a box with one GPU; its value is a "
                         "functional check, not a scaling measurement, and the line says so")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with python -m torch.distributed.run")
        args.gpus = world

    import torch
    import torch.distributed as dist

    from sparse_gslam_amd import capi, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    host_transport = world > 1 and args.transport == "host"
    if host_transport:
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    if world > 1:
        dist.init_process_group("gloo" if host_transport else "nccl", rank=rank, world_size=world)
    red_dev = "cpu" if host_transport else "cuda"   # where the host layer's own small reductions live

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def note(msg):   # progress on stderr (a run that stays silent for minutes is taken to be hung by the GPU runner)
        if rank == 0:
            print(f"[bench] {msg}", file=sys.stderr, flush=True)

    note(f"generating {args.config}")
    synth.TRAJECTORY_FILE = os.path.join(ROOT, "tests", "golden", "ref_trajectories.npz")   # (C1i / C1a only: the fixture is the caller's)
    g = synth.config(args.config)   # every rank builds the same graph (deterministic generator)
    note(f"graph ready: V={g.V} E={g.E}")

    opts = {}
    if args.solver:
        opts["solver"] = dict(pcg=capi.SOLVER_PCG_BJ, bj=capi.SOLVER_PCG_BJ, amg=capi.SOLVER_PCG_AMG)[args.solver]
    if args.tol:
        opts["pcg_tol"] = args.tol
    opt = capi.Optimizer(local_rank, **opts)
    sharding = "single GPU"   # (N > 1: replaced by the library's own description of the mode it chose for this graph)
    if host_transport:
        def _allreduce(a):
            dist.all_reduce(torch.from_numpy(a))

        def _allgather(send, recv):
            parts = [torch.empty(send.size, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(parts, torch.from_numpy(send.copy()))
            for r, t in enumerate(parts):
                recv[r * send.size:(r + 1) * send.size] = t.numpy()

        opt.comm_init_host(world, rank, _allreduce, _allgather)
    elif world > 1 or os.environ.get("SGO_BENCH_FORCE_COMM"):
        # rendezvous for libsgo's own RCCL communicator: rank 0 makes the id, torch broadcasts it.  No
        # communicator, no multi-GPU number: a failure on any rank ends the run with a non-zero exit code
        # instead of silently benchmarking N replicas.
        uid = [capi.comm_unique_id() if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(uid, src=0)
        comm_error = None
        try:
            opt.comm_init(world, rank, uid[0])
        except capi.SgoError as e:
            comm_error = str(e)
        if world > 1:
            ok = torch.tensor([0 if comm_error else 1], dtype=torch.int32, device=red_dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 0:
                opt.close()
                dist.destroy_process_group()
                raise SystemExit(f"[bench] rank {rank}: RCCL communicator unavailable ({comm_error or 'failed on another rank'}); "
                                 "no multi-GPU measurement")
        elif comm_error:
            raise SystemExit(comm_error)
    opt.set_graph(*g.arrays())
    if world > 1:
        sharding = opt.solver_description().split("; multi-GPU ", 1)[-1]
    sg_ms = []                     # steady state of repeated calls (the reference re-initialises before every optimize(20)):
    if args.full:
        for _ in range(11):        # median of 11 -- host threads decide single samples
            t_sg = time.perf_counter()
            opt.set_graph(*g.arrays())
            sg_ms.append(1e3 * (time.perf_counter() - t_sg))
        set_graph_steady_ms = float(np.median(sg_ms))
        note(f"set_graph steady state {set_graph_steady_ms:.1f} ms")

    def step():
        opt.set_poses(g.poses)
        done, st = opt.optimize(args.iters)
        if done != args.iters:
            raise SystemExit(f"optimize stopped after {done} iterations: {st}")
        return st

    note("warm-up")
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    st = None
    for _ in range(args.steps):
        st = step()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())

    out = None
    if rank == 0:
        value = args.steps * args.iters * g.E / dt
        o = capi.default_opts()
        out = {
            "metric": "edge-Jacobians/sec per GN iter on SE(2) graph; final chi2 vs g2o",
            "value": value, "unit": "edge-Jacobians/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{args.config}: manhattan(V={g.V}, E={g.E}, seed={g.meta['seed']}, "
                                   f"p_random={g.meta['p_random']}), init={g.meta['init']}, "
                                   f"optimize({args.iters}) per step",
                       "closure_radius_m": g.meta.get("closure_radius"),
                       "generator_note": "closures between poses within closure_radius of each other (SURVEY 8(d) says <= 2 m; "
                                         "the generator widens the radius until E - V + 1 candidates exist: 3 m for C4); "
                                         "init=incremental is the state optimize(20) sees in the reference (slc.cpp:205-224); "
                                         "from a dead-reckoned start (init=odom) undamped GN + DCS does not converge: "
                                         "init_odom_probe below",
                       "V": g.V, "E": g.E, "gn_iters_per_step": args.iters,
                       "solver": opt.solver_description().split(":")[0],
                       "pcg_tol": opts.get("pcg_tol", o.pcg_tol),
                       "pcg_tol_cap": opts.get("pcg_tol_cap", o.pcg_tol_cap),
                       "pcg_stop_rule": "||r|| <= pcg_tol * max(||b||, min(||b_first||, pcg_tol_cap / pcg_tol * ||b||)): "
                                        "the absolute accuracy of the call's first solve, capped at pcg_tol_cap relative",
                       "parallelism": sharding,
                       "transport": ("host (sgo_comm_init_host + gloo; rank processes share GPUs: a functional run of the --gpus N "
                                     "path, NOT a scaling measurement)" if host_transport else
                                     ("rccl" if world > 1 else "none (single GPU)"))},
            "final_chi2": st["chi2"][-1], "final_robust_chi2": st["robust_chi2"][-1],
            "pcg_iters_per_gn_iter": float(np.mean(st["pcg_iters"])), "pcg_iters": st["pcg_iters"],
            "gn_iter_ms_median": 1e3 * float(np.median(st["seconds"])),
            "linearize_ms_median": 1e3 * float(np.median(st["seconds_linearize"])),
            # lagged refresh of the multigrid hierarchy's coarse operators (sgo_solve.cpp): how many solves of the last timed
            # optimize() call kept the operators of the solve before (every solve runs to pcg_tol on the current Hessian either way;
            # SGO_AMG_LAG=0 refreshes before every solve)
            "coarse_operator_refresh": (opt.solver_description().split("; last sgo_optimize_gn: ")[1].split(";")[0]
                                        if "; last sgo_optimize_gn: " in opt.solver_description() else "refreshed before every solve"),
        }
        if args.full:
            out["final_chi2_rel_err_vs_oracle"] = golden_rel_err(args.config, args.iters, st)
            out["set_graph_ms"] = set_graph_steady_ms   # host structure build + upload + multigrid set-up (not in value); median of 11 calls
            out["set_graph_ms_min_max"] = [float(min(sg_ms)), float(max(sg_ms))]
            # what one accepted loop closure costs in the reference's flow (slc.cpp:286-287: initializeOptimization +
            # optimize(20)): the second headline next to `value`
            out["setup_plus_optimize_ms"] = set_graph_steady_ms + 1e3 * dt / args.steps
            out["edge_jacobians_per_s_incl_setup"] = args.iters * g.E / (1e-3 * set_graph_steady_ms + dt / args.steps)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, opt.get_poses(), st)
    opt.close()

    note(f"timed region done: {1e3 * dt / args.steps:.1f} ms per step")
    if args.full and rank == 0 and world == 1 and not args.no_roofline and args.config in synth.CONFIGS and g.V <= 200_000:
        # BASELINE.md's dead-reckoned start on the same graph: PCG iterations per GN iteration and where the robust
        # chi2 goes over optimize(20) -- the evidence behind init=incremental as the bench workload
        go = synth.config(args.config, init="odom")
        with capi.Optimizer(local_rank, **opts) as po:
            po.set_graph(*go.arrays())
            po.optimize(args.iters)            # (a first pass: the timed one then runs at the clocks of a busy chip, as `value` does)
            po.set_graph(*go.arrays())
            odom_desc = po.solver_description()
            t_od = time.perf_counter()
            pd, ps = po.optimize(args.iters)
            t_od = time.perf_counter() - t_od
        # the BASELINE.md-literal workload ("dead-reckoned initial guess") as a second top-level number: `value` holds for
        # the near-converged start the reference's optimize(20) sees, this one for a start GN + DCS does not converge from
        out["value_init_odom"] = g.E / float(np.median(ps["seconds"][:max(pd, 1)]))
        out["init_odom_probe"] = {"iters_done": pd, "pcg_iters": ps["pcg_iters"][:max(pd, 1)],
                                  "robust_chi2_first": ps["robust_chi2"][0], "robust_chi2_last": ps["robust_chi2"][-1],
                                  "robust_chi2_min": min(ps["robust_chi2"]),
                                  "gn_iter_ms_median": 1e3 * float(np.median(ps["seconds"][:max(pd, 1)])),
                                  # the whole call, hierarchy rebuilds inside it included (the weights keep changing from this
                                  # start; DESIGN.md section 5 "filtered smoothing")
                                  "optimize_ms": 1e3 * t_od,
                                  "value_over_the_whole_call": (pd * g.E / t_od) if pd > 0 else None,
                                  "all_solves_converged": bool(pd == args.iters and all(ps["pcg_converged"][:pd])),
                                  "hierarchy_at_the_start": odom_desc.split("; direct path")[0],
                                  # this is the SECOND optimize() of this graph on the context (clocks of a busy chip,
                                  # as `value`); what the context learned in the first pass (lagged-refresh slope) carries over
                                  "pass": "second optimize() of this graph on a context that has already run it once"}
        # parity of this leg: the direct-solver fixture of THIS workload, both CPU oracles
        # (tests/golden/<config>_odom_direct.npz, scripts/make_golden_odom.py).  At C4 the two exact CPU solvers agree on the start
        # and are 8.5e-3 apart in chi2 after ONE step (the iteration is chaotic from this start at 10^5 poses): the GPU's distance
        # from the C++ oracle is printed next to the oracles' own distance from each other; what pins this leg is solver
        # independent (tests/test_gpu_golden.py::test_dead_reckoned_start_c4_...).
        opath = os.path.join(ROOT, "tests", "golden", f"{args.config}_odom_direct.npz")
        if os.path.exists(opath) and pd == args.iters:
            of = np.load(opath)
            if int(of["iters"]) == args.iters:
                rel = [abs(ps["chi2"][k] - of["chi2"][k]) / of["chi2"][k] for k in range(args.iters + 1)]
                out["init_odom_probe"]["chi2_vs_cpu_oracle"] = {
                    "reference": os.path.relpath(opath, ROOT), "iterates_the_two_cpu_oracles_agree_on_to_1e-6": int(of["agree"]),
                    "rel_diff_iterate_0": rel[0], "rel_diff_iterate_1": rel[1], "final_chi2_rel_diff": rel[-1],
                    "the_two_cpu_oracles_rel_diff_iterate_1": float(of["oracle_rel_diff"][1]),
                    "the_two_cpu_oracles_rel_diff_final": float(of["oracle_rel_diff"][-1]),
                    "the_two_cpu_oracles_rel_diff_max": float(np.max(of["oracle_rel_diff"]))}
    if args.full and rank == 0 and world == 1 and not args.no_roofline:
        note("roofline leg")
        # roofline leg: the same workload again with every launch bracketed by HIP events on the
        # context's stream (profile=1 disables the hipGraph so that single launches can be timed)
        popts = dict(opts)
        popts["profile"] = 1
        with capi.Optimizer(local_rank, **popts) as p:
            p.set_graph(*g.arrays())
            p.profile_reset()
            p.optimize(min(args.iters, 4))
            raw = p.kernel_profile(quantiles=True)
            overhead_us = 1e3 * p.profile_overhead_ms()
        prof = raw
        # dominant kernel: the kernel FUNCTION with the largest summed time (the three epilogue forms of the
        # level-0 product, k_spmv0t<mode, threads>, are one function body), reported through its most
        # expensive instantiation so that the name matches a row of the rocprofv3 summary
        fam = {}
        for n, v in prof.items():
            f = fam.setdefault(n.split("<")[0].split(" ")[0], {"ms": 0.0, "launches": 0, "bytes": 0.0, "members": []})
            f["ms"] += v["ms"]; f["launches"] += v["launches"]; f["bytes"] += v["bytes"]; f["members"].append(n)
        fname, fk = max(fam.items(), key=lambda kv: kv[1]["ms"])
        name, k = max(((n, prof[n]) for n in fk["members"]), key=lambda kv: kv[1]["ms"])
        import glob as _glob

        def kernel_roofline(kname):
            """per launch: algorithmic bytes / MEDIAN single-launch duration (profile mode reads the stop flag after every PCG
            iteration: no early-exit launch past convergence among the samples; the mean is reported beside it), the HBM
            traffic of the same kernel from the separate rocprofv3 --pmc passes (FETCH_SIZE x2, WRITE_SIZE;
            scripts/pmc_summary.py) and its median INSIDE the replayed hipGraph of a solve (working dispatches of a
            rocprofv3 --kernel-trace pass in graph mode: scripts/profile_round.sh -> scripts/trace_summary.py), both committed
            per round under profiles/"""
            kk = prof[kname]
            bpl = kk["bytes"] / kk["launches"]
            med = kk.get("median_us", 1e3 * kk["ms"] / kk["launches"])
            ach = bpl / (med * 1e-6) / 1e9
            tr, tr_src, ins = None, None, None
            # (both summaries record the hash of the kernel sources they were taken on: `..._current` says whether those are
            # the sources of the library this run loaded -- VERDICT round 5: "nothing checks it")
            sys.path.insert(0, os.path.join(ROOT, "scripts"))
            from pmc_summary import kernel_source_sha16
            now_sha = kernel_source_sha16()
            tr_cur = ins_cur = None
            for cand in sorted(_glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_traffic_{solver_name}_{args.config.lower()}.json"))):
                doc = json.load(open(cand))
                e = doc["kernels"].get(kname)
                if e:
                    tr, tr_src = e["hbm_bytes_per_launch"], os.path.relpath(cand, ROOT)
                    tr_cur = doc.get("kernel_source_sha16") == now_sha
            for cand in sorted(_glob.glob(os.path.join(ROOT, "profiles", f"r*_trace_summary_{args.config.lower()}_graph.json"))):
                doc = json.load(open(cand))
                e = doc["kernels"].get(kname)
                ins_cur = doc.get("kernel_source_sha16") == now_sha if e else ins_cur
                if e:
                    ins = {"median_us": e["median_us"], "p10_us": e["p10_us"], "p90_us": e["p90_us"],
                           "working_dispatches": e["working"], "dispatches": e["dispatches"],
                           "achieved": bpl / (e["median_us"] * 1e-6) / 1e9,
                           "frac": bpl / (e["median_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS,
                           "frac_of_measured_copy": bpl / (e["median_us"] * 1e-6) / 1e9 / HBM_COPY_GBS,
                           "source": os.path.relpath(cand, ROOT)}
            return {"kernel": kname, "achieved": ach, "frac": ach / HBM_PEAK_GBS, "frac_of_measured_copy": ach / HBM_COPY_GBS,
                    "traffic": tr, "traffic_source": tr_src, "traffic_over_algorithmic": (tr / bpl) if tr else None,
                    "traffic_source_taken_on_these_kernel_sources": tr_cur, "in_solve_source_taken_on_these_kernel_sources": ins_cur,
                    "median_launch_us": med, "p10_launch_us": kk.get("p10_us"), "p90_launch_us": kk.get("p90_us"),
                    "avg_launch_us": 1e3 * kk["ms"] / kk["launches"], "launches": kk["launches"],
                    "algorithmic_bytes_per_launch": bpl, "in_solve": ins}

        solver_name = {0: "bj", 1: "amg"}[opts.get("solver", capi.default_opts().solver)]
        dom = kernel_roofline(name)
        achieved, traffic, traffic_src, med_us, bytes_per_launch, in_solve = (dom["achieved"], dom["traffic"], dom["traffic_source"],
                                                                               dom["median_launch_us"], dom["algorithmic_bytes_per_launch"],
                                                                               dom["in_solve"])
        # the Hessian product of the solve (level 0, fp64 blocks) whatever the dominant kernel is: at C5's size HBM is its bound
        hp_name = next((n for n in ("k_spmv0t<0, 1024, false>", "k_spmv0<0>") if n in prof), None)
        # whole-iteration figure of SURVEY.md section 8(d): B_GN = B_lin + K B_pcg + 48 V over the median
        # GN iteration time, B_lin = 200 E + 72 V, B_pcg = 76 E + 430 V, K = PCG iterations per GN iteration
        K = float(np.mean(st["pcg_iters"]))
        b_gn = (200.0 * g.E + 72.0 * g.V) + K * (76.0 * g.E + 430.0 * g.V) + 48.0 * g.V
        t_gn = float(np.median(st["seconds"]))
        out["roofline"] = {
            "bound": "hbm", "kernel": name, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS, "frac_of_measured_copy": achieved / HBM_COPY_GBS, "measured_copy_GBs": HBM_COPY_GBS,
            "traffic": traffic, "traffic_source": traffic_src,
            "traffic_source_taken_on_these_kernel_sources": dom["traffic_source_taken_on_these_kernel_sources"],
            "in_solve_source_taken_on_these_kernel_sources": dom["in_solve_source_taken_on_these_kernel_sources"],
            "median_launch_us": med_us, "p10_launch_us": k.get("p10_us"), "p90_launch_us": k.get("p90_us"),
            "avg_launch_us": 1e3 * k["ms"] / k["launches"], "launches": k["launches"],
            "event_bracket_overhead_us": overhead_us,
            "algorithmic_bytes_per_launch": bytes_per_launch,
            "in_solve": in_solve,
            "level0_product": kernel_roofline(hp_name) if hp_name else None,
            "kernel_function": {"name": fname, "instantiations": sorted(fk["members"]), "launches": fk["launches"],
                                "ms": round(fk["ms"], 3), "avg_launch_us": 1e3 * fk["ms"] / fk["launches"],
                                "achieved": fk["bytes"] / (fk["ms"] * 1e-3) / 1e9,
                                "frac": fk["bytes"] / (fk["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS},
            "gn_iteration": {"bytes": b_gn, "seconds": t_gn, "pcg_iters": K, "achieved": b_gn / t_gn / 1e9,
                             "frac": b_gn / t_gn / 1e9 / HBM_PEAK_GBS, "frac_of_measured_copy": b_gn / t_gn / 1e9 / HBM_COPY_GBS},
            # share of the profiled kernel time spent in kernels that a rank of a multi-GPU run (row-owner mode)
            # evaluates for ITS rows only: level-0 products, linearisation, vector updates, level-0 transfers and the
            # level-0 part of the hierarchy refresh ("@level0" slots); the rest (coarse levels, dense inverse) is replicated
            "row_owner_sharded_frac": (lambda sh, tot: sh / tot if tot > 0 else None)(
                sum(v["ms"] for n, v in prof.items() if n.startswith(("k_spmv0", "k_linearize", "k_finalize", "k_update_", "k_dot", "k_chi2",
                                                                        "k_pose_update")) or n.endswith("@level0")),
                sum(v["ms"] for v in prof.values())),
            "note": "achieved = algorithmic bytes per launch (SURVEY.md section 8(d): every stored block once with one index, "
                    "76 B per edge, + the per-row vectors; DESIGN.md section 4) / the MEDIAN HIP-event duration of this "
                    "kernel's launches (no launch past convergence among them); the events are the dispatch's own start/stop stamps "
                    "(hipExtLaunchKernelGGL), comparable with rocprofv3 kernel durations; traffic = mean HBM "
                    "bytes per launch from rocprofv3 --pmc passes; gn_iteration = B_GN / t_GN of section 8(d); "
                    "per-kernel table uses rocprofv3's kernel names",
            "kernels": {n: {"launches": v["launches"], "ms": round(v["ms"], 3),
                            "avg_us": round(1e3 * v["ms"] / v["launches"], 2),
                            "median_us": round(v.get("median_us", 0.0), 2), "p10_us": round(v.get("p10_us", 0.0), 2),
                            "p90_us": round(v.get("p90_us", 0.0), 2),
                            "GB/s": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1)}
                        for n, v in prof.items() if v["ms"] > 0}}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        note("cpu baseline")
        out["cpu_baseline"] = cpu_baseline(g, args.iters, args.config)
        out["reference_usage_session"] = reference_usage_session(local_rank)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and args.config == "C3s":
        note("mid-size usage session")
        out["midsize_usage_session"] = midsize_usage_session(local_rank, args.config)
    if args.full and rank == 0 and world == 1 and not args.no_roofline and args.config in ("C2", "C4"):
        note("incremental session")
        out["incremental_session"] = incremental_session(local_rank, g.V, g.E, g.meta["seed"], iters=args.iters)
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
