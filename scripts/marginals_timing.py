"""Time of sgo_marginals for the last pose's diagonal block (NOTES.md section 34): per config the first call on a context -- on a
graph that optimises through a factorisation path it builds the row plan and the multigrid hierarchy -- and the median of five warm
calls, a host clock around calls that end in a device synchronise; beside them the PCG iterations of the three unit columns
(sgo_solve_rhs) and of a Gauss-Newton solve at the same estimates.  The estimates are those of optimize(8) from the config's
initial poses.

C1i is the 1 051-pose graph on the reference's intel-lab trajectory (tests/golden/ref_trajectories.npz), which takes the
single-launch direct path; C1 and C3s take the multifrontal path, C2 and C4 the multigrid PCG.

--selected (NOTES.md section 35): sgo_marginals_selected with the diagonal blocks of ALL poses instead -- first call and median of
nine warm calls --, beside it one Gauss-Newton iteration of the same graph (the median of sgo_stats.seconds), sgo_marginals for 1,
8 and 64 vertices (warm medians), the vertex count at which the two routes cross (the selected inversion's time over sgo_marginals'
time per vertex, from the 8- and 64-vertex figures), and from a second, profiled context the new kernels' slots: milliseconds per
call and the median single launch.

usage: python scripts/marginals_timing.py [--selected] [C1i C1 C3s C2 C4]   -> one JSON line per config"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparse_gslam_amd import capi, synth  # noqa: E402

synth.TRAJECTORY_FILE = synth.TRAJECTORY_FILE or os.path.join(ROOT, "tests", "golden", "ref_trajectories.npz")


def run(name):
    g = synth.config(name)
    last = g.V - 1
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        path = opt.solver_description().split(":")[0]
        done, st = opt.optimize(8)
        t0 = time.perf_counter()
        cov = opt.marginals([last], [last])
        first = time.perf_counter() - t0
        warm = []
        for _ in range(5):
            t0 = time.perf_counter()
            again = opt.marginals([last], [last])
            warm.append(time.perf_counter() - t0)
        assert np.array_equal(cov, again) and opt.last_marginal_solves == 3
        b = opt.linearize()[0]
        gn_iters = opt.solve()[1]
        h = int(np.flatnonzero(opt.free_ids() == last)[0])
        col_iters = []
        for k in range(3):
            e = np.zeros_like(b)
            e[h, k] = 1.0
            col_iters.append(opt.solve_rhs(e)[1])
    return dict(config=name, V=g.V, E=g.E, path=path, gn_iterations_done=done, optimize_pcg_iters=st["pcg_iters"][:done],
                first_call_ms=1e3 * first, warm_call_ms_median=1e3 * float(np.median(warm)), warm_call_ms=[1e3 * w for w in warm],
                pcg_iters_per_column=col_iters, pcg_iters_gn_solve=gn_iters, sigma_diag=np.diag(cov[0]).tolist())


def _warm(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


SLOTS = ("k_mf_edges + k_mf_merge + k_mf_panels (multifrontal factor phase)", "k_si_gather", "k_si_panels", "k_si_result")


def run_selected(name):
    g = synth.config(name)
    free = np.flatnonzero(~g.fixed)
    pick = {k: free[np.linspace(0, free.size - 1, k).astype(int)] for k in (1, 8, 64)}
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        path = opt.solver_description().split(":")[0]
        done, st = opt.optimize(8)
        t0 = time.perf_counter()
        D, _ = opt.marginals_selected()
        first = 1e3 * (time.perf_counter() - t0)
        fronts = opt.last_selected_fronts
        sel = _warm(lambda: opt.marginals_selected(), 9)
        opt.marginals(pick[1], pick[1])      # (the first call builds the PCG structures of a graph on a factorisation path)
        marg = {k: _warm(lambda v=v: opt.marginals(v, v), 5) for k, v in pick.items()}
        old = opt.marginals(pick[64], pick[64])
    scale = np.sqrt(np.abs(D[pick[64]]).max(axis=(1, 2)) ** 2)
    agree = float((np.abs(D[pick[64]] - old).max(axis=(1, 2)) / scale).max())
    with capi.Optimizer(0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.optimize(8)
        opt.marginals_selected()
        opt.profile_reset()
        for _ in range(9):
            opt.marginals_selected()
        prof = opt.kernel_profile(quantiles=True)
    per_vertex = (marg[64] - marg[8]) / 56.0
    return dict(config=name, V=g.V, E=g.E, path=path, fronts=fronts, gn_iteration_ms=1e3 * float(np.median(st["seconds"][:done])),
                selected_first_call_ms=first, selected_warm_ms=sel, marginals_warm_ms=marg, marginals_ms_per_vertex=per_vertex,
                crossover_vertices=sel / per_vertex, selected_over_gn_iteration=sel / (1e3 * float(np.median(st["seconds"][:done]))),
                worst_disagreement_on_64=agree,
                kernels={k: dict(ms_per_call=prof[k]["ms"] / 9.0, launches_per_call=prof[k]["launches"] / 9.0,
                                 median_launch_us=prof[k].get("median_us")) for k in SLOTS if k in prof})


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--selected"]
    if "--selected" in sys.argv[1:]:
        for name in args or ["C1i", "C1", "C3s"]:
            print(json.dumps(run_selected(name)), flush=True)
    else:
        for name in args or ["C1i", "C1", "C3s", "C2", "C4"]:
            print(json.dumps(run(name)), flush=True)
