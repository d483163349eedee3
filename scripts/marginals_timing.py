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

--candidates (NOTES.md section 36): sgo_candidate_gate for 1, 5, 16, 64 and 256 candidate closures -- revisits of the true
trajectory that are not edges of the graph, measured with noise, at the estimates of optimize(8); first call and median of nine warm
calls --, beside it, in the same session, the only other way to the same numbers: sgo_marginals for the candidates' Sigma_ii,
Sigma_jj and Sigma_ij (six solves per candidate), one Gauss-Newton iteration of the same graph, and from a second, profiled context
the four kernels' slots for the 5- and the 256-candidate call.

usage: python scripts/marginals_timing.py [--selected | --candidates] [C1i C1 C3s C2 C4]   -> one JSON line per config"""
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


FS_SLOTS = (SLOTS[0], "k_fs_rhs", "k_fs_forward", "k_fs_backward", "k_fs_gate")
COUNTS = (1, 5, 16, 64, 256)


def _closure_candidates(g, k, seed=9):
    rng = np.random.default_rng(seed)
    truth = g.truth if g.truth is not None else g.poses
    ci, cj, _ = synth._closure_candidates(truth, 100000, 2.0, 10)
    own = set(zip(g.ei.tolist(), g.ej.tolist())) | set(zip(g.ej.tolist(), g.ei.tolist()))
    keep = np.array([(a, b) not in own and not (g.fixed[a] and g.fixed[b]) for a, b in zip(ci.tolist(), cj.tolist())])
    ci, cj = ci[keep], cj[keep]
    pick = rng.choice(ci.size, size=k, replace=ci.size < k)
    ci, cj = ci[pick].astype(np.int32), cj[pick].astype(np.int32)
    sig = np.array([0.05, 0.05, 0.02])
    meas = synth._rel(truth[ci], truth[cj]) + rng.standard_normal((k, 3)) * sig
    meas[:, 2] = synth._wrap(meas[:, 2])
    info = np.tile(np.array([1 / sig[0]**2, 0, 0, 1 / sig[1]**2, 0, 1 / sig[2]**2]), (k, 1))
    return ci, cj, meas, info


def run_candidates(name):
    g = synth.config(name)
    ci, cj, meas, info = _closure_candidates(g, max(COUNTS))
    gate = lambda opt, k: opt.candidate_gate(ci[:k], cj[:k], meas[:k], info[:k], 11.345)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        path = opt.solver_description().split(":")[0]
        done, st = opt.optimize(8)
        t0 = time.perf_counter()
        gate(opt, 1)
        first = 1e3 * (time.perf_counter() - t0)
        warm = {k: _warm(lambda k=k: gate(opt, k), 9) for k in COUNTS}
        npass = gate(opt, max(COUNTS))[0]
        opt.marginals(ci[:1], ci[:1])      # (the first call builds the PCG structures of a graph on a factorisation path)
        old = {k: _warm(lambda k=k: opt.marginals(np.r_[ci[:k], cj[:k], ci[:k]], np.r_[ci[:k], cj[:k], cj[:k]]), 3) for k in COUNTS[:3]}
    kernels = {}
    with capi.Optimizer(0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.optimize(8)
        for k in (5, 256):
            gate(opt, k)
            opt.profile_reset()
            for _ in range(9):
                gate(opt, k)
            prof = opt.kernel_profile(quantiles=True)
            kernels[k] = {s: dict(ms_per_call=prof[s]["ms"] / 9.0, launches_per_call=prof[s]["launches"] / 9.0,
                                  median_launch_us=prof[s].get("median_us")) for s in FS_SLOTS if s in prof}
    gn = 1e3 * float(np.median(st["seconds"][:done]))
    return dict(config=name, V=g.V, E=g.E, path=path, gn_iteration_ms=gn, gate_first_call_ms=first, gate_warm_ms=warm,
                marginals_route_warm_ms=old, gate_5_over_gn_iteration=warm[5] / gn, pass_of_256=npass, kernels=kernels)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a not in ("--selected", "--candidates")]
    if "--candidates" in sys.argv[1:]:
        for name in args or ["C1i", "C1", "C3s"]:
            print(json.dumps(run_candidates(name)), flush=True)
    elif "--selected" in sys.argv[1:]:
        for name in args or ["C1i", "C1", "C3s"]:
            print(json.dumps(run_selected(name)), flush=True)
    else:
        for name in args or ["C1i", "C1", "C3s", "C2", "C4"]:
            print(json.dumps(run(name)), flush=True)
