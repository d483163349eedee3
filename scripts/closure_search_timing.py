"""Time of sgo_closure_search (NOTES.md section 48), per graph at the estimates of optimize(20), medians of 21 warm calls (a host
clock around calls that end in a device synchronise; the first call of each kind is left out):

  one_query_ms          the last pose against all V poses
  sixteen_queries_ms    16 queries spread over the trajectory against all V poses (48 columns: three panels)
  gate_all_pairs_ms     sgo_candidate_gate over the same V - 1 pairs (j, last pose) on the same build, measurement = the relative
                        pose of the estimates: three right-hand sides per pair where the search solves three per QUERY
  selected_diag_ms      sgo_marginals_selected(diag) alone: the factor phase and the selected inversion the search shares
  near / within         poses the search keeps at radius 2 m, chi2 6.635 (99 %, 1 degree of freedom) against poses within 2 m
  kernel                the search's slots of sgo_kernel_profile from a second, profiled context, for one query: ms per call,
                        launches per call, median launch

usage: python scripts/closure_search_timing.py [C3s 2500x3400 ...]   -> one JSON line per graph"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparse_gslam_amd import capi, synth  # noqa: E402

synth.TRAJECTORY_FILE = synth.TRAJECTORY_FILE or os.path.join(ROOT, "tests", "golden", "ref_trajectories.npz")
RADIUS, GATE, REPS = 2.0, 6.635, 21


def _warm(fn, reps=REPS):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def _graph(name):
    if "x" in name:
        V, E = (int(v) for v in name.split("x"))
        return synth.manhattan(V, E, seed=31, info_mode="full", phi=10.0)
    return synth.config(name)


def run(name):
    g = _graph(name)
    V = g.V
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        path = opt.solver_description().split(":")[0]
        done, st = opt.optimize(20)
        count, m2, rel, _, sg, near = opt.closure_search([V - 1], None, RADIUS, GATE)
        within = int((np.hypot(rel[0, :, 0], rel[0, :, 1]) <= RADIUS).sum()) - 1
        out = dict(graph=name, V=V, E=g.E, path=path, gn_iteration_ms=1e3 * float(np.median(st["seconds"][:done])), near=count, within=within,
                   median_sigma_lin_of_near=float(np.median(sg[0, near[0], 0])) if count else None)
        out["one_query_ms"] = _warm(lambda: opt.closure_search([V - 1], None, RADIUS, GATE))
        sixteen = np.linspace(V // 16, V - 1, 16).astype(np.int32)
        out["sixteen_queries_ms"] = _warm(lambda: opt.closure_search(sixteen, None, RADIUS, GATE))
        out["selected_diag_ms"] = _warm(lambda: opt.marginals_selected())
        P = opt.get_poses()
        ci = np.arange(V - 1, dtype=np.int32)
        cj = np.full(V - 1, V - 1, dtype=np.int32)
        meas = synth._rel(P[ci], P[cj])
        info = np.tile(np.array([400.0, 0, 0, 400.0, 0, 2500.0]), (V - 1, 1))
        out["gate_all_pairs_ms"] = _warm(lambda: opt.candidate_gate(ci, cj, meas, info, 11.345), 5)
    with capi.Optimizer(0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.optimize(20)
        opt.closure_search([V - 1], None, RADIUS, GATE)
        opt.profile_reset()
        for _ in range(REPS):
            opt.closure_search([V - 1], None, RADIUS, GATE)
        prof = opt.kernel_profile(quantiles=True)
    out["kernel"] = {k: dict(ms_per_call=v["ms"] / REPS, launches_per_call=v["launches"] / REPS, median_launch_us=v.get("median_us"))
                     for k, v in prof.items() if k.startswith(("k_closure", "k_si_", "k_fs_", "k_mf_edges + k_mf_merge"))}
    return out


if __name__ == "__main__":
    for name in sys.argv[1:] or ["C3s", "2500x3400"]:
        print(json.dumps(run(name)), flush=True)
