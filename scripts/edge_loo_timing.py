"""Time of sgo_edge_leave_one_out (NOTES.md section 42), per graph at the estimates of optimize(20), medians of nine warm calls
(a host clock around calls that end in a device synchronise; the first call of each kind is left out):

  all_edges_ms          the call for all E edges
  selected_diag_ms      sgo_marginals_selected(diag) alone on the same build: the factor phase and the selected inversion the call shares
  selected_pairs_ms     sgo_marginals_selected with pairs = every edge (what a caller had to pull to the host before), and
  host_arithmetic_ms    the per-edge arithmetic it then had to redo there (numpy, batched over the edges: J Sigma J^T, Cholesky, eigh)
  loo_64_ms             the call for 64 closures
  hypotheses_64_ms      sgo_optimize_gn_hypotheses with 64 hypotheses, each switching one of those closures off (max_iters 20,
                        gain_tol 1e-4), and its route
  kernel                k_loo_edges' own slot of sgo_kernel_profile from a second, profiled context: ms per call, median launch

usage: python scripts/edge_loo_timing.py [C3s 2500x3400 ...]   -> one JSON line per graph"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import np_oracle as npo  # noqa: E402
from sparse_gslam_amd import capi, synth  # noqa: E402

synth.TRAJECTORY_FILE = synth.TRAJECTORY_FILE or os.path.join(ROOT, "tests", "golden", "ref_trajectories.npz")
GATE, MIN_RED, REPS = 11.345, 1e-3, 9


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


def host_arithmetic(g, P, D, Sij, w):
    """What the call replaces on the host once Sigma's blocks are there: every edge's P, then the closed forms, batched"""
    A, B = npo.edge_jacobians(P[g.ei], P[g.ej], g.meas)
    e = npo.edge_error(P[g.ei], P[g.ej], g.meas)
    O = npo.info_full(g.info)
    Q = A @ D[g.ei] @ A.transpose(0, 2, 1) + B @ D[g.ej] @ B.transpose(0, 2, 1) + A @ Sij @ B.transpose(0, 2, 1)
    Q = Q + B @ Sij.transpose(0, 2, 1) @ A.transpose(0, 2, 1)
    Pm = 0.5 * (Q + Q.transpose(0, 2, 1))
    G = np.linalg.cholesky(O)
    N = G.transpose(0, 2, 1) @ Pm @ G
    nu, Vv = np.linalg.eigh(0.5 * (N + N.transpose(0, 2, 1)))
    c = np.einsum("nji,nj->ni", Vv, np.einsum("nji,nj->ni", G, e))
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = np.sum(c * c / ((1.0 + (1.0 - w[:, None]) * nu) * (1.0 - w[:, None] * nu)), axis=1)
    return d2, 1.0 - w * nu.max(axis=1)


def run(name):
    g = _graph(name)
    closures = np.flatnonzero(np.abs(g.ei.astype(np.int64) - g.ej) != 1)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        path = opt.solver_description().split(":")[0]
        done, st = opt.optimize(20)
        nfail, d2, red, _, _ = opt.edge_leave_one_out(None, GATE, MIN_RED)
        pick = closures[np.argsort(-red[closures])[:64]].astype(np.int32)
        out = dict(graph=name, V=g.V, E=g.E, path=path, gn_iteration_ms=1e3 * float(np.median(st["seconds"][:done])), fail=nfail,
                   bridges=int((~(red >= MIN_RED)).sum()))
        out["all_edges_ms"] = _warm(lambda: opt.edge_leave_one_out(None, GATE, MIN_RED))
        out["selected_diag_ms"] = _warm(lambda: opt.marginals_selected())
        out["selected_pairs_ms"] = _warm(lambda: opt.marginals_selected(g.ei, g.ej))
        D, Sij = opt.marginals_selected(g.ei, g.ej)
        P, w = opt.get_poses(), opt.edge_robust()[1]
        out["host_arithmetic_ms"] = _warm(lambda: host_arithmetic(g, P, D, Sij, w))
        h2, hred = host_arithmetic(g, P, D, Sij, w)
        ok = red >= 1e-2
        out["host_vs_device_d2"] = float(np.max(np.abs(h2[ok] - d2[ok]) / d2[ok]))
        out["loo_64_ms"] = _warm(lambda: opt.edge_leave_one_out(pick, GATE, MIN_RED))
        masks = np.zeros((pick.size, g.E), dtype=np.uint8)
        masks[np.arange(pick.size), pick] = 1
        hyp = lambda: opt.optimize_hypotheses(masks, 20, 1e-4, want=("edge_chi2",))
        out["hypotheses_route"] = int(hyp()["route"])
        out["hypotheses_64_ms"] = _warm(hyp, 3)
    with capi.Optimizer(0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.optimize(20)
        opt.edge_leave_one_out(None, GATE, MIN_RED)
        opt.profile_reset()
        for _ in range(REPS):
            opt.edge_leave_one_out(None, GATE, MIN_RED)
        prof = opt.kernel_profile(quantiles=True)
    out["kernel"] = {k: dict(ms_per_call=v["ms"] / REPS, launches_per_call=v["launches"] / REPS, median_launch_us=v.get("median_us"))
                     for k, v in prof.items() if k.startswith(("k_loo", "k_si_", "k_mf_edges + k_mf_merge"))}
    return out


if __name__ == "__main__":
    for name in sys.argv[1:] or ["C3s", "2500x3400"]:
        print(json.dumps(run(name)), flush=True)
