"""Time of sgo_marginals for the last pose's diagonal block (NOTES.md section 34): per config the first call on a context -- on a
graph that optimises through a factorisation path it builds the row plan and the multigrid hierarchy -- and the median of five warm
calls, a host clock around calls that end in a device synchronise; beside them the PCG iterations of the three unit columns
(sgo_solve_rhs) and of a Gauss-Newton solve at the same estimates.  The estimates are those of optimize(8) from the config's
initial poses.

C1i is the 1 051-pose graph on the reference's intel-lab trajectory (tests/golden/ref_trajectories.npz), which takes the
single-launch direct path; C1 and C3s take the multifrontal path, C2 and C4 the multigrid PCG.

usage: python scripts/marginals_timing.py [C1i C1 C3s C2 C4]   -> one JSON line per config"""
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


if __name__ == "__main__":
    for name in sys.argv[1:] or ["C1i", "C1", "C3s", "C2", "C4"]:
        print(json.dumps(run(name)), flush=True)
