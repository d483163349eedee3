#!/usr/bin/env python3
"""The reference's final clean-up (log_runner.cpp:182-204: chi2 gate at 11.345, removeEdge, initializeOptimization, optimize(20)) on a
graph with corrupted closures, two ways on the same library: (a) sgo_gate_edges + optimize(20) -- the edges are deactivated on the
device, every resident structure is kept --, (b) sgo_edge_chi2 + host filter + sgo_set_graph_se2 of the reduced arrays + optimize(20),
which is what a caller had to do before.  Medians over `reps` repetitions from the same state (the graph set up with all edges and
optimised once); prints one JSON line.
Usage: python scripts/gate_session.py [config=C4] [bad=200] [reps=5]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_gslam_amd import capi, synth  # noqa: E402

GATE = 11.345


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "C4"
    nbad = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    g = synth.config(name)
    rng = np.random.default_rng(0)
    n_odom = g.meta["n_odom"]
    bad = n_odom + rng.choice(g.E - n_odom, size=nbad, replace=False)
    g.meas[bad, :2] += rng.normal(0, 3.0, (nbad, 2))
    rows = {k: [] for k in ("a_gate_ms", "a_optimize_ms", "a_total_ms", "b_edge_chi2_ms", "b_set_graph_ms", "b_optimize_ms", "b_total_ms",
                            "setup_ms")}
    gated = pcg_a = pcg_b = 0
    worst = 0.0
    with capi.Optimizer(0) as opt:
        for _ in range(reps):
            t = time.perf_counter()
            opt.set_graph(*g.arrays())
            rows["setup_ms"].append(1e3 * (time.perf_counter() - t))
            done, _ = opt.optimize(20)
            assert done == 20, opt.last_error()
            P1 = opt.get_poses()
            # (a) gate on the device
            t0 = time.perf_counter()
            gated, mask = opt.gate_edges(None, GATE)
            t1 = time.perf_counter()
            da, sa = opt.optimize(20)
            t2 = time.perf_counter()
            assert da == 20, opt.last_error()
            desc = opt.solver_description()
            # (b) the same from the same state: all edges back, the poses of before the gate
            opt.set_graph(*g.arrays())
            opt.set_poses(P1)
            t3 = time.perf_counter()
            e2 = opt.edge_chi2()
            keep = ~((g.phi >= 0) & (e2 > GATE))
            t4 = time.perf_counter()
            opt.set_graph(P1, g.fixed, g.ei[keep], g.ej[keep], g.meas[keep], g.info[keep], g.phi[keep])
            t5 = time.perf_counter()
            db, sb = opt.optimize(20)
            t6 = time.perf_counter()
            assert db == 20 and int((~keep).sum()) == gated
            worst = max(worst, max(abs(x - y) / y for x, y in zip(sa["chi2"], sb["chi2"])))
            pcg_a, pcg_b = sum(sa["pcg_iters"]), sum(sb["pcg_iters"])
            for k, v in (("a_gate_ms", t1 - t0), ("a_optimize_ms", t2 - t1), ("a_total_ms", t2 - t0), ("b_edge_chi2_ms", t4 - t3),
                         ("b_set_graph_ms", t5 - t4), ("b_optimize_ms", t6 - t5), ("b_total_ms", t6 - t3)):
                rows[k].append(1e3 * v)
    out = {k: round(statistics.median(v), 3) for k, v in rows.items()}
    out.update(config=name, V=g.V, E=g.E, corrupted=nbad, gated=int(gated), reps=reps, pcg_iters_a=int(pcg_a), pcg_iters_b=int(pcg_b),
               worst_rel_chi2_a_vs_b=worst, first_gate_ms=round(rows["a_gate_ms"][0], 3), description=desc.split(";")[0] + "; ..." + desc[-24:])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
