"""What the leave-group-out calls cost (NOTES.md section 44).

Host clock around calls that end in a synchronise, median [min, max] of nine warm calls, after optimize(8) on a multifrontal config
(default C3s):
  * sgo_edge_joint over the first 256 resident closures (with N, e and w copied out, and with none of them), beside
    sgo_candidate_joint over the same edges offered as candidates;
  * sgo_edge_groups over 256 groups of 8 (group b: table rows b .. b + 7, cyclic), and over 256 groups of 2 and of 40;
  * the same 256 clusters of 8 as hypotheses of sgo_optimize_gn_hypotheses(20, gain 0) on the same build, through the batched
    multifrontal route (a workspace for all 256) -- the only route to a cluster's verdict without these calls;
  * profile mode: per-call milliseconds and per-launch medians of the table's kernels and of k_edge_groups.
Usage: python scripts/edge_groups_timing.py [C3s C1 ...]   -> one JSON line per config"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparse_gslam_amd import capi, synth  # noqa: E402

synth.TRAJECTORY_FILE = synth.TRAJECTORY_FILE or os.path.join(ROOT, "tests", "golden", "ref_trajectories.npz")
REPS = 9
SLOTS = ("k_edge_cands + k_edge_table", "k_fs_rhs", "k_fs_forward", "k_fs_backward", "k_fs_gram", "k_edge_groups",
         "k_mf_edges + k_mf_merge + k_mf_panels (multifrontal factor phase)")


def _spread(fn, reps=REPS):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return [round(float(np.median(t)), 4), round(min(t), 4), round(max(t), 4)]


def _windows(B, size, n):
    M = np.zeros((B, n), dtype=np.uint8)
    for b in range(B):
        M[b, (b + np.arange(size)) % n] = 1
    return M


def run(name):
    g = synth.config(name)
    closures = np.flatnonzero(np.abs(g.ei.astype(np.int64) - g.ej) != 1)[:256].astype(np.int32)
    n = closures.size
    out = dict(config=name, V=g.V, E=g.E, closures=int(n))
    L, ip = capi.lib(), capi._ip
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        out["path"] = opt.solver_description().split(":")[0]
        opt.optimize(8)
        out["edge_joint_ms"] = _spread(lambda: opt.edge_joint(closures))
        out["edge_joint_no_copy_ms"] = _spread(lambda: L.sgo_edge_joint(opt._h, n, ip(closures), None, None, None))
        out["candidate_joint_same_edges_ms"] = _spread(lambda: opt.candidate_joint(g.ei[closures], g.ej[closures], g.meas[closures], g.info[closures]))
        opt.edge_joint(closures)
        groups = {}
        for size in (2, 8, 40):
            M = _windows(256, size, n)
            groups[f"256 x {size}"] = _spread(lambda M=M: opt.edge_groups(M, np.full(256, 40.0)))
        out["edge_groups_ms"] = groups
        _, d2, _, piv, _ = opt.edge_groups(_windows(256, 8, n), np.full(256, 40.0))
        out["groups_of_8_decided"] = int((piv >= 1e-3).sum())
        # the same clusters as hypotheses
        off = np.zeros((256, g.E), dtype=np.uint8)
        for b in range(256):
            off[b, closures[(b + np.arange(8)) % n]] = 1
        per = opt.hypotheses_bytes(20, False)
        opt.set_hypotheses_workspace(256 * per)
        r = opt.optimize_hypotheses(off, 20, 0.0, want=("hist",))
        out["hypotheses"] = dict(B=256, route=int(r["route"]), iters_done=[int(r["iters_done"].min()), int(r["iters_done"].max())],
                                 ms=_spread(lambda: opt.optimize_hypotheses(off, 20, 0.0, want=("hist",)), 3))
        out["hypotheses_over_groups"] = out["hypotheses"]["ms"][0] / (out["edge_joint_no_copy_ms"][0] + groups["256 x 8"][0])
    with capi.Optimizer(0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.optimize(8)
        M = _windows(256, 8, n)
        opt.edge_joint(closures)
        opt.edge_groups(M)
        opt.profile_reset()
        for _ in range(REPS):
            opt.edge_joint(closures)
            opt.edge_groups(M)
        prof = opt.kernel_profile(quantiles=True)
        out["kernels"] = {s: dict(ms_per_call=prof[s]["ms"] / REPS, launches_per_call=prof[s]["launches"] / REPS, median_launch_us=prof[s].get("median_us"))
                          for s in SLOTS if s in prof}
        for size in (2, 40):
            M = _windows(256, size, n)
            opt.edge_groups(M)
            opt.profile_reset()
            for _ in range(REPS):
                opt.edge_groups(M)
            prof = opt.kernel_profile(quantiles=True)
            out["kernels"][f"k_edge_groups, 256 x {size}"] = dict(median_launch_us=prof["k_edge_groups"].get("median_us"))
    return out


if __name__ == "__main__":
    for name in [a for a in sys.argv[1:] if not a.startswith("-")] or ["C3s"]:
        print(json.dumps(run(name)), flush=True)
