"""What the joint-compatibility calls cost (NOTES.md section 40).

Host clock around calls that end in a synchronise, median of nine warm calls, on C1i (single-launch direct path), C1 and C3s
(multifrontal) after optimize(8):
  * sgo_candidate_joint(n), n = 5, 16, 64, 256 (with S and e copied out, and with neither), beside sgo_candidate_gate(n) on the same
    candidates.  With --gate the gate alone is
    timed and nothing newer is used: run that with --root pointing at a built checkout of the commit to compare against.
  * sgo_joint_subsets for B = 1, 256, 4 096 subsets of 2, 10 and 40 of 64 candidates, and sgo_joint_pairs at n = 64 and 256, beside
    a host loop of scipy.linalg.cho_factor / cho_solve on the returned S over the same subsets, and beside the only route the parent
    has to the same decision: the candidates inserted as edges of the graph and masked off per hypothesis,
    sgo_optimize_gn_hypotheses(20, gain 0) over --hyp-b (default 8) of the subsets of 10.
  * profile mode: the per-launch medians of k_fs_gram, k_fs_joint_table and k_joint_subsets.
  * --search (NOTES.md section 43), at n = 64 and 256 candidates, median [min, max] of the warm calls:
    (a) sgo_joint_extend over B = 1, 64, 1 024 parents of 2, 10 and 39 candidates beside sgo_joint_subsets over the same B (n - k)
    extended sets (the route without the search's calls: every extension factorised from scratch by its own workgroup);
    (b) sgo_joint_greedy from the n singleton seeds under the 99 % chi2 ladder beside the host loop that calls sgo_joint_subsets once
    per step over every live path's extensions; and k_joint_grow's per-launch median in profile mode.
Usage: python scripts/joint_timing.py [--gate | --search] [--root DIR] [--hyp-b N] [C1i C1 C3s]   -> one JSON line per config"""
import json
import os
import sys
import time

import numpy as np

ARGS = sys.argv[1:]
ROOT = ARGS[ARGS.index("--root") + 1] if "--root" in ARGS else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparse_gslam_amd import capi, synth  # noqa: E402

synth.TRAJECTORY_FILE = synth.TRAJECTORY_FILE or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                              "ref_trajectories.npz")
COUNTS = (5, 16, 64, 256)
BATCHES = (1, 256, 4096)
SIZES = (2, 10, 40)
SLOTS = ("k_fs_gram", "k_fs_joint_table", "k_joint_subsets")
REPS = 9


def _warm(fn, reps=REPS):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def _closure_candidates(g, k, seed=9):
    """k revisits of the trajectory that are not edges of the graph, measured with N(0, sig) noise (scripts/marginals_timing.py's)"""
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


def _masks(B, size, n, seed=3):
    rng = np.random.default_rng(seed + 31 * size)
    M = np.zeros((B, n), dtype=np.uint8)
    for b in range(B):
        M[b, rng.choice(n, size=size, replace=False)] = 1
    return M


def _host_loop(S, e, M):
    import scipy.linalg as sla
    ev = e.reshape(-1)
    out = np.empty(M.shape[0])
    for b, m in enumerate(M):
        r = (3 * np.flatnonzero(m)[:, None] + np.arange(3)[None, :]).reshape(-1)
        out[b] = ev[r] @ sla.cho_solve(sla.cho_factor(S[np.ix_(r, r)], lower=True), ev[r])
    return out


def run_gate(name):
    g = synth.config(name)
    ci, cj, meas, info = _closure_candidates(g, max(COUNTS))
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        path = opt.solver_description().split(":")[0]
        opt.optimize(8)
        warm = {k: _warm(lambda k=k: opt.candidate_gate(ci[:k], cj[:k], meas[:k], info[:k], 11.345)) for k in COUNTS}
    return dict(config=name, lib=ROOT, path=path, what="gate alone", gate_warm_ms=warm)


def _spread(fn, reps=REPS):
    """median [min, max] of `reps` warm calls, milliseconds"""
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return [round(float(np.median(t)), 4), round(min(t), 4), round(max(t), 4)]


def _extension_masks(parents, n):
    """the sets parent + {c}, c not in the parent: [B (n - k)][n]"""
    rows = []
    for p in parents:
        base = np.zeros(n, dtype=np.uint8)
        base[p] = 1
        free = np.flatnonzero(base == 0)
        M = np.repeat(base[None, :], free.size, axis=0)
        M[np.arange(free.size), free] = 1
        rows.append(M)
    return np.concatenate(rows)


def _host_greedy(opt, n, chi, max_len=40):
    """the greedy search of the n singleton seeds driven from the host: one sgo_joint_subsets per step over every live path's
    extensions -> (orders, steps)"""
    sets = [[s] for s in range(n)]
    live = list(range(n))
    steps = 0
    while live:
        M = _extension_masks([sets[b] for b in live], n)
        d2 = opt.joint_subsets(M)[1]
        steps += 1
        nxt, at = [], 0
        for b in live:
            k = len(sets[b])
            v = d2[at:at + n - k]
            at += n - k
            free = np.setdiff1d(np.arange(n), sets[b])
            ok = v <= chi[k + 1]
            if ok.any():
                sets[b].append(int(free[np.argmin(np.where(ok, v, np.inf))]))
                if len(sets[b]) < max_len:
                    nxt.append(b)
        live = nxt
    return sets, steps


def run_search(name):
    from scipy.stats import chi2 as chi2_dist
    g = synth.config(name)
    ci, cj, meas, info = _closure_candidates(g, 256)
    chi = np.concatenate([[0.0], chi2_dist.ppf(0.99, 3 * np.arange(1, 41))])
    out = dict(config=name, lib=ROOT, V=g.V, E=g.E, what="search: median [min, max] ms")
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        out["path"] = opt.solver_description().split(":")[0]
        opt.optimize(8)
        for n in (64, 256):
            opt.candidate_joint(ci[:n], cj[:n], meas[:n], info[:n])
            rng = np.random.default_rng(17)
            ext, sub, agree = {}, {}, 0.0
            for k in (2, 10, 39):
                for B in (1, 64, 1024):
                    parents = [rng.permutation(n)[:k] for _ in range(B)]
                    M = _extension_masks(parents, n)
                    ext[f"{k}x{B}"] = _spread(lambda parents=parents: opt.joint_extend(parents))
                    sub[f"{k}x{B}"] = _spread(lambda M=M: opt.joint_subsets(M), 3 if M.shape[0] > 20000 else REPS)
                    if B <= 64:
                        a, b = opt.joint_extend(parents)[1], opt.joint_subsets(M)[1]
                        free = np.concatenate([np.setdiff1d(np.arange(n), p) + n * i for i, p in enumerate(parents)])
                        agree = max(agree, float(np.nanmax(np.abs(a.reshape(-1)[free] - b) / b)))
            seeds = [[t] for t in range(n)]
            order, count, _, _, _ = opt.joint_greedy(seeds, chi)
            host_sets, steps = _host_greedy(opt, n, chi)
            same = sum(list(order[b, :count[b]]) == host_sets[b] for b in range(n))
            out[f"n={n}"] = dict(extend_ms=ext, subsets_same_sets_ms=sub, worst_disagreement=agree,
                                 greedy_ms=_spread(lambda: opt.joint_greedy(seeds, chi)), host_loop_ms=_spread(lambda: _host_greedy(opt, n, chi), 2),
                                 host_loop_steps=steps, path_lengths=[int(count.min()), int(np.median(count)), int(count.max())],
                                 paths_equal_to_host_loop=f"{same}/{n}")
    with capi.Optimizer(0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.optimize(8)
        kernels = {}
        for n in (64, 256):
            opt.candidate_joint(ci[:n], cj[:n], meas[:n], info[:n])
            seeds = [[t] for t in range(n)]
            opt.joint_greedy(seeds, chi)
            opt.profile_reset()
            for _ in range(REPS):
                opt.joint_greedy(seeds, chi)
            prof = opt.kernel_profile(quantiles=True)
            kernels[f"n={n}, {n} singleton seeds"] = dict(ms_per_call=prof["k_joint_grow"]["ms"] / REPS, median_launch_us=prof["k_joint_grow"].get("median_us"))
        out["kernels"] = kernels
    return out


def run(name, hyp_b):
    g = synth.config(name)
    ci, cj, meas, info = _closure_candidates(g, max(COUNTS))
    out = dict(config=name, lib=ROOT, V=g.V, E=g.E)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        out["path"] = opt.solver_description().split(":")[0]
        done, st = opt.optimize(8)
        P8 = opt.get_poses()
        out["gn_iteration_ms"] = 1e3 * float(np.median(st["seconds"][:done]))
        out["gate_warm_ms"] = {k: _warm(lambda k=k: opt.candidate_gate(ci[:k], cj[:k], meas[:k], info[:k], 11.345)) for k in COUNTS}
        out["joint_warm_ms"] = {k: _warm(lambda k=k: opt.candidate_joint(ci[:k], cj[:k], meas[:k], info[:k])) for k in COUNTS}
        L, ip, dp = capi.lib(), capi._ip, capi._dp
        out["joint_no_copy_warm_ms"] = {k: _warm(lambda k=k: L.sgo_candidate_joint(opt._h, k, ip(ci[:k]), ip(cj[:k]), dp(meas[:k]), dp(info[:k]), None, None))
                                        for k in COUNTS}
        out["joint_over_gate"] = {k: out["joint_warm_ms"][k] / out["gate_warm_ms"][k] for k in COUNTS}
        pairs = {}
        for n in (64, 256):
            opt.candidate_joint(ci[:n], cj[:n], meas[:n], info[:n])
            pairs[n] = _warm(opt.joint_pairs)
        out["pairs_warm_ms"] = pairs
        S, e = opt.candidate_joint(ci[:64], cj[:64], meas[:64], info[:64])
        sub, host, agree = {}, {}, 0.0
        for size in SIZES:
            for B in BATCHES:
                M = _masks(B, size, 64)
                sub[f"{size}x{B}"] = _warm(lambda M=M: opt.joint_subsets(M))
                if B <= 256:
                    host[f"{size}x{B}"] = _warm(lambda M=M: _host_loop(S, e, M), 3)
                    d2 = opt.joint_subsets(M)[1]
                    want = _host_loop(S, e, M)
                    agree = max(agree, float(np.max(np.abs(d2 - want) / want)))
        out["subsets_warm_ms"], out["host_cho_loop_ms"], out["worst_disagreement_with_host_loop"] = sub, host, agree
    # the parent's route to the same decision: the candidates as edges, masked off per hypothesis, optimised per subset
    Mh = _masks(hyp_b, 10, 64)
    arr = list(g.arrays())
    arr[2] = np.r_[arr[2], ci[:64]].astype(np.int32)
    arr[3] = np.r_[arr[3], cj[:64]].astype(np.int32)
    arr[4] = np.vstack([arr[4], meas[:64]])
    arr[5] = np.vstack([arr[5], info[:64]])
    arr[6] = np.r_[arr[6], np.full(64, -1.0)]
    arr[0] = P8
    off = np.zeros((hyp_b, g.E + 64), dtype=np.uint8)
    off[:, g.E:] = 1 - Mh
    with capi.Optimizer(0) as opt:
        opt.set_graph(*arr)
        r = opt.optimize_hypotheses(off, 20, 0.0, want=("hist",))
        out["hypotheses"] = dict(B=hyp_b, subset_size=10, route=int(r["route"]), iters_done=r["iters_done"].tolist(),
                                 warm_ms=_warm(lambda: opt.optimize_hypotheses(off, 20, 0.0, want=("hist",)), 3))
    with capi.Optimizer(0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.optimize(8)
        kernels = {}
        for n, size, B in ((64, 10, 256), (256, 40, 4096)):
            M = _masks(B, size, n)
            opt.candidate_joint(ci[:n], cj[:n], meas[:n], info[:n])
            opt.joint_subsets(M)
            opt.profile_reset()
            for _ in range(REPS):
                opt.candidate_joint(ci[:n], cj[:n], meas[:n], info[:n])
                opt.joint_subsets(M)
            prof = opt.kernel_profile(quantiles=True)
            kernels[f"n={n}, {B} subsets of {size}"] = {s: dict(ms_per_call=prof[s]["ms"] / REPS, launches_per_call=prof[s]["launches"] / REPS,
                                                                 median_launch_us=prof[s].get("median_us")) for s in SLOTS if s in prof}
        out["kernels"] = kernels
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.optimize(8)
        opt.candidate_joint(ci[:64], cj[:64], meas[:64], info[:64])
        out["hypotheses"]["joint_subsets_same_B_ms"] = _warm(lambda: opt.joint_subsets(Mh))
    return out


if __name__ == "__main__":
    names = [a for a in ARGS if a in ("C1i", "C1", "C3s", "C2", "C4")] or ["C1i", "C1", "C3s"]
    hyp_b = int(ARGS[ARGS.index("--hyp-b") + 1]) if "--hyp-b" in ARGS else 8
    for name in names:
        print(json.dumps(run_gate(name) if "--gate" in ARGS else run_search(name) if "--search" in ARGS else run(name, hyp_b)), flush=True)
