"""What tests/test_gpu_dogleg.py and tests/test_gpu_dogleg_pcg.py share: the cases, the measured tolerances and the comparison of a
device trace with tests/dogleg_reference.py's.  TEST INFRASTRUCTURE ONLY.

Graphs and starts are tests/test_gpu_lm.py's (its _graph, lm_reference.perturbed): no kernel, poses 1 .. V - 1 perturbed, starts from
which undamped Gauss-Newton's chi2 rises and the dogleg's first iterations reject trials.

Tolerances are measured, not fixed:
  d        sgo_optimize_gn's worst relative chi2 disagreement with np_oracle.gauss_newton on the same context options, start and
           iteration count (test_gpu_lm._gn_disagreement), floored at 1e-12;
  d_rho    per reference trial, 10 d (cur + tmp) / |L|: what such a disagreement of both chi2 does to the gain ratio.
Input condition, on the reference alone, for every trial compared: rho is at least 100 d_rho from each of 0, 0.25 and 0.75 -- no
rounding can turn the acceptance or the trust region's move --, and |h_gn| and |h_sd| are at least 1e-2 delta from delta -- none can
turn the kind.  Then trials[], step_kind[], iters_done and stop_reason are equal, robust_chi2[] and chi2[] agree within 10 d.
delta[] is EQUAL where the reference's value is delta_0 halved some times (a halving rounds nothing) and within 10 d elsewhere:
there it is 3 |h| of an accepted step, a norm the device forms from its own solve and sums -- the one quantity of the trace that
cannot be equal to numpy's bit for bit.
tolerated(ref) is the largest d for which every trial of a reference still meets the rho condition; each case records it (computed
on the CPU, asserted within 5 %), so a measured d above it fails at the input condition, not at a flipped decision."""
import functools
import math

import numpy as np

import dogleg_reference as dr
import lm_reference as lr
from sparse_gslam_amd import capi
from test_gpu_lm import _bits, _graph

ITERS = 8
RHO_POINTS = (0.0, 0.25, 0.75)
# name -> (V, E, seed, sigma, iterations, the reference's trials, its kinds, the largest d tolerated, the smallest kind margin)
GRAPHS = {
    "300_400": (300, 400, 2, 2.0, 8, [7, 1, 1, 2, 1, 1, 1, 1], "GGGGDDD D D DD D D D D", 5.6e-6, 0.32),
    "300_1200": (300, 1200, 5, 2.0, 8, [7, 1, 1, 1, 1, 1, 1, 1], "GGGGGDD D D G G G G G", 2.0e-5, 0.16),
    "2500_3400": (2500, 3400, 31, 1.0, 8, [3, 2, 1, 1, 1, 1, 1, 1], "GDD DD D D D D D D", 1.1e-5, 0.32),
    "1000_4000": (1000, 4000, 5, 1.0, 6, [4, 1, 1, 1, 1, 1], "GGDD G G G G G", 2.6e-5, 0.24),   # (the graph the analysis refuses)
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> graph, start (read-only), the reference's trace: computed once, shared"""
    V, E, seed, sigma, iters = GRAPHS[name][:5]
    g = _graph(V, E, seed)
    start = lr.perturbed(g, sigma)
    start.setflags(write=False)
    ref = dr.dogleg(start, *g.arrays()[1:], iters)
    trials, kinds, d_max, margin = GRAPHS[name][5:]
    assert ref["trials"] == trials and dr.pattern(ref) == kinds, (ref["trials"], dr.pattern(ref))
    assert abs(tolerated(ref) - d_max) <= 0.05 * d_max, (tolerated(ref), d_max)
    assert abs(kind_margin(ref) - margin) <= 0.05 * margin, (kind_margin(ref), margin)
    return g, start, ref


def tolerated(ref):
    return min(abs(r["rho"] - t) * abs(r["L"]) / (1000.0 * (r["cur"] + r["tmp"])) for r in ref["records"] for t in RHO_POINTS)


def kind_margin(ref):
    return min(abs(r[k] - r["delta"]) / r["delta"] for r in ref["records"] for k in ("gn_norm", "sd_norm"))


def twice(opt, start, iters, pcg=False, delta_init=0.0):
    """two calls from the same state -> the first call's (rc, stats, poses, sgo_chi2 after it); the second must repeat its bits"""
    runs = []
    for _ in range(2):
        opt.set_poses(start)
        rc, st = (opt.optimize_dogleg_pcg if pcg else opt.optimize_dogleg)(iters, delta_init)
        runs.append((rc, st, opt.get_poses(), opt.chi2()))
    a, b = runs
    assert a[0] == b[0] and np.array_equal(_bits(a[2]), _bits(b[2])) and a[3] == b[3]
    for k in ("iters_done", "trials_total", "solves", "stop_reason", "sync_rounds", "trials", "step_kind"):
        assert a[1][k] == b[1][k], k
    for k in ("delta", "robust_chi2", "chi2", "lam", "delta0"):
        assert np.array_equal(_bits(a[1][k]), _bits(b[1][k])), k
    return a


def properties(rc, st, chi2_after, pcg=False, rejected=None):
    r = st["robust_chi2"]
    assert rc == st["iters_done"] == len(st["trials"]) == len(st["delta"]) == len(st["step_kind"]) and len(r) == rc + 1 == len(st["chi2"])
    assert all(a >= b for a, b in zip(r, r[1:])), r
    assert (st["chi2"][rc], r[rc]) == chi2_after, ((st["chi2"][rc], r[rc]), chi2_after)
    assert st["stop_reason"] in (capi.DL_STOP_MAX_ITERS, capi.DL_STOP_TRIALS, capi.DL_STOP_DAMPING)
    assert st["trials_total"] == sum(st["trials"]) and all(1 <= q <= 100 for q in st["trials"])
    assert all(k in (capi.DL_STEP_GN, capi.DL_STEP_SD, capi.DL_STEP_DL, -1) for k in st["step_kind"])
    assert all(math.isfinite(x) and x > 0 for x in st["delta"]) and st["delta0"] > 0
    if st["lam"] == 0.0:                                   # H stayed positive definite: one solve per iteration, whatever the trials
        assert st["solves"] == st["iters_done"]
    else:
        assert st["lam"] > 0 and st["solves"] > st["iters_done"]
    # rejected trials: the reference's count where the traces are compared, else every trial but the accepted ones
    if rejected is None:
        rejected = st["trials_total"] - sum(1 for k in st["step_kind"] if k >= 0)
    if pcg:                                                # one read per solve, plus what the re-trials need
        assert st["solves"] <= st["sync_rounds"] <= st["solves"] + rejected or rc == 0
    elif st["lam"] == 0.0:
        assert 1 <= st["sync_rounds"] <= 1 + rejected
    else:
        assert 1 <= st["sync_rounds"] <= 1 + rejected + st["solves"] - st["iters_done"]


def compare(st, ref, d, whole):
    """the device's trace against the reference's: every trial (whole), or the prefix that meets the input condition -> iterations compared"""
    recs = ref["records"]
    d_rho = [10.0 * d * (r["cur"] + r["tmp"]) / abs(r["L"]) for r in recs]
    ok = [all(abs(r["rho"] - t) >= 100.0 * e for t in RHO_POINTS) and
          all(abs(r[k] - r["delta"]) >= 1e-2 * r["delta"] for k in ("gn_norm", "sd_norm")) for r, e in zip(recs, d_rho)]
    print("d", d, "tolerated", tolerated(ref), "kind margin", kind_margin(ref), "trials", ref["trials"], "device", st["trials"], "kinds",
          dr.pattern(ref), "device", st["step_kind"], "rounds", st["sync_rounds"], "solves", st["solves"])
    if whole:
        assert all(ok), [(r["it"], r["rho"], e) for r, e, o in zip(recs, d_rho, ok) if not o]
    n_ok = ok.index(False) if False in ok else len(ok)
    iters, t = 0, 0                     # whole iterations inside the prefix
    while iters < ref["iters_done"] and t + ref["trials"][iters] <= n_ok:
        t += ref["trials"][iters]
        iters += 1
    if whole:
        assert iters == ref["iters_done"] == st["iters_done"] and st["stop_reason"] == ref["stop_reason"]
        assert st["solves"] == ref["solves"] and st["trials_total"] == ref["trials_total"]
    assert st["iters_done"] >= iters and st["trials"][:iters] == ref["trials"][:iters]
    assert st["step_kind"][:iters] == ref["step_kind"][:iters]
    assert st["delta0"] == ref["delta0"]
    for k in ("robust_chi2", "chi2"):
        for i in range(iters + 1):
            print(k, i, st[k][i], ref[k][i], abs(st[k][i] - ref[k][i]) / ref[k][i])
            assert abs(st[k][i] - ref[k][i]) <= 10.0 * d * ref[k][i], (k, i, st[k][i], ref[k][i])
    for i in range(iters):
        a, b = st["delta"][i], ref["delta"][i]
        halved = math.frexp(b / ref["delta0"])[0] == 0.5 and b <= ref["delta0"]
        print("delta", i, a, b, "halved" if halved else abs(a - b) / b)
        assert a == b if halved else abs(a - b) <= 10.0 * d * b, (i, a, b)
    return iters
