"""sgo_optimize_lm (include/sgo.h) on the device against tests/lm_reference.py, the numpy statement of g2o's
Levenberg-Marquardt schedule.

Graphs: synth.manhattan(V, E, seed, info_mode="full", init="incremental") with no kernel (phi = -1), poses 1 .. V - 1 perturbed with
default_rng(1) (theta by N(0, sigma), then x and y): starts from which undamped Gauss-Newton's chi2 goes UP first and LM rejects trials.

Tolerances, derived per case and not fixed:
  d        the worst relative chi2 disagreement of sgo_optimize_gn against np_oracle.gauss_newton on the same graph, start and
           iteration count -- existing code against the reference, measured here --, floored at 1e-12;
  d_rho    per reference trial, 10 d (cur + tmp) / scale: what such a disagreement of both chi2 does to the gain ratio.
Input condition, on the reference alone: |rho| >= 100 d_rho for EVERY trial of the case, so that no rounding can turn a decision.  Then
the accept / reject pattern (trials[]), iters_done and stop_reason match exactly, robust_chi2[] and chi2[] agree within 10 d, lambda_k
within the sum of 18 d_rho over the trials so far (d lambda / lambda <= 6 (2 rho - 1)^2 d rho / alpha with alpha >= 1/3), and
lambda_0 within 1e-12 of 1e-5 max diag of the reference's H.
On the DCS graph (where LM stalls: g2o's rho' = s^2 is not the derivative of rho) the trace is compared over the prefix of reference
trials that meets the input condition; the one-iteration front-shape cases are held to the whole of it, as the listed cases are.
Every case, the mixed-kernel graph included, is held to the properties: robust_chi2[] never increases, its last entries are
sgo_chi2()'s bits, two calls from the same state agree bitwise, stop_reason is one of the four, sync_rounds <= 1 + rejected trials."""
import ctypes as C
import functools

import numpy as np
import pytest

import lm_reference as lr
import mfront_cases as mc
from oracle import np_oracle
from sparse_gslam_amd import capi, synth

pytestmark = pytest.mark.gpu

# name -> (V, E, seed, sigma, iterations, context options, the path optimize() takes)
CASES = {
    "300_direct": (300, 400, 2, 2.0, 8, {}, "direct_ldlt"),
    "300_pcg": (300, 400, 2, 2.0, 8, dict(direct_rows=0), "pcg"),
    "600_direct": (600, 620, 3, 1.5, 6, {}, "direct_ldlt"),
    "2500_mfront": (2500, 3400, 31, 1.0, 8, {}, "multifrontal_cholesky"),
}
DCS = (600, 620, 3, 1.5, 8)


def _graph(V, E, seed, phi=-1.0, init="incremental"):
    g = synth.manhattan(V, E, seed, info_mode="full", init=init, phi=max(phi, 1.0))
    if phi < 0:
        g.phi[:] = -1.0
    return g


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _lm_twice(opt, start, iters, lambda_init=0.0):
    """two calls from the same state -> the first call's (rc, stats, poses, sgo_chi2 after it); the second must repeat its bits"""
    runs = []
    for _ in range(2):
        opt.set_poses(start)
        rc, st = opt.optimize_lm(iters, lambda_init)
        runs.append((rc, st, opt.get_poses(), opt.chi2()))
    a, b = runs
    assert a[0] == b[0] and np.array_equal(_bits(a[2]), _bits(b[2])) and a[3] == b[3]
    for k in ("iters_done", "trials_total", "stop_reason", "sync_rounds", "trials"):
        assert a[1][k] == b[1][k], k
    for k in ("lam", "robust_chi2", "chi2"):
        assert np.array_equal(_bits(a[1][k]), _bits(b[1][k])), k
    assert a[1]["lambda0"] == b[1]["lambda0"]
    return a


def _properties(rc, st, chi2_after, ref=None):
    r = st["robust_chi2"]
    assert rc == st["iters_done"] == len(st["trials"]) == len(st["lam"]) and len(r) == rc + 1 == len(st["chi2"])
    assert all(a >= b for a, b in zip(r, r[1:])), r
    assert (st["chi2"][rc], r[rc]) == chi2_after, ((st["chi2"][rc], r[rc]), chi2_after)
    assert st["stop_reason"] in (capi.LM_STOP_MAX_ITERS, capi.LM_STOP_TRIALS, capi.LM_STOP_ZERO_GAIN, capi.LM_STOP_LAMBDA)
    assert st["trials_total"] == sum(st["trials"]) and all(1 <= q <= 10 for q in st["trials"])
    # rejected trials: the reference's count where the traces are compared, else every trial but those that lowered chi2
    rejected = (sum(1 for t in ref["records"] if not t["accepted"]) if ref is not None
                else st["trials_total"] - sum(1 for a, b in zip(r, r[1:]) if b < a))
    assert 1 <= st["sync_rounds"] <= 1 + rejected
    assert st["lambda0"] > 0 and all(np.isfinite(st["lam"]))


def _gn_disagreement(opt, g, start, iters):
    """d: sgo_optimize_gn against np_oracle.gauss_newton from `start`, over the entries both have"""
    opt.set_poses(start)
    _, st = opt.optimize(iters)
    _, ref = np_oracle.gauss_newton(start, *g.arrays()[1:], iters=iters)
    d = 1e-12
    for k in ("chi2", "robust_chi2"):
        for a, b in zip(st[k], ref[k]):
            if np.isfinite(a) and np.isfinite(b) and b > 0:
                d = max(d, abs(a - b) / b)
    return d


def _compare(st, ref, d, whole):
    """the device's trace against the reference's: every trial (whole), or the prefix that meets the input condition -> iterations compared"""
    recs = ref["records"]
    d_rho = [10.0 * d * (r["cur"] + r["tmp"]) / r["scale"] for r in recs]
    ok = [abs(r["rho"]) >= 100.0 * e for r, e in zip(recs, d_rho)]
    print("d", d, "min |rho| / d_rho", min(abs(r["rho"]) / e for r, e in zip(recs, d_rho)), "trials", ref["trials"], "device", st["trials"])
    if whole:
        assert all(ok), [(r["it"], r["rho"], e) for r, e, o in zip(recs, d_rho, ok) if not o]
    n_ok = ok.index(False) if False in ok else len(ok)
    iters, t = 0, 0                     # whole iterations inside the prefix
    while iters < ref["iters_done"] and t + ref["trials"][iters] <= n_ok:
        t += ref["trials"][iters]
        iters += 1
    if whole:
        assert iters == ref["iters_done"] == st["iters_done"] and st["stop_reason"] == ref["stop_reason"]
    assert st["iters_done"] >= iters and st["trials"][:iters] == ref["trials"][:iters]
    assert abs(st["lambda0"] - ref["lambda0"]) <= 1e-12 * ref["lambda0"], (st["lambda0"], ref["lambda0"])
    for k in ("robust_chi2", "chi2"):
        for i in range(iters + 1):
            assert abs(st[k][i] - ref[k][i]) <= 10.0 * d * ref[k][i], (k, i, st[k][i], ref[k][i])
    t = 0
    for i in range(iters):
        t += ref["trials"][i]
        bound = 18.0 * sum(d_rho[:t])
        assert abs(st["lam"][i] - ref["lam"][i]) <= bound * ref["lam"][i], (i, st["lam"][i], ref["lam"][i], bound)
    return iters


@functools.lru_cache(maxsize=None)
def _case(name):
    V, E, seed, sigma, iters, opts, path = CASES[name]
    g = _graph(V, E, seed)
    start = lr.perturbed(g, sigma)
    start.setflags(write=False)
    ref = lr.levenberg(start, *g.arrays()[1:], iters)
    return g, start, ref


@pytest.mark.parametrize("name", list(CASES))
def test_trace_against_the_reference(name):
    V, E, seed, sigma, iters, opts, path = CASES[name]
    g, start, ref = _case(name)
    assert sum(ref["trials"]) > iters                      # (the case is there for its rejections)
    with capi.Optimizer(0, **opts) as opt:
        opt.set_graph(*g.arrays())
        assert opt.solver_description().startswith(path), opt.solver_description()
        d = _gn_disagreement(opt, g, start, iters)
        rc, st, P, chi2_after = _lm_twice(opt, start, iters)
        assert opt.solver_description().startswith(path)
    _properties(rc, st, chi2_after, ref)
    assert _compare(st, ref, d, whole=True) == iters
    assert np.abs(P - ref["poses"]).max() <= 1e-6
    assert np.array_equal(_bits(P[g.fixed]), _bits(start[g.fixed]))


def test_dcs_graph_over_the_prefix_that_meets_the_condition():
    V, E, seed, sigma, iters = DCS
    g = _graph(V, E, seed, phi=10.0)
    start = lr.perturbed(g, sigma)
    ref = lr.levenberg(start, *g.arrays()[1:], iters)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        d = _gn_disagreement(opt, g, start, iters)
        rc, st, P, chi2_after = _lm_twice(opt, start, iters)
    _properties(rc, st, chi2_after)
    compared = _compare(st, ref, d, whole=False)
    accepted = sum(1 for i in range(compared) if st["robust_chi2"][i + 1] < st["robust_chi2"][i])
    assert accepted >= 2, (compared, accepted)


def test_mixed_kernels_hold_the_properties():
    """... and follow the reference's trace (lm_reference.levenberg with kinds: information w Omega, chi2 = sum rho0) over the prefix
    of its trials that meets the input condition: the reference stalls in its seventh iteration, whose last rejected trials have
    |rho| down to 4e-5, as the DCS graph's do.  d is measured as in every case here, with the kinds set and
    robust_reference.gauss_newton (the CPU oracle under the same identity) as the reference."""
    import robust_reference as rr
    from oracle import c_oracle
    from test_gpu_robust_kernels import _mixed
    g = _graph(600, 630, 5, phi=10.0)
    kind, delta = _mixed(g)
    start = lr.perturbed(g, 0.5)
    ref = lr.levenberg(start, *g.arrays()[1:], 8, kind=kind, delta=delta)
    _, gn = rr.gauss_newton(c_oracle, start, g, kind, delta, 8)
    for opts in ({}, dict(direct_rows=1)):
        with capi.Optimizer(0, **opts) as opt:
            opt.set_graph(*g.arrays())
            opt.set_robust_kernels(np.arange(g.E), kind, delta)
            opt.set_poses(start)
            _, st_gn = opt.optimize(8)
            d = max([1e-12] + [abs(a - b) / b for k in ("chi2", "robust_chi2") for a, b in zip(st_gn[k], gn[k])
                               if np.isfinite(a) and np.isfinite(b) and b > 0])
            rc, st, P, chi2_after = _lm_twice(opt, start, 8)
        _properties(rc, st, chi2_after)
        assert st["robust_chi2"][rc] < st["robust_chi2"][0] and np.isfinite(P).all()
        whole = all(abs(r["rho"]) >= 1000.0 * d * (r["cur"] + r["tmp"]) / r["scale"] for r in ref["records"])
        compared = _compare(st, ref, d, whole=whole)
        accepted = sum(1 for i in range(compared) if st["robust_chi2"][i + 1] < st["robust_chi2"][i])
        print("mixed kinds", opts, "compared", compared, "of", ref["iters_done"], "iterations, accepted inside", accepted, "whole", whole)
        assert accepted >= 2, (compared, accepted)


@pytest.mark.parametrize("name", mc.NAMES)
def test_one_iteration_on_every_front_shape(name):
    """the panel kernel's LM instantiation on the shapes tests/mfront_cases.py is there for: panel tails, the merge's K bodies, both
    branches of the substitution, widely scaled blocks"""
    c = mc.make(name)
    ref = lr.levenberg(*c.arrays(), 1)
    with mc.environment(c.env):
        with capi.Optimizer(0, direct_rows=1) as opt:
            opt.set_graph(*c.arrays())
            assert opt.solver_description().startswith("multifrontal_cholesky"), opt.solver_description()
            d = _gn_disagreement(opt, c, c.poses, 1)
            rc, st, P, chi2_after = _lm_twice(opt, c.poses, 1)
            # a lambda below every diagonal entry's last bit: the trial is the undamped step, through the same launches but for the
            # panel kernel's instantiation -- accepted at once, it leaves the bits of optimize(1)
            opt.set_poses(c.poses)
            assert opt.optimize(1)[0] == 1
            P_gn = opt.get_poses()
            opt.set_poses(c.poses)
            rc_t, st_t = opt.optimize_lm(1, 1e-300)
            P_t = opt.get_poses()
    _properties(rc, st, chi2_after, ref)
    assert rc == 1 and rc_t == 1 and st_t["lambda0"] == 1e-300
    assert ref["trials"] == [1] and ref["records"][0]["accepted"]          # (every case's undamped step lowers chi2: rho 0.94 .. 1.01)
    assert _compare(st, ref, d, whole=True) == 1
    assert st_t["trials"] == [1] and st_t["robust_chi2"][1] < st_t["robust_chi2"][0], st_t
    assert np.array_equal(_bits(P_t), _bits(P_gn))


def test_a_call_without_rejections_is_one_round():
    g = _graph(600, 620, 3, init="odom")
    ref = lr.levenberg(*g.arrays(), 12)
    assert ref["trials"] == [1] * 12
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        rc, st = opt.optimize_lm(12)
        assert rc == 12 and st["trials"] == [1] * 12 and st["sync_rounds"] == 1 and st["stop_reason"] == capi.LM_STOP_MAX_ITERS
        _properties(rc, st, opt.chi2())
        # lambda_init > 0 replaces 1e-5 max diag(H); zero iterations report the start and change nothing
        P = opt.get_poses()
        rc0, st0 = opt.optimize_lm(0, 0.125)
        assert rc0 == 0 and st0["lambda0"] == 0.125 and st0["sync_rounds"] == 1 and st0["trials_total"] == 0
        assert (st0["chi2"][0], st0["robust_chi2"][0]) == opt.chi2() and np.array_equal(_bits(opt.get_poses()), _bits(P))


@pytest.mark.parametrize("name", ["300_direct", "300_pcg", "2500_mfront"])
def test_gauss_newton_afterwards_has_the_bits_of_a_fresh_context(name):
    V, E, seed, sigma, iters, opts, path = CASES[name]
    g, start, _ = _case(name)
    with capi.Optimizer(0, **opts) as opt, capi.Optimizer(0, **opts) as fresh:
        for o in (opt, fresh):
            o.set_graph(*g.arrays())
        opt.set_poses(start)
        assert opt.optimize_lm(iters)[0] == iters
        P = opt.get_poses()
        fresh.set_poses(P)
        (da, sa), (db, sb) = opt.optimize(3), fresh.optimize(3)
        assert da == db == 3
        for k in ("chi2", "robust_chi2"):
            assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
        assert np.array_equal(_bits(opt.get_poses()), _bits(fresh.get_poses()))
        assert opt.solver_description() == fresh.solver_description()


def _raw_call(opt, iters, lambda_init):
    """the C call with a pre-filled stats block -> (rc, the block's bytes untouched?)"""
    st = capi.LmStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    before = bytes(st)
    rc = capi.lib().sgo_optimize_lm(opt._h, iters, lambda_init, C.byref(st))
    return rc, bytes(st) == before


def test_refusals_leave_poses_and_history_untouched():
    g, start, _ = _case("300_direct")
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(start)
        P0, c0 = _bits(opt.get_poses()), opt.chi2()
        for iters, lam in ((-1, 0.0), (capi.SGO_MAX_ITERS + 1, 0.0), (3, float("nan")), (3, float("inf")), (3, float("-inf"))):
            rc, untouched = _raw_call(opt, iters, lam)
            assert rc == -2 and untouched, (iters, lam, rc)
            assert "sgo_optimize_lm" in opt.last_error()
            assert np.array_equal(_bits(opt.get_poses()), P0) and opt.chi2() == c0
        assert opt.optimize_lm(2)[0] == 2                        # the context stays usable
    # the rank emulation of a multi-GPU context
    with capi.Optimizer(0, direct_rows=0, solver=capi.SOLVER_PCG_BJ) as opt:
        opt.debug_set_shard(2, 0)
        opt.set_graph(*g.arrays())
        P0 = _bits(opt.get_poses())
        rc, untouched = _raw_call(opt, 3, 0.0)
        assert rc == -2 and untouched and "multi-GPU" in opt.last_error()
        assert np.array_equal(_bits(opt.get_poses()), P0)


def test_an_active_overlay_is_refused():
    from test_gpu_edge_gate import _grow, _overlay_session
    base, steps, g, arrs, V, fixed, ids = _overlay_session()
    with capi.Optimizer(0, direct_rows=0) as opt:
        _grow(opt, base, steps, g, 6)
        assert "incremental overlay" in opt.solver_description()
        P0, c0 = _bits(opt.get_poses()), opt.chi2()
        rc, untouched = _raw_call(opt, 3, 0.0)
        assert rc == -2 and untouched and "incremental overlay" in opt.last_error()
        assert np.array_equal(_bits(opt.get_poses()), P0) and opt.chi2() == c0


def test_a_graph_the_analysis_refuses_returns_enothing():
    g = synth.manhattan(1000, 4000, seed=3, info_mode="full")
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        desc = opt.solver_description()
        why = desc.split("multifrontal path not used: ")[1].split(";")[0]
        P0 = _bits(opt.get_poses())
        for _ in range(2):                                       # (the refusal is cached per set-up)
            rc, st = opt.optimize_lm(3)
            assert rc == -1
            assert why in opt.last_error() and "sgo_optimize_gn" in opt.last_error(), (why, opt.last_error())
        assert np.array_equal(_bits(opt.get_poses()), P0)
        assert opt.optimize(2)[0] == 2


def test_an_indefinite_information_is_a_rejected_trial_not_a_failed_call():
    g, start, _ = _case("300_direct")
    info = g.info.copy()
    info[:, [0, 3, 5]] *= -1.0
    for opts in ({}, dict(direct_rows=1)):
        with capi.Optimizer(0, **opts) as opt:
            opt.set_graph(g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)
            rc, st = opt.optimize_lm(2)
            assert rc >= 1 and st["trials"][0] >= 2, st                  # H + lambda_0 I is not positive definite: trial 1 is rejected
            _properties(rc, st, opt.chi2())
            assert np.isfinite(opt.get_poses()).all()
            if st["trials"][0] == 10:                                    # (no lambda of the ladder made a trial acceptable)
                assert st["stop_reason"] == capi.LM_STOP_TRIALS and st["lam"][0] == st["lambda0"] * 2.0 ** 55
            # the context stays usable: a good graph then works
            opt.set_graph(*g.arrays())
            assert opt.optimize_lm(2)[0] == 2
