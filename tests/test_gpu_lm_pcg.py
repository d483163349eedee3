"""sgo_optimize_lm_pcg (include/sgo.h) on the device against tests/lm_reference.py: g2o's Levenberg-Marquardt
schedule with every trial's (H + lambda I) x = b solved by the context's PCG, on every single-GPU context.

Graphs, starts, tolerances and the input condition are tests/test_gpu_lm.py's (its _graph, _lm_twice, _properties, _gn_disagreement
and _compare, with optimize_lm_pcg in place of optimize_lm): d is sgo_optimize_gn's measured disagreement with
np_oracle.gauss_newton ON THE SAME CONTEXT OPTIONS, floored at 1e-12; d_rho = 10 d (cur + tmp) / scale; every reference trial must
have |rho| >= 100 d_rho.  CASES lists the reference's trials per iteration (computed on the CPU with lm_reference.levenberg and
asserted here) and the largest d for which every trial of the case still meets the input condition; a case whose measured d exceeds
it fails at the input condition.

sync_rounds: the PCG route reads the state once per trial, so sync_rounds == trials_total -- checked here; _properties, which holds
the factor route to 1 + the rejected trials, is given the stats with that one field set to 1."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import lm_reference as lr
from oracle import np_oracle
from sparse_gslam_amd import capi, synth
from test_gpu_lm import _bits, _compare, _gn_disagreement, _graph, _properties

pytestmark = pytest.mark.gpu

AMG, BJ = dict(direct_rows=0), dict(direct_rows=0, solver=capi.SOLVER_PCG_BJ)
# name -> (V, E, seed, sigma, context options, the path optimize() takes, the reference's trials, the largest d tolerated)
CASES = {
    "300_400_amg": (300, 400, 2, 2.0, AMG, "pcg_amg", [3, 1, 1, 1, 2, 1, 1, 1], 4.5e-6),
    "300_400_bj": (300, 400, 2, 2.0, BJ, "pcg_block_jacobi", [3, 1, 1, 1, 2, 1, 1, 1], 4.5e-6),
    "300_1200_amg": (300, 1200, 5, 2.0, AMG, "pcg_amg", [1, 1, 1, 1, 1, 2, 1, 1], 2.3e-5),
    "1000_4000_refused": (1000, 4000, 3, 2.0, {}, "pcg_amg", [1, 1, 1, 1, 1, 1, 3, 1], 1.9e-5),   # (the graph the analysis refuses)
    "2500_3400_mfront": (2500, 3400, 31, 1.0, {}, "multifrontal_cholesky", [1, 1, 1, 1, 1, 1, 1, 4], 5.2e-7),
}
ITERS = 8


class _Pcg:
    """an Optimizer whose optimize_lm is the PCG route's, for test_gpu_lm.py's helpers"""

    def __init__(self, opt):
        self._opt = opt

    def __getattr__(self, name):
        return getattr(self._opt, "optimize_lm_pcg" if name == "optimize_lm" else name)


def _lm_twice(opt, start, iters, lambda_init=0.0):
    from test_gpu_lm import _lm_twice as twice
    return twice(_Pcg(opt), start, iters, lambda_init)


def _props(rc, st, chi2_after, ref=None):
    assert st["sync_rounds"] == st["trials_total"], st
    _properties(rc, dict(st, sync_rounds=1), chi2_after, ref)


@functools.lru_cache(maxsize=None)
def _case(name):
    V, E, seed, sigma = CASES[name][:4]
    g = _graph(V, E, seed)
    start = lr.perturbed(g, sigma)
    start.setflags(write=False)
    ref = lr.levenberg(start, *g.arrays()[1:], ITERS)
    return g, start, ref


def _wrapped(P, Q):
    """P - Q with the angle's difference wrapped"""
    D = np.asarray(P) - np.asarray(Q)
    D[:, 2] = np_oracle.normalize_theta(D[:, 2])
    return D


@pytest.mark.parametrize("name", list(CASES))
def test_trace_against_the_reference(name):
    V, E, seed, sigma, opts, path, trials, d_max = CASES[name]
    g, start, ref = _case(name)
    assert ref["trials"] == trials and sum(trials) > ITERS
    tolerated = min(abs(r["rho"]) * r["scale"] / (1000.0 * (r["cur"] + r["tmp"])) for r in ref["records"])
    assert abs(tolerated - d_max) <= 0.05 * d_max, (tolerated, d_max)
    with capi.Optimizer(0, **opts) as opt:
        opt.set_graph(*g.arrays())
        desc = opt.solver_description()
        assert desc.startswith(path), desc
        if name == "1000_4000_refused":                       # 300 rows are inverted densely: this is the case with a coarse level
            assert "multifrontal path not used" in desc and "L1 n=" in desc, desc
        d = _gn_disagreement(opt, g, start, ITERS)
        rc, st, P, chi2_after = _lm_twice(opt, start, ITERS)
        its, how = opt.lm_pcg_trace()
        assert opt.solver_description().startswith(path)
    print(name, "d", d, "PCG iterations per trial", its.tolist(), "solves", how.tolist())
    assert len(its) == st["trials_total"] and set(how.tolist()) <= {capi.LM_SOLVE_CONVERGED, capi.LM_SOLVE_FLOOR}
    _props(rc, st, chi2_after, ref)
    assert _compare(st, ref, d, whole=True) == ITERS
    # (the poses are printed, not bounded: these starts are far from converged after eight iterations, and sgo_optimize_gn's own chi2
    # disagrees with the oracle's by up to 1.4e-5 from them)
    print(name, "poses against the reference's, worst component", np.abs(_wrapped(P, ref["poses"])).max())
    assert np.array_equal(_bits(P[g.fixed.astype(bool)]), _bits(start[g.fixed.astype(bool)]))


@pytest.mark.parametrize("opts", [AMG, BJ], ids=["amg", "block_jacobi"])
def test_the_shift_reaches_the_operator(opts):
    """one iteration with lambda = max |diag H|, a shift as large as H itself: the poses afterwards are start (+) x with
    x = solve_direct(H + lambda I, b) within 100 pcg_tol |x|_inf per component -- kappa(H + lambda I) is below 10 (computed here:
    its largest eigenvalue is at most |H|_inf + lambda and its smallest at least lambda), so a relative residual of pcg_tol bounds
    the relative error by 10 pcg_tol"""
    g, start, _ = _case("300_1200_amg")
    H, b, _, _ = np_oracle.linearize(start, *g.arrays()[1:])
    lam = float(np.max(np.abs(H.diagonal())))
    w = np.linalg.eigvalsh(H.toarray() + lam * np.eye(H.shape[0]))
    kappa = w[-1] / w[0]
    x = np_oracle.solve_direct((H + lam * sp.identity(H.shape[0], format="csc")).tocsc(), b)
    want = np_oracle.oplus(start, g.fixed, x)
    with capi.Optimizer(0, **opts) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(start)
        tol = 100.0 * capi.default_opts().pcg_tol * np.abs(x).max()
        rc, st = opt.optimize_lm_pcg(1, lam)
        P = opt.get_poses()
        its, how = opt.lm_pcg_trace()
    err = np.abs(_wrapped(P, want)).max()
    print("kappa(H + lambda I)", kappa, "lambda", lam, "PCG iterations", its.tolist(), "error", err, "tolerance", tol)
    assert kappa < 10.0
    assert rc == 1 and st["trials"] == [1] and st["lambda0"] == lam and how.tolist() == [capi.LM_SOLVE_CONVERGED]
    assert st["robust_chi2"][1] < st["robust_chi2"][0]
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("name", ["300_1200_amg", "1000_4000_refused"])
def test_the_shift_reaches_the_preconditioner(name):
    """H + lambda I is no worse conditioned than H: the first trial's solve, behind a hierarchy refreshed for the shifted system, takes
    no more PCG iterations than sgo_optimize_gn's first solve from the same start on the same context, but for the margin of a
    preconditioner that is merely different -- the larger of +3 and +25 %.  A level that missed the shift shows up as a multiple."""
    V, E, seed, sigma, opts, path, _, _ = CASES[name]
    g, start, _ = _case(name)
    with capi.Optimizer(0, **opts) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(start)
        _, gn = opt.optimize(1)
        opt.set_poses(start)
        rc, st = opt.optimize_lm_pcg(1)
        its, how = opt.lm_pcg_trace()
    n_gn, n_lm = int(gn["pcg_iters"][0]), int(its[0])
    print(name, "PCG iterations: GN's first solve", n_gn, "LM's first trial", n_lm, "ratio", n_lm / max(n_gn, 1))
    assert how[0] == capi.LM_SOLVE_CONVERGED and n_gn >= 1
    assert n_lm <= max(n_gn + 3, int(np.floor(1.25 * n_gn))), (n_lm, n_gn)


def test_both_routes_agree_on_a_multifrontal_context():
    g, start, _ = _case("2500_3400_mfront")
    with capi.Optimizer(0) as opt, capi.Optimizer(0) as fresh:
        for o in (opt, fresh):
            o.set_graph(*g.arrays())
        d = _gn_disagreement(opt, g, start, ITERS)
        opt.set_poses(start)
        rc_f, st_f = opt.optimize_lm(ITERS)
        opt.set_poses(start)
        rc_p, st_p = opt.optimize_lm_pcg(ITERS)
        print("d", d, "factor", st_f["robust_chi2"], "pcg", st_p["robust_chi2"])
        assert rc_f == rc_p and st_f["trials"] == st_p["trials"] and st_f["stop_reason"] == st_p["stop_reason"]
        for k in ("robust_chi2", "chi2"):
            for a, b in zip(st_f[k], st_p[k]):
                assert abs(a - b) <= 10.0 * d * a, (k, a, b, d)
        # Gauss-Newton afterwards: the bits of a context that never ran LM
        for o in (opt, fresh):
            o.set_poses(start)
        (da, sa), (db, sb) = opt.optimize(3), fresh.optimize(3)
        assert da == db == 3 and opt.solver_description().startswith("multifrontal_cholesky")
        for k in ("chi2", "robust_chi2"):
            assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
        assert np.array_equal(_bits(opt.get_poses()), _bits(fresh.get_poses()))


@pytest.mark.parametrize("name", ["1000_4000_refused", "300_400_bj"])
def test_no_trace_on_a_pcg_context(name):
    """set_graph; set_poses(P); optimize(3) against set_graph; optimize_lm_pcg(4); set_poses(P); optimize(3)"""
    V, E, seed, sigma, opts, path, _, _ = CASES[name]
    g = _graph(V, E, seed)
    P = lr.perturbed(g, 0.05)
    with capi.Optimizer(0, **opts) as a, capi.Optimizer(0, **opts) as b:
        for o in (a, b):
            o.set_graph(*g.arrays())
        assert b.optimize_lm_pcg(4)[0] == 4
        for o in (a, b):
            o.set_poses(P)
        (da, sa), (db, sb) = a.optimize(3), b.optimize(3)
        assert da == db == 3
        for k in ("chi2", "robust_chi2"):
            assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
        assert list(sa["pcg_iters"]) == list(sb["pcg_iters"]), (sa["pcg_iters"], sb["pcg_iters"])
        assert np.array_equal(_bits(a.get_poses()), _bits(b.get_poses()))
        assert a.solver_description() == b.solver_description()


def test_an_indefinite_information_is_a_rejected_trial_not_a_failed_call():
    g, start, _ = _case("300_400_amg")
    info = g.info.copy()
    info[:, [0, 3, 5]] *= -1.0
    with capi.Optimizer(0, **AMG) as opt:
        opt.set_graph(g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)
        rc, st = opt.optimize_lm_pcg(2)
        its, how = opt.lm_pcg_trace()
        print(st, its.tolist(), how.tolist())
        assert rc >= 1 and st["trials"][0] >= 2, st                  # H + lambda_0 I is not positive definite: trial 1 is rejected
        assert how[0] < 0, how                                       # ... because its solve failed (minus the PCG stop code)
        _props(rc, st, opt.chi2())
        assert np.isfinite(opt.get_poses()).all()
        opt.set_graph(*g.arrays())                                   # the context stays usable: a good graph then works
        assert opt.optimize_lm_pcg(2)[0] == 2 and opt.optimize(2)[0] == 2


def _raw_call(opt, iters, lambda_init):
    """the C call with a pre-filled stats block -> (rc, the block's bytes untouched?)"""
    st = capi.LmStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    before = bytes(st)
    rc = capi.lib().sgo_optimize_lm_pcg(opt._h, iters, lambda_init, C.byref(st))
    return rc, bytes(st) == before


def test_refusals_leave_poses_and_history_untouched():
    g, start, _ = _case("300_400_amg")
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(start)
        P0, c0 = _bits(opt.get_poses()), opt.chi2()
        for iters, lam in ((-1, 0.0), (capi.SGO_MAX_ITERS + 1, 0.0), (3, float("nan")), (3, float("inf")), (3, float("-inf"))):
            rc, untouched = _raw_call(opt, iters, lam)
            assert rc == -2 and untouched, (iters, lam, rc)
            assert "sgo_optimize_lm_pcg" in opt.last_error()
            assert np.array_equal(_bits(opt.get_poses()), P0) and opt.chi2() == c0
        assert opt.optimize_lm_pcg(2)[0] == 2                    # the context (a single-launch direct one) stays usable
    with capi.Optimizer(0, **BJ) as opt:                         # the rank emulation of a multi-GPU context
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


def test_the_graph_the_analysis_refuses_takes_the_pcg_route():
    g = synth.manhattan(1000, 4000, seed=3, info_mode="full")
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        assert opt.optimize_lm(3)[0] == -1 and "sgo_optimize_lm_pcg" in opt.last_error()
        rc, st = opt.optimize_lm_pcg(3)
        assert rc == 3
        _props(rc, st, opt.chi2())
        # zero iterations report the start and change nothing; lambda_init > 0 replaces 1e-5 max diag(H)
        P = opt.get_poses()
        rc0, st0 = opt.optimize_lm_pcg(0, 0.125)
        assert rc0 == 0 and st0["lambda0"] == 0.125 and st0["sync_rounds"] == 0 == st0["trials_total"] and len(opt.lm_pcg_trace()[0]) == 0
        assert (st0["chi2"][0], st0["robust_chi2"][0]) == opt.chi2() and np.array_equal(_bits(opt.get_poses()), _bits(P))


def test_dcs_graph_holds_the_properties():
    from test_gpu_lm import DCS
    V, E, seed, sigma, iters = DCS
    g = _graph(V, E, seed, phi=10.0)
    start = lr.perturbed(g, sigma)
    ref = lr.levenberg(start, *g.arrays()[1:], iters)
    with capi.Optimizer(0, **AMG) as opt:
        opt.set_graph(*g.arrays())
        d = _gn_disagreement(opt, g, start, iters)
        rc, st, P, chi2_after = _lm_twice(opt, start, iters)
    _props(rc, st, chi2_after)
    # The properties are the check here.  On this PCG context sgo_optimize_gn under DCS from this start disagrees with the oracle by
    # d = 1.2e-2 (measured; 1.5e-4 on the single-launch context of test_gpu_lm.py), so the prefix of reference trials that meets the input
    # condition may be empty: the trace is compared over whatever prefix there is, and its length is printed.
    compared = _compare(st, ref, d, whole=False)
    print("DCS: d", d, "compared", compared, "of", ref["iters_done"], "iterations; trials", st["trials"], "reference", ref["trials"])
    assert st["robust_chi2"][rc] < st["robust_chi2"][0] and np.isfinite(P).all()


def test_mixed_kernels_hold_the_properties():
    """test_gpu_lm.py's mixed-kernel graph on a PCG context: the properties, and the reference's trace over the prefix of its trials
    that meets the input condition (d measured with the kinds set, against robust_reference.gauss_newton)"""
    import robust_reference as rr
    from oracle import c_oracle
    from test_gpu_robust_kernels import _mixed
    g = _graph(600, 630, 5, phi=10.0)
    kind, delta = _mixed(g)
    start = lr.perturbed(g, 0.5)
    ref = lr.levenberg(start, *g.arrays()[1:], 8, kind=kind, delta=delta)
    _, gn = rr.gauss_newton(c_oracle, start, g, kind, delta, 8)
    with capi.Optimizer(0, **AMG) as opt:
        opt.set_graph(*g.arrays())
        opt.set_robust_kernels(np.arange(g.E), kind, delta)
        opt.set_poses(start)
        _, st_gn = opt.optimize(8)
        d = max([1e-12] + [abs(a - b) / b for k in ("chi2", "robust_chi2") for a, b in zip(st_gn[k], gn[k])
                           if np.isfinite(a) and np.isfinite(b) and b > 0])
        rc, st, P, chi2_after = _lm_twice(opt, start, 8)
    _props(rc, st, chi2_after)
    assert st["robust_chi2"][rc] < st["robust_chi2"][0] and np.isfinite(P).all()
    whole = all(abs(r["rho"]) >= 1000.0 * d * (r["cur"] + r["tmp"]) / r["scale"] for r in ref["records"])
    compared = _compare(st, ref, d, whole=whole)
    accepted = sum(1 for i in range(compared) if st["robust_chi2"][i + 1] < st["robust_chi2"][i])
    print("mixed kinds: compared", compared, "of", ref["iters_done"], "iterations, accepted inside", accepted, "whole", whole)
    assert accepted >= 2, (compared, accepted)
