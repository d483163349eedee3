"""sgo_optimize_dogleg (include/sgo.h) on the device against tests/dogleg_reference.py, the numpy statement of
g2o's dogleg schedule: one factorisation per iteration, every trial a blend of the Gauss-Newton and the Cauchy step.

Cases, tolerances and the input condition: tests/dogleg_cases.py.  Contexts are tests/test_gpu_lm.py's for the same graphs: the
single-launch direct one and the PCG one for 300 / 400 (the call analyses a plan of its own there), the resident multifrontal plan
for 2 500 / 3 400.  The tolerated d of each graph, from the CPU reference: 5.6e-6 and 1.1e-5 (measured before on these contexts:
1.6e-8, 2.6e-8).  300 / 1 200 has four edges per pose: the multifrontal analysis refuses it, as it refuses 1 000 / 4 000, and the
graph is tests/test_gpu_dogleg_pcg.py's.

Beyond the traces: solves == iters_done < trials_total wherever a trial is rejected -- the point of the algorithm --; one round for a
call without a rejection and at most 1 + rejected otherwise; from the mild 600 / 620 dead-reckoned start every step is the GN step and
on a multifrontal_cholesky context poses and sgo_chi2 are sgo_optimize_gn(3)'s bit for bit (the history entries are sgo_chi2's
launches' and agree with sgo_optimize_gn's own sums, which are k_mf_edges', to 10 d); two calls give the same bits; sgo_chi2 after the
call is the last history entry; an indefinite information leads to damping; refusals leave everything untouched; Gauss-Newton
afterwards has the bits of a context that never ran dogleg; DCS and mixed kernels hold the properties."""
import ctypes as C

import numpy as np
import pytest

import dogleg_cases as dc
import dogleg_reference as dr
import lm_reference as lr
from sparse_gslam_amd import capi, synth
from test_gpu_lm import _bits, _gn_disagreement, _graph

pytestmark = pytest.mark.gpu

# name -> (graph, context options, the path optimize() takes)
CASES = {
    "300_direct": ("300_400", {}, "direct_ldlt"),
    "300_pcg": ("300_400", dict(direct_rows=0), "pcg"),
    "2500_mfront": ("2500_3400", {}, "multifrontal_cholesky"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_trace_against_the_reference(name):
    graph, opts, path = CASES[name]
    iters = dc.GRAPHS[graph][4]
    g, start, ref = dc.case(graph)
    rejected = sum(1 for r in ref["records"] if not r["accepted"])
    assert rejected > 0
    with capi.Optimizer(0, **opts) as opt:
        opt.set_graph(*g.arrays())
        assert opt.solver_description().startswith(path), opt.solver_description()
        d = _gn_disagreement(opt, g, start, iters)
        rc, st, P, chi2_after = dc.twice(opt, start, iters)
        assert opt.solver_description().startswith(path)
    dc.properties(rc, st, chi2_after, rejected=rejected)
    assert dc.compare(st, ref, d, whole=True) == iters
    assert st["solves"] == st["iters_done"] == iters < st["trials_total"] and st["lam"] == 0.0
    assert np.array_equal(_bits(P[g.fixed.astype(bool)]), _bits(start[g.fixed.astype(bool)]))
    assert np.isfinite(P).all()


@pytest.mark.parametrize("opts", [{}, dict(direct_rows=1)], ids=["direct", "mfront"])
def test_a_mild_start_is_gauss_newton_in_one_round(opts):
    g = _graph(600, 620, 3, init="odom")
    ref = dr.dogleg(*g.arrays(), 3)
    assert ref["trials"] == [1, 1, 1] and ref["step_kind"] == [dr.STEP_GN] * 3
    with capi.Optimizer(0, **opts) as opt:
        opt.set_graph(*g.arrays())
        desc = opt.solver_description()
        d = _gn_disagreement(opt, g, g.poses, 3)
        P_gn, chi2_gn = opt.get_poses(), opt.chi2()
        opt.set_poses(g.poses)
        _, st_gn = opt.optimize(3)
        rc, st, P, chi2_after = dc.twice(opt, g.poses, 3)
        dc.properties(rc, st, chi2_after)
        assert rc == 3 and st["trials"] == [1, 1, 1] and st["step_kind"] == [capi.DL_STEP_GN] * 3
        assert st["sync_rounds"] == 1 and st["solves"] == 3 and st["stop_reason"] == capi.DL_STOP_MAX_ITERS
        assert all(x >= 1e4 for x in st["delta"])                 # (never halved)
        assert dc.compare(st, ref, d, whole=True) == 3
        for k in ("chi2", "robust_chi2"):
            for a, b in zip(st[k], st_gn[k]):
                assert abs(a - b) <= 10.0 * d * b, (k, a, b)
        if desc.startswith("multifrontal_cholesky"):           # the same launches but for the panel kernel's instantiation, lambda = 0.0
            assert np.array_equal(_bits(P), _bits(P_gn)) and chi2_after == chi2_gn
        else:
            assert not opts
        # zero iterations report the start and change nothing; delta_init > 0 replaces 1e4
        rc0, st0 = opt.optimize_dogleg(0, 0.125)
        assert rc0 == 0 and st0["delta0"] == 0.125 and st0["sync_rounds"] == 1 and st0["trials_total"] == 0 == st0["solves"]
        assert (st0["chi2"][0], st0["robust_chi2"][0]) == opt.chi2() and np.array_equal(_bits(opt.get_poses()), _bits(P))


def test_a_small_trust_region_scales_the_cauchy_step():
    """delta_init far below |h_sd|: the first trial is the scaled Cauchy step, which the listed cases never take"""
    g, start, _ = dc.case("300_400")
    ref = dr.dogleg(start, *g.arrays()[1:], 2, 1e-3)
    assert ref["records"][0]["kind"] == dr.STEP_SD and ref["records"][0]["accepted"]
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        d = _gn_disagreement(opt, g, start, 2)
        rc, st, P, chi2_after = dc.twice(opt, start, 2, delta_init=1e-3)
    dc.properties(rc, st, chi2_after)
    assert st["step_kind"][0] == capi.DL_STEP_SD and st["delta0"] == 1e-3
    dc.compare(st, ref, d, whole=False)


@pytest.mark.parametrize("name", ["300_direct", "300_pcg", "2500_mfront"])
def test_gauss_newton_afterwards_has_the_bits_of_a_fresh_context(name):
    graph, opts, path = CASES[name]
    g, start, _ = dc.case(graph)
    with capi.Optimizer(0, **opts) as opt, capi.Optimizer(0, **opts) as fresh:
        for o in (opt, fresh):
            o.set_graph(*g.arrays())
        opt.set_poses(start)
        assert opt.optimize_dogleg(4)[0] == 4
        P = opt.get_poses()
        fresh.set_poses(P)
        (da, sa), (db, sb) = opt.optimize(3), fresh.optimize(3)
        assert da == db == 3
        for k in ("chi2", "robust_chi2"):
            assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
        assert list(sa["pcg_iters"]) == list(sb["pcg_iters"])
        assert np.array_equal(_bits(opt.get_poses()), _bits(fresh.get_poses()))
        assert opt.solver_description() == fresh.solver_description()


def _raw_call(opt, iters, delta_init, fn="sgo_optimize_dogleg"):
    """the C call with a pre-filled stats block -> (rc, the block's bytes untouched?)"""
    st = capi.DoglegStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    before = bytes(st)
    rc = getattr(capi.lib(), fn)(opt._h, iters, delta_init, C.byref(st))
    return rc, bytes(st) == before


def test_refusals_leave_poses_and_history_untouched():
    g, start, _ = dc.case("300_400")
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(start)
        P0, c0 = _bits(opt.get_poses()), opt.chi2()
        for iters, delta in ((-1, 0.0), (capi.SGO_MAX_ITERS + 1, 0.0), (3, float("nan")), (3, float("inf")), (3, float("-inf"))):
            rc, untouched = _raw_call(opt, iters, delta)
            assert rc == -2 and untouched, (iters, delta, rc)
            assert "sgo_optimize_dogleg" in opt.last_error()
            assert np.array_equal(_bits(opt.get_poses()), P0) and opt.chi2() == c0
        assert opt.optimize_dogleg(2)[0] == 2                    # the context stays usable
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
    g, start, _ = dc.case("1000_4000")
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        desc = opt.solver_description()
        why = desc.split("multifrontal path not used: ")[1].split(";")[0]
        P0 = _bits(opt.get_poses())
        for _ in range(2):                                       # (the refusal is cached per set-up)
            rc, st = opt.optimize_dogleg(3)
            assert rc == -1
            assert why in opt.last_error() and "sgo_optimize_dogleg_pcg" in opt.last_error(), (why, opt.last_error())
        assert np.array_equal(_bits(opt.get_poses()), P0)
        assert opt.optimize(2)[0] == 2


def test_an_indefinite_information_leads_to_damping():
    g, start, _ = dc.case("300_400")
    info = g.info.copy()
    info[:, [0, 3, 5]] *= -1.0
    for opts in ({}, dict(direct_rows=1)):
        with capi.Optimizer(0, **opts) as opt:
            opt.set_graph(g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)
            P0 = _bits(opt.get_poses())
            rc, st = opt.optimize_dogleg(2)
            print(st)
            assert st["lam"] > 0 and st["solves"] > st["iters_done"], st   # the undamped pivot is not positive: the solve is repeated damped
            dc.properties(rc, st, opt.chi2())
            assert np.isfinite(opt.get_poses()).all()
            if st["stop_reason"] == capi.DL_STOP_DAMPING:                 # (no lambda up to 1e3 made H + lambda I positive definite)
                assert rc == 0 and st["lam"] == 1e3 and st["solves"] == 11 and st["trials_total"] == 0
                assert np.array_equal(_bits(opt.get_poses()), P0)
            else:
                assert rc >= 1
            # the context stays usable: a good graph then works
            opt.set_graph(*g.arrays())
            assert opt.optimize_dogleg(2)[0] == 2


def test_dcs_graph_holds_the_properties():
    """g2o's DCS sets rho' = s^2, which is not the derivative of rho: neither step need be a descent direction of the robust chi2 the
    gain ratio tests, and from a dead-reckoned start the call may reject until the trust region has shrunk -- the safe no-op.  The
    properties are the check."""
    g = _graph(600, 620, 3, phi=10.0, init="odom")
    for start in (g.poses, lr.perturbed(g, 1.5)):
        with capi.Optimizer(0) as opt:
            opt.set_graph(*g.arrays())
            rc, st, P, chi2_after = dc.twice(opt, start, 8)
        print("DCS", st["trials"], st["step_kind"], st["robust_chi2"], st["stop_reason"], st["sync_rounds"])
        dc.properties(rc, st, chi2_after)
        assert np.isfinite(P).all()


def test_mixed_kernels_hold_the_properties():
    from test_gpu_robust_kernels import _mixed
    g = _graph(600, 630, 5, phi=10.0)
    kind, delta = _mixed(g)
    start = lr.perturbed(g, 0.5)
    ref = dr.dogleg(start, *g.arrays()[1:], 8, kind=kind, delta=delta)
    for opts in ({}, dict(direct_rows=1)):
        with capi.Optimizer(0, **opts) as opt:
            opt.set_graph(*g.arrays())
            opt.set_robust_kernels(np.arange(g.E), kind, delta)
            rc, st, P, chi2_after = dc.twice(opt, start, 8)
        print("mixed kinds", opts, st["trials"], st["step_kind"], "reference", ref["trials"], ref["step_kind"], st["robust_chi2"][-1],
              ref["robust_chi2"][-1])
        dc.properties(rc, st, chi2_after)
        assert np.isfinite(P).all() and st["robust_chi2"][rc] <= st["robust_chi2"][0]
