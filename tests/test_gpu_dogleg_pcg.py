"""sgo_optimize_dogleg_pcg (include/sgo.h) on the device against tests/dogleg_reference.py: g2o's dogleg schedule
with the iteration's ONE solve done by the context's PCG, on every single-GPU context.

Cases, tolerances and the input condition: tests/dogleg_cases.py.  Contexts are tests/test_gpu_lm_pcg.py's for the same graphs: AMG
and block-Jacobi for 300 / 400, AMG for 300 / 1 200, the multifrontal context for 2 500 / 3 400 (which builds its row plan and
hierarchy on first use).  Tolerated d: 5.6e-6, 2.0e-5, 1.1e-5 (measured before: 1.6e-8 -- 1.5e-7 under block-Jacobi --, 5.7e-11, 2.6e-8).

The graph the multifrontal analysis refuses is 1 000 / 4 000, seed 5, sigma 1.0: trials 4 1 1 1 1 1 (GGDD G G G G G) over six
iterations, tolerated d 2.6e-5 against 1.4e-5 measured on that shape.  That margin is thin, so the case compares the prefix of
reference trials that meets the input condition -- and fails, instead of passing empty, unless the prefix contains the whole first
iteration: its two rejections and its blend.

sync_rounds: one read of the state per solve, and one per group of re-trials while an iteration stays open: solves <= sync_rounds <=
solves + rejected trials."""
import ctypes as C

import numpy as np
import pytest

import dogleg_cases as dc
import dogleg_reference as dr
import lm_reference as lr
from sparse_gslam_amd import capi
from test_gpu_lm import _bits, _gn_disagreement, _graph

pytestmark = pytest.mark.gpu

AMG, BJ = dict(direct_rows=0), dict(direct_rows=0, solver=capi.SOLVER_PCG_BJ)
# name -> (graph, context options, the path optimize() takes)
CASES = {
    "300_400_amg": ("300_400", AMG, "pcg_amg"),
    "300_400_bj": ("300_400", BJ, "pcg_block_jacobi"),
    "300_1200_amg": ("300_1200", AMG, "pcg_amg"),
    "2500_3400_mfront": ("2500_3400", {}, "multifrontal_cholesky"),
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
        rc, st, P, chi2_after = dc.twice(opt, start, iters, pcg=True)
        assert opt.solver_description().startswith(path)
    dc.properties(rc, st, chi2_after, pcg=True, rejected=rejected)
    assert dc.compare(st, ref, d, whole=True) == iters
    assert st["solves"] == st["iters_done"] == iters < st["trials_total"] and st["lam"] == 0.0
    assert np.array_equal(_bits(P[g.fixed.astype(bool)]), _bits(start[g.fixed.astype(bool)]))
    assert np.isfinite(P).all()


def test_the_graph_the_analysis_refuses_over_the_prefix_that_meets_the_condition():
    g, start, ref = dc.case("1000_4000")
    iters = dc.GRAPHS["1000_4000"][4]
    assert ref["trials"][0] == 4 and [r["accepted"] for r in ref["records"][:4]] == [False, False, False, True]
    assert [r["kind"] for r in ref["records"][:4]] == [dr.STEP_GN, dr.STEP_GN, dr.STEP_DL, dr.STEP_DL]
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        desc = opt.solver_description()
        assert desc.startswith("pcg_amg") and "multifrontal path not used" in desc, desc
        assert opt.optimize_dogleg(3)[0] == -1 and "sgo_optimize_dogleg_pcg" in opt.last_error()
        d = _gn_disagreement(opt, g, start, iters)
        rc, st, P, chi2_after = dc.twice(opt, start, iters, pcg=True)
        # zero iterations report the start and change nothing
        rc0, st0 = opt.optimize_dogleg_pcg(0, 0.125)
        assert rc0 == 0 and st0["delta0"] == 0.125 and st0["trials_total"] == 0 == st0["solves"]
        assert (st0["chi2"][0], st0["robust_chi2"][0]) == opt.chi2() and np.array_equal(_bits(opt.get_poses()), _bits(P))
    dc.properties(rc, st, chi2_after, pcg=True)
    compared = dc.compare(st, ref, d, whole=False)
    print("compared", compared, "of", ref["iters_done"], "iterations")
    assert compared >= 1, (compared, d)                     # the whole first iteration: two rejections of the GN step, one of a blend, the blend
    assert st["trials"][0] == 4 and st["solves"] == st["iters_done"] < st["trials_total"]


@pytest.mark.parametrize("opts", [AMG, BJ], ids=["amg", "block_jacobi"])
def test_a_mild_start_is_one_gauss_newton_step(opts):
    """on the contexts whose sgo_optimize_gn is itself the PCG: the same cold solve behind a refreshed hierarchy, the step copied --
    chi2 after one iteration within 10 d of sgo_optimize_gn(1)'s (measured: equal; on a direct_ldlt context, whose Gauss-Newton step
    is a factorisation's, d is that solver's 3.5e-11 while the two steps differ by what pcg_tol allows, 4.6e-10)"""
    g = _graph(600, 620, 3, init="odom")
    with capi.Optimizer(0, **opts) as opt:
        opt.set_graph(*g.arrays())
        assert opt.solver_description().startswith("pcg_")
        d = _gn_disagreement(opt, g, g.poses, 1)
        opt.set_poses(g.poses)
        _, st_gn = opt.optimize(1)
        rc, st, P, chi2_after = dc.twice(opt, g.poses, 1, pcg=True)
    dc.properties(rc, st, chi2_after, pcg=True)
    assert rc == 1 and st["trials"] == [1] and st["step_kind"] == [capi.DL_STEP_GN] and st["sync_rounds"] == 1 == st["solves"]
    for k in ("chi2", "robust_chi2"):
        for a, b in zip(st[k], st_gn[k]):
            print(k, a, b, d)
            assert abs(a - b) <= 10.0 * d * b, (k, a, b, d)


def test_both_routes_agree_on_a_multifrontal_context():
    g, start, _ = dc.case("2500_3400")
    with capi.Optimizer(0) as opt, capi.Optimizer(0) as fresh:
        for o in (opt, fresh):
            o.set_graph(*g.arrays())
        d = _gn_disagreement(opt, g, start, dc.ITERS)
        opt.set_poses(start)
        rc_f, st_f = opt.optimize_dogleg(dc.ITERS)
        opt.set_poses(start)
        rc_p, st_p = opt.optimize_dogleg_pcg(dc.ITERS)
        print("d", d, "factor", st_f["robust_chi2"], "pcg", st_p["robust_chi2"])
        assert rc_f == rc_p and st_f["trials"] == st_p["trials"] and st_f["step_kind"] == st_p["step_kind"]
        assert st_f["stop_reason"] == st_p["stop_reason"] and st_f["solves"] == st_p["solves"]
        for k in ("robust_chi2", "chi2"):
            for a, b in zip(st_f[k], st_p[k]):
                assert abs(a - b) <= 10.0 * d * a, (k, a, b, d)
        # Gauss-Newton afterwards: the bits of a context that never ran dogleg
        for o in (opt, fresh):
            o.set_poses(start)
        (da, sa), (db, sb) = opt.optimize(3), fresh.optimize(3)
        assert da == db == 3 and opt.solver_description().startswith("multifrontal_cholesky")
        for k in ("chi2", "robust_chi2"):
            assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
        assert np.array_equal(_bits(opt.get_poses()), _bits(fresh.get_poses()))


@pytest.mark.parametrize("name", ["1000_4000", "300_400_bj"])
def test_no_trace_on_a_pcg_context(name):
    """set_graph; set_poses(P); optimize(3) against set_graph; optimize_dogleg_pcg(4); set_poses(P); optimize(3)"""
    graph, opts = (name, {}) if name == "1000_4000" else CASES[name][:2]
    V, E, seed = dc.GRAPHS[graph][:3]
    g = _graph(V, E, seed)
    P = lr.perturbed(g, 0.05)
    with capi.Optimizer(0, **opts) as a, capi.Optimizer(0, **opts) as b:
        for o in (a, b):
            o.set_graph(*g.arrays())
        assert b.optimize_dogleg_pcg(4)[0] == 4
        for o in (a, b):
            o.set_poses(P)
        (da, sa), (db, sb) = a.optimize(3), b.optimize(3)
        assert da == db == 3
        for k in ("chi2", "robust_chi2"):
            assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
        assert list(sa["pcg_iters"]) == list(sb["pcg_iters"]), (sa["pcg_iters"], sb["pcg_iters"])
        assert np.array_equal(_bits(a.get_poses()), _bits(b.get_poses()))
        assert a.solver_description() == b.solver_description()


def test_an_indefinite_information_leads_to_damping():
    g, start, _ = dc.case("300_400")
    info = g.info.copy()
    info[:, [0, 3, 5]] *= -1.0
    with capi.Optimizer(0, **AMG) as opt:
        opt.set_graph(g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)
        P0 = _bits(opt.get_poses())
        rc, st = opt.optimize_dogleg_pcg(2)
        print(st)
        assert st["lam"] > 0 and st["solves"] > st["iters_done"], st     # the PCG breaks down on p . H p <= 0: the solve is repeated damped
        dc.properties(rc, st, opt.chi2(), pcg=True)
        assert np.isfinite(opt.get_poses()).all()
        if st["stop_reason"] == capi.DL_STOP_DAMPING:
            assert rc == 0 and st["lam"] == 1e3 and st["trials_total"] == 0 and np.array_equal(_bits(opt.get_poses()), P0)
        else:
            assert rc >= 1
        opt.set_graph(*g.arrays())                                   # the context stays usable: a good graph then works
        assert opt.optimize_dogleg_pcg(2)[0] == 2 and opt.optimize(2)[0] == 2


def _raw_call(opt, iters, delta_init):
    """the C call with a pre-filled stats block -> (rc, the block's bytes untouched?)"""
    st = capi.DoglegStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    before = bytes(st)
    rc = capi.lib().sgo_optimize_dogleg_pcg(opt._h, iters, delta_init, C.byref(st))
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
            assert "sgo_optimize_dogleg_pcg" in opt.last_error()
            assert np.array_equal(_bits(opt.get_poses()), P0) and opt.chi2() == c0
        assert opt.optimize_dogleg_pcg(2)[0] == 2                # the context (a single-launch direct one) stays usable
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


def test_dcs_graph_holds_the_properties():
    g = _graph(600, 620, 3, phi=10.0, init="odom")
    with capi.Optimizer(0, **AMG) as opt:
        opt.set_graph(*g.arrays())
        rc, st, P, chi2_after = dc.twice(opt, g.poses, 8, pcg=True)
    print("DCS", st["trials"], st["step_kind"], st["robust_chi2"], st["stop_reason"], st["sync_rounds"])
    dc.properties(rc, st, chi2_after, pcg=True)
    assert np.isfinite(P).all()


def test_mixed_kernels_hold_the_properties():
    from test_gpu_robust_kernels import _mixed
    g = _graph(600, 630, 5, phi=10.0)
    kind, delta = _mixed(g)
    start = lr.perturbed(g, 0.5)
    with capi.Optimizer(0, **AMG) as opt:
        opt.set_graph(*g.arrays())
        opt.set_robust_kernels(np.arange(g.E), kind, delta)
        rc, st, P, chi2_after = dc.twice(opt, start, 8, pcg=True)
    print("mixed kinds", st["trials"], st["step_kind"], st["robust_chi2"])
    dc.properties(rc, st, chi2_after, pcg=True)
    assert np.isfinite(P).all() and st["robust_chi2"][rc] <= st["robust_chi2"][0]
