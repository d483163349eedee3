"""The floor rule on the GPU (sgo_solve.cpp: solve_backward_error; sgo_rules.h: floor_backward_error).  A solve that stops short of
pcg_tol is accepted -- the step applied, sgo_stats.pcg_converged = 2 -- only when its x is at the floating-point floor of the
Jacobi-scaled system, measured with the TRUE residual b - H x.  On graphs with one stiff row (a prior-like edge of information 1e14 I
from the fixed pose 0) a solve cut off far from its solution is rejected as g2o rejects a failed solve (optimize() returns 0, the
estimates stay), where round 6's normwise measure, |r| / (2 max_i |D_i| |x| + |b|), accepted it; a solve run to the floor of the same
system is accepted and its iterates are the direct solver's.  Multigrid PCG on C2 + the prior on pose 5000, block-Jacobi PCG (which
converges too slowly on C2) on C1 + the prior on pose 500; the incremental overlay's operator (U M U^T beside the resident graph)
through an update_graph session.  Every solve is iterative: direct_rows = 0, SGO_MFRONT = 0."""
import numpy as np
import pytest

from oracle import c_oracle, np_oracle
from sparse_gslam_amd import capi, synth

pytestmark = pytest.mark.gpu

STIFF = 1e14
# (solver, graph, pose the prior ends in, pcg_maxit that takes every solve of a 3-iteration call to the floor, relres < 1e-11 at the
# cut-off, and stops it before it reaches pcg_tol = 1e-17.  Measured on an MI355X, relative residuals of the three solves:
#   multigrid     30: 1.5e-11 8.6e-12 2.1e-10 (the third rejected)   45: 1.6e-17 1.2e-17 1.9e-16   46 - 49: pcg_tol reached
#   block-Jacobi  3000: 1.2e-15 5.0e-13 1.7e-13   4000: 6.7e-14 9.1e-13 1.0e-16                   4462 - 4582: pcg_tol reached
# -- 40 lies between 30 and 45, a few decades from either end.)
CASES = {
    "amg": (capi.SOLVER_PCG_AMG, "C2", 5000, 40),
    "bj": (capi.SOLVER_PCG_BJ, "C1", 500, 4000),
}


def with_prior(g, s, j):
    """g plus one edge from the fixed pose 0 to pose j that agrees with the current poses, information s I, no robust kernel."""
    rel = np_oracle.se2_mul(np_oracle.se2_inv(g.poses[0:1]), g.poses[j:j + 1])
    return synth.Graph(g.poses, g.fixed, np.append(g.ei, 0).astype(g.ei.dtype), np.append(g.ej, j).astype(g.ej.dtype),
                       np.vstack([g.meas, rel]), np.vstack([g.info, [[s, 0.0, 0.0, s, 0.0, s]]]), np.append(g.phi, -1.0))


@pytest.fixture(autouse=True)
def _iterative(monkeypatch):
    monkeypatch.setenv("SGO_MFRONT", "0")


def _graph(case):
    solver, name, j, _ = CASES[case]
    g = synth.config(name)
    assert g.fixed[0]
    return solver, with_prior(g, STIFF, j)


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_solve_cut_off_far_from_its_solution_is_rejected_despite_a_stiff_row(case):
    """8 PCG iterations (relative residual of a few per cent) and a tolerance out of reach: the call fails at its first solve, as g2o's
    optimize() does on a failed solve.  (Round 6's measure took this solve for one at the floor: the stiff row made max_i |D_i| 1e14.)"""
    solver, g = _graph(case)
    with capi.Optimizer(0, solver=solver, direct_rows=0, pcg_tol=1e-17, pcg_tol_cap=0.0, pcg_maxit=8) as o:
        o.set_graph(*g.arrays())
        P0 = o.get_poses()
        done, st = o.optimize(3)
        err = o.last_error()
        P = o.get_poses()
    assert done == 0, (done, st["pcg_converged"][:3], st["pcg_relres"][:3])
    assert st["pcg_converged"][0] == 0, st["pcg_converged"][:3]
    assert "pcg_maxit" in err, err
    assert np.array_equal(P, P0)


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_solve_at_the_floor_of_a_system_with_a_stiff_row_is_accepted(case):
    """The same systems with every solve run to the floating-point floor and cut off before pcg_tol = 1e-17 (relative residual < 1e-11
    at the cut-off): the steps are applied (pcg_converged = 2) and the iterates are the CPU oracle's with a direct solver."""
    solver, g = _graph(case)
    maxit = CASES[case][3]
    with capi.Optimizer(0, solver=solver, direct_rows=0, pcg_tol=1e-17, pcg_tol_cap=0.0, pcg_maxit=maxit) as o:
        o.set_graph(*g.arrays())
        done, st = o.optimize(3)
        err = o.last_error()
        P = o.get_poses()
    assert done == 3, (done, err, st["pcg_iters"][:3], st["pcg_relres"][:3])
    assert st["pcg_converged"][:3] == [2, 2, 2], st["pcg_converged"][:3]
    assert max(st["pcg_relres"][:3]) < 1e-11, st["pcg_relres"][:3]
    oP, ost = c_oracle.gauss_newton(*g.arrays(), iters=3, solver="direct")
    for k in range(4):
        assert abs(st["chi2"][k] - ost["chi2"][k]) <= 1e-9 * ost["chi2"][k], (k, st["chi2"][k], ost["chi2"][k])
    assert np.abs(P - oP).max() <= 1e-6, np.abs(P - oP).max()


# takes every solve of the updated system to the floor before pcg_tol: measured, 30 iterations: 6.6e-12 1.6e-12 1.2e-12 (all accepted),
# 45: the second and third solves reach pcg_tol = 1e-17 at 44
OVERLAY_MAXIT = 36


def test_the_floor_rule_measures_the_overlay_operator():
    """An incremental update (sgo_update_graph_se2: the resident graph + an appended chain and a closure, solved with the overlay's
    U M U^T beside the resident operator), pcg_tol = 1e-17: solves run to the floor and cut off before pcg_tol are accepted, and every
    iterate is a fresh set-up's of the same graph run the same way; solves cut off at 8 iterations are rejected.  A true residual
    without the overlay's term would not be at the floor, and the first half would fail."""
    base, steps, g = synth.append_session(3000, 12000, 1, 20, seed=3)
    odom_meas = g.meas[: g.V - 1]
    st0 = steps[0]
    V = st0["V"]
    fixed = np.zeros(V, dtype=bool)
    fixed[:base.V] = base.fixed
    ei, ej, meas, info, phi = (np.concatenate([getattr(base, k), st0[k]]) for k in ("ei", "ej", "meas", "info", "phi"))
    P = base.poses   # (near the optimum, as after the reference's previous optimize(20))
    P0 = np.empty((V, 3))
    P0[: P.shape[0]] = P
    synth.chain_init(P0, odom_meas, P.shape[0], V - 1)
    for maxit in (OVERLAY_MAXIT, 8):
        opts = dict(direct_rows=0, pcg_tol=1e-17, pcg_tol_cap=0.0, pcg_maxit=maxit)
        with capi.Optimizer(0, **opts) as inc, capi.Optimizer(0, **opts) as fresh:
            inc.set_graph(*base.arrays())
            inc.update_graph(P0, fixed, ei, ej, meas, info, phi, base.E)
            desc = inc.solver_description()
            assert "incremental overlay" in desc, desc
            d, st = inc.optimize(3)
            err = inc.last_error()
            Pi = inc.get_poses()
            fresh.set_graph(P0, fixed, ei, ej, meas, info, phi)
            df, sf = fresh.optimize(3)
            Pf = fresh.get_poses()
        if maxit == 8:
            assert d == 0 and st["pcg_converged"][0] == 0 and "pcg_maxit" in err, (d, st["pcg_converged"][:3], err)
            assert np.array_equal(Pi, P0)
            continue
        assert d == 3, (d, err, st["pcg_iters"][:3], st["pcg_relres"][:3])
        assert st["pcg_converged"][:3] == [2, 2, 2], st["pcg_converged"][:3]
        assert max(st["pcg_relres"][:3]) < 1e-11, st["pcg_relres"][:3]
        assert df == 3 and sf["pcg_converged"][:3] == [2, 2, 2], (df, sf["pcg_converged"][:3])
        for k in range(4):
            assert abs(st["chi2"][k] - sf["chi2"][k]) <= 1e-9 * sf["chi2"][k], (k, st["chi2"][k], sf["chi2"][k])
        assert np.abs(Pi - Pf).max() <= 1e-6, np.abs(Pi - Pf).max()
