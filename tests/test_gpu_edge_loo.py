"""The leave-one-out test of every resident edge from one selected inversion (sgo_edge_leave_one_out; kernel in
sparse_gslam_amd/csrc/sgo_loo.hip, driver in sgo_loo.cpp, the rule in sgo_rules.h).

Reference: tests/loo_reference.py's closed forms with P from SuperLU solves of np_oracle's robustified Hessian AT THE DEVICE'S
POSES (tests/test_loo_reference.py qualifies it against the explicit leave-out on the CPU).

Bars.  The project's 1e-6 relative bar for solver-dependent quantities (tests/test_gpu_marginals.py BAR), amplified by 1 / lambda
with lambda = the REFERENCE's lambda_min of I - w N, on the edges with lambda >= 5e-3:
    d2          |d2 - ref| <= (1e-6 / lambda) d2_ref + 1e-12
    cov_loo     the same on its max-norm
    redundancy  |delta| <= 1e-6 max(1, w ||N||)
The cap is a condition: at least 80 % of each graph's closures must be compared.  Edges whose reference lambda is below 1e-6
(bridges) must come back NaN with fail = 0 at min_redundancy = 1e-3.  Every test prints what it measured."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loo_reference as lr
import mfront_cases as mc
import robust_reference as rr
from sparse_gslam_amd import capi
from test_gpu_hypotheses import DIRECT, MFRONT, PCG, bits, graph, same_bits
from test_gpu_marginals import BAR
from test_shim_replay import _write_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE, MIN_RED, CAP, BRIDGE = 11.345, 1e-3, 5e-3, 1e-6
SENTINEL = -777.25


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _compare(name, g, opt, edges, w=None, min_compared=0.8):
    """The device's answers for `edges` against the reference at the device's poses -> (reference, device d2, redundancy, fail)"""
    edges = np.asarray(edges, dtype=np.int32)
    S = lr.Edges(opt.get_poses(), g.fixed, g.ei, g.ej, g.meas, g.info, g.phi, w=w)
    F = lr.by_formulas(S, edges)
    nfail, d2, red, cov, fail = opt.edge_leave_one_out(edges, GATE, MIN_RED)
    lam = F["redundancy"]
    cmp_ = lam >= CAP
    closure = np.abs(np.asarray(g.ei)[edges].astype(np.int64) - np.asarray(g.ej)[edges]) != 1
    share = cmp_[closure].sum() / max(closure.sum(), 1)
    r_d2 = np.abs(d2[cmp_] - F["d2"][cmp_]) / ((BAR / lam[cmp_]) * F["d2"][cmp_] + 1e-12)
    cn = np.abs(F["cov_loo"][cmp_]).reshape(-1, 9).max(1)
    r_cov = np.abs(cov[cmp_] - F["cov_loo"][cmp_]).reshape(-1, 9).max(1) / ((BAR / lam[cmp_]) * cn + 1e-12)
    fin = np.isfinite(lam)
    r_red = np.abs(red[fin] - lam[fin]) / (BAR * np.maximum(1.0, F["w"][fin] * F["normN"][fin]))
    bridge = lam < BRIDGE
    print(f"{name}: {cmp_.sum()} of {edges.size} edges compared ({cmp_[closure].sum()} of {closure.sum()} closures, smallest lambda "
          f"{lam[closure].min() if closure.any() else float('nan'):.3g}), {bridge.sum()} bridges, smallest w {F['w'].min():.3g}; ratios to the bars: d2 "
          f"{r_d2.max():.3g}, cov_loo {r_cov.max():.3g}, redundancy {r_red.max():.3g}")
    assert share >= min_compared, (name, share)
    assert r_d2.max() <= 1.0 and r_cov.max() <= 1.0 and r_red.max() <= 1.0, (name, r_d2.max(), r_cov.max(), r_red.max())
    assert np.isnan(d2[bridge]).all() and np.isnan(cov[bridge]).all() and not fail[bridge].any()
    decided = red >= MIN_RED
    assert np.array_equal(fail, decided & (d2 > GATE)) and nfail == int(fail.sum())
    assert np.isnan(d2[~decided]).all() and np.isfinite(d2[decided]).all()
    assert np.array_equal(bits(cov), bits(cov.transpose(0, 2, 1).copy()))
    return F, d2, red, fail


@pytest.mark.parametrize("name", ["contributions", "tree_shapes", "dcs_switches_closures_off"])
def test_cases_of_the_stage_tests(name):
    c = mc.make(name)
    with mc.environment(c.env), capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(*c.arrays())
        assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
        assert o.optimize(20)[0] == 20
        F, d2, red, fail = _compare(name, c, o, np.arange(c.ei.size))
        e2 = o.edge_chi2()
    if name == "contributions":
        both = np.flatnonzero(c.fixed[c.ei] & c.fixed[c.ej])
        assert both.size == 1
        assert abs(d2[both[0]] - e2[both[0]]) <= 1e-12 * e2[both[0]] and red[both[0]] == 1.0
        # duplicates of one pair in both orientations were answered through the same stored block: all compared above
        assert ((c.ei == 12) & (c.ej == 40)).sum() == 3 and ((c.ei == 40) & (c.ej == 12)).sum() == 2
    if name == "dcs_switches_closures_off":
        assert F["w"].min() < 1e-6 and (F["redundancy"] < BRIDGE).sum() >= 40


@pytest.mark.parametrize("shape,path", [(DIRECT, "direct_ldlt"), (MFRONT, "multifrontal_cholesky")], ids=["direct", "mfront"])
def test_mid_size_graphs(shape, path):
    g = graph(shape)
    closures = np.flatnonzero(np.abs(g.ei.astype(np.int64) - g.ej) != 1)
    edges = np.arange(g.E) if shape == DIRECT else np.r_[closures[::3], np.arange(0, g.V - 1, 25)]
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        assert o.solver_description().startswith(path), o.solver_description()
        assert o.optimize(20)[0] == 20
        desc = o.solver_description()
        _compare(str(shape), g, o, edges)
        assert o.solver_description() == desc


def test_cov_loo_is_the_candidate_gates_prediction_without_the_edge():
    """At unchanged poses: the edge's information is zeroed, the edge offered to sgo_candidate_gate -- its cov_pred is cov_loo"""
    g = graph(MFRONT)
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.optimize(20)
        closures = np.flatnonzero(np.abs(g.ei.astype(np.int64) - g.ej) != 1)
        _, _, red, cov, _ = o.edge_leave_one_out(closures, GATE, MIN_RED)
        pick = closures[np.argsort(-red)[[0, 40, 200]]]
        _, _, red, cov, _ = o.edge_leave_one_out(pick, GATE, MIN_RED)
        for t, k in enumerate(pick):
            o.set_edge_information([k], np.zeros((1, 6)))
            _, _, P, _ = o.candidate_gate(g.ei[[k]], g.ej[[k]], g.meas[[k]], g.info[[k]], GATE)
            o.set_edge_information([k], g.info[[k]])
            ratio = np.abs(P[0] - cov[t]).max() / ((BAR / red[t]) * np.abs(P[0]).max() + 1e-12)
            print(f"edge {k}: redundancy {red[t]:.3g}, |cov_pred - cov_loo| at {ratio:.3g} of the bar")
            assert ratio <= 1.0


def test_the_motivating_graph():
    """A closure shifted by 0.4 m passes the raw chi2 gate after the fit and has the largest leave-one-out d2 of its graph"""
    g, bad = lr.motivating_graph()
    g.phi = np.full(g.E, -1.0)
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        assert o.optimize(20)[0] == 20
        F, d2, red, fail = _compare("motivating", g, o, np.arange(g.E))
        e2 = o.edge_chi2()
        assert e2[bad] < GATE < d2[bad] and fail[bad] and np.nanargmax(d2) == bad
        print(f"edge {bad}: e2 {e2[bad]:.4g}, d2 {d2[bad]:.4g} (reference {F['d2'][bad]:.4g}), {int(fail.sum())} edges fail")
        k, gated = o.gate_edges(np.arange(g.E), GATE)
        assert k == 0 and not gated.any()


def test_mixed_kernel_kinds():
    g = graph(MFRONT)
    cl = np.flatnonzero(g.phi >= 0)
    kind = np.zeros(g.E, dtype=np.int32)
    kind[cl] = np.array([rr.DCS, rr.HUBER, rr.CAUCHY, rr.TUKEY])[np.arange(cl.size) % 4]
    delta = np.where(g.phi >= 0, 1.5, 1.0)
    delta[kind == rr.DCS] = 10.0
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.set_robust_kernels(np.arange(g.E), kind, delta)
        assert o.optimize(20)[0] == 20
        S0 = lr.Edges(o.get_poses(), g.fixed, g.ei, g.ej, g.meas, g.info, np.full(g.E, -1.0))
        w = rr.rho_mixed(kind, S0.e2, delta)[1]
        _, wd = o.edge_robust()
        assert np.abs(wd - w).max() <= 1e-9 and (w[cl] < 0.999).sum() >= 20, (np.abs(wd - w).max(), (w[cl] < 0.999).sum())
        _compare("mixed kinds", g, o, np.r_[cl[::3], np.arange(0, g.V - 1, 25)], w=w)


def test_the_analysis_refusing_the_graph_returns_enothing():
    g = graph(PCG)
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*g.arrays())
        o.optimize(2)
        for _ in range(2):
            with pytest.raises(capi.SgoError, match="rc=-1"):
                o.edge_leave_one_out(None, GATE, MIN_RED)
            assert "sgo_optimize_gn_hypotheses" in o.last_error(), o.last_error()
        assert o.optimize(2)[0] == 2


def test_contracts_of_the_call():
    g = graph(MFRONT)
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.optimize(20)
        ids = np.arange(g.E, dtype=np.int32)
        A = o.edge_leave_one_out(None, GATE, MIN_RED)
        B = o.edge_leave_one_out(ids, GATE, MIN_RED)
        for a, b in zip(A[1:4], B[1:4]):                                   # same bits twice, with and without ids
            assert same_bits(a, b)
        assert A[0] == B[0] and np.array_equal(A[4], B[4])
        pick = np.array([3001, 7, 3001, 2600, 0, 3399], dtype=np.int32)    # another n, other places, one id twice
        Cc = o.edge_leave_one_out(pick, GATE, MIN_RED)
        for a, c in zip(A[1:4], Cc[1:4]):
            assert same_bits(a[pick], c)
        assert np.array_equal(A[4][pick], Cc[4]) and Cc[0] == int(Cc[4].sum())
        # a deactivated edge: 0 / 1 / no fail; the others see a graph without it
        k = int(np.flatnonzero((g.phi >= 0) & (A[2] > 0.2))[5])
        o.set_edge_information([k], np.zeros((1, 6)))
        _, d2, red, cov, fail = o.edge_leave_one_out([k, 0], GATE, MIN_RED)
        assert d2[0] == 0.0 and red[0] == 1.0 and not fail[0] and np.isfinite(cov[0]).all()
        assert np.abs(cov[0] - A[3][k]).max() <= (BAR / A[2][k]) * np.abs(A[3][k]).max()      # P of the graph without it = its cov_loo
        o.set_edge_information([k], g.info[[k]])
        assert same_bits(o.edge_leave_one_out(pick, GATE, MIN_RED)[1], Cc[1])


def test_marginals_selected_keeps_its_bits_around_the_call():
    g = graph(DIRECT)
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.optimize(20)
        vi, vj = g.ei[g.V - 1:g.V + 9], g.ej[g.V - 1:g.V + 9]
        D0, c0 = o.marginals_selected(vi, vj)
        o.edge_leave_one_out(None, GATE, MIN_RED)
        D1, c1 = o.marginals_selected(vi, vj)
        assert same_bits(D0, D1) and same_bits(c0, c1)


@pytest.mark.parametrize("shape,path", [(DIRECT, "direct_ldlt"), (MFRONT, "multifrontal_cholesky")], ids=["direct", "mfront"])
def test_a_later_optimize_has_the_bits_of_a_context_that_never_called(shape, path):
    g = graph(shape)
    with capi.Optimizer(0) as opt, capi.Optimizer(0) as fresh:
        for o in (opt, fresh):
            o.set_graph(*g.arrays())
            assert o.solver_description().startswith(path)
        a = [opt.optimize(5)]
        opt.edge_leave_one_out(None, GATE, MIN_RED)
        a.append(opt.optimize(5))
        b = [fresh.optimize(5), fresh.optimize(5)]
        assert same_bits(opt.get_poses(), fresh.get_poses())
        if shape == MFRONT:
            assert same_bits(opt.mfront_arrays(("X",))["X"], fresh.mfront_arrays(("X",))["X"])
    for (d, st), (df, sf) in zip(a, b):
        assert d == df == 5 and st["chi2"] == sf["chi2"] and st["robust_chi2"] == sf["robust_chi2"]


def _raw(o, n, ids, chi2, min_red, d2, red, cov, fail, null_d2=False):
    return capi.lib().sgo_edge_leave_one_out(o._h, n, None if ids is None else capi._ip(ids), chi2, min_red, None if null_d2 else capi._dp(d2),
                                             capi._dp(red), capi._dp(cov), _u8(fail))


def test_refusals_leave_the_outputs_untouched():
    g = graph(DIRECT)
    n = 4
    d2, red, cov, fail = (np.full(n, SENTINEL), np.full(n, SENTINEL), np.full((n, 9), SENTINEL), np.full(n, 7, dtype=np.uint8))
    ok = np.arange(n, dtype=np.int32)
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.optimize(3)
        P = o.get_poses()
        refusals = [(-1, ok, GATE, MIN_RED, False), (n, ok, GATE, MIN_RED, True), (n, np.array([0, 1, g.E, 2], dtype=np.int32), GATE, MIN_RED, False),
                    (n, np.array([0, -1, 1, 2], dtype=np.int32), GATE, MIN_RED, False), (n, ok, np.inf, MIN_RED, False), (n, ok, np.nan, MIN_RED, False),
                    (n, ok, GATE, 0.0, False), (n, ok, GATE, -0.5, False), (n, ok, GATE, 1.5, False), (n, ok, GATE, np.nan, False),
                    (g.E + 1, None, GATE, MIN_RED, False)]
        for nn, ids, chi2, mr, null in refusals:
            assert _raw(o, nn, ids, chi2, mr, d2, red, cov, fail, null) == -2, (nn, ids, chi2, mr, null)
            assert "sgo_edge_leave_one_out" in o.last_error()
        assert np.all(d2 == SENTINEL) and np.all(red == SENTINEL) and np.all(cov == SENTINEL) and np.all(fail == 7)
        assert same_bits(o.get_poses(), P)
        assert _raw(o, n, ok, GATE, 1.0, d2, red, cov, fail) >= 0 and np.all(d2 != SENTINEL)            # min_redundancy = 1 is allowed
        assert _raw(o, 0, ok, GATE, MIN_RED, d2, red, cov, fail) == 0
    with capi.Optimizer(0) as o:
        assert _raw(o, n, ok, GATE, MIN_RED, d2, red, cov, fail) == -4                                   # no graph
    d2[:] = SENTINEL
    with capi.Optimizer(0, direct_rows=0, solver=capi.SOLVER_PCG_BJ) as o:                               # a multi-GPU context's emulation
        o.debug_set_shard(2, 0)
        o.set_graph(*g.arrays())
        assert _raw(o, n, ok, GATE, MIN_RED, d2, red, cov, fail) == -2 and "multi-GPU" in o.last_error()
    assert np.all(d2 == SENTINEL)


def test_an_active_overlay_is_refused():
    from test_gpu_edge_gate import _grow, _overlay_session
    base, steps, gg = _overlay_session()[:3]
    d2 = np.full(4, SENTINEL)
    with capi.Optimizer(0, direct_rows=0) as o:
        _grow(o, base, steps, gg, 6)
        assert "incremental overlay" in o.solver_description()
        rc = capi.lib().sgo_edge_leave_one_out(o._h, 4, None, GATE, MIN_RED, capi._dp(d2), None, None, None)
        assert rc == -2 and "overlay" in o.last_error() and np.all(d2 == SENTINEL)


def test_an_indefinite_hessian_fails_and_leaves_the_outputs():
    """the failure path of test_gpu_selinv.py's indefinite graph (negated information: a pivot block fails its test, no fault)"""
    import test_gpu_mfront as tmf
    g = tmf.chain_graph(700, 150, seed=16)
    info = g.info.copy()
    info[:, [0, 3, 5]] *= -1.0
    d2, red, cov, fail = (np.full(4, SENTINEL), np.full(4, SENTINEL), np.full((4, 9), SENTINEL), np.full(4, 7, dtype=np.uint8))
    with capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)
        assert o.solver_description().startswith("multifrontal_cholesky")
        rc = _raw(o, 4, None, GATE, MIN_RED, d2, red, cov, fail)
        assert rc == -2 and "not positive definite" in o.last_error(), (rc, o.last_error())
        assert np.all(d2 == SENTINEL) and np.all(red == SENTINEL) and np.all(cov == SENTINEL) and np.all(fail == 7)
        rc, st = o.optimize(5)                           # as without the call: fails at iteration 0, the estimates stay
        assert rc == 0 and st["iters_done"] == 0 and np.array_equal(o.get_poses(), g.poses)


# ------------------------------------------------------------------ the compat headers
@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    """replay_edge_loo, built with the g++ line test_gpu_fsolve.py uses"""
    libdir = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("replay_edge_loo") / "replay_edge_loo")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "replay_edge_loo.cpp"), "-L" + libdir, "-lsgo", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_the_call_through_the_compat_headers(replay, tmp_path):
    """SparseOptimizer::sgoEdgeLeaveOneOut returns the C-ABI call's bits for every edge at the same estimates, and -1 for an edge
    that is not active, after an addVertex without initializeOptimization, under the host Levenberg solver and when the call refuses"""
    g = graph(DIRECT)
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 10.0)
    env = dict(os.environ)
    for k in ("SGO_DIRECT_ROWS", "SGO_INCREMENTAL", "SGO_SOLVER"):
        env.pop(k, None)
    res = subprocess.run([replay, str(gf), str(of), "8", repr(GATE), repr(MIN_RED)], env=env, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    lines = open(of).read().split("\n")
    assert int(lines[0]) == 8 and lines[1].startswith("direct_ldlt") and lines[2] == lines[1], lines[:3]
    P = np.array([[float(v) for v in ln.split()] for ln in lines[3:3 + g.V]])
    rows = [ln.split() for ln in lines[3 + g.V:] if ln and ln.split()[0] == "edge"]
    tail = dict(ln.split() for ln in lines[3 + g.V:] if ln and ln.split()[0] in ("nfail", "not_active", "stale", "levenberg", "refused"))
    assert len(rows) == g.E
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P)
        nfail, d2, red, _, fail = opt.edge_leave_one_out(None, GATE, MIN_RED)
    # (equal values: the text carries 17 digits; a NaN's sign and payload do not survive it)
    assert np.array_equal(np.array([float(r[2]) for r in rows]), d2, equal_nan=True) and np.array_equal(np.array([float(r[3]) for r in rows]), red)
    assert np.array_equal(np.array([int(r[4]) for r in rows], dtype=bool), fail) and int(tail["nfail"]) == nfail
    assert all(int(tail[k]) == -1 for k in ("not_active", "stale", "levenberg", "refused")), tail
    said = [ln for ln in res.stderr.split("\n") if "sgoEdgeLeaveOneOut" in ln]
    assert len(said) == 4, res.stderr
