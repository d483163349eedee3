"""The leave-one-out statistic on the CPU (tests/loo_reference.py; no GPU):
 * the INPUT CONDITION of the device tests: the closed forms (P from solves with the full H) and the explicit leave-out (H_
   factorised, the linear step taken, the candidate gate's formula) agree on the reference alone, for edges with lambda_min >= 1e-2,
   to 1e-9 (measured: <= 3e-12 in d2 and <= 3e-13 in cov_loo on 2500 / 3400 over 302 sampled edges, 8e-12 on 600 / 620, <= 2e-13 on the
   small cases; here every 37th edge of 2500 / 3400 is taken out, a factorisation each);
 * sgo_edge_loo_rule -- the text the kernel compiles -- against numpy's cholesky and eigh;
 * the motivating case: a shifted closure that the raw chi2 gate lets through has the largest d2 of its graph, and one number
   means the same with and without DCS."""
import numpy as np
import pytest

import loo_reference as lr
import mfront_cases as mc
from oracle import np_oracle as npo
from sparse_gslam_amd import capi, synth

CONDITION = 1e-9
_CACHE = {}


def _small(name):
    c = mc.make(name)
    return c, npo.gauss_newton(*c.arrays(), iters=20)[0]


def _state(key):
    """(graph or case, Edges at the poses after gauss_newton(20)): computed once, shared, never modified"""
    if key not in _CACHE:
        if key in mc.NAMES:
            g, P = _small(key)
        elif key == "motivating" or key == "motivating_none":
            g, _ = lr.motivating_graph()
            if key == "motivating_none":
                g.phi = np.full(g.E, -1.0)
            else:
                g.phi = np.where(np.arange(g.E) >= g.V - 1, 10.0, -1.0)
            P, _ = npo.gauss_newton(*g.arrays(), iters=20)
        else:
            V, E, seed = key
            g = synth.manhattan(V, E, seed=seed, info_mode="full")
            P, _ = npo.gauss_newton(*g.arrays(), iters=20)
        _CACHE[key] = (g, lr.Edges(P, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi))
    return _CACHE[key]


@pytest.fixture(autouse=True)
def _the_library_has_the_statistic():
    """the reference qualifies a statistic the library computes: without its entry points nothing here says anything"""
    for name in ("sgo_edge_leave_one_out", "sgo_edge_loo_rule"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name


def test_symbols_are_bound():
    assert callable(capi.edge_loo_rule) and callable(capi.Optimizer.edge_leave_one_out)


@pytest.mark.parametrize("key,stride", [("contributions", 1), ("tree_shapes", 1), ("dcs_switches_closures_off", 1), ((600, 620, 3), 1),
                                        ((2500, 3400, 31), 37)], ids=str)
def test_two_routes_agree(key, stride):
    g, S = _state(key)
    edges = np.arange(0, S.ei.size, stride)
    F = lr.by_formulas(S, edges)
    worst_d2 = worst_cov = 0.0
    compared = 0
    for t, k in enumerate(edges):
        if not (F["redundancy"][t] >= 1e-2) or not S.O[k].any():
            continue
        d2, Pm = lr.by_leaving_out(S, k)
        worst_d2 = max(worst_d2, abs(d2 - F["d2"][t]) / max(abs(d2), 1e-300))
        worst_cov = max(worst_cov, np.abs(Pm - F["cov_loo"][t]).max() / np.abs(Pm).max())
        compared += 1
    print(f"{key}: {compared} of {edges.size} edges compared, worst d2 {worst_d2:.3g}, worst cov_loo {worst_cov:.3g}")
    assert compared >= 10
    assert worst_d2 <= CONDITION and worst_cov <= CONDITION, (worst_d2, worst_cov)


def test_redundancy_is_in_the_unit_interval_and_bridges_sit_at_zero():
    g, S = _state("dcs_switches_closures_off")
    F = lr.by_formulas(S, np.arange(S.ei.size))
    assert F["redundancy"].min() >= -1e-9 and F["redundancy"].max() <= 1.0 + 1e-12
    assert (np.abs(F["redundancy"]) < 1e-6).sum() >= 40          # the chain stretches inside no loop
    assert F["w"].min() < 1e-6                                   # DCS switches closures off: the weights the rule must survive


# ---------------------------------------------------------------------------- the rule against numpy
def _random_case(rng, w, nus, cond):
    """Omega with condition number ~cond, N = Q diag(nus) Q^T in Omega's Cholesky frame, hence P = G^-T N G^-1"""
    Q1, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    O = (Q1 * np.logspace(0, np.log10(cond), 3) * rng.uniform(0.5, 2.0)) @ Q1.T
    O = 0.5 * (O + O.T)
    G = np.linalg.cholesky(O)
    Q2, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    N = (Q2 * np.asarray(nus)) @ Q2.T
    Gi = np.linalg.inv(G)
    P = Gi.T @ N @ Gi
    return O, 0.5 * (P + P.T), rng.standard_normal(3) * 0.1


def _info6(O):
    return np.array([O[0, 0], O[0, 1], O[0, 2], O[1, 1], O[1, 2], O[2, 2]])


@pytest.mark.parametrize("w", [0.0, 4e-9, 0.033, 0.5, 1.0])
def test_rule_against_numpy(w):
    rng = np.random.default_rng(int(w * 1e9) + 5)
    worst = dict(d2=0.0, cov=0.0, red=0.0)
    for trial in range(200):
        kind = trial % 4
        if kind == 0:
            nus = rng.uniform(0.0, 0.9, 3)
        elif kind == 1:
            a = rng.uniform(0.05, 0.9)
            nus = np.array([a, a, rng.uniform(0.0, 0.9)])        # two equal eigenvalues
        elif kind == 2:
            nus = np.full(3, rng.uniform(0.05, 0.9))             # a multiple of the identity in Omega's frame
        else:
            nus = rng.uniform(0.0, 0.9, 3) * 10.0 ** rng.uniform(-6, np.log10(min(1e3, 1.0 / max(w, 1e-300))))   # w nu < 0.9, ||N|| up to 900
        O, P, e = _random_case(rng, w, nus, cond=10.0 ** rng.uniform(0, 3))
        ref = lr.closed_forms(O, P, e, w)
        rc, d2, red, cov = capi.edge_loo_rule(_info6(O), P, e, w)
        assert rc == 0
        worst["d2"] = max(worst["d2"], abs(d2 - ref["d2"]) / abs(ref["d2"]))
        scale = np.abs(ref["cov_loo"]).max()
        if scale > 0.0:
            worst["cov"] = max(worst["cov"], np.abs(cov - ref["cov_loo"]).max() / scale)
        worst["red"] = max(worst["red"], abs(red - ref["redundancy"]) / max(1.0, w * ref["normN"]))
        assert np.array_equal(cov, cov.T)
    print(f"w = {w}: worst relative d2 {worst['d2']:.3g}, cov_loo {worst['cov']:.3g}, redundancy {worst['red']:.3g}")
    assert worst["d2"] <= 1e-12 and worst["cov"] <= 1e-12 and worst["red"] <= 1e-12, worst


def test_rule_limits():
    """w = 1: the normalised-residual test e^T (Omega^-1 - P)^-1 e; w = 0: the candidate gate's e^T (Omega^-1 + P)^-1 e, cov_loo = P"""
    rng = np.random.default_rng(9)
    for _ in range(50):
        O, P, e = _random_case(rng, 1.0, rng.uniform(0.0, 0.8, 3), cond=30.0)
        Oi = np.linalg.inv(O)
        _, d2, _, cov = capi.edge_loo_rule(_info6(O), P, e, 1.0)
        assert d2 == pytest.approx(e @ np.linalg.solve(Oi - P, e), rel=1e-10)
        _, d2, red, cov = capi.edge_loo_rule(_info6(O), P, e, 0.0)
        assert d2 == pytest.approx(e @ np.linalg.solve(Oi + P, e), rel=1e-10)
        assert red == 1.0 and np.allclose(cov, P, rtol=1e-10, atol=0.0)


def test_rule_zero_and_indefinite_information():
    P = np.array([[2.0, 0.3, 0.1], [0.3, 1.0, 0.2], [0.1, 0.2, 0.5]])
    e = np.array([0.1, -0.2, 0.05])
    rc, d2, red, cov = capi.edge_loo_rule(np.zeros(6), P, e, 1.0)
    assert rc == 1 and d2 == 0.0 and red == 1.0 and np.array_equal(cov, P)
    for bad in ([1.0, 2.0, 0.0, 1.0, 0.0, 1.0], [-1.0, 0.0, 0.0, 1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 1.0, 1.0, 1.0]):
        rc, d2, red, cov = capi.edge_loo_rule(np.array(bad), P, e, 0.5)
        assert rc == 2 and np.isnan(d2) and np.isnan(red) and np.isnan(cov).all(), bad
    # cov_loo is optional
    L = capi.lib()
    import ctypes as C
    d2c, redc = C.c_double(), C.c_double()
    O = np.array([4.0, 0.0, 0.0, 4.0, 0.0, 4.0])
    assert L.sgo_edge_loo_rule(capi._dp(O), capi._dp(np.zeros(9)), capi._dp(e), 1.0, C.byref(d2c), C.byref(redc), None) == 0
    assert d2c.value == pytest.approx(4.0 * e @ e, rel=1e-14) and redc.value == 1.0


# ---------------------------------------------------------------------------- the motivating case
def test_motivating_case():
    g, bad = lr.motivating_graph()
    _, S0 = _state("motivating_none")
    F0 = lr.by_formulas(S0, np.arange(g.E))
    assert S0.e2[bad] < 11.345 < F0["d2"][bad], (S0.e2[bad], F0["d2"][bad])
    ok = F0["redundancy"] >= 1e-3
    assert ok[bad] and np.nanargmax(np.where(ok, F0["d2"], -1.0)) == bad
    _, S1 = _state("motivating")
    F1 = lr.by_formulas(S1, [bad])
    print(f"edge {bad}: no kernel e2 {S0.e2[bad]:.4g} d2 {F0['d2'][bad]:.4g}; DCS w {S1.w[bad]:.3g} e2 {S1.e2[bad]:.4g} d2 {F1['d2'][0]:.4g}")
    assert abs(F1["d2"][0] - F0["d2"][bad]) < 0.05 * F0["d2"][bad]
