"""tests/dogleg_reference.py, the numpy statement of sgo_optimize_dogleg's schedule (g2o 2020.5.29's OptimizationAlgorithmDogleg::solve;
DESIGN.md section 5o), and the two pure rules the library exports for it (sgo_dogleg_step_rule, sgo_dogleg_trial_rule:
rules::dogleg_step / dogleg_trial of sparse_gslam_amd/csrc/sgo_rules.h, the statements k_dl_trial and k_dl_decide compile), without
a GPU.

The reference: on tests/test_gpu_lm.py's graphs and starts, 8 iterations, it reproduces the trial patterns the feature was specified
with (G = Gauss-Newton step, D = blend, S = scaled Cauchy step); chi2 never rises; on the 600 / 620 dead-reckoned start every trial
is the GN step and three iterations are np_oracle.gauss_newton's chi2 to 1e-12; a reference with one constant changed (0.25, 0.75,
the factor 3, the beta branch) gives another trace, so a comparison against it notices.

The rules against the reference's per-trial records.  The step rule works from six scalars {b.b, b.g, g.g, b.Hb, b.Hg, g.Hg} where the
reference works on the vectors: the kind must be equal, |h| and the linear gain L agree to 1e-8 relative -- the forms are sums of
up to 7 500 products (relative error <= 1e-12 of the sum of their absolute values), and the recorded trials keep |g - alpha b|^2 and
L above 1e-4 of the terms they are differences of.  The trial rule takes the record's own numbers: accepted and delta after the
trial must be EQUAL (a halving and a maximum round nothing).  Then both rules at their branch points, on fabricated numbers."""
import functools
import math

import numpy as np
import pytest

import dogleg_reference as dr
import lm_reference as lr
from oracle import np_oracle
from sparse_gslam_amd import capi, synth

ITERS = 8
# name -> (V, E, seed, sigma, trials per iteration, the kinds)
CASES = {
    "300_400": (300, 400, 2, 2.0, [7, 1, 1, 2, 1, 1, 1, 1], "GGGGDDD D D DD D D D D"),
    "300_1200": (300, 1200, 5, 2.0, [7, 1, 1, 1, 1, 1, 1, 1], "GGGGGDD D D G G G G G"),
    "2500_3400": (2500, 3400, 31, 1.0, [3, 2, 1, 1, 1, 1, 1, 1], "GDD DD D D D D D D"),
}
# robust chi2 at the start and after 8 iterations, to three digits
CHI2 = {"300_400": (6.19e6, 1.71e6), "300_1200": (2.37e7, 2.08e5), "2500_3400": (2.32e7, 3.17e6)}


def _graph(V, E, seed, init="incremental"):
    g = synth.manhattan(V, E, seed, info_mode="full", init=init, phi=1.0)
    g.phi[:] = -1.0
    return g


@functools.lru_cache(maxsize=None)
def _case(name):
    V, E, seed, sigma = CASES[name][:4]
    g = _graph(V, E, seed)
    start = lr.perturbed(g, sigma)
    start.setflags(write=False)
    return g, start, dr.dogleg(start, *g.arrays()[1:], ITERS)


@pytest.mark.parametrize("name", list(CASES))
def test_the_trial_patterns_of_the_specification(name):
    g, start, ref = _case(name)
    trials, kinds = CASES[name][4:]
    assert ref["trials"] == trials and dr.pattern(ref) == kinds, (ref["trials"], dr.pattern(ref))
    assert ref["iters_done"] == ITERS and ref["stop_reason"] == dr.STOP_MAX_ITERS and ref["solves"] == ITERS
    assert ref["trials_total"] == len(ref["records"]) == sum(trials) > ITERS
    r = ref["robust_chi2"]
    assert all(a >= b for a, b in zip(r, r[1:])), r
    assert ref["chi2"] == r                                             # no kernel
    for got, want in zip((r[0], r[-1]), CHI2[name]):
        assert abs(got - want) <= 0.005 * want, (got, want)
    # the trace's own bookkeeping
    assert ref["step_kind"] == [rec["kind"] for rec in ref["records"] if rec["accepted"]]
    assert ref["delta"] == [rec["delta_after"] for rec in ref["records"] if rec["accepted"]]
    assert ref["delta0"] == ref["records"][0]["delta"] == 1e4 and ref["lam"] == 0.0


def test_gauss_newton_blows_up_where_dogleg_descends():
    g, start, ref = _case("300_400")
    _, gn = np_oracle.gauss_newton(start, *g.arrays()[1:], iters=2)
    assert gn["robust_chi2"][1] > 4e7 > ref["robust_chi2"][0] and gn["robust_chi2"][2] > 5e7


def test_a_mild_start_is_gauss_newton():
    g = _graph(600, 620, 3, init="odom")
    ref = dr.dogleg(*g.arrays(), 3)
    _, gn = np_oracle.gauss_newton(*g.arrays(), iters=3)
    assert ref["trials"] == [1, 1, 1] and dr.pattern(ref) == "G G G" and ref["step_kind"] == [dr.STEP_GN] * 3
    for k in ("chi2", "robust_chi2"):
        assert len(ref[k]) == len(gn[k]) == 4
        for a, b in zip(ref[k], gn[k]):
            assert abs(a - b) <= 1e-12 * b, (k, a, b)
    assert ref["robust_chi2"][3] < 1e-2 * ref["robust_chi2"][0]


@pytest.mark.parametrize("constants", [dict(lo=0.4), dict(hi=0.5), dict(grow=2.0), dict(grow=4.0)])
def test_a_mutated_constant_changes_the_trace(constants):
    changed = 0
    for name in CASES:
        g, start, ref = _case(name)
        mut = dr.dogleg(start, *g.arrays()[1:], ITERS, **constants)
        changed += mut["trials"] != ref["trials"] or mut["delta"] != ref["delta"] or dr.pattern(mut) != dr.pattern(ref)
    assert changed >= 1, constants


def test_the_beta_branch_matters_where_c_is_positive():
    """both expressions are roots of the same quadratic: with c > 0 the mutated reference takes the one that cancels, which differs in
    the last places on the recorded blends and visibly where c dominates"""
    g, start, ref = _case("300_400")
    mut = dr.dogleg(start, *g.arrays()[1:], ITERS, beta_by_sign=False)
    assert any(r["kind"] == dr.STEP_DL for r in ref["records"])
    assert [r["h_norm"] for r in mut["records"]] != [r["h_norm"] for r in ref["records"]] or mut["robust_chi2"] != ref["robust_chi2"]
    h_sd, h_gn = np.array([1.0, 0.0]), np.array([1.0 + 1e-9, 1e-3])     # c = 1e-9, |d|^2 = 1e-6: -c + D cancels nothing here ...
    a = dr.choose_step(h_gn * 1e3, h_sd, 2.0)[1]
    b = dr.choose_step(h_gn * 1e3, h_sd, 2.0, beta_by_sign=False)[1]
    assert abs(np.linalg.norm(a) - 2.0) <= 1e-15 * 2.0 + 4e-16           # ... the stated branch lands on the trust region
    assert np.allclose(a, b, rtol=1e-9)


# ---------------------------------------------------------------------------- the rules
@pytest.mark.parametrize("name", list(CASES))
def test_the_rules_against_every_recorded_trial(name):
    _, _, ref = _case(name)
    kinds = set()
    for rec in ref["records"]:
        kind, a, c, step_norm, gain = capi.dogleg_step_rule(rec["delta"], rec["forms"])
        assert kind == rec["kind"], rec
        assert abs(step_norm - rec["h_norm"]) <= 1e-8 * rec["h_norm"], (step_norm, rec)
        assert abs(gain - rec["L"]) <= 1e-8 * abs(rec["L"]), (gain, rec)
        if kind == capi.DL_STEP_GN:
            assert (a, c) == (0.0, 1.0) and step_norm == math.sqrt(rec["forms"][2])
        elif kind == capi.DL_STEP_SD:
            assert c == 0.0 and abs(step_norm - rec["delta"]) <= 1e-12 * rec["delta"]
        else:
            assert 0.0 < c < 1.0 and abs(step_norm - rec["delta"]) <= 1e-8 * rec["delta"]
        kinds.add(kind)
        for L, n in ((rec["L"], rec["h_norm"]), (gain, step_norm)):
            accepted, delta = capi.dogleg_trial_rule(rec["cur"], rec["tmp"], L, n, rec["delta"])
            assert accepted == rec["accepted"], rec
            if n == rec["h_norm"] or not rec["rho"] > 0.75:
                assert delta == rec["delta_after"], (delta, rec)
            else:
                assert abs(delta - rec["delta_after"]) <= 1e-8 * rec["delta_after"]
    assert {capi.DL_STEP_GN, capi.DL_STEP_DL} <= kinds


def _forms(b, g, H):
    b, g, H = np.asarray(b, float), np.asarray(g, float), np.asarray(H, float)
    return [b @ b, b @ g, g @ g, b @ H @ b, b @ H @ g, g @ H @ g]


def _step_check(b, g, H, delta):
    """the rule against the reference's vector arithmetic on a fabricated system -> the rule's tuple"""
    b, g, H = np.asarray(b, float), np.asarray(g, float), np.asarray(H, float)
    f = _forms(b, g, H)
    h_sd = (f[0] / f[3]) * b
    kind_ref, h = dr.choose_step(g, h_sd, delta)
    kind, a, c, step_norm, gain = capi.dogleg_step_rule(delta, f)
    assert kind == kind_ref
    assert np.allclose(a * b + c * g, h, rtol=1e-12, atol=1e-15)
    assert abs(step_norm - np.linalg.norm(h)) <= 1e-12 * np.linalg.norm(h)
    L = -(h @ H @ h) + 2.0 * (b @ h)
    if abs(L) >= 1e-12:
        assert abs(gain - L) <= 1e-12 * (abs(h @ H @ h) + 2.0 * abs(b @ h))
    return kind, a, c, step_norm, gain


def test_step_rule_at_the_norms_that_equal_delta():
    H = np.diag([1.0, 4.0])
    b = np.array([3.0, 4.0])
    g = np.linalg.solve(H, b)                                            # (3, 1): |g|^2 = 10
    alpha = 25.0 / 73.0                                                  # |h_sd| = 5 alpha
    # |h_gn| = delta exactly: `<` is strict, not the GN step
    g4 = np.array([0.0, 4.0])
    assert math.sqrt(g4 @ g4) == 4.0
    assert _step_check(b, g4, H, 4.0)[0] == capi.DL_STEP_DL
    assert _step_check(b, g4, H, math.nextafter(4.0, 5.0))[0] == capi.DL_STEP_GN
    # |h_sd| = delta exactly: `>` is strict, the blend (which starts at the Cauchy point: beta = 0 for c > 0)
    b1, H1 = np.array([2.0, 0.0]), np.diag([1.0, 1.0])                   # alpha = 1, h_sd = (2, 0)
    kind, a, c, n, _ = _step_check(b1, [3.0, 3.0], H1, 2.0)
    assert kind == capi.DL_STEP_DL and c == 0.0 and a == 1.0 and n == 2.0
    assert _step_check(b1, [3.0, 3.0], H1, math.nextafter(2.0, 0.0))[0] == capi.DL_STEP_SD
    # the three kinds on one system
    assert _step_check(b, g, H, 10.0)[0] == capi.DL_STEP_GN
    assert _step_check(b, g, H, 2.0)[0] == capi.DL_STEP_DL and 5.0 * alpha < 2.0
    kind, a, c, n, _ = _step_check(b, g, H, 0.5)
    assert kind == capi.DL_STEP_SD and c == 0.0 and abs(n - 0.5) <= 1e-15


def test_step_rule_on_both_signs_of_c():
    H = np.eye(2)                                                        # (the forms need not come from a solve: the PCG's g is inexact)
    b = np.array([1.0, 0.0])                                             # alpha = 1, h_sd = b
    for g, sign in (([0.5, 3.0], -1), ([1.0, 3.0], 0), ([2.0, 3.0], 1)):
        g = np.array(g)
        c = b @ (g - b)
        assert np.sign(c) == sign
        kind, a, cc, n, _ = _step_check(b, g, H, 2.0)
        assert kind == capi.DL_STEP_DL and abs(n - 2.0) <= 4e-16 * 2.0 and 0.0 < cc < 1.0


def test_step_rule_floors_a_vanishing_gain():
    for bg, gHg, want in ((1e-14, 1e-14, 1e-12), (1e-14, 3e-14, 1e-12), (0.0, 0.0, 1e-12), (1.0, 1.0, 1.0), (1.0, 3.0, -1.0)):
        kind, a, c, n, gain = capi.dogleg_step_rule(10.0, [1.0, bg, 1.0, 1.0, bg, gHg])
        assert kind == capi.DL_STEP_GN and gain == want, (bg, gHg, gain)


def _trial_check(cur, tmp, L, n, delta):
    accepted, after = capi.dogleg_trial_rule(cur, tmp, L, n, delta)
    rho, acc_ref, after_ref = dr.decide(cur, tmp, L, n, delta)
    assert accepted == acc_ref and after == after_ref, (cur, tmp, L, n, delta, rho)
    return accepted, after


def test_trial_rule_at_its_branch_points():
    assert _trial_check(10.0, 10.0, 2.0, 1.0, 8.0) == (False, 4.0)                     # rho = 0 exactly: rejected, halved
    assert _trial_check(10.0, math.nextafter(10.0, 0.0), 2.0, 1.0, 8.0) == (True, 4.0)  # just above: accepted, still < 0.25
    assert _trial_check(1.0, 0.75, 1.0, 1.0, 8.0) == (True, 8.0)                       # rho = 0.25 exactly: not < 0.25
    assert _trial_check(1.0, math.nextafter(0.75, 1.0), 1.0, 1.0, 8.0) == (True, 4.0)
    assert _trial_check(1.0, 0.25, 1.0, 5.0, 8.0) == (True, 8.0)                       # rho = 0.75 exactly: not > 0.75
    assert 1.0 - 0.25 + 2.0 ** -53 == math.nextafter(0.75, 1.0)
    assert _trial_check(1.0, 0.25 - 2.0 ** -53, 1.0, 5.0, 8.0) == (True, 15.0)         # one ulp above: max(delta, 3 |h|)
    assert _trial_check(1.0, 0.0, 1.0, 1.0, 8.0) == (True, 8.0)                        # ... a maximum: 3 |h| < delta keeps delta
    assert _trial_check(10.0, 11.0, 2.0, 1.0, 8.0) == (False, 4.0)
    assert _trial_check(10.0, 11.0, -2.0, 1.0, 8.0) == (True, 8.0)                     # a negative gain turns a rise into rho = 0.5 > 0 (g2o's)
    # |L| < 1e-12 is L = 1e-12
    assert _trial_check(1.0, 1.0 - 1e-12, 1e-14, 1.0, 8.0) == (True, 8.0)              # rho = 1 - ..., not 100
    assert _trial_check(1.0, 1.0 - 1e-12, -1e-14, 1.0, 8.0)[0] is True


def test_trial_rule_on_non_finite_numbers():
    for tmp in (math.nan, math.inf, -math.inf):
        assert _trial_check(10.0, tmp, 2.0, 1.0, 8.0) == (False, 4.0)                  # -inf would be rho = +inf: still rejected
    assert _trial_check(math.nan, 9.0, 2.0, 1.0, 8.0) == (False, 4.0)
    assert _trial_check(10.0, 9.0, math.nan, 1.0, 8.0) == (False, 4.0)
    delta = 1e4
    for q in range(100):                                                               # a hundred such trials shrink, never stall
        delta = _trial_check(10.0, math.nan, 2.0, 1.0, delta)[1]
    assert delta == 1e4 * 2.0 ** -100
