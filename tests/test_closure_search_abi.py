"""sgo_closure_search and sgo_closure_search_rule (include/sgo.h) are declared, bound and exported; the pure pair rule
(rules::closure_search of sgo_rules.h, the text k_closure_search compiles too) against numpy through ctypes, no device; the refusals
that need none.

Bars (tests/search_reference.py): |P - P_np|_max <= RULE_BAR scale, the same relative bar on rel, and for m2 and sigma the bar
carried through u^T P u: relative error 2 RULE_BAR scale / (u^T P u) (for sigma_lin through lambda_max, for sigma_ang through
P_phiphi; a square root halves a relative error, which the factor 2 covers).  m2's numerator adds 8 eps |t| / (|t| - radius): the two
roundings of |t|, amplified by the difference and squared."""
import ctypes as C
import os
import re

import numpy as np

import search_reference as sr
from sparse_gslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sgo_closure_search", "sgo_closure_search_rule")
SENTINEL = -777.25


def test_the_two_symbols_are_declared_bound_and_exported(sgo_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgo.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in capi.SYMBOLS and hasattr(sgo_lib, name), name
    assert sgo_lib.sgo_version() == 107
    assert callable(capi.Optimizer.closure_search) and callable(capi.closure_search_rule)


def _joint(rng, spread):
    """a random SPD 6 x 6 joint covariance of (x_j, x_c) with entries around spread^2"""
    M = rng.standard_normal((6, 6)) * spread
    return M @ M.T + 1e-6 * spread * spread * np.eye(6)


def _against_numpy(xj, xc, Sjj, Sjc, Scc, radius):
    """the library's pair rule against search_reference.pair on identical inputs -> the ratios to the bars (P, rel, m2, sigma)"""
    rel, P, m2, sg = capi.closure_search_rule(xj, xc, Sjj, Sjc, Scc, radius)
    r = sr.pair(xj, xc, Sjj, Sjc, Scc, radius)
    assert np.array_equal(P.view(np.uint64), P.T.copy().view(np.uint64)), P            # exactly symmetric, bit for bit
    scale = r["scale"]
    rp = np.abs(P - r["P"]).max() / (sr.RULE_BAR * scale) if scale > 0 else float(np.abs(P).max() > 0)
    rr = np.abs(rel - r["rel"]).max() / (sr.RULE_BAR * max(1.0, np.abs(r["rel"]).max()))
    if r["m2"] == 0.0 or np.isinf(r["m2"]):
        rm = 0.0 if m2 == r["m2"] else np.inf
    else:
        # the numerator's share: |t| carries two roundings, which the difference |t| - radius amplifies by |t| / excess, squared
        norm = float(np.hypot(r["rel"][0], r["rel"][1]))
        rm = abs(m2 - r["m2"]) / r["m2"] / (2.0 * sr.RULE_BAR * scale / r["den"] + 8.0 * 2.0**-52 * norm / (norm - radius))
    rs = 0.0
    for k, var in enumerate((r["sigma"][0] ** 2, r["P"][2, 2])):
        if var > 0.0:
            rs = max(rs, abs(sg[k] - r["sigma"][k]) / r["sigma"][k] / (2.0 * sr.RULE_BAR * scale / var))
        else:
            assert sg[k] == 0.0
    return rp, rr, rm, rs


def test_rule_against_numpy_on_random_joint_covariances():
    rng = np.random.default_rng(2024)
    worst = np.zeros(4)
    cases = 0
    for spread in (1e-3, 0.05, 1.0):
        for reach in (0.5, 5.0, 50.0):
            for _ in range(40):
                S = _joint(rng, spread)
                xj = np.r_[rng.uniform(-100, 100, 2), rng.uniform(-np.pi, np.pi)]
                ang = rng.uniform(0, 2 * np.pi)
                xc = np.r_[xj[:2] + reach * rng.uniform(0.1, 1.0) * np.array([np.cos(ang), np.sin(ang)]), rng.uniform(-np.pi, np.pi)]
                worst = np.maximum(worst, _against_numpy(xj, xc, S[:3, :3], S[:3, 3:], S[3:, 3:], rng.choice([0.0, 0.3, 2.0])))
                cases += 1
    print(f"{cases} random pairs, |t| up to 50 m: worst ratios to the bars: P {worst[0]:.3g}, rel {worst[1]:.3g}, m2 {worst[2]:.3g}, sigma {worst[3]:.3g}")
    assert (worst <= 1.0).all(), worst


def test_fixed_endpoints_drop_out():
    rng = np.random.default_rng(5)
    S = _joint(rng, 0.1)
    xj, xc = np.array([1.0, -2.0, 0.7]), np.array([4.0, 1.5, -2.9])
    for Sjj, Sjc, Scc in ((None, None, S[3:, 3:]), (S[:3, :3], None, None), (None, S[:3, 3:], S[3:, 3:]), (S[:3, :3], S[:3, 3:], None)):
        assert max(_against_numpy(xj, xc, Sjj, Sjc, Scc, 2.0)) <= 1.0
    rel, P, m2, sg = capi.closure_search_rule(xj, xc, None, None, None, 2.0)         # both fixed: P = 0, a positive excess: +inf
    assert not P.any() and m2 == np.inf and not sg.any() and abs(np.hypot(rel[0], rel[1]) - np.hypot(3.0, 3.5)) <= 1e-14
    rel, P, m2, sg = capi.closure_search_rule(xj, xc, None, None, None, 5.0)         # ... and none: 0
    assert not P.any() and m2 == 0.0


def test_radius_zero_translation_and_angles():
    rng = np.random.default_rng(6)
    S = _joint(rng, 0.2)
    blocks = (S[:3, :3], S[:3, 3:], S[3:, 3:])
    xj = np.array([10.0, 20.0, 3.0])
    inside = np.array([10.6, 20.8, -3.0])                                              # |t| = 1 <= radius
    rel, P, m2, sg = capi.closure_search_rule(xj, inside, *blocks, 1.5)
    assert m2 == 0.0 and (sg > 0).all() and max(_against_numpy(xj, inside, *blocks, 1.5)) <= 1.0
    assert abs(rel[2] - (2 * np.pi - 6.0)) <= 1e-15                                    # theta_c - theta_j = -6 wraps to +0.283
    same_place = np.array([10.0, 20.0, -3.1])                                          # |t| = 0: no direction, m2 = 0 at any radius
    for radius in (0.0, 1.0):
        rel, P, m2, sg = capi.closure_search_rule(xj, same_place, *blocks, radius)
        assert m2 == 0.0 and rel[0] == 0.0 and rel[1] == 0.0 and np.isfinite(P).all() and np.isfinite(sg).all()
    for tj, tc in ((3.1, -3.1), (-3.1, 3.1), (np.pi - 1e-9, -np.pi + 1e-9), (0.5, 0.5 + np.pi), (-3.0, 9.0)):
        a, b = np.array([0.0, 0.0, tj]), np.array([3.0, 1.0, tc])
        rel = capi.closure_search_rule(a, b, *blocks, 1.0)[0]
        assert -np.pi <= rel[2] < np.pi and abs(np.angle(np.exp(1j * (rel[2] - (tc - tj))))) <= 1e-12, (tj, tc, rel[2])
        assert max(_against_numpy(a, b, *blocks, 1.0)) <= 1.0
    # a positive excess with P = 0 between two free poses whose blocks are zero: +inf
    Z = np.zeros((3, 3))
    assert capi.closure_search_rule(xj, xj + np.array([3.0, 0.0, 0.0]), Z, Z, Z, 1.0)[2] == np.inf


def test_refusals_that_need_no_device():
    L = capi.lib()
    m2 = np.full(4, SENTINEL)
    q = np.zeros(2, dtype=np.int32)
    assert L.sgo_closure_search(None, 2, capi._ip(q), 2, None, 2.0, 6.635, 0, capi._dp(m2), None, None, None, None) == -2
    assert L.sgo_closure_search(None, 0, None, 0, None, 2.0, 6.635, 0, None, None, None, None, None) == -2
    assert np.all(m2 == SENTINEL)
    x = np.zeros(3)
    S = np.eye(3).reshape(9)
    out = C.c_double(SENTINEL)
    assert L.sgo_closure_search_rule(None, capi._dp(x), None, None, None, 1.0, None, None, C.byref(out), None) == -2
    assert L.sgo_closure_search_rule(capi._dp(x), capi._dp(x), None, None, None, 1.0, None, None, None, None) == -2
    assert L.sgo_closure_search_rule(capi._dp(x), capi._dp(x), capi._dp(S), None, capi._dp(S), 1.0, None, None, C.byref(out), None) == -2
    assert out.value == SENTINEL
    assert L.sgo_closure_search_rule(capi._dp(x), capi._dp(x), None, None, None, 1.0, None, None, C.byref(out), None) == 0 and out.value == 0.0
