"""sgo_lm_trial_rule (rules::lm_trial, sparse_gslam_amd/csrc/sgo_rules.h: the one statement k_lm_decide and the host compile) against
the numpy statement of a trial in oracle/np_lm_oracle.py::levenberg, on fabricated sequences and without a GPU."""
import math

import pytest

from sparse_gslam_amd import capi

DBL_MAX = 1.7976931348623157e308


def np_trial(cur, tmp, scale, ok, lam, nu):
    """one pass of the oracle's `while True` body from rho on -> (accepted, rho, lambda, nu)"""
    if not ok:
        tmp, scale = DBL_MAX, 1e-3       # (the oracle: tmp = inf over scale = 1e-3; g2o and the rule: DBL_MAX -- rho is -inf either way)
    rho = (cur - tmp) / scale if scale != 0 else math.nan
    if rho > 0 and math.isfinite(tmp) and ok:
        return True, rho, lam * max(1.0 / 3.0, min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)), 2.0
    return False, rho, lam * nu, nu * 2


def code_of(accepted, rho):
    if accepted:
        return capi.LM_ACCEPT
    return capi.LM_RETRY if rho < 0 else (capi.LM_ZERO_GAIN if rho == 0 else capi.LM_END)


def check(cur, tmp, scale, ok, lam, nu):
    code, l1, n1 = capi.lm_trial_rule(cur, tmp, scale, ok, lam, nu)
    acc, rho, l0, n0 = np_trial(cur, tmp, scale, ok, lam, nu)
    assert code == code_of(acc, rho), (cur, tmp, scale, ok, code, rho)
    assert n1 == n0
    assert (l1 == l0) or (math.isnan(l1) and math.isnan(l0)) or abs(l1 - l0) <= 4e-16 * abs(l0), (l1, l0)   # (t * t * t against ** 3)
    return code, l1, n1


def test_accept_just_above_zero_and_the_clamps():
    code, lam, nu = check(10.0, 10.0 - 1e-12, 5.0, True, 3.0, 16.0)         # rho = 2e-13 > 0
    assert code == capi.LM_ACCEPT and lam == 3.0 * (2.0 / 3.0) and nu == 2.0
    for rho in (1e-9, 0.2, 0.5, 0.8, 0.85, 0.9, 0.93, 0.95, 1.0, 1.7, 40.0):
        code, lam, _ = check(100.0, 100.0 - rho * 7.0, 7.0, True, 1.0, 2.0)
        assert code == capi.LM_ACCEPT and 1.0 / 3.0 <= lam <= 2.0 / 3.0
    assert check(100.0, 100.0 - 0.9 * 7.0, 7.0, True, 1.0, 2.0)[1] == pytest.approx(1.0 - 0.8 ** 3, rel=1e-12)   # inside the band
    assert check(1.0, 0.0, 1e300, True, 1.0, 2.0)[0] == capi.LM_ACCEPT      # rho = 1e-300


def test_zero_gain_rejects_and_ends():
    code, lam, nu = check(10.0, 10.0, 5.0, True, 3.0, 4.0)
    assert code == capi.LM_ZERO_GAIN and lam == 12.0 and nu == 8.0
    assert check(0.0, 0.0, 1e-3, True, 1.0, 2.0)[0] == capi.LM_ZERO_GAIN


def test_non_finite_trials():
    assert check(10.0, math.inf, 5.0, True, 1.0, 2.0)[0] == capi.LM_RETRY       # rho = -inf
    assert check(10.0, math.nan, 5.0, True, 1.0, 2.0)[0] == capi.LM_END         # rho NaN: rejected, no further trial
    assert check(10.0, -math.inf, 5.0, True, 1.0, 2.0)[0] == capi.LM_END        # rho = +inf but the trial is not finite
    assert check(10.0, 9.0, math.nan, True, 1.0, 2.0)[0] == capi.LM_END
    assert check(10.0, 9.0, -5.0, True, 1.0, 2.0)[0] == capi.LM_RETRY           # a negative scale turns a decrease into rho < 0
    assert check(math.nan, 9.0, 5.0, True, 1.0, 2.0)[0] == capi.LM_END


def test_failed_solve_is_a_rejection_whatever_the_numbers():
    for tmp, scale in ((1.0, 5.0), (math.nan, math.nan), (0.0, 0.0), (-math.inf, 1.0)):
        code, lam, nu = check(10.0, tmp, scale, False, 3.0, 2.0)
        assert code == capi.LM_RETRY and lam == 6.0 and nu == 4.0


def test_nu_doubles_over_nine_rejections_then_the_tenth():
    lam, nu = 1e-3, 2.0
    for q in range(10):
        code, lam, nu = check(10.0, 11.0, 2.0, True, lam, nu)
        assert code == capi.LM_RETRY and nu == 2.0 ** (q + 2)
    assert lam == 1e-3 * 2.0 ** 55                                               # 2 * 4 * ... * 1024
    code, lam, nu = check(10.0, 9.5, 2.0, True, lam, nu)                         # an accepted trial puts nu back
    assert code == capi.LM_ACCEPT and nu == 2.0


def test_lambda_overflow():
    code, lam, nu = check(10.0, 11.0, 2.0, True, 1e300, 1e10)
    assert code == capi.LM_RETRY and math.isinf(lam) and nu == 2e10
    code, lam, _ = check(10.0, 9.0, 2.0, True, math.inf, 2.0)                    # lambda stays what it is
    assert code == capi.LM_ACCEPT and math.isinf(lam)
