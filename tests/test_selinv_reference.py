"""The selected-inversion reference on the CPU (tests/selinv_reference.py; no GPU): on every case of tests/mfront_cases.py the
fp64 model of sgo_selinv.hip's panel recurrence equals, entry by entry for every stored entry of every front, the dense inverse
of the oracle's Hessian refined in long double.  This also fixes which cases are accuracy cases for the device
(tests/test_gpu_selinv.py): a case whose fp64 model is further than 1e-8 of the natural scale from the inverse is listed in
selinv_reference.ILL_CONDITIONED by name with its ratio -- only closure_weight_1e10, rows_scaled_1e6 and long_thin_chain may be."""
import numpy as np
import pytest

import marginals_reference as mref
import mfront_cases as mc
import selinv_reference as sr
from sparse_gslam_amd import capi

MAY_BE_ILL = {"closure_weight_1e10", "rows_scaled_1e6", "long_thin_chain"}
_CACHE = {}


def _case(name):
    """(case, plan, H, dense inverse, size of its last correction): computed once per case and shared, never modified."""
    if name not in _CACHE:
        c = mc.make(name)
        with mc.environment(c.env):
            X = capi.mfront_plan_arrays(*c.arrays()[:4])
        H = mref.hessian(c.poses, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
        Sigma, last = sr.dense_inverse(H)
        Sigma.setflags(write=False)
        _CACHE[name] = (c, sr.Plan(X, c.fixed), H, Sigma, last)
    return _CACHE[name]


def test_only_the_three_scaling_cases_may_be_listed():
    assert set(sr.ILL_CONDITIONED) <= MAY_BE_ILL


def test_symbol_is_bound():
    assert "sgo_marginals_selected" in capi.SYMBOLS and hasattr(capi.lib(), "sgo_marginals_selected")
    assert capi.MFRONT_ARRAYS["SEL"][0] == 15


@pytest.mark.parametrize("name", mc.NAMES)
def test_model_equals_the_long_double_inverse_on_every_stored_entry(name):
    c, plan, H, Sigma, last = _case(name)
    S = sr.model(plan, H)
    ratio, where = sr.worst_ratio(plan, S, Sigma)
    print(f"{name}: fp64 model / long-double inverse: worst {ratio:.3e} of the natural scale at {where}; last correction {last:.1e}")
    if name in sr.ILL_CONDITIONED:
        assert ratio > sr.MODEL_BAR, (name, ratio, "the case meets the bar: take it off the list")
        assert np.isfinite(ratio) and 0.1 <= ratio / sr.ILL_CONDITIONED[name] <= 10.0, (ratio, "the recorded ratio is stale")
    else:
        # the reference itself: a correction of this relative size times cond(H) U is far below the bar
        assert last <= 1e-12, last
        assert ratio <= sr.MODEL_BAR, (name, ratio, where)
    # the model's diagonal blocks are covariances
    for F, Sf in zip(plan.fronts, S):
        for p in range(F.own):
            B = Sf[3 * p:3 * p + 3, 3 * p:3 * p + 3]
            B = np.tril(B) + np.tril(B, -1).T
            assert np.linalg.eigvalsh(B).min() > 0.0


@pytest.mark.parametrize("mut", ["upper_triangle_read_as_stored", "diagonal_term_dropped"])
def test_the_comparison_rejects_a_wrong_recurrence(mut):
    c, plan, H, Sigma, _ = _case("tree_shapes")
    ratio, _ = sr.worst_ratio(plan, sr.model(plan, H, mut=mut), Sigma)
    assert ratio > 1e-3, (mut, ratio)


def test_an_indefinite_hessian_is_refused_by_the_model():
    c, plan, H, _, _ = _case("child_own3_12")
    Hn = H.toarray().copy()
    Hn[4, 4] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        sr.model(plan, Hn)
