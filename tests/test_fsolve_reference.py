"""The multi-right-hand-side substitution's reference on the CPU (tests/fsolve_reference.py; no GPU): on every case of
tests/mfront_cases.py the fp64 model of sgo_fsolve.hip's front-by-front recurrence
  * is backward stable by the project's own rule: the Jacobi-scaled backward error of every column (sgo_rules.h) is at most
    rules::kFloorEta = 1e-12, on ALL cases;
  * gives the gate's P and d2 within selinv_reference.MODEL_BAR = 1e-8 of the long-double-refined reference -- except on the cases
    selinv_reference.ILL_CONDITIONED lists, where it must be ABOVE the bar (listed <=> above: no case beyond those three is left out
    of the device's accuracy comparison, tests/test_gpu_fsolve.py);
and the comparison rejects mutated recurrences.  Every test prints what it measured."""
import numpy as np
import pytest

import fsolve_reference as fr
import marginals_reference as mref
import mfront_cases as mc
import selinv_reference as sr
from sparse_gslam_amd import capi

_CACHE = {}


def _case(name):
    """(case, plan, H, candidates, R, e, refined X, size of its last correction): computed once per case and shared, never modified."""
    if name not in _CACHE:
        c = mc.make(name)
        with mc.environment(c.env):
            X = capi.mfront_plan_arrays(*c.arrays()[:4])
        H = mref.hessian(c.poses, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
        cand = fr.candidates(c)
        R, e = fr.rhs(c.poses, c.fixed, *cand[:3])
        Xr, last = fr.refined(H, R)
        for a in (R, e, Xr):
            a.setflags(write=False)
        _CACHE[name] = (c, sr.Plan(X, c.fixed), H, cand, R, e, Xr, last)
    return _CACHE[name]


def test_symbols_are_bound():
    import os
    import re
    L = capi.lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgo.h")).read()
    for name in ("sgo_factor_solve", "sgo_candidate_gate"):
        assert name in capi.SYMBOLS and hasattr(L, name) and re.search(r"\bint " + name + r"\(sgo_ctx\* ctx", src), name
    assert capi.MFRONT_ARRAYS["FS_Y"][0] == 16 and capi.MFRONT_ARRAYS["FS_X"][0] == 17
    assert "#define SGO_MF_FS_Y 16" in src and "#define SGO_MF_FS_X 17" in src
    assert L.sgo_version() == 107


def test_the_candidates_are_what_the_tests_say():
    c = mc.make("contributions")            # two fixed vertices
    ci, cj, meas, info = fr.candidates(c)
    assert ci.size == fr.K and (ci != cj).all()
    assert c.fixed[ci[0]] and cj[0] == np.flatnonzero(~c.fixed)[-1]
    assert c.fixed[ci[1]] and c.fixed[cj[1]]
    assert np.array_equal(fr.candidates(c)[2], meas)


@pytest.mark.parametrize("name", mc.NAMES)
def test_model_is_backward_stable_and_meets_the_gate_bar(name):
    c, plan, H, (ci, cj, meas, info), R, e, Xr, last = _case(name)
    Y, Xe = fr.model(plan, H, R)
    X = fr.to_hessian_order(plan, Xe)
    eta = fr.backward_error(H, X, R)
    used = np.abs(R).sum(0) > 0              # (a candidate between two fixed vertices has zero columns)
    assert not X[:, ~used].any()
    P, d2 = fr.gate(R, X, e, info)
    Pr, d2r = fr.gate(R, Xr, e, info)
    rp, rd = fr.gate_ratios(P, d2, Pr, d2r, info)
    print(f"{name}: model backward error {eta[used].max():.2e}; P {rp:.3e}, d2 {rd:.3e} of the refined reference; last correction {last:.1e}")
    assert eta[used].max() <= fr.FLOOR_ETA, (name, eta.max())
    assert np.array_equal(P, P.transpose(0, 2, 1))
    fixed_both = c.fixed[ci] & c.fixed[cj]
    assert not P[fixed_both].any()
    if name in sr.ILL_CONDITIONED:
        assert max(rp, rd) > sr.MODEL_BAR, (name, rp, rd, "the case meets the bar: it is an accuracy case")
        assert np.isfinite(P).all() and np.isfinite(d2).all()
    else:
        assert last <= 1e-12, last
        assert rp <= sr.MODEL_BAR and rd <= sr.MODEL_BAR, (name, rp, rd)


@pytest.mark.parametrize("name", ["tree_shapes", "child_own3_33"])
@pytest.mark.parametrize("mut", [None, "child_update_dropped", "backward_boundary_dropped", "not_symmetrised"])
def test_the_comparison_rejects_a_wrong_recurrence(name, mut):
    c, plan, H, (ci, cj, meas, info), R, e, Xr, _ = _case(name)
    _, Xe = fr.model(plan, H, R, mut=mut)
    X = fr.to_hessian_order(plan, Xe)
    P, d2 = fr.gate(R, X, e, info, mut=mut)
    Pr, d2r = fr.gate(R, Xr, e, info)
    rp, rd = fr.gate_ratios(P, d2, Pr, d2r, info)
    eta = fr.backward_error(H, X, R).max()
    ok = eta <= fr.FLOOR_ETA and rp <= sr.MODEL_BAR and rd <= sr.MODEL_BAR and np.array_equal(P, P.transpose(0, 2, 1))
    print(f"{name} / {mut}: backward error {eta:.2e}, P {rp:.3e}, d2 {rd:.3e}, symmetric {np.array_equal(P, P.transpose(0, 2, 1))}")
    assert ok == (mut is None), (name, mut, eta, rp, rd)


def test_the_forward_pass_carries_what_the_factorisation_carries():
    """Y of the linearisation's own b is L^-1 b: the model's forward pass against a triangular solve of the whole factor"""
    c, plan, H, _, _, _, _, _ = _case("tree_shapes")
    b = np.random.default_rng(3).standard_normal((H.shape[0], 2))
    Y, Xe = fr.model(plan, H, b)
    L = np.linalg.cholesky(np.asarray(H.todense())[np.ix_(plan.perm, plan.perm)])
    want = np.linalg.solve(L, b[plan.perm])
    assert np.abs(Y - want).max() <= 1e-12 * np.abs(want).max()


def test_an_indefinite_hessian_is_refused_by_the_model():
    c, plan, H, _, R, _, _, _ = _case("child_own3_12")
    Hn = H.toarray().copy()
    Hn[4, 4] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        fr.model(plan, Hn, R)
