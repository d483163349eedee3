"""The selected-inversion reference on the CPU (tests/selinv_reference.py; no GPU): on every case of tests/mfront_cases.py the
fp64 model of sgo_selinv.hip's panel recurrence equals, entry by entry for every stored entry of every front, the dense inverse
of the oracle's Hessian refined in long double.  This also fixes which cases are accuracy cases for the device
(tests/test_gpu_selinv.py): a case whose fp64 model is further than 1e-8 of the natural scale from the inverse is listed in
selinv_reference.ILL_CONDITIONED by name with its ratio -- only closure_weight_1e10, rows_scaled_1e6 and long_thin_chain may be."""
import numpy as np
import pytest

import marginals_reference as mref
import mfront_cases as mc
import mfront_reference as mr
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


# ------------------------------------------------------------------ the stage checks (selinv_reference.check) on the model
_STAGE = {}


def _moved(c, scale=1e-6, seed=21):
    """the case's poses moved by scale x N(0, 1) on the free vertices: the second call of the device test"""
    P = c.poses + scale * np.random.default_rng(seed).standard_normal(c.poses.shape) * (~c.fixed)[:, None]
    return P


def _stage(name, moved=False):
    """(case, plan, H, host factor): computed once per case and shared, never modified"""
    key = (name, moved)
    if key not in _STAGE:
        c = mc.make(name)
        with mc.environment(c.env):
            X = capi.mfront_plan_arrays(*c.arrays()[:4])
        P = _moved(c) if moved else c.poses
        H = mref.hessian(P, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
        plan = sr.Plan(X, c.fixed)
        fac = sr.host_factor(plan, H)
        for a in fac:
            a.setflags(write=False)
        _STAGE[key] = (c, plan, H, fac)
    return _STAGE[key]


def _synthetic(name, **mut):
    """the model's output packed as the device exports it: (case dict, X, D, cov, vi, vj, S)"""
    c, plan, H, fac = _stage(name)
    S = sr.model(plan, H, factor=fac, **mut)
    X = dict(plan.X, ARENA=fac[0], YINV=fac[1], SEL=sr.pack(plan.X, S))
    vi, vj = np.r_[c.ei, c.ej], np.r_[c.ej, c.ei]
    D, cov = sr.results(plan, S, vi, vj, c.poses.shape[0])
    return c.as_dict(), X, D, cov, vi, vj, S


_CHECKED = {}


def _checked(name):
    if name not in _CHECKED:
        cd, X, D, cov, vi, vj, _ = _synthetic(name)
        _CHECKED[name] = sr.check(cd, X, D, cov, vi, vj)
    return _CHECKED[name]


def test_constants_are_four_times_the_model_rounded_up_to_a_power_of_two():
    assert set(sr.C_STAGE) == set(sr.MODEL) == set(sr.MEASURED) == {"offdiag", "diag"} and set(sr.C_STAGE) < set(sr.STAGES)
    for k, v in sr.MODEL.items():
        assert sr.C_STAGE[k] == mr.constant(v) and 4.0 * v <= sr.C_STAGE[k] < 8.0 * v
        assert 0.0 < sr.MEASURED[k][0] <= sr.C_STAGE[k] and sr.MEASURED[k][1] in mc.NAMES      # (the device's figure: never a reason to raise C)


def test_the_packer_is_the_inverse_of_front_from_arena():
    c, plan, H, fac = _stage("tree_shapes")
    rng = np.random.default_rng(2)
    S = [np.tril(rng.standard_normal((F.m, F.m))) for F in plan.fronts]
    sel = sr.pack(plan.X, S)
    for F, Sf in zip(plan.fronts, S):
        assert np.array_equal(sr.front_from_arena(sel, F), Sf)
    assert np.count_nonzero(sel) == sum(np.count_nonzero(Sf) for Sf in S)
    # ... and the packed factor is the one numpy made: L L^T = H front by front, Y L_dd = I
    L = np.zeros((plan.perm.size, plan.perm.size))
    for F in plan.fronts:
        r = plan.rows(F)
        L[np.ix_(r, r[:F.own3])] = mr.front_matrix(fac[0], F)[:F.m, :F.own3]
    Hp = H.toarray()[np.ix_(plan.perm, plan.perm)]
    assert np.abs(L @ L.T - Hp).max() <= 1e-12 * np.abs(Hp).max()


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_model_passes_every_stage(name):
    """on every case, the three ill-conditioned ones included: no bound carries a condition number"""
    R = _checked(name)
    print(sr.report(name, R))
    assert not sr.failures(R), sr.report(name, R)
    for stage, v in sr.worst_by_stage(R).items():
        assert v <= sr.MODEL[stage], (stage, v)


def test_the_recorded_model_figures_are_reached():
    worst = {}
    for name in mc.NAMES:
        for stage, v in sr.worst_by_stage(_checked(name)).items():
            worst[stage] = max(worst.get(stage, 0.0), v)
    print({k: float(f"{v:.5g}") for k, v in worst.items()})
    for stage, v in sr.MODEL.items():
        assert 0.99 * v <= worst[stage] <= v, (stage, worst[stage], v)


def _front(plan, pred):
    at = [f for f, F in enumerate(plan.fronts) if pred(f, F)]
    assert at
    return at[0]


STAGE_MUTATIONS = [
    # mutation, case, the front it is applied at (None: every front), the stages that own it
    ("upper_triangle_read_as_stored", "tree_shapes", None, ("offdiag",)),
    ("diagonal_term_dropped", "tree_shapes", None, ("diag",)),
    ("last_k_dropped", "tree_shapes", lambda f, F: F.own3 > 0 and F.m > F.own3, ("offdiag", "diag")),
    ("wave_share_dropped", "child_own3_48", lambda f, F: F.own3 > 0 and F.m - F.own3 > 0, ("diag",)),
    ("narrow_panel_rows_as_stored", "child_own3_12", lambda f, F: f == 0 and F.own3 % 16 != 0, ("diag",)),
    ("gather_neighbour_pose", "tree_shapes", lambda f, F: F.parent >= 0 and F.m > F.own3, ("gather",)),
    ("stale_offdiag", "tree_shapes", lambda f, F: F.own3 > 0 and F.m > F.own3, ("offdiag",)),
]


def _stale(name):
    c, plan, H, fac = _stage(name)
    _, _, Hm, facm = _stage(name, moved=True)
    return sr.model(plan, Hm, factor=facm)


@pytest.mark.parametrize("mut,name,where,owners", STAGE_MUTATIONS, ids=[m[0] for m in STAGE_MUTATIONS])
def test_mutation_is_rejected_by_the_stage_that_owns_it(mut, name, where, owners):
    c, plan, H, fac = _stage(name)
    front = None if where is None else _front(plan, where)
    kw = dict(stale=_stale(name)) if mut == "stale_offdiag" else {}
    cd, X, D, cov, vi, vj, _ = _synthetic(name, mut=mut, mut_front=front, **kw)
    R = sr.check(cd, X, D, cov, vi, vj)
    s = sr.scaled(R)
    print(sr.report(f"{name} / {mut} at front {front}", R))
    assert max(v for k, v in s.items() if mr.stage_of(k) in owners) >= 10.0, sr.report(name, R)
    order = ("structure",) + sr.STAGES
    first = min(order.index(o) for o in owners)
    assert all(v <= 1.0 for k, v in s.items() if mr.stage_of(k) in order[:first]), sr.report(name, R)


def test_a_stale_entry_passes_the_old_comparison():
    """the gap the stage checks close: one front's Sigma_RJ kept from a run at poses moved by 1e-6 is within DEVICE_BAR = 1e-6 of
    the natural scale of the dense inverse, which was all the device was held to"""
    name = "tree_shapes"
    c, plan, H, Sigma, _ = _case(name)
    front = _front(plan, STAGE_MUTATIONS[-1][2])
    S = sr.model(plan, H, factor=_stage(name)[3], mut="stale_offdiag", mut_front=front, stale=_stale(name))
    ratio, where = sr.worst_ratio(plan, S, Sigma)
    fresh, _ = sr.worst_ratio(plan, sr.model(plan, H, factor=_stage(name)[3]), Sigma)
    print(f"stale Sigma_RJ at front {front}: {ratio:.3e} of the natural scale at {where} (fresh: {fresh:.3e}); the old bar {sr.DEVICE_BAR:.0e}")
    assert fresh < ratio <= sr.DEVICE_BAR


def test_every_shape_class_is_reached():
    """selinv_reference.COVERS names one case per class of k_si_panels' panels, k_si_gather's blocks and the tree; from the host plan"""
    assert set(sr.COVERS.values()) <= set(mc.NAMES)
    for cls, name in sr.COVERS.items():
        cov = sr.coverage(_stage(name)[1].X)
        assert set(cov) == set(sr.COVERS)
        assert cov[cls], (cls, name)
    # unconnected components hang under ONE root without own columns: a plan has no second root
    X = _stage("front_without_pivots")[1].X
    F = np.asarray(X["FRONTS"])
    assert (F[:, 13] < 0).sum() == 1 and F[F[:, 13] < 0][0, 1] == 0 and (F[F[:, 13] < 0][0, 7:9] >= 0).all()
