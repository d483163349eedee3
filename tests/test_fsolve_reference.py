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


# ------------------------------------------------------------------ the stage checks (fsolve_reference.check / check_gate) on the model
NRHS = 35                                    # two full panels and a tail of 3 (tests/test_gpu_fsolve.py's)
_STAGE = {}


def rhs35(c, H, R):
    """the device test's 35 right-hand sides (tests/test_gpu_fsolve.py): 24 candidate columns, 9 random ones, a unit vector and the
    linearisation's own b"""
    from oracle import np_oracle as npo
    w = mref.weights(c.poses, c.ei, c.ej, c.meas, c.info, c.phi)
    b = npo.linearize(c.poses, c.fixed, c.ei, c.ej, c.meas, c.info * w[:, None], np.full(c.ei.size, -1.0))[1]
    N = H.shape[0]
    unit = np.zeros((N, 1))
    unit[N // 2] = 1.0
    return np.concatenate([R[:, :24], np.random.default_rng(123).standard_normal((N, 9)), unit, b[:, None]], axis=1)


_INPUTS = {}


def inputs(name):
    """(case, H, candidates, R, e, B): what the calls are handed, shared with tests/test_gpu_fsolve_reference.py; never modified"""
    if name not in _INPUTS:
        c = mc.make(name)
        H = mref.hessian(c.poses, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
        cand = fr.candidates(c)
        R, e = fr.rhs(c.poses, c.fixed, *cand[:3])
        B = rhs35(c, H, R)
        for a in (R, e, B):
            a.setflags(write=False)
        _INPUTS[name] = (c, H, cand, R, e, B)
    return _INPUTS[name]


def _stage(name):
    """(case, plan, H, host factor, candidates, R, e, B): computed once per case and shared, never modified"""
    if name not in _STAGE:
        c, H, cand, R, e, B = inputs(name)
        with mc.environment(c.env):
            X = capi.mfront_plan_arrays(*c.arrays()[:4])
        plan = sr.Plan(X, c.fixed)
        fac = sr.host_factor(plan, H)
        for a in fac:
            a.setflags(write=False)
        _STAGE[name] = (c, plan, H, fac, cand, R, e, B)
    return _STAGE[name]


def _synthetic(name, mut=None, mut_front=None):
    """the model's output packed as the device exports it, checked: the stages' raw ratios"""
    c, plan, H, fac, cand, R, e, B = _stage(name)
    gate_mut = mut if mut == "not_symmetrised" else None
    Y, Xe = fr.model(plan, H, B, factor=fac, mut=None if gate_mut else mut, mut_front=mut_front)
    X = dict(plan.X, ARENA=fac[0], YINV=fac[1], FS_Y=np.ascontiguousarray(Y.T).ravel(), FS_X=np.ascontiguousarray(Xe.T).ravel())
    Xh = fr.to_hessian_order(plan, Xe)
    Res = fr.check(c.as_dict(), X, B, np.ascontiguousarray(Xh.T), Xh[:, 20].copy())
    _, Xc = fr.model(plan, H, R, factor=fac, mut=None if gate_mut else mut, mut_front=mut_front)
    P, d2 = fr.gate(R, fr.to_hessian_order(plan, Xc), e, cand[3], mut=gate_mut)
    X["FS_X"] = np.ascontiguousarray(Xc.T).ravel()
    Res.update(fr.check_gate(c.as_dict(), X, cand, d2, P))
    return Res


_CHECKED = {}


def _checked(name):
    if name not in _CHECKED:
        _CHECKED[name] = _synthetic(name)
    return _CHECKED[name]


def test_constants_are_four_times_the_model_rounded_up_to_a_power_of_two():
    import mfront_reference as mr
    assert set(fr.C_STAGE) == set(fr.MODEL) == set(fr.MEASURED) == set(fr.STAGES) - {"columns"}
    for k, v in fr.MODEL.items():
        assert fr.C_STAGE[k] == mr.constant(v) and 4.0 * v <= fr.C_STAGE[k] < 8.0 * v
        assert 0.0 < fr.MEASURED[k][0] <= fr.C_STAGE[k] and fr.MEASURED[k][1] in mc.NAMES      # (the device's figure: never a reason to raise C)


def test_the_chunk_size_is_the_drivers():
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sparse_gslam_amd", "csrc")
    dev = open(os.path.join(src, "sgo_mfront_dev.h")).read()
    panels = int(re.search(r"constexpr int kFsChunkPanels = (\d+);", dev).group(1))
    panel = int(re.search(r"constexpr int kMfPanel = (\d+);", open(os.path.join(src, "sgo_mfront.h")).read() + dev).group(1))
    assert "kChunkCands = kFsChunkPanels * kMfPanel / 3" in open(os.path.join(src, "sgo_fsolve.cpp")).read()
    assert fr.CHUNK_CANDS == panels * panel // 3 and fr.PANEL == panel


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_model_passes_every_stage(name):
    """on every case, the three ill-conditioned ones included: no bound carries the condition of H"""
    R = _checked(name)
    print(fr.report(name, R))
    assert not fr.failures(R), fr.report(name, R)
    for stage, v in fr.worst_by_stage(R).items():
        assert v <= fr.MODEL[stage], (stage, v)


def test_the_recorded_model_figures_are_reached():
    worst = {}
    for name in mc.NAMES:
        for stage, v in fr.worst_by_stage(_checked(name)).items():
            worst[stage] = max(worst.get(stage, 0.0), v)
    print({k: float(f"{v:.5g}") for k, v in worst.items()})
    for stage, v in fr.MODEL.items():
        assert 0.99 * v <= worst[stage] <= v, (stage, worst[stage], v)


STAGE_MUTATIONS = [
    # mutation, case, the front it is applied at (None: every front), the stages that own it
    ("child_update_dropped", "tree_shapes", None, ("forward",)),
    ("backward_boundary_dropped", "tree_shapes", None, ("backward",)),
    ("column_contaminated_by_its_neighbour", "child_own3_33", 0, ("backward",)),
    ("backward_inverse_not_transposed", "child_own3_33", 0, ("backward",)),
    ("not_symmetrised", "tree_shapes", None, ("gate",)),
]


@pytest.mark.parametrize("mut,name,front,owners", STAGE_MUTATIONS, ids=[m[0] for m in STAGE_MUTATIONS])
def test_mutation_is_rejected_by_the_stage_that_owns_it(mut, name, front, owners):
    import mfront_reference as mr
    R = _synthetic(name, mut=mut, mut_front=front)
    s = fr.scaled(R)
    print(fr.report(f"{name} / {mut} at front {front}", R))
    assert max(v for k, v in s.items() if mr.stage_of(k) in owners) >= 10.0, fr.report(name, R)
    first = min(fr.STAGES.index(o) for o in owners)
    assert all(v <= 1.0 for k, v in s.items() if mr.stage_of(k) in fr.STAGES[:first]), fr.report(name, R)
