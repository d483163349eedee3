"""The direct path's stage reference on the CPU (tests/direct_reference.py, tests/direct_cases.py; no GPU): every case has the shape
it declares, its host plan passes the exact structure checks, the plain fp64 model passes every stage within the constants taken
from it, its solution is the sparse direct solve's, the analysis refuses 61 separators, and the stage checks reject the
mutations of the model at >= 10 C in the stage that owns them while every stage before it stays within C."""
import os
import re

import numpy as np
import pytest

import direct_cases as dc
import direct_reference as dr
from oracle import np_oracle as npo
from sparse_gslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _case(name):
    """(case, host plan, the model's arrays, its ratios): computed once per case and shared, never modified."""
    if name not in _CACHE:
        c = dc.make(name)
        plan = capi.direct_plan_arrays(c.fixed, c.ei, c.ej)
        X = dr.model(c.as_dict(), plan)
        _CACHE[name] = (c, plan, X, dr.check(c.as_dict(), X))
    return _CACHE[name]


def test_constants_are_four_times_the_model_rounded_up_to_a_power_of_two():
    assert set(dr.C_STAGE) == set(dr.STAGES) == set(dr.MODEL) == set(dr.MODEL_CASE)
    for k, v in dr.MODEL.items():
        c = dr.C_STAGE[k]
        assert c == 2.0 ** round(np.log2(c)) and 4.0 * v <= c < 8.0 * v, (k, v, c)


def test_numbering_equals_the_header():
    src = open(os.path.join(ROOT, "include", "sgo.h")).read()
    hdr = {k: int(v) for k, v in re.findall(r"#define\s+SGO_DR_([A-Z_0-9]+)\s+(\d+)", src)}
    assert hdr == {k: v[0] for k, v in capi.DIRECT_ARRAYS.items()}
    assert capi.DIRECT_PLAN_ARRAYS == tuple(capi.DIRECT_ARRAYS)[:13] and len(capi.DIRECT_INFO) == 13


def test_every_case_of_the_issue_is_there():
    want = ("two_poses chain_3 chain_65 chain_130 one_closure two_seps multi_pairs hub seps_48 seps_49 seps_60 wide_column "
            "tasks_over_512 xg_below xg_above kinds_mixed kinds_xg long_chain_2048 weight_1e10 rows_scaled_1e6 angles_pi "
            "dcs_switches_closures_off").split()
    assert set(want) <= set(dc.NAMES) and set(dc.REFUSED) == {"seps_61"} and set(dc.SECOND_ITERATION) <= set(dc.NAMES)


@pytest.mark.parametrize("name", dc.NAMES)
def test_case_has_its_shape_and_the_model_passes_every_stage(name):
    """The declared shape and the exact structure checks from the host plan alone; every ratio of the model within C, and within
    the recorded worst of the model (the figure the constants were taken from)."""
    c, plan, X, R = _case(name)
    shape = dc.check_shape(c, plan)
    assert shape and all(shape.values()), (name, shape)
    S = dr.structure(c.as_dict(), plan)
    assert len(S) >= 15 and S.worst() == 0.0, dr.report(name, S)
    assert not dr.failures(R), dr.report(name, R)
    assert set(dr.worst_by_stage(R)) >= set(dr.STAGES) - ({"dense"} if c.shape and int(plan["INFO"][2]) == 0 else set())
    for stage, v in dr.worst_by_stage(R).items():
        assert v <= dr.MODEL[stage], (stage, v, dr.report(name, R))


def test_the_recorded_model_figures_are_reached():
    """MODEL is the worst over the cases, not a guess above it: every stage's figure is met within 1 % by the case MODEL_CASE
    names."""
    for stage, v in dr.MODEL.items():
        got = dr.worst_by_stage(_case(dr.MODEL_CASE[stage])[3])[stage]
        assert 0.99 * v <= got <= v, (stage, got, v)


def test_sixty_one_separators_are_refused_with_the_reason_the_description_gives():
    c = dc.make("seps_61")
    with pytest.raises(capi.SgoError, match=c.refused):
        capi.direct_plan_arrays(c.fixed, c.ei, c.ej)
    c60 = dc.make("seps_60")
    assert int(capi.direct_plan_arrays(c60.fixed, c60.ei, c60.ej, names=("INFO",))["INFO"][2]) == 60
    with pytest.raises(capi.SgoError, match="more free poses than direct_rows"):
        capi.direct_plan_arrays(c60.fixed, c60.ei, c60.ej, max_rows=100)


@pytest.mark.parametrize("name", ["multi_pairs", "hub", "wide_column", "weight_1e10", "rows_scaled_1e6", "chain_130"])
def test_model_solution_is_the_sparse_direct_solve(name):
    """x of the model in hessian order against scipy's sparse LU of np_oracle's H, b.  A forward error: two backward-stable
    solves differ by a small multiple of kappa_2(H) U in the relative 2-norm; 8 kappa U holds both solves' share."""
    from scipy.sparse.linalg import spsolve
    c, plan, X, R = _case(name)
    H, b, _, _ = npo.linearize(*c.arrays())
    ref = spsolve(H.tocsc(), b).reshape(-1, 3)
    hidx, free = npo.hessian_index(c.fixed)
    got = np.zeros_like(ref)
    got[hidx[plan["POS_VERTEX"].astype(np.int64)]] = X["X"].reshape(-1, 3)
    kappa = np.linalg.cond(H.toarray())
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"{name}: kappa {kappa:.3g}, relative difference {rel:.3g} = {rel / (kappa * dr.U):.3g} kappa U")
    assert kappa * dr.U < 0.1 and rel <= 8.0 * kappa * dr.U, (rel, kappa)


MUTATIONS = [
    # mutation of model(), case, the checks that own it
    ("contribution_dropped", "seps_49", ("forward",)),
    ("contribution_doubled", "seps_49", ("forward",)),
    ("flag_flipped_stored", "three_seps", ("assembly.A_WO",)),
    ("flag_flipped_separator", "three_seps", ("assembly.A_SD_off_diagonal",)),
    ("overflow_entry_skipped", "hub", ("assembly.A_WD", "assembly.A_XB", "assembly.A_SD_diagonal")),
    ("multi_edge_skipped", "multi_pairs", ("assembly.A_WO", "assembly.A_SD_off_diagonal")),
    ("zero_slot_not_cleared", "chain_65", ("assembly.zero_slots_are_zero",)),
    ("pivot_factors_wrong_order", "two_seps", ("substitution.separators",)),
    ("permutation_off_by_one", "hub", ("update",)),
]


def _owned_and_early(Rm, owners):
    s = dr.scaled(Rm)
    owned = {k: v for k, v in s.items() if any(k == o or dr.stage_of(k) == o for o in owners)}
    order = ("structure",) + dr.STAGES
    first = min(order.index(dr.stage_of(o)) for o in owners)
    early = {k: v for k, v in s.items() if dr.stage_of(k) in order[:first]}
    return owned, early


@pytest.mark.parametrize("mut,name,owners", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_rejected_by_the_stage_that_owns_it(mut, name, owners):
    c, plan, X, R = _case(name)
    Rm = dr.check(c.as_dict(), dr.model(c.as_dict(), plan, mut=mut))
    owned, early = _owned_and_early(Rm, owners)
    assert owned and max(owned.values()) >= 10.0, (mut, dr.report(name, Rm))
    # ... and by no stage before the first owner (an error is charged to the stage that made it)
    assert all(v <= 1.0 for v in early.values()), (mut, dr.report(name, Rm))


@pytest.mark.parametrize("name", ["hub", "seps_49"])
def test_a_stale_separator_entry_in_the_second_iteration_is_rejected_by_the_assembly(name):
    """The clear of the separator triangle after the back substitution matters from the second iteration on: the assembly stores
    where edges reach and the forward tasks add elsewhere, so what the first iteration left in a block no edge reaches would be
    added to H.  The second iteration's model, started from the first one's P1 with the first one's D_SD left in place, fails the
    exact check of the unreached entries; with the triangle cleared it passes every stage."""
    c, plan, X, R = _case(name)
    ns = int(plan["INFO"][2])
    second = dict(c.as_dict(), P0=X["P1"])
    good = dr.check(second, dr.model(second, plan))
    assert not dr.failures(good), dr.report(name, good)
    Rm = dr.check(second, dr.model(second, plan, stale=dr.unpack_tri(X["D_SD"], ns)))
    owned, early = _owned_and_early(Rm, ("assembly.unreached_entries_of_A_SD_are_zero",))
    assert max(owned.values()) == float("inf"), dr.report(name, Rm)
    assert all(v <= 1.0 for v in early.values()), dr.report(name, Rm)


def test_explicit_inverse_in_place_of_the_factor_solve_is_what_the_forward_stage_rejects():
    """k_direct applies its pivot blocks through their 3 x 3 LDL^T factors because the pivots of the upper levels are Schur
    complements of long chain segments.  The same model with numpy's explicit inverse in their place, recorded (worst error /
    (U abs) of the forward stage, the factor solve's own figure in brackets): long_chain_2048 7.4e4 (4.2), rows_scaled_1e6 6.2e6
    (2.8) with the composed residual at 1.4e3 (0.43), xg_above 1.1e3 (2.5), weight_1e10 10 (2.4): what the componentwise bound of
    a solve through the factor rejects by orders of magnitude, and nothing before the forward stage notices."""
    out = {}
    for name in ("long_chain_2048", "rows_scaled_1e6", "weight_1e10"):
        c, plan, X, R = _case(name)
        Rm = dr.check(c.as_dict(), dr.model(c.as_dict(), plan, mut="explicit_inverse"))
        out[name] = dr.worst_by_stage(Rm)
        owned, early = _owned_and_early(Rm, ("forward",))
        assert all(v <= 1.0 for v in early.values()), dr.report(name, Rm)
    print("explicit inverse, worst ratio by stage:", {k: {s: float(f"{v:.3g}") for s, v in w.items()} for k, w in out.items()})
    assert out["long_chain_2048"]["forward"] >= 100.0 * dr.C_STAGE["forward"], out
    assert out["rows_scaled_1e6"]["forward"] >= 100.0 * dr.C_STAGE["forward"], out
    assert out["rows_scaled_1e6"]["composed"] >= 100.0 * dr.C_STAGE["composed"], out
