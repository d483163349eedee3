"""The joint table's reference on the CPU (tests/joint_reference.py; no GPU): on every case of tests/mfront_cases.py, with the 48
candidates of fsolve_reference.candidates (a fixed-to-free one and a both-fixed one among them),
  * S from the fp64 model of sgo_fsolve.hip's recurrence (fsolve_reference.model's X) and d2 of the subset list are within
    selinv_reference.MODEL_BAR = 1e-8 of the table from the long-double-refined columns and its long-double Cholesky -- except on the
    cases selinv_reference.ILL_CONDITIONED lists, where they must be ABOVE the bar (listed <=> above) and finite;
  * the reference's own fp64 Cholesky stays within 1e-9 of the long-double one (three orders under DEVICE_BAR) on the kept cases;
and the comparison rejects a table without its cross blocks, one not symmetrised and one without Omega^-1.  Every test prints what
it measured."""
import os
import re

import numpy as np
import pytest

import fsolve_reference as fr
import joint_reference as jr
import marginals_reference as mref
import mfront_cases as mc
import selinv_reference as sr
from oracle import np_oracle as npo
from sparse_gslam_amd import capi

_CACHE = {}


def _case(name, k=jr.K):
    """(case, plan, H, candidates, R, e, refined X, size of its last correction, reference S, reference d2 of the subset list, the
    masks): computed once per case and shared, never modified."""
    if (name, k) not in _CACHE:
        c = mc.make(name)
        with mc.environment(c.env):
            A = capi.mfront_plan_arrays(*c.arrays()[:4])
        H = mref.hessian(c.poses, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
        cand = fr.candidates(c, k)
        R, e = fr.rhs(c.poses, c.fixed, *cand[:3])
        Xr, last = fr.refined(H, R)
        Sr = jr.joint_table(R, Xr, e, cand[3])
        M = jr.masks(jr.subsets(k), k)
        d2r = jr.all_d2(Sr, e, M, long=True)
        for a in (R, e, Xr, Sr, d2r, M):
            a.setflags(write=False)
        _CACHE[(name, k)] = (c, sr.Plan(A, c.fixed), H, cand, R, e, Xr, last, Sr, d2r, M)
    return _CACHE[(name, k)]


def test_symbols_are_bound():
    L = capi.lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgo.h")).read()
    for name in ("sgo_candidate_joint", "sgo_joint_subsets", "sgo_joint_pairs"):
        assert name in capi.SYMBOLS and hasattr(L, name) and re.search(r"\bint " + name + r"\(sgo_ctx\* ctx", src), name
    assert f"#define SGO_JOINT_MAX_CANDIDATES {capi.JOINT_MAX_CANDIDATES}" in src and capi.JOINT_MAX_CANDIDATES == jr.MAX_CANDIDATES == 256
    assert f"#define SGO_JOINT_MAX_SUBSET {capi.JOINT_MAX_SUBSET}" in src and capi.JOINT_MAX_SUBSET == jr.MAX_SUBSET == 40
    assert L.sgo_version() == 107


def test_the_subset_list_is_what_the_tests_say():
    lists = jr.subsets(jr.K)
    sizes = [len(s) for s in lists]
    assert sizes[0] == 0 and sizes[1:1 + jr.K] == [1] * jr.K and list(lists[1 + jr.K]) == [0, 1]
    assert sizes[2 + jr.K:5 + jr.K] == [5, 6, 11] and list(lists[5 + jr.K]) == list(range(40))
    assert len(lists) == jr.K + 9 and all(8 <= n <= 40 for n in sizes[-3:])
    assert all(np.all(np.diff(s) > 0) for s in lists if len(s) > 1)
    M = jr.masks(lists, jr.K)
    assert M.shape == (jr.K + 9, jr.K) and np.array_equal(M.sum(1), sizes)
    c = mc.make("contributions")            # two fixed vertices: candidate 0 fixed-to-free, candidate 1 both fixed
    ci, cj, _, _ = fr.candidates(c, jr.K)
    assert c.fixed[ci[0]] and not c.fixed[cj[0]] and c.fixed[ci[1]] and c.fixed[cj[1]]


@pytest.mark.parametrize("name", mc.NAMES)
def test_model_meets_the_bar_on_table_and_subsets(name):
    c, plan, H, (ci, cj, meas, info), R, e, Xr, last, Sr, d2r, M = _case(name)
    X = fr.to_hessian_order(plan, fr.model(plan, H, R)[1])
    S = jr.joint_table(R, X, e, info)
    d2 = jr.all_d2(S, e, M)
    rs, rd = jr.table_ratio(S, Sr), jr.rel(d2, d2r)
    gap = jr.rel(jr.all_d2(Sr, e, M), d2r)
    cond = float(np.linalg.cond(Sr))
    print(f"{name}: S {rs:.3e}, d2 {rd:.3e} of the refined reference; fp64 / long-double Cholesky of the reference {gap:.1e}; "
          f"cond(S) {cond:.2e}; last correction {last:.1e}")
    assert np.array_equal(S, S.T) and np.array_equal(Sr, Sr.T)
    assert d2[0] == 0.0 and d2r[0] == 0.0
    both = np.flatnonzero(c.fixed[ci] & c.fixed[cj])
    O = npo.info_full(info)
    for t in both:                           # S_tt = Omega^-1 and zero cross blocks
        blk = S[3 * t:3 * t + 3].copy()
        assert np.array_equal(blk[:, 3 * t:3 * t + 3], np.linalg.inv(O[t]))
        blk[:, 3 * t:3 * t + 3] = 0.0
        assert not blk.any()
    if name in sr.ILL_CONDITIONED:
        assert max(rs, rd) > sr.MODEL_BAR, (name, rs, rd, "the case meets the bar: it is an accuracy case")
        assert np.isfinite(S).all() and np.isfinite(d2).all()
    else:
        assert last <= 1e-12, last
        assert rs <= sr.MODEL_BAR and rd <= sr.MODEL_BAR, (name, rs, rd)
        assert gap <= 1e-3 * sr.DEVICE_BAR, (name, gap)


@pytest.mark.parametrize("name", ["tree_shapes", "child_own3_33"])
@pytest.mark.parametrize("mut", [None, "cross_dropped", "not_symmetrised", "no_omega"])
def test_the_comparison_rejects_a_wrong_table(name, mut):
    c, plan, H, (ci, cj, meas, info), R, e, Xr, last, Sr, d2r, M = _case(name)
    S = jr.joint_table(R, Xr, e, info, mut=mut)
    d2 = jr.all_d2(0.5 * (S + S.T) if mut == "not_symmetrised" else S, e, M)
    rs, rd = jr.table_ratio(S, Sr), (jr.rel(d2, d2r) if np.isfinite(d2).all() else np.inf)
    sym = np.array_equal(S, S.T)
    ok = rs <= sr.MODEL_BAR and rd <= sr.MODEL_BAR and sym
    multi = M.sum(1) > 2
    drop = jr.rel(d2[multi], d2r[multi]) if np.isfinite(d2).all() else np.inf
    print(f"{name} / {mut}: S {rs:.3e}, d2 {rd:.3e}, symmetric {sym}; d2 of the subsets of more than two moves by up to {drop:.3e}")
    assert ok == (mut is None), (name, mut, rs, rd, sym)
    if mut == "cross_dropped":
        assert drop >= 0.11, drop            # the joint number is not the sum of the single ones


def test_the_small_candidate_set_too():
    """k = 21 (fsolve_reference.K): the table's diagonal blocks are the gate's Omega^-1 + P and its singletons the gate's d2"""
    c, plan, H, (ci, cj, meas, info), R, e, Xr, last, Sr, d2r, M = _case("tree_shapes", fr.K)
    P, d2g = fr.gate(R, Xr, e, info)
    O = npo.info_full(info)
    for t in range(fr.K):
        want = np.linalg.inv(O[t]) + P[t]
        assert np.abs(Sr[3 * t:3 * t + 3, 3 * t:3 * t + 3] - want).max() <= 1e-13 * np.abs(want).max()
    assert jr.rel(d2r[1:1 + fr.K], d2g) <= 1e-10


def test_a_candidate_listed_twice():
    """{a, a'} identical: d2 = 2 e^T (Omega^-1 + 2 P)^-1 e"""
    c, plan, H, (ci, cj, meas, info), R, e, Xr, last, Sr, d2r, M = _case("tree_shapes", fr.K)
    O = npo.info_full(info)
    for a in (0, 3, 7):
        dup = np.r_[np.arange(fr.K), a]
        R2, e2 = fr.rhs(c.poses, c.fixed, ci[dup], cj[dup], meas[dup])
        X2 = np.concatenate([Xr, Xr[:, 3 * a:3 * a + 3]], axis=1)
        S2 = jr.joint_table(R2, X2, e2, info[dup])
        m = np.zeros(fr.K + 1, dtype=np.uint8)
        m[[a, fr.K]] = 1
        P = S2[3 * a:3 * a + 3, 3 * fr.K:]
        want = 2.0 * e[a] @ np.linalg.solve(np.linalg.inv(O[a]) + 2.0 * P, e[a])
        got, got_long = jr.subset_d2(S2, e2, m), jr.subset_d2_long(S2, e2, m)
        assert abs(got - want) <= 1e-9 * want and abs(got_long - want) <= 1e-9 * want, (a, got, got_long, want)


def test_a_table_that_is_not_positive_definite_gives_nan():
    S = np.array([[1.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]])
    e = np.ones((1, 3))
    assert np.isnan(jr.subset_d2(S, e, [1])) and np.isnan(jr.subset_d2_long(S, e, [1]))
    assert jr.subset_d2(S, e, [0]) == 0.0 and jr.subset_d2_long(S, e, [0]) == 0.0
