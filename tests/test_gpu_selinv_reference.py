"""Every kernel of one sgo_marginals_selected call on the device against tests/selinv_reference.check, on the cases of
tests/mfront_cases.py -- the three selinv_reference.ILL_CONDITIONED lists included: the stage bounds carry no condition number.

Per case: sgo_set_graph_se2 (the path must be the multifrontal one), optimize(1), the case's poses again, ONE call and ONE export of
what it left resident (the factor it made, YINV, the second arena).  The device's tables equal the host plan's, the shape classes
selinv_reference.COVERS names for the case are reached by the device's own front table, then the stage checks.  A second arena
that is zeroed once and reused is covered by the session on lattice_50: a call at poses moved by 1e-6 must rewrite every entry,
and a call after an interleaved sgo_factor_solve must give the bits of the call before it.  Every test prints its ratios."""
import numpy as np
import pytest

import mfront_cases as mc
import selinv_reference as sr
from sparse_gslam_amd import capi

pytestmark = pytest.mark.gpu
EXPORT = ("INFO", "FRONTS", "BND", "PINV", "ELIM_VERTEX", "ARENA", "YINV", "SEL", "FLAGS")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _pairs(c):
    return np.r_[c.ei, c.ej], np.r_[c.ej, c.ei]       # every edge in both orientations (fixed endpoints: zero blocks)


def _open(o, c):
    o.set_graph(*c.arrays())
    assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
    o.optimize(1)
    o.set_poses(c.poses)


def _passes(name, c, X, D, cov, refs=None):
    vi, vj = _pairs(c)
    assert not X["FLAGS"][0]
    R = sr.check(c.as_dict(), X, D, cov, vi, vj, refs=refs)
    print(sr.report(name, R))
    print("worst_by_stage", name, {k: float(f"{v:.4g}") for k, v in sr.worst_by_stage(R).items()})
    assert not sr.failures(R), sr.report(name, R)


@pytest.mark.parametrize("name", mc.NAMES)
def test_selinv_stages(name):
    c = mc.make(name)
    vi, vj = _pairs(c)
    with mc.environment(c.env):
        plan = capi.mfront_plan_arrays(*c.arrays()[:4])
        with capi.Optimizer(0, direct_rows=1) as o:
            _open(o, c)
            D, cov = o.marginals_selected(vi, vj)
            X = o.mfront_arrays(EXPORT)
    for k in set(EXPORT) & set(capi.MFRONT_PLAN_ARRAYS):
        assert np.array_equal(X[k], plan[k]), (name, k)
    reached = sr.coverage(X)
    assert reached == sr.coverage(plan)
    for cls, at in sr.COVERS.items():
        assert at != name or reached[cls], (name, cls)
    _passes(name, c, X, D, cov)


@pytest.fixture(scope="module")
def session():
    """lattice_50: a call at P0, a call at P0 + 1e-6 noise, sgo_factor_solve, a third call -- and the export after each call"""
    c = mc.make("lattice_50")
    vi, vj = _pairs(c)
    rng = np.random.default_rng(21)
    P1 = c.poses + 1e-6 * rng.standard_normal(c.poses.shape) * (~c.fixed)[:, None]
    out = []
    with mc.environment(c.env), capi.Optimizer(0, direct_rows=1) as o:
        _open(o, c)
        for step in range(3):
            if step == 1:
                o.set_poses(P1)
            if step == 2:
                o.factor_solve(rng.standard_normal((3, o.n_free, 3)))
            D, cov = o.marginals_selected(vi, vj)
            out.append((o.mfront_arrays(EXPORT), D, cov))
    return c, P1, out


def test_a_second_call_at_moved_poses_rewrites_every_entry(session):
    c, P1, out = session
    moved = mc.Case(c.name, P1, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
    refs = [np.full(X["SEL"].size, np.nan) for X, _, _ in out[:2]]
    vi, vj = _pairs(c)
    sr.check(c.as_dict(), *out[0], vi, vj, refs=refs[0])
    _passes("lattice_50, second call", moved, *out[1], refs=refs[1])           # against the SECOND factor
    own = ~np.isnan(refs[1])
    assert np.array_equal(own, ~np.isnan(refs[0])) and own.sum() > 100000
    same = own & (_bits(out[0][0]["SEL"]) == _bits(out[1][0]["SEL"]))
    excused = same & (refs[0] == refs[1])
    print(f"lattice_50: {int(own.sum())} stored entries of the own columns; {int(same.sum())} keep their bits, {int(excused.sum())} of them with an "
          "unchanged reference value (the gathered entries are their bit copies: the gather stage)")
    assert not (same & ~excused).any(), np.flatnonzero(same & ~excused)[:8]
    assert same.sum() <= 1e-3 * own.sum()           # (the poses did move)


def test_a_call_after_an_interleaved_factor_solve(session):
    c, P1, out = session
    moved = mc.Case(c.name, P1, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
    _passes("lattice_50, after sgo_factor_solve", moved, *out[2])
    # the same poses, the same arithmetic in a fixed order: the bits of the call before sgo_factor_solve rewrote the factor's arrays
    for k in ("ARENA", "YINV", "SEL"):
        assert np.array_equal(_bits(out[1][0][k]), _bits(out[2][0][k])), k
    assert np.array_equal(_bits(out[1][1]), _bits(out[2][1])) and np.array_equal(_bits(out[1][2]), _bits(out[2][2]))
