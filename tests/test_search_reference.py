"""tests/search_reference.py, the numpy reference of sgo_closure_search, qualified on the CPU before tests/test_gpu_closure_search.py
holds the device to it: the block formula against a route that shares no cancellation with it, the half-plane bound against the
disc, and the conditions under which the device's decisions are compared (asserted on the reference alone).  Every test prints
what it measured."""
import numpy as np

import fsolve_reference as fr
import search_reference as sr
from selinv_reference import DEVICE_BAR
from test_gpu_hypotheses import DIRECT, graph

RADIUS, GATE = 2.0, 6.635     # metres; the 99 % quantile of chi2 with 1 degree of freedom


def _reference(g):
    return sr.Reference(g.poses, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi)


def test_block_formula_equals_the_non_cancelling_route():
    """P from the four blocks of Sigma against R^T H^-1 R of fsolve_reference.gate for the candidate edge (j, c) whose measurement
    is rel.  With that measurement the edge's error lives in c's frame: its Jacobians are Rz times the reference's, Rz the
    rotation by -phi, so the gate's matrix is Rz P Rz^T exactly (a similarity: m2 and sigma do not see it).  The block route
    cancels (A Sjj A^T against the cross terms), the gate's route is one quadratic form.  A reference is fit to hold the device
    to 9 DEVICE_BAR scale when its two routes agree to a thousandth of that."""
    g = graph(DIRECT)
    S = _reference(g)
    c = g.V - 1
    ids = np.r_[0, np.random.default_rng(11).choice(np.arange(1, g.V - 1), 40, replace=False)]
    worst = 0.0
    for j in ids:
        r = S.pair(int(j), c, RADIUS)
        R, e = fr.rhs(g.poses, g.fixed, np.array([j]), np.array([c]), r["rel"][None])
        assert np.abs(e).max() <= 1e-12, e
        Pg, _ = fr.gate(R, S.lu.solve(R), e, np.array([[1.0, 0, 0, 1.0, 0, 1.0]]))
        cz, sz = np.cos(-r["rel"][2]), np.sin(-r["rel"][2])
        Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
        worst = max(worst, float(np.abs(Rz @ r["P"] @ Rz.T - Pg[0]).max() / (9.0 * DEVICE_BAR * r["scale"])))
    print(f"block formula against R^T H^-1 R on {ids.size} pairs: worst difference {worst:.3g} of the device's bar")
    assert worst <= 1e-3


def test_m2_is_a_lower_bound_of_the_distance_to_the_disc():
    g = graph(DIRECT)
    S = _reference(g)
    R = S.search([g.V - 1, 300], np.arange(g.V), RADIUS, GATE)
    checked, tightest = 0, np.inf
    for a in range(2):
        for j in np.flatnonzero((R["m2"][a] > 0.0) & np.isfinite(R["m2"][a]))[::7]:
            exact = sr.boundary_minimum(R["rel"][a, j], R["P"][a, j], RADIUS)
            assert R["m2"][a, j] <= exact * (1.0 + 1e-12), (a, j, R["m2"][a, j], exact)
            tightest = min(tightest, exact / R["m2"][a, j])
            checked += 1
    print(f"{checked} pairs: m2 <= the minimum over 720 boundary points everywhere, the tightest ratio {tightest:.6g}")
    assert checked >= 100


def test_conditions_of_the_decision_test_and_what_the_search_finds():
    """At least 95 % of all pairs and 90 % of the reference's near pairs must be decidable (search_reference.decided), and the
    covariance-aware search keeps more poses than the Euclidean threshold"""
    g = graph(DIRECT)
    S = _reference(g)
    for c in (g.V - 1, 300):
        R = S.search([c], np.arange(g.V), RADIUS, GATE)
        dec = sr.decided(R, RADIUS, GATE)[0]
        near = R["near"][0]
        within = (R["norm"][0] <= RADIUS) & (np.arange(g.V) != c)
        others = np.arange(g.V) != c
        loose = np.median(9 * DEVICE_BAR * R["scale"][0, others] / np.abs(R["P"][0, others]).reshape(-1, 9).max(1))
        print(f"query {c}: {within.sum()} poses within {RADIUS} m, {near.sum()} near at chi2 {GATE}; decided {dec.mean():.1%} of the pairs, "
              f"{(dec & near).sum()} of {near.sum()} near pairs; median 9 BAR scale / |P|max {loose:.3g}")
        assert dec.mean() >= 0.95 and (dec & near).sum() >= 0.9 * near.sum()
        assert not near[c] and R["m2"][0, c] == 0.0 and not R["P"][0, c].any()
        assert (near | ~within)[np.arange(g.V) != c].all()                  # a pose inside the radius is never dropped
        if c == g.V - 1:
            assert near.sum() > within.sum() > 0, (near.sum(), within.sum())


def test_fixed_poses_drop_out():
    g = graph(DIRECT)
    S = _reference(g)
    f = int(np.flatnonzero(g.fixed)[0])
    r = S.pair(f, g.V - 1, RADIUS)
    A, B = sr.jacobians(g.poses[f], g.poses[g.V - 1])
    assert np.abs(r["P"] - B @ S.block(g.V - 1, g.V - 1) @ B.T).max() <= 1e-15 * r["scale"]
    r = S.pair(g.V - 1, f, RADIUS)
    A, B = sr.jacobians(g.poses[g.V - 1], g.poses[f])
    assert np.abs(r["P"] - A @ S.block(g.V - 1, g.V - 1) @ A.T).max() <= 1e-15 * r["scale"]
    r = sr.pair(g.poses[f], g.poses[g.V - 1], None, None, None, 0.5)
    assert not r["P"].any() and r["m2"] == np.inf and not r["sigma"].any()
