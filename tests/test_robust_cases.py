"""tests/robust_cases.py on the CPU: the table covers what it says, the fp64 statement of the kernels (robust_reference.rho) alone
meets the bound the device is held to, the comparison notices every listed wrong statement at a point of the table, and the cell
graph is what its docstring says -- e^T Omega e the table's e2 bit for bit, the closed form np_oracle's system."""
import numpy as np
import pytest

import robust_cases as rc
import robust_reference as rr
from oracle import np_oracle as npo

POINTS = rc.POINTS


def _pairs(mutation=None):
    out = [rr.rho(p.kind, p.e2, p.d, mutation) for p in POINTS]
    return np.array([float(a) for a, _ in out]), np.array([float(b) for _, b in out])


def test_long_double_is_wider_than_the_bound_needs():
    assert np.finfo(np.longdouble).eps < 2e-19


def test_the_table_covers_both_sides_of_every_threshold():
    kind, d, e2 = rc.arrays()
    assert np.isfinite(e2).all() and (e2 >= 0).all()
    assert set(kind) == set(range(10))
    for p in POINTS:
        assert p.solve == (2.0 ** -20 <= p.e2 <= 2.0 ** 20)
        b = rr.branch(p.kind, p.e2, p.d)
        assert (b is None and p.branch is None) or bool(b) == p.branch, p      # the declared side is the fp64 predicate's
    for k in rr.PIECEWISE:
        pts = [p for p in POINTS if p.kind == k and p.d > 0]
        thr = [p for p in pts if p.e2 == float(rr.threshold(k, p.d))]
        assert len(thr) == 1 and thr[0].branch is True and thr[0].e2 == 16.0, rr.NAMES[k]
        near = [p for p in pts if p.e2 == 16.0 and p.d in (np.nextafter(thr[0].d, 0.0), np.nextafter(thr[0].d, np.inf))]
        assert sorted(p.branch for p in near) == [False, True], rr.NAMES[k]
        assert any(p.e2 == 0.0 for p in pts)
        far = [p for p in pts if not 0.5 <= p.e2 / float(rr.threshold(k, p.d)) <= 2.0 and p.e2 > 0]
        assert {p.branch for p in far} == {False, True} and all(p.solve for p in far)
    # the pair that separates sqrt(e2) <= d from e2 <= d d
    split = [p for p in POINTS if p.d == rc.D_SPLIT]
    assert sorted(p.kind for p in split) == [rr.HUBER, rr.TUKEY, rr.SATURATED]
    for p in split:
        assert p.e2 == 1.6123582984512492 and np.sqrt(p.e2) <= p.d and not p.e2 <= p.d * p.d
        assert p.branch == (p.kind == rr.TUKEY)
    # the smooth kinds: the listed ratios with both d, Welsch's first exact zero and the value before it
    z, zp = rc._welsch_zero()
    assert np.exp(-z) == 0.0 and np.exp(-zp) > 0.0 and np.nextafter(zp, np.inf) == z
    for k in (rr.PSEUDO_HUBER, rr.CAUCHY, rr.GEMAN_MCCLURE, rr.WELSCH, rr.FAIR):
        for d in (0.5, 4.0):
            xs = {p.e2 / (d * d) for p in POINTS if p.kind == k and p.d == d}
            assert xs >= {0.0, 2.0 ** -60, 2.0 ** -30, 2.0 ** -10, 1.0, 2.0 ** 10, z, zp, 1e150}, (rr.NAMES[k], d)
    assert float(rr.rho(rr.WELSCH, z * 16.0, 4.0)[1]) == 0.0 and float(rr.rho(rr.WELSCH, zp * 16.0, 4.0)[1]) > 0.0
    assert any(p.kind == rr.DCS and p.d == 0.0 for p in POINTS) and any(p.kind == rr.NONE for p in POINTS)


def test_the_fp64_statement_alone_meets_the_bound():
    r0, w = _pairs()
    bad, worst = rc.check(POINTS, r0, w, "fp64")
    print("fp64 statement against long double, worst ratio to the bound per kind:", {k: round(v, 4) for k, v in worst.items()})
    assert not bad, bad
    assert all(v <= 1.0 for v in worst.values())


@pytest.mark.parametrize("mutation", rr.MUTATIONS)
def test_the_comparison_notices(mutation):
    r0, w = _pairs(mutation)
    bad, _ = rc.check(POINTS, r0, w, mutation)
    by_values = [b for b in bad]
    # a `<` for `<=` in a kind that is continuous at its threshold changes no value there: the side itself is what differs
    kind = dict(dcs_lt=rr.DCS, huber_lt=rr.HUBER, tukey_lt=rr.TUKEY, saturated_lt=rr.SATURATED).get(mutation)
    sides = [p for p in POINTS if kind is not None and p.kind == kind and bool(rr.branch(p.kind, p.e2, p.d, mutation)) != p.branch]
    print(mutation, "caught by values at", [(b[2], b[3], b[4], b[8]) for b in by_values], "by the side at", [(p.d, p.e2) for p in sides])
    assert by_values or sides
    if kind is not None:
        assert (16.0 if kind == rr.DCS else 4.0, 16.0) in [(p.d, p.e2) for p in sides]      # the threshold itself
    else:
        assert by_values


def test_the_other_side_of_a_threshold_is_told_apart_where_it_differs():
    """observed_branch on the reference's own two sides: wherever the sides' weights differ it names the side; at the thresholds of
    the continuous kinds (DCS, Huber, Tukey at d = 4, e2 = 16) and where a side has no finite weight (Huber's d / s at e2 = 0) it
    says so by returning None"""
    none = []
    for p in POINTS:
        if p.branch is None:
            continue
        ws = [float(rr.rho_ld(p.kind, p.e2, p.d, lo=np.bool_(s))[1]) for s in (True, False)]
        if ws[0] == ws[1] or not np.isfinite(ws).all():
            none.append((p.kind, p.d, p.e2))
            assert rc.observed_branch(p, ws[0]) is None
        else:
            assert rc.observed_branch(p, ws[0]) is True and rc.observed_branch(p, ws[1]) is False
    # (at the pair that separates the predicates sqrt(e2) is d itself: Huber's d / s is 1 on either side; Saturated's jump shows)
    assert sorted(none) == sorted([(rr.DCS, 16.0, 16.0), (rr.HUBER, 4.0, 16.0), (rr.TUKEY, 4.0, 16.0), (rr.HUBER, 4.0, 0.0),
                                   (rr.HUBER, rc.D_SPLIT, 1.6123582984512492)]), none


def test_the_cell_graph_is_what_the_closed_form_says():
    C = rc.cells()
    n = C.n_anchor
    assert C.poses.shape[0] == 3 * n and n == 2 * len(POINTS)
    assert np.array_equal(64 * C.poses, np.round(64 * C.poses)) and not C.poses[:, 1:].any() and C.poses.max() < 16   # a line, theta = 0
    e = npo.edge_error(C.poses[C.ei], C.poses[C.ej], C.meas)
    assert np.array_equal(e[:n], np.tile(rc.E_ANCHOR, (n, 1))) and np.array_equal(e[n:], np.tile([1.0, 0.0, 0.0], (n, 1)))
    O = npo.info_full(C.info)
    e2 = np.einsum("ni,nij,nj->n", e, O, e)
    assert np.array_equal(e2[n:].view(np.uint64), rc.arrays()[2][C.point].view(np.uint64))  # the table's e2, bit for bit
    # the closed form against np_oracle's linearisation with information w Omega
    r0, w, _, _ = rc.reference()
    w64 = np.ones(2 * n)
    w64[n:] = w[C.point].astype(np.float64)
    H, b, _, _ = npo.linearize(C.poses, C.fixed.astype(bool), C.ei, C.ej, C.meas, C.info * w64[:, None], np.full(2 * n, -1.0))
    H = H.toarray()
    Hc, bc, Ha, ba, _, _ = rc.cell_systems(C, POINTS, w)
    for k in range(n):
        s = slice(3 * k, 3 * k + 3)
        assert np.abs(H[s, s] - Hc[k].astype(np.float64)).max() <= 1e-14 * float(Ha[k].max())
        assert np.abs(b[s] - bc[k].astype(np.float64)).max() <= 1e-14 * float(ba[k].max())
    assert np.count_nonzero(H) <= 9 * n                                                      # block diagonal
    # the step of a cell solves its system
    sel = [t for t, p in enumerate(POINTS) if p.solve]
    Cs = rc.cells([POINTS[t] for t in sel])
    dx, dw = rc.cell_steps(Cs, [POINTS[t] for t in sel], w[sel])
    Hs, bs = rc.cell_systems(Cs, [POINTS[t] for t in sel], w[sel])[:2]
    for k in range(Cs.point.size):
        assert float(np.abs(Hs[k] @ dx[k] - bs[k]).max()) <= 1e-17 * float(np.abs(Hs[k]).max() * np.abs(dx[k]).max() + np.abs(bs[k]).max())
    assert np.isfinite(dx.astype(np.float64)).all() and (dw >= 0).all()
