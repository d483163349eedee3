"""tests/wrap_cases.py qualified on the CPU: the table's exactness condition in exact rationals, every host statement of the wrap
against every other bit for bit, the cells' closed forms against np_oracle, and wrong wraps that the table must catch -- each
mutant names the points that catch it.  No GPU; tests/test_gpu_wrap_points.py carries the same table through the kernels."""
import math
from fractions import Fraction

import numpy as np

import wrap_cases as wc
from oracle import c_oracle, np_lm_oracle
from oracle import np_oracle as npo
from sparse_gslam_amd import capi, synth

PI, TWO_PI = wc.PI, wc.TWO_PI
POINTS = wc.POINTS


def test_the_table_covers_what_it_says():
    kinds = {p.kind for p in POINTS}
    assert kinds == {"branch", "range", "part", "side", "small", "interior"}
    es = {(p.why.split(":")[0].split(" ")[0], wc.route(p.ti, p.tj, p.zeta)["e"]) for p in POINTS if p.kind == "branch"}
    for way in ("outer", "inner"):
        assert {(way, -PI), (way, PI - wc.ULP)} <= es            # pi -> -pi and -pi stays; pi - ulp stays and -pi - ulp -> pi - ulp
    assert {("prepare", -PI), ("prepare", PI - wc.ULP)} <= es
    # each of the four landings is an argument of the named wrap, by each of the three ways
    for L, _ in wc.LANDINGS:
        hit = {"outer": False, "inner": False, "prepare": False}
        for p in POINTS:
            r = wc.route(p.ti, p.tj, p.zeta)
            if p.why.startswith("outer") and r["s2"] == L and -PI <= r["s1"] < PI:
                hit["outer"] = True
            if p.why.startswith("inner") and r["s1"] == L:
                hit["inner"] = True
            if p.why.startswith("prepare") and r["s2"] == L and not (-PI < -p.zeta < PI):
                hit["prepare"] = True
        assert hit["outer"] and hit["inner"], (L, hit)
        assert hit["prepare"], (L, hit)
    assert any(p.ti == PI for p in POINTS) and any(p.ti == -PI for p in POINTS)
    assert all(wc.route(t, 0.5, 0.0)["tin"] == -PI for t in (PI, -PI))
    assert wc.route(PI, -PI, 0.0)["s1"] == -TWO_PI and wc.route(PI, -PI, 0.0)["e"] == 0.0


def test_exactness_of_every_branch_point_and_update_cell():
    """No rounding decides a side: on a branch point every fp64 operation of the route is exact in rationals."""
    for p in POINTS:
        if p.kind == "branch":
            assert wc.route_is_exact(p.ti, p.tj, p.zeta), p
    # (not vacuous: the condition is false where a rounding happens)
    assert not wc.route_is_exact(0.0, 1e6, 0.0) and not wc.route_is_exact(2.0 ** -60, 1.0, 0.0)
    C = wc.cells(points=())
    e, b, new, dx = wc.closed_form(C)
    for k, u in enumerate(wc.UPDATES):
        ti, tj = (u.tc, u.tv) if u.orient == 0 else (u.tv, u.tc)
        assert wc.route_is_exact(ti, tj, u.zeta), u
        assert Fraction(u.tv) + Fraction(float(dx[k])) == Fraction(u.landing), u          # theta_v + dx is the landing, exactly
        assert new[k] == wc.wrap(u.landing) and -PI <= new[k] < PI
    want = {PI: -PI, PI - wc.ULP: PI - wc.ULP, -PI: -PI, -PI - wc.ULP: PI - wc.ULP, 6.0: 6.0 - TWO_PI, -6.0: TWO_PI - 6.0}
    for o in (0, 1):
        got = {u.landing: new[k] for k, u in enumerate(wc.UPDATES) if u.kind == "exact" and u.orient == o}
        assert got == want, (o, got)
        # the shifted cells stand 2^-30 off a landing, on both sides of each
        sh = sorted(u.landing for u in wc.UPDATES if u.kind == "shifted" and u.orient == o)
        assert len(sh) == 8 and all(min(abs(abs(s) - PI), abs(abs(s) - (PI + wc.ULP))) <= 2.0 ** -30 + 2 * wc.ULP for s in sh)
        assert sum(u.kind == "interior" and u.orient == o for u in wc.UPDATES) >= 3


def test_the_parting_points_part():
    """`range`: the fused form gives the literal bits on the whole route.  `part`: another value on the same side.  `side`: a wrap on
    the route lands across the branch -- all in exact rationals, correctly rounded."""
    n_side = 0
    for p in POINTS:
        a, f = wc.route(p.ti, p.tj, p.zeta), wc.route(p.ti, p.tj, p.zeta, w=wc.wrap_fused)
        if p.kind in ("branch", "range", "interior"):
            assert a == f, p
        if p.kind == "part":
            assert a["e"] != f["e"] and abs(a["e"] - f["e"]) < 1e-10, (p, a["e"], f["e"])
        if p.kind == "side":
            across = [k for k in ("zinv", "tin", "dth", "e") if abs(a[k] - f[k]) > 6.0]
            assert across and a["e"] != f["e"], (p, a, f)
            n_side += abs(a["e"] - f["e"]) > 6.0
    assert n_side >= 2                                               # ... of which the error itself changes side
    assert wc.wrap(1e6) == -0.35756416701340044 and wc.wrap_fused(1e6) == -0.3575641670467533
    # fp64 pi ends in three zero bits: m 2pi is exact up to |m| = 10 and inexact at 11, which is why 7pi parts nowhere and 23pi does
    assert Fraction(PI).denominator == 2 ** 48                      # (ulp 2^-51: three spare bits)
    assert all(Fraction(m * TWO_PI) == m * Fraction(TWO_PI) for m in range(-10, 11))
    assert all(Fraction(m * TWO_PI) != m * Fraction(TWO_PI) for m in (11, 17, -19, 159154))


def _rule_rel2(t):
    """rel[2] of the library's host pair rule for theta_c - theta_j = t - 0 (host closure_norm_theta)"""
    rel, _, _, _ = capi.closure_search_rule(np.zeros(3), np.array([0.0, 0.0, t]), None, None, np.eye(3), 1.0)
    return rel[2]


def test_every_host_statement_of_the_wrap_agrees_bit_for_bit():
    args = wc.wrap_arguments(POINTS)
    assert args.size >= 60 and (np.abs(args) >= 1e5).any()
    want = np.array([wc.wrap(float(t)) for t in args])
    assert np.all((want >= -PI) & (want < PI))
    got = {
        "np_oracle.normalize_theta": npo.normalize_theta(args),
        "c_oracle.normalize_theta": np.array([c_oracle.normalize_theta(float(t)) for t in args]),
        "synth._wrap": synth._wrap(args),
        "np_lm_oracle.normalize_theta": np.array([np_lm_oracle.normalize_theta(float(t)) for t in args]),
        "capi.closure_search_rule rel[2]": np.array([_rule_rel2(float(t)) for t in args]),
    }
    for name, g in got.items():
        bad = np.flatnonzero(~wc.same(g, want))
        assert bad.size == 0, (name, [(float(args[k]).hex(), float(g[k]).hex(), float(want[k]).hex()) for k in bad])
    # the whole error, statement by statement
    xi, xj, z = (np.zeros((len(POINTS), 3)) for _ in range(3))
    xi[:, 2], xj[:, 2], z[:, 2] = [p.ti for p in POINTS], [p.tj for p in POINTS], [p.zeta for p in POINTS]
    e = np.array([wc.route(p.ti, p.tj, p.zeta)["e"] for p in POINTS])
    en = npo.edge_error(xi, xj, z)
    assert np.all(wc.same(en[:, 2], e)) and np.all(en[:, :2] == 0.0)
    ec = np.array([c_oracle.se2_mul(c_oracle.se2_inv(z[k]), c_oracle.se2_mul(c_oracle.se2_inv(xi[k]), xj[k])) for k in range(len(POINTS))])
    assert np.all(wc.same(ec[:, 2], e)) and np.all(ec[:, :2] == 0.0)


def test_the_cells_closed_forms_against_np_oracle():
    C = wc.cells()
    assert C.ti.size == 2 * len(POINTS) + len(wc.UPDATES) and C.poses.shape[0] <= 400
    e, b, new, dx = wc.closed_form(C)
    Hm, bb, c2, _ = npo.linearize(C.poses, C.fixed.astype(bool), C.ei, C.ej, C.meas, C.info, C.phi)
    Hm, bb = Hm.toarray(), bb.reshape(-1, 3)
    n = C.free.size
    assert np.all(wc.same(bb[:, 2], b)) and np.all(bb[:, :2] == 0.0)
    th = np.arange(2, 3 * n, 3)
    assert np.all(Hm[th, th] == 1.0)                                       # H_thth = 1 ...
    off = Hm[th].copy()
    off[np.arange(n), th] = 0.0
    assert np.all(off == 0.0)                                              # ... and theta is decoupled from everything, exactly
    assert c2 == float(np.sum(e * e)) or abs(c2 - np.sum(e * e)) <= 1e-12 * c2
    P, st = npo.gauss_newton(C.poses, C.fixed.astype(bool), C.ei, C.ej, C.meas, C.info, C.phi, iters=1)
    assert np.all(wc.same(P[C.free, 2], new)) and np.all(P[:, :2] == 0.0)
    assert np.all(wc.same(P[C.c], C.poses[C.c]))
    assert np.all((new >= -PI) & (new < PI))
    # the coupled cells: e_x is not zero, and the side of e_theta shows in e^2 -- by far more than kernel_reference's bound
    import kernel_reference as kr
    K = wc.cells(coupled=True)
    ref = kr.reference(K.poses, K.fixed.astype(bool), K.ei, K.ej, K.meas, K.info, K.phi)
    ee = npo.edge_error(K.poses[K.ei], K.poses[K.ej], K.meas)
    assert np.all(wc.same(ee[:, 2], e)) and np.abs(ee[:, 0]).min() > 0.05
    flipped = 4.0 * wc.INFO_COUPLED[2] * np.abs(ee[:, 0] * ee[:, 2])       # what e_theta -> -e_theta moves of e^2
    at_pi = np.abs(np.abs(e) - PI) < 1e-9
    assert at_pi.sum() >= 40 and np.all(flipped[at_pi] > 1e6 * kr.C * kr.U * ref.e2_abs[at_pi])


# ------------------------------------------------------------------ mutants: wrong wraps the table must catch
def _post(t):
    if t >= PI:
        t -= TWO_PI
    if t < -PI:
        t += TWO_PI
    return t


def m_half_open_the_other_way(t):
    """the range (-pi, pi]"""
    if -PI < t <= PI:
        return t
    t = t - math.floor(t / TWO_PI) * TWO_PI
    if t > PI:
        t -= TWO_PI
    if t <= -PI:
        t += TWO_PI
    return t


def m_no_wrap(t):
    return t


def m_one_if(t):
    """one step of 2pi, no floor"""
    return _post(t)


def m_fmod(t):
    return math.fmod(t + PI, TWO_PI) - PI


def m_remainder(t):
    return math.remainder(t, TWO_PI)


def m_atan2(t):
    return math.atan2(math.sin(t), math.cos(t))


def _err(w, inner=True, outer=True, prepare=True):
    def e(p):
        zinv = w(-p.zeta) if prepare else -p.zeta
        s1 = w(-p.ti) + p.tj
        dth = w(s1) if inner else s1
        s2 = zinv + dth
        return w(s2) if outer else s2
    return e


MUTANTS = {
    "the range (-pi, pi]": _err(m_half_open_the_other_way),
    "no wrap": _err(m_no_wrap),
    "one if, no floor": _err(m_one_if),
    "fmod": _err(m_fmod),
    "remainder": _err(m_remainder),
    "atan2(sin, cos)": _err(m_atan2),
    "the fused product": _err(wc.wrap_fused),
    "no inner wrap": _err(wc.wrap, inner=False),
    "no outer wrap": _err(wc.wrap, outer=False),
    "zeta not wrapped at prepare": _err(wc.wrap, prepare=False),
}


def test_every_mutant_is_caught_and_by_which_points():
    assert all(_err(wc.wrap)(p) == wc.route(p.ti, p.tj, p.zeta)["e"] for p in POINTS)       # the harness itself is the specification
    caught = {}
    for name, f in MUTANTS.items():
        hits = [t for t, p in enumerate(POINTS) if not f(p) == wc.route(p.ti, p.tj, p.zeta)["e"]]
        caught[name] = hits
        kinds = sorted({POINTS[t].kind for t in hits})
        print(f"mutant {name!r}: caught by {len(hits)} of {len(POINTS)} points, kinds {kinds}; first: "
              + "; ".join(f"#{t} ({POINTS[t].why})" for t in hits[:3]))
    assert all(caught.values()), {k: v for k, v in caught.items() if not v}
    why = lambda name: {POINTS[t].kind for t in caught[name]}
    # what catches which: the boundary's side by the exact branch points, the fused product only by the parting points
    assert "branch" in why("the range (-pi, pi]") and "branch" in why("remainder") and "branch" in why("atan2(sin, cos)")
    assert "branch" in why("no outer wrap") and "range" in why("one if, no floor") and "range" in why("no wrap")
    assert why("the fused product") == {"part", "side", "small"}
    assert {"small"} <= why("no inner wrap") and {"small"} <= why("zeta not wrapped at prepare")
    # an update that forgets its wrap, or wraps the other way, is caught by the exact update cells
    C = wc.cells(points=())
    for w in (m_no_wrap, m_half_open_the_other_way):
        new_ok, new_bad = wc.closed_form(C)[2], np.array([w(float(C.poses[C.free[k], 2]) + float(wc.closed_form(C)[1][k]))
                                                          for k in range(C.ti.size)])
        assert (~wc.same(new_ok, new_bad)).any(), w.__name__
