"""The angle wrap at its branch points (sparse_gslam_amd/csrc/sgo_device.h: norm_theta; sgo_rules.h: closure_norm_theta): a table of
single-edge points, and a graph of cells that carries every point through the kernels bit for bit.  TEST INFRASTRUCTURE ONLY.

The specification is g2o::normalize_theta in fp64, every operation rounded on its own (oracle.np_oracle.normalize_theta): inside
[-pi, pi) the angle is returned; otherwise m = floor(t / 2pi), t - (m 2pi) -- the product rounded, then the difference -- and one
step of 2pi back where that left the range.  An edge error forms it four times: zinv = wrap(-zeta) once per edge (k_edge_prepare),
tin = wrap(-theta_i), dth = wrap(tin + theta_j) (the inner wrap), e_theta = wrap(zinv + dth) (the outer one).

The table.  A Point is (ti, tj, zeta, kind, why); kind says what the point is there for and what tests/test_wrap_cases.py proves
of it on the CPU with exact rationals:
  branch    a wrap on the route lands on pi (-> -pi), pi - ulp (stays), -pi (stays) or -pi - ulp (-> pi - ulp), reached by the inner
            wrap, by the outer one, or behind k_edge_prepare's wrap of -zeta (zeta = -pi, pi, and 3/2 pi from outside the range);
            theta_i = +-pi (both give tin = -pi); -pi + -pi -> 0.  EXACTNESS: every fp64 operation on the route -- every sum, and
            inside every wrap the floor's argument, the product and the differences -- returns the exact rational result, so no
            rounding, fused or not, in any order, decides a side.  Built from halves of fp64 pi and differences inside a binade.
  range     caller-set angles outside [-pi, pi) whose product m 2pi is exact, so that the fused and the literal form agree: m a
            power of two (3pi, -3pi, 2pi + 0.5, -7), and every |m| <= 10, because fp64 pi ends in three zero bits (7pi and its
            neighbours, m = 3 and -4; the first inexact product is m = 11)
  part      m 2pi inexact: t - m 2pi contracted into one FMA rounds to another value than product-then-difference (1e6: 3e-11
            apart; fl(35 pi) and fl(-37 pi) and their neighbours, m = 17 and -19: a few ulp apart)
  side      ... and to the OTHER SIDE of the branch: fl(23 pi), fl(-25 pi), fl(53 pi) -- literal and fused results 2pi - 16 ulp apart
  small     where dropping one of the wraps changes the value's last bits although the angle is the same modulo 2pi (the mutants of
            the CPU test)
  interior  controls

The cell.  A fixed pose c and a free pose v, both at the ORIGIN, one edge with measurement (0, 0, zeta), information the identity,
no robust kernel; orientation 0 is c -> v (the free pose is the edge's second vertex, J = B), orientation 1 is v -> c (J = A).  At
the origin every translation term is a product with 0: e_x = e_y = 0, the theta row and column of A and B are (0, 0, -+1), so
H_thth = 1, H_xth = H_yth = 0 and b_th = -+e_theta exactly, whatever the order of evaluation and the contraction, and e^2 =
fl(e_theta^2).  The solve of such a block is exact in its theta row (pivot 1, zero coupling), so the update is
theta_v <- wrap(fl(theta_v + b_th)), one rounded sum and one wrap: bit for bit on every path whose solve is a factorisation.

The update cells (Update: orient, tc, tv, zeta, landing, kind, why) are cells whose zeta is chosen so that theta_v + dx_theta is exact
and lands on pi, pi - ulp, -pi, -pi - ulp, 6 (-> 6 - 2pi) or an interior value, with every sum on the way exact ("exact"), and the
same landings moved by +-2^-30 ("shifted"), for paths whose solve is not exact: 2^-30 is far above any solve's error and far below
anything that would hide a wrap to the wrong side.

The coupled cells are the same cells with measurement (0.5, -0.25, zeta) and information INFO_COUPLED, which has a theta-x entry:
there e_x = -(0.5 cos - 0.25 sin)(zinv) is not zero and the SIGN of e_theta shows in e^2 itself.  Their reference is
kernel_reference's (the error from the fp64 specification -- the side is the specification's --, products and sums in long double)
with its own bound C U abs.

MEASURED keeps what tests/test_gpu_wrap_points.py printed on an MI355X: figures to read, never a reason to move a bar."""
import collections
import math
from fractions import Fraction

import numpy as np

PI = math.pi
TWO_PI = 2.0 * PI
ULP = 2.0 ** -51                     # of fp64 pi (and of every fp64 in [2, 4))
Point = collections.namedtuple("Point", "ti tj zeta kind why")
Update = collections.namedtuple("Update", "orient tc tv zeta landing kind why")
INFO_ID = (1.0, 0.0, 0.0, 1.0, 0.0, 1.0)
INFO_COUPLED = (2.0, 0.0, 0.5, 1.0, 0.0, 1.0)       # upper triangle: Omega_x,theta = 0.5; positive definite
MEAS_COUPLED = (0.5, -0.25)

# figures of tests/test_gpu_wrap_points.py on an MI355X (see that file's docstring)
MEASURED = {
    # 170 cells (68 points in two orientations, 34 update cells); cells that differ from the closed form in any bit
    "k_linearize (group, tile)": 0, "k_chi2 / k_edge_robust": 0, "k_ov_lin (edge_chi2, 186 edges)": 0, "k_edge_cands (e_theta)": 0,
    "optimize(1) direct": 0, "optimize(1) mfront": 0, "optimize_lm(1, 1e-300)": "the bits of optimize(1)",
    "optimize_dogleg(1)": "the bits of optimize(1)", "k_closure_search (85 wrap arguments, rel[2])": 0,
    "k_edge_gate": "20 of 170 gated at chi2_max = (pi - ulp)^2, the flags of e^2 > chi2_max",
    # per path: (d_path, worst |theta - closed form| mod 2pi over 10 d_path |dx| with the cell's own |dx|, shifted cells on the wrong side,
    # cells bit-identical to the closed form)
    "optimize(1) pcg": (1e-14, 0.00307, 0, "52 of 170"), "optimize_lm_pcg(1, 1e-300)": (1e-14, 0.00307, 0, "52 of 170"),
    "optimize_dogleg_pcg(1)": (1e-14, 0.00307, 0, "52 of 170"),
    "optimize(1) overlay (178 chain rows, 8 hubs)": (1e-14, 0.0, 0, "186 of 186"),
    # coupled cells, error / (U abs) against kernel_reference, whose bound is 16
    "coupled": dict(b=0.229, diag=2.61, chi2=6.78e-5, robust_chi2=7.9e-5, edge_chi2=0.201, edge_robust=0.201),
    # against their own references, bars 1e-6
    "k_fs_rhs": dict(P=9.12e-17, d2=4.61e-16), "k_edge_cands (N)": 4.12e-16,
    "optimize_hypotheses": "the unbatched loop's bits",
    # the same tests on a library built WITHOUT contraction switched off in the wraps: linearize(): 34 of 170 cells with another
    # b_theta, the largest difference 6.28; closure_search: 12 of 85 arguments (NOTES.md section 50)
}


# ------------------------------------------------------------------ the wrap, stated once more, and traced in exact rationals
def wrap(t):
    """the specification on one Python float (every operation of a Python float expression is one IEEE fp64 operation)"""
    if t >= -PI and t < PI:
        return t
    m = math.floor(t / TWO_PI)
    p = m * TWO_PI
    t = t - p
    if t >= PI:
        t -= TWO_PI
    if t < -PI:
        t += TWO_PI
    return t


def wrap_fused(t):
    """the wrap with t - m 2pi rounded ONCE (the FMA a contracting compiler makes of it): what the device computed before its
    norm_theta switched contraction off.  Exact rationals, correctly rounded (Fraction -> float rounds to nearest even)."""
    if t >= -PI and t < PI:
        return t
    m = math.floor(t / TWO_PI)
    t = float(Fraction(t) - Fraction(m) * Fraction(TWO_PI))
    if t >= PI:
        t -= TWO_PI
    if t < -PI:
        t += TWO_PI
    return t


def _is(x, f):
    """the float f is the rational x exactly"""
    return Fraction(f) == x


def wrap_exact(t):
    """-> (wrap(t), whether every operation inside returned the exact rational result)"""
    if t >= -PI and t < PI:
        return t, True
    T, P2 = Fraction(t), Fraction(TWO_PI)
    q = t / TWO_PI
    m = math.floor(q)
    ok = m == math.floor(T / P2)
    p = m * TWO_PI
    ok = ok and _is(m * P2, p)
    u = t - p
    ok = ok and _is(T - Fraction(p), u)
    if u >= PI:
        v = u - TWO_PI
        ok = ok and _is(Fraction(u) - P2, v)
        u = v
    if u < -PI:
        v = u + TWO_PI
        ok = ok and _is(Fraction(u) + P2, v)
        u = v
    return u, ok


def route(ti, tj, zeta, w=wrap):
    """The four wraps of one edge error with the wrap `w` -> dict of the wraps' arguments and results: zinv = w(-zeta),
    tin = w(-ti), s1 = tin + tj, dth = w(s1), s2 = zinv + dth, e = w(s2)."""
    zinv, tin = w(-zeta), w(-ti)
    s1 = tin + tj
    dth = w(s1)
    s2 = zinv + dth
    return dict(zinv=zinv, tin=tin, s1=s1, dth=dth, s2=s2, e=w(s2))


def route_is_exact(ti, tj, zeta):
    """the exactness condition of a branch point: both sums and the inside of all four wraps are exact"""
    r = route(ti, tj, zeta)
    ok = _is(Fraction(r["tin"]) + Fraction(tj), r["s1"]) and _is(Fraction(r["zinv"]) + Fraction(r["dth"]), r["s2"])
    for a in (-zeta, -ti, r["s1"], r["s2"]):
        ok = ok and wrap_exact(a)[1]
    return ok


def wrap_arguments(points):
    """every argument that reaches a wrap on the points' routes, without repeats: what k_closure_search is fed"""
    out = {}
    for p in points:
        r = route(p.ti, p.tj, p.zeta)
        for a in (-p.zeta, -p.ti, r["s1"], r["s2"], p.ti, p.tj, p.zeta):
            out.setdefault(float(a).hex(), float(a))
    return np.array(list(out.values()))


# ------------------------------------------------------------------ the table
def _step(x, n):
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


H = 0.5 * PI                                      # exact: a power of two times fp64 pi
LANDINGS = ((PI, "pi -> -pi"), (PI - ULP, "pi - ulp stays"), (-PI, "-pi stays"), (-PI - ULP, "-pi - ulp -> pi - ulp"))
SIDE = (float.fromhex("0x1.2106ca4910069p+6"), float.fromhex("-0x1.3a28c59d5433bp+6"), float.fromhex("0x1.4d02421c87558p+7"))
Z32 = 1.5 * PI                                    # fl(3/2 pi): outside the range, m = -1 for its negative


def _points():
    P = []

    def add(ti, tj, zeta, kind, why):
        P.append(Point(float(ti), float(tj), float(zeta), kind, why))

    for L, what in LANDINGS:
        a = H if L > 0 else -H
        add(0.0, L - a, -a, "branch", f"outer wrap: zinv + dth = {what}")
        add(-a, L - a, 0.0, "branch", f"inner wrap: tin + tj = {what}")
        add(-a, L - a, -0.25, "branch", f"inner wrap: tin + tj = {what}, then an interior outer sum")
    for zeta in (PI, -PI):
        add(0.0, 0.0, zeta, "branch", f"prepare: zeta = {zeta!r} -> zinv = -pi, outer sum -pi stays")
        add(0.0, -ULP, zeta, "branch", f"prepare: zeta = {zeta!r} -> zinv = -pi, outer sum -pi - ulp -> pi - ulp")
        add(0.0, H, zeta, "branch", f"prepare: zeta = {zeta!r} -> zinv = -pi, outer sum -pi/2")
    w32 = wrap(-Z32)                              # 2pi - fl(3/2 pi), exact
    for L, what in LANDINGS[:2]:
        add(0.0, L - w32, Z32, "branch", f"prepare from outside the range: zeta = fl(3/2 pi), outer sum {what}")
    for ti in (PI, -PI):
        add(ti, 0.5, 0.0, "branch", f"theta_i = {ti!r} -> tin = -pi")
        add(ti, -PI, 0.0, "branch", f"theta_i = {ti!r}: -pi + -pi -> 0 (the double wrap)")
        add(ti, -H, H, "branch", f"theta_i = {ti!r}: tin + tj = -3/2 pi wraps to pi/2, outer sum 0")
    for t, what in ((3.0 * PI, "3pi"), (-3.0 * PI, "-3pi"), (TWO_PI + 0.5, "2pi + 0.5"), (-7.0, "-7")):
        add(0.0, t, 0.0, "range", f"theta_j = {what}")
        add(t, 0.25, 0.0, "range", f"theta_i = {what}")
        add(0.0, 0.25, t, "range", f"zeta = {what}")
    add(0.0, 1e6, 0.0, "part", "theta_j = 1e6 (m = 159154)")
    add(1e6, 0.25, 0.0, "part", "theta_i = 1e6")
    add(0.0, 0.25, 1e6, "part", "zeta = 1e6")
    add(0.0, -1e6, 0.0, "part", "theta_j = -1e6")
    # fp64 pi ends in three zero bits, so m 2pi is exact for every |m| <= 10 and the forms agree there (7pi: m = 3); at m = 11
    # (SIDE[0]), 17, 19 they part
    for n in (0, 1, 3):
        add(0.0, _step(7.0 * PI, n), 0.0, "range", f"theta_j = fl(7pi) + {n} ulp (m = 3: the product is still exact)")
    for n in (1, 2):
        add(0.0, _step(-7.0 * PI, -n), 0.0, "range", f"theta_j = fl(-7pi) - {n} ulp (m = -4)")
    for n in (-1, 0, 1, 3):
        add(0.0, _step(35.0 * PI, n), 0.0, "part", f"theta_j = fl(35pi) {n:+d} ulp (m = 17)")
    for n in (-2, 0, 1):
        add(0.0, _step(-37.0 * PI, n), 0.0, "part", f"theta_j = fl(-37pi) {n:+d} ulp (m = -19)")
    for t in SIDE:
        add(0.0, t, 0.0, "side", f"theta_j = {t.hex()}: the fused form lands across the branch")
    add(-SIDE[0], 0.25, 0.0, "side", "theta_i = -fl(23pi): tin across the branch")
    add(0.0, 0.25, -SIDE[1], "side", "zeta = fl(25pi): zinv across the branch")
    # the inner wrap keeps 2^-60 that the unwrapped sum 2pi - 2 ulp + 2^-60 rounds away; prepare's wrap keeps 3 2^-40 beside 1e6
    add(-(PI - ULP), PI - ULP, -(2.0 ** -60), "small", "tin + tj = 2pi - 2 ulp -> -2 ulp, zinv = 2^-60")
    add(0.0, 3.0 * 2.0 ** -40, 1e6, "small", "zinv = wrap(-1e6) beside dth = 3 2^-40")
    add(0.0, 3.0, -3.0, "small", "outer sum 6 -> 6 - 2pi")
    for ti, tj, zeta in ((0.25, 1.0, 0.5), (-2.0, 2.5, 1.0), (1.0, -1.0, -0.75), (0.0, 0.5, 0.0), (3.0, -3.0, 0.125), (-0.5, 0.0, 2.0)):
        add(ti, tj, zeta, "interior", "control")
    return tuple(P)


POINTS = _points()


def _exact_sum(a, b):
    s = a + b
    return s if _is(Fraction(a) + Fraction(b), s) else None


_CANDS = (H, -H, 0.25 * PI, -0.25 * PI, 3.0, -3.0, 1.0, -1.0, 0.5, 0.0, 0.75 * PI, -0.75 * PI)


def _update(orient, L, kind, why):
    """An update cell whose free pose lands on L = theta_v + dx_theta, every sum on the way exact and every wrap's argument but
    the last in range: dx_theta = -e (orientation 0) or +e (orientation 1), e = zinv + (-theta_i + theta_j)."""
    for tv in _CANDS:
        e = _exact_sum(tv, -L) if orient == 0 else _exact_sum(L, -tv)
        if e is None or not (-PI <= e < PI) or e == 0.0:
            continue
        if _exact_sum(tv, -e if orient == 0 else e) != L:
            continue
        for tc in _CANDS:
            ti, tj = (tc, tv) if orient == 0 else (tv, tc)
            if not (-PI <= -ti < PI):
                continue
            dth = _exact_sum(-ti, tj)
            if dth is None or not (-PI <= dth < PI):
                continue
            zinv = _exact_sum(e, -dth)
            if zinv is None or not (-PI <= zinv < PI) or _exact_sum(zinv, dth) != e:
                continue
            return Update(orient, tc, tv, -zinv, L, kind, why)
    raise AssertionError(("no exact update cell", orient, L))


def _updates():
    Us = []
    for o in (0, 1):
        for L, what in LANDINGS + ((6.0, "6 -> 6 - 2pi"), (-6.0, "-6 -> 2pi - 6")):
            Us.append(_update(o, L, "exact", "theta + dx = " + what))
        for L, what in LANDINGS:
            for s in (2.0 ** -30, -(2.0 ** -30)):
                Us.append(_update(o, L + s, "shifted", f"theta + dx = ({what}) {'+' if s > 0 else '-'} 2^-30"))
        for L in (0.75, -1.5, 2.0):
            Us.append(_update(o, L, "interior", f"theta + dx = {L}"))
    return tuple(Us)


UPDATES = _updates()


# ------------------------------------------------------------------ the cell graph
Cells = collections.namedtuple("Cells", "poses fixed ei ej meas info phi ti tj zeta orient kind point update free c")


OMEGA_ANCHOR = (4.0, 0.5, 0.25, 9.0, 0.75, 16.0)     # test_gpu_kat.OMEGA's upper triangle


def cells(points=POINTS, updates=UPDATES, coupled=False, orients=(0, 1), anchored=False):
    """The cell graph -> Cells: set_graph's seven arrays; per cell its edge's theta_i, theta_j, zeta, its orientation, its kind, the
    index of its point or of its update (-1: none), the free pose's id and the fixed one's.  Cell k has the poses 2k (fixed) and
    2k + 1 (free) and the edge k.  anchored: n more edges behind those, edge n + k from cell k's fixed pose to its free one with
    measurement 0 and information OMEGA_ANCHOR -- a second edge at every free pose, so that no edge is a bridge and the cell's own edge
    can be gated, left out or switched off."""
    cl = [(p.ti, p.tj, p.zeta, o, p.kind, t, -1) for o in orients for t, p in enumerate(points)]
    cl += [((u.tc, u.tv) if u.orient == 0 else (u.tv, u.tc)) + (u.zeta, u.orient, "update-" + u.kind, -1, t) for t, u in enumerate(updates)]
    n = len(cl)
    poses, fixed = np.zeros((2 * n, 3)), np.zeros(2 * n, dtype=np.uint8)
    ei, ej = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    meas, info, phi = np.zeros((n, 3)), np.zeros((n, 6)), np.full(n, -1.0)
    for k, (ti, tj, zeta, o, _, _, _) in enumerate(cl):
        c, v = 2 * k, 2 * k + 1
        fixed[c] = 1
        ei[k], ej[k] = (c, v) if o == 0 else (v, c)
        poses[ei[k], 2], poses[ej[k], 2] = ti, tj
        meas[k] = (MEAS_COUPLED if coupled else (0.0, 0.0)) + (zeta,)
        info[k] = INFO_COUPLED if coupled else INFO_ID
    if anchored:
        ei, ej = np.r_[ei, np.arange(0, 2 * n, 2)].astype(np.int32), np.r_[ej, np.arange(1, 2 * n, 2)].astype(np.int32)
        meas, info, phi = np.r_[meas, np.zeros((n, 3))], np.r_[info, np.tile(OMEGA_ANCHOR, (n, 1))], np.full(2 * n, -1.0)
    col = lambda q, dt=np.float64: np.array([r[q] for r in cl], dtype=dt)
    return Cells(poses, fixed, ei, ej, meas, info, phi, col(0), col(1), col(2), col(3, np.int64), np.array([r[4] for r in cl]),
                 col(5, np.int64), col(6, np.int64), np.arange(1, 2 * n, 2), np.arange(0, 2 * n, 2))


def closed_form(C, w=wrap):
    """Per cell, in fp64 with the wrap `w`: e_theta, b_theta = -+e_theta, and the free pose's angle after one Gauss-Newton step,
    w(fl(theta_v + b_theta)) -> (e, b, theta_new, dx)"""
    n = C.ti.size
    e = np.array([route(C.ti[k], C.tj[k], C.zeta[k], w)["e"] for k in range(n)])
    b = np.where(C.orient == 0, -e, e)
    tv = C.poses[C.free, 2]
    new = np.array([w(float(tv[k]) + float(b[k])) for k in range(n)])
    return e, b, new, b.copy()


def same(a, b):
    """"Bit for bit" as these tests mean it, elementwise: the same uint64 pattern, or both a zero of either sign (-0.0 and 0.0 are
    one angle and one gradient, and the sum that assembles b may give either); a NaN is never the same."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) & ~np.isnan(a) | ((a == 0.0) & (b == 0.0))
