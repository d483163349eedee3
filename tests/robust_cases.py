"""The robust kernels at their branch points (sparse_gslam_amd/csrc/sgo_device.h: robustify): a table of single-edge points, and a
graph that carries every point through the kernels bit for bit.  TEST INFRASTRUCTURE ONLY.

The table.  A Point is (kind, d, e2, branch, solve, why): `branch` is the side the specification's fp64 predicate takes (True the
quadratic side, None for a smooth kind), declared here by hand and checked against robust_reference.branch in
tests/test_robust_cases.py; `solve` is set where 2^-20 <= e2 <= 2^20, the points that also go through the solver paths.
  piecewise kinds   e2 = 0; the threshold exactly (d = 4, e2 = 16; DCS: phi = e2 = 16); the same e2 with the parameter one ulp down
                    and one ulp up; a point far below and one far above; and the pair d = 1.2697867137638703,
                    e2 = nextafter(d d, inf), at which sqrt(e2) <= d holds and e2 <= d d does not -- Tukey's predicate and Huber's
                    and Saturated's part there
  smooth kinds      e2 / d^2 in {0, 2^-60, 3 2^-40, 2^-30, 2^-10, 1, 2^10, the first value at which fp64 exp(-x) is 0 and the one
                    before it, 1e150} with d in {0.5, 4}.  3 2^-40 is the one value whose Fair a = sqrt(e2) / d is not a power of
                    two: log(1 + a) and log1p(a) part only where 1 + a rounds
  NONE, and DCS with phi = 0 (scale = 0: rho0 = 0 and weight 0 exactly; e2 = 0 is 0 / 0 there, as in g2o, and not a point)

The bound.  |got - ref| <= C_BOUND EPS scale with robust_reference.rho_ld, scale, C_BOUND = 8, EPS = 2^-53: no formula has more than
six roundings after its inputs plus one library call of at most 2 ulp; contraction removes roundings.  MEASURED keeps the worst
ratios a device run printed -- figures to read, never a reason to change C_BOUND.

The cell graph.  One cell per point and orientation: a fixed pose a, a free pose v and a fixed pose c on a line, theta = 0,
coordinates that are multiples of 1/64 below 16 (their differences are exact, and a pose's own last bit stays below 2e-15).  The
anchor a -> v has no kernel, information test_gpu_kat.OMEGA and error (1/8, -1/16, 0); the kerneled edge is c -> v (orientation
0: J = B = I) or v -> c (orientation 1: J = A), with no rotation in its measurement, e = (1, 0, 0) exactly and
information diag(e2, 1, 1): e^T Omega e is the table's e2 bit for bit in any order of evaluation, so no rounding on the device or
on the host moves a point across its threshold.  H is block diagonal; a cell's 3x3 system Omega_a + w J^T Omega J,
b = -(Omega_a e_a + w J^T Omega e) is formed and solved in long double.  The edge list holds every anchor first and then every
kerneled edge, so that the kerneled edges can also be appended to a resident graph of anchors."""
import collections

import numpy as np

import robust_reference as rr

LD = rr.LD
Point = collections.namedtuple("Point", "kind d e2 branch solve why")
OMEGA = np.array([[4.0, 0.5, 0.25], [0.5, 9.0, 0.75], [0.25, 0.75, 16.0]])    # test_gpu_kat.OMEGA (that module needs a GPU to import)
E_ANCHOR = np.array([0.125, -0.0625, 0.0])
D_SPLIT = 1.2697867137638703

# worst ratios to the bounds, as tests/test_gpu_robust_points.py printed them on an MI355X (see that file's docstring)
MEASURED = {
    # per kind: the worst |got - ref| / (C_BOUND EPS scale) over both of a pair's numbers, all 131 points in both orientations
    "k_edge_robust": dict(none=0.0, dcs=0.125, huber=0.0397, pseudo_huber=0.077, cauchy=0.0657, geman_mcclure=0.14, welsch=0.014,
                          fair=0.115, tukey=0.0625, saturated=0.0756),
    "k_chi2": dict(none=0.0, dcs=0.125, huber=3.79e-5, pseudo_huber=0.077, cauchy=0.0657, geman_mcclure=0.0734, welsch=0.014,
                   fair=0.0719, tukey=0.0625, saturated=0.0756),
    # per kind: the worst entry of b and of the diagonal block over its tolerance; the group and the tile kernel give the same figures
    "k_linearize": dict(none=0.0, dcs=0.0926, huber=0.0615, pseudo_huber=0.0921, cauchy=0.113, geman_mcclure=0.125, welsch=0.0859,
                        fair=0.12, tukey=0.0, saturated=0.0),
    "k_ov_lin (edge_robust)": dict(none=0.0, dcs=0.125, huber=0.0397, pseudo_huber=0.077, cauchy=0.0657, geman_mcclure=0.14,
                                   welsch=0.014, fair=0.115, tukey=0.0625, saturated=0.0756),
    # per path: (d_path, the worst pose entry over its tolerance), the 77 points with `solve` in both orientations
    "optimize(1)": dict(direct=(1e-14, 0.0255), mfront=(1e-14, 0.0255), pcg=(1e-14, 0.0255), overlay=(2.65e-6, 0.0117)),
    # optimize_lm(1, 1e-300) on the multifrontal path: the bits of optimize(1), one trial
    "k_mf_edges<LM>": "bit for bit",
    # against loo_reference (ratios to test_gpu_edge_loo.py's bars) and egroup_reference (N of max |N_ref|, d2 relative, pivot
    # absolute; the bar is 1e-6)
    "k_loo_edges": dict(d2=8.68e-10, cov_loo=1.72e-9, redundancy=4.44e-10),
    "egroup": dict(N=3.43e-16, d2=7.49e-15, pivot=3.33e-16),
}


def _welsch_zero():
    """the first x at which fp64 exp(-x) is exactly 0, and its predecessor"""
    lo, hi = 700.0, 800.0
    assert np.exp(-lo) > 0.0 and np.exp(-hi) == 0.0
    while np.nextafter(lo, np.inf) < hi:
        mid = 0.5 * (lo + hi)
        if np.exp(-mid) == 0.0:
            hi = mid
        else:
            lo = mid
    return hi, lo


def _points():
    P = []

    def add(kind, d, e2, branch, why):
        e2 = float(e2)
        assert np.isfinite(e2) and e2 >= 0.0
        P.append(Point(kind, float(d), e2, branch, bool(2.0 ** -20 <= e2 <= 2.0 ** 20), why))

    dn, up = np.nextafter(4.0, 3.0), np.nextafter(4.0, 5.0)
    for kind in (rr.HUBER, rr.TUKEY, rr.SATURATED):
        add(kind, 4.0, 0.0, True, "e2 = 0")
        add(kind, 4.0, 16.0, True, "the threshold exactly")
        add(kind, dn, 16.0, False, "d d one step below e2")
        add(kind, up, 16.0, True, "d d one step above e2")
        add(kind, 4.0, 0.0625, True, "far below")
        add(kind, 4.0, 4096.0, False, "far above")
        # sqrt(e2) <= d holds, e2 <= d d does not
        add(kind, D_SPLIT, np.nextafter(D_SPLIT * D_SPLIT, np.inf), kind == rr.TUKEY, "where sqrt(e2) <= d and e2 <= d d part")
    add(rr.DCS, 16.0, 0.0, True, "e2 = 0")
    add(rr.DCS, 16.0, 16.0, True, "scale = 1 exactly")
    add(rr.DCS, np.nextafter(16.0, 15.0), 16.0, False, "phi one step below e2")
    add(rr.DCS, np.nextafter(16.0, 17.0), 16.0, True, "phi one step above e2")
    add(rr.DCS, 16.0, 0.0625, True, "far below")
    add(rr.DCS, 16.0, 4096.0, False, "far above")
    add(rr.DCS, 0.0, 16.0, False, "phi = 0")
    add(rr.DCS, 0.0, 2.0 ** -10, False, "phi = 0")
    add(rr.NONE, 1.0, 16.0, None, "no kernel")
    add(rr.NONE, 1.0, 2.0 ** -10, None, "no kernel")
    z, zp = _welsch_zero()
    xs = [(0.0, "e2 = 0"), (2.0 ** -60, "small"), (3 * 2.0 ** -40, "small, sqrt not a power of two"), (2.0 ** -30, "small"),
          (2.0 ** -10, "small"), (1.0, "e2 = d d"), (2.0 ** 10, "large"), (zp, "the last x with exp(-x) > 0"),
          (z, "the first x with exp(-x) = 0"), (1e150, "huge")]
    for kind in (rr.PSEUDO_HUBER, rr.CAUCHY, rr.GEMAN_MCCLURE, rr.WELSCH, rr.FAIR):
        for d in (0.5, 4.0):
            for x, why in xs:
                add(kind, d, x * (d * d), None, why)          # (d d is a power of two: e2 / (d d) is x again, exactly)
    return tuple(P)


POINTS = _points()


def arrays(points=POINTS):
    """kind, d, e2 of the points as arrays"""
    return (np.array([p.kind for p in points], dtype=np.int32), np.array([p.d for p in points]), np.array([p.e2 for p in points]))


def reference(points=POINTS):
    """-> rho0, w in long double, and the bounds C_BOUND EPS scale on each, per point"""
    r0, w, b0, b1 = (np.zeros(len(points), dtype=LD) for _ in range(4))
    for t, p in enumerate(points):
        a, b = rr.rho_ld(p.kind, p.e2, p.d)
        s0, s1 = rr.scale(p.kind, p.e2, p.d)
        r0[t], w[t] = a, b
        b0[t], b1[t] = rr.C_BOUND * rr.EPS * LD(float(s0)), rr.C_BOUND * rr.EPS * LD(float(s1))
    return r0, w, b0, b1


def observed_branch(p, w):
    """The side a result's weight shows for a piecewise point: True / False, or None where the two sides' fp64 weights are the same
    number (Huber, DCS and Tukey are continuous at their thresholds).  The weight of a piecewise kind is one product or quotient of
    values no contraction touches, so the nearer of the two sides' weights is the side that was taken; a tie is no side at all."""
    if p.branch is None:
        return None
    w_lo, w_hi = (float(rr.rho_ld(p.kind, p.e2, p.d, lo=np.bool_(s))[1]) for s in (True, False))
    if w_lo == w_hi or not (np.isfinite(w_lo) and np.isfinite(w_hi)):
        return None
    a, b = abs(w - w_lo), abs(w - w_hi)
    return "neither" if a == b else bool(a < b)


def check(points, rho0, w, name=""):
    """A device's (or any statement's) per-point pairs against the reference -> (failures, worst ratio to the bound per kind):
    the bound on both, the declared side, and the exact values the quadratic and the cut-off sides promise."""
    r0, rw, b0, b1 = reference(points)
    bad, worst = [], {}
    for t, p in enumerate(points):
        g0, g1 = LD(float(rho0[t])), LD(float(w[t]))
        q0 = float(abs(g0 - r0[t]) / b0[t]) if b0[t] > 0 else (0.0 if g0 == r0[t] else np.inf)
        q1 = float(abs(g1 - rw[t]) / b1[t])
        worst[p.kind] = max(worst.get(p.kind, 0.0), q0, q1)
        why = []
        if not (q0 <= 1.0 and q1 <= 1.0):          # (a NaN fails too)
            why.append(f"ratios {q0:.3g} {q1:.3g}")
        if p.branch is not None:
            side = observed_branch(p, float(w[t]))
            if side is not None and side != p.branch:
                why.append(f"side {side}, declared {p.branch}")
            if p.branch and p.kind in (rr.DCS, rr.HUBER, rr.SATURATED) and not (w[t] == 1.0 and rho0[t] == p.e2):
                why.append("the quadratic side is (e2, 1) exactly")
            if not p.branch and p.kind in (rr.TUKEY, rr.SATURATED) and not w[t] == 0.0:
                why.append("the cut-off side has weight 0 exactly")
        if why:
            bad.append((name, t, rr.NAMES[p.kind], p.d, p.e2, p.why, float(rho0[t]), float(w[t]), "; ".join(why)))
    return bad, {rr.NAMES[k]: v for k, v in worst.items()}


# ------------------------------------------------------------------ the cell graph
Cells = collections.namedtuple("Cells", "poses fixed ei ej meas info phi kind delta point orient free kedge n_anchor")


def _jac(orient):
    """the kerneled edge's Jacobian over the free pose: B = I (c -> v), A at theta = 0, dx = 3, dy = 0 (v -> c)"""
    return np.eye(3) if orient == 0 else np.array([[-1.0, 0.0, 0.0], [0.0, -1.0, -3.0], [0.0, 0.0, -1.0]])


def cells(points=POINTS, orients=(0, 1), kerneled=True):
    """The cell graph of `points` -> Cells: set_graph's seven arrays (phi carries NONE and DCS: -1 and d), kind and delta per edge
    for set_robust_kernels, and per cell its point, orientation, free pose id and kerneled edge id.  kerneled=False: every kerneled
    edge has kind NONE (the same systems without a kernel)."""
    cl = [(t, o) for o in orients for t in range(len(points))]
    n = len(cl)
    poses, fixed = np.zeros((3 * n, 3)), np.ones(3 * n, dtype=np.uint8)
    ei, ej = np.zeros(2 * n, dtype=np.int32), np.zeros(2 * n, dtype=np.int32)
    meas, info, phi = np.zeros((2 * n, 3)), np.zeros((2 * n, 6)), np.full(2 * n, -1.0)
    kind, delta = np.zeros(2 * n, dtype=np.int32), np.ones(2 * n)
    for k, (t, o) in enumerate(cl):
        p = points[t]
        a, v, c = 3 * k, 3 * k + 1, 3 * k + 2
        poses[a, 0], poses[v, 0], poses[c, 0] = k / 64.0, k / 64.0 + 1.0, k / 64.0 + 4.0
        fixed[v] = 0
        ei[k], ej[k], meas[k], info[k] = a, v, (1.0 - E_ANCHOR[0], -E_ANCHOR[1], 0.0), OMEGA[np.triu_indices(3)]
        q = n + k
        ei[q], ej[q] = (c, v) if o == 0 else (v, c)
        meas[q] = (-4.0, 0.0, 0.0) if o == 0 else (2.0, 0.0, 0.0)             # e = (dx, 0, 0) - meas = (1, 0, 0)
        info[q] = (p.e2, 0.0, 0.0, 1.0, 0.0, 1.0)
        if kerneled:
            kind[q], delta[q] = p.kind, p.d
            phi[q] = p.d if p.kind == rr.DCS else -1.0
    return Cells(poses, fixed, ei, ej, meas, info, phi, kind, delta, np.array([t for t, _ in cl]), np.array([o for _, o in cl]),
                 np.arange(1, 3 * n, 3), np.arange(n, 2 * n), n)


def cell_systems(C, points, w):
    """Per cell, in long double, from the weights w (per point): H, b, their entrywise magnitudes Ha, ba (the sums of the absolute
    values of the terms that make them) and the weight's carriers Hw = |J|^T Omega |J|, bw = |J|^T Omega |e| (what a unit change of
    w moves)."""
    n = C.point.size
    H, b, Ha, ba, Hw, bw = (np.zeros(s, dtype=LD) for s in ((n, 3, 3), (n, 3), (n, 3, 3), (n, 3), (n, 3, 3), (n, 3)))
    Oa, ea, e = OMEGA.astype(LD), E_ANCHOR.astype(LD), np.array([1.0, 0.0, 0.0], dtype=LD)
    for k in range(n):
        p = points[C.point[k]]
        J = _jac(C.orient[k]).astype(LD)
        O = np.diag(np.array([p.e2, 1.0, 1.0], dtype=LD))
        wk = LD(w[C.point[k]])
        Hw[k], bw[k] = np.abs(J).T @ O @ np.abs(J), np.abs(J).T @ (O @ e)
        H[k], b[k] = Oa + wk * (J.T @ O @ J), -(Oa @ ea + wk * (J.T @ (O @ e)))
        Ha[k], ba[k] = np.abs(Oa) + wk * Hw[k], np.abs(Oa) @ np.abs(ea) + wk * bw[k]
    return H, b, Ha, ba, Hw, bw


def solve3_ld(H, b):
    """H^-1 b and H^-1 of one symmetric positive definite 3x3 system by Cholesky in long double"""
    L = np.zeros((3, 3), dtype=LD)
    for j in range(3):
        L[j, j] = np.sqrt(H[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, 3):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    Li = np.zeros((3, 3), dtype=LD)
    for c in range(3):
        for i in range(3):
            Li[i, c] = ((LD(1) if i == c else LD(0)) - L[i, :i] @ Li[:i, c]) / L[i, i]
    Hi = Li.T @ Li
    return Hi @ b, Hi


def cell_steps(C, points, w):
    """One Gauss-Newton step per cell in long double -> (the step dx (n, 3), what the weight's bound C_BOUND EPS moves of it per
    entry: |H^-1| (bw + Hw |dx|) C_BOUND EPS)"""
    H, b, _, _, Hw, bw = cell_systems(C, points, w)
    n = C.point.size
    dx, dw = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    for k in range(n):
        dx[k], Hi = solve3_ld(H[k], b[k])
        dw[k] = rr.C_BOUND * rr.EPS * (np.abs(Hi) @ (bw[k] + Hw[k] @ np.abs(dx[k])))
    return dx, dw
