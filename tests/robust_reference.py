"""The robust kernels of sgo_set_robust_kernels in numpy (include/sgo.h lists the pairs; kinds in SGO_KERNEL_* numbering), and the
identity the GPU tests lean on: with w = rho1(e2) the robustified Gauss-Newton system is the unrobustified one with information
w Omega, so the CPU oracle -- which knows DCS only -- serves as the reference of every kind:

    c_oracle.linearize(P, ..., info * w[:, None], phi = -1)   b and the diagonal blocks
    sum rho0                                                  the robust chi2
    c_oracle.gauss_newton(..., iters=1) per iteration         the iterates

e = e^T Omega e, d = delta, s = sqrt(e)."""
import numpy as np

NONE, DCS, HUBER, PSEUDO_HUBER, CAUCHY, GEMAN_MCCLURE, WELSCH, FAIR, TUKEY, SATURATED = range(10)
NAMES = ("none", "dcs", "huber", "pseudo_huber", "cauchy", "geman_mcclure", "welsch", "fair", "tukey", "saturated")
PIECEWISE = (DCS, HUBER, TUKEY, SATURATED)


# wrong statements of the pairs that tests/test_robust_cases.py must tell from the right ones on tests/robust_cases.py's table
MUTATIONS = ("dcs_lt", "huber_lt", "tukey_lt", "saturated_lt", "tukey_e2", "saturated_d", "fair_log", "cauchy_w_squared", "geman_d2")


def branch(kind, e, d, mutation=None):
    """The branch predicate of a piecewise kind in fp64, as the specification states it (True: the quadratic side, DCS: scale >= 1);
    None for the smooth kinds."""
    e = np.asarray(e, dtype=np.float64)
    d = np.broadcast_to(np.asarray(d, dtype=np.float64), e.shape)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == DCS:
            scale = (2.0 * d) / (d + e)
            return scale > 1.0 if mutation == "dcs_lt" else scale >= 1.0
        if kind == HUBER:
            return e < d * d if mutation == "huber_lt" else e <= d * d
        if kind == TUKEY:
            if mutation == "tukey_e2":
                return e <= d * d
            return np.sqrt(e) < d if mutation == "tukey_lt" else np.sqrt(e) <= d
        if kind == SATURATED:
            t = d if mutation == "saturated_d" else d * d
            return e < t if mutation == "saturated_lt" else e <= t
    return None


def rho(kind, e, d, mutation=None):
    """(rho0, rho1) of one kind for arrays e (>= 0) and d (> 0; >= 0 for DCS; ignored by NONE).  `mutation`: one of MUTATIONS."""
    e = np.asarray(e, dtype=np.float64)
    d = np.broadcast_to(np.asarray(d, dtype=np.float64), e.shape)
    one = np.ones_like(e)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d2, s = d * d, np.sqrt(e)
        lo = branch(kind, e, d, mutation)
        if kind == NONE:
            return e.copy(), one
        if kind == DCS:
            scale = (2.0 * d) / (d + e)
            return np.where(lo, e, scale * e * scale), np.where(lo, 1.0, scale * scale)
        if kind == HUBER:
            return np.where(lo, e, 2.0 * s * d - d2), np.where(lo, 1.0, d / s)
        if kind == PSEUDO_HUBER:
            a = np.sqrt(1.0 + e / d2)
            return 2.0 * d2 * (a - 1.0), 1.0 / a
        if kind == CAUCHY:
            a = 1.0 + e / d2
            return d2 * np.log(a), (1.0 / a) * (1.0 / a) if mutation == "cauchy_w_squared" else 1.0 / a
        if kind == GEMAN_MCCLURE:
            if mutation == "geman_d2":
                a = d2 / (d2 + e)
                return e * a, a * a
            a = 1.0 / (1.0 + e)
            return e * a, a * a
        if kind == WELSCH:
            a = np.exp(-e / d2)
            return d2 * (1.0 - a), a
        if kind == FAIR:
            a = s / d
            return 2.0 * d2 * (a - (np.log(1.0 + a) if mutation == "fair_log" else np.log1p(a))), 1.0 / (1.0 + a)
        if kind == TUKEY:
            u = 1.0 - e / d2
            return np.where(lo, d2 * (1.0 - u * u * u) / 3.0, d2 / 3.0), np.where(lo, u * u, 0.0)
        if kind == SATURATED:
            t = d if mutation == "saturated_d" else d2
            return np.where(lo, e, t), np.where(lo, 1.0, 0.0)
    raise ValueError(kind)


# ------------------------------------------------------------------ one edge's pair in long double, and the bound it is held to
LD = np.longdouble
EPS, C_BOUND = 2.0 ** -53, 8.0


def rho_ld(kind, e, d, lo=None):
    """(rho0, rho1) by the same formulas in np.longdouble on the fp64 inputs.  The branch predicates are part of the specification
    and are evaluated in fp64 (branch()); `lo` forces a side instead (the tests use it to ask what the other side would give)."""
    assert np.finfo(LD).eps < 2e-19
    e64 = np.asarray(e, dtype=np.float64)
    d64 = np.broadcast_to(np.asarray(d, dtype=np.float64), e64.shape)
    if lo is None:
        lo = branch(kind, e64, d64)
    e, d = e64.astype(LD), d64.astype(LD)
    one, two, three = LD(1), LD(2), LD(3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        d2, s = d * d, np.sqrt(e)
        if kind == NONE:
            return e.copy(), np.ones_like(e)
        if kind == DCS:
            scale = (two * d) / (d + e)
            return np.where(lo, e, scale * e * scale), np.where(lo, one, scale * scale)
        if kind == HUBER:
            return np.where(lo, e, two * s * d - d2), np.where(lo, one, d / s)
        if kind == PSEUDO_HUBER:
            a = np.sqrt(one + e / d2)
            return two * d2 * (a - one), one / a
        if kind == CAUCHY:
            a = one + e / d2
            return d2 * np.log(a), one / a
        if kind == GEMAN_MCCLURE:
            a = one / (one + e)
            return e * a, a * a
        if kind == WELSCH:
            a = np.exp(-e / d2)
            return d2 * (one - a), a
        if kind == FAIR:
            a = s / d
            return two * d2 * (a - np.log1p(a)), one / (one + a)
        if kind == TUKEY:
            u = one - e / d2
            return np.where(lo, d2 * (one - u * u * u) / three, d2 / three), np.where(lo, u * u, LD(0))
        if kind == SATURATED:
            return np.where(lo, e, d2), np.where(lo, one, LD(0))
    raise ValueError(kind)


def scale(kind, e, d):
    """(scale of rho0, scale of rho1): the largest magnitude the formula forms, in the result's units, on the way to each -- the
    larger operand of its subtraction where it has one (1 of Welsch's 1 - a and of Tukey's 1 - u^3, a of Pseudo-Huber's a - 1 and of
    Fair's a - log1p a, 2 s d of Huber's), max(1, log a) for Cauchy (a's own rounding moves log a by an absolute eps), the result
    itself where the formula only multiplies and divides -- and 1 for every weight.  A result passes within C_BOUND EPS scale."""
    e = np.asarray(e, dtype=np.float64)
    d = np.broadcast_to(np.asarray(d, dtype=np.float64), e.shape)
    lo = branch(kind, e, d)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d2, s = d * d, np.sqrt(e)
        if kind == NONE:
            s0 = e.copy()
        elif kind == DCS:
            s0 = np.where(lo, e, (2.0 * d) / (d + e) * e)
        elif kind == HUBER:
            s0 = np.where(lo, e, 2.0 * s * d)
        elif kind == PSEUDO_HUBER:
            s0 = 2.0 * d2 * np.sqrt(1.0 + e / d2)
        elif kind == CAUCHY:
            s0 = d2 * np.maximum(1.0, np.log(1.0 + e / d2))
        elif kind == GEMAN_MCCLURE:
            s0 = e / (1.0 + e)
        elif kind == WELSCH:
            s0 = d2.copy()
        elif kind == FAIR:
            s0 = 2.0 * d2 * (s / d)
        elif kind == TUKEY:
            s0 = np.where(lo, d2, d2 / 3.0)
        elif kind == SATURATED:
            s0 = np.where(lo, e, d2)
        else:
            raise ValueError(kind)
    return s0, np.ones_like(e)


def threshold(kind, d):
    """e at which a piecewise kind changes branch (None for the smooth ones): DCS switches at scale = 1, e = d."""
    d = np.asarray(d, dtype=np.float64)
    if kind == DCS:
        return d
    if kind in (HUBER, TUKEY, SATURATED):
        return d * d
    return None


def rho_mixed(kind, e, d):
    """(rho0, rho1) per edge for arrays of kinds."""
    kind = np.asarray(kind)
    e = np.asarray(e, dtype=np.float64)
    d = np.broadcast_to(np.asarray(d, dtype=np.float64), e.shape)
    r0, r1 = np.empty_like(e), np.empty_like(e)
    for k in np.unique(kind):
        m = kind == k
        r0[m], r1[m] = rho(int(k), e[m], np.where(k == NONE, 1.0, d[m]))
    return r0, r1


def branch_report(kind, e, d):
    """For the piecewise kinds among `kind`: {kind: (edges below the threshold, edges above, smallest relative distance to it)}."""
    kind = np.asarray(kind)
    out = {}
    for k in PIECEWISE:
        m = kind == k
        if not m.any():
            continue
        t = np.broadcast_to(threshold(k, np.broadcast_to(d, kind.shape)[m]), e[m].shape)
        out[k] = (int((e[m] <= t).sum()), int((e[m] > t).sum()), float(np.abs(e[m] / t - 1.0).min()))
    return out


def edge_e2(co, P, g):
    """e^T Omega e of every edge at the poses P, from the CPU oracle"""
    return co.edges(P[g.ei], P[g.ej], g.meas, g.info, -1.0)[3]


def linearize(co, P, g, kind, delta):
    """-> b, diag, chi2, robust chi2, rho0, w of the graph with the given kinds, through the oracle's unrobustified system"""
    e2 = edge_e2(co, P, g)
    r0, w = rho_mixed(kind, e2, delta)
    b, diag, c2, _ = co.linearize(P, g.fixed, g.ei, g.ej, g.meas, g.info * w[:, None], np.full(g.E, -1.0))
    return b, diag, float(e2.sum()), float(r0.sum()), r0, w


def gauss_newton(co, P, g, kind, delta, iters):
    """-> poses, dict(chi2, robust_chi2, e2 per iterate): one unrobustified oracle iteration with information w Omega per iteration"""
    P = np.array(P, dtype=np.float64)
    chi2, rchi2, e2s = [], [], []
    none = np.full(g.E, -1.0)
    for it in range(iters + 1):
        e2 = edge_e2(co, P, g)
        r0, w = rho_mixed(kind, e2, delta)
        chi2.append(float(e2.sum()))
        rchi2.append(float(r0.sum()))
        e2s.append(e2)
        if it == iters:
            break
        P, st = co.gauss_newton(P, g.fixed, g.ei, g.ej, g.meas, g.info * w[:, None], none, iters=1)
        assert st["iters_done"] == 1
    return P, dict(chi2=chi2, robust_chi2=rchi2, e2=e2s)
