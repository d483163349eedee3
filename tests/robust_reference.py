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


def rho(kind, e, d):
    """(rho0, rho1) of one kind for arrays e (>= 0) and d (> 0; >= 0 for DCS; ignored by NONE)."""
    e = np.asarray(e, dtype=np.float64)
    d = np.broadcast_to(np.asarray(d, dtype=np.float64), e.shape)
    one = np.ones_like(e)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d2, s = d * d, np.sqrt(e)
        if kind == NONE:
            return e.copy(), one
        if kind == DCS:
            scale = (2.0 * d) / (d + e)
            sat = scale >= 1.0
            return np.where(sat, e, scale * e * scale), np.where(sat, 1.0, scale * scale)
        if kind == HUBER:
            lo = e <= d2
            return np.where(lo, e, 2.0 * s * d - d2), np.where(lo, 1.0, d / s)
        if kind == PSEUDO_HUBER:
            a = np.sqrt(1.0 + e / d2)
            return 2.0 * d2 * (a - 1.0), 1.0 / a
        if kind == CAUCHY:
            a = 1.0 + e / d2
            return d2 * np.log(a), 1.0 / a
        if kind == GEMAN_MCCLURE:
            a = 1.0 / (1.0 + e)
            return e * a, a * a
        if kind == WELSCH:
            a = np.exp(-e / d2)
            return d2 * (1.0 - a), a
        if kind == FAIR:
            a = s / d
            return 2.0 * d2 * (a - np.log1p(a)), 1.0 / (1.0 + a)
        if kind == TUKEY:
            lo = s <= d
            u = 1.0 - e / d2
            return np.where(lo, d2 * (1.0 - u * u * u) / 3.0, d2 / 3.0), np.where(lo, u * u, 0.0)
        if kind == SATURATED:
            lo = e <= d2
            return np.where(lo, e, d2), np.where(lo, 1.0, 0.0)
    raise ValueError(kind)


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
