"""The leave-one-out statistic of sgo_edge_leave_one_out in numpy, by two routes that share nothing but
the edge arithmetic of oracle.np_oracle:

  formulas   P = J H^-1 J^T from sparse solves H X = J^T of the FULL graph, then the closed forms through Omega = G G^T
             (numpy cholesky) and N = G^T P G = V diag(nu) V^T (numpy eigh);
  explicit   the edge is taken out: H_ = H - J^T (w Omega) J is factorised, b_ = J^T (w Omega) e, Delta = H_^-1 b_,
             e~ = e + J Delta, P_ = J H_^-1 J^T, d2 = e~^T (Omega^-1 + P_)^-1 e~.

b_ is the gradient the removal CAUSES: the right-hand side of the graph without the edge is b + J^T (w Omega) e, and the statistic
is defined at the full graph's stationary point, b = 0 ("the one linear step that removing it causes").  At poses that are merely
close to that point the residual b would enter Delta linearly and has nothing to do with the edge: measured after gauss_newton(20),
with b left in, 2e-7 in d2 on dcs_switches_closures_off (|b| = 4e-7) and 4e-5 on 2500 / 3400 (DCS at phi = 1 keeps Gauss-Newton
from settling); with b_ as above the routes agree to 1e-13 and 3e-12 there.

The weights w are passed in (np_oracle.dcs_rho for DCS, tests/robust_reference.py for the other kinds): with w = rho1(e2) the
robustified system is the plain one with information w Omega."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import np_oracle as npo


class Edges:
    """e, A, B, Omega, e2 of every edge at the poses P, the DCS weights unless given, and the system (H, b) they make."""

    def __init__(self, P, fixed, ei, ej, meas, info, phi=None, w=None):
        self.P = np.asarray(P, dtype=np.float64)
        self.fixed = np.asarray(fixed, dtype=bool)
        self.ei, self.ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
        self.e = npo.edge_error(self.P[self.ei], self.P[self.ej], meas)
        self.A, self.B = npo.edge_jacobians(self.P[self.ei], self.P[self.ej], meas)
        self.O = npo.info_full(info)
        self.e2 = np.einsum("ni,nij,nj->n", self.e, self.O, self.e)
        self.w = npo.dcs_rho(self.e2, phi)[1] if w is None else np.asarray(w, dtype=np.float64)
        self.hidx, free = npo.hessian_index(self.fixed)
        self.n = free.size
        E = self.ei.size
        self.H, self.b, _, _ = npo.linearize(self.P, self.fixed, self.ei, self.ej, meas, np.asarray(info) * self.w[:, None], np.full(E, -1.0))
        self._lu = None

    def lu(self):
        if self._lu is None:
            self._lu = spla.splu(self.H.tocsc())
        return self._lu

    def J(self, k):
        """the edge's Jacobian over the free poses, dense (3, 3 n); a fixed endpoint drops out"""
        J = np.zeros((3, 3 * self.n))
        for v, M in ((self.ei[k], self.A[k]), (self.ej[k], self.B[k])):
            h = self.hidx[v]
            if h >= 0:
                J[:, 3 * h:3 * h + 3] += M
        return J


def closed_forms(O, P, e, w):
    """The statistic from an edge's own quantities -> dict(d2, redundancy, cov_loo, nu, normN).  A zero Omega: 0, 1, P; an
    Omega that is not positive definite: NaN."""
    P = 0.5 * (P + P.T)
    if not O.any():
        return dict(d2=0.0, redundancy=1.0, cov_loo=P, nu=np.zeros(3), normN=0.0, rc=1)
    try:
        G = np.linalg.cholesky(O)
    except np.linalg.LinAlgError:
        return dict(d2=np.nan, redundancy=np.nan, cov_loo=np.full((3, 3), np.nan), nu=np.full(3, np.nan), normN=np.nan, rc=2)
    N = G.T @ P @ G
    nu, V = np.linalg.eigh(0.5 * (N + N.T))
    c = V.T @ (G.T @ e)
    d2 = float(np.sum(c * c / ((1.0 + (1.0 - w) * nu) * (1.0 - w * nu))))
    Y = np.linalg.solve(G.T, V)
    cov = (Y * (nu / (1.0 - w * nu))) @ Y.T
    return dict(d2=d2, redundancy=float(1.0 - w * nu.max()), cov_loo=0.5 * (cov + cov.T), nu=nu, normN=float(np.abs(nu).max()), rc=0)


def by_formulas(S: Edges, edges, chunk=128):
    """-> dict of arrays over `edges`: d2, redundancy (= lambda_min of I - w N), cov_loo, P, normN (= ||N||_2), w, e2"""
    edges = np.asarray(edges, dtype=np.int64)
    out = dict(d2=np.empty(edges.size), redundancy=np.empty(edges.size), cov_loo=np.empty((edges.size, 3, 3)), P=np.zeros((edges.size, 3, 3)),
               normN=np.empty(edges.size), w=S.w[edges], e2=S.e2[edges])
    for t0 in range(0, edges.size, chunk):
        ks = edges[t0:t0 + chunk]
        if S.n > 0:
            Js = [S.J(k) for k in ks]
            X = S.lu().solve(np.concatenate(Js, axis=0).T)          # (3 n, 3 |ks|)
            for q, J in enumerate(Js):
                out["P"][t0 + q] = J @ X[:, 3 * q:3 * q + 3]
        for q, k in enumerate(ks):
            r = closed_forms(S.O[k], out["P"][t0 + q], S.e[k], S.w[k])
            out["P"][t0 + q] = 0.5 * (out["P"][t0 + q] + out["P"][t0 + q].T)
            for name in ("d2", "redundancy", "cov_loo", "normN"):
                out[name][t0 + q] = r[name]
    return out


def by_leaving_out(S: Edges, k):
    """Edge k taken out of the system -> (d2, cov_loo = P_); only for an edge whose removal leaves H_ positive definite"""
    J = S.J(k)
    W = S.w[k] * S.O[k]
    Hm = (S.H - sp.csc_matrix(J.T @ W @ J)).tocsc()
    bm = J.T @ (W @ S.e[k])
    lu = spla.splu(Hm)
    et = S.e[k] + J @ lu.solve(bm)
    Pm = J @ lu.solve(J.T)
    Pm = 0.5 * (Pm + Pm.T)
    return float(et @ np.linalg.solve(np.linalg.inv(S.O[k]) + Pm, et)), Pm


def motivating_graph():
    """The graph the statistic was prototyped on: 300 poses, 360 edges, closure 7 (edge 306) shifted by 0.4 m in x and y, which the
    raw chi2 gate at 11.345 lets through after the fit."""
    from sparse_gslam_amd import synth
    g = synth.manhattan(300, 360, seed=4, info_mode="full", init="incremental", tail=20)
    g.meas = g.meas.copy()
    g.meas[306, :2] += 0.4
    return g, 306
