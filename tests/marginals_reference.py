"""Reference of sgo_marginals / sgo_solve_rhs (include/sgo.h) in numpy and scipy: blocks of H^-1 from SuperLU solves of unit
columns, with H the robustified Gauss-Newton Hessian of oracle.np_oracle.linearize -- information pre-scaled by the kernels'
weights under the identity of tests/robust_reference.py (the robustified system is the unrobustified one with information
w Omega), so every kernel kind and a gated (zero-information) edge are covered.  The rules are sgo_marginals': a pair with a fixed
vertex on either side is the zero block, a block with vi == vj is (S + S^T) / 2, off-diagonal blocks come as solved.

The natural scale of a block (i, j) is sqrt(max |Sigma_ii| max |Sigma_jj|) of the reference: what an entry of a covariance's
off-diagonal block is bounded by (Cauchy-Schwarz), and the size of the diagonal blocks' own entries."""
import numpy as np
import scipy.sparse.linalg as spla

import robust_reference as rr
from oracle import np_oracle as npo


def weights(P, ei, ej, meas, info, phi, kind=None, delta=None):
    """rho1 of every edge at the poses P; kind / delta as sgo_set_robust_kernels takes them (None: what phi says, NONE or DCS)"""
    e2 = npo.chi2(P, ei, ej, meas, info, np.full(ei.size, -1.0))[2]
    if kind is None:
        kind, delta = np.where(phi >= 0, rr.DCS, rr.NONE), np.where(phi >= 0, phi, 1.0)
    return rr.rho_mixed(kind, e2, delta)[1]


def hessian(P, fixed, ei, ej, meas, info, phi, kind=None, delta=None):
    """H (csc, hessian order: free vertices in ascending id) at the poses P"""
    w = weights(P, ei, ej, meas, info, phi, kind, delta)
    return npo.linearize(P, fixed, ei, ej, meas, info * w[:, None], np.full(ei.size, -1.0))[0]


class Reference:
    """Blocks of H^-1 by vertex id.  worst_residual: the largest |H x - e|_inf over the unit columns solved so far."""

    def __init__(self, H, fixed):
        self.H = H.tocsc()
        self.hidx, self.free = npo.hessian_index(fixed)
        self.lu = spla.splu(self.H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        self.worst_residual = 0.0
        self._cols = {}

    def column(self, v):
        """H^-1 [:, 3h .. 3h + 3) of the free vertex v, (3n, 3)"""
        if v not in self._cols:
            h = int(self.hidx[v])
            assert h >= 0
            E = np.zeros((self.H.shape[0], 3))
            E[3 * h:3 * h + 3] = np.eye(3)
            X = self.lu.solve(E)
            self.worst_residual = max(self.worst_residual, float(np.abs(self.H @ X - E).max()))
            X.setflags(write=False)
            self._cols[v] = X
        return self._cols[v]

    def block(self, i, j):
        hi, hj = int(self.hidx[i]), int(self.hidx[j])
        if hi < 0 or hj < 0:
            return np.zeros((3, 3))
        S = self.column(j)[3 * hi:3 * hi + 3].copy()
        return 0.5 * (S + S.T) if i == j else S

    def blocks(self, vi, vj):
        return np.array([self.block(int(i), int(j)) for i, j in zip(vi, vj)]).reshape(-1, 3, 3)

    def scale(self, i, j):
        return float(np.sqrt(np.abs(self.block(i, i)).max() * np.abs(self.block(j, j)).max()))

    def scales(self, vi, vj):
        return np.array([self.scale(int(i), int(j)) for i, j in zip(vi, vj)])


def worst_ratio(cov, ref, vi, vj):
    """max over the pairs of |cov - ref|_max / natural scale; a pair whose reference is the zero block must be exactly zero"""
    want, sc = ref.blocks(vi, vj), ref.scales(vi, vj)
    worst = 0.0
    for t in range(len(sc)):
        d = float(np.abs(cov[t] - want[t]).max())
        if sc[t] == 0.0:
            assert d == 0.0, (t, cov[t])
        else:
            worst = max(worst, d / sc[t])
    return worst
