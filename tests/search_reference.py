"""The pair quantities of sgo_closure_search in numpy: for a query pose c and a listed pose j at the poses
P, with Sigma = H^-1 of tests/marginals_reference.py's robustified Hessian (SuperLU blocks),

  rel      (t, phi): c in j's frame, t = R(theta_j)^T (p_c - p_j), phi = normalize(theta_c - theta_j)
  A, B     the Jacobians of rel with respect to the two poses: np_oracle.edge_jacobians for the edge j -> c at the ZERO measurement
           (Rz = I, the kernel's sz = 0 and cz = 1), so cov_rel is the covariance of rel in j's frame
  cov_rel  P = 1/2 (Q + Q^T), Q = A Sjj A^T + A Sjc B^T + B Sjc^T A^T + B Scc B^T; a fixed endpoint drops out
  m2       max(0, |t| - radius)^2 / (u^T P_tt u), u = t / |t|: 0 for a zero excess, +inf for a positive excess over a zero denominator
  sigma    (sqrt(lambda_max(P_tt)), sqrt(P_phiphi))
  near     m2 <= chi2_max and j != c and |j - c| >= min_sep; j == c: zeros and near = 0

The bars of the tests (derived in the issue that introduced the call; eps = 2^-52):
  scale = (|A|_max sqrt(max |Sjj|) + |B|_max sqrt(max |Scc|))^2 bounds every term of Q (Cauchy-Schwarz on the cross blocks)
  RULE_BAR = 1e-13: the rule against numpy on identical inputs, |P - P_np|_max <= RULE_BAR scale (36 products of three factors per
             entry, sum |terms| <= 9 scale, gamma_12 = 2.7e-15 -> 2.4e-14 scale: a 4x margin); the same relative bar on rel; m2 and
             sigma through u^T P u: relative error 2 RULE_BAR scale / (u^T P u)
  device against this reference: |P - P_ref|_max <= 9 DEVICE_BAR scale (selinv_reference.DEVICE_BAR on each Sigma block through the four
             products), rel at 1e-12; a decision counts where |m2_ref / chi2_max - 1| > 18 DEVICE_BAR scale / (u^T P_ref u)."""
import numpy as np
import scipy.sparse.linalg as spla

import marginals_reference as mr
from oracle import np_oracle as npo
from selinv_reference import DEVICE_BAR

RULE_BAR = 1e-13
REL_BAR = 1e-12


def jacobians(xj, xc):
    """A = d rel / d x_j, B = d rel / d x_c (3, 3): the edge j -> c at the zero measurement"""
    A, B = npo.edge_jacobians(np.asarray(xj, dtype=np.float64)[None], np.asarray(xc, dtype=np.float64)[None], np.zeros((1, 3)))
    return A[0], B[0]


def pair(xj, xc, Sjj, Sjc, Scc, radius):
    """-> dict(rel, P, m2, sigma, scale, den): den = u^T P_tt u (NaN where |t| = 0).  Sjj / Scc None: that pose is fixed."""
    xj, xc = np.asarray(xj, dtype=np.float64), np.asarray(xc, dtype=np.float64)
    c, s = np.cos(xj[2]), np.sin(xj[2])
    d = xc[:2] - xj[:2]
    t = np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]])
    rel = np.array([t[0], t[1], float(npo.normalize_theta(xc[2] - xj[2]))])
    A, B = jacobians(xj, xc)
    Q = np.zeros((3, 3))
    scale = 0.0
    if Sjj is not None:
        Q += A @ Sjj @ A.T
        scale += np.abs(A).max() * np.sqrt(np.abs(Sjj).max())
    if Scc is not None:
        Q += B @ Scc @ B.T
        scale += np.abs(B).max() * np.sqrt(np.abs(Scc).max())
    if Sjj is not None and Scc is not None:
        Q += A @ Sjc @ B.T + B @ Sjc.T @ A.T
    P = 0.5 * (Q + Q.T)
    norm = float(np.hypot(t[0], t[1]))
    excess = max(0.0, norm - radius)
    den = float("nan")
    if norm > 0.0:
        u = t / norm
        den = float(u @ P[:2, :2] @ u)
    if excess == 0.0:
        m2 = 0.0
    elif den > 0.0:
        m2 = excess * excess / den
    else:
        m2 = float("inf")
    lam = float(np.linalg.eigvalsh(P[:2, :2])[-1])
    sigma = np.array([np.sqrt(max(lam, 0.0)), np.sqrt(max(P[2, 2], 0.0))])
    return dict(rel=rel, P=P, m2=m2, sigma=sigma, scale=scale * scale, den=den)


class Reference:
    """Sigma's blocks at the poses P from SuperLU solves of the robustified Hessian (kind / delta: sgo_set_robust_kernels' arrays,
    None: what phi says), and the pair quantities of a search."""

    def __init__(self, P, fixed, ei, ej, meas, info, phi, kind=None, delta=None):
        self.P = np.asarray(P, dtype=np.float64)
        self.fixed = np.asarray(fixed, dtype=bool)
        self.active = np.zeros(self.P.shape[0], dtype=bool)
        self.active[np.asarray(ei)] = True
        self.active[np.asarray(ej)] = True
        # a vertex without an edge has no row in the device's Hessian: it is left out of the reference's too
        self.held = self.fixed | ~self.active
        self.hidx, self.free = npo.hessian_index(self.held)
        self.H = mr.hessian(self.P, self.held, np.asarray(ei), np.asarray(ej), meas, info, phi, kind, delta).tocsc()
        self.lu = (spla.splu(self.H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
                   if self.free.size else None)
        self._cols = {}

    def prefetch(self, vs, chunk=256):
        """the columns of the free vertices among vs, `chunk` vertices per solve (marginals_reference.Reference solves one at a time)"""
        vs = [int(v) for v in np.unique(np.asarray(vs, dtype=np.int64)) if self.hidx[v] >= 0 and int(v) not in self._cols]
        for k0 in range(0, len(vs), chunk):
            part = vs[k0:k0 + chunk]
            E = np.zeros((self.H.shape[0], 3 * len(part)))
            for q, v in enumerate(part):
                E[3 * self.hidx[v]:3 * self.hidx[v] + 3, 3 * q:3 * q + 3] = np.eye(3)
            X = self.lu.solve(E)
            for q, v in enumerate(part):
                self._cols[v] = X[:, 3 * q:3 * q + 3].copy()

    def block(self, i, j):
        """Sigma_ij (rows of i); the zero block where either vertex is held; (S + S^T) / 2 for i == j, as marginals_reference"""
        hi, hj = int(self.hidx[i]), int(self.hidx[j])
        if hi < 0 or hj < 0:
            return np.zeros((3, 3))
        self.prefetch([j])
        S = self._cols[int(j)][3 * hi:3 * hi + 3].copy()
        return 0.5 * (S + S.T) if i == j else S

    def pair(self, j, c, radius):
        fj, fc = not self.held[j], not self.held[c]
        return pair(self.P[j], self.P[c], self.block(j, j) if fj else None, self.block(j, c) if fj and fc else None,
                    self.block(c, c) if fc else None, radius)

    def search(self, query, ids, radius, chi2_max, min_sep=0):
        """-> dict of arrays over (query, id): m2, rel, P, sigma, near, scale, den, norm (= |t|)"""
        query, ids = np.asarray(query, dtype=np.int64), np.asarray(ids, dtype=np.int64)
        nq, n = query.size, ids.size
        self.prefetch(np.r_[query, ids])
        out = dict(m2=np.zeros((nq, n)), rel=np.zeros((nq, n, 3)), P=np.zeros((nq, n, 3, 3)), sigma=np.zeros((nq, n, 2)),
                   near=np.zeros((nq, n), dtype=bool), scale=np.zeros((nq, n)), den=np.full((nq, n), np.nan), norm=np.zeros((nq, n)))
        for a, c in enumerate(query):
            for b, j in enumerate(ids):
                if j == c:
                    continue
                if not self.active[j]:
                    for k in ("m2", "rel", "P", "sigma", "scale", "norm"):
                        out[k][a, b] = np.nan
                    continue
                r = self.pair(j, c, radius)
                for k in ("m2", "rel", "P", "sigma", "scale", "den"):
                    out[k][a, b] = r[k]
                out["norm"][a, b] = np.hypot(r["rel"][0], r["rel"][1])
                out["near"][a, b] = r["m2"] <= chi2_max and abs(int(j) - int(c)) >= min_sep
        return out


def decided(R, radius, chi2_max):
    """The pairs of a reference search whose decision a device within its bar must reproduce: m2_ref further from chi2_max than
    the bar on P can move it, |m2_ref / chi2_max - 1| > 18 DEVICE_BAR scale / (u^T P_ref u); a pose inside the radius (m2 = 0
    whatever P) and a positive excess over P = 0 (+inf) are decided unless |t| sits on the radius itself."""
    m2, den, scale, norm = R["m2"], R["den"], R["scale"], R["norm"]
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.abs(m2 / chi2_max - 1.0) > 18.0 * DEVICE_BAR * scale / den
    off_radius = np.abs(norm - radius) > 1e-9
    return np.where((m2 == 0.0) | np.isinf(m2), off_radius, margin & off_radius)


def boundary_minimum(rel, P, radius, samples=720):
    """The smallest squared Mahalanobis distance from rel's translation to `samples` points of the circle |y| = radius"""
    a = 2.0 * np.pi * np.arange(samples) / samples
    Y = radius * np.stack([np.cos(a), np.sin(a)], axis=1) - rel[:2]
    return float(np.einsum("ni,ij,nj->n", Y, np.linalg.inv(P[:2, :2]), Y).min())
