"""Reference of sgo_marginals_selected (include/sgo.h) -- CPU only, test infrastructure.

model(): the panel recurrence of sgo_selinv.hip in plain fp64 numpy.  Input: the front table of the HOST plan
(capi.mfront_plan_arrays) and H (marginals_reference.hessian, hessian order); the factor is numpy's own Cholesky of H in the
plan's elimination order, cut into the fronts' columns.  Top-down over the tree, per front with own rows o and boundary rows b:
Sigma_bb gathered from the parent's selected inverse, then the own columns in panels J of 16 from the last to the first, with
R = every row of the front after J,
    T = L_RJ L_JJ^-1,   Sigma_RJ = -Sigma_RR T,   Sigma_JJ = L_JJ^-T L_JJ^-1 - T^T Sigma_RJ
(Sigma_RR kept as a lower triangle and read as a full symmetric matrix, as the device does).  It returns every front's selected
inverse as a dense [m, m] lower triangle.  It does not imitate the matrix cores' summation order.

dense_inverse(): the inverse every stored entry is checked against.  Columns of H^-1 from a sparse LU in fp64, then refined in
np.longdouble: R = I - H X is formed in long double (H's entries and X are exact in it), the correction H^-1 R is solved in fp64 and
added in long double, until a correction is below 1e-17 of the largest entry or no longer shrinks.  The error of a refined
column is cond(H) U times the size of the LAST correction, which the function returns and the tests bound; the result is handed out rounded to fp64 (one rounding, 1e-16 of an entry, against bars of 1e-8 and
1e-6 of the natural scale).

Natural scale of an entry in the rows of pose i and the columns of pose j: sqrt(max |Sigma_ii| max |Sigma_jj|)
(marginals_reference.py: Cauchy-Schwarz bounds the off-diagonal block by it).
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from mfront_reference import Front, local_elim
from oracle import np_oracle as npo

PANEL = 16
LD = np.longdouble
MODEL_BAR = 1e-8      # a case whose fp64 model is further than this from the long-double inverse is not an accuracy case on the GPU
DEVICE_BAR = 1e-6     # the project's bar for marginals (tests/test_gpu_marginals.py)
# Cases of tests/mfront_cases.py the fp64 model itself misses MODEL_BAR on: {name: the model's worst ratio}.  Only these three
# are allowed here (tests/test_selinv_reference.py asserts both directions: listed <=> above the bar).
# (For these the long-double refinement itself stalls at corrections of 6e-9, 9e-11 and 4e-10 of the largest entry: cond(H) times
# the long-double roundoff of the residual.)
ILL_CONDITIONED = {"closure_weight_1e10": 1.93e-5, "rows_scaled_1e6": 1.27e-7, "long_thin_chain": 2.80e-7}


def dense_inverse(H, chunk=1024, refine=True):
    """(H^-1 as fp64 [N, N], size of the last long-double correction relative to max |H^-1|); refine=False: the sparse LU's fp64
    columns as they are (the device tests' reference on the cases the refined one has qualified: their bar is 1e-6)"""
    H = sp.csr_matrix(H)
    N = H.shape[0]
    lu = spla.splu(H.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    indptr, indices, data = H.indptr, H.indices, H.data.astype(LD)
    X = np.empty((N, N))
    last = 0.0
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        E = np.zeros((N, c1 - c0))
        E[np.arange(c0, c1), np.arange(c1 - c0)] = 1.0
        Xc = lu.solve(E).astype(LD)
        step = np.inf
        for _ in range(8 if refine else 0):               # (two steps on a well-conditioned H; stops when a correction no longer shrinks)
            R = E.astype(LD)
            for i in range(N):
                a, b = indptr[i], indptr[i + 1]
                R[i] -= data[a:b] @ Xc[indices[a:b]]
            D = lu.solve(R.astype(np.float64))
            now = float(np.abs(D).max())
            if not now < step:
                break
            Xc += D.astype(LD)
            step = now
            if step <= 1e-17 * float(np.abs(Xc).max()):
                break
        last = max(last, step if refine else 0.0)
        X[:, c0:c1] = Xc.astype(np.float64)
    return X, last / float(np.abs(X).max())


class Plan:
    """The front table and the permutation between the hessian order (free vertices by ascending id) and the elimination order."""

    def __init__(self, X, fixed):
        self.X = X
        self.fronts = [Front(r) for r in X["FRONTS"]]
        hidx, _ = npo.hessian_index(np.asarray(fixed, dtype=bool))
        self.elim_vertex = np.asarray(X["ELIM_VERTEX"], dtype=np.int64)
        self.hpos = np.asarray(hidx)[self.elim_vertex].astype(np.int64)      # elimination position -> hessian index
        assert (self.hpos >= 0).all()
        self.perm = (3 * self.hpos[:, None] + np.arange(3)[None, :]).ravel()  # scalar rows: elimination order -> hessian order

    def rows(self, F):
        """global scalar rows (elimination order) of the front's local rows 0 .. m - 1"""
        le = local_elim(self.X, F)
        return (3 * le[:, None] + np.arange(3)[None, :]).ravel()


def model(plan, H, mut=None):
    """[front] -> its selected inverse, dense [m, m], lower triangle (zeros above); np.linalg.LinAlgError when H is not positive definite"""
    Hp = np.asarray(H.todense() if sp.issparse(H) else H)[np.ix_(plan.perm, plan.perm)]
    L = np.linalg.cholesky(Hp)
    S = [None] * len(plan.fronts)
    rows = [plan.rows(F) for F in plan.fronts]
    for f in range(len(plan.fronts) - 1, -1, -1):      # parents have the higher numbers
        F = plan.fronts[f]
        m, s3 = F.m, F.own3
        Sf = np.zeros((m, m))
        if F.parent >= 0:
            pr = rows[F.parent]
            loc = {int(g): i for i, g in enumerate(pr)}
            idx = np.array([loc[int(g)] for g in rows[f][s3:]], dtype=np.int64)
            Sp = S[F.parent]
            full = np.tril(Sp) + np.tril(Sp, -1).T
            Sf[s3:, s3:] = np.tril(full[np.ix_(idx, idx)])
        Lf = L[np.ix_(rows[f], rows[f][:s3])]           # [m, own3]: L11 over L21
        for k0 in range(((s3 - 1) // PANEL) * PANEL if s3 else -1, -1, -PANEL):
            wp = min(PANEL, s3 - k0)
            rb = k0 + wp
            Y = sla.solve_triangular(Lf[k0:rb, k0:rb], np.eye(wp), lower=True)
            T = Lf[rb:, k0:rb] @ Y
            SRR = np.tril(Sf[rb:, rb:]) + np.tril(Sf[rb:, rb:], -1).T
            if mut == "upper_triangle_read_as_stored":
                SRR = Sf[rb:, rb:]
            SRJ = -SRR @ T
            SJJ = Y.T @ Y - T.T @ SRJ
            if mut == "diagonal_term_dropped":
                SJJ = -T.T @ SRJ
            Sf[rb:, k0:rb] = SRJ
            Sf[k0:rb, k0:rb] = np.tril(SJJ)
        S[f] = Sf
    return S


def front_from_arena(arena, F):
    """A front's selected inverse out of SGO_MF_SEL as [row, column], m x m"""
    return arena[F.off:F.off + F.ld * F.m].reshape(F.m, F.ld).T[:F.m]


def worst_ratio(plan, S, Sigma):
    """max over every stored (lower-triangle) entry of every front of |S - Sigma| / natural scale, Sigma = dense H^-1 in hessian
    order; (ratio, (front, row, column)).  Also asserts the strictly upper part of what is handed in is untouched zeros."""
    Sg = Sigma[np.ix_(plan.perm, plan.perm)]
    n = plan.perm.size // 3
    dmax = np.array([np.abs(Sg[3 * p:3 * p + 3, 3 * p:3 * p + 3]).max() for p in range(n)])
    srow = np.sqrt(np.repeat(dmax, 3))
    worst, where = 0.0, None
    for f, F in enumerate(plan.fronts):
        if F.m == 0:
            continue
        r = plan.rows(F)
        want = Sg[np.ix_(r, r)]
        sc = srow[r][:, None] * srow[r][None, :]
        lo = np.tril(np.ones((F.m, F.m), dtype=bool))
        got = np.asarray(S[f])
        if not np.isfinite(got[lo]).all():
            return float("inf"), (f, -1, -1)
        q = np.where(lo, np.abs(got - want) / sc, 0.0)
        k = int(np.argmax(q))
        if q.flat[k] > worst:
            worst, where = float(q.flat[k]), (f, k // F.m, k % F.m)
    return worst, where


def block_ratio(blocks, vi, vj, Sigma, hidx):
    """max |block - Sigma block| / natural scale over the pairs; a pair with a fixed or edgeless vertex must be exactly zero"""
    worst = 0.0
    for t, (i, j) in enumerate(zip(vi, vj)):
        hi, hj = int(hidx[i]), int(hidx[j])
        if hi < 0 or hj < 0:
            assert not np.asarray(blocks[t]).any(), (t, i, j)
            continue
        want = Sigma[3 * hi:3 * hi + 3, 3 * hj:3 * hj + 3]
        sc = np.sqrt(np.abs(Sigma[3 * hi:3 * hi + 3, 3 * hi:3 * hi + 3]).max() * np.abs(Sigma[3 * hj:3 * hj + 3, 3 * hj:3 * hj + 3]).max())
        worst = max(worst, float(np.abs(blocks[t] - want).max() / sc))
    return worst
