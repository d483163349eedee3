"""Reference of sgo_factor_solve / sgo_candidate_gate (include/sgo.h) -- CPU only, test infrastructure.

model(): the front-by-front recurrence of sgo_fsolve.hip in plain fp64 numpy on the HOST plan (capi.mfront_plan_arrays) and H
(marginals_reference.hessian, hessian order).  The factor is numpy's own Cholesky of H in the plan's elimination order, cut into the
fronts' columns, with the explicit inverses of the 16 x 16 diagonal blocks' factors.  Forward, bottom-up: a front takes its own rows
of the right-hand sides, adds its children's boundary updates through the extend-add maps (child 0 before child 1), walks its own
columns in blocks J of 16 -- y_J = L_JJ^-1 t_J, t_R -= L_RJ y_J for every row R after J -- and hands its boundary rows up.
Backward, top-down: x_J = L_JJ^-T (y_J - L_RJ^T x_R), the boundary rows of x read from the fronts above.  It returns Y and X by
elimination position.  It does not imitate the matrix cores' summation order.

refined(): the solution every column is checked against -- SuperLU's fp64 columns refined in np.longdouble as
selinv_reference.dense_inverse refines (residual in long double, correction in fp64, added in long double).

candidates() / gate(): the candidate closures of the tests and sgo_candidate_gate's formula on any X = H^-1 R,
    P = 1/2 (Q + Q^T), Q = R^T X;  d2 = e^T (Omega^-1 + P)^-1 e.
backward_error(): sgo_rules.h's Jacobi-scaled backward error (rules::floor_backward_error) per column.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import mfront_cases as mc
from oracle import np_oracle as npo
from sparse_gslam_amd import synth

PANEL = 16
LD = np.longdouble
FLOOR_ETA = 1e-12          # rules::kFloorEta
K = 21                     # candidates per case of tests/mfront_cases.py


def _dense(H):
    return np.asarray(H.todense() if sp.issparse(H) else H)


def model(plan, H, R, mut=None):
    """(Y, X), both [3 n, columns] by elimination position, for the right-hand sides R [3 n, columns] in HESSIAN order"""
    Hp = _dense(H)[np.ix_(plan.perm, plan.perm)]
    L = np.linalg.cholesky(Hp)
    B = np.asarray(R, dtype=np.float64)[plan.perm]
    nf = len(plan.fronts)
    rows = [plan.rows(F) for F in plan.fronts]
    Y, X = np.zeros_like(B), np.zeros_like(B)
    U = [None] * nf
    Lf = [L[np.ix_(rows[f], rows[f][:plan.fronts[f].own3])] for f in range(nf)]
    Yinv = [[sla.solve_triangular(Lf[f][k0:min(k0 + PANEL, F.own3), k0:min(k0 + PANEL, F.own3)], np.eye(min(PANEL, F.own3 - k0)), lower=True)
             for k0 in range(0, F.own3, PANEL)] for f, F in enumerate(plan.fronts)]
    for f, F in enumerate(plan.fronts):                 # children have the lower numbers
        m, s3 = F.m, F.own3
        t = np.zeros((m, B.shape[1]))
        t[:s3] = B[rows[f][:s3]]
        loc = {int(g): i for i, g in enumerate(rows[f])}
        for k, kid in enumerate(F.kid):
            if kid < 0 or (mut == "child_update_dropped" and k == 0):
                continue
            C = plan.fronts[kid]
            idx = np.array([loc[int(g)] for g in rows[kid][C.own3:]], dtype=np.int64)
            t[idx] += U[kid]
        for b, k0 in enumerate(range(0, s3, PANEL)):
            rb = min(k0 + PANEL, s3)
            t[k0:rb] = Yinv[f][b] @ t[k0:rb]
            t[rb:] -= Lf[f][rb:, k0:rb] @ t[k0:rb]
        Y[rows[f][:s3]] = t[:s3]
        U[f] = t[s3:]
    for f in range(nf - 1, -1, -1):
        F = plan.fronts[f]
        m, s3 = F.m, F.own3
        if s3 == 0:
            continue
        x = np.zeros((m, B.shape[1]))
        x[:s3] = Y[rows[f][:s3]]
        x[s3:] = X[rows[f][s3:]]
        for k0 in range(((s3 - 1) // PANEL) * PANEL, -1, -PANEL):
            rb = min(k0 + PANEL, s3)
            lo = s3 if mut == "backward_boundary_dropped" else m
            v = x[k0:rb] - Lf[f][rb:lo, k0:rb].T @ x[rb:lo]
            x[k0:rb] = Yinv[f][k0 // PANEL].T @ v
        X[rows[f][:s3]] = x[:s3]
    return Y, X


def to_hessian_order(plan, Xe):
    out = np.empty_like(Xe)
    out[plan.perm] = Xe
    return out


def refined(H, R, refine=True):
    """(H^-1 R as fp64 [3 n, columns], size of the last long-double correction relative to the largest entry)"""
    H = sp.csr_matrix(H)
    R = np.asarray(R, dtype=np.float64)
    lu = spla.splu(H.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    indptr, indices, data = H.indptr, H.indices, H.data.astype(LD)
    Xc = lu.solve(R).astype(LD)
    step = np.inf
    for _ in range(8 if refine else 0):
        Res = R.astype(LD)
        for i in range(H.shape[0]):
            a, b = indptr[i], indptr[i + 1]
            Res[i] -= data[a:b] @ Xc[indices[a:b]]
        D = lu.solve(Res.astype(np.float64))
        now = float(np.abs(D).max())
        if not now < step:
            break
        Xc += D.astype(LD)
        step = now
        if step <= 1e-17 * float(np.abs(Xc).max()):
            break
    X = Xc.astype(np.float64)
    return X, (step if refine and np.isfinite(step) else 0.0) / max(float(np.abs(X).max()), 1e-300)


def backward_error(H, X, R):
    """rules::floor_backward_error of every column: |S r| / (|S^-1 x| + |S b|), S = diag(H)^-1/2 (|S H S| taken as 1)"""
    H = sp.csr_matrix(H)
    h = H.diagonal()[:, None]
    Res = np.asarray(R) - H @ np.asarray(X)
    den = np.sqrt((np.asarray(X)**2 * h).sum(0)) + np.sqrt((np.asarray(R)**2 / h).sum(0))
    num = np.sqrt((Res**2 / h).sum(0))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


# ------------------------------------------------------------------ candidates and the gate's formula
def candidates(c, k=K, seed=77):
    """(ci, cj, meas (k, 3), info (k, 6)) for a case of tests/mfront_cases.py: endpoints random over ALL vertices (fixed ones
    included), candidate 0 from a fixed vertex to the last free one, a both-fixed candidate where the case has two fixed vertices;
    measurement = the relative pose of the case's poses + N(0, SIG), every fourth shifted by 1 m; Omega = diag(1 / SIG^2)"""
    rng = np.random.default_rng(seed)
    V = c.poses.shape[0]
    ci = rng.integers(0, V, k)
    cj = (ci + 1 + rng.integers(0, V - 1, k)) % V          # never ci itself
    fx, free = np.flatnonzero(c.fixed), np.flatnonzero(~c.fixed)
    ci[0], cj[0] = fx[0], free[-1]
    if fx.size >= 2:
        ci[1], cj[1] = fx[0], fx[1]
    meas = synth._rel(c.poses[ci], c.poses[cj]) + rng.standard_normal((k, 3)) * mc.SIG
    meas[::4, 0] += 1.0
    meas[:, 2] = synth._wrap(meas[:, 2])
    info = np.tile(np.array([1 / mc.SIG[0]**2, 0, 0, 1 / mc.SIG[1]**2, 0, 1 / mc.SIG[2]**2]), (k, 1))
    return ci.astype(np.int32), cj.astype(np.int32), meas, info


def rhs(P, fixed, ci, cj, meas):
    """(R [3 n, 3 k] in hessian order -- A^T at the rows of ci[t], B^T at the rows of cj[t], columns 3 t .. 3 t + 2 --, e (k, 3))"""
    hidx, free = npo.hessian_index(fixed)
    A, B = npo.edge_jacobians(P[ci], P[cj], meas)
    e = npo.edge_error(P[ci], P[cj], meas)
    R = np.zeros((3 * free.size, 3 * len(ci)))
    for t, (i, j) in enumerate(zip(ci, cj)):
        hi, hj = int(hidx[i]), int(hidx[j])
        if hi >= 0:
            R[3 * hi:3 * hi + 3, 3 * t:3 * t + 3] = A[t].T
        if hj >= 0:
            R[3 * hj:3 * hj + 3, 3 * t:3 * t + 3] = B[t].T
    return R, e


def gate(R, X, e, info, mut=None):
    """(P (k, 3, 3), d2 (k,)) from X = H^-1 R (hessian order)"""
    k = e.shape[0]
    O = npo.info_full(info)
    P, d2 = np.empty((k, 3, 3)), np.empty(k)
    for t in range(k):
        Q = R[:, 3 * t:3 * t + 3].T @ X[:, 3 * t:3 * t + 3]
        P[t] = Q if mut == "not_symmetrised" else 0.5 * (Q + Q.T)
        S = np.linalg.inv(O[t]) + P[t]
        d2[t] = e[t] @ np.linalg.solve(S, e[t])
    return P, d2


def gate_ratios(P, d2, Pref, d2ref, info):
    """(worst |P - P_ref|max / max |Omega^-1 + P_ref|, worst |d2 - d2_ref| / d2_ref)"""
    O = npo.info_full(info)
    rp = max(float(np.abs(P[t] - Pref[t]).max() / np.abs(np.linalg.inv(O[t]) + Pref[t]).max()) for t in range(len(d2)))
    rd = float(np.max(np.abs(d2 - d2ref) / d2ref))
    return rp, rd
