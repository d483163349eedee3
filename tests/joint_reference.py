"""Reference of sgo_candidate_joint / sgo_joint_subsets / sgo_joint_pairs (include/sgo.h) -- CPU only, test
infrastructure.

joint_table(): the table of n stacked candidates on any X = H^-1 R (hessian order; R, e from fsolve_reference.rhs),
    S = blockdiag(Omega_t^-1) + 1/2 (G + G^T),   G = R^T X   (3 n x 3 n).
subset_d2(): d2 = e_s^T (S_ss)^-1 e_s by an fp64 Cholesky (LAPACK) of the selected rows and columns, candidates ascending;
subset_d2_long(): the same by a Cholesky written out in np.longdouble -- what the fp64 numbers are checked against.
subsets(): the subset list of the tests for k candidates; masks(): index lists -> the [B][k] mask sgo_joint_subsets takes.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla

from oracle import np_oracle as npo

LD = np.longdouble
K = 48                     # candidates per case of tests/mfront_cases.py in the joint tests (fsolve_reference.K = 21 is the small set)
MAX_CANDIDATES = 256       # SGO_JOINT_MAX_CANDIDATES
MAX_SUBSET = 40            # SGO_JOINT_MAX_SUBSET


def joint_table(R, X, e, info, mut=None):
    """S (3 k, 3 k) from X = H^-1 R.  mut: a wrong table the comparison must reject"""
    k = e.shape[0]
    G = np.asarray(R).T @ np.asarray(X)
    if mut == "cross_dropped":
        keep = np.kron(np.eye(k), np.ones((3, 3)))
        G = G * keep
    S = G.copy() if mut == "not_symmetrised" else 0.5 * (G + G.T)
    if mut != "no_omega":
        O = npo.info_full(info)
        for t in range(k):
            S[3 * t:3 * t + 3, 3 * t:3 * t + 3] += np.linalg.inv(O[t])
    return S


def rows_of(mask):
    idx = np.flatnonzero(np.asarray(mask) != 0)
    return (3 * idx[:, None] + np.arange(3)[None, :]).reshape(-1)


def subset_d2(S, e, mask):
    """d2 of the candidates mask selects (ascending), fp64; 0 for the empty subset, NaN where S_ss is not positive definite"""
    r = rows_of(mask)
    if r.size == 0:
        return 0.0
    try:
        L = np.linalg.cholesky(S[np.ix_(r, r)])
    except np.linalg.LinAlgError:
        return float("nan")
    z = sla.solve_triangular(L, np.asarray(e).reshape(-1)[r], lower=True)
    return float(z @ z)


def subset_d2_long(S, e, mask):
    """the same in np.longdouble: right-looking Cholesky of the lower triangle, the right-hand side carried as one more row"""
    r = rows_of(mask)
    m = r.size
    if m == 0:
        return 0.0
    A = np.empty((m + 1, m), dtype=LD)
    A[:m] = np.asarray(S)[np.ix_(r, r)].astype(LD)
    A[m] = np.asarray(e).reshape(-1)[r].astype(LD)
    d2 = LD(0)
    for k in range(m):
        if not A[k, k] > 0:
            return float("nan")
        A[k:, k] /= np.sqrt(A[k, k])
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:m, k])
        d2 += A[m, k] * A[m, k]
    return float(d2)


def subsets(k=K, seed=5):
    """the tests' subsets of k candidates as index lists: the empty one, every singleton, {0, 1} (the candidates with fixed
    endpoints), 5, 6 and 11 candidates (15, 18 and 33 rows: below, across and two past a 16-wide block edge), the first 40 (the cap)
    and three random halves cut to the cap"""
    rng = np.random.default_rng(seed)
    out = [np.zeros(0, dtype=np.int64)] + [np.array([t]) for t in range(k)] + [np.array([0, 1])]
    for size in (5, 6, 11):
        out.append(np.sort(rng.choice(k, size=size, replace=False)))
    out.append(np.arange(min(MAX_SUBSET, k)))
    for _ in range(3):
        out.append(np.flatnonzero(rng.random(k) < 0.5)[:MAX_SUBSET])
    return out


def masks(lists, k):
    M = np.zeros((len(lists), k), dtype=np.uint8)
    for b, idx in enumerate(lists):
        M[b, np.asarray(idx, dtype=np.int64)] = 1
    return M


def all_d2(S, e, M, long=False):
    f = subset_d2_long if long else subset_d2
    return np.array([f(S, e, m) for m in M])


def rel(got, want):
    """worst |got - want| / |want| over the entries (both zero: 0)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    den = np.where(want != 0, np.abs(want), 1.0)
    return float(np.max(np.abs(got - want) / den)) if got.size else 0.0


def table_ratio(S, Sref):
    return float(np.abs(S - Sref).max() / np.abs(Sref).max())
