"""Reference of sgo_joint_greedy / sgo_joint_extend / sgo_joint_greedy_rule (include/sgo.h) -- CPU only, test
infrastructure.

greedy(): the block-pivoted recurrence in np.longdouble, written plainly (whole matrices, none of the kernel's layout).  After the
ordered pivots t_1 .. t_k every candidate c holds W_c (3 k x 3), C_c = S_cc - W_c^T W_c and q_c = e_c - W_c^T z; the extension value is
v_c = d2 + q_c^T C_c^-1 q_c; the pivot step of p is G = chol(C_p), z+ = G^-1 q_p, w = G^-1 (S_p: - W_p^T W), C_c -= w_c^T w_c,
q_c -= w_c^T z+, d2 += z+^T z+.  At count k the candidates that are not pivots, are allowed and have a finite v_c <= chi[k + 1] are
eligible; the smallest v is chosen, ties to the lowest index.
Every decision's MARGIN comes with it: the relative gap between the best and the second-best eligible v, and the relative distance of
every finite v of a candidate that could be chosen from chi[k + 1].  A seed whose smallest margin is >= MARGIN has a path no fp64
rounding of the arithmetic can change; only those seeds' orders are compared.
mut: a wrong recurrence the comparisons must reject.
ladders(): the two threshold ladders of the tests; lists(): index lists -> the -1 padded rows the calls take.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
from scipy.stats import chi2 as chi2_dist

import joint_reference as jr

LD = np.longdouble
MAX_SUBSET = jr.MAX_SUBSET
MARGIN = 1e-8
STOP_MAX_LEN, STOP_NONE, STOP_NOT_PD = 0, 1, 2
MUTATIONS = ("q_not_updated", "last_w_dropped", "g_transposed", "ties_high")

Path = namedtuple("Path", "order count stop d2_path d2_ext margin")


def chol3(C):
    """lower Cholesky factors of the (k, 3, 3) blocks C in longdouble; NaN rows where a block is not positive definite"""
    C = np.asarray(C, dtype=LD)
    G = np.zeros_like(C)
    with np.errstate(invalid="ignore", divide="ignore"):
        G[:, 0, 0] = np.sqrt(C[:, 0, 0])
        G[:, 1, 0] = C[:, 1, 0] / G[:, 0, 0]
        G[:, 2, 0] = C[:, 2, 0] / G[:, 0, 0]
        t11 = C[:, 1, 1] - G[:, 1, 0] ** 2
        G[:, 1, 1] = np.sqrt(t11)
        G[:, 2, 1] = (C[:, 2, 1] - G[:, 2, 0] * G[:, 1, 0]) / G[:, 1, 1]
        t22 = C[:, 2, 2] - G[:, 2, 0] ** 2 - G[:, 2, 1] ** 2
        G[:, 2, 2] = np.sqrt(t22)
        bad = ~((C[:, 0, 0] > 0) & (t11 > 0) & (t22 > 0) & np.isfinite(G[:, 2, 2]))
    G[bad] = np.nan
    return G


def solve3(G, b):
    """x = G^-1 b for (k, 3, 3) lower factors and (k, 3, r) right-hand sides"""
    x = np.empty_like(b)
    x[:, 0] = b[:, 0] / G[:, 0, 0, None]
    x[:, 1] = (b[:, 1] - G[:, 1, 0, None] * x[:, 0]) / G[:, 1, 1, None]
    x[:, 2] = (b[:, 2] - G[:, 2, 0, None] * x[:, 0] - G[:, 2, 1, None] * x[:, 1]) / G[:, 2, 2, None]
    return x


def values(d2, C, q):
    """v_c = d2 + q_c^T C_c^-1 q_c for every candidate; NaN where C_c is not positive definite"""
    x = solve3(chol3(C), q[:, :, None])[:, :, 0]
    return d2 + (x * x).sum(1)


def greedy(S, e, seed, chi, max_len=MAX_SUBSET, allow=None, mut=None):
    S = np.asarray(S).astype(LD)
    n = S.shape[0] // 3
    ev = np.asarray(e).reshape(n, 3).astype(LD)
    allow = np.ones(n, dtype=bool) if allow is None else np.asarray(allow) != 0
    W = np.zeros((0, 3 * n), dtype=LD)
    C = np.stack([S[3 * c:3 * c + 3, 3 * c:3 * c + 3] for c in range(n)])
    q = ev.copy()
    Cuse = C
    pivot = np.zeros(n, dtype=bool)
    order, path, d2, margin, stop = [], [LD(0)], LD(0), 1.0, STOP_MAX_LEN
    seed = [int(t) for t in seed]
    while len(order) < max_len:
        k = len(order)
        if k < len(seed):
            p = seed[k]
        else:
            if chi is None:
                stop = STOP_NONE
                break
            v = values(d2, Cuse, q)
            could = ~pivot & allow & np.isfinite(v)
            if could.any():
                margin = min(margin, float(np.min(np.abs(v[could] - chi[k + 1]) / chi[k + 1])))
            el = np.flatnonzero(could & (v <= chi[k + 1]))
            if el.size == 0:
                stop = STOP_NONE
                break
            srt = np.sort(v[el])
            if srt.size > 1:
                margin = min(margin, float((srt[1] - srt[0]) / srt[0]))
            best = el[v[el] == srt[0]]
            p = int(best[-1] if mut == "ties_high" else best[0])
        G = chol3(Cuse[p:p + 1])
        if not np.isfinite(G).all():
            stop = STOP_NOT_PD
            break
        R = S[3 * p:3 * p + 3, :] - W[:, 3 * p:3 * p + 3].T @ W
        if mut == "g_transposed":                                      # G^T in G's place (a general solve: the mutation is upper triangular)
            Gi = np.linalg.inv(G[0].T.astype(np.float64)).astype(LD)
            zp, w = Gi @ q[p], Gi @ R
        else:
            zp, w = solve3(G, q[p][None, :, None])[0, :, 0], solve3(G, R[None])[0]
        wc = w.reshape(3, n, 3).transpose(1, 0, 2)                     # (n, 3, 3): candidate c's w
        Cuse = C if mut == "last_w_dropped" else None                  # (the mutation: the values never see the last pivot's w)
        C = C - np.einsum("cra,crb->cab", wc, wc)
        Cuse = C if Cuse is None else Cuse
        if mut != "q_not_updated":
            q = q - np.einsum("cra,r->ca", wc, zp)
        W = np.vstack([W, w])
        pivot[p] = True
        d2 = d2 + zp @ zp
        order.append(p)
        path.append(d2)
    count = len(order)
    if stop == STOP_NOT_PD:
        ext = np.full(n, np.nan)
    else:
        ext = np.where(pivot, d2, values(d2, Cuse, q)).astype(np.float64)
    d2_path = np.full(MAX_SUBSET + 1, np.nan)
    d2_path[:count + 1] = np.array(path, dtype=LD).astype(np.float64)
    out = np.full(MAX_SUBSET, -1, dtype=np.int32)
    out[:count] = order
    return Path(out, count, stop, d2_path, ext, margin)


def ladders(S, e):
    """name -> chi2_max (41,) by count: the 99 % quantile of chi2 with 3 k degrees of freedom, and a tight ladder (the median of the
    singletons' d2 times k) that stops paths midway"""
    n = np.asarray(e).reshape(-1, 3).shape[0]
    single = np.array([jr.subset_d2(S, e, jr.masks([[t]], n)[0]) for t in range(n)])
    k = np.arange(1, MAX_SUBSET + 1)
    return {"q99": np.concatenate([[0.0], chi2_dist.ppf(0.99, 3 * k)]), "tight": np.concatenate([[0.0], np.median(single) * k])}


def lists(rows):
    out = np.full((len(rows), MAX_SUBSET), -1, dtype=np.int32)
    for b, idx in enumerate(rows):
        out[b, :len(idx)] = np.asarray(idx, dtype=np.int32)
    return out


# the cases of the search's tests: name -> (case of tests/mfront_cases.py, candidates); n = 1, 2 and 65 (one past a wave) are the first
# candidates of tree_shapes' list, 256 (the cap, every thread live) needs lattice_48's 2 304 poses
CASES = {"tree_shapes": ("tree_shapes", jr.K), "child_own3_33": ("child_own3_33", jr.K), "n1": ("tree_shapes", 1), "n2": ("tree_shapes", 2),
         "n65": ("tree_shapes", 65), "n256": ("lattice_48", jr.MAX_CANDIDATES)}
_TABLES = {}


def table(name):
    """(case, candidates (ci, cj, meas, info), S, e) of CASES[name] from the long-double-refined columns: computed once and shared,
    never modified"""
    if name not in _TABLES:
        import fsolve_reference as fr
        import marginals_reference as mref
        import mfront_cases as mc
        graph, k = CASES[name]
        c = mc.make(graph)
        H = mref.hessian(c.poses, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
        cand = fr.candidates(c, k)
        R, e = fr.rhs(c.poses, c.fixed, *cand[:3])
        Xr, last = fr.refined(H, R)
        assert last <= 1e-12, last
        S = np.asarray(jr.joint_table(R, Xr, e, cand[3]), dtype=np.float64)
        for a in (S, e):
            a.setflags(write=False)
        _TABLES[name] = (c, cand, S, e)
    return _TABLES[name]


# The one combination whose threshold decision is a tie by construction: the tight ladder is the median of the singletons' d2 times k,
# and the median of ONE number is the number, so at n = 1 the empty seed's only extension value equals chi[1] up to the rounding of two
# routes to the same quantity.  Listed <=> its margin is below MARGIN; every other combination must qualify nine seeds of ten.
DEGENERATE = {("n1", "tight")}


def seeds(n, every=1):
    """the tests' seeds of n candidates: the empty one, every singleton (every `every`-th: the long-double reference of all 256 at the
    cap takes half a minute), then (n permitting) a seed of 39 and one of 40 candidates"""
    rng = np.random.default_rng(9)
    out = [[]] + [[t] for t in range(0, n, every)]
    if n >= 48:
        perm = rng.permutation(n)
        out += [list(perm[:39]), list(perm[:40])]
    return out
