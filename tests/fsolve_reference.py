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

check() / check_gate(): one call's kernels stage by stage from the arrays sgo_debug_mfront_array exports after it (forward, backward,
columns; gate, d2 -- the functions' docstrings have the bounds), in the style of mfront_reference.check: inputs as stored,
references in long double, |got - ref| <= C U abs with no condition of H, so they run on every case, the three ill-conditioned
ones included.  MODEL / C_STAGE / MEASURED below; DESIGN.md section 5g has the table.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import kernel_reference as kr
import mfront_cases as mc
import selinv_reference as sr
from amg_reference import Result, entry_ratio
from mfront_reference import constant, front_matrix, stage_of
from oracle import np_oracle as npo
from overlay_reference import edge_parts_ld
from sparse_gslam_amd import synth

PANEL = 16
LD = np.longdouble
FLOOR_ETA = 1e-12          # rules::kFloorEta
K = 21                     # candidates per case of tests/mfront_cases.py


def _dense(H):
    return np.asarray(H.todense() if sp.issparse(H) else H)


def model(plan, H, R, mut=None, factor=None, mut_front=None):
    """(Y, X), both [3 n, columns] by elimination position, for the right-hand sides R [3 n, columns] in HESSIAN order.
    factor: selinv_reference.host_factor's (ARENA, YINV), made here when not given.  mut: one of the CPU tests' mutations, applied
    at front mut_front where it concerns one front."""
    arena, yinv = sr.host_factor(plan, H) if factor is None else factor
    B = np.asarray(R, dtype=np.float64)[plan.perm]
    nf = len(plan.fronts)
    rows = [plan.rows(F) for F in plan.fronts]
    Y, X = np.zeros_like(B), np.zeros_like(B)
    U = [None] * nf
    Lf = [front_matrix(arena, F)[:F.m, :F.own3] for F in plan.fronts]
    Yinv = [[yinv[3 * F.e0 + k0:3 * F.e0 + min(k0 + PANEL, F.own3), :min(PANEL, F.own3 - k0)] for k0 in range(0, F.own3, PANEL)]
            for F in plan.fronts]
    for f, F in enumerate(plan.fronts):                 # children have the lower numbers
        m, s3 = F.m, F.own3
        here = mut_front is None or mut_front == f
        t = np.zeros((m, B.shape[1]))
        t[:s3] = B[rows[f][:s3]]
        loc = {int(g): i for i, g in enumerate(rows[f])}
        for k, kid in enumerate(F.kid):
            if kid < 0 or (mut == "child_update_dropped" and k == 0 and here):
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
        here = mut_front is None or mut_front == f
        if s3 == 0:
            continue
        x = np.zeros((m, B.shape[1]))
        x[:s3] = Y[rows[f][:s3]]
        x[s3:] = X[rows[f][s3:]]
        for k0 in range(((s3 - 1) // PANEL) * PANEL, -1, -PANEL):
            rb = min(k0 + PANEL, s3)
            lo = s3 if mut == "backward_boundary_dropped" else m
            v = x[k0:rb] - Lf[f][rb:lo, k0:rb].T @ x[rb:lo]
            Yj = Yinv[f][k0 // PANEL]
            x[k0:rb] = (Yj if mut == "backward_inverse_not_transposed" and here else Yj.T) @ v
            if mut == "column_contaminated_by_its_neighbour" and here and B.shape[1] > 1:
                x[k0:rb, 0] += 2.0 ** -40 * x[k0:rb, 1]
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


# ------------------------------------------------------------------ the stage checks (the style of mfront_reference.check)
CHUNK_CANDS = 85           # kFsChunkPanels * kMfPanel / 3 (sgo_mfront_dev.h, sgo_fsolve.cpp): candidates per pass over the factor
STAGES = ("forward", "backward", "columns", "gate", "d2")
# Worst error / (U abs) of model() / gate() over the cases of tests/mfront_cases.py against the long-double expressions of check()
# and check_gate(), and where (tests/test_fsolve_reference.py holds the model to them); C = 4 x that, rounded up to a power of two:
#   stage     model   case                 C
#   forward   4.97    lattice_48           32
#   backward  19.0    lattice_48           128   (numpy sums nR products in a row; abs carries no factor nR)
#   gate      2.34    root_own3_6          16    (P)
#   d2        0.0261  solve_fast_144       0.125 (of a bound that carries kappa of the 3 x 3 block)
MODEL = dict(forward=4.97, backward=19.0, gate=2.34, d2=0.0261)
C_STAGE = {k: constant(v) for k, v in MODEL.items()}
# Worst error / (U abs) measured on the MI355X over tests/test_gpu_fsolve_reference.py, and where
MEASURED = dict(forward=(6.278, "lattice_48"), backward=(6.135, "lattice_50"), gate=(2.741, "root_own3_6"), d2=(0.0224, "root_own3_6"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def scaled(R):
    """{check: ratio / C_stage}: a value above 1 fails (exact checks: 0 or inf)."""
    return {k: (v if stage_of(k) not in C_STAGE or v in (0.0, float("inf")) else v / C_STAGE[stage_of(k)]) for k, (v, _) in R.items()}


def failures(R):
    return {k: R[k] for k, v in scaled(R).items() if not v <= 1.0}


def worst_by_stage(R):
    return {s: max(v for k, (v, _) in R.items() if stage_of(k) == s) for s in C_STAGE if any(stage_of(k) == s for k in R)}


def report(name, R):
    s = scaled(R)
    return "\n".join([f"{name}:"] + [f"  {k:45s} {R[k][0]:10.3g}  / C -> {s[k]:9.3g}  at {R[k][1]}" for k in R])


def check(case, X, B, Xret, x20=None):
    """Raw worst ratios {"stage.name": (error / (U abs), where)} of one sgo_factor_solve call; exact checks give 0 or inf.
    case: mfront_reference's dict; X: FRONTS, BND, PINV, ELIM_VERTEX, ARENA, YINV, FS_Y and FS_X exported AFTER the call (one chunk: at
    most 256 columns); B [3 n, columns] in hessian order as handed in, Xret what the call returned ([columns, n, 3]), x20 what a call with
    column 20 alone returned (None: not asked).  Every stage reads its inputs from the exported arrays, so an error is charged to
    the kernel that made it and no bound carries a condition number: |got - ref| <= C_stage U abs, ref in np.longdouble, abs the
    same expression on magnitudes; no bound carries a term count (the constants come from the model, whose sums are as long).
      forward   the own-column blocks J of 16 in elimination order: y_J against Y_J (b_J - sum over the earlier columns c of L_Jc y_c)
                with the exported y_c, the update accumulated front by front (a front's L21 y_own lands on its boundary poses'
                rows wherever the tree takes them: the check does not follow the traversal); abs = |Y_J| (|b_J| + |L| |y|).
      backward  per front and block, downwards: x_J against Y_J^T (y_J - L_RJ^T x_R), R = every row of the front after J, y and
                x_R as exported, the boundary rows of x through BND; abs = |Y_J^T| (|y_J| + |L_RJ^T| |x_R|).
      columns   exact: FS_X permuted to the hessian order is the returned X bit for bit; column 20 solved alone has the same bits."""
    R = Result()
    plan = sr.Plan(X, case["fixed"])
    n3 = plan.perm.size
    B = np.asarray(B, dtype=np.float64)
    nc = B.shape[1]
    ok = B.shape[0] == n3 and 0 < nc <= 3 * CHUNK_CANDS + 1 and X["FS_Y"].size == nc * n3 == X["FS_X"].size
    R.exact("columns.the_export_holds_every_column", ok)
    if not ok:
        return R
    Yd, Xd = X["FS_Y"].reshape(nc, n3).T, X["FS_X"].reshape(nc, n3).T
    Xh = np.asarray(Xret, dtype=np.float64).reshape(nc, n3).T
    R.exact("columns.the_returned_solution_is_the_export_permuted", np.array_equal(_bits(to_hessian_order(plan, Xd)), _bits(Xh)))
    if x20 is not None:
        R.exact("columns.column_20_alone_has_the_same_bits", nc > 20 and np.array_equal(_bits(np.asarray(x20).ravel()), _bits(Xh[:, 20])))
    arena, yinv = X["ARENA"], X["YINV"]
    Bp = B[plan.perm]
    upd, upda = np.zeros((n3, nc), dtype=LD), np.zeros((n3, nc))
    worst = {"forward.y": (0.0, None), "backward.x": (0.0, None)}

    def note(name, r, at, where):
        if r > worst[name][0]:
            worst[name] = (r, where + tuple(at or ()))
    rows = [plan.rows(F) for F in plan.fronts]
    for f, F in enumerate(plan.fronts):
        m, s3 = F.m, F.own3
        if s3 == 0:
            continue
        own, bnd = rows[f][:s3], rows[f][s3:]
        A = front_matrix(arena, F)[:m, :s3]
        yo = Yd[own]
        t, ta = Bp[own].astype(LD) - upd[own], np.abs(Bp[own]) + upda[own]
        for k0 in range(0, s3, PANEL):
            rb = min(k0 + PANEL, s3)
            Yj = yinv[3 * F.e0 + k0:3 * F.e0 + rb, :rb - k0]
            note("forward.y", *entry_ratio(yo[k0:rb], Yj.astype(LD) @ t[k0:rb], np.abs(Yj) @ ta[k0:rb]), (f, k0))
            t[rb:] -= A[rb:s3, k0:rb].astype(LD) @ yo[k0:rb].astype(LD)
            ta[rb:] += np.abs(A[rb:s3, k0:rb]) @ np.abs(yo[k0:rb])
        upd[bnd] += A[s3:].astype(LD) @ yo.astype(LD)
        upda[bnd] += np.abs(A[s3:]) @ np.abs(yo)
    for f in range(len(plan.fronts) - 1, -1, -1):
        F = plan.fronts[f]
        m, s3 = F.m, F.own3
        if s3 == 0:
            continue
        A = front_matrix(arena, F)[:m, :s3]
        x, y = Xd[rows[f]], Yd[rows[f][:s3]]
        for k0 in range(((s3 - 1) // PANEL) * PANEL, -1, -PANEL):
            rb = min(k0 + PANEL, s3)
            Yj = yinv[3 * F.e0 + k0:3 * F.e0 + rb, :rb - k0]
            v = y[k0:rb].astype(LD) - A[rb:, k0:rb].astype(LD).T @ x[rb:].astype(LD)
            va = np.abs(y[k0:rb]) + np.abs(A[rb:, k0:rb]).T @ np.abs(x[rb:])
            note("backward.x", *entry_ratio(x[k0:rb], Yj.astype(LD).T @ v, np.abs(Yj).T @ va), (f, k0))
    for k, v in worst.items():
        R.put(k, *v)
    return R


def check_gate(case, X, cand, d2, P):
    """The gate stage of one sgo_candidate_gate call for the candidates cand = (ci, cj, meas, info): raw ratios as check()'s.
    X: ELIM_VERTEX and FS_X exported AFTER the call.  FS_X holds the LAST chunk of CHUNK_CANDS candidates only; exactly the candidates
    whose columns it holds are checked, at least one (asserted).
      gate.P    P against (Q + Q^T) / 2, Q = R^T W: W the exported columns, R from overlay_reference.edge_parts_ld (np_oracle's
                Jacobians in long double) at the case's poses; abs from kernel_reference.edge_terms' magnitudes of A and B.
      d2.mahalanobis   d2 against e^T (Omega^-1 + P)^-1 e in long double with the device's OWN P (this stage's input) and e from
                edge_parts_ld.  d2 passes through a 3 x 3 inverse, so the bound has the form the project's other block inverses
                have (amg_reference.inverse_ratio, dinvF): C U kappa abs, kappa = |S^-1|_2 | |S| |_2 of S = Omega^-1 + P, and
                abs = |z|^T (kappa_Omega |Omega^-1| + |P|) |z| + 2 |z|^T abs(e), z = S^-1 e -- the first-order change of d2 under
                U-relative changes of S's terms (Omega^-1 by cofactors carries Omega's own kappa) and of e.
      gate.both_fixed_is_zero / gate.P_symmetric   exact."""
    from amg_reference import inv3
    R = Result()
    ci, cj, meas, info = (np.asarray(a) for a in cand)
    n = int(np.asarray(X["ELIM_VERTEX"]).size)
    n3, k = 3 * n, ci.size
    t0 = (k - 1) // CHUNK_CANDS * CHUNK_CANDS
    held = np.arange(t0, k)
    ok = held.size >= 1 and X["FS_X"].size == 3 * held.size * n3
    R.exact("gate.the_export_holds_whole_candidates", ok, (t0, k, int(X["FS_X"].size)))
    if not ok:
        return R
    W = X["FS_X"].reshape(3 * held.size, n3).T.astype(LD)
    P0 = np.asarray(case["P0"], dtype=np.float64)
    pos = np.full(P0.shape[0], -1, dtype=np.int64)
    pos[np.asarray(X["ELIM_VERTEX"], dtype=np.int64)] = np.arange(n)
    hi, hj = ci[held].astype(np.int64), cj[held].astype(np.int64)
    e, A, Bm = edge_parts_ld(P0, hi, hj, meas[held])
    tm = kr.edge_terms(P0[hi], P0[hj], meas[held], info[held], np.full(held.size, -1.0))
    Oinv, _ = inv3(npo.info_full(info[held]))
    Oa = np.abs(npo.info_full(info[held]))
    Pd, d2d = np.asarray(P, dtype=np.float64)[held], np.asarray(d2, dtype=np.float64)[held]
    wp, wd, sym, zero = (0.0, None), (0.0, None), True, True
    for q in range(held.size):
        Q, Qa = np.zeros((3, 3), dtype=LD), np.zeros((3, 3))
        for p, J, Ja in ((pos[hi[q]], A[q], tm["A_abs"][q]), (pos[hj[q]], Bm[q], tm["B_abs"][q])):
            if p >= 0:
                Wp = W[3 * p:3 * p + 3, 3 * q:3 * q + 3]
                Q += J @ Wp
                Qa += Ja @ np.abs(Wp).astype(np.float64)
        if pos[hi[q]] < 0 and pos[hj[q]] < 0:
            zero = zero and not Pd[q].any()
        sym = sym and np.array_equal(_bits(Pd[q]), _bits(Pd[q].T.copy()))
        r, at = entry_ratio(Pd[q], (Q + Q.T) / 2, (Qa + Qa.T) / 2)
        if r > wp[0]:
            wp = (r, (int(held[q]),) + at)
        S = Oinv[q] + Pd[q].astype(LD)
        Si, _ = inv3(S[None])
        z = Si[0] @ e[q]
        za = np.abs(z).astype(np.float64)
        O64 = Oinv[q].astype(np.float64)
        kO = np.linalg.norm(O64, 2) * np.linalg.norm(Oa[q], 2)
        kS = np.linalg.norm(Si[0].astype(np.float64), 2) * np.linalg.norm(np.abs(S).astype(np.float64), 2)
        ab = kS * (za @ (kO * np.abs(O64) + np.abs(Pd[q])) @ za + 2.0 * za @ tm["e_abs"][q])
        r, _ = entry_ratio(d2d[q:q + 1], np.array([e[q] @ z]), np.array([ab]))
        if r > wd[0]:
            wd = (r, (int(held[q]),))
    R.put("gate.P", *wp)
    R.put("d2.mahalanobis", *wd)
    R.exact("gate.P_symmetric", sym)
    R.exact("gate.both_fixed_is_zero", zero)
    return R
