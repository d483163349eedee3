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

check(): one call's kernels stage by stage from the arrays sgo_debug_mfront_array exports after it (gather, untouched, offdiag, diag,
result; the function's docstring has the bounds), in the style of mfront_reference.check: inputs as stored, references in long
double, |got - ref| <= C U abs with no condition number -- so it runs on every case, ILL_CONDITIONED's three included.  host_factor()
and pack() put the model's factor and output into the exported layout for the CPU tests; coverage() / COVERS name the panel, gather
and tree shapes the cases must reach.  MODEL / C_STAGE / MEASURED below; DESIGN.md section 5f has the table.

Natural scale of an entry in the rows of pose i and the columns of pose j: sqrt(max |Sigma_ii| max |Sigma_jj|)
(marginals_reference.py: Cauchy-Schwarz bounds the off-diagonal block by it).
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from amg_reference import Result, entry_ratio
from mfront_reference import Front, child_rows, constant, front_matrix, local_elim, stage_of
from oracle import np_oracle as npo

PANEL = 16
NW, KSTEP = 8, 4       # k_si_panels: eight waves share Sigma_JJ's contraction in matrix-core steps of four rows
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


def host_factor(plan, H):
    """(ARENA, YINV) as the factorisation leaves them, from numpy's own Cholesky of H in the plan's elimination order: every
    front's L11 over L21 in the front's layout (mfront_reference.front_matrix; row m, the right-hand side, stays zero) and
    the explicit inverses of the 16 x 16 diagonal blocks' factors, zero right of the diagonal.  np.linalg.LinAlgError when H
    is not positive definite."""
    X = plan.X
    Hp = np.asarray(H.todense() if sp.issparse(H) else H)[np.ix_(plan.perm, plan.perm)]
    L = np.linalg.cholesky(Hp)
    arena = np.zeros(int(X["INFO"][4]))
    yinv = np.zeros((plan.perm.size, PANEL))
    for F in plan.fronts:
        r, s3 = plan.rows(F), F.own3
        Lf = L[np.ix_(r, r[:s3])]
        front_matrix(arena, F)[:F.m, :s3] = np.where(np.arange(F.m)[:, None] >= np.arange(s3)[None, :], Lf, 0.0)
        for k0 in range(0, s3, PANEL):
            rb = min(k0 + PANEL, s3)
            yinv[3 * F.e0 + k0:3 * F.e0 + rb, :rb - k0] = sla.solve_triangular(Lf[k0:rb, k0:rb], np.eye(rb - k0), lower=True)
    return arena, yinv


def wave_share(nR, wave):
    """[k0, k1): the rows of R that wave `wave` of k_si_panels' eight contracts for Sigma_JJ (steps of four, fixed shares)"""
    steps = (nR + KSTEP - 1) // KSTEP
    per = (steps + NW - 1) // NW
    return min(nR, KSTEP * wave * per), min(nR, KSTEP * min(steps, (wave + 1) * per))


def model(plan, H, mut=None, factor=None, mut_front=None, stale=None):
    """[front] -> its selected inverse, dense [m, m], lower triangle (zeros above); np.linalg.LinAlgError when H is not positive
    definite.  factor: host_factor's arrays (made here when not given).  mut: one of the CPU tests' mutations, applied at
    front mut_front where it concerns one front; stale: another run's result, for mut = "stale_offdiag"."""
    arena, yinv = host_factor(plan, H) if factor is None else factor
    S = [None] * len(plan.fronts)
    rows = [plan.rows(F) for F in plan.fronts]
    for f in range(len(plan.fronts) - 1, -1, -1):      # parents have the higher numbers
        F = plan.fronts[f]
        m, s3 = F.m, F.own3
        here = mut_front is None or mut_front == f
        Sf = np.zeros((m, m))
        if F.parent >= 0:
            pr = rows[F.parent]
            loc = {int(g): i for i, g in enumerate(pr)}
            idx = np.array([loc[int(g)] for g in rows[f][s3:]], dtype=np.int64)
            if mut == "gather_neighbour_pose" and here:
                idx = (idx + 3) % pr.size
            Sp = S[F.parent]
            full = np.tril(Sp) + np.tril(Sp, -1).T
            Sf[s3:, s3:] = np.tril(full[np.ix_(idx, idx)])
        Lf = front_matrix(arena, F)[:m, :s3]             # [m, own3]: L11 over L21
        for k0 in range(((s3 - 1) // PANEL) * PANEL if s3 else -1, -1, -PANEL):
            wp = min(PANEL, s3 - k0)
            rb = k0 + wp
            nR = m - rb
            Y = yinv[3 * F.e0 + k0:3 * F.e0 + rb, :wp]
            T = Lf[rb:, k0:rb] @ Y
            SRR = np.tril(Sf[rb:, rb:]) + np.tril(Sf[rb:, rb:], -1).T
            if mut == "upper_triangle_read_as_stored":
                SRR = Sf[rb:, rb:]
            SRJ = -SRR @ T
            TS = T.T @ SRJ
            if mut == "last_k_dropped" and here and nR:
                SRJ = -SRR[:, :-1] @ T[:-1]
                TS = T[:-1].T @ SRJ[:-1]
            if mut == "stale_offdiag" and here:
                SRJ = stale[f][rb:, k0:rb].copy()
                TS = T.T @ SRJ
            if mut == "wave_share_dropped" and here and nR:
                a, b = wave_share(nR, ((nR + KSTEP - 1) // KSTEP - 1) // max(1, ((nR + KSTEP - 1) // KSTEP + NW - 1) // NW))
                TS = TS - T[a:b].T @ SRJ[a:b]
            YY = Y.T @ Y
            if mut == "narrow_panel_rows_as_stored" and here and wp < PANEL:
                Y16 = yinv[3 * F.e0 + k0:3 * F.e0 + k0 + PANEL, :wp]      # (the rows after the panel: the next front's inverses)
                YY = Y16.T @ Y16
            SJJ = YY - TS
            if mut == "diagonal_term_dropped":
                SJJ = 0.0 - TS
            Sf[rb:, k0:rb] = SRJ
            Sf[k0:rb, k0:rb] = np.tril(SJJ)
        S[f] = Sf
    return S


def pack(X, S):
    """SGO_MF_SEL from every front's dense selected inverse: the inverse of front_from_arena (lower triangles; the rest zero)"""
    sel = np.zeros(int(X["INFO"][4]))
    for r, Sf in zip(X["FRONTS"], S):
        F = Front(r)
        front_from_arena(sel, F)[:] = np.tril(Sf)
    return sel


def results(plan, S, vi, vj, V):
    """(D (V, 3, 3), cov (pairs, 3, 3)) as k_si_result copies them out of the fronts' selected inverses S"""
    X = plan.X
    n = plan.elim_vertex.size
    pos = np.full(V, -1, dtype=np.int64)
    pos[plan.elim_vertex] = np.arange(n)
    front_of = np.repeat(np.arange(len(plan.fronts)), [F.own for F in plan.fronts])
    D, cov = np.zeros((V, 3, 3)), np.zeros((len(vi), 3, 3))

    def block(ph, pl):
        F = plan.fronts[front_of[pl]]
        lh = int(np.flatnonzero(local_elim(X, F) == ph)[0])
        ll = pl - F.e0
        return S[front_of[pl]][3 * lh:3 * lh + 3, 3 * ll:3 * ll + 3]
    for p in range(n):
        b = block(p, p)
        D[plan.elim_vertex[p]] = np.tril(b) + np.tril(b, -1).T
    for t, (i, j) in enumerate(zip(vi, vj)):
        pi, pj = pos[i], pos[j]
        if pi < 0 or pj < 0:
            continue
        cov[t] = D[i] if pi == pj else (block(pi, pj) if pi > pj else block(pj, pi).T)
    return D, cov


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


# ------------------------------------------------------------------ the stage checks (the style of mfront_reference.check)
STAGES = ("gather", "untouched", "offdiag", "diag", "result")
# Worst error / (U abs) of model() over the cases of tests/mfront_cases.py against check()'s long-double expressions, and where
# (tests/test_selinv_reference.py holds the model to them); C = 4 x that, rounded up to a power of two (mfront_reference.constant):
#   stage     model   case                 C
#   offdiag   22.15   lattice_50           128   (numpy sums nR products in a row; abs carries no factor nR)
#   diag      17.29   lattice_50           128
# gather, untouched and result are exact.
MODEL = dict(offdiag=22.15, diag=17.29)
C_STAGE = {k: constant(v) for k, v in MODEL.items()}
# Worst error / (U abs) measured on the MI355X over tests/test_gpu_selinv_reference.py, and where
MEASURED = dict(offdiag=(22.46, "lattice_50"), diag=(6.879, "lattice_48"))


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


def check(case, X, D, cov, vi, vj, refs=None):
    """Raw worst ratios {"stage.name": (error / (U abs), where)} of one sgo_marginals_selected call; exact checks give 0 or inf.
    case: mfront_reference's dict; X: FRONTS, BND, PINV, ELIM_VERTEX, ARENA, YINV and SEL exported AFTER the call (the factor the call
    made and what it left in the second arena, as stored); D, cov: what the call returned for the pairs (vi, vj).  Every stage
    reads its inputs from the exported arrays themselves, front by front (no dense 3 n x 3 n matrix), so an error is charged to
    the kernel that made it and no bound carries a condition number: |got - ref| <= C_stage U abs, ref in np.longdouble, abs the
    same expression on magnitudes.  No bound carries the term count (nR or 16): the constants are measured on the model, whose
    sums are as long.
      gather     exact: every stored entry (row >= column) of a non-root front's boundary block has the bits of its parent's
                 stored entry, found through the boundary map (PINV) in the parent's lower triangle with (lo, hi) ordered.
      untouched  exact: zero bits everywhere else in SEL -- the strict upper triangles, row m, the rows between m and ld, the
                 gaps between the fronts, and a root's boundary-less rest: k_si_panels writes the own columns from the diagonal
                 down, k_si_gather the boundary block's lower triangle, nothing else is written after the arena was zeroed.
      offdiag    per panel J of 16 own columns, last to first, R = every row of the front after J: Sigma_RJ against
                 -Sigma_RR T, T = L_RJ Y_J from ARENA and YINV, Sigma_RR the front's own exported lower triangle read as a symmetric
                 matrix; abs = |Sigma_RR| (|L_RJ| |Y_J|).  T is not exported: its fp64 rounding, U |L_RJ| |Y_J| per entry, is inside abs.
      diag       the stored lower triangle of Sigma_JJ against Y_J^T Y_J - T^T Sigma_RJ with the device's Sigma_RJ;
                 abs = |Y_J|^T |Y_J| + (|L_RJ| |Y_J|)^T |Sigma_RJ|.
      result     exact: D[v] and cov[t] are bit copies of the entries they name (the upper triangle of a diagonal block mirrored,
                 (vj, vi) the transpose of (vi, vj)); a pair with a fixed or edgeless vertex is exactly zero.
    refs: an array of SEL's size that receives the reference value (rounded to fp64) of every stored entry of the own columns."""
    R = Result()
    fronts = [Front(r) for r in X["FRONTS"]]
    arena, sel, yinv = X["ARENA"], X["SEL"], X["YINV"]
    R.exact("structure.one_root_and_the_arenas_agree", sel.size == arena.size and sum(F.parent < 0 for F in fronts) == 1)
    if R.worst() > 0:
        return R
    written = np.zeros(sel.size, dtype=bool)
    gather_bad = None
    worst = {"offdiag.Sigma_RJ": (0.0, None), "diag.Sigma_JJ": (0.0, None)}

    def note(name, r, at, where):
        if r > worst[name][0]:
            worst[name] = (r, where + tuple(at or ()))
    for f, F in enumerate(fronts):
        m, s3 = F.m, F.own3
        if m == 0:
            continue
        Sf = front_from_arena(sel, F)
        low = np.arange(m)[:, None] >= np.arange(m)[None, :]
        front_from_arena(written, F)[:] = low & ((np.arange(m)[None, :] < s3) | (F.parent >= 0))
        if F.parent >= 0 and m > s3:
            P = fronts[F.parent]
            pr, cr = child_rows(X, P, P.kid.index(f), F)
            pr, cr = pr[:-1], cr[:-1]
            Sp = front_from_arena(sel, P)
            want = np.where(pr[:, None] >= pr[None, :], Sp[np.ix_(pr, pr)], Sp[np.ix_(pr, pr)].T)
            stored = cr[:, None] >= cr[None, :]
            bad = stored & (_bits(Sf[np.ix_(cr, cr)]) != _bits(want))
            if (cr.size != m - s3 or bad.any()) and gather_bad is None:
                at = np.argwhere(bad)
                gather_bad = (f,) + (tuple(int(v) for v in (cr[at[0, 0]], cr[at[0, 1]])) if at.size else ())
        if s3 == 0:
            continue
        A = front_matrix(arena, F)[:m, :s3]
        full = np.where(low, Sf, Sf.T).astype(LD)
        fabs = np.abs(np.where(low, Sf, Sf.T))
        for k0 in range(((s3 - 1) // PANEL) * PANEL, -1, -PANEL):
            wp = min(PANEL, s3 - k0)
            rb = k0 + wp
            Y = yinv[3 * F.e0 + k0:3 * F.e0 + rb, :wp]
            T = A[rb:, k0:rb].astype(LD) @ Y.astype(LD)
            Ta = np.abs(A[rb:, k0:rb]) @ np.abs(Y)
            if m > rb:
                ref = -(full[rb:, rb:] @ T)
                note("offdiag.Sigma_RJ", *entry_ratio(Sf[rb:, k0:rb], ref, fabs[rb:, rb:] @ Ta), (f, k0))
                if refs is not None:
                    front_from_arena(refs, F)[rb:, k0:rb] = ref.astype(np.float64)
            lo = np.tril(np.ones((wp, wp), dtype=bool))
            ref = Y.astype(LD).T @ Y.astype(LD) - T.T @ full[rb:, k0:rb]
            ab = np.abs(Y).T @ np.abs(Y) + Ta.T @ fabs[rb:, k0:rb]
            note("diag.Sigma_JJ", *entry_ratio(np.where(lo, Sf[k0:rb, k0:rb], 0.0), np.where(lo, ref, 0), np.where(lo, ab, 0.0)), (f, k0))
            if refs is not None:
                blk = front_from_arena(refs, F)[k0:rb, k0:rb]
                blk[lo] = ref.astype(np.float64)[lo]
    R.exact("gather.boundary_blocks_are_the_parents_bits", gather_bad is None, gather_bad)
    stray = np.flatnonzero(~written & (_bits(sel) != 0))
    R.exact("untouched.zero_bits_outside_the_stored_entries", stray.size == 0, tuple(int(v) for v in stray[:4]))
    for k, v in worst.items():
        R.put(k, *v)
    # the outputs
    S = [front_from_arena(sel, F) for F in fronts]
    plan = Plan(X, case["fixed"])
    V = np.asarray(case["fixed"]).size
    Dw, cw = results(plan, S, vi, vj, V)
    bad = np.flatnonzero((_bits(D).reshape(V, 9) != _bits(Dw).reshape(V, 9)).any(1)) if D is not None else np.zeros(0, dtype=int)
    R.exact("result.diag_blocks_are_copies", bad.size == 0, tuple(int(v) for v in bad[:4]))
    bad = np.flatnonzero((_bits(cov).reshape(-1, 9) != _bits(cw).reshape(-1, 9)).any(1))
    R.exact("result.pair_blocks_are_copies", bad.size == 0, tuple(int(v) for v in bad[:4]))
    return R


# ------------------------------------------------------------------ the shapes the kernels' branches need
def _panels(X):
    for r in np.asarray(X["FRONTS"], dtype=np.int64):
        s3, m = int(r[1]), int(r[2])
        for k0 in range(0, s3, PANEL):
            wp = min(PANEL, s3 - k0)
            yield wp, m - k0 - wp


def coverage(X):
    """{class: reached} for one front table (host plan or device export): the panels of k_si_panels (wp columns, nR rows after
    them), the gathers of k_si_gather (nb3 boundary rows) and the tree."""
    F = np.asarray(X["FRONTS"], dtype=np.int64)
    own3, m, parent = F[:, 1], F[:, 2], F[:, 13]
    nb3 = (m - own3)[parent >= 0]
    pn = list(_panels(X))
    steps = lambda nR: (nR + KSTEP - 1) // KSTEP
    # (a pose's three rows straddle two panels exactly where a panel ends off a multiple of 3: wp in {1, 2} is the tail of such a front)
    return {
        "wp_16": any(wp == 16 for wp, _ in pn),
        "wp_1_or_2_a_pose_straddles_two_panels": any(wp in (1, 2) for wp, _ in pn),
        "wp_3_to_15": any(3 <= wp <= 15 for wp, _ in pn),
        "nR_0": any(nR == 0 for _, nR in pn),
        "nR_below_16": any(0 < nR < 16 for _, nR in pn),
        "nR_no_multiple_of_4": any(nR % 4 for _, nR in pn),
        "nR_17_to_32": any(16 < nR <= 32 for _, nR in pn),
        "nR_in_9_steps_a_waves_share_starts_beyond": any(steps(nR) == 9 for _, nR in pn),   # per = 2: wave 5's share starts at step 10
        "nR_above_128_two_row_tiles_per_wave": any(nR > 128 for _, nR in pn),
        "gather_nb3_below_16": bool(((nb3 > 0) & (nb3 < 16)).any()),
        "gather_nb3_above_16_offdiagonal_tiles_a_pose_straddles": bool((nb3 > 16).any()),     # (nb3 >= 18: pose 5 holds rows 15 .. 17)
        "front_without_own_columns": bool((own3 == 0).any()),
    }


# One case per class, by name (asserted from the host plan on the CPU and from the device's export on the GPU).  The issue's
# "more than one root" does not exist: the nested dissection returns ONE root for any graph, and joins unconnected components under
# a front without own columns (sgo_mfront_host.cpp, Dissector::dissect) -- front_without_pivots is that case; check() asserts the
# single root.
COVERS = {
    "wp_16": "child_own3_48", "wp_1_or_2_a_pose_straddles_two_panels": "child_own3_18", "wp_3_to_15": "child_own3_12",
    "nR_0": "root_own3_15", "nR_below_16": "child_own3_12", "nR_no_multiple_of_4": "child_own3_15", "nR_17_to_32": "child_own3_33",
    "nR_in_9_steps_a_waves_share_starts_beyond": "child_own3_48", "nR_above_128_two_row_tiles_per_wave": "lattice_50",
    "gather_nb3_below_16": "child_own3_12", "gather_nb3_above_16_offdiagonal_tiles_a_pose_straddles": "tree_shapes",
    "front_without_own_columns": "front_without_pivots",
}
