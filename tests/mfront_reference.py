"""Stage-by-stage reference for the multifrontal path (CPU only, test infrastructure; sibling of overlay_reference.py).

What it checks.  One Gauss-Newton iteration of sgo_mfront.hip from the arrays sgo_debug_mfront_array exports after optimize(1)
(include/sgo.h names them), the poses P0 before the call and P1 after it -- stage by stage in the order the launches run:
k_mf_edges, per level k_mf_merge + k_mf_panels, per level k_mf_solve, k_mf_update.  Every stage takes its inputs from the
exported arrays themselves (a parent's assembly from its children's stored factors, the substitution from the stored x of the
boundary poses), so an error is charged to the stage that made it.

A case (dict): P0 (V,3), fixed (V,), ei, ej, meas, info, phi as sgo_set_graph_se2's.
X (dict): the SGO_MF_* arrays by name (capi.MFRONT_ARRAYS), "P1" (V,3) and "hist" = (chi2[0], robust[0], chi2[1], robust[1]).

Part A, model(): the same iteration in plain fp64 numpy from the HOST plan (capi.mfront_plan_arrays): the edges' elements by
np_oracle's formulas, a straightforward extend-add, column Cholesky, triangular solves.  It does not imitate the kernels'
products with explicit 16 x 16 inverses or their summation order; it is what the constants are taken from, and what the CPU
tests mutate.

Part B, check(): every entry gets |got - ref| <= C_stage U abs, ref in np.longdouble, abs the same expression on magnitudes.
  structure   exact: the tables are consistent with the graph (fronts partition the elimination order, BND ascending and later
              than the own poses, PINV the inverse of the children's boundaries, every edge's parts at the front of its
              first-eliminated endpoint exactly once, levels = heights).
  elements    ELEM against the edge algebra in long double at P0 (overlay_reference.edge_blocks_ld, robust weight included);
              abs from kernel_reference.edge_terms' magnitudes.
  assembly    per front F = the edges' parts (ELEM as exported, through TARGETS / CONTRIB) + sum over the children of
              F22_c - L21_c L21_c^T (the children's matrices as exported, positions through PINV, row m = the right-hand side).
              The stored boundary block (rows and columns >= own3, row m included) against F per entry, abs = sum |terms| +
              |L21_c| |L21_c^T|; entries nothing reaches have abs = 0 and must be exactly 0.
  factor      |F - L L^T|_ij <= C U ((j + 1) (|L| |L^T|)_ij + abs(F)_ij) on the own columns j, rows j .. m: the componentwise
              bound of a stable Cholesky with j + 1 terms per sum; row m is the forward-substituted right-hand side.  abs(F):
              the device factorises ITS assembled F, which the stage above holds to U abs(F) and which is not stored.
  inverses    per 16-column panel |Y L_dd - I| <= C U |Y| |L_dd|, Y exactly zero right of the diagonal; |INVD L_cc - 1| <= C U.
  substitution per front, x of the boundary poses as exported: |L11^T x_own - (y - L21^T x_bnd)|_j <=
              C s U (|L11^T| |x_own| + |y| + |L21^T| |x_bnd|)_j, s = own3.
  update      P1 = P0 (+) x through ELIM_VERTEX: one rounding of the add, U (|P0| + |x|), and for the angle of its normalisation
              as well, 2 U (|theta| + |x| + 2 pi) modulo 2 pi (overlay_reference's finish bound); angles in [-pi, pi); every
              other vertex bit-equal.
  composed    independent of the tree: |b - H x|_i <= C U (abs(b) + abs(H x) + |L| |L^T| |x|)_i with b, H x and their abs from
              kernel_reference at P0 (H never formed) and the last term -- the backward error of any Cholesky solve, the
              condition-scaled part -- accumulated front by front from the exported factor.
  history     hist against kernel_reference's long-double chi2 / robust chi2 at P0 and at P1.

Constants.  Each C is taken from the reference side alone: tests/test_mfront_reference.py measures model()'s worst ratio
against the same long-double expressions over all cases of tests/mfront_cases.py; C = that ratio x 4, rounded up to a power
of two (the margin: the kernels sum in another order -- 4-wide matrix-core accumulation -- and take a Newton-refined reciprocal
square root where the model divides by a square root).  MODEL / C_STAGE / MEASURED below; DESIGN.md section 5c has the table.
"""
from __future__ import annotations

import math

import numpy as np

import kernel_reference as kr
from amg_reference import Result, entry_ratio
from kernel_reference import LD, U
from oracle import np_oracle as npo
from overlay_reference import edge_blocks_ld

PANEL = 16
SOLVE_OWN, SOLVE_BND = 144, 256          # k_mf_solve's fast branch: own3 <= 144 and nb3 <= 256
FRONT_COLS = "e0 own3 m ld off nb bnd_off kid0 kid1 pinv_off0 pinv_off1 tgt0 tgt1 parent".split()
STAGES = ("elements", "assembly", "factor", "inverses", "substitution", "update", "composed", "history")

# Worst error / (U abs) of model() over the cases of tests/mfront_cases.py, and where (tests/test_mfront_reference.py holds the model
# to them); the constants they give, 4 x rounded up to a power of two:
#   stage         model   case                          C
#   elements      4.78    lattice_50                    32
#   assembly      12.4    lattice_50                    64    (numpy sums a child's K products in a row; abs carries no factor K)
#   factor        3.92    lattice_50                    16
#   inverses      18.2    child_own3_114                128   (Y from L_dd Y = I: it is the RIGHT residual a substitution keeps small)
#   substitution  0.343   long_thin_chain               2     (of a bound that carries s = own3)
#   update        0.9992  lattice_48                    4
#   composed      0.277   long_thin_chain               2
#   history       0.0688  dcs_switches_closures_off     0.5
MODEL = dict(elements=4.78, assembly=12.4, factor=3.92, inverses=18.2, substitution=0.343, update=0.9992, composed=0.277, history=0.0688)
# Worst error / (U abs) measured on the MI355X over tests/test_gpu_mfront_reference.py, and where:
# elements lattice_50, assembly lattice_48, factor lattice_50, inverses solve_generic_147, substitution long_thin_chain, update
# lattice_48, composed rows_scaled_1e6, history dcs_switches_closures_off.  Before k_mf_panels refined its product with the
# explicit inverse (D3): factor 2.51e4 and composed 599 on rows_scaled_1e6; model(mut="explicit_inverse_product") restates that
# arithmetic in fp64 and measures 2.44e4 and 528.
MEASURED = dict(elements=4.58, assembly=13.2, factor=4.53, inverses=20.0, substitution=0.685, update=0.998, composed=0.451, history=0.126)


def constant(model_ratio):
    return 2.0 ** math.ceil(math.log2(4.0 * model_ratio))


C_STAGE = {k: constant(v) for k, v in MODEL.items()}


def stage_of(name):
    return name.split(".")[0]


def scaled(R):
    """{check: ratio / C_stage}: a value above 1 fails (exact checks: 0 or inf)."""
    return {k: (v if stage_of(k) not in C_STAGE or v in (0.0, float("inf")) else v / C_STAGE[stage_of(k)]) for k, (v, _) in R.items()}


def failures(R):
    return {k: R[k] for k, v in scaled(R).items() if not v <= 1.0}


def worst_by_stage(R):
    w = {}
    for k, (v, _) in R.items():
        s = stage_of(k)
        if s in C_STAGE:
            w[s] = max(w.get(s, 0.0), v)
    return w


# ------------------------------------------------------------------ the tables
class Front:
    def __init__(self, row):
        for k, v in zip(FRONT_COLS, row):
            setattr(self, k, int(v))
        self.kid = (self.kid0, self.kid1)
        self.pinv_off = (self.pinv_off0, self.pinv_off1)
        self.own = self.own3 // 3
        self.nb3 = self.m - self.own3


def fronts_of(X):
    return [Front(r) for r in X["FRONTS"]]


def front_matrix(arena, F):
    """The front's stored matrix as [row, column], rows 0 .. m (a view: column-major with leading dimension ld)."""
    return arena[F.off:F.off + F.ld * F.m].reshape(F.m, F.ld).T[:F.m + 1]


def local_elim(X, F):
    """Elimination position of every local pose of the front (own first, then boundary)."""
    return np.r_[np.arange(F.e0, F.e0 + F.own), X["BND"][F.bnd_off:F.bnd_off + F.nb]].astype(np.int64)


def child_rows(X, F, k, C):
    """(parent scalar rows 0 .. m, child scalar rows) of the entries child k = C holds of front F; the last pair is row m."""
    pinv = X["PINV"][F.pinv_off[k]:F.pinv_off[k] + F.m // 3].astype(np.int64)
    lp = np.flatnonzero(pinv >= 0)
    pr = (3 * lp[:, None] + np.arange(3)[None, :]).ravel()
    cr = (C.own3 + 3 * pinv[lp][:, None] + np.arange(3)[None, :]).ravel()
    return np.r_[pr, F.m], np.r_[cr, C.m]


def tril_rhs(m):
    """Mask of the stored part of an (m + 1) x m front: rows >= columns (row m is the right-hand side)."""
    return np.arange(m + 1)[:, None] >= np.arange(m)[None, :]


_TRI = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def add_edges(Fm, Fa, X, F, elem, mut=None):
    """The edges' parts of front F added to Fm (and their magnitudes to Fa, when given) in contribution order."""
    m = F.m
    for t in range(F.tgt0, F.tgt1):
        li, lj, c0, c1 = (int(v) for v in X["TARGETS"][t])
        for q, c in enumerate(range(c0, c1)):
            if mut == "fifth_contribution_dropped" and q == 4:
                continue
            w = int(X["CONTRIB"][c])
            el = elem[w >> 2]
            if li == lj:
                s, r0 = w & 1, 3 * li
                for z, (a, b) in enumerate(_TRI):
                    Fm[r0 + b, r0 + a] += el[6 * s + z]
                    if Fa is not None:
                        Fa[r0 + b, r0 + a] += abs(el[6 * s + z])
                Fm[m, r0:r0 + 3] += el[21 + 3 * s:24 + 3 * s]
                if Fa is not None:
                    Fa[m, r0:r0 + 3] += np.abs(el[21 + 3 * s:24 + 3 * s])
            else:
                H = el[12:21].reshape(3, 3)
                if (w & 3) == 3 and mut != "hij_not_transposed":
                    H = H.T
                Fm[3 * li:3 * li + 3, 3 * lj:3 * lj + 3] += H
                if Fa is not None:
                    Fa[3 * li:3 * li + 3, 3 * lj:3 * lj + 3] += np.abs(H)


def assemble(X, F, fronts, arena, elem, dtype, mut=None, want_abs=True):
    """(F, abs F) of front F, [m + 1, m], lower part, from its children's stored matrices and the edges' elements."""
    m = F.m
    Fm = np.zeros((m + 1, m), dtype=dtype)
    Fa = np.zeros((m + 1, m)) if want_abs else None
    for k in range(2):
        if F.kid[k] < 0 or (mut == "child_left_out" and k == 1):
            continue
        C = fronts[F.kid[k]]
        pr, cr = child_rows(X, F, k, C)
        A = front_matrix(arena, C)
        L21 = A[cr][:, :C.own3].astype(dtype)
        if mut == "schur_last_k_dropped":
            L21 = L21[:, :-1]
        # (both orders ascend with the elimination position -- structure() holds PINV to that --, so the child's stored lower
        # part lands in the parent's lower part; what either stores above the diagonal is never written and never read)
        lo = tril_rhs(cr.size - 1)
        F22 = np.where(lo, A[np.ix_(cr, cr[:-1])], 0.0).astype(dtype)
        Fm[np.ix_(pr, pr[:-1])] += np.where(lo, F22 - L21 @ L21[:-1].T, 0)
        if want_abs:
            La = np.abs(L21).astype(np.float64)
            Fa[np.ix_(pr, pr[:-1])] += np.where(lo, np.abs(F22).astype(np.float64) + La @ La[:-1].T, 0.0)
    add_edges(Fm, Fa, X, F, elem, mut)
    return Fm, Fa


# ------------------------------------------------------------------ part A: the fp64 model
def _elem_from_terms(t):
    E = t["e2"].shape[0]
    el = np.zeros((E, 28))
    for z, (a, b) in enumerate(_TRI):
        el[:, z] = t["Hii"][:, a, b]
        el[:, 6 + z] = t["Hjj"][:, a, b]
    el[:, 12:21] = t["Hij"].reshape(E, 9)
    el[:, 21:24] = t["bi"]
    el[:, 24:27] = t["bj"]
    return el


def _elem_abs(t):
    E = t["e2"].shape[0]
    el = np.zeros((E, 28))
    for z, (a, b) in enumerate(_TRI):
        el[:, z] = t["Hii_abs"][:, a, b]
        el[:, 6 + z] = t["Hjj_abs"][:, a, b]
    el[:, 12:21] = t["Hij_abs"].reshape(E, 9)
    el[:, 21:24] = t["bi_abs"]
    el[:, 24:27] = t["bj_abs"]
    return el


def edge_terms(case, P=None):
    P = case["P0"] if P is None else P
    ei, ej = np.asarray(case["ei"], dtype=np.int64), np.asarray(case["ej"], dtype=np.int64)
    return kr.edge_terms(P[ei], P[ej], case["meas"], case["info"], case["phi"])


def model(case, plan, mut=None, mut_front=None):
    """One Gauss-Newton iteration in plain fp64 from the host plan's tables: X as the device exports it (+ P1, hist).
    mut: one of the CPU tests' mutations, applied at front mut_front where it concerns one front."""
    X = dict(plan)
    fronts = fronts_of(X)
    n = int(X["INFO"][0])
    P0 = np.asarray(case["P0"], dtype=np.float64)
    t = edge_terms(case)
    X["ELEM"] = _elem_from_terms(t)
    arena = np.zeros(int(X["INFO"][4]))
    x = np.zeros(3 * n)
    invd = np.zeros(3 * n)
    yinv = np.zeros((3 * n, PANEL))
    for fi, F in enumerate(fronts):
        here = mut_front is None or mut_front == fi
        m, s3 = F.m, F.own3
        Fm, Fa = assemble(X, F, fronts, arena, X["ELEM"], np.float64, mut if here else None, want_abs=mut == "unreached_entry_left")
        if mut == "unreached_entry_left" and here:
            at = np.argwhere(tril_rhs(m)[s3:, s3:] & (Fa[s3:, s3:] == 0.0))
            if at.size:
                Fm[s3 + at[0, 0], s3 + at[0, 1]] = 1e-300
        L = Fm
        explicit = mut in ("explicit_inverse_product", "explicit_inverse_refined") and here
        if explicit:
            # k_mf_panels' arithmetic: the rows below a panel's diagonal block, row m included, as the PRODUCT with the explicit
            # inverse of the block's factor (not backward stable: the error carries the block's condition), as it was; _refined:
            # with the one refinement against the factor that D3 now makes
            for k0 in range(0, s3, PANEL):
                wp = min(PANEL, s3 - k0)
                Pn = L[k0:, k0:k0 + wp] - L[k0:, :k0] @ L[k0:k0 + wp, :k0].T
                L11 = np.linalg.cholesky(Pn[:wp])
                Y = np.zeros((wp, wp))
                for c in range(wp):
                    for i in range(c, wp):
                        Y[i, c] = ((1.0 if i == c else 0.0) - L11[i, c:i] @ Y[c:i, c]) / L11[i, i]
                L[k0:k0 + wp, k0:k0 + wp] = L11
                L[k0 + wp:, k0:k0 + wp] = Pn[wp:] @ Y.T
                if mut == "explicit_inverse_refined":
                    L[k0 + wp:, k0:k0 + wp] += (Pn[wp:] - L[k0 + wp:, k0:k0 + wp] @ L11.T) @ Y.T
                invd[3 * F.e0 + k0:3 * F.e0 + k0 + wp] = 1.0 / np.diag(L11)
        for j in range(0 if explicit else s3):
            k0 = j - j % PANEL
            col = L[j:, j] - L[j:, :j] @ L[j, :j]
            if mut == "row_m_not_updated" and here and k0 > 0 and k0 == (s3 - 1) // PANEL * PANEL:
                col[-1] = L[m, j] - L[m, k0:j] @ L[j, k0:j]
            d = col[0]
            if not d > 0.0:
                if mut is None:
                    raise np.linalg.LinAlgError(f"front {fi}: pivot {j} = {d}")
                d = abs(d) + 1.0                      # (a mutation may leave the matrix indefinite: go on, the checks reject it)
            r = math.sqrt(d)
            L[j:, j] = col / r
            L[j, j] = r
            invd[3 * F.e0 + j] = 1.0 / d if (mut == "invd_is_1_over_d" and here) else 1.0 / r
        if mut == "l_rounded_to_fp32" and here:
            L[:, :s3] = L[:, :s3].astype(np.float32)
        for k0 in range(0, s3, PANEL):
            wp = min(PANEL, s3 - k0)
            Ldd = np.tril(L[k0:k0 + wp, k0:k0 + wp])
            Y = np.zeros((wp, wp))
            for c in range(wp):                      # L_dd Y = I, column by column: forward substitution
                for i in range(c, wp):
                    Y[i, c] = ((1.0 if i == c else 0.0) - Ldd[i, c:i] @ Y[c:i, c]) / Ldd[i, i]
            if mut == "y_above_diagonal" and here and wp > 1:
                Y[0, 1] = 1e-300
            yinv[3 * F.e0 + k0:3 * F.e0 + k0 + wp, :wp] = Y
        front_matrix(arena, F)[:] = np.where(tril_rhs(m), L, 0.0)
    for fi in range(len(fronts) - 1, -1, -1):
        F = fronts[fi]
        if F.own3 == 0:
            continue
        A = front_matrix(arena, F)
        s3, m = F.own3, F.m
        bp = X["BND"][F.bnd_off:F.bnd_off + F.nb].astype(np.int64)
        if mut == "x_bnd_wrong_pose" and (mut_front is None or mut_front == fi) and F.nb > 1:
            bp = np.roll(bp, 1)
        xb = x.reshape(n, 3)[bp].ravel()
        rhs = A[m, :s3] - A[s3:m, :s3].T @ xb
        xo = np.zeros(s3)
        for j in range(s3 - 1, -1, -1):
            xo[j] = (rhs[j] - A[j + 1:s3, j] @ xo[j + 1:]) / A[j, j]
        x[3 * F.e0:3 * F.e0 + s3] = xo
    ev = X["ELIM_VERTEX"].astype(np.int64)
    if mut == "elim_vertex_swapped" and n > 1:
        ev = ev.copy()
        ev[[0, n - 1]] = ev[[n - 1, 0]]
    P1 = P0.copy()
    P1[ev] = P0[ev] + x.reshape(n, 3)
    if mut != "angle_not_wrapped":
        P1[ev, 2] = npo.normalize_theta(P1[ev, 2])
    t1 = edge_terms(case, P1)
    X.update(ARENA=arena, X=x, INVD=invd, YINV=yinv, FLAGS=np.array([0, 0, 0, 1, 0, 0, 0, 0], dtype=np.int32), P1=P1,
             hist=(float(np.sum(t["e2"].astype(np.float64))), float(np.sum(t["rho0"])),
                   float(np.sum(t1["e2"].astype(np.float64))), float(np.sum(t1["rho0"]))))
    return X


# ------------------------------------------------------------------ part B: the stage checks
def structure(case, X):
    R = Result()
    fronts = fronts_of(X)
    n, E, nf, nlev = (int(v) for v in X["INFO"][:4])
    fixed = np.asarray(case["fixed"], dtype=bool)
    ei, ej = np.asarray(case["ei"], dtype=np.int64), np.asarray(case["ej"], dtype=np.int64)
    deg = np.bincount(np.r_[ei, ej], minlength=fixed.size)
    free = np.flatnonzero(~fixed & (deg > 0))
    ev = X["ELIM_VERTEX"].astype(np.int64)
    R.exact("structure.elim_vertex_is_a_permutation_of_the_free_poses", n == free.size and np.array_equal(np.sort(ev), free))
    ok = len(fronts) == nf and X["LEVEL_PTR"].size == nlev + 1
    e0, height = 0, np.zeros(nf, dtype=np.int64)
    for f, F in enumerate(fronts):
        ok = ok and F.e0 == e0 and F.m == F.own3 + 3 * F.nb and F.ld >= F.m + 1 and F.ld % 2 == 0
        e0 += F.own
        b = X["BND"][F.bnd_off:F.bnd_off + F.nb]
        ok = ok and bool((np.diff(b) > 0).all()) and (F.nb == 0 or b[0] >= F.e0 + F.own)
        le = local_elim(X, F)
        for k in range(2):
            if F.kid[k] < 0:
                continue
            C = fronts[F.kid[k]]
            ok = ok and F.kid[k] < f and C.parent == f
            height[f] = max(height[f], height[F.kid[k]] + 1)
            pinv = X["PINV"][F.pinv_off[k]:F.pinv_off[k] + F.m // 3]
            lp = np.flatnonzero(pinv >= 0)
            cb = X["BND"][C.bnd_off:C.bnd_off + C.nb]
            ok = ok and lp.size == C.nb and np.array_equal(np.sort(pinv[lp]), np.arange(C.nb)) and np.array_equal(le[lp], cb[pinv[lp]])
    R.exact("structure.fronts_boundaries_and_inverse_maps", bool(ok and e0 == n))
    spans = sorted((F.off, F.off + F.ld * F.m) for F in fronts)
    R.exact("structure.matrices_do_not_overlap", all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and
            (not spans or spans[-1][1] <= int(X["INFO"][4])))
    lf, lp_ = X["LEVEL_FRONT"], X["LEVEL_PTR"]
    ok = np.array_equal(np.sort(lf), np.arange(nf)) and lp_[0] == 0 and lp_[-1] == nf
    for h in range(nlev):
        ok = ok and bool((height[lf[lp_[h]:lp_[h + 1]]] == h).all())
    R.exact("structure.levels_are_heights", bool(ok))
    # every edge's parts exactly once, at the front of its first-eliminated endpoint
    pos = np.full(fixed.size, -1, dtype=np.int64)
    pos[ev] = np.arange(n)
    front_of = np.repeat(np.arange(nf), [F.own for F in fronts])
    want = set()
    for e in range(E):
        pa, pb = pos[ei[e]], pos[ej[e]]
        if pa < 0 and pb < 0:
            continue
        home = front_of[min(p for p in (pa, pb) if p >= 0)]
        if pa >= 0:
            want.add((home, pa, pa, e, 0))
        if pb >= 0:
            want.add((home, pb, pb, e, 1))
        if pa >= 0 and pb >= 0:
            want.add((home, max(pa, pb), min(pa, pb), e, 2 if pa > pb else 3))
    got, dup = set(), False
    for f, F in enumerate(fronts):
        le = local_elim(X, F)
        for t in range(F.tgt0, F.tgt1):
            li, lj, c0, c1 = (int(v) for v in X["TARGETS"][t])
            if not (0 <= lj <= li < le.size and c0 < c1):
                dup = True
                continue
            for c in range(c0, c1):
                w = int(X["CONTRIB"][c])
                key = (f, int(le[li]), int(le[lj]), w >> 2, w & 3)
                dup = dup or key in got
                got.add(key)
    R.exact("structure.every_edge_part_once_at_its_home_front", not dup and got == want)
    return R


def check(case, X, stages=STAGES):
    """Raw worst ratios {"stage.name": (error / (U abs), where)}: exact checks give 0 or inf."""
    R = structure(case, X)
    if R.worst() > 0:
        return R                                      # the later stages read the tables
    fronts = fronts_of(X)
    n = int(X["INFO"][0])
    P0 = np.asarray(case["P0"], dtype=np.float64)
    fixed = np.asarray(case["fixed"], dtype=bool)
    ei, ej = np.asarray(case["ei"], dtype=np.int64), np.asarray(case["ej"], dtype=np.int64)
    arena, elem, x = X["ARENA"], X["ELEM"], X["X"]
    R.exact("factor.no_failure_flag", int(X["FLAGS"][0]) == 0 and int(X["FLAGS"][2]) == 0 and int(X["FLAGS"][3]) == 1)
    if "elements" in stages:
        bi, bj, Hii, Hjj, Hij = edge_blocks_ld(P0, ei, ej, case["meas"], case["info"], case["phi"])
        ref = np.zeros((ei.size, 27), dtype=LD)
        for z, (a, b) in enumerate(_TRI):
            ref[:, z], ref[:, 6 + z] = Hii[:, a, b], Hjj[:, a, b]
        ref[:, 12:21], ref[:, 21:24], ref[:, 24:27] = Hij.reshape(-1, 9), bi, bj
        R.put("elements.ELEM", *entry_ratio(elem[:, :27], ref[:, :27], _elem_abs(edge_terms(case))[:, :27]))
    lltx = np.zeros(3 * n)                            # |L| |L^T| |x|, front by front (the composed check's last term)
    worst = {k: (0.0, None) for k in ("assembly.F22", "factor.L", "factor.y", "inverses.Y", "inverses.INVD", "substitution.x")}
    exact_ok = dict(y_zero=True)

    def note(name, r, at, f):
        if r > worst[name][0]:
            worst[name] = (r, (f,) + tuple(at or ()))
    for f, F in enumerate(fronts):
        m, s3 = F.m, F.own3
        A = front_matrix(arena, F)
        low = tril_rhs(m)
        if "assembly" in stages or "factor" in stages:
            Fm, Fa = assemble(X, F, fronts, arena, elem, LD)
        if "assembly" in stages and m > s3:
            got = np.where(low, A, 0.0)[s3:, s3:]
            note("assembly.F22", *entry_ratio(got, np.where(low, Fm, 0)[s3:, s3:], np.where(low, Fa, 0.0)[s3:, s3:]), f)
        L64 = np.where(low, A, 0.0)[:, :s3]
        if "factor" in stages and s3:
            Ll = L64.astype(LD)
            LLt = Ll @ Ll[:s3].T
            La = np.abs(L64)
            den = (np.arange(s3) + 1.0)[None, :] * (La @ La[:s3].T) + Fa[:, :s3]
            msk = low[:, :s3]
            e = np.where(msk, Fm[:, :s3] - LLt, 0)
            den = np.where(msk, den, 0.0)
            note("factor.L", *entry_ratio(e[:m], np.zeros_like(e[:m]), den[:m]), f)
            note("factor.y", *entry_ratio(e[m:], np.zeros_like(e[m:]), den[m:]), f)
        if "inverses" in stages:
            for k0 in range(0, s3, PANEL):
                wp = min(PANEL, s3 - k0)
                Ldd = L64[k0:k0 + wp, k0:k0 + wp]
                Yf = X["YINV"][3 * F.e0 + k0:3 * F.e0 + k0 + wp]
                exact_ok["y_zero"] = exact_ok["y_zero"] and not np.any(np.triu(Yf, 1) != 0.0)
                Y = Yf[:, :wp]
                res = Y.astype(LD) @ Ldd.astype(LD) - np.eye(wp)
                note("inverses.Y", *entry_ratio(res, np.zeros_like(res), np.abs(Y) @ np.abs(Ldd)), f)
                dg = np.diag(Ldd)
                iv = X["INVD"][3 * F.e0 + k0:3 * F.e0 + k0 + wp]
                note("inverses.INVD", *entry_ratio(iv.astype(LD) * dg.astype(LD), np.ones(wp, dtype=LD), np.ones(wp)), f)
        bp = X["BND"][F.bnd_off:F.bnd_off + F.nb].astype(np.int64)
        xo, xb = x[3 * F.e0:3 * F.e0 + s3], x.reshape(n, 3)[bp].ravel()
        if "substitution" in stages and s3:
            L11, L21, y = L64[:s3], L64[s3:m], L64[m]
            lhs = L11.astype(LD).T @ xo.astype(LD) - (y.astype(LD) - L21.astype(LD).T @ xb.astype(LD))
            den = s3 * (np.abs(L11).T @ np.abs(xo) + np.abs(y) + np.abs(L21).T @ np.abs(xb))
            note("substitution.x", *entry_ratio(lhs, np.zeros_like(lhs), den), f)
        if "composed" in stages and s3:
            La = np.abs(L64[:m])
            tj = La.T @ np.r_[np.abs(xo), np.abs(xb)]
            rows = (3 * local_elim(X, F)[:, None] + np.arange(3)[None, :]).ravel()
            np.add.at(lltx, rows, La @ tj)
    for k, v in worst.items():
        if stage_of(k) in stages:
            R.put(k, *v)
    if "inverses" in stages:
        R.exact("inverses.Y_zero_right_of_the_diagonal", exact_ok["y_zero"])
    ev = X["ELIM_VERTEX"].astype(np.int64)
    if "update" in stages:
        P1 = np.asarray(X["P1"], dtype=np.float64)
        xs = x.reshape(n, 3)
        d = P1[ev].astype(LD) - (P0[ev].astype(LD) + xs.astype(LD))
        d[:, 2] -= 2 * LD(np.pi) * np.round(d[:, 2] / (2 * LD(np.pi)))
        ab = np.abs(P0[ev]) + np.abs(xs)
        ab[:, 2] = 2 * (np.abs(P0[ev, 2]) + np.abs(xs[:, 2]) + 2 * np.pi)
        R.put("update.poses", *entry_ratio(d, np.zeros_like(d), ab))
        R.exact("update.angles_normalised", bool(((P1[ev, 2] >= -np.pi) & (P1[ev, 2] <= np.pi)).all()))
        rest = np.ones(fixed.size, dtype=bool)
        rest[ev] = False
        R.exact("update.fixed_and_unused_poses_bit_equal", np.array_equal(P1[rest], P0[rest]) and not rest[~fixed & (np.bincount(np.r_[ei, ej], minlength=fixed.size) > 0)].any())
    if "composed" in stages or "history" in stages:
        hidx, free = npo.hessian_index(fixed)
        xh = np.zeros((free.size, 3))
        ok = hidx[ev].min() >= 0 if n else True
        if ok and free.size == n:
            xh[hidx[ev]] = x.reshape(n, 3)
            ref = kr.reference(P0, fixed, ei, ej, case["meas"], case["info"], case["phi"], xs=[xh])
            if "composed" in stages:
                lh = np.zeros((n, 3))
                lh[hidx[ev]] = lltx.reshape(n, 3)
                R.put("composed.residual", *entry_ratio(ref.b - ref.hx[0], np.zeros_like(ref.b), ref.b_abs + ref.hx_abs[0] + lh))
            if "history" in stages:
                h = X["hist"]
                R.put("history.chi2_0", kr.ratio(h[0], ref.chi2, ref.chi2_abs))
                R.put("history.robust_0", kr.ratio(h[1], ref.robust, ref.robust_abs))
                r1 = kr.reference(X["P1"], fixed, ei, ej, case["meas"], case["info"], case["phi"])
                R.put("history.chi2_1", kr.ratio(h[2], r1.chi2, r1.chi2_abs))
                R.put("history.robust_1", kr.ratio(h[3], r1.robust, r1.robust_abs))
        else:
            R.exact("composed.hessian_order", False)
    return R


def solution_hessian_order(case, X):
    """x in hessian order [n,3] from the exported step (for comparisons with other solvers)."""
    n = int(X["INFO"][0])
    hidx, free = npo.hessian_index(np.asarray(case["fixed"], dtype=bool))
    xh = np.zeros((n, 3))
    xh[hidx[X["ELIM_VERTEX"].astype(np.int64)]] = X["X"].reshape(n, 3)
    return xh


def report(name, R):
    """Every ratio of a case, one per line (a failing check prints them all)."""
    s = scaled(R)
    return "\n".join([f"{name}:"] + [f"  {k:55s} {R[k][0]:10.3g}  / C -> {s[k]:9.3g}  at {R[k][1]}" for k in R])
