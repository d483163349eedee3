"""Stage-by-stage reference for the single-launch direct path (CPU only, test infrastructure; sibling of mfront_reference.py).

What it checks.  One Gauss-Newton iteration of k_direct (sgo_direct.hip) from the arrays sgo_debug_direct_array exports after
optimize(1) of a debug run (include/sgo.h names them, SGO_DR_*), the poses P0 before the call and P1 after it -- stage by stage in
the order the kernel's phases run: edges, assembly, forward levels, dense elimination, back substitution, backward levels,
update.  Every stage takes its inputs from the exported arrays themselves (the Schur updates from the stored W and D, the
substitution from the stored x of the later positions), so an error is charged to the stage that made it.

A case (dict): P0 (V,3), fixed (V,), ei, ej, meas, info, phi as sgo_set_graph_se2's; optionally kind, delta (E,) as
sgo_set_robust_kernels' (robust_reference's numbering) for edges with kernels other than DCS.
X (dict): the SGO_DR_* arrays by name (capi.DIRECT_ARRAYS), "P1" (V,3) and "hist" = (chi2[0], robust[0], chi2[1], robust[1]).

Part A, model(): the same iteration in plain fp64 numpy from the HOST plan (capi.direct_plan_arrays): the edges' elements by
np_oracle's formulas (kernel_reference.edge_terms), assembly through VREC / VOVER / EDGE_TGT / MULTI, level-wise Schur updates
through TK / CTR, block LDL^T of the separator triangle, back substitution, update.  Pivot blocks are applied through a 3 x 3 LDL^T
solve, as the kernel does; it does not imitate the kernel's summation order (numpy sums a target's contributions as it likes) or
its reciprocal (it divides).  It is what the constants are taken from, and what the CPU tests mutate.

Part B, check(): every entry gets |got - ref| <= C_stage U abs, ref in np.longdouble, abs the same expression on magnitudes.
  structure    exact, also on the host plan alone: POS_VERTEX a permutation of the free poses with the separators last and every
               non-chain free-free pair touching one; every column's stored rows = the symbolic fill of the graph in this order
               (computed here by plain elimination on sets); no column's slots straddle a multiple of 64, padding and dummy slots
               where SLOT_RC says; the contributions of level l = exactly the pairs of rows of the level's columns, reading slots
               of that level and writing a higher level or the separator block; one task per target and level; VREC / VOVER list
               every incident (edge, side) once; every free-free edge reaches exactly one target directly or through MULTI / ENEXT
               with the transposed flag its endpoints' positions demand; ZERO_SLOTS = the stored blocks no edge reaches; the first
               m (m + 1) / 2 entries of DPAIR = the trailing pairs of every pivot.
  elements     ESCR's Hii, bi, Hjj, bj (and Hij for the edges of multi pairs) against the edge algebra in long double at P0, robust
               weight of every kind included; abs from kernel_reference.edge_terms' magnitudes.
  assembly     A_WD, A_XB and the diagonal blocks of A_SD = sums of ESCR's parts as exported, abs = sum |parts|; the off-diagonal
               blocks of A_WO and A_SD against the edge algebra (single edges) or ESCR's sum (multi pairs); zero slots and every
               entry of A_SD nothing reaches exactly 0.
  forward      every target of TK: WD, WO, F_SD = the assembled value - sum W_ik D_k^-1 W_jk^T and F_XB = A_XB - sum W_ik D_k^-1
               F_XB_k, sources the exported WD / WO / F_XB; abs = |assembled| + sum |W| Dinv |W^T| with Dinv = |L^-T| diag(1/p)
               |L^-1| of the block's own LDL^T (the componentwise bound of a solve through the factor).
  dense        block LDL^T backward error of F_SD against D_SD's panel and D_PINV's factors:
               |S0 - sum_p W_p D_p^-1 W_p^T|_ij <= C U ((bj + 1) sum |W| Dinv |W^T| + |S0|), the pivot's own term D_j read from
               D_PINV (D_SD keeps no pivot >= 1); D_BS against F_XB the same way.
  substitution separators D_i x_i = bs_i - sum_{j>i} W_ji^T x_j and sparse columns D_k x_k = F_XB_k - sum_i W_ik^T x_i, the x of
               later positions as exported: a residual bound, |D x - rhs| <= C U (|L| |P| |L^T| |x| + |rhs terms|).
  update       P1 = P0 (+) X through POS_VERTEX with overlay_reference's finish bound for the angle; fixed and unused vertices
               bit-equal.
  history      hist against the long-double chi2 and robust chi2 at P0 and at P1.
  composed     |b - H x|_i <= C U (abs(b) + abs(H x) + |L| |D| |L^T| |x|)_i with b, H x from the long-double edge algebra at P0 and
               the last term from the exported factor (L_ik = W_ik D_k^-1 of WD / WO, D_SD / D_PINV).

Constants.  mfront_reference.constant: C = 4 x the model's worst ratio over the cases of tests/direct_cases.py, rounded up to a
power of two (the margin: the kernel sums in another order and takes a Newton-refined reciprocal where the model divides).
tests/test_direct_reference.py measures MODEL on the CPU; MEASURED is what the MI355X gave (DESIGN.md section 5a has the table).
"""
from __future__ import annotations

import numpy as np

import kernel_reference as kr
import robust_reference as rr
from amg_reference import Result, entry_ratio
from kernel_reference import LD, U
from mfront_reference import constant
from oracle import np_oracle as npo
from overlay_reference import edge_blocks_ld

STAGES = ("elements", "assembly", "forward", "dense", "substitution", "update", "history", "composed")
BS = 10                                   # doubles of a stored block record
T_OFF, T_DIAG, T_DENSE = 0, 1, 2

# Worst error / (U abs) of model() over the cases of tests/direct_cases.py, and where (tests/test_direct_reference.py holds the
# model to them); the constants they give, 4 x rounded up to a power of two -- table in DESIGN.md section 5a.
#   stage         model   case                          C
#   elements      5.34    tasks_over_512                32
#   assembly      5.34    tasks_over_512                32    (a single edge's block against the edge algebra: the elements' figure)
#   forward       4.17    long_chain_2048               32
#   dense         1.66    weight_1e10                   8
#   substitution  2.39    xg_below                      16
#   update        0.9974  chain_130                     4
#   history       0.0688  dcs_switches_closures_off     0.5
#   composed      0.826   xg_below                      4
MODEL = dict(elements=5.34, assembly=5.34, forward=4.17, dense=1.66, substitution=2.39, update=0.9974, history=0.0688, composed=0.826)
MODEL_CASE = dict(elements="tasks_over_512", assembly="tasks_over_512", forward="long_chain_2048", dense="weight_1e10",
                  substitution="xg_below", update="chain_130", history="dcs_switches_closures_off", composed="xg_below")
# Worst error / (U abs) measured on the MI355X over tests/test_gpu_direct_reference.py (first and second iterations), and where.
# No stage came near its C: the kernel's summation order and its Newton-refined reciprocal cost what the model's own do.
MEASURED = dict(elements=5.611, assembly=5.611, forward=3.605, dense=0.8372, substitution=2.369, update=0.9989, history=0.1911, composed=0.5983)
MEASURED_CASE = dict(elements="wide_column", assembly="wide_column", forward="rows_scaled_1e6", dense="seps_49", substitution="long_chain_2048",
                     update="long_chain_2048", history="tasks_over_512", composed="xg_below")

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


def report(name, R):
    s = scaled(R)
    return "\n".join([f"{name}:"] + [f"  {k:55s} {R[k][0]:10.3g}  / C -> {s[k]:9.3g}  at {R[k][1]}" for k in R])


# ------------------------------------------------------------------ the tables
class Plan:
    """The plan tables in the terms the stages use."""

    def __init__(self, X):
        (self.n, self.nI, self.ns, self.NL, self.E, self.NB, self.tri, self.nzero, self.nmulti, self.ntask, self.ncontrib,
         self.lds_bytes, self.xb_global) = (int(v) for v in X["INFO"])
        self.pos_vertex = X["POS_VERTEX"].astype(np.int64)
        self.row = X["SLOT_RC"][:, 0].astype(np.int64)
        self.col = X["SLOT_RC"][:, 1].astype(np.int64)
        lm = X["LMETA"].astype(np.int64)
        self.lslot, self.ltask = lm[:self.NL + 1], lm[self.NL + 1:]
        tk = X["TK"].astype(np.int64).reshape(-1, 4)
        self.t_kind, self.t_idx, self.t_c0, self.t_c1 = tk[:, 0] >> 28, tk[:, 0] & 0x0fffffff, tk[:, 1], tk[:, 2]
        ctr = X["CTR"].astype(np.int64).reshape(-1, 4)
        self.c_a, self.c_b, self.c_k = ctr[:, 0], ctr[:, 1], ctr[:, 2]
        self.c_task = np.repeat(np.arange(self.ntask), self.t_c1 - self.t_c0)
        self.t_level = np.searchsorted(self.ltask, np.arange(self.ntask), side="right") - 1
        self.real = (self.row >= 0) & (self.col >= 0)          # stored blocks proper
        et = X["EDGE_TGT"].astype(np.int64)[:self.E]
        self.e_kind, self.e_tr, self.e_idx = et >> 30, (et >> 29) & 1, et & 0x1fffffff
        self.multi = X["MULTI"].astype(np.int64).reshape(-1, 2).copy()
        self.multi[:, 0] &= 0xffffffff                           # (the target word is unsigned: kind 2 sets bit 31)
        self.enext = X["ENEXT"].astype(np.int64)

    def incident(self, X, f):
        """The (edge << 1 | side) entries of position f, in the kernel's order."""
        vr = [int(v) for v in X["VREC"][f]]
        out = [v for v in vr[:3] if v >= 0]
        if vr[3] >= 0:
            out.append(vr[3])
        elif vr[3] <= -2:
            at = -2 - vr[3]
            cnt = int(X["VOVER"][at])
            out += [int(v) for v in X["VOVER"][at + 1:at + 1 + cnt]]
        return out

    def pair_edges(self, first):
        out, t = [], int(first)
        while t >= 0:
            out.append(t)
            t = int(self.enext[t >> 1])
        return out


def tri_index(i, j):
    return i * (i + 1) // 2 + j


def unpack_tri(sd, ns, dtype=np.float64):
    """The packed lower triangle as a dense [3 ns, 3 ns] matrix (upper part zero)."""
    m = 3 * ns
    S = np.zeros((m, m), dtype=dtype)
    S[np.tril_indices(m)] = sd
    return S


def pack_tri(S):
    return S[np.tril_indices(S.shape[0])]


def blocks9(W):
    """[m][10] records -> [m, 3, 3]."""
    return W[:, :9].reshape(-1, 3, 3)


# ------------------------------------------------------------------ 3 x 3 LDL^T, batched
def ldl3(D, recip=None):
    """f = (l10, l20, l21, 1/p0, 1/p1, 1/p2) of D = L diag(p) L^T for D [m, 3, 3] (the kernel's inv_sym3, with a division)."""
    one = D.dtype.type(1)
    r = (lambda v: one / v) if recip is None else recip
    d00, d01, d02, d11, d12, d22 = D[:, 0, 0], D[:, 0, 1], D[:, 0, 2], D[:, 1, 1], D[:, 1, 2], D[:, 2, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        r0 = r(d00)
        l10, l20 = d01 * r0, d02 * r0
        p1 = d11 - l10 * d01
        r1 = r(p1)
        u21 = d12 - l20 * d01
        l21 = u21 * r1
        p2 = d22 - l20 * d02 - l21 * u21
        r2 = r(p2)
    return np.stack([l10, l20, l21, r0, r1, r2], axis=1)


def solve3(f, Y):
    """X = D^-1 Y through the factors, Y [m, 3] (the kernel's solve3)."""
    z1 = Y[:, 1] - f[:, 0] * Y[:, 0]
    z2 = Y[:, 2] - f[:, 1] * Y[:, 0] - f[:, 2] * z1
    x2 = z2 * f[:, 5]
    x1 = z1 * f[:, 4] - f[:, 2] * x2
    x0 = Y[:, 0] * f[:, 3] - f[:, 0] * x1 - f[:, 1] * x2
    return np.stack([x0, x1, x2], axis=1)


def mul_sym(W, f):
    """T = W D^-1, W [m, 3, 3]: every row of W solved through the factors."""
    return np.stack([solve3(f, W[:, r, :]) for r in range(3)], axis=1)


def unit_lower(f):
    m = f.shape[0]
    L = np.zeros((m, 3, 3), dtype=f.dtype)
    L[:, 0, 0] = L[:, 1, 1] = L[:, 2, 2] = 1
    L[:, 1, 0], L[:, 2, 0], L[:, 2, 1] = f[:, 0], f[:, 1], f[:, 2]
    return L


def dinv_exact(f):
    """D^-1 = L^-T diag(r) L^-1 from the factors, in their dtype."""
    Li = np.zeros_like(unit_lower(f))
    Li[:, 0, 0] = Li[:, 1, 1] = Li[:, 2, 2] = 1
    Li[:, 1, 0] = -f[:, 0]
    Li[:, 2, 1] = -f[:, 2]
    Li[:, 2, 0] = f[:, 0] * f[:, 2] - f[:, 1]
    return np.swapaxes(Li, 1, 2) @ (f[:, 3:6, None] * Li)


def dinv_abs(f):
    """|L^-T| diag(|r|) |L^-1|: the componentwise bound of a solve through the factors."""
    f = np.abs(np.asarray(f, dtype=np.float64))
    Li = np.zeros((f.shape[0], 3, 3))
    Li[:, 0, 0] = Li[:, 1, 1] = Li[:, 2, 2] = 1
    Li[:, 1, 0] = f[:, 0]
    Li[:, 2, 1] = f[:, 2]
    Li[:, 2, 0] = f[:, 0] * f[:, 2] + f[:, 1]
    return np.swapaxes(Li, 1, 2) @ (f[:, 3:6, None] * Li)


def d_of(f):
    """D = L diag(1 / r) L^T from the factors, and |L| |P| |L^T|."""
    L = unit_lower(f)
    p = 1 / f[:, 3:6]
    D = L @ (p[:, :, None] * np.swapaxes(L, 1, 2))
    La = np.abs(L).astype(np.float64)
    Da = La @ (np.abs(p).astype(np.float64)[:, :, None] * np.swapaxes(La, 1, 2))
    return D, Da


# ------------------------------------------------------------------ the edges
_TRI = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def _w_ld(kind, e2, d):
    """(rho0, rho1) in long double for the kinds the cases use."""
    e2 = e2.astype(LD)
    d = np.asarray(d, dtype=np.float64).astype(LD)
    r0, w = e2.copy(), np.ones_like(e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        d2, s = d * d, np.sqrt(e2)
        for k in np.unique(kind):
            m = kind == k
            if k == rr.NONE:
                continue
            if k == rr.DCS:
                sc = 2 * d / (d + e2)
                a0, a1 = np.where(sc >= 1, e2, sc * sc * e2), np.where(sc >= 1, LD(1), sc * sc)
            elif k == rr.HUBER:
                a0, a1 = np.where(e2 <= d2, e2, 2 * s * d - d2), np.where(e2 <= d2, LD(1), d / s)
            elif k == rr.PSEUDO_HUBER:
                a = np.sqrt(1 + e2 / d2)
                a0, a1 = 2 * d2 * (a - 1), 1 / a
            elif k == rr.CAUCHY:
                a = 1 + e2 / d2
                a0, a1 = d2 * np.log(a), 1 / a
            elif k == rr.GEMAN_MCCLURE:
                a = 1 / (1 + e2)
                a0, a1 = e2 * a, a * a
            elif k == rr.WELSCH:
                a = np.exp(-e2 / d2)
                a0, a1 = d2 * (1 - a), a
            else:
                raise ValueError(f"kind {k}: not among the kinds of the direct cases")
            r0[m], w[m] = a0[m], a1[m]
    return r0, w


def kinds_of(case):
    """(kind, delta) per edge: the case's own, or DCS with phi (phi < 0: none)."""
    phi = np.asarray(case["phi"], dtype=np.float64)
    if case.get("kind") is not None:
        return np.asarray(case["kind"]), np.asarray(case["delta"], dtype=np.float64)
    return np.where(phi >= 0, rr.DCS, rr.NONE), np.where(phi >= 0, phi, 1.0)


def edge_parts(case, P=None):
    """Per edge, at the poses P: the fp64 terms (np_oracle's formulas with the robust weight), their long-double references and
    magnitudes.  The weight: w = rho1(e2), its magnitude wbar = w + |dw / de2| abs(e2) (kernel_reference's DCS term, for every
    kind, the derivative by a central difference)."""
    P = np.asarray(case["P0"] if P is None else P, dtype=np.float64)
    ei, ej = np.asarray(case["ei"], dtype=np.int64), np.asarray(case["ej"], dtype=np.int64)
    E = ei.size
    none = np.full(E, -1.0)
    t = kr.edge_terms(P[ei], P[ej], case["meas"], case["info"], none)
    kind, delta = kinds_of(case)
    e2 = t["e2"].astype(np.float64)
    rho0, w = rr.rho_mixed(kind, e2, delta)
    r0l, wl = _w_ld(kind, t["e2"], delta)
    h = 1e-6 * np.maximum(e2, 1e-300)
    dw = np.abs(rr.rho_mixed(kind, e2 + h, delta)[1] - rr.rho_mixed(kind, np.maximum(e2 - h, 0.0), delta)[1]) / (2 * h)
    wbar = w + dw * t["e2_abs"]
    bi, bj, Hii, Hjj, Hij = edge_blocks_ld(P, ei, ej, case["meas"], case["info"], none)
    out = dict(E=E, e2=t["e2"], e2_abs=t["e2_abs"], rho0=rho0, rho0_ld=r0l, w=w, wbar=wbar)
    for k, ref in (("bi", bi), ("bj", bj), ("Hii", Hii), ("Hjj", Hjj), ("Hij", Hij)):
        sh = (E,) + (1,) * (ref.ndim - 1)
        out[k] = t[k] * w.reshape(sh)
        out[k + "_ld"] = ref * wl.reshape(sh)
        out[k + "_abs"] = t[k + "_abs"] * wbar.reshape(sh)
    return out


def escr_of(t, suffix="", dtype=np.float64):
    """[27][E] in ESCR's layout from edge_parts' terms."""
    E = t["E"]
    o = np.zeros((27, E), dtype=dtype)
    for z, (a, b) in enumerate(_TRI):
        o[z], o[9 + z] = t["Hii" + suffix][:, a, b], t["Hjj" + suffix][:, a, b]
    o[6:9], o[15:18] = t["bi" + suffix].T, t["bj" + suffix].T
    o[18:27] = t["Hij" + suffix].reshape(E, 9).T
    return o


def _sym6(v):
    """[..., 6] upper triangle by rows -> [..., 3, 3]."""
    M = np.zeros(v.shape[:-1] + (3, 3), dtype=v.dtype)
    for z, (a, b) in enumerate(_TRI):
        M[..., a, b] = M[..., b, a] = v[..., z]
    return M


def multi_edges(pl):
    """Edges of multi pairs (their Hij is in ESCR)."""
    return np.flatnonzero(pl.e_kind == 3)


def assemble(pl, X, escr, dtype, mut=None, want_abs=False):
    """(Wd [nI,3,3], Wo [NB,3,3], S [3ns,3ns] lower, xb [n,3]) from ESCR-layout terms `escr` (single edges' Hij included at rows
    18 .. 27) through the plan's assembly lists; with want_abs the same on magnitudes (escr is then |terms|)."""
    n, nI, ns = pl.n, pl.nI, pl.ns
    Wd = np.zeros((nI, 3, 3), dtype=dtype)
    Wo = np.zeros((pl.NB, 3, 3), dtype=dtype)
    S = np.zeros((3 * ns, 3 * ns), dtype=dtype)
    xb = np.zeros((n, 3), dtype=dtype)
    skipped = False
    for f in range(n):
        d = np.zeros(9, dtype=dtype)
        inc = pl.incident(X, f)
        for q, tq in enumerate(inc):
            if mut == "overflow_entry_skipped" and not skipped and len(inc) > 4 and q == len(inc) - 1:
                skipped = True
                continue
            d += escr[9 * (tq & 1):9 * (tq & 1) + 9, tq >> 1]
        xb[f] = d[6:9]
        M = _sym6(d[:6])
        if f < nI:
            Wd[f] = M
        else:
            r = 3 * (f - nI)
            S[r:r + 3, r:r + 3] = np.tril(M)

    def store(kind, tr, idx, H):
        H = H.T if tr else H
        if kind == 1:
            Wo[idx] = H
        elif kind == 2:
            si, sj = idx >> 12, idx & 4095
            S[3 * si:3 * si + 3, 3 * sj:3 * sj + 3] = H
    flipped = dict(slot=False, sep=False)
    for e in range(pl.E):
        k = int(pl.e_kind[e])
        if k in (1, 2):
            tr = int(pl.e_tr[e])
            if mut == "flag_flipped_stored" and k == 1 and not flipped["slot"]:
                tr, flipped["slot"] = 1 - tr, True
            if mut == "flag_flipped_separator" and k == 2 and not flipped["sep"]:
                tr, flipped["sep"] = 1 - tr, True
            store(k, tr, int(pl.e_idx[e]), escr[18:27, e].reshape(3, 3))
    for q, (tgt, first) in enumerate(pl.multi):
        b = np.zeros((3, 3), dtype=dtype)
        lst = pl.pair_edges(first)
        if mut == "multi_edge_skipped" and q == 0:
            lst = lst[:-1]
        for tq in lst:
            H = escr[18:27, tq >> 1].reshape(3, 3)
            b += (np.abs(H.T) if want_abs else H.T) if tq & 1 else H
        store(int(tgt) >> 30, 0, int(tgt) & 0x1fffffff, b)
    return Wd, Wo, S, xb


def schur(pl, Wo, f, xb, sel, dtype, apply=None):
    """The contributions `sel` (indices into CTR): (prod [m,3,3] = W_a D_k^-1 W_b^T, rhs [m,3] = W_a D_k^-1 xb_k)."""
    a, b, k = pl.c_a[sel], pl.c_b[sel], pl.c_k[sel]
    if apply is None:
        T = mul_sym(Wo[a].astype(dtype), f[k].astype(dtype))
    else:
        T = Wo[a].astype(dtype) @ apply[k]
    return T @ np.swapaxes(Wo[b].astype(dtype), 1, 2), np.einsum("nij,nj->ni", T, xb[k].astype(dtype))


def scatter_tasks(pl, sel, prod, rhs, Wd, Wo, S, xb, sign=-1):
    """Add sign x the contributions to their tasks' targets (the diagonal targets own the right-hand side as well)."""
    task = pl.c_task[sel]
    kind, idx = pl.t_kind[task], pl.t_idx[task]
    m = kind == T_OFF
    np.add.at(Wo, idx[m], sign * prod[m])
    m = kind == T_DIAG
    np.add.at(Wd, idx[m], sign * prod[m])
    np.add.at(xb, idx[m], sign * rhs[m])
    for q in np.flatnonzero(kind == T_DENSE):
        si, sj = int(idx[q]) >> 12, int(idx[q]) & 4095
        if si == sj:
            S[3 * si:3 * si + 3, 3 * si:3 * si + 3] += sign * np.tril(prod[q])
            xb[pl.nI + si] += sign * rhs[q]
        else:
            S[3 * si:3 * si + 3, 3 * sj:3 * sj + 3] += sign * prod[q]


# ------------------------------------------------------------------ part A: the fp64 model
def model(case, plan, mut=None, stale=None):
    """One Gauss-Newton iteration in plain fp64 from the host plan's tables: X as the device exports it (+ P1, hist).
    mut: one of the CPU tests' mutations.  stale: what an earlier iteration left in the separator triangle (the mutation "the
    clear after the back substitution is missing"): added to the triangle before the assembly writes into it."""
    X = dict(plan)
    pl = Plan(X)
    n, nI, ns, NL = pl.n, pl.nI, pl.ns, pl.NL
    P0 = np.asarray(case["P0"], dtype=np.float64)
    t = edge_parts(case)
    escr = escr_of(t)
    Wd, Wo, S, xb = assemble(pl, X, escr, np.float64, mut)
    if stale is not None:
        # the assembly STORES the blocks edges reach and ADDS nothing: a stale entry survives where no edge writes
        reached = assemble(pl, X, np.abs(escr) + 1.0, np.float64, None, want_abs=True)[2] != 0
        S = np.where(reached, S, S + stale)
    if mut == "zero_slot_not_cleared" and pl.nzero:
        Wo[int(X["ZERO_SLOTS"][0])] = 1e-3 * np.abs(Wd).max()
    esc = escr.copy()
    esc[18:27, pl.e_kind != 3] = 0.0                    # (single edges' Hij goes straight to its target)
    Wd10, Wo10 = np.zeros((nI, BS)), np.zeros((pl.NB, BS))
    X.update(ESCR=esc.ravel(), A_SD=pack_tri(S), A_XB=xb.ravel().copy())
    Wd10[:, :9], Wo10[:, :9] = Wd.reshape(nI, 9), Wo.reshape(-1, 9)
    X.update(A_WD=Wd10.copy(), A_WO=Wo10.copy())
    sel_drop = sel_dup = None
    if mut in ("contribution_dropped", "contribution_doubled") and pl.ncontrib:
        cnt = pl.t_c1 - pl.t_c0                         # in a task of several contributions, the last one
        tq = int(np.argmax(cnt >= 2)) if (cnt >= 2).any() else 0
        which = int(pl.t_c1[tq]) - 1
        sel_drop, sel_dup = (which, None) if mut == "contribution_dropped" else (None, which)
    for l in range(NL):
        sel = np.flatnonzero((pl.t_level[pl.c_task] == l))
        if sel_drop is not None:
            sel = sel[sel != sel_drop]
        if sel_dup is not None and sel_dup in sel:
            sel = np.r_[sel, sel_dup]
        if sel.size == 0:
            continue
        f = ldl3(Wd)
        if mut == "explicit_inverse":
            prod, rhs = schur(pl, Wo, None, xb, sel, np.float64, apply=np.linalg.inv(Wd))
        else:
            prod, rhs = schur(pl, Wo, f, xb, sel, np.float64)
        scatter_tasks(pl, sel, prod, rhs, Wd, Wo, S, xb)
    Wd10[:, :9], Wo10[:, :9] = Wd.reshape(nI, 9), Wo.reshape(-1, 9)
    X.update(WD=Wd10, WO=Wo10, F_SD=pack_tri(S), F_XB=xb.ravel().copy())
    # ---- separators: right-looking block LDL^T, W form (the panel stays), the next pivot block kept as its factor only
    pinv = np.zeros((ns, 6))
    bs = xb[nI:].copy()
    piv = S[0:3, 0:3].copy() if ns else None
    for p in range(ns):
        Dp = (piv + np.tril(piv, -1).T)[None]
        fp = ldl3(Dp)
        if mut == "explicit_inverse":
            ap = np.linalg.inv(Dp)
        pinv[p] = fp[0]
        if p + 1 == ns:
            break
        W = S[3 * (p + 1):, 3 * p:3 * p + 3].reshape(-1, 3, 3)                 # W_ip, i > p
        T = (W @ ap) if mut == "explicit_inverse" else mul_sym(W, np.repeat(fp, W.shape[0], axis=0))
        Tf = T.reshape(-1, 3)
        upd = Tf @ S[3 * (p + 1):, 3 * p:3 * p + 3].T
        nxt = S[3 * (p + 1):3 * (p + 2), 3 * (p + 1):3 * (p + 2)].copy()
        S[3 * (p + 1):, 3 * (p + 1):] -= np.tril(upd)
        piv = nxt - np.tril(upd[:3, :3])
        S[3 * (p + 1):3 * (p + 2), 3 * (p + 1):3 * (p + 2)] = nxt                # (the block itself is not stored back)
        bs[p + 1:] -= (Tf @ bs[p]).reshape(-1, 3)
    if mut == "pivot_factors_wrong_order" and ns:
        pinv_used = pinv[:, [0, 1, 2, 5, 4, 3]]
    else:
        pinv_used = pinv
    X.update(D_SD=pack_tri(S), D_PINV=pinv.copy(), D_BS=bs.ravel().copy())
    # ---- back substitution of the separators, then the sparse levels backward
    x = xb.copy()
    b = bs.copy()
    for i in range(ns - 1, -1, -1):
        xi = solve3(pinv_used[i:i + 1], b[i:i + 1])[0]
        x[nI + i] = xi
        if i:
            W = S[3 * i:3 * i + 3, :3 * i]                                       # W_ij, j < i, as [3, 3 i]
            b[:i] -= (W.T @ xi).reshape(-1, 3)
    f = ldl3(Wd) if nI else None
    for l in range(NL - 1, -1, -1):
        s0, s1 = int(pl.lslot[l]), int(pl.lslot[l + 1])
        sl = np.arange(s0, s1)
        cols = np.unique(pl.col[sl][pl.col[sl] >= 0])
        acc = np.zeros((nI, 3))
        rl = sl[pl.real[sl]]
        np.add.at(acc, pl.col[rl], np.einsum("nij,ni->nj", Wo[rl], x[pl.row[rl]]))
        x[cols] = solve3(f[cols], x[cols] - acc[cols])
    X["X"] = x.ravel().copy()
    pv = pl.pos_vertex
    if mut == "permutation_off_by_one" and n > 1:
        pv = np.roll(pv, 1)
    P1 = P0.copy()
    P1[pv] = P0[pv] + x
    P1[pv, 2] = npo.normalize_theta(P1[pv, 2])
    t1 = edge_parts(case, P1)
    X.update(P1=P1, hist=(float(np.sum(t["e2"].astype(np.float64))), float(np.sum(t["rho0"])),
                          float(np.sum(t1["e2"].astype(np.float64))), float(np.sum(t1["rho0"]))))
    return X


# ------------------------------------------------------------------ part B: structure (exact)
def symbolic_fill(n, nI, pairs):
    """Rows of every sparse column: plain elimination on sets, positions 0 .. nI in order (independent of the plan's tree)."""
    adj = [set() for _ in range(n)]
    for a, b in pairs:
        adj[a].add(b)
        adj[b].add(a)
    cols = []
    for k in range(nI):
        rows = sorted(v for v in adj[k] if v > k)
        cols.append(rows)
        for q, i in enumerate(rows):
            for j in rows[:q]:
                adj[i].add(j)
                adj[j].add(i)
    return cols


def structure(case, X):
    R = Result()
    pl = Plan(X)
    n, nI, ns, NL, E, NB = pl.n, pl.nI, pl.ns, pl.NL, pl.E, pl.NB
    fixed = np.asarray(case["fixed"], dtype=bool)
    ei, ej = np.asarray(case["ei"], dtype=np.int64), np.asarray(case["ej"], dtype=np.int64)
    V = fixed.size
    deg = np.bincount(np.r_[ei, ej], minlength=V)
    free = np.flatnonzero(~fixed & (deg > 0))
    R.exact("structure.sizes", E == ei.size and n == free.size and n == nI + ns and pl.tri == 3 * ns * (3 * ns + 1) // 2 and
            X["POS_VERTEX"].size == n and X["VREC"].shape[0] == n and X["SLOT_RC"].shape[0] == NB and X["CTR"].shape[0] == pl.ncontrib and
            X["TK"].shape[0] == pl.ntask and X["ZERO_SLOTS"].size == pl.nzero and pl.multi.shape[0] == pl.nmulti and
            X["DPAIR"].size == ns * (ns + 1) // 2 and X["LMETA"].size == 2 * (NL + 1))
    if R.worst() > 0:
        return R
    pv = pl.pos_vertex
    R.exact("structure.order_is_a_permutation_of_the_free_poses", np.array_equal(np.sort(pv), free))
    if R.worst() > 0:
        return R
    pos = np.full(V, -1, dtype=np.int64)
    pos[pv] = np.arange(n)
    fidx = np.full(V, -1, dtype=np.int64)
    fidx[free] = np.arange(n)
    pa, pb = pos[ei], pos[ej]
    ff = (pa >= 0) & (pb >= 0)
    chain = np.abs(fidx[ei] - fidx[ej]) == 1
    R.exact("structure.every_non_chain_pair_has_a_separator_endpoint", bool((np.maximum(pa, pb)[ff & ~chain] >= nI).all()))
    R.exact("structure.separators_ascend_with_the_free_index", bool((np.diff(fidx[pv[nI:]]) > 0).all()))
    # ---- columns: symbolic fill, slots, levels
    pairs = set((int(min(a, b)), int(max(a, b))) for a, b in zip(pa[ff], pb[ff]))
    fill = symbolic_fill(n, nI, pairs)
    ok = pl.lslot[0] == 0 and pl.lslot[-1] == NB and bool((pl.lslot % 64 == 0).all()) and pl.ltask[0] == 0 and pl.ltask[-1] == pl.ntask
    ok = ok and bool((np.diff(pl.lslot) >= 0).all()) and bool((np.diff(pl.ltask) >= 0).all())
    colbase = np.full(max(nI, 1), -1, dtype=np.int64)
    collevel = np.full(max(nI, 1), -1, dtype=np.int64)
    fill_ok = straddle_ok = pad_ok = True
    s = 0
    slot_level = np.searchsorted(pl.lslot, np.arange(NB), side="right") - 1
    while s < NB:
        c = int(pl.col[s])
        if c < 0:
            pad_ok = pad_ok and pl.row[s] == -1
            s += 1
            continue
        if not (0 <= c < nI) or colbase[c] >= 0:
            fill_ok = False
            break
        want = fill[c]
        ln = max(1, len(want))
        got = pl.row[s:s + ln]
        same_col = bool((pl.col[s:s + ln] == c).all()) and (s + ln == NB or pl.col[s + ln] != c)
        fill_ok = fill_ok and same_col and (list(got) == want if want else list(got) == [-1])
        straddle_ok = straddle_ok and (s // 64 == (s + ln - 1) // 64) and slot_level[s] == slot_level[s + ln - 1]
        colbase[c], collevel[c] = s, slot_level[s]
        s += ln
    fill_ok = fill_ok and bool((colbase[:nI] >= 0).all())
    R.exact("structure.level_ranges", bool(ok))
    R.exact("structure.columns_hold_the_symbolic_fill", bool(fill_ok))
    R.exact("structure.no_column_straddles_64_slots", bool(straddle_ok))
    R.exact("structure.padding_slots_have_no_row", bool(pad_ok))
    if R.worst() > 0:
        return R
    # a column's level is above every column it receives from (its children in the elimination order)
    lev_ok = True
    for k in range(nI):
        for i in fill[k]:
            if i < nI:
                lev_ok = lev_ok and collevel[i] > collevel[k]
    R.exact("structure.targets_lie_in_higher_levels", bool(lev_ok))
    # ---- contributions: exactly the pairs of rows of every column, at the column's level, one task per target and level
    want = {}
    for k in range(nI):
        rows = fill[k]
        for x_, i in enumerate(rows):
            for y_ in range(x_ + 1):
                j = rows[y_]
                if j >= nI:
                    tg = (T_DENSE, (i - nI) << 12 | (j - nI))
                elif i == j:
                    tg = (T_DIAG, j)
                else:
                    tg = (T_OFF, int(colbase[j]) + fill[j].index(i))
                want.setdefault((int(collevel[k]), tg), []).append((int(colbase[k]) + x_, int(colbase[k]) + y_, k))
    got, dup = {}, False
    for tq in range(pl.ntask):
        key = (int(pl.t_level[tq]), (int(pl.t_kind[tq]), int(pl.t_idx[tq])))
        dup = dup or key in got or pl.t_c1[tq] <= pl.t_c0[tq]
        got[key] = [(int(pl.c_a[c]), int(pl.c_b[c]), int(pl.c_k[c])) for c in range(int(pl.t_c0[tq]), int(pl.t_c1[tq]))]
    R.exact("structure.one_task_per_target_and_level", not dup)
    R.exact("structure.contributions_are_the_pairs_of_every_column", set(got) == set(want) and
            all(sorted(got[k]) == sorted(want[k]) for k in want))
    tiled = pl.ncontrib == 0 or (np.array_equal(np.sort(np.concatenate([np.arange(a, b) for a, b in zip(pl.t_c0, pl.t_c1)])),
                                                np.arange(pl.ncontrib)))
    R.exact("structure.tasks_tile_the_contribution_list", bool(tiled))
    # ---- incident lists
    wanti = [[] for _ in range(n)]
    for e in range(E):
        if pa[e] >= 0:
            wanti[pa[e]].append(e << 1)
        if pb[e] >= 0:
            wanti[pb[e]].append(e << 1 | 1)
    R.exact("structure.incident_lists_hold_every_edge_side_once", all(sorted(pl.incident(X, f)) == wanti[f] for f in range(n)))
    inl_ok = all((len(wanti[f]) <= 4) == (int(X["VREC"][f][3]) > -2) for f in range(n))
    R.exact("structure.four_incident_edges_are_inline_five_overflow", bool(inl_ok))
    # ---- off-diagonal targets
    def target_of(e):
        row, col = max(pa[e], pb[e]), min(pa[e], pb[e])
        tr = 0 if row == pa[e] else 1
        if col < nI:
            return (1, int(colbase[col]) + fill[col].index(int(row))), tr
        return (2, int(row - nI) << 12 | int(col - nI)), tr
    reach, ok = {}, True
    for e in range(E):
        k = int(pl.e_kind[e])
        if not ff[e]:
            ok = ok and k == 0
            continue
        tg, tr = target_of(e)
        if k == 3:
            continue
        ok = ok and (k, int(pl.e_idx[e])) == tg and int(pl.e_tr[e]) == tr
        reach.setdefault(tg, []).append(e)
    seen_multi = set()
    for tgt, first in pl.multi:
        tg = (int(tgt) >> 30, int(tgt) & 0x1fffffff)
        ok = ok and not (int(tgt) >> 29) & 1 and tg not in reach
        for tq in pl.pair_edges(first):
            e = tq >> 1
            ok = ok and pl.e_kind[e] == 3 and e not in seen_multi and target_of(e) == (tg, tq & 1)
            seen_multi.add(e)
            reach.setdefault(tg, []).append(e)
    ok = ok and seen_multi == set(int(e) for e in multi_edges(pl))
    ok = ok and all((len(v) == 1) == (pl.e_kind[v[0]] != 3) for v in reach.values())
    ok = ok and sum(len(v) for v in reach.values()) == int(ff.sum())
    R.exact("structure.every_free_free_edge_reaches_one_target_with_its_flag", bool(ok))
    reached_slots = set(idx for (k, idx) in reach if k == 1)
    R.exact("structure.zero_slots_are_the_blocks_no_edge_reaches",
            sorted(int(v) for v in X["ZERO_SLOTS"]) == [q for q in np.flatnonzero(pl.real) if q not in reached_slots])
    dp = X["DPAIR"].astype(np.int64)
    ok = True
    for p in range(ns):
        m = ns - 1 - p
        head = set((int(v) >> 8, int(v) & 255) for v in dp[:m * (m + 1) // 2])
        ok = ok and head == set((bi, bj) for bj in range(p + 1, ns) for bi in range(bj, ns))
    R.exact("structure.dpair_prefixes_are_the_trailing_pairs_of_every_pivot", bool(ok) and len(set(dp)) == dp.size)
    return R


# ------------------------------------------------------------------ part B: the stage checks
def check(case, X, stages=STAGES):
    """Raw worst ratios {"stage.name": (error / (U abs), where)}: exact checks give 0 or inf."""
    R = structure(case, X)
    if R.worst() > 0:
        return R                                      # the later stages read the tables
    pl = Plan(X)
    n, nI, ns, NL, E = pl.n, pl.nI, pl.ns, pl.NL, pl.E
    P0 = np.asarray(case["P0"], dtype=np.float64)
    fixed = np.asarray(case["fixed"], dtype=bool)
    ei, ej = np.asarray(case["ei"], dtype=np.int64), np.asarray(case["ej"], dtype=np.int64)
    escr = X["ESCR"].reshape(27, E)
    t = edge_parts(case)
    ref, mag = escr_of(t, "_ld", LD), escr_of(t, "_abs")
    me = multi_edges(pl)
    if "elements" in stages:
        R.put("elements.Hii_bi_Hjj_bj", *entry_ratio(escr[:18], ref[:18], mag[:18]))
        R.put("elements.Hij_of_multi_pairs", *entry_ratio(escr[18:, me], ref[18:, me], mag[18:, me]))
    A_WD, A_WO, WD, WO = blocks9(X["A_WD"]), blocks9(X["A_WO"]), blocks9(X["WD"]), blocks9(X["WO"])
    A_S, F_S, D_S = (unpack_tri(X[k], ns) for k in ("A_SD", "F_SD", "D_SD"))
    A_XB, F_XB, XS = X["A_XB"].reshape(n, 3), X["F_XB"].reshape(n, 3), X["X"].reshape(n, 3)
    dblk = [(slice(3 * i, 3 * i + 3),) * 2 for i in range(ns)]
    diag_mask = np.zeros((3 * ns, 3 * ns), dtype=bool)
    for sl in dblk:
        diag_mask[sl] = True
    low = np.tril(np.ones((3 * ns, 3 * ns), dtype=bool))
    if "assembly" in stages:
        # sums of ESCR's parts as exported; the off-diagonal blocks of single edges from the edge algebra itself
        src, srca = escr.astype(LD), np.abs(escr)
        single = pl.e_kind != 3
        src[18:, single], srca[18:, single] = ref[18:, single], mag[18:, single]
        Wd, Wo, S, xb = assemble(pl, X, src, LD)
        Wda, Woa, Sa, xba = assemble(pl, X, srca, np.float64, want_abs=True)
        R.put("assembly.A_WD", *entry_ratio(A_WD, Wd, Wda))
        R.put("assembly.A_XB", *entry_ratio(A_XB, xb, xba))
        R.put("assembly.A_SD_diagonal", *entry_ratio(np.where(diag_mask, A_S, 0.0), np.where(diag_mask, S, 0), np.where(diag_mask, Sa, 0.0)))
        R.put("assembly.A_SD_off_diagonal", *entry_ratio(np.where(~diag_mask, A_S, 0.0), np.where(~diag_mask, S, 0), np.where(~diag_mask, Sa, 0.0)))
        R.put("assembly.A_WO", *entry_ratio(A_WO[pl.real], Wo[pl.real], Woa[pl.real]))
        R.exact("assembly.zero_slots_are_zero", not np.any(A_WO[X["ZERO_SLOTS"].astype(np.int64)] != 0.0))
        R.exact("assembly.unreached_entries_of_A_SD_are_zero", not np.any(A_S[(Sa == 0.0) & low] != 0.0))
    fD = ldl3(WD.astype(LD)) if nI else np.zeros((0, 6), dtype=LD)
    fDa = dinv_abs(fD)
    if "forward" in stages and pl.ncontrib:
        sel = np.arange(pl.ncontrib)
        Di = dinv_exact(fD)
        prod, rhs = schur(pl, WO, None, F_XB, sel, LD, apply=Di)
        Wa, Wb = np.abs(WO[pl.c_a]), np.abs(WO[pl.c_b])
        Ta = Wa @ fDa[pl.c_k]
        proda, rhsa = Ta @ np.swapaxes(Wb, 1, 2), np.einsum("nij,nj->ni", Ta, np.abs(F_XB[pl.c_k]))
        Wd, Wo, S, xb = A_WD.astype(LD), A_WO.astype(LD), A_S.astype(LD), A_XB.astype(LD)
        Wda, Woa, Sa, xba = np.abs(A_WD), np.abs(A_WO), np.abs(A_S), np.abs(A_XB)
        scatter_tasks(pl, sel, prod, rhs, Wd, Wo, S, xb)
        scatter_tasks(pl, sel, proda, rhsa, Wda, Woa, Sa, xba, sign=1)
        R.put("forward.WD", *entry_ratio(WD, Wd, Wda))
        R.put("forward.WO", *entry_ratio(WO[pl.real], Wo[pl.real], Woa[pl.real]))
        R.put("forward.F_SD", *entry_ratio(F_S, S, Sa))
        R.put("forward.F_XB", *entry_ratio(F_XB, xb, xba))
    elif "forward" in stages:
        R.exact("forward.nothing_to_update", np.array_equal(WD, A_WD) and np.array_equal(F_S, A_S) and np.array_equal(F_XB, A_XB))
    fP = X["D_PINV"].reshape(ns, 6).astype(LD)
    if ns:
        Dp, Dpa = d_of(fP)
        Pi, Pia = dinv_exact(fP), dinv_abs(fP)
    bs = X["D_BS"].reshape(ns, 3)
    if "dense" in stages and ns:
        # W_ip = D_S block (i, p), i > p; the pivot D_p from its factors
        Wl = np.where(diag_mask, 0.0, D_S)
        err = np.zeros((3 * ns, 3 * ns), dtype=LD)
        den = np.zeros((3 * ns, 3 * ns))
        rb, rba = F_XB[nI:].astype(LD).copy(), np.abs(F_XB[nI:]).copy()
        S0 = F_S.astype(LD)
        acc = np.zeros((3 * ns, 3 * ns), dtype=LD)
        acca = np.zeros((3 * ns, 3 * ns))
        for j in range(ns):
            c = slice(3 * j, 3 * j + 3)
            # column j of S0 - sum_{p<j} W_p Dp^-1 W_jp^T
            stage = np.zeros((3 * ns, 3), dtype=LD)
            stage[3 * j:3 * j + 3] = np.tril(Dp[j])
            stage[3 * j + 3:] = Wl[3 * j + 3:, c]
            err[3 * j:, c] = S0[3 * j:, c] - acc[3 * j:, c] - stage[3 * j:]
            den[3 * j:, c] = (j + 1) * (acca[3 * j:, c] + np.abs(stage[3 * j:]).astype(np.float64)) + np.abs(F_S[3 * j:, c])
            if j + 1 < ns:
                Wj = Wl[3 * j + 3:, c].astype(LD)                     # [(ns-j-1) 3, 3]
                T = Wj @ Pi[j]
                Ta = np.abs(Wl[3 * j + 3:, c]) @ Pia[j]
                acc[3 * j + 3:, 3 * j + 3:] += T @ Wj.T
                acca[3 * j + 3:, 3 * j + 3:] += Ta @ np.abs(Wl[3 * j + 3:, c]).T
                rb[j + 1:] -= (T @ bs[j].astype(LD)).reshape(-1, 3)
                rba[j + 1:] += (Ta @ np.abs(bs[j])).reshape(-1, 3)
        err, den = np.where(low, err, 0), np.where(low, den, 0.0)
        R.put("dense.S0_minus_W_Dinv_Wt", *entry_ratio(err, np.zeros_like(err), den))
        R.put("dense.D_BS", *entry_ratio(bs, rb, (np.arange(ns)[:, None] + 1.0) * rba))
        R.exact("dense.pivots_positive", bool((fP[:, 3:6] > 0).all()))
    if "substitution" in stages:
        if ns:
            Wl = np.where(diag_mask, 0.0, D_S).astype(LD)
            xs = XS[nI:].astype(LD)
            lhs = np.einsum("nij,nj->ni", Dp, xs)
            rest = (Wl.T @ xs.ravel()).reshape(ns, 3)               # sum_{j>i} W_ji^T x_j
            resta = (np.abs(Wl).astype(np.float64).T @ np.abs(XS[nI:]).ravel()).reshape(ns, 3)
            den = np.einsum("nij,nj->ni", Dpa, np.abs(XS[nI:])) + np.abs(bs) + resta
            R.put("substitution.separators", *entry_ratio(lhs - (bs.astype(LD) - rest), np.zeros_like(lhs), den))
        if nI:
            rl = np.flatnonzero(pl.real)
            acc = np.zeros((nI, 3), dtype=LD)
            acca = np.zeros((nI, 3))
            np.add.at(acc, pl.col[rl], np.einsum("nij,ni->nj", WO[rl].astype(LD), XS[pl.row[rl]].astype(LD)))
            np.add.at(acca, pl.col[rl], np.einsum("nij,ni->nj", np.abs(WO[rl]), np.abs(XS[pl.row[rl]])))
            Dk, Dka = d_of(fD)
            # (the kernel reads a diagonal block's upper triangle; the lower one differs by the Schur updates' rounding)
            lhs = np.einsum("nij,nj->ni", Dk, XS[:nI].astype(LD))
            den = np.einsum("nij,nj->ni", Dka, np.abs(XS[:nI])) + np.abs(F_XB[:nI]) + acca
            R.put("substitution.sparse_columns", *entry_ratio(lhs - (F_XB[:nI].astype(LD) - acc), np.zeros_like(lhs), den))
    pv = pl.pos_vertex
    P1 = np.asarray(X["P1"], dtype=np.float64)
    if "update" in stages:
        d = P1[pv].astype(LD) - (P0[pv].astype(LD) + XS.astype(LD))
        d[:, 2] -= 2 * LD(np.pi) * np.round(d[:, 2] / (2 * LD(np.pi)))
        ab = np.abs(P0[pv]) + np.abs(XS)
        ab[:, 2] = 2 * (np.abs(P0[pv, 2]) + np.abs(XS[:, 2]) + 2 * np.pi)
        R.put("update.poses", *entry_ratio(d, np.zeros_like(d), ab))
        R.exact("update.angles_normalised", bool(((P1[pv, 2] >= -np.pi) & (P1[pv, 2] <= np.pi)).all()))
        rest = np.ones(fixed.size, dtype=bool)
        rest[pv] = False
        R.exact("update.fixed_and_unused_poses_bit_equal", np.array_equal(P1[rest], P0[rest]) and bool(rest[fixed].all()))
    if "history" in stages:
        h = X["hist"]
        t1 = edge_parts(case, P1)
        for q, tt in ((0, t), (1, t1)):
            R.put(f"history.chi2_{q}", kr.ratio(h[2 * q], tt["e2"].sum(), float(tt["e2_abs"].sum())))
            R.put(f"history.robust_{q}", kr.ratio(h[2 * q + 1], tt["rho0_ld"].sum(), float((tt["wbar"] * tt["e2_abs"]).sum())))
    if "composed" in stages:
        pos = np.full(fixed.size, -1, dtype=np.int64)
        pos[pv] = np.arange(n)
        pa, pb = pos[ei], pos[ej]
        xf = np.zeros((n + 1, 3), dtype=LD)
        xf[:n] = XS
        xa = np.abs(xf).astype(np.float64)
        b, ba = np.zeros((n + 1, 3), dtype=LD), np.zeros((n + 1, 3))
        hx, hxa = np.zeros((n + 1, 3), dtype=LD), np.zeros((n + 1, 3))
        np.add.at(b, pa, t["bi_ld"])
        np.add.at(b, pb, t["bj_ld"])
        np.add.at(ba, pa, t["bi_abs"])
        np.add.at(ba, pb, t["bj_abs"])
        Hij, Hija = t["Hij_ld"], t["Hij_abs"]
        np.add.at(hx, pa, np.einsum("nij,nj->ni", t["Hii_ld"], xf[pa]) + np.einsum("nij,nj->ni", Hij, xf[pb]))
        np.add.at(hx, pb, np.einsum("nij,nj->ni", t["Hjj_ld"], xf[pb]) + np.einsum("nji,nj->ni", Hij, xf[pa]))
        np.add.at(hxa, pa, np.einsum("nij,nj->ni", t["Hii_abs"], xa[pa]) + np.einsum("nij,nj->ni", Hija, xa[pb]))
        np.add.at(hxa, pb, np.einsum("nij,nj->ni", t["Hjj_abs"], xa[pb]) + np.einsum("nji,nj->ni", Hija, xa[pa]))
        # |L| |D| |L^T| |x| from the exported factor: L_ik = W_ik D_k^-1, unit diagonal blocks
        tt = xa[:n].copy()                                           # (|L^T| |x|)_k
        rl = np.flatnonzero(pl.real)
        La = np.abs(WO[rl]) @ fDa[pl.col[rl]] if rl.size else np.zeros((0, 3, 3))
        np.add.at(tt, pl.col[rl], np.einsum("nij,ni->nj", La, xa[pl.row[rl]]))
        u = np.zeros((n, 3))
        if nI:
            u[:nI] = np.einsum("nij,nj->ni", d_of(fD)[1], tt[:nI])
        if ns:
            Wl = np.abs(np.where(diag_mask, 0.0, D_S))
            Ls = np.zeros((3 * ns, 3 * ns))
            for j in range(ns):
                Ls[3 * j + 3:, 3 * j:3 * j + 3] = Wl[3 * j + 3:, 3 * j:3 * j + 3] @ Pia[j]
            tt[nI:] += (Ls.T @ xa[nI:n].ravel()).reshape(ns, 3)
            u[nI:] = np.einsum("nij,nj->ni", Dpa, tt[nI:])
        llt = u.copy()
        np.add.at(llt, pl.row[rl], np.einsum("nij,nj->ni", La, u[pl.col[rl]]))
        if ns:
            llt[nI:] += (Ls @ u[nI:].ravel()).reshape(ns, 3)
        res = (b - hx)[:n]
        R.put("composed.residual", *entry_ratio(res, np.zeros_like(res), (ba + hxa)[:n] + llt))
    return R
