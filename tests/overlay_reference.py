"""Stage-by-stage reference for the incremental overlay (CPU only, test infrastructure; sibling of amg_reference.py).

What it checks.  The arrays sgo_debug_overlay_array exports (include/sgo.h; shapes as OverlayDev documents them in
sparse_gslam_amd/csrc/sgo_overlay.h), the right-hand side of sgo_debug_overlay_linearize, the product and dot product of
sgo_debug_overlay_apply and the appended poses after one optimize(1) -- stage by stage in the order overlay_build, k_ov_lin,
k_ov_solve, k_ov_ax and k_ov_finish run.  The input of every stage is the DEVICE's exported output of the stage before it, so a
stage's bound is the rounding bound of that stage alone; the exceptions are the pivot inverses, the chain solve and the hubs.

A case (dict): V0 resident vertices, fixed (V,) bool over all vertices, P0 (V,3) the poses given to the update, the resident
edges res = (ei, ej, meas, info, phi), the appended edges app = (ei, ej, meas, info, phi) of all updates since the base, in
order, and hpos (V0,): the internal row of every resident vertex (any injective map on the free ones; the device's is its
level-0 row order, SGO_AMG_ROW_ORDER before the update) -- the order of the touched rows is taken from it as given.

Part A, forward(): overlay_build's classification and the four kernels restated in plain fp64 from the formulas of
sgo_overlay.h: chain rows / hubs (the LATER endpoint of an edge between non-neighbouring appended poses, unless one endpoint
already is a hub) / touched rows, the entries in edge order, Dn, Un, H0, M0, bt, the block-tridiagonal LDL^T with its
right-hand sides (every pivot solve: the stored inverse applied and refined once against the pivot), S, gk, the hubs' W, M, g, the operator's term with its dot product and the back-substitution.  It serves
the CPU tests, their mutations, and as the rounding scale eps_case of the composed check.

Part B, check(): every entry gets |got - ref| <= C_stage U abs, ref in np.longdouble from the exported inputs, abs the same
expression on magnitudes.
1 structure  exact: HDR, RP, ENT_*, VTX, NZ equal structure()'s; TROW strictly ascending and equal to hpos of the touched
             vertices, which every touched row's entries name through (ENT_EDGE, ENT_SIDE).
2 lin        Dn, Un, H0 (with b_N in the last column), M0, bt from kernel_reference.edge_terms' per-edge fp64 terms, summed
             in long double over the rows' entries; Un zero across segment ends, nothing towards fixed endpoints (both follow
             from the sums being taken over the matching entries only: an entry the kernel adds elsewhere has abs = 0 there).
3 pivot      Sinv_i against the long-double inverse of S_i = Dn_i - U_{i-1}^T Sinv_{i-1} U_{i-1} from the exported arrays:
             |Sinv_i - S_i^-1|_2 <= C U (kappa |S_i^-1|_2 + | |S_i^-1| abs(S_i) |S_i^-1| |_2), kappa as inverse_ratio's.
4 solve      the componentwise backward error of H_NN Y = H0: |H0 - H_NN Y| over U (|H0| + (|H_NN| + |L||S||L^T|) |Y|), the
             factors from the long-double elimination of the exported Dn / Un.
5 schur      S = sym(M0 - H0_K^T Y_K), gk = bt - H0_K^T y_b over the rows of NZ; S bitwise symmetric; H0_K zero off NZ.
6 hubs       Wx against S_XX^-1 [S_XT | g_X] per column in the 2-norm, amg_reference stage 8's bound with C_DENSE;
  m          M = sym(S_TT - S_TX W_T) entry-wise, bitwise symmetric; bitwise S when there is no hub.
7 rhs        the linearize hook's b against the resident edges' b (kernel_reference.reference) + g_T = gk_T - S_TX W_g at the
             touched vertices; every other row against the resident reference alone.
8 operator   the apply hook's y against H_res x (kernel_reference) + M x_T; every row outside T against the resident product.
  dot        its dot against sum x . y_ref within C U sum |x| abs(y).
9 finish     x_X = W_g - W_T x_T, x_N = y_b - Y_K [x_T; x_X], appended poses = P0 (+) x within C U abs(x) plus one rounding of
             the add (and of theta's normalisation); fixed appended poses bitwise unchanged.

Part C, composed(): independent of the exported structure.  H and b of the APPENDED edges alone, np_oracle.linearize's formulas
at P0 (S_TT - H_base,TT of the whole graph is the appended edges' H_TT - H_TA H_AA^-1 H_AT: the resident edges have no block
in the appended rows and cancel identically, so they are left out instead of being subtracted with their rounding), the
appended free poses eliminated in long double (plain Gaussian elimination, written out: numpy has no long-double solver);
M and the hook's b_T are compared in the relative 2-norm against K_OV * eps_case, eps_case the same norm between forward()
and the long-double elimination.  The edge algebra is evaluated in long double as well (edge_blocks_ld; a CPU test holds it
to np_oracle.linearize): np_oracle returns fp64 terms, the very ones forward() sums, and with them on both sides eps_case
would leave out the rounding of the edge terms -- which a closure's lever arm amplifies to 10^2 U in M (measured: moving
the poses by one ulp moves M by 1e-13 .. 3e-13 relative at a closure 30 m from the origin) and the device commits like any
fp64 evaluation.

Constants: at least 2 x and at most 8 x the worst error / (U abs) measured on the MI355X over tests/test_gpu_overlay_reference.py;
the mutation tests (tests/test_overlay_reference.py) require every mutation to be rejected at >= 10 C.  See MEASURED.
"""
from __future__ import annotations

import ctypes as C_

import numpy as np

import kernel_reference as kr
from amg_reference import C_DENSE, Result, entry_ratio, inv3
from kernel_reference import LD, U
from oracle import np_oracle as npo

TILE = 8                      # chain rows per LDS tile of k_ov_solve
OTHER_FIXED = -(1 << 30)
NAMES = "HDR RP ENT_EDGE ENT_OTHER ENT_SIDE VTX TROW NZ DN UN H0 Y SINV M0 BT S GK WX M XT".split()
WHAT = {k: i for i, k in enumerate(NAMES)}          # SGO_OV_* of include/sgo.h
_INT = ("HDR", "RP", "ENT_EDGE", "ENT_OTHER", "VTX", "TROW", "NZ")

# Worst error / (U abs) per stage over the 22 cases of tests/overlay_cases.py: measured on the MI355X
# (tests/test_gpu_overlay_reference.py) | forward() itself on the CPU (tests/test_overlay_reference.py), and where:
#   stage     MI355X   case                       CPU model  case                    constant
#   lin       3.84     multiblock_k257_nk2        2.32       wave_nk64_nx0           12     (3.1 x)
#   pivot     0.555    wave_nk21_nx0              0.748      multiblock_k257_nk2     2      (3.6 x)
#   solve     1.14     multiblock_k512_nk64       2.08       closure_weight_1e10     4      (3.5 x)
#   schur     2.35     wave_nk64_nx8              2.52       wave_nk64_nx8           8      (3.4 x)
#   hubs      0.0823   accumulation               0.082      accumulation            0.5    (6.1 x; C_DENSE, of its normwise bound)
#   m         2.40     wave_nk43_nx8              2.36       wave_nk64_nx8           8      (3.3 x)
#   rhs       0.697    the wave cases             0.006      multiblock_k257_nk2     4      (5.7 x)
#   operator  6.87     multiblock_k512_nk64       1.70       wave_nk42_nx0           24     (3.5 x)
#   dot       2.18e-5  wave_nk22_nx8              4.4e-6     tile_k1                 1e-4   (4.6 x)
#   finish    0.890    wave_nk64_nx0              0.74       multiblock_k512_nk64    4      (4.5 x)
#   composed  5.28     closure_weight_1e10        1 (it is the scale)                16     (3.0 x; 2.44 without the 10^10 closure)
# rhs, operator and dot of the CPU model: its resident part IS the long-double reference rounded once, only the overlay's share errs.
# dot: the bound sums |x| abs(y) over all rows, rows scaled by 10^6 included, and the kernels' tree sums stay far inside it.
# finish is 0 wherever the one rounding of the add at the size of the coordinates covers the whole error.
# solve, before k_ov_solve refined its pivot solves (ov_pivot_solve): 174 at k = 257, 109 at k = 512, 1.7e7 next to the closure of
# weight 10^10 -- the product with an explicit inverse is not backward stable; the fp64 model of that arithmetic measured the same.
# GPU-machine time of tests/test_gpu_overlay_reference.py: 1.8 s for the 22 cases (0.32 s the first, which loads the library).
MEASURED = dict(lin=(3.84, 2.32), pivot=(0.555, 0.748), solve=(1.14, 2.08), schur=(2.35, 2.52), hubs=(0.0823, 0.082), m=(2.40, 2.36),
                rhs=(0.697, 0.006), operator=(6.87, 1.70), dot=(2.18e-5, 4.4e-6), finish=(0.890, 0.74), composed=(5.28, 1.0))
C_STAGE = dict(lin=12.0, pivot=2.0, solve=4.0, schur=8.0, hubs=C_DENSE, m=8.0, rhs=4.0, operator=24.0, dot=1e-4, finish=4.0)
K_OV = 16.0


# ------------------------------------------------------------------ export (the only part that touches the library)
def _fetch(opt, what):
    from sparse_gslam_amd import capi
    L = capi.lib()
    dtype = np.int32 if what in _INT else (np.uint8 if what == "ENT_SIDE" else np.float64)
    size = L.sgo_debug_overlay_array(opt._h, WHAT[what], None, 0)
    if size < 0:
        raise capi.SgoError(f"sgo_debug_overlay_array({what}): {size}: {opt.last_error()}")
    out = np.empty(size // np.dtype(dtype).itemsize, dtype=dtype)
    if size:
        got = L.sgo_debug_overlay_array(opt._h, WHAT[what], out.ctypes.data_as(C_.c_void_p), out.nbytes)
        assert got == size, (what, got, size)
    return out


def shape_arrays(X):
    """Reshape the flat exported arrays in place as OverlayDev documents them."""
    k, nt, ncol, nnz, nx = (int(v) for v in X["HDR"])
    nk = nt + nx
    for key, shp in (("DN", (k, 6)), ("UN", (k, 3, 3)), ("H0", (3 * k, ncol)), ("Y", (3 * k, ncol)), ("SINV", (k, 6)),
                     ("M0", (3 * nk, 3 * nk)), ("S", (3 * nk, 3 * nk)), ("WX", (3 * nx, 3 * nt + 1)), ("M", (3 * nt, 3 * nt))):
        if key in X:
            X[key] = np.asarray(X[key]).reshape(shp)
    return X


def export_overlay(opt, names=NAMES):
    return shape_arrays({k: _fetch(opt, k) for k in names})


def overlay_linearize(opt, n):
    from sparse_gslam_amd import capi
    b = np.empty((n, 3))
    opt._check(capi.lib().sgo_debug_overlay_linearize(opt._h, capi._dp(b)), "sgo_debug_overlay_linearize")
    return b


def overlay_apply(opt, x):
    from sparse_gslam_amd import capi
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    d = C_.c_double()
    opt._check(capi.lib().sgo_debug_overlay_apply(opt._h, capi._dp(x), capi._dp(y), C_.byref(d)), "sgo_debug_overlay_apply")
    return y, d.value


# ------------------------------------------------------------------ helpers
def sym6(p, dtype=np.float64):
    p = np.asarray(p)
    return np.stack([p[..., [0, 1, 2]], p[..., [1, 3, 4]], p[..., [2, 4, 5]]], axis=-2).astype(dtype)


def pack6(M):
    return np.stack([M[..., 0, 0], M[..., 0, 1], M[..., 0, 2], M[..., 1, 1], M[..., 1, 2], M[..., 2, 2]], axis=-1)


def edge_terms(case, which="app"):
    """kernel_reference.edge_terms of the case's appended (or resident) edges at P0, with the off-diagonal block A^T W B."""
    ei, ej, meas, info, phi = case[which]
    P = case["P0"]
    t = kr.edge_terms(P[ei], P[ej], meas, info, phi)
    return t


def _b2(x):
    return np.linalg.norm(np.asarray(x, dtype=np.float64), 2, axis=(-2, -1))


# ------------------------------------------------------------------ part A: the forward model
def structure(case, mut=None):
    """overlay_build's classification: dict(k, nt, nx, HDR, RP, ENT_*, VTX, TROW, NZ, tv: vertex of every touched row)."""
    V0, fixed, hpos = case["V0"], np.asarray(case["fixed"], dtype=bool), case["hpos"]
    ei, ej = (np.asarray(a, dtype=np.int64) for a in case["app"][:2])
    ends = np.r_[ei, ej]
    free = ends[~fixed[ends]]
    tv = np.unique(free[free < V0])
    tv = tv[np.argsort(hpos[tv], kind="stable")]
    nv = np.unique(free[free >= V0])
    new_idx = {int(v): i for i, v in enumerate(nv)}
    is_hub = np.zeros(nv.size, dtype=bool)
    for a, b in zip(ei, ej):
        if fixed[a] or fixed[b] or a < V0 or b < V0:
            continue
        ia, ib = new_idx[int(a)], new_idx[int(b)]
        if abs(ia - ib) != 1 and not is_hub[ia] and not is_hub[ib]:
            is_hub[min(ia, ib) if mut == "hub_earlier" else max(ia, ib)] = True
    chain_v, hub_v = nv[~is_hub], nv[is_hub]
    k, nt, nx = chain_v.size, tv.size, hub_v.size
    nk = nt + nx
    code = {}
    for i, v in enumerate(chain_v):
        code[int(v)] = i
    for t, v in enumerate(tv):
        code[int(v)] = -1 - t
    for j, v in enumerate(hub_v):
        code[int(v)] = -1 - (nt + j)
    cod = lambda v: OTHER_FIXED if fixed[v] else code[int(v)]      # noqa: E731
    rowof = lambda c: c if c >= 0 else k + (-1 - c)                # noqa: E731
    rows = [[] for _ in range(k + nk)]
    for e, (a, b) in enumerate(zip(ei, ej)):
        ca, cb = cod(a), cod(b)
        if ca >= 0 and cb >= 0 and abs(ca - cb) != 1:
            raise ValueError("appended edges among the new poses do not form chain segments")
        if ca != OTHER_FIXED:
            rows[rowof(ca)].append((e, cb, 0))
        if cb != OTHER_FIXED:
            rows[rowof(cb)].append((e, ca, 1))
    rp = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    ent = [t for r in rows for t in r]
    ee = np.array([t[0] for t in ent], dtype=np.int32)
    eo = np.array([t[1] for t in ent], dtype=np.int32)
    es = np.array([t[2] for t in ent], dtype=np.uint8)
    nz = np.array([i for i in range(k) if any(o < 0 and o != OTHER_FIXED for _, o, _ in rows[i])], dtype=np.int32)
    if mut == "side_swap" and es.size:
        es[es.size // 2] ^= 1
    if mut == "nz_missing" and nz.size:
        nz = nz[:-1]
    return dict(k=k, nt=nt, nx=nx, nk=nk, ncol=3 * nk + 1, tv=tv, HDR=np.array([k, nt, 3 * nk + 1, nz.size, nx], dtype=np.int32),
                RP=rp, ENT_EDGE=ee, ENT_OTHER=eo, ENT_SIDE=es, VTX=np.r_[chain_v, hub_v].astype(np.int32),
                TROW=hpos[tv].astype(np.int32), NZ=nz)


def _entry_terms(X, t, dtype):
    """Per entry: its overlay row, the diagonal term, the right-hand-side term, the block towards the other endpoint; magnitudes."""
    row = np.repeat(np.arange(X["RP"].size - 1), np.diff(X["RP"]))
    e, s = X["ENT_EDGE"].astype(np.int64), (X["ENT_SIDE"] != 0)
    Hij, Hij_abs = t["Hij"], t["Hij_abs"]
    s3, s1 = s[:, None, None], s[:, None]
    D = np.where(s3, t["Hjj"][e], t["Hii"][e]).astype(dtype)
    Da = np.where(s3, t["Hjj_abs"][e], t["Hii_abs"][e])
    b = np.where(s1, t["bj"][e], t["bi"][e]).astype(dtype)
    ba = np.where(s1, t["bj_abs"][e], t["bi_abs"][e])
    blk = np.where(s3, np.swapaxes(Hij, 1, 2)[e], Hij[e]).astype(dtype)
    blka = np.where(s3, np.swapaxes(Hij_abs, 1, 2)[e], Hij_abs[e])
    return row, D, Da, b, ba, blk, blka


def lin_sums(X, t, dtype=LD):
    """Stage 2's sums over the entries: (DN, UN, H0, M0, BT) and their magnitudes, accumulated in `dtype`."""
    k, nt, ncol, _, nx = (int(v) for v in X["HDR"])
    nk = nt + nx
    row, D, Da, b, ba, blk, blka = _entry_terms(X, t, dtype)
    oth = X["ENT_OTHER"].astype(np.int64)
    out = [np.zeros(s, dtype=d) for d in (dtype, np.float64) for s in ((k, 3, 3), (k, 3, 3), (3 * k, ncol), (3 * nk, 3 * nk), (3 * nk,))]
    for (Dn, Un, H0, M0, bt), (vD, vb, vblk) in ((out[:5], (D, b, blk)), (out[5:], (Da, ba, blka))):
        for q in range(row.size):                         # entry order: the kernel's
            r, o = int(row[q]), int(oth[q])
            if r < k:
                Dn[r] += vD[q]
                H0[3 * r:3 * r + 3, ncol - 1] += vb[q]
                if o == OTHER_FIXED:
                    continue
                if o >= 0:
                    if o == r + 1:
                        Un[r] += vblk[q]
                else:
                    c = 3 * (-1 - o)
                    H0[3 * r:3 * r + 3, c:c + 3] += vblk[q]
            else:
                t0 = r - k
                M0[3 * t0:3 * t0 + 3, 3 * t0:3 * t0 + 3] += vD[q]
                bt[3 * t0:3 * t0 + 3] += vb[q]
                if o != OTHER_FIXED and o < 0:
                    c = 3 * (-1 - o)
                    M0[3 * t0:3 * t0 + 3, c:c + 3] += vblk[q]
    return out[:5], out[5:]


def _pivot_solve(V, S, B, refine):
    """k_ov_solve's ov_pivot_solve: the stored inverse applied, then one step of iterative refinement against the pivot itself
    (the long-double reference does without: its inverse is exact to 2^-64 kappa)."""
    x = V @ B
    return x + V @ (B - S @ x) if refine else x


def _chain(Dn, Un, H0, dtype, mut=None):
    """Block-tridiagonal LDL^T with right-hand sides: (Sinv [k,3,3], S [k,3,3], L [k,3,3] (L_0 = 0), Y)."""
    k = Dn.shape[0]
    Dn, Un, R = Dn.astype(dtype), Un.astype(dtype), H0.astype(dtype).copy()
    Sinv = np.zeros((k, 3, 3), dtype=dtype)
    Sp = np.zeros((k, 3, 3), dtype=dtype)
    Lf = np.zeros((k, 3, 3), dtype=dtype)
    fp64 = dtype is not LD
    for i in range(k):
        S = Dn[i].copy()
        if i > 0 and not (mut == "tile_skip" and i % TILE == TILE - 1):
            W = _pivot_solve(Sinv[i - 1], Sp[i - 1], Un[i - 1], fp64)
            Lf[i] = W.T
            S = S - Un[i - 1].T @ W
            R[3 * i:3 * i + 3] -= Un[i - 1].T @ _pivot_solve(Sinv[i - 1], Sp[i - 1], R[3 * i - 3:3 * i], fp64)
        if fp64:
            S = sym6(pack6(S))                           # (the kernel carries the upper triangle)
        Sp[i] = S
        Sinv[i] = _inv_sym64(S) if fp64 else inv3(S[None])[0][0]
    Y = R
    for i in range(k - 1, -1, -1):
        if mut == "back_short" and i == 0 and k > 1:
            break
        r = Y[3 * i:3 * i + 3]
        if i < k - 1:
            r = r - Un[i] @ Y[3 * i + 3:3 * i + 6]
        Y[3 * i:3 * i + 3] = _pivot_solve(Sinv[i], Sp[i], r, fp64)
    return Sinv, Sp, Lf, Y


def _inv_sym64(S):
    """k_ov_solve's symmetric cofactor inverse in fp64 (upper triangle of S)."""
    d = pack6(S)
    c00, c01, c02 = d[3] * d[5] - d[4] * d[4], d[2] * d[4] - d[1] * d[5], d[1] * d[4] - d[2] * d[3]
    c11, c12, c22 = d[0] * d[5] - d[2] * d[2], d[1] * d[2] - d[0] * d[4], d[0] * d[3] - d[1] * d[1]
    idet = 1.0 / (d[0] * c00 + d[1] * c01 + d[2] * c02)
    return sym6(np.array([c00, c01, c02, c11, c12, c22]) * idet)


def solve_ld(A, B, dtype=LD):
    """A^-1 B by Gaussian elimination without pivoting (A symmetric positive definite), in `dtype`."""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    n = A.shape[0]
    M = np.concatenate([A, B.reshape(n, -1)], axis=1)
    for p in range(n):
        M[p] = M[p] / M[p, p]
        f = M[:, p].copy()
        f[p] = 0
        M -= f[:, None] * M[p][None, :]
    return M[:, n:].reshape(B.shape)


def forward(case, mut=None, xs=(), xt=None):
    """The fp64 forward model: every exported array, g (3 nt), b (with the resident reference's b), the products of xs with
    their dots, and -- given the step xt at the touched rows -- the appended poses after the update (P1)."""
    X = structure(case, mut)
    k, nt, nx, nk, ncol = X["k"], X["nt"], X["nx"], X["nk"], X["ncol"]
    t = edge_terms(case)
    (Dn, Un, H0, M0, bt), _ = lin_sums(X, t, np.float64)
    if mut == "un_transposed":
        Un = np.swapaxes(Un, 1, 2).copy()
    X.update(DN=pack6(Dn), UN=Un, H0=H0, M0=M0, BT=bt)
    Sinv, _, _, Y = _chain(sym6(X["DN"]), Un, H0, np.float64, mut)
    X.update(SINV=pack6(Sinv), Y=Y)
    nt3, nk3 = 3 * nt, 3 * nk
    rows = np.concatenate([np.arange(3 * z, 3 * z + 3) for z in X["NZ"]]).astype(np.int64) if X["NZ"].size else np.zeros(0, np.int64)
    HK, YK = H0[rows][:, :nk3], Y[rows]
    Sm = M0 - HK.T @ YK[:, :nk3]
    S = Sm if mut == "no_sym" else 0.5 * (Sm + Sm.T)
    gk = bt - HK.T @ YK[:, nk3]
    W = np.zeros((3 * nx, nt3 + 1))
    if nx:
        W = np.linalg.solve(S[nt3:, nt3:], np.concatenate([S[nt3:, :nt3], gk[nt3:, None]], axis=1))
    corr = S[:nt3, nt3:] @ W * (0.0 if mut == "no_stx_w" else 1.0)
    Mm = S[:nt3, :nt3] - corr[:, :nt3]
    M = Mm if mut == "no_sym" else 0.5 * (Mm + Mm.T)
    g = gk[:nt3] - corr[:, nt3]
    if mut == "g_sign":
        g = -g
    X.update(S=S, GK=gk, WX=W, M=M, g=g)
    # ---- right-hand side and operator on the resident rows (hessian order of the resident free poses)
    res = resident_reference(case, xs)
    hidx = res["hidx"]
    tr = hidx[X["tv"]]
    b = res["ref"].b.astype(np.float64)
    b[tr] += g.reshape(nt, 3)
    X["b"] = b
    X["apply"] = []
    for q, x in enumerate(xs):
        y = res["ref"].hx[q].astype(np.float64)
        mx = (M @ x[tr].reshape(nt3)).reshape(nt, 3)
        dot = float((x * y).sum())
        if mut == "mx_wrong_row" and nt:
            y[(tr + 1) % y.shape[0]] += mx
        else:
            y[tr] += mx
        if mut != "dot_share":
            dot = float((x * y).sum())
        X["apply"].append((x, y, dot))
    if xt is not None:
        X["XT"] = np.asarray(xt, dtype=np.float64).reshape(nt3)
        xX = W[:, nt3] - W[:, :nt3] @ X["XT"]
        xk = np.r_[X["XT"], np.zeros_like(xX) if mut == "xn_no_hubs" else xX]
        xN = Y[:, nk3] - Y[:, :nk3] @ xk
        P1 = case["P0"].copy()
        upd = np.r_[xN, xX].reshape(-1, 3)
        v = X["VTX"]
        P1[v, :2] += upd[:, :2]
        P1[v, 2] = npo.normalize_theta(P1[v, 2] + upd[:, 2])
        X["P1"] = P1
    return X


_RES_CACHE = {}


def resident_reference(case, xs=()):
    """kernel_reference.reference of the resident graph at P0 (computed once per case and vector set)."""
    key = (id(case), len(xs))
    if key not in _RES_CACHE or _RES_CACHE[key]["case"] is not case:
        V0 = case["V0"]
        fx = np.asarray(case["fixed"], dtype=bool)[:V0]
        ref = kr.reference(case["P0"][:V0], fx, *case["res"], xs=list(xs))
        hidx, _ = npo.hessian_index(fx)
        _RES_CACHE[key] = dict(case=case, ref=ref, hidx=hidx)
    return _RES_CACHE[key]


# ------------------------------------------------------------------ part B: the stage checks
def check(case, X, stages=(1, 2, 3, 4, 5, 6, 7, 8, 9)):
    """Raw worst ratios {"stage.name": (error / (U abs), where)}: exact checks give 0 or inf."""
    R = Result()
    k, nt, ncol, nnz, nx = (int(v) for v in X["HDR"])
    nk, nt3, nk3 = nt + nx, 3 * nt, 3 * (nt + nx)
    St = structure(case)
    if 1 in stages:
        for name in ("HDR", "RP", "ENT_EDGE", "ENT_OTHER", "ENT_SIDE", "VTX", "NZ", "TROW"):
            R.exact("structure." + name, np.array_equal(np.asarray(X[name]), St[name]))
        R.exact("structure.trow_ascending", bool((np.diff(X["TROW"]) > 0).all()))
        ok = X["RP"].size == k + nk + 1 and X["ENT_EDGE"].size == (X["RP"][-1] if X["RP"].size else 0)
        if ok:
            ei, ej = case["app"][:2]
            v = np.where(X["ENT_SIDE"] != 0, np.asarray(ej)[X["ENT_EDGE"]], np.asarray(ei)[X["ENT_EDGE"]])
            rowv = np.r_[X["VTX"][:k], St["tv"], X["VTX"][k:]] if St["tv"].size == nt else None
            ok = rowv is not None and np.array_equal(v, np.repeat(rowv, np.diff(X["RP"])))
        R.exact("structure.entries_name_their_row", bool(ok))
        if R.worst() > 0:
            return R                                  # the later stages read the structure
    t = edge_terms(case)
    if 2 in stages:
        (Dn, Un, H0, M0, bt), (Dna, Una, H0a, M0a, bta) = lin_sums(X, t, LD)
        R.put("lin.DN", *entry_ratio(X["DN"], pack6(Dn), pack6(Dna)))
        R.put("lin.UN", *entry_ratio(X["UN"], Un, Una))
        R.put("lin.H0", *entry_ratio(X["H0"], H0, H0a))
        R.put("lin.M0", *entry_ratio(X["M0"], M0, M0a))
        R.put("lin.BT", *entry_ratio(X["BT"], bt, bta))
    Dn, Un, H0, Y = sym6(X["DN"], LD), X["UN"].astype(LD), X["H0"].astype(LD), X["Y"].astype(LD)
    if 3 in stages and k:
        Sv = sym6(X["SINV"], LD)
        UtS = np.einsum("kji,kjl->kil", Un[:-1], Sv[:-1])
        S = Dn.copy()
        S[1:] -= np.einsum("kij,kjl->kil", UtS, Un[:-1])
        Sa = np.abs(Dn).astype(np.float64)
        Ua = np.abs(X["UN"][:-1])
        Sa[1:] += np.swapaxes(Ua, 1, 2) @ np.abs(sym6(X["SINV"][:-1])) @ Ua
        ref, det = inv3(S)
        ra = np.abs(ref).astype(np.float64)
        kappa = _b2(ref) * _b2(np.abs(S))
        err = _b2(Sv - ref)
        r = err / (U * (kappa * _b2(ref) + _b2(ra @ Sa @ ra)))
        r = np.where(np.isfinite(r) & (det.astype(np.float64) > 0), r, np.inf)
        R.put("pivot.SINV", float(r.max()), (int(np.argmax(r)),))
    if 4 in stages and k:
        _, Sp, Lf, _ = _chain(Dn, Un, H0, LD)
        Yb, Hb = Y.reshape(k, 3, ncol), H0.reshape(k, 3, ncol)
        AY = np.einsum("kij,kjc->kic", Dn, Yb)
        AY[:-1] += np.einsum("kij,kjc->kic", Un[:-1], Yb[1:])
        AY[1:] += np.einsum("kji,kjc->kic", Un[:-1], Yb[:-1])
        Ya = np.abs(Yb).astype(np.float64)
        La, Spa, Dna, Una = (np.abs(a).astype(np.float64) for a in (Lf, Sp, Dn, Un))
        dg = Dna + Spa
        dg[1:] += La[1:] @ Spa[:-1] @ np.swapaxes(La[1:], 1, 2)
        lo = np.swapaxes(Una[:-1], 1, 2) + La[1:] @ Spa[:-1]                 # block (i, i-1)
        den = np.abs(Hb).astype(np.float64) + dg @ Ya
        den[1:] += lo @ Ya[:-1]
        den[:-1] += np.swapaxes(lo, 1, 2) @ Ya[1:]
        R.put("solve.Y", *entry_ratio(Hb - AY, np.zeros_like(AY), den))
    rows = np.concatenate([np.arange(3 * z, 3 * z + 3) for z in X["NZ"]]).astype(np.int64) if nnz else np.zeros(0, np.int64)
    if 5 in stages:
        off = np.setdiff1d(np.arange(3 * k), rows)
        R.exact("schur.H0_zero_off_NZ", not np.any(X["H0"][off][:, :nk3] != 0.0))
        HK, YK = H0[rows][:, :nk3], Y[rows]
        Sm = X["M0"].astype(LD) - HK.T @ YK[:, :nk3]
        Sa = np.abs(X["M0"]) + np.abs(X["H0"][rows][:, :nk3]).T @ np.abs(X["Y"][rows][:, :nk3])
        R.put("schur.S", *entry_ratio(X["S"], (Sm + Sm.T) / 2, (Sa + Sa.T) / 2))
        R.exact("schur.S_symmetric", np.array_equal(X["S"], X["S"].T))
        R.put("schur.GK", *entry_ratio(X["GK"], X["BT"].astype(LD) - HK.T @ YK[:, nk3],
                                       np.abs(X["BT"]) + np.abs(X["H0"][rows][:, :nk3]).T @ np.abs(X["Y"][rows][:, nk3])))
    S, W = X["S"], X["WX"]
    if 6 in stages:
        if nx:
            Sxx = S[nt3:, nt3:]
            rhs = np.concatenate([S[nt3:, :nt3], X["GK"][nt3:, None]], axis=1)
            ref = solve_ld(Sxx, rhs)
            kap = np.linalg.cond(Sxx, 2)
            err = np.linalg.norm((W.astype(LD) - ref).astype(np.float64), axis=0)
            nrm = np.linalg.norm(ref.astype(np.float64), axis=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(nrm > 0, err / (3 * nx * U * kap * nrm), np.where(err > 0, np.inf, 0.0))
            r = np.where(np.isfinite(W).all(axis=0), r, np.inf)
            R.put("hubs.WX", float(r.max()), (int(np.argmax(r)),))
            Mm = S[:nt3, :nt3].astype(LD) - S[:nt3, nt3:].astype(LD) @ W[:, :nt3].astype(LD)
            Ma = np.abs(S[:nt3, :nt3]) + np.abs(S[:nt3, nt3:]) @ np.abs(W[:, :nt3])
            R.put("m.M", *entry_ratio(X["M"], (Mm + Mm.T) / 2, (Ma + Ma.T) / 2))
        else:
            R.exact("m.M_is_S", np.array_equal(X["M"], S))
        R.exact("m.M_symmetric", np.array_equal(X["M"], X["M"].T))
    tv = St["tv"]
    if 7 in stages and "b" in X:
        res = resident_reference(case, [a[0] for a in X.get("apply", [])])
        tr = res["hidx"][tv]
        ref, ab = res["ref"].b.copy(), res["ref"].b_abs.copy()
        g = X["GK"][:nt3].astype(LD) - S[:nt3, nt3:].astype(LD) @ W[:, nt3].astype(LD)
        ref[tr] += g.reshape(nt, 3)
        ab[tr] += (np.abs(X["GK"][:nt3]) + np.abs(S[:nt3, nt3:]) @ np.abs(W[:, nt3])).reshape(nt, 3)
        R.put("rhs.b", *entry_ratio(X["b"], ref, ab))
    if 8 in stages and X.get("apply"):
        res = resident_reference(case, [a[0] for a in X["apply"]])
        tr = res["hidx"][tv]
        for q, (x, y, dot) in enumerate(X["apply"]):
            ref, ab = res["ref"].hx[q].copy(), res["ref"].hx_abs[q].copy()
            ref[tr] += (X["M"].astype(LD) @ x[tr].reshape(nt3).astype(LD)).reshape(nt, 3)
            ab[tr] += (np.abs(X["M"]) @ np.abs(x[tr].reshape(nt3))).reshape(nt, 3)
            R.put(f"operator.y{q}", *entry_ratio(y, ref, ab))
            R.put(f"dot.d{q}", *entry_ratio(np.array([dot]), np.array([(x.astype(LD) * ref).sum()]), np.array([float((np.abs(x) * ab).sum())])))
    if 9 in stages and "P1" in X:
        P0, P1, xt = case["P0"], X["P1"], X["XT"].astype(LD)
        Wl, Yl = W.astype(LD), Y
        xX = Wl[:, nt3] - Wl[:, :nt3] @ xt
        xXa = np.abs(W[:, nt3]) + np.abs(W[:, :nt3]) @ np.abs(X["XT"])
        xN = Yl[:, nk3] - Yl[:, :nt3] @ xt - Yl[:, nt3:nk3] @ xX
        xNa = np.abs(X["Y"][:, nk3]) + np.abs(X["Y"][:, :nt3]) @ np.abs(X["XT"]) + np.abs(X["Y"][:, nt3:nk3]) @ xXa
        x = np.r_[xN, xX].reshape(-1, 3)
        xa = np.r_[xNa, xXa].reshape(-1, 3)
        v = X["VTX"].astype(np.int64)
        ref = P0[v].astype(LD) + x
        d = (P1[v].astype(LD) - ref)
        d[:, 2] -= 2 * LD(np.pi) * np.round(d[:, 2] / (2 * LD(np.pi)))
        extra = U * (np.abs(P0[v]) + np.abs(x).astype(np.float64))
        extra[:, 2] = 2 * U * (np.abs(P0[v, 2]) + np.abs(x[:, 2]).astype(np.float64) + 2 * np.pi)
        R.put("finish.poses", *entry_ratio(d, np.zeros_like(d), xa, extra=extra))
        fa = np.flatnonzero(np.asarray(case["fixed"], dtype=bool)[case["V0"]:]) + case["V0"]
        R.exact("finish.fixed_unchanged", np.array_equal(P1[fa], P0[fa]))
    return R


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


# ------------------------------------------------------------------ part C: the composed check
def _wrap_ld(t):
    two_pi = LD("6.283185307179586476925286766559005768")
    u = t - np.floor(t / two_pi) * two_pi
    u = np.where(u >= two_pi / 2, u - two_pi, u)
    return np.where((t >= -two_pi / 2) & (t < two_pi / 2), t, u)


def edge_parts_ld(P, ei, ej, meas):
    """(e, A, B) per edge in long double: np_oracle's edge_error and edge_jacobians, the part of edge_blocks_ld's algebra before
    the information matrix (the candidates of sgo_candidate_gate have no more than this: tests/fsolve_reference.py)."""
    xi, xj, z = (np.asarray(a, dtype=np.float64).astype(LD) for a in (P[ei], P[ej], meas))
    m = xi.shape[0]
    ci, si = np.cos(xi[:, 2]), np.sin(xi[:, 2])
    dx, dy = xj[:, 0] - xi[:, 0], xj[:, 1] - xi[:, 1]
    cz, sz = np.cos(-z[:, 2]), np.sin(-z[:, 2])
    rx, ry = ci * dx + si * dy - z[:, 0], -si * dx + ci * dy - z[:, 1]
    e = np.stack([cz * rx - sz * ry, sz * rx + cz * ry, _wrap_ld(_wrap_ld(xj[:, 2] - xi[:, 2]) - z[:, 2])], axis=1)
    A0 = np.zeros((m, 3, 3), dtype=LD)
    B0 = np.zeros((m, 3, 3), dtype=LD)
    A0[:, 0, 0], A0[:, 0, 1], A0[:, 0, 2] = -ci, -si, -si * dx + ci * dy
    A0[:, 1, 0], A0[:, 1, 1], A0[:, 1, 2] = si, -ci, -ci * dx - si * dy
    A0[:, 2, 2] = -1
    B0[:, 0, 0], B0[:, 0, 1], B0[:, 1, 0], B0[:, 1, 1], B0[:, 2, 2] = ci, si, -si, ci, 1
    Rz = np.zeros((m, 3, 3), dtype=LD)
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = cz, -sz, sz, cz, 1
    A, B = Rz @ A0, Rz @ B0
    return e, A, B


def edge_blocks_ld(P, ei, ej, meas, info, phi):
    """np_oracle's edge algebra (edge_error, edge_jacobians, dcs_rho, the quadratic form) evaluated in long double throughout:
    (b_i, b_j, H_ii, H_jj, H_ij) per edge.  np_oracle itself returns fp64 for any input, and forward() shares those fp64 terms."""
    e, A, B = edge_parts_ld(P, ei, ej, meas)
    O = npo.info_full(info).astype(LD)
    e2 = np.einsum("ni,nij,nj->n", e, O, e)
    ph = np.asarray(phi, dtype=np.float64).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(ph >= 0, 2 * ph / (ph + e2), LD(1))
    w = np.where((ph < 0) | (scale >= 1), LD(1), scale * scale)
    Ow = O * w[:, None, None]
    At, Bt = np.swapaxes(A, 1, 2), np.swapaxes(B, 1, 2)
    Oe = np.einsum("nij,nj->ni", Ow, e)
    return -np.einsum("nij,nj->ni", At, Oe), -np.einsum("nij,nj->ni", Bt, Oe), At @ Ow @ A, Bt @ Ow @ B, At @ Ow @ B


def appended_system_ld(case):
    """(av, tv, [H | b]) dense in long double: the appended edges' Gauss-Newton system at P0 on the appended free poses av
    (ascending id) followed by the touched resident poses tv (ascending id)."""
    V0, fixed = case["V0"], np.asarray(case["fixed"], dtype=bool)
    ei, ej, meas, info, phi = case["app"]
    ei, ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
    ends = np.unique(np.r_[ei, ej])
    ends = ends[~fixed[ends]]
    tv, av = ends[ends < V0], ends[ends >= V0]
    pos = np.full(fixed.size, -1, dtype=np.int64)
    pos[np.r_[av, tv]] = np.arange(av.size + tv.size)
    bi, bj, Hii, Hjj, Hij = edge_blocks_ld(case["P0"], ei, ej, meas, info, phi)
    N = 3 * (av.size + tv.size)
    M = np.zeros((N, N + 1), dtype=LD)
    for q in range(ei.size):
        a, c = pos[ei[q]], pos[ej[q]]
        if a >= 0:
            M[3 * a:3 * a + 3, 3 * a:3 * a + 3] += Hii[q]
            M[3 * a:3 * a + 3, N] += bi[q]
        if c >= 0:
            M[3 * c:3 * c + 3, 3 * c:3 * c + 3] += Hjj[q]
            M[3 * c:3 * c + 3, N] += bj[q]
        if a >= 0 and c >= 0:
            M[3 * a:3 * a + 3, 3 * c:3 * c + 3] += Hij[q]
            M[3 * c:3 * c + 3, 3 * a:3 * a + 3] += Hij[q].T
    return av, tv, M


def composed_reference(case):
    """(tv, M_ref [3nt,3nt], g_ref [3nt]) in long double: the appended edges' H and b at P0 with the appended free poses
    eliminated; tv: the touched vertices in ascending id."""
    av, tv, M = appended_system_ld(case)
    na = 3 * av.size
    for p in range(na):
        f = M[p + 1:, p] / M[p, p]
        nzr = np.flatnonzero(f != 0)
        if nzr.size:
            M[p + 1 + nzr, p:] -= f[nzr, None] * M[p, p:][None, :]
    return tv, M[na:, na:-1], M[na:, -1]


def composed(case, M_got, b_got, tv_got):
    """{"M": (relative 2-norm error of M over eps_case, eps_case), "b": the same for the hook's b at the touched rows}.
    tv_got: the vertex of every touched row of M_got; b_got: the linearize hook's b ([n][3], hessian order of the resident free
    poses).  eps_case of b: forward()'s distance, or -- where that is larger -- the resident rows' own rounding scale
    U |abs(b_T)|_2 / |b_T|_2 from kernel_reference (forward() takes the resident part from the long-double reference; the
    device sums it in fp64)."""
    tv, Mr, gr = composed_reference(case)
    F = forward(case)
    res = resident_reference(case)

    def perm(tvx):
        p = np.searchsorted(tv, tvx)
        return (3 * p[:, None] + np.arange(3)[None, :]).ravel()

    def rel(a, ref):
        n = np.sqrt((ref * ref).sum())
        return float(np.sqrt(((np.asarray(a, dtype=LD) - ref) ** 2).sum()) / n) if n > 0 else 0.0

    pf, pg = perm(F["tv"]), perm(np.asarray(tv_got))
    out = {}
    eps = max(rel(F["M"], Mr[np.ix_(pf, pf)]), U)
    out["M"] = (rel(M_got, Mr[np.ix_(pg, pg)]) / eps, eps)
    tr = res["hidx"][tv]
    bref = res["ref"].b[tr] + gr.reshape(-1, 3)
    nb = float(np.sqrt((bref * bref).sum()))
    eps = max(rel(F["b"][tr], bref), U * float(np.linalg.norm(res["ref"].b_abs[tr])) / nb if nb > 0 else 0.0, U)
    out["b"] = (rel(np.asarray(b_got)[tr], bref) / eps, eps)
    return out
