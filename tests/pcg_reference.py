"""A long-double restatement of the device-resident PCG recurrence, checked LOCALLY (CPU only, test infrastructure).

What is checked.  The start (k_finalize's start state, k_init_scalars, k_warm_start, k_restart_scalars) and one iteration
(the product with its p.q, k_update_xr, the preconditioner, k_update_p) of sparse_gslam_amd/csrc/sgo_kernels.hip as
sgo_solve.cpp's start_pcg / pcg_iteration / run_pcg drive them.  CG trajectories diverge legitimately (a last bit of alpha moves
every later iterate), so no stage is compared with a reference trajectory: every stage is evaluated in np.longdouble from the
DEVICE'S OWN exported inputs of that stage (sgo_debug_pcg_array) and compared with the device's exported output of it.

How adjacent runs fit together.  State k is what a run capped at maxit = k leaves (sgo_debug_pcg_run; maxit = 0: the start
alone).  The iteration that sets a stop does not update p, so run k holds x_k, r_k, z_k, beta_{k-1} and still p_{k-1}; run
k + 1 holds p_k, q_k = H p_k, alpha_k, p_k . q_k, x_{k+1}, r_{k+1}, z_{k+1}, beta_k.  check_step(run k, run k + 1) therefore
reads p_k from the later run and everything "before" from the earlier one.  This rests on run-to-run bitwise determinism,
which every case asserts first (same_bits of two runs with the same cap).

Bounds.  Every figure is error / (C U abs): U = 2^-53, abs the sum of the absolute values of the terms of the checked entry
or scalar, C the stage's constant below.  A value above 1 fails.  Bitwise checks give 0 or inf.
* dot products and sums (r.z, b.b, p.q, r.r, z.q, b.x_prev, x_prev.q; a scalar against its exported partial-sum row, a row's
  sum against the vectors): abs = sum |a_i b_i|, constant min(C_DOT = 16, number of terms) -- number of terms is the provable
  bound of ANY summation order (gamma_m ~ m U), so the constant is never above it; a row of one partial sum must match bitwise.
* x + alpha p, r - alpha q, z + beta p: abs = |x| + |alpha| |p| (...); two roundings, or one with an FMA: C_AXPY = 2 is the
  provable bound itself.
* z = Dinv r per entry: a three-term dot, abs = sum |Dinv_ij| |r_j|, C_Z = 3 (provable);  xs0 = omega (Dinv r): one more
  rounding, C_XS = 4.
* alpha = rz / pq, the plain beta = rz / rz_prev, probe_rel = rr / bb: one correctly rounded division, C_DIV = 1.
  tol2: three roundings (tol tol, bb_ref / bb, their product), C_TOL = 3.  The flexible beta = -alpha (z.q) / rz_prev: the
  dot's bound on z.q plus two roundings.
* q = H p: tests/kernel_reference.py's product and its constant (16).
* drift |b - H x_k - r_k| per entry at EVERY iterate of a whole solve (the GPU test exports the runs capped at 0 .. N + 1 of a
  solve of N iterations; the run capped at N is bitwise the uncapped solve), accumulated from the exported states themselves:
  D_{k+1} = D_k + U [2 (|r_k| + |alpha_k q_k|) + 16 |alpha_k| abs(H p_k) + 2 abs(H (|x_k| + |alpha_k p_k|))] -- the two updates'
  own roundings, the product's bound, and the update of x seen through H -- plus the reference product's own 16 U abs(H x_k).
  The bound grows faster than the error: the model's worst figure (0.08) falls in the first three iterations, at the end of its
  whole solves (N = 145, 290) it stands at 0.007 of the bound.  C_DRIFT = 0.5 is therefore set by the first iterations and is
  not tight at N: there it rejects anything that is not rounding (a few hundred U abs), no more.
* the multigrid cycle inside the loop: amg_reference's normwise figure, |z - z_ref| / |z_ref| / eps_case <= K_CYCLE.

The constants.  Rule of the project: 4 x the worst ratio of a plain fp64 numpy model of the same arithmetic (model() below: numpy
dots per 256-row block, numpy sums of the blocks' results, einsum for the 3x3 products) over the CPU cases of tests/pcg_cases.py,
rounded up to a power of two -- and never above the provable bound where the stage has one (PROVABLE: a stage of m roundings
cannot err by more than m U abs in any order, with or without FMA).  No constant was set from a kernel's output.

    stage                  model worst   4 x, power of two   provable   C         MI355X worst
    dot / row sums         3.83          16                  terms      16        2.33  bj_n255
    axpy (x, r, p)         1.72          8                   2          2         1.00  bj_large_chain
    z = Dinv r             2.81          16                  3          3         2.90  bj_large_chain
    xs0 = omega Dinv r     2.80          16                  4          4         3.27  amg_c2
    alpha, beta, probe     0.83          4                   1          1         0.974 bj_n255
    tol2                   0             -                   3          3         0 (bitwise)
    drift                  0.08          0.5                 -          0.5       0.064 bj_scaled_rows at k = 1, over every cap 1 .. N of
                                                                                  every case but the large chain (N = 1 .. 303); at k = N:
                                                                                  0.047 amg_c2_kcycle, 0.040 amg_c2, 0.007 - 0.017 block-Jacobi
    q = H p (kernel_reference, C = 16)                                            4.66  bj_large_chain
    cycle in the loop (amg_reference.K_CYCLE = 8, units of eps_case)              2.98  amg_c2 over its 24 caps; 0.30 the dense single level
                                                                                  (both bitwise equal to sgo_precondition's; the K-cycle,
                                                                                  outside that stage, is held to those bits alone)
The MI355X column is over every state of the whole solves (caps 0 .. N + 1) of every case but the large chain (caps 0 .. 3).
(MODEL and MEASURED: the dicts below; tests/test_pcg_reference.py asserts the model's figures and the rule, and prints them;
tests/test_gpu_pcg_reference.py prints the device's per case.)
"""
from __future__ import annotations

import numpy as np

import kernel_reference as kr

LD = np.longdouble
U = kr.U

C_DOT, C_AXPY, C_Z, C_XS, C_DIV, C_TOL, C_DRIFT = 16.0, 2.0, 3.0, 4.0, 1.0, 3.0, 0.5
# worst error / (U abs) of the fp64 numpy model over tests/pcg_cases.py's CPU cases (tests/test_pcg_reference.py prints them)
MODEL = dict(dot=3.83, axpy=1.72, z=2.81, xs=2.80, div=0.83, tol=0.0, drift=0.08)
PROVABLE = dict(axpy=2.0, z=3.0, xs=4.0, div=1.0, tol=3.0)      # (dot: the number of terms, applied per check)
# worst error / (U abs) on the MI355X over tests/test_gpu_pcg_reference.py (from its printed figures; a record, asserted nowhere)
MEASURED = dict(dot=2.33, axpy=1.00, z=2.90, xs=3.27, div=0.974, tol=0.0, drift=0.064, product=4.66, cycle=2.98)

BLOCK = 256          # rows per workgroup of the vector kernels
MAX_GRID = 2048      # kMaxGrid: the grid-stride loops start above BLOCK * MAX_GRID rows
VECTORS = ("B", "X", "R", "Z", "P", "Q")


def grid_for(n, per_block=BLOCK):
    """workgroups of a vector kernel over n items (sgo_internal.h): at least 8, at most MAX_GRID, a multiple of 8"""
    g = min(max((n + per_block - 1) // per_block, 8), MAX_GRID)
    return (g + 7) // 8 * 8


# ------------------------------------------------------------------ export (the only part that touches the library)
def export_state(o):
    """Everything sgo_debug_pcg_array gives, vectors in hessian order.  'raw': the bytes, for bitwise comparisons."""
    order = o.pcg_array("ROW_ORDER").astype(np.int64)         # hessian row -> internal row
    raw = {k: o.pcg_array(k) for k in VECTORS + ("DINV", "XS0", "SCALARS", "HOST_SCALARS", "MIRROR", "PARTIALS", "ZPARTS", "COUNTS",
                                                  "LANCZOS", "START_ARGS")}
    st = dict(n=order.size, raw=raw, amg=raw["ZPARTS"] is not None)
    for k in VECTORS + ("DINV", "XS0"):
        st[k.lower()] = None if raw[k] is None else raw[k][order]
    for k, name in (("S", "SCALARS"), ("H", "HOST_SCALARS"), ("M", "MIRROR")):
        st[k] = {f: raw[name][0][f].item() for f in raw[name].dtype.names}
    c = dict(zip(("start_bb", "start_rz", "n_pq", "n_rz", "n_rr", "n_zq", "n_xq", "n_bx"), (int(v) for v in raw["COUNTS"])))
    st["counts"] = c
    P, Z = raw["PARTIALS"], raw["ZPARTS"]
    amg = st["amg"]
    st["rows"] = dict(start_bb=P[1, :c["start_bb"]], start_rz=(Z[0] if amg else P[0])[:c["start_rz"]], xq=P[0, :c["n_xq"]],
                      bx=P[2, :c["n_bx"]], pq=P[0, :c["n_pq"]], rr=P[2, :c["n_rr"]], rz=(Z[0] if amg else P[1])[:c["n_rz"]],
                      zq=Z[1, :c["n_zq"]] if amg else P[0, :0])
    st["args"] = dict(zip(("tol", "tol_cap", "bb_ref", "maxit"), (float(v) for v in raw["START_ARGS"])))
    st["lanczos"] = raw["LANCZOS"]
    st["cmp"] = _comparable(st)
    return st


def _scalar_bytes(S):
    return b"".join(np.asarray(S[k]).tobytes() for k in sorted(S) if k != "pad")


def _comparable(st):
    """What a bitwise comparison of two states reads: every vector, the partial-sum rows up to their counts (the rows' tails and
    the record's padding are memory no launch of the solve has written), the three copies of the scalars, counts, records."""
    out = {k: (None if st[k] is None else np.ascontiguousarray(st[k]).tobytes()) for k in ("b", "x", "r", "z", "p", "q", "dinv", "xs0")}
    out.update({"row." + k: np.ascontiguousarray(v, dtype=np.float64).tobytes() for k, v in st["rows"].items()})
    out.update({k: _scalar_bytes(st[k]) for k in ("S", "H", "M")})
    out["counts"] = repr(sorted(st["counts"].items()))
    out["args"] = repr(sorted(st["args"].items()))
    out["lanczos"] = None if st["lanczos"] is None else np.ascontiguousarray(st["lanczos"]).tobytes()
    return out


def same_bits(A, B, skip=()):
    """The parts of two exported states that differ in a bit ([] = bitwise equal)."""
    return [k for k, a in A["cmp"].items() if k not in skip and a != B["cmp"][k]]


# ------------------------------------------------------------------ arithmetic helpers
class Fig(float):
    """a figure error / (C U abs) that remembers error / (U abs) and C"""
    raw = 0.0
    c = 1.0


def fig(ratio, c):
    f = Fig(ratio / c)
    f.raw, f.c = float(ratio), float(c)
    return f


def ldot(a, b):
    """(long-double dot, sum of |terms|, number of terms)"""
    a = np.asarray(a, dtype=LD).ravel()
    b = np.asarray(b, dtype=LD).ravel()
    t = a * b
    return t.sum(), float(np.abs(t).sum()), t.size


def dot_ratio(got, a, b):
    """error / (min(C_DOT, terms) U abs) of a scalar (or of a partial-sum row's long-double sum) against a . b"""
    ref, ab, m = ldot(a, b)
    return fig(kr.ratio(got, ref, ab), min(C_DOT, max(m, 1)))


def row_sum(row):
    return np.asarray(row, dtype=LD).sum()


def scalar_of_row(got, row):
    """a scalar against the partial-sum row it was reduced from: any order of row.size - 1 additions"""
    row = np.asarray(row)
    if row.size <= 1:
        return 0.0 if (row.size == 1 and np.float64(got).tobytes() == row[:1].tobytes()) or (row.size == 0 and got == 0.0) else np.inf
    return fig(kr.ratio(got, row_sum(row), float(np.abs(row).sum())), min(C_DOT, row.size - 1))


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return 0.0 if a.shape == b.shape and a.tobytes() == b.tobytes() else np.inf


def flag(ok):
    return 0.0 if ok else np.inf


def dinv_apply(dinv, r, dtype=LD):
    """(Dinv r, |Dinv| |r|) per entry; dinv (n,6): the upper triangle by rows"""
    d = np.asarray(dinv)
    M = np.empty((d.shape[0], 3, 3), dtype=dtype)
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2] = (d[:, k] for k in range(6))
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]
    r = np.asarray(r, dtype=dtype)
    return np.einsum("nij,nj->ni", M, r), np.einsum("nij,nj->ni", np.abs(M), np.abs(r)).astype(np.float64)


class Operator:
    """H x of a graph at its poses through tests/kernel_reference.py: products([x, ...]) -> [(H x long double, abs), ...]"""

    def __init__(self, arrays, poses=None):
        self.arrays = arrays
        self.poses = np.asarray(arrays[0] if poses is None else poses, dtype=np.float64)
        self.ref0 = None

    def products(self, xs):
        p, fixed, ei, ej, meas, info, phi = self.arrays
        ref = kr.reference(self.poses, fixed, ei, ej, meas, info, phi, xs=[np.asarray(x, dtype=np.float64) for x in xs])
        self.ref0 = ref
        return list(zip(ref.hx, ref.hx_abs))


# ------------------------------------------------------------------ the rules in plain words (fp64, as the kernels evaluate them)
def tol2_rule(tol, tol_cap, bb_ref, bb, capped=True):
    t2 = np.float64(tol) * np.float64(tol)
    if bb_ref > 0.0 and bb > 0.0 and bb < bb_ref:
        t = t2 * (np.float64(bb_ref) / np.float64(bb))
        t2 = min(np.float64(tol_cap) * np.float64(tol_cap), t) if capped else t
    return float(t2)


def stop_rule(S):
    """k_update_p's decision from the scalars it left"""
    rr, bb = np.float64(S["rr"]), np.float64(S["bb"])
    stop = 0
    if not (np.isfinite(S["rz"]) and np.isfinite(rr)):
        stop = 3
    elif rr <= np.float64(S["tol2"]) * bb:
        stop = 1
    elif S["iter"] >= S["maxit"]:
        stop = 2
    if S["iter"] == S["probe_k"] and not stop and S["probe_max"] > 0.0 and rr > np.float64(S["probe_max"]) * bb:
        stop = 4
    return stop


def gamma_rule(bx, xq):
    with np.errstate(all="ignore"):
        g = np.float64(bx) / np.float64(xq)
    if not (xq > 0.0) or not np.isfinite(g) or not (g > 0.0) or g > 4.0:
        return 0.0
    return float(g)


# ------------------------------------------------------------------ stage 1: the start
def check_start(S0, x_prev=None, prod_xprev=None, omega=None, xs0_kept=True):
    """Stage 1 on the state a start alone leaves (maxit = 0).  x_prev / prod_xprev = (H x_prev, abs): a warm start."""
    s, R, A = S0["S"], S0["rows"], S0["args"]
    res = {}
    b, x, r, z, p = (S0[k] for k in "bxrzp")
    warm = x_prev is not None
    cold_start = True
    if warm:
        xp = np.asarray(x_prev, dtype=np.float64).reshape(-1, 3)
        q = S0["q"]                                                # the device's H x_prev
        res["warm.q"] = fig(kr.ratio(q, prod_xprev[0], prod_xprev[1]), kr.C)
        res["warm.xq_row"] = dot_ratio(row_sum(R["xq"]), xp, q)
        res["warm.bx_row"] = dot_ratio(row_sum(R["bx"]), b, xp)
        bx, bx_abs, m = ldot(b, xp)
        xq, xq_abs, _ = ldot(xp, q)
        g = gamma_rule(float(bx), float(xq))
        S0["gamma_ref"] = g
        # a gamma within rounding of a threshold (0, 4) may fall on either side: the cases keep away from them
        if g > 0.0:
            cold_start = False
            c = min(C_DOT, m)
            rel = c * bx_abs / abs(float(bx)) + c * xq_abs / abs(float(xq)) + 2.0        # gamma's own error / U, + the product's rounding
            gx = LD(bx) / LD(xq) * xp.astype(LD)
            gq = LD(bx) / LD(xq) * q.astype(LD)
            res["warm.x0"] = kr.ratio(x, gx, np.abs(gx).astype(np.float64) * rel)
            res["warm.r0"] = kr.ratio(r, b.astype(LD) - gq, np.abs(b) + np.abs(gq).astype(np.float64) * rel)
    if cold_start:
        res["x0=0"] = flag(not x.any())        # (0 x_prev of a refused warm start may be -0.0: equal to zero, not bitwise)
        res["r0=b"] = bits(r, b)
    res["p0=z0"] = bits(p, z)
    zz, zabs = dinv_apply(S0["dinv"], r)
    if not S0["amg"]:
        res["z0"] = fig(kr.ratio(z, zz, zabs), C_Z)
    elif S0["xs0"] is not None and xs0_kept:
        res["xs0"] = fig(kr.ratio(S0["xs0"], LD(omega) * zz, abs(omega) * zabs), C_XS)
    res["rz_row"] = dot_ratio(row_sum(R["start_rz"]), r, z)
    res["rz"] = scalar_of_row(s["rz"], R["start_rz"])
    if warm:   # (the product H x_prev has stored both of its partial-sum rows over k_finalize's since k_init_scalars read them)
        res["bb"] = dot_ratio(s["bb"], b, b)
    else:
        res["bb_row"] = dot_ratio(row_sum(R["start_bb"]), b, b)
        res["bb"] = scalar_of_row(s["bb"], R["start_bb"])
    res["grid"] = flag(S0["counts"]["start_bb"] == grid_for(S0["n"]))
    t2 = tol2_rule(A["tol"], A["tol_cap"], A["bb_ref"], s["bb"])
    res["tol2"] = fig(kr.ratio(s["tol2"], t2, abs(t2)), C_TOL)
    res["scalars"] = flag(s["rr"] == s["bb"] and s["pq"] == 0.0 and s["alpha"] == 0.0 and s["beta"] == 0.0 and s["iter"] == 0
                          and s["iter_prev"] == 0 and s["maxit"] == int(A["maxit"]) and np.float64(s["rz_prev"]).tobytes() == np.float64(s["rz"]).tobytes())
    init_stop = 1 if s["bb"] == 0.0 else (0 if np.isfinite(s["bb"]) else 3)      # (k_init_scalars; its own r.z is finite with b)
    if warm:   # k_restart_scalars(keep_stop = 1) behind k_init_scalars
        rz = s["rz"]
        want = init_stop if init_stop else ((1 if rz == 0.0 else 0) if (np.isfinite(rz) and rz >= 0.0) else 3)
    else:
        want = init_stop if np.isfinite(s["rz"]) or init_stop == 1 else 3
    res["stop"] = flag(s["stop"] == want)
    return res


# ------------------------------------------------------------------ stages 2, 3, 5: one iteration
def check_step(prev, cur, prod_p, omega=None, xs0_kept=True):
    """Iteration k from run k (prev) and run k + 1 (cur); prod_p = (H p_k, abs) for cur's exported p."""
    k = prev["S"]["iter"]
    s0, s, R = prev["S"], cur["S"], cur["rows"]
    res = {}
    p, q = cur["p"], cur["q"]
    # 5 (of iteration k - 1): p_k = z_k + beta_{k-1} p_{k-1}; the start leaves p_0 and a stopping iteration leaves p alone
    if k == s0["iter_prev"] and s0["beta"] == 0.0 and s0["alpha"] == 0.0:        # prev is a start (or a restart): p_k = p as it stands
        res["p"] = bits(p, prev["p"])
    else:
        bt = LD(s0["beta"])
        res["p"] = fig(kr.ratio(p, prev["z"].astype(LD) + bt * prev["p"].astype(LD), np.abs(prev["z"]) + abs(s0["beta"]) * np.abs(prev["p"])), C_AXPY)
    # 2: the product and p.q
    res["q"] = fig(kr.ratio(q, prod_p[0], prod_p[1]), kr.C)
    res["pq_row"] = dot_ratio(row_sum(R["pq"]), p, q)
    res["pq"] = scalar_of_row(s["pq"], R["pq"])
    # 3: k_update_xr
    res["rz_prev"] = flag(np.float64(s["rz_prev"]).tobytes() == np.float64(s0["rz"]).tobytes() and s["iter_prev"] == k)
    if s["stop"] == 3 and s["iter"] == k:                                        # breakdown in k_update_xr: nothing else moves
        res["breakdown"] = flag(not (s["pq"] > 0.0) or not np.isfinite(s["pq"]))
        res["breakdown.x"] = bits(cur["x"], prev["x"])
        res["breakdown.r"] = bits(cur["r"], prev["r"])
        return res
    al = LD(s0["rz"]) / LD(s["pq"])
    res["alpha"] = fig(kr.ratio(s["alpha"], al, abs(float(al))), C_DIV)
    a = LD(s["alpha"])
    aa = abs(s["alpha"])
    res["x"] = fig(kr.ratio(cur["x"], prev["x"].astype(LD) + a * p.astype(LD), np.abs(prev["x"]) + aa * np.abs(p)), C_AXPY)
    res["r"] = fig(kr.ratio(cur["r"], prev["r"].astype(LD) - a * q.astype(LD), np.abs(prev["r"]) + aa * np.abs(q)), C_AXPY)
    zz, zabs = dinv_apply(cur["dinv"], cur["r"])
    if not cur["amg"]:
        res["z"] = fig(kr.ratio(cur["z"], zz, zabs), C_Z)
    elif cur["xs0"] is not None and xs0_kept:
        res["xs0"] = fig(kr.ratio(cur["xs0"], LD(omega) * zz, abs(omega) * zabs), C_XS)
    res["rr_row"] = dot_ratio(row_sum(R["rr"]), cur["r"], cur["r"])
    res["rr"] = scalar_of_row(s["rr"], R["rr"])
    res["rz_row"] = dot_ratio(row_sum(R["rz"]), cur["r"], cur["z"])
    res["rz"] = scalar_of_row(s["rz"], R["rz"])
    n = cur["n"]
    res["grid"] = flag(cur["counts"]["n_rr"] == grid_for(n))
    # 5: k_update_p's scalars
    if R["zq"].size:                                                             # flexible beta = -alpha z.q / rz_prev
        res["zq_row"] = dot_ratio(row_sum(R["zq"]), cur["z"], q)
        zq, zq_abs, m = ldot(cur["z"], q)
        bref = -a * zq / LD(s["rz_prev"])
        babs = min(C_DOT, m) * aa * zq_abs / abs(s["rz_prev"]) + 2.0 * abs(float(bref))
        res["beta"] = fig(kr.ratio(s["beta"], bref, babs), 1.0)
    else:
        bref = LD(s["rz"]) / LD(s["rz_prev"])
        res["beta"] = fig(kr.ratio(s["beta"], bref, abs(float(bref))), C_DIV)
    res["iter"] = flag(s["iter"] == k + 1 and s["maxit"] == int(cur["args"]["maxit"]) and s["bb"] == s0["bb"] and s["tol2"] == s0["tol2"])
    res["stop"] = flag(s["stop"] == stop_rule(s))
    # ... and iteration k ran at all: under this run's cap the scalars iteration k - 1 left must not have stopped the solve
    res["went_on"] = flag(k == 0 or stop_rule(dict(s0, maxit=s["maxit"], probe_k=s["probe_k"], probe_max=s["probe_max"])) == 0)
    if s["iter"] == s["probe_k"]:
        pr = LD(s["rr"]) / LD(s["bb"])
        res["probe_rel"] = fig(kr.ratio(s["probe_rel"], pr, abs(float(pr))), C_DIV)
    return res


def drift_terms(prev, cur, prod_p_abs, prod_scale_abs):
    """U-free growth of the drift bound over iteration k (module docstring); prod_scale_abs: abs(H (|x_k| + |alpha_k p_k|))"""
    aa = abs(cur["S"]["alpha"])
    return 2.0 * (np.abs(prev["r"]) + aa * np.abs(cur["q"])) + kr.C * aa * prod_p_abs + 2.0 * prod_scale_abs


def drift_scale_vector(prev, cur):
    return np.abs(prev["x"]) + abs(cur["S"]["alpha"]) * np.abs(cur["p"])


def check_drift(state, prod_x, D):
    """|b - H x - r| per entry against U (D + 16 abs(H x)) -- D accumulated by drift_terms; prod_x = (H x, abs) of state's x"""
    ref = state["b"].astype(LD) - prod_x[0]
    return fig(kr.ratio(state["r"], ref, D + kr.C * prod_x[1]), C_DRIFT)


# ------------------------------------------------------------------ stages 6, 7: records, the whole solve
def check_records(cur, lanczos_runs=None):
    """After a solve of >= 1 iterations: the pinned mirror and the host copy equal d_S bitwise; Lanczos row k of the run that made
    iteration k its last: (alpha_k, beta_k, rz_prev) bitwise (lanczos_runs: {k: state after run k + 1})."""
    res = {}
    c = cur["cmp"]
    res["host=d_S"] = flag(c["H"] == c["S"])
    if cur["S"]["iter"] >= 1:
        res["mirror=d_S"] = flag(c["M"] == c["S"])
    if cur["lanczos"] is not None:
        L = cur["lanczos"]
        s = cur["S"]
        res["lanczos.rows"] = flag(L.shape[0] == min(s["iter"], 2048))
        if s["iter"] >= 1 and s["iter"] <= 2048:
            last = np.array([s["alpha"], s["beta"], s["rz_prev"]])
            res["lanczos.last"] = bits(L[s["iter"] - 1], last)
        for k, st in (lanczos_runs or {}).items():
            if st["S"]["iter"] == k + 1 and k < L.shape[0]:
                t = st["S"]
                res[f"lanczos.{k}"] = bits(L[k], np.array([t["alpha"], t["beta"], t["rz_prev"]]))
    return res


def check_frozen(prev, cur):
    """A run with a later cap after a stop that no cap set: nothing may have moved (every kernel behind the flag leaves every array
    alone).  Every vector, partial-sum row and record bitwise, every scalar but the cap itself."""
    moved = same_bits(prev, cur, skip=("args", "counts", "S", "H", "M") + tuple("row." + k for k in prev["rows"]))
    for k, a in prev["rows"].items():     # (a row's exported length follows the launch bookkeeping: a start alone knows no iteration's)
        m = min(a.size, cur["rows"][k].size)
        if a[:m].tobytes() != cur["rows"][k][:m].tobytes():
            moved.append("row." + k)
    sc = [k for k in prev["S"] if k not in ("maxit", "pad") and np.float64(prev["S"][k]).tobytes() != np.float64(cur["S"][k]).tobytes()]
    return {"frozen": flag(not moved and not sc)}


def check_sequence(states, op, omega=None, xs0_kept=True, x_prev=None, drift=True, lanczos=True):
    """Stages 1-3, 5, 6 and the drift of stage 7 over the states of runs capped at consecutive iteration counts ({cap: state}, cap 0
    = the start alone).  -> {"stage@cap": figure}; every reference product of the case in one pass over its edges."""
    caps = sorted(states)
    assert caps[0] == 0
    pairs = [(a, b) for a, b in zip(caps[:-1], caps[1:]) if b == a + 1]
    steps = [(a, b) for a, b in pairs if states[a]["S"]["iter"] == a and states[a]["S"]["stop"] in (0, 2)
             and (states[b]["S"]["iter"] == b or states[b]["S"]["stop"] == 3)]
    warm = x_prev is not None
    xs, at = ([np.asarray(x_prev, dtype=np.float64).reshape(-1, 3)] if warm else []), {}
    for a, b in steps:
        at[b] = len(xs)
        xs.append(states[b]["p"])
        if drift and not warm:
            xs += [drift_scale_vector(states[a], states[b]), states[b]["x"]]
    prods = op.products(xs) if xs else []
    out = {}

    def add(res, cap):
        out.update({f"{k}@{cap}": v for k, v in res.items()})
    add(check_start(states[0], x_prev, prods[0] if warm else None, omega, xs0_kept), 0)
    D = np.zeros_like(states[0]["b"])
    for a, b in pairs:
        if (a, b) in steps:
            q = at[b]
            add(check_step(states[a], states[b], prods[q], omega, xs0_kept), b)
            if drift and not warm and states[b]["S"]["iter"] == b:
                D = D + drift_terms(states[a], states[b], prods[q][1], prods[q + 1][1])
                out[f"drift@{b}"] = check_drift(states[b], prods[q + 2], D)
        elif states[a]["S"]["stop"] in (1, 3, 4):
            add(check_frozen(states[a], states[b]), b)
    add(check_records(states[caps[-1]], {k: states[k + 1] for k in caps if k + 1 in states} if lanczos else None), caps[-1])
    return out


def relres_of(S):
    return float(np.sqrt(np.float64(S["rr"]) / np.float64(S["bb"]))) if S["bb"] > 0 else 0.0


def failures(res):
    return {k: v for k, v in res.items() if not v <= 1.0}


def worst(res_list):
    out = {}
    for res in res_list:
        for k, v in res.items():
            out[k] = max(out.get(k, 0.0), v)
    return out


# ------------------------------------------------------------------ the fp64 numpy model of the recurrence (CPU tests)
def _block_dot(a, b, short=False):
    """per-256-row partial sums of a . b, as one workgroup each"""
    n = a.shape[0]
    starts = range(0, n, BLOCK)
    row = np.zeros(grid_for(n))                                      # (workgroups past the last row store a zero)
    for k, s in enumerate(starts):
        row[k] = np.dot(a[s:s + BLOCK].ravel(), b[s:s + BLOCK].ravel())
    return row[:len(starts) - 1] if short else row


def _state(n, b, x, r, z, p, q, dinv, xs0, S, rows, counts, args, amg, lanczos):
    st = dict(n=n, amg=amg, b=b.copy(), x=x.copy(), r=r.copy(), z=z.copy(), p=p.copy(), q=q.copy(), dinv=dinv, xs0=None if xs0 is None else xs0.copy(),
              S=dict(S), H=dict(S), M=dict(S), rows={k: np.array(v, dtype=np.float64) for k, v in rows.items()}, counts=dict(counts), args=dict(args),
              lanczos=None if lanczos is None else np.array(lanczos).reshape(-1, 3))
    st["cmp"] = _comparable(st)
    return st


MUTATIONS = ("beta_stale_rz_prev", "alpha_short_row", "z_from_old_r", "p_updated_on_stop", "plain_beta_variable_precond", "tol2_uncapped",
             "gamma_above_4", "gamma_negative", "xs0_without_omega", "rr_from_rz", "probe_against_rz", "stop_not_frozen",
             "x_with_old_alpha", "r_plus_alpha_q")


def model(matvec, b, dinv, caps, tol=1e-8, tol_cap=1e-6, bb_ref=0.0, precond=None, omega=0.8, x_prev=None, probe_k=0, probe_max=0.0,
          mutate=None, record=True):
    """The recurrence in plain fp64 numpy, one state per cap in `caps` (0: the start alone), in export_state's format.  matvec(x) ->
    H x (fp64).  precond(r, k) -> z: a (variable) preconditioner in the multigrid's place (then xs0 = omega Dinv r is left too and
    beta is the flexible one); None: block-Jacobi.  mutate: one of MUTATIONS."""
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    amg = precond is not None
    D = lambda v: dinv_apply(dinv, v, np.float64)[0]                 # noqa: E731
    grid = grid_for(n)
    counts = dict(start_bb=grid, start_rz=grid, n_pq=0, n_rz=0, n_rr=0, n_zq=0, n_xq=0, n_bx=0)
    states = {}
    x, r = np.zeros_like(b), b.copy()
    q = np.zeros_like(b)
    rows = dict(start_bb=_block_dot(b, b), start_rz=[0.0], xq=[], bx=[], pq=[], rr=[], rz=[], zq=[])
    bb = float(np.sum(rows["start_bb"]))
    t2 = tol2_rule(tol, tol_cap, bb_ref, bb, capped=mutate != "tol2_uncapped")
    stop = 1 if bb == 0.0 else 0
    if x_prev is not None:
        xp = np.asarray(x_prev, dtype=np.float64)
        q = matvec(xp)
        rows["xq"], rows["bx"] = _block_dot(xp, q), _block_dot(b, xp)
        counts["n_xq"] = counts["n_bx"] = grid
        xq, bx = float(np.sum(rows["xq"])), float(np.sum(rows["bx"]))
        g = gamma_rule(bx, xq)
        with np.errstate(all="ignore"):
            if mutate == "gamma_above_4" and xq > 0 and bx / xq > 4.0:
                g = bx / xq
            if mutate == "gamma_negative" and xq > 0 and bx / xq < 0.0:
                g = bx / xq
        x, r = g * xp, b - g * q
    z0 = D(r)
    xs0 = None
    if amg:
        xs0 = z0 if mutate == "xs0_without_omega" else omega * z0
        z = precond(r, 0)
    else:
        z = z0
    p = z.copy()
    rows["start_rz"] = _block_dot(r, z)
    rz = float(np.sum(rows["start_rz"]))
    if x_prev is not None and not stop:
        stop = (1 if rz == 0.0 else 0) if (np.isfinite(rz) and rz >= 0.0) else 3
    S = dict(rz=rz, pq=0.0, rr=bb, bb=bb, alpha=0.0, beta=0.0, tol2=t2, rz_prev=rz, iter=0, maxit=0, stop=stop, iter_prev=0,
             probe_k=probe_k, probe_rel=0.0, probe_max=probe_max)
    args = dict(tol=tol, tol_cap=tol_cap, bb_ref=bb_ref, maxit=0)
    lanczos = [] if record else None
    rz_hist = [rz]
    alpha_old = 0.0
    BIG = 10 ** 6                                                      # (pcg_maxit: no cap)
    S["maxit"] = args["maxit"] = BIG
    for cap in sorted(caps):
        # the one trajectory carried on to `cap` iterations; S["stop"] is the decision without a cap, and p is updated lazily, at the
        # start of the next iteration: a snapshot holds the p its last iteration used, as a capped or stopped run does
        while S["iter"] < cap and (S["stop"] == 0 or (mutate == "stop_not_frozen" and S["stop"] in (1, 4))):
            k = S["iter"]
            p = S.pop("p_next", p)
            q = matvec(p)
            rows["pq"] = _block_dot(p, q, short=mutate == "alpha_short_row")
            pq = float(np.sum(rows["pq"])) if len(rows["pq"]) else 0.0
            S.update(pq=pq, rz_prev=S["rz"], iter_prev=k)
            counts.update(n_pq=len(rows["pq"]), n_rr=grid, n_rz=grid, n_zq=grid if amg else 0)
            if not (pq > 0.0) or not np.isfinite(pq):
                S["stop"] = 3
                break
            alpha = S["rz"] / pq
            S["alpha"] = alpha
            r_old = r
            x = x + (alpha_old if mutate == "x_with_old_alpha" else alpha) * p
            r = r + alpha * q if mutate == "r_plus_alpha_q" else r - alpha * q
            alpha_old = alpha
            zsrc = r_old if mutate == "z_from_old_r" else r
            z0 = D(zsrc)
            if amg:
                xs0 = z0 if mutate == "xs0_without_omega" else omega * z0
                z = precond(zsrc, k + 1)
            else:
                z = z0
            rows["rr"], rows["rz"] = _block_dot(r, r), _block_dot(r, z)
            rz, rr = float(np.sum(rows["rz"])), float(np.sum(rows["rr"]))
            if mutate == "rr_from_rz":
                rr = rz
            rz_hist.append(rz)
            rzp = rz_hist[-3] if (mutate == "beta_stale_rz_prev" and len(rz_hist) >= 3) else S["rz_prev"]
            if amg:
                rows["zq"] = _block_dot(z, q)
            if amg and mutate != "plain_beta_variable_precond":
                beta = -alpha * float(np.sum(rows["zq"])) / rzp
            else:
                beta = rz / rzp
            S.update(beta=beta, rz=rz, rr=rr, iter=k + 1)
            st = stop_rule(S)
            if mutate == "probe_against_rz" and k + 1 == probe_k and probe_max > 0.0 and st in (0, 4):
                st = 4 if rz > probe_max * bb else 0
            if k + 1 == probe_k:
                S["probe_rel"] = rr / bb
            if lanczos is not None:
                lanczos.append([alpha, beta, S["rz_prev"]])
            S["stop"] = st
            S["p_next"] = z + beta * p
            if mutate == "p_updated_on_stop":
                p = S["p_next"]
        snap = {k: v for k, v in S.items() if k != "p_next"}
        snap["maxit"] = cap if cap > 0 else BIG
        if cap > 0 and snap["iter"] >= cap and snap["stop"] in (0, 4) and snap["iter"] == cap:
            snap["stop"] = 2 if snap["stop"] == 0 or mutate != "probe_against_rz" else snap["stop"]
        states[cap] = _state(n, b, x, r, z, p, q, dinv, xs0, snap, rows, counts, dict(args, maxit=snap["maxit"]), amg,
                             None if lanczos is None else lanczos[:snap["iter"]])
    return states
