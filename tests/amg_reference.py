"""Stage-by-stage reference for the multigrid refresh and its cycle (CPU only, test infrastructure; sibling of kernel_reference.py).

What it checks.  The hierarchy sgo_debug_amg_array exports (include/sgo.h) -- per level the operator, positions, lever arms,
partition, transfer P with its streamed fp32 copies, the filter's mask and D_F, A P, the folded transfer P~, and the coarsest
dense inverse -- stage by stage in the order amg_update / level_values (sgo_amg.hip) run them.  The input of every stage is the
DEVICE's exported output of the stage before it, so a stage's bound is the rounding bound of that stage alone, with no condition
number in it (the exceptions are the matrix inverses, below).  The reference restates formulas only: the partition `agg` is
taken as given, and whether a level is smoothed, filtered, tentative or folded is read from the exported flags.

Arithmetic.  Blocks, positions and lever arms are the exported fp64 values; products of 3x3 blocks and every sum are evaluated in
np.longdouble (x86-64: eps 1.08e-19, asserted in kernel_reference), so the reference's own rounding is 2^-11 of fp64's and every
output entry y gets  |y_device - y_ref| <= C_stage * U * abs(y),  U = 2^-53, abs(y) the same expression evaluated on magnitudes.
Large stages run in chunks of CHUNK block products.

The stages, with the comment in sgo_amg.hip that states the formula (T(d), B T(d), T(d)^T M and the cofactor inverse of a
symmetric block are stated once, in sgo_device.h under "the arithmetic of the multigrid cycle"):
1 partition   agg maps onto [0, nc), every aggregate non-empty, (mem_ptr, mem) lists the same partition.
2 geometry    (k_positions0, k_centres) level-0 pos = the free poses' xy, bitwise; pos_{l+1}[a] = mean of its members: the kernel
              forms sum * (1 / count), lanes then a wave tree: abs = sum |pos| / count; d_i = pos_i - c_agg(i) with the exported
              centres: one rounding, abs = |pos_i| + |c|.
3 filtered    (k_filtered_diag) D_F,i = D_i + sum_{weak k=(i,j)} A_k T(p_j - p_i), T(d) = [[1,0,-d_y],[0,1,d_x],[0,0,1]]; a row
              without a kept off-diagonal slot keeps D_i.  abs: |D| + sum |A_k| |T|(|p_j - p_i|).  dinvF is the inverse of the
              exported dF (per block  |dinvF - dF^-1|_2 <= C_INV U kappa |dF^-1|_2, kappa = |dF^-1|_2 | |dF| |_2: the cofactor
              inverse's error grows with the block's own condition, as in the block-Jacobi test) or exactly zero; a zero row needs
              one of the two documented reasons: no kept off-diagonal slot, or trace(D^-1 L) > 0.5 with L = -sum of the weak
              terms (rows within TRACE_BAND of 0.5 either way).  The mask: w_ij >= theta_f sqrt(w_ii w_jj) on Frobenius norms
              (host_coarsen / k_filter_mask; slots within MASK_BAND relative of the threshold either way; only where the mask was
              made from the exported values, i.e. before any optimize()).
4 transfer    (k_p_values) P_e = [col(e) = agg(i)] T(d_i) - omega_p Dinv_i sum_{k in e} A_k T(d_col(k)); filtered levels: kept slots,
              D_F in place of the diagonal slot's block and dinvF (a zero dinvF row gives T(d_i)).  abs = [..] |T(d_i)| +
              omega_p |Dinv_i| sum |A_k| |T(d_col(k))|.  The pattern is exactly {(i, agg(j))} over the listed slots plus the
              own-aggregate entry, rows ascending, columns ascending, nothing doubled.
5 copies      (k_p_values' stores) r_blk[e] == float32(blk[e]) == t_blk[t_pos[e]] bitwise; t_row / t_col agree with row / col; t_pos
              is a permutation that sorts by column.
6 Galerkin    (k_block_products) AP_f = sum A_k P_e over k = (i, j), e = (j, c): complete pattern; A_{l+1}(a, c) = sum P_e^T AP_f
              over e = (i, a), f = (i, c) on the slots c >= a, the others bitwise transposes; tentative levels (k_galerkin)
              A_{l+1}(a, c) = sum T_i^T A_k T_j over the slots with agg(i) = a, agg(j) = c.  abs: the same sums on magnitudes.
              dinv of level l+1 (k_level_dinv, dinv_from_block): inverse of its SYMMETRISED diagonal blocks (D + D^T) / 2 -- the diagonal slot is
              summed in full, symmetric only up to the Galerkin sum's rounding, which is U abs of that sum and not U |D|: next to
              closures of 10^10 the two inverses differ by 10^4 U kappa --, bound as dinvF's.
7 folded      (k_ptilde_values) P~_f = P_(row, col) - omega Dinv_i AP_f on A P's pattern; the two fp32 copies agree bitwise and lie
              within 2^-24 |ref| + 2^-126 + C U abs of the reference (one fp32 rounding of an fp64 value within the stage's bound;
              2^-126, fp32's smallest normal: below it the conversion rounds absolutely or flushes to zero -- reached on levels
              1-2 of hierarchies from a dead-reckoned start, where DCS has switched closures off and their weights compound).
8 coarsest    (k_dense_fill_unique, k_gj_*) the exported inverse against the exported coarsest operator, per column in the 2-norm:
              |inv e_k - H^-1 e_k| <= C_DENSE N U kappa_2(H) |H^-1 e_k|, the bound and constant of
              test_single_level_hierarchy_is_the_exact_inverse.
9 cycle       z = M r in long double from the exported arrays as stored (fp32 transfers, the fp32 level-0 copy where the passes
              read it, fp64 elsewhere), in the form each level runs ("folded V-cycle" in sgo_amg.hip, cycle_form):
              unfolded, nu sweeps per side: x = 0; nu x [x += w Dinv res; res -= A (w Dinv res)]; x += P cycle(P^T res);
                                            nu x [x += w Dinv (r - A x)];
              folded:               z = x1 + w Dinv (r - A x1) + P~ cycle(P~^T r), x1 = w Dinv r;
              folded in two sweeps: x1 = w Dinv r; t = x1 + folded(r - A x1); z = t + w Dinv (r - A t);
              coarsest level: the exported inverse.  A tentative transfer restricts with sum_{i in a} T(d_i)^T res_i and
              prolongates with x_i += T(d_i) w[agg(i)], on the exported fp64 lever arms.
              The driver is coarse_solve()'s, read from the exported flags: the last level is the dense inverse; a smoothed level
              l > kdepth is walked by the V-cycle; every other level (a tentative one always) by fcg(), Notay's flexible CG:
                z1 = cycle(bk), q = A z1, a1 = (z1.bk)/(z1.q);  one step, x = a1 z1, where l > fcg2_depth;  otherwise
                bk2 = bk - a1 q, z2 = cycle'(bk2), b = (q.z2)/(z1.q), p2 = z2 - b z1, q2 = A p2, a2 = (p2.bk2)/(p2.q2), x = a1 z1 + a2 p2;
              a coefficient whose denominator is not positive, or not finite, is 0 (cycle_ratio).  The form of each inner cycle
              follows cycle_form by call site: cycle' (it carries the right-hand-side update and a dot request) is unfolded with
              nu sweeps per side, the first cycle of a folded level stays folded.
              There is no entry-wise bound through a composition with an inverse: per case the measure is
              |z_gpu - z_ref|_2 / |z_ref|_2 against K_CYCLE * eps_case (K_KCYCLE where a level runs fcg(): the K-cycle is
              nonlinear in r), eps_case the same norm between this reference in plain fp64 and in long double (the rounding
              scale of the hierarchy, from the reference alone).
10 kcycle     per-step checks on the work vectors sgo_debug_amg_array exports (SGO_AMG_W_*) as the last sgo_precondition left
              them: every level's LAST visit (a level >= 2 is visited several times per cycle; every level's last visit lies
              inside its parent's last visit, so the chain below is self-consistent).  Each step takes the DEVICE's exported
              inputs: |got - ref| <= C U abs entry-wise, abs the same expression on magnitudes.
              restrict   bk_{l+1} against the residual the level's last cycle restricted (which buffer: _last_visit), tentative:
                         abs = sum |T|^T |res|; smoothed / folded: through the exported fp32 copies t_blk / ps_t as stored.
              product    q = A z1, q2 = A p2.
              dots       the long-double sum of the exported partial sums [0, g) against the long-double dot product:
                         |delta| <= C_DOT U sum |a_i b_i| for pA = (z1.q | z1.bk), pC = (q.z2), pB = (p2.q2 | p2.bk2); entries
                         beyond the exported grid counts are not read; a step that ran has g > 0, one that did not has g = 0.
              bk2, p2    bk2 = bk - a1 q, p2 = z2 - b z1 with a1, b recomputed from the exported partial sums in fp64 IN THE
                         KERNEL'S ORDER (block_reduce_parts_n: thread t of 256 adds entries t, t + 256, ... serially from 0.0;
                         wave_sum is a balanced tree over adjacent lanes; thread 0 adds the four waves' sums in order): reduce_parts.
                         That order is k_spmv's (ratios2), which makes bk2 and p2: there the coefficient is reproduced bit for bit.
                         k_prolong_fold (level 0's folded last launch) reduces the same partial sums in a loop of its own over
                         kFoldThreads = 1024 threads and 16 waves; the reference does not restate that order, so in that launch
                         the coefficients agree to a few ulps only, which C_K['last'] holds with the launch's own rounding.
              last       the level's last launch(es), out = x' + w Dinv (rhs - A x'), x' = xs + T (c1 u1 + c2 u2), abs = |x'| +
                         w |Dinv| (|rhs| + |A| |x'|); out is the parent's z1 / z2 / xk, on level 0 the returned z.  Which buffer
                         holds what: a tentative level >= 1 below kUnfuseSlots slots fuses the prolongation into the sweep
                         (SPMV_JACOBI_P) and leaves xs as the pre-smoothing left it; everywhere else (level 0, k_prolong_p,
                         k_prolong_add on a large level) the prolongation updates xs IN PLACE, the exported xs is x' itself and
                         is checked against the pre-smoothing sweeps recomputed from rhs; with nu = 2 the first post-smoothing
                         sweep lands in rs (the restricted residual is then tR's).  Folded forms: out = M2 rhs + P~ w (k_up_fold),
                         on level 0 z = rs + P~ w with rs = M2 r (k_prolong_fold).
              coarsest   xk = inv bk entry-wise, abs = |inv| |bk|.
              rules      r = 0 leaves every exported vector and z exactly zero; a denominator <= 0 gives the coefficient 0.

Constants.  Each C is a small multiple of the worst error / (U abs) measured on the MI355X over the cases of
tests/test_gpu_amg_reference.py (recorded there per case class), at least 2 x and at most 8 x of it; the CPU mutation tests
(tests/test_amg_reference.py) require every mutation to be rejected at >= 10 C.  See MEASURED below.
"""
from __future__ import annotations

import ctypes as C_

import numpy as np

from kernel_reference import LD, U

CHUNK = 1_500_000
TRACE_BAND = 1e-9
MASK_BAND = 1e-12
BAND_SHARE = 1e-3          # rows / slots a band may excuse, of the level's rows
C_DENSE = 0.5              # test_single_level_hierarchy_is_the_exact_inverse's
F32_TINY = 2.0 ** -126     # smallest normal fp32: below it a conversion from fp64 rounds absolutely (or flushes to zero), not relatively
# Measured on the MI355X (tests/test_gpu_amg_reference.py, 26 cases), worst error / (U abs) per stage and case class:
#   class      geometry  filtered  inverse  transfer  galerkin  folded  cycle / eps_case
#   small      3.16      -         0.44     3.91      3.49      0       1.18     (C1, C2 and C2 under every producer / switch)
#   filtered   2.68      1.85      1.39     4.01      5.72      0.45    1.06     (C2 from the dead-reckoned start, every producer / switch,
#                                                                                and with three poses between heavy neighbours)
#   large      3.34      -         0.48     4.37      5.08      0       1.72     (30k/300k, 70k/250k, C4, 24k with fixed + duplicates)
#   tentative  3.14      -         0.43     3.50      4.20      0       -        (20k random closures, hubs, C4r)
# the coarsest inverse: 0.25 of its normwise bound next to the 10^10 closures, below 1e-3 elsewhere.  folded: the figure is what is
# left of the error after the fp32 rounding 2^-24 |ref| (+ the underflow threshold F32_TINY: on the dead-reckoned hierarchies
# entries of P~ on levels 1-2 lie below fp32's normal range, where the stored value is 0 or a subnormal and the error is absolute).
# inverse: the kernels' cofactor inverses measure 1.39 next to the 10^10 closures (0.53 without them); numpy's LU inverse of the
# forward-built CPU hierarchy with such closures (blocks of kappa ~ 1e8) measures 2.25 of the same bound: 4 holds both.
MEASURED = dict(geometry=3.34, filtered=1.85, inverse=1.39, transfer=4.37, galerkin=5.72, folded=0.447, cycle=1.72)
C_STAGE = dict(geometry=8.0, filtered=6.0, inverse=4.0, transfer=16.0, galerkin=16.0, folded=2.0)   # 2.4, 3.2, 2.9, 3.7, 2.8, 4.5 x measured
# Stage 10 and the K-cycle's end-to-end figure, measured on the MI355X (tests/test_gpu_kcycle_reference.py, the three tentative cases
# of tests/test_gpu_amg_reference.py and amg_c2_kcycle of tests/test_gpu_pcg_reference.py), worst error / (U abs) per step and case class:
#   class      restrict  product  dots   bk2    p2     last   coarsest  cycle / eps_case
#   tentative  2.72      2.80     0.58   1.00   0.99   3.31   1.92      6.25    (SGO_AMG_SMOOTH=0: C2, 20k random closures, the same with
#                                                                               fcg2_depth 0 and 9, C4r with its 627-member aggregate)
#   smoothed   3.01      2.51     0.64   1.00   1.00   4.92   0.68      20.27   (SGO_AMG_KDEPTH = 2, 1 on C2 and on 30k / 300k, and with
#                                                                               two steps on level 2; amg_c2_kcycle over its caps: 7.35)
#   mixed      3.33      2.79     0.44   1.00   0.99   3.79   0.98      4.07    (defaults: 20k random closures, hubs, C4r)
# (every case with the full vector set: two random vectors, rows scaled by 10^+-6, a single non-zero row.)
# bk2, p2: one fused multiply-add per entry with the coefficient reproduced bit for bit (reduce_parts): half an ulp of the result, 1 in
# these units only where the two terms cancel; the fp64 forward model of the CPU tests, which rounds twice, measures 1.6.  cycle: the
# V-cycle measures 1.72; the K-cycle's coefficients are ratios of dot products, so z is not linear in r and one fp64 evaluation lies
# further from another than a V-cycle's does -- the CPU forward model, fp64 with other summation orders and no kernel in it, lies
# 4.9 eps_case from the long-double reference on the 600-pose mixed hierarchy.  eps_case is ONE fp64 evaluation's distance from the
# reference, a sample of the rounding scale and not a bound on it: over the four vectors of 30k / 300k under SGO_AMG_KDEPTH=1 it is
# 2.7e-7, 1.5e-7, 6.1e-9 and 1.2e-7.  20.27 is that case's vector with rows scaled by 10^+-6, the one whose sample came out at 6.1e-9:
# the device's error there is 1.2e-7, inside the spread of the same case's other samples, and every step of that run is within
# 4.87 U abs, so the figure is the measure's, not a step's.  The same holds for C2's scaled vector under SGO_AMG_KDEPTH=2 (9.31,
# eps_case 1.3e-10 against 5e-10 to 9e-10 on its other vectors, every step within 4.85 U abs).
MEASURED_K = dict(restrict=3.33, product=2.80, dots=0.644, bk2=0.996, p2=0.996, last=4.92, coarsest=1.92, cycle=20.27)
C_K = dict(restrict=8.0, product=8.0, dots=2.0, bk2=2.5, p2=2.5, last=12.0, coarsest=4.0, grids=1.0)   # 2.4, 2.9, 3.1, 2.5, 2.5, 2.4, 2.1 x measured
C_DOT = C_K["dots"]
K_KCYCLE = 48.0                                                                                     # 2.4 x measured
K_CYCLE = 8.0                                                                                       # 4.6 x measured

NAMES = ("INFO A_ROWPTR A_COL A_BLK A_BLK_F32 A_DINV POS D AGG MEM_PTR MEM P_ROWPTR P_ROW P_COL P_BLK P_RBLK P_TBLK P_TPOS P_TROW "
         "P_TCOL STRONG DF DINVF AP_A AP_B AP_TGT AP_BLK PS_ROW PS_COL PS_RBLK PS_TBLK PS_TROW PS_TCOL PS_STPOS INV ROW_ORDER "
         "W_XS W_RS W_TR W_BK W_XK W_Z1 W_Q W_BK2 W_Z2 W_P2 W_Q2 W_PA W_PB W_PC W_GRIDS").split()
WHAT = {k: i for i, k in enumerate(NAMES)}           # SGO_AMG_* of include/sgo.h
INFO = ("n nslot nc smoothed filtered folded kind nu omega omega_p np nap nval n_ap_prod n_rap_prod levels f32 N Np t_nlong "
        "ps_t_nlong kdepth theta_filter nslot_c fcg2_depth").split()
WORK = ("xs rs tR bk xk z1 q bk2 z2 p2 q2").split()           # SGO_AMG_W_* vectors [n][3]; pA pB pC [2][MAX_PARTS]; grids (gA, gB, gC)
MAX_PARTS = 2048                                              # kMaxPartials
UNFUSE_SLOTS = 400000                                         # kUnfuseSlots (sgo_amg.hip)
UNFOLDED, FOLDED, FOLDED2 = 0, 1, 2


# ------------------------------------------------------------------ export (the only part that touches the library)
def _fetch(opt, level, what, dtype):
    from sparse_gslam_amd import capi
    L = capi.lib()
    size = L.sgo_debug_amg_array(opt._h, level, WHAT[what], None, 0)
    if size < 0:
        raise capi.SgoError(f"sgo_debug_amg_array({level}, {what}): {size}: {opt.last_error()}")
    if size == 0:
        return None
    out = np.empty(size // np.dtype(dtype).itemsize, dtype=dtype)
    got = L.sgo_debug_amg_array(opt._h, level, WHAT[what], out.ctypes.data_as(C_.c_void_p), out.nbytes)
    assert got == size, (level, what, got, size)
    return out


def _unquad(raw):
    """A streamed fp32 copy as stored (components 0..3 [m][4], 4..7 [m][4], 8 [m]) -> (m, 9)."""
    m = raw.size // 9
    return np.concatenate([raw[:4 * m].reshape(m, 4), raw[4 * m:8 * m].reshape(m, 4), raw[8 * m:].reshape(m, 1)], axis=1)


def export_hierarchy(opt):
    """Every level of opt's resident hierarchy as a dict (keys as in the module docstring's stages), [] without one."""
    info0 = _fetch(opt, 0, "INFO", np.float64)
    if info0 is None:
        return []
    levels = []
    for l in range(int(info0[INFO.index("levels")])):
        v = _fetch(opt, l, "INFO", np.float64)
        L = {k: (float(x) if k in ("omega", "omega_p", "theta_filter") else int(x)) for k, x in zip(INFO, v)}
        i32, f64, f32 = np.int32, np.float64, np.float32
        for key, what, dt in (("rowptr", "A_ROWPTR", i32), ("col", "A_COL", i32), ("blk", "A_BLK", f64), ("blk32", "A_BLK_F32", f64),
                              ("dinv", "A_DINV", f64), ("pos", "POS", f64), ("d", "D", f64), ("agg", "AGG", i32),
                              ("mem_ptr", "MEM_PTR", i32), ("mem", "MEM", i32), ("p_rowptr", "P_ROWPTR", i32), ("p_row", "P_ROW", i32),
                              ("p_col", "P_COL", i32), ("p_blk", "P_BLK", f64), ("r_blk", "P_RBLK", f32), ("t_blk", "P_TBLK", f32),
                              ("t_pos", "P_TPOS", i32), ("t_row", "P_TROW", i32), ("t_col", "P_TCOL", i32), ("strong", "STRONG", np.uint8),
                              ("dF", "DF", f64), ("dinvF", "DINVF", f64), ("ap_a", "AP_A", i32), ("ap_b", "AP_B", i32),
                              ("ap_tgt", "AP_TGT", i32), ("apblk", "AP_BLK", f64), ("ps_row", "PS_ROW", i32), ("ps_col", "PS_COL", i32),
                              ("ps_r", "PS_RBLK", f32), ("ps_t", "PS_TBLK", f32), ("ps_trow", "PS_TROW", i32), ("ps_tcol", "PS_TCOL", i32),
                              ("ps_stpos", "PS_STPOS", i32), ("inv", "INV", f64), ("row_order", "ROW_ORDER", i32)):
            a = _fetch(opt, l, what, dt)
            if a is not None:
                L[key] = a
        for k in ("blk", "blk32", "p_blk", "apblk", "dF", "dinvF"):
            if k in L:
                L[k] = L[k].reshape(-1, 3, 3)
        for k in ("pos", "d"):
            if k in L:
                L[k] = L[k].reshape(-1, 2)
        L["dinv"] = L["dinv"].reshape(-1, 6)
        for k in ("r_blk", "t_blk", "ps_r", "ps_t"):
            if k in L:
                L[k] = _unquad(L[k])
        if "inv" in L:
            L["inv"] = L["inv"].reshape(L["Np"], L["Np"])
        if L["smoothed"]:
            # the pattern of A P as the product list numbers it: entry tgt sits at (row of slot a, column of P entry b)
            row = slot_rows(L)
            t, fr, fc = L["ap_tgt"], row[L["ap_a"]], L["p_col"][L["ap_b"]]
            ar = np.full(L["nap"], -1, dtype=np.int64)
            ac = np.full(L["nap"], -1, dtype=np.int64)
            ar[t], ac[t] = fr, fc
            L["ap_list_consistent"] = bool(np.array_equal(ar[t], fr) and np.array_equal(ac[t], fc) and (ar >= 0).all())
            if L["folded"]:
                L["ap_list_consistent"] &= bool(np.array_equal(ar, L["ps_row"]) and np.array_equal(ac, L["ps_col"]))
            L["ap_row"], L["ap_col"] = ar, ac
        levels.append(L)
    return levels


# ------------------------------------------------------------------ helpers
def slot_rows(L):
    return np.repeat(np.arange(L["n"], dtype=np.int64), np.diff(L["rowptr"]))


def T_of(d, dtype=np.float64):
    d = np.asarray(d)
    T = np.zeros((d.shape[0], 3, 3), dtype=dtype)
    T[:, 0, 0] = T[:, 1, 1] = T[:, 2, 2] = 1
    T[:, 0, 2] = -d[:, 1]
    T[:, 1, 2] = d[:, 0]
    return T


def sym6(p, dtype=np.float64):
    p = np.asarray(p)
    M = np.empty((p.shape[0], 3, 3), dtype=dtype)
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = p[:, 0], p[:, 1], p[:, 2]
    M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = p[:, 1], p[:, 3], p[:, 4]
    M[:, 2, 0], M[:, 2, 1], M[:, 2, 2] = p[:, 2], p[:, 4], p[:, 5]
    return M


def bmm(X, Y, dtype=LD):
    """Block products X_k Y_k with long-double products and sums."""
    return np.einsum("kij,kjl->kil", np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype))


def seg_add(acc, tgt, vals):
    """acc[tgt[t]] += vals[t] with the segment sums in vals' dtype."""
    if tgt.size == 0:
        return
    order = np.argsort(tgt, kind="stable")
    t = tgt[order]
    starts = np.flatnonzero(np.r_[True, t[1:] != t[:-1]])
    acc[t[starts]] += np.add.reduceat(vals[order], starts, axis=0)


def expand(starts, counts):
    """Indices starts[q] .. starts[q] + counts[q] - 1 for every q, concatenated, and the q of each."""
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    q = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
    first = np.r_[0, np.cumsum(counts)[:-1]]
    return np.asarray(starts, dtype=np.int64)[q] + (np.arange(total, dtype=np.int64) - first[q]), q


def lookup(sorted_keys, order, keys):
    """Position (in the unsorted array) of every key, -1 where it is absent."""
    if sorted_keys.size == 0:
        return np.full(keys.shape, -1, dtype=np.int64)
    p = np.minimum(np.searchsorted(sorted_keys, keys), sorted_keys.size - 1)
    return np.where(sorted_keys[p] == keys, order[p], -1)


def inv3(M):
    """Long-double cofactor inverse of (m,3,3) blocks and their determinants."""
    M = np.asarray(M, dtype=LD)
    c = np.empty_like(M)
    for r in range(3):
        for s in range(3):
            r1, r2, s1, s2 = (r + 1) % 3, (r + 2) % 3, (s + 1) % 3, (s + 2) % 3
            c[:, s, r] = M[:, r1, s1] * M[:, r2, s2] - M[:, r1, s2] * M[:, r2, s1]     # adjugate
    det = M[:, 0, 0] * c[:, 0, 0] + M[:, 0, 1] * c[:, 1, 0] + M[:, 0, 2] * c[:, 2, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return c / det[:, None, None], det


class Result(dict):
    """{check name: (ratio error / (U abs) or 0 / inf for an exact check, where)}."""

    def put(self, name, ratio, where=None):
        self[name] = (float(ratio), where)

    def exact(self, name, ok, where=None):
        self[name] = (0.0 if ok else float("inf"), where)

    def worst(self):
        return max((v[0] for v in self.values()), default=0.0)


def entry_ratio(got, ref, abs_sum, extra=None):
    """Worst |got - ref| / (U abs) over the entries and its index; extra: an allowance subtracted from the error first."""
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    if extra is not None:
        err = np.maximum(err - extra, 0.0)
    if err.size == 0:
        return 0.0, None
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(abs_sum > 0, err / (U * abs_sum), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isfinite(np.asarray(got, dtype=np.float64)), r, np.inf)
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[at]), tuple(int(q) for q in at)


def inverse_ratio(got, M):
    """Worst per-block |got - M^-1|_2 / (U kappa |M^-1|_2), kappa = |M^-1|_2 | |M| |_2."""
    if len(M) == 0:
        return 0.0, None
    ref, _ = inv3(M)
    ref64 = ref.astype(np.float64)
    kappa = np.linalg.norm(ref64, 2, axis=(1, 2)) * np.linalg.norm(np.abs(np.asarray(M, dtype=np.float64)), 2, axis=(1, 2))
    err = np.linalg.norm((np.asarray(got, dtype=LD) - ref).astype(np.float64), 2, axis=(1, 2))
    r = err / (U * kappa * np.linalg.norm(ref64, 2, axis=(1, 2)))
    r = np.where(np.isfinite(r), r, np.inf)
    at = int(np.argmax(r))
    return float(r[at]), (at,)


# ------------------------------------------------------------------ stages 1-8
def stage1_partition(L):
    R = Result()
    n, nc, agg = L["n"], L["nc"], L["agg"]
    ok = agg.size == n and nc > 0 and agg.min() >= 0 and agg.max() < nc and (np.bincount(agg, minlength=nc) > 0).all()
    R.exact("partition.onto", ok)
    mp, mem = L["mem_ptr"], L["mem"]
    ok = (mp.size == nc + 1 and mp[0] == 0 and mp[-1] == n and (np.diff(mp) > 0).all() and mem.size == n
          and np.array_equal(np.sort(mem), np.arange(n)) and np.array_equal(agg[mem], np.repeat(np.arange(nc), np.diff(mp))))
    R.exact("partition.members", bool(ok))
    return R


def stage2_geometry(L, Nx, poses_xy=None):
    """poses_xy: level 0's expected positions (the free poses' xy in the level's row order)."""
    R = Result()
    if poses_xy is not None:
        R.exact("geometry.pos0", np.array_equal(L["pos"], poses_xy))
    pos, agg, nc = L["pos"], L["agg"], L["nc"]
    cnt = np.bincount(agg, minlength=nc).astype(np.float64)
    s = np.zeros((nc, 2), dtype=LD)
    a = np.zeros((nc, 2))
    seg_add(s, agg.astype(np.int64), pos.astype(LD))
    seg_add(a, agg.astype(np.int64), np.abs(pos))
    R.put("geometry.centres", *entry_ratio(Nx["pos"], s / cnt[:, None], a / cnt[:, None]))
    c = Nx["pos"][agg]
    R.put("geometry.lever", *entry_ratio(L["d"], pos.astype(LD) - c.astype(LD), np.abs(pos) + np.abs(c)))
    return R


def _weak_sums(L):
    """Per row: sum over its weak off-diagonal slots of A_k T(p_j - p_i) (long double), its magnitudes, kept off-diagonal slots."""
    n, row, col = L["n"], slot_rows(L), L["col"].astype(np.int64)
    off = col != row
    weak = off & (L["strong"] == 0)
    k = np.flatnonzero(weak)
    dp = L["pos"][col[k]].astype(LD) - L["pos"][row[k]].astype(LD)
    acc = np.zeros((n, 3, 3), dtype=LD)
    aab = np.zeros((n, 3, 3))
    seg_add(acc, row[k], bmm(L["blk"][k], T_of(dp, LD)))
    seg_add(aab, row[k], np.abs(L["blk"][k]) @ np.abs(T_of(dp.astype(np.float64))))
    kept = np.bincount(row[off & (L["strong"] != 0)], minlength=n)
    return acc, aab, kept


def stage3_filtered(L, check_mask=True):
    R = Result()
    n, rp = L["n"], L["rowptr"]
    D = L["blk"][rp[:-1]]
    acc, aab, kept = _weak_sums(L)
    keep = (kept > 0)[:, None, None]
    ref = D.astype(LD) + np.where(keep, acc, LD(0))
    R.put("filtered.dF", *entry_ratio(L["dF"], ref, np.abs(D) + np.where(keep, aab, 0.0)))
    # zero rows of dinvF: justified by no kept slot or trace(D^-1 L) > 0.5, L = -acc
    zero = ~np.any(L["dinvF"] != 0.0, axis=(1, 2))
    tr = -np.einsum("nij,nji->n", sym6(L["dinv"], LD), acc).astype(np.float64)
    band = np.abs(tr - 0.5) <= TRACE_BAND
    must_zero = (kept == 0) | (tr > 0.5 + TRACE_BAND) | ~np.isfinite(tr)
    may_zero = must_zero | band
    bad = (zero & ~may_zero) | (~zero & must_zero)
    R.exact("filtered.zero_rows", not bad.any(), tuple(np.flatnonzero(bad)[:4].tolist()))
    R.exact("filtered.trace_band_share", (band & (kept > 0)).sum() <= BAND_SHARE * n)
    nz = np.flatnonzero(~zero)
    r, at = inverse_ratio(L["dinvF"][nz], L["dF"][nz])
    R.put("filtered.dinvF", r, None if at is None else (int(nz[at[0]]),))
    L["_zero_rows"], L["_nonzero_rows"] = int(zero.sum()), int(nz.size)
    if check_mask:
        row, col = slot_rows(L), L["col"].astype(np.int64)
        w = np.sqrt((L["blk"].astype(LD) ** 2).sum(axis=(1, 2)))
        th = (LD(L["theta_filter"]) ** 2) * w[rp[:-1]][row] * w[rp[:-1]][col]
        off = col != row
        want = (w > 0) & (w * w >= th)
        near = np.abs(w * w - th) <= MASK_BAND * th
        bad = off & ~near & (want != (L["strong"] != 0))
        R.exact("filtered.mask", not bad.any(), tuple(np.flatnonzero(bad)[:4].tolist()))
        R.exact("filtered.mask_diag", bool((L["strong"][rp[:-1]] != 0).all()))
        R.exact("filtered.mask_band_share", (off & near).sum() <= BAND_SHARE * n)
    return R


def _p_keys(L):
    return L["p_row"].astype(np.int64) * L["nc"] + L["p_col"]


def stage4_transfer(L):
    R = Result()
    n, nc, rp = L["n"], L["nc"], L["rowptr"]
    row, col, agg = slot_rows(L), L["col"].astype(np.int64), L["agg"].astype(np.int64)
    filt = bool(L["filtered"])
    kept = (L["strong"] != 0) if filt else np.ones(L["nslot"], dtype=bool)
    # ---- the pattern: (i, agg(j)) over the listed slots and the own-aggregate entry
    want = np.unique(np.r_[row[kept] * nc + agg[col[kept]], np.arange(n, dtype=np.int64) * nc + agg])
    keys = _p_keys(L)
    R.exact("transfer.pattern", np.array_equal(keys, want), (int(keys.size), int(want.size)))
    R.exact("transfer.rowptr", np.array_equal(L["p_rowptr"], np.searchsorted(keys, np.arange(n + 1, dtype=np.int64) * nc)))
    if not np.array_equal(keys, want):
        return R
    # ---- the values
    blk = L["blk"]
    if filt:
        blk = blk.copy()
        blk[rp[:-1]] = L["dF"]
    npent = keys.size
    S = np.zeros((npent, 3, 3), dtype=LD)
    Sa = np.zeros((npent, 3, 3))
    ks = np.flatnonzero(kept)
    for c0 in range(0, ks.size, CHUNK):
        k = ks[c0:c0 + CHUNK]
        e = np.searchsorted(keys, row[k] * nc + agg[col[k]])
        Td = T_of(L["d"][col[k]])
        seg_add(S, e, bmm(blk[k], Td))
        seg_add(Sa, e, np.abs(blk[k]) @ np.abs(Td))
    i = L["p_row"].astype(np.int64)
    Dinv = L["dinvF"] if filt else sym6(L["dinv"])
    own = (L["p_col"] == agg[i])[:, None, None]
    Ti = T_of(L["d"][i])
    ref = np.where(own, Ti.astype(LD), LD(0)) - LD(L["omega_p"]) * bmm(Dinv[i], S)
    ab = np.where(own, np.abs(Ti), 0.0) + L["omega_p"] * (np.abs(Dinv[i]) @ Sa)
    R.put("transfer.values", *entry_ratio(L["p_blk"], ref, ab))
    return R


def stage5_copies(L, pre=""):
    """pre = "": P's copies; "ps": the folded transfer's (its two copies against each other)."""
    R = Result()
    if pre == "":
        f = L["p_blk"].reshape(-1, 9).astype(np.float32)
        r, t, tp, row, col, trow, tcol = L["r_blk"], L["t_blk"], L["t_pos"], L["p_row"], L["p_col"], L["t_row"], L["t_col"]
        R.exact("copies.r_blk", r.shape == f.shape and np.array_equal(r.view(np.uint32), f.view(np.uint32)))
    else:
        r, t, tp, row, col, trow, tcol = L["ps_r"], L["ps_t"], L["ps_stpos"], L["ap_row"], L["ap_col"], L["ps_trow"], L["ps_tcol"]
    m = r.shape[0]
    perm = tp.size == m and np.array_equal(np.sort(tp), np.arange(m))
    R.exact(pre + "copies.t_pos_permutation", perm)
    if not perm:
        return R
    bad = np.flatnonzero(np.any(t[tp].view(np.uint32) != r.view(np.uint32), axis=1))
    R.exact(pre + "copies.t_blk", bad.size == 0, tuple(bad[:4].tolist()))
    R.exact(pre + "copies.t_row_col", np.array_equal(trow[tp], row) and np.array_equal(tcol[tp], col))
    R.exact(pre + "copies.sorted_by_column", bool((np.diff(tcol.astype(np.int64)) >= 0).all()))
    return R


def _sorted(keys):
    order = np.argsort(keys, kind="stable")
    return keys[order], order


def stage6_galerkin(L, Nx):
    R = Result()
    n, nc = L["n"], L["nc"]
    row, col = slot_rows(L), L["col"].astype(np.int64)
    ncn = Nx["n"]
    crow, ccol = slot_rows(Nx), Nx["col"].astype(np.int64)
    ckeys = crow * ncn + ccol
    csk, cord = _sorted(ckeys)
    R.exact("galerkin.coarse_pattern_unique", ncn == nc and bool((np.diff(csk) > 0).all()))
    R.exact("galerkin.coarse_diagonal_first", np.array_equal(ccol[Nx["rowptr"][:-1]], np.arange(ncn)))
    Cb = Nx["blk"]
    if not L["smoothed"]:
        agg = L["agg"].astype(np.int64)
        acc = np.zeros((Nx["nslot"], 3, 3), dtype=LD)
        aab = np.zeros((Nx["nslot"], 3, 3))
        hit = np.zeros(Nx["nslot"], dtype=bool)
        missing = 0
        for c0 in range(0, L["nslot"], CHUNK):
            k = np.arange(c0, min(L["nslot"], c0 + CHUNK))
            t = lookup(csk, cord, agg[row[k]] * ncn + agg[col[k]])
            missing += int((t < 0).sum())
            k, t = k[t >= 0], t[t >= 0]
            Ti, Tj = T_of(L["d"][row[k]]), T_of(L["d"][col[k]])
            seg_add(acc, t, bmm(np.swapaxes(Ti, 1, 2), bmm(L["blk"][k], Tj)))
            seg_add(aab, t, np.abs(np.swapaxes(Ti, 1, 2)) @ np.abs(L["blk"][k]) @ np.abs(Tj))
            hit[t] = True
        R.exact("galerkin.coarse_pattern", missing == 0 and bool(hit.all()), (missing, int((~hit).sum())))
        R.put("galerkin.coarse", *entry_ratio(Cb, acc, aab))
    else:
        # ---- A P
        ak = L["ap_row"].astype(np.int64) * nc + L["ap_col"]
        ask, aord = _sorted(ak)
        R.exact("galerkin.ap_list", bool(L.get("ap_list_consistent", True)))
        R.exact("galerkin.ap_pattern_unique", bool((np.diff(ask) > 0).all()))
        prp, pcol = L["p_rowptr"].astype(np.int64), L["p_col"].astype(np.int64)
        pcnt = np.diff(prp)
        nap = ak.size
        acc = np.zeros((nap, 3, 3), dtype=LD)
        aab = np.zeros((nap, 3, 3))
        hit = np.zeros(nap, dtype=bool)
        missing = 0
        per = pcnt[col]
        bounds = np.r_[0, np.searchsorted(np.cumsum(per), np.arange(CHUNK, int(per.sum()) + CHUNK, CHUNK))]
        bounds = np.unique(np.r_[bounds, L["nslot"]])
        for b0, b1 in zip(bounds[:-1], bounds[1:]):
            e, q = expand(prp[col[b0:b1]], per[b0:b1])
            k = q + b0
            t = lookup(ask, aord, row[k] * nc + pcol[e])
            missing += int((t < 0).sum())
            k, e, t = k[t >= 0], e[t >= 0], t[t >= 0]
            seg_add(acc, t, bmm(L["blk"][k], L["p_blk"][e]))
            seg_add(aab, t, np.abs(L["blk"][k]) @ np.abs(L["p_blk"][e]))
            hit[t] = True
        R.exact("galerkin.ap_pattern", missing == 0 and bool(hit.all()), (missing, int((~hit).sum())))
        R.put("galerkin.ap", *entry_ratio(L["apblk"], acc, aab))
        # ---- P^T (A P) on the slots c >= a
        upper = ccol >= crow
        acc = np.zeros((Nx["nslot"], 3, 3), dtype=LD)
        aab = np.zeros((Nx["nslot"], 3, 3))
        hit = np.zeros(Nx["nslot"], dtype=bool)
        missing = 0
        api = L["ap_row"].astype(np.int64)
        per = pcnt[api]
        bounds = np.r_[0, np.searchsorted(np.cumsum(per), np.arange(CHUNK, int(per.sum()) + CHUNK, CHUNK))]
        bounds = np.unique(np.r_[bounds, nap])
        for b0, b1 in zip(bounds[:-1], bounds[1:]):
            e, q = expand(prp[api[b0:b1]], per[b0:b1])
            f = q + b0
            sel = pcol[e] <= L["ap_col"][f]
            e, f = e[sel], f[sel]
            t = lookup(csk, cord, pcol[e] * ncn + L["ap_col"][f].astype(np.int64))
            missing += int((t < 0).sum())
            e, f, t = e[t >= 0], f[t >= 0], t[t >= 0]
            Pt = np.swapaxes(L["p_blk"][e], 1, 2)
            seg_add(acc, t, bmm(Pt, L["apblk"][f]))
            seg_add(aab, t, np.abs(Pt) @ np.abs(L["apblk"][f]))
            hit[t] = True
        R.exact("galerkin.coarse_pattern", missing == 0 and bool(hit[upper].all()) and not hit[~upper].any(),
                (missing, int((~hit[upper]).sum())))
        u = np.flatnonzero(upper)
        r, at = entry_ratio(Cb[u], acc[u], aab[u])
        R.put("galerkin.coarse", r, None if at is None else (int(u[at[0]]),) + at[1:])
        lo = np.flatnonzero(~upper)
        mk = lookup(csk, cord, ccol[lo] * ncn + crow[lo])
        ok = (mk >= 0).all() and np.array_equal(Cb[lo].view(np.uint64), np.swapaxes(Cb[np.maximum(mk, 0)], 1, 2).copy().view(np.uint64))
        R.exact("galerkin.mirror", bool(ok))
    D = Cb[Nx["rowptr"][:-1]].astype(LD)
    R.put("galerkin.dinv", *inverse_ratio(sym6(Nx["dinv"]), (D + np.swapaxes(D, 1, 2)) / 2))   # (k_level_dinv symmetrises first)
    return R


def ptilde_reference(L):
    """P~ on A P's pattern in long double, and its magnitudes."""
    nc = L["nc"]
    i = L["ap_row"].astype(np.int64)
    keys = _p_keys(L)
    e = lookup(keys, np.arange(keys.size), i * nc + L["ap_col"])
    Pf = np.where((e >= 0)[:, None, None], L["p_blk"][np.maximum(e, 0)], 0.0)
    Dinv = sym6(L["dinv"])[i]
    ref = Pf.astype(LD) - LD(L["omega"]) * bmm(Dinv, L["apblk"])
    return ref, np.abs(Pf) + L["omega"] * (np.abs(Dinv) @ np.abs(L["apblk"]))


def stage7_folded(L):
    R = stage5_copies(L, "ps")
    ref, ab = ptilde_reference(L)
    got = L["ps_r"].reshape(-1, 3, 3)
    r, at = entry_ratio(got, ref, ab, extra=2.0 ** -24 * np.abs(ref).astype(np.float64) + F32_TINY)
    R.put("folded.values", r, at)
    if at is not None:
        L["_folded_worst"] = (float(got[at]), float(ref[at]), float(ab[at]))
    return R


def dense_of(L):
    n = L["n"]
    H = np.zeros((3 * n, 3 * n))
    row, col = slot_rows(L), L["col"].astype(np.int64)
    for r in range(3):
        for c in range(3):
            np.add.at(H, (3 * row + r, 3 * col + c), L["blk"][:, r, c])
    return H


def matmul_ld(A, B, block=256):
    """A @ B with long-double products and sums (blocked to bound the temporaries)."""
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for k0 in range(0, A.shape[1], block):
        out += A[:, k0:k0 + block] @ B[k0:k0 + block]
    return out


def stage8_coarsest(L):
    """The error of the exported inverse Z is H^-1 (I - H Z): the residual in long double from the level's blocks (the operator is
    sparse), the solve in fp64 (a relative kappa U of an error that is itself small)."""
    R = Result()
    n = L["n"]
    N = 3 * n
    R.exact("coarsest.size", L["N"] == N and L["inv"].shape[0] >= N)
    H = dense_of(L)
    Z = L["inv"][:N, :N]
    row, col = slot_rows(L), L["col"].astype(np.int64)
    Zb = Z.reshape(n, 3, N).astype(LD)
    HZ = np.zeros((n, 3, N), dtype=LD)
    step = max(1, 40_000_000 // (3 * N))
    for k0 in range(0, L["nslot"], step):
        k = slice(k0, k0 + step)
        seg_add(HZ, row[k], np.einsum("kij,kjm->kim", L["blk"][k].astype(LD), Zb[col[k]]))
    res = (np.eye(N, dtype=LD) - HZ.reshape(N, N)).astype(np.float64)
    Hinv = np.linalg.inv(H)
    err = Hinv @ res
    kappa = np.linalg.cond(H, 2)
    r = np.linalg.norm(err, axis=0) / (N * U * kappa * np.linalg.norm(Hinv, axis=0))
    r = np.where(np.isfinite(r), r, np.inf)
    R.put("coarsest.inverse", float(r.max()), (int(np.argmax(r)),))
    L["_kappa"] = float(kappa)
    return R


# ------------------------------------------------------------------ stage 9: the cycle
def _rowsum(rows, vals, n):
    out = np.zeros((n, 3), dtype=vals.dtype)
    seg_add(out, rows, vals)
    return out


def cycle_coefficient(num, den):
    """cycle_ratio's rule (sgo_device.h): num / den, 0 where the denominator is not positive or either is not finite."""
    return num / den if (den > 0 and np.isfinite(den) and np.isfinite(num)) else 0.0


def reduce_parts(p, g):
    """The fp64 sum of p[0 .. g) in block_reduce_parts_n's order: thread t of 256 adds the entries t, t + 256, ... serially from 0.0,
    wave_sum adds adjacent lanes as a balanced tree, thread 0 adds the four waves' sums in order.  Entries beyond g are not read."""
    v = np.zeros(MAX_PARTS)
    v[:g] = np.asarray(p, dtype=np.float64)[:g]
    s = np.zeros(256)
    for k in range(MAX_PARTS // 256):
        s = s + v[256 * k:256 * (k + 1)]
    w = s.reshape(4, 64)
    while w.shape[1] > 1:
        w = w[:, 0::2] + w[:, 1::2]
    return float(((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


def solve_kind(levels, l):
    """How coarse_solve() solves for level l >= 1's right-hand side: "dense" | "V" | "fcg1" | "fcg2", from the exported flags."""
    kdepth, fcg2 = levels[0].get("kdepth", 0), levels[0].get("fcg2_depth", 1)
    if l == len(levels) - 1:
        return "dense"
    if l > kdepth and levels[l]["smoothed"]:
        return "V"
    return "fcg1" if l > fcg2 else "fcg2"


def has_kcycle(levels):
    return any(solve_kind(levels, l).startswith("fcg") for l in range(1, len(levels)))


def model_grid(n):
    """How many partial sums the forward model leaves for a level of n rows (the device: its k_spmv grid)."""
    return max(1, min(MAX_PARTS, (n + 15) // 16))


class Cycle:
    """z = M r from the exported levels in `dtype` arithmetic (np.longdouble: the reference; np.float64: the rounding scale).
    record: keep every level's work vectors as the device's buffers hold them after the cycle (self.W: the forward model of the
    SGO_AMG_W_* export; coefficients then come from partial sums reduced in the kernel's order).  inner(l, rhs): a stand-in for
    the inner cycles of fcg().  (The CPU mutation tests subclass it with mistakes built in: tests/test_amg_reference.py.)"""

    def __init__(self, levels, dtype=LD, skip_post=False, record=False, inner=None):
        self.lv, self.dt, self.skip_post = levels, dtype, skip_post
        self.inner = inner
        self.trace = {}
        self.W = None
        if record:
            self.W = [{k: np.zeros((L["n"], 3)) for k in (WORK if l else WORK[:3])} for l, L in enumerate(levels)]
            for l, w in enumerate(self.W[1:], 1):
                w.update(pA=np.zeros((2, MAX_PARTS)), pB=np.zeros((2, MAX_PARTS)), pC=np.zeros((2, MAX_PARTS)), grids=np.zeros(3, dtype=np.int32))
        self.c = []
        for l, L in enumerate(levels):
            c = dict(row=slot_rows(L), col=L["col"].astype(np.int64), dinv=sym6(L["dinv"], dtype))
            A = L["blk32"] if (l == 0 and L["f32"] and "blk32" in L) else L["blk"]
            c["A"] = A.astype(dtype)
            self.c.append(c)

    def A(self, l, x):
        c = self.c[l]
        return _rowsum(c["row"], np.einsum("kij,kj->ki", c["A"], x[c["col"]]), self.lv[l]["n"])

    def jac(self, l, v):
        return self.dt(self.lv[l]["omega"]) * np.einsum("nij,nj->ni", self.c[l]["dinv"], v)

    def restrict(self, l, res, folded):
        L = self.lv[l]
        if not L["smoothed"]:
            return _rowsum(L["agg"].astype(np.int64), np.einsum("kji,kj->ki", T_of(L["d"], self.dt), res), L["nc"])
        t, trow, tcol = (L["ps_t"], L["ps_trow"], L["ps_tcol"]) if folded else (L["t_blk"], L["t_row"], L["t_col"])
        B = t.reshape(-1, 3, 3).astype(self.dt)
        return _rowsum(tcol.astype(np.int64), np.einsum("kji,kj->ki", B, res[trow]), L["nc"])

    def prolong(self, l, xc, folded):
        L = self.lv[l]
        if not L["smoothed"]:
            return np.einsum("kij,kj->ki", T_of(L["d"], self.dt), xc[L["agg"]])
        r, row, col = (L["ps_r"], L["ap_row"], L["ap_col"]) if folded else (L["r_blk"], L["p_row"], L["p_col"])
        B = r.reshape(-1, 3, 3).astype(self.dt)
        return _rowsum(np.asarray(row, dtype=np.int64), np.einsum("kij,kj->ki", B, xc[col]), L["n"])

    def _rec(self, l, **kw):
        if self.W is not None:
            for k, v in kw.items():
                self.W[l][k] = np.array(v, dtype=np.float64)

    def dot(self, l, a, b, buf, half):
        """a . b; recording: per-chunk partial sums left in W[l][buf][half] and reduced in the kernel's order."""
        if self.W is None:
            return (a * b).sum()
        g = model_grid(self.lv[l]["n"])
        p = np.array([c.sum() for c in np.array_split((a * b).sum(axis=1), g)], dtype=np.float64)
        self.W[l][buf][half, :] = 0.0
        self.W[l][buf][half, :g] = p
        return reduce_parts(p, g)

    def fcg(self, l, bk):
        """fcg() of sgo_amg.hip for A x = bk on level l; the steps' vectors are kept in self.trace[l] (in self.dt)."""
        fcg2 = self.lv[0].get("fcg2_depth", 1)
        two = l <= fcg2
        g = model_grid(self.lv[l]["n"])
        z1 = self.inner(l, bk) if self.inner else self.cycle(l, bk)
        q = self.A(l, z1)
        zq, zb = self.dot(l, z1, q, "pA", 0), self.dot(l, z1, bk, "pA", 1)
        a1 = cycle_coefficient(zb, zq)
        self._rec(l, z1=z1, q=q)
        if self.W is not None:
            self.W[l]["grids"][:] = (g, 0, 0)
        self.trace[l] = dict(bk=bk, z1=z1, q=q, a1=a1, x=a1 * z1)
        if not two:
            return a1 * z1
        bk2 = bk - a1 * q
        self._rec(l, bk2=bk2)
        z2 = self.inner(l, bk2) if self.inner else self.cycle(l, bk2, unfolded=True)
        b = cycle_coefficient(self.dot(l, q, z2, "pC", 0), zq)
        p2 = z2 - b * z1
        q2 = self.A(l, p2)
        a2 = cycle_coefficient(self.dot(l, p2, bk2, "pB", 1), self.dot(l, p2, q2, "pB", 0))
        self._rec(l, z2=z2, p2=p2, q2=q2)
        if self.W is not None:
            self.W[l]["grids"][:] = (g, g, g)
        x = a1 * z1 + a2 * p2
        self.trace[l].update(bk2=bk2, z2=z2, b=b, p2=p2, q2=q2, a2=a2, x=x)
        return x

    def coarse_solve(self, l, bk):
        """coarse_solve() of sgo_amg.hip: the solution for level l + 1's right-hand side as level l prolongates it."""
        C = l + 1
        self._rec(C, bk=bk)
        kind = solve_kind(self.lv, C)
        if kind.startswith("fcg"):
            return self.fcg(C, bk)
        if kind == "dense":
            N = 3 * self.lv[C]["n"]
            xk = (self.lv[C]["inv"][:N, :N].astype(self.dt) @ bk.reshape(N)).reshape(-1, 3)
        else:
            xk = self.cycle(C, bk)
        self._rec(C, xk=xk)
        return xk

    def cycle(self, l, rhs, unfolded=False):
        """cycle0 / cycle_coarse: one cycle of level l for rhs, in the level's exported form or unfolded (cycle_form with an
        RhsSub or a dot request), leaving the work vectors where the device's launches leave them."""
        L = self.lv[l]
        kind, nu = (UNFOLDED if unfolded else L["kind"]), L["nu"]
        if kind == FOLDED:
            cs = self.coarse_solve(l, self.restrict(l, rhs, True))
            x1 = self.jac(l, rhs)
            m2 = x1 + self.jac(l, rhs - self.A(l, x1))
            if l == 0:
                self._rec(0, xs=x1, rs=m2)
            return m2 + self.prolong(l, cs, True)
        if kind == FOLDED2:
            xs = self.jac(l, rhs)
            rs = rhs - self.A(l, xs)
            cs = self.coarse_solve(l, self.restrict(l, rs, True))
            x1 = self.jac(l, rs)
            tR = xs + (x1 + self.jac(l, rs - self.A(l, x1)) + self.prolong(l, cs, True))
            self._rec(l, xs=xs, rs=rs, tR=tR)
            return tR + self.jac(l, rhs - self.A(l, tR))
        x = np.zeros_like(rhs)
        res = rhs
        for sw in range(nu):
            dx = self.jac(l, res)
            x = x + dx
            res = res - self.A(l, dx)
            self._rec(l, **{"tR" if sw % 2 else "rs": res})
        cs = self.coarse_solve(l, self.restrict(l, res, False))
        xp = x + self.prolong(l, cs, False)
        # the fused launch (SPMV_JACOBI_P) leaves xs as the pre-smoothing made it; every other path prolongates in place
        self._rec(l, xs=x if (not L["smoothed"] and l >= 1 and L["nslot"] < UNFUSE_SLOTS) else xp)
        if not self.skip_post:
            src = "xs"
            for sw in range(nu):
                xp = xp + self.jac(l, rhs - self.A(l, xp))
                if sw < nu - 1:
                    src = "tR" if src == "rs" else "rs"
                    self._rec(l, **{src: xp})
        return xp

    def __call__(self, l, r):
        r = np.asarray(r, dtype=self.dt)
        if l == len(self.lv) - 1:
            N = 3 * self.lv[l]["n"]
            return (self.lv[l]["inv"][:N, :N].astype(self.dt) @ r.reshape(N)).reshape(-1, 3)
        return self.cycle(l, r)


def cycle_scale(levels, r):
    """(z_ref long double, eps_case = |z_fp64 - z_ref| / |z_ref|)."""
    z = Cycle(levels, LD)(0, r)
    z64 = Cycle(levels, np.float64)(0, r)
    nz = np.sqrt((z * z).sum())
    return z, float(np.sqrt(((z64.astype(LD) - z) ** 2).sum()) / nz)


def cycle_ratio(z_got, z_ref, eps):
    d = np.asarray(z_got, dtype=LD) - z_ref
    return float(np.sqrt((d * d).sum()) / np.sqrt((z_ref * z_ref).sum())) / eps


# ------------------------------------------------------------------ stage 10: the K-cycle's steps on the exported work vectors
def export_work(opt, levels):
    """Per level the SGO_AMG_W_* arrays as the last sgo_precondition left them (keys: WORK, pA pB pC (2, MAX_PARTS), grids)."""
    out = []
    for l, L in enumerate(levels):
        w = {}
        for k in WORK:
            a = _fetch(opt, l, "W_" + k.upper(), np.float64)
            if a is not None:
                w[k] = a.reshape(L["n"], 3)
        for k in ("pA", "pB", "pC"):
            a = _fetch(opt, l, "W_" + k.upper(), np.float64)
            if a is not None:
                w[k] = a.reshape(2, MAX_PARTS)
        g = _fetch(opt, l, "W_GRIDS", np.int32)
        if g is not None:
            w["grids"] = g
        out.append(w)
    return out


class _Ops:
    """One level's operator and block-Jacobi sweep in long double, each with the same expression on magnitudes."""

    def __init__(self, levels, l):
        L = levels[l]
        self.n, self.w = L["n"], L["omega"]
        self.row, self.col = slot_rows(L), L["col"].astype(np.int64)
        A = L["blk32"] if (l == 0 and L["f32"] and "blk32" in L) else L["blk"]      # (what the level's passes read: Cycle's rule)
        self.Ab, self.Aa = np.asarray(A, dtype=LD), np.abs(np.asarray(A, dtype=np.float64))
        D = sym6(L["dinv"])
        self.D, self.Da = D.astype(LD), np.abs(D)

    def A(self, x):
        return _rowsum(self.row, np.einsum("kij,kj->ki", self.Ab, x[self.col]), self.n)

    def Aabs(self, xa):
        return _rowsum(self.row, np.einsum("kij,kj->ki", self.Aa, xa[self.col]), self.n)

    def jac(self, v):
        return LD(self.w) * np.einsum("nij,nj->ni", self.D, v)

    def jacabs(self, va):
        return self.w * np.einsum("nij,nj->ni", self.Da, va)

    def sweep(self, x, xa, rhs):
        """x + w Dinv (rhs - A x) for an iterate x of magnitudes xa, and its magnitudes."""
        return x + self.jac(rhs.astype(LD) - self.A(x)), xa + self.jacabs(np.abs(rhs) + self.Aabs(xa))


def _ld(a):
    return np.asarray(a, dtype=LD)


def _restrict10(L, res, folded):
    """(P^T res | P~^T res | sum_{i in a} T(d_i)^T res_i, the same on magnitudes) for the level's transfer as stored."""
    if not L["smoothed"]:
        agg = L["agg"].astype(np.int64)
        return (_rowsum(agg, np.einsum("kji,kj->ki", T_of(L["d"], LD), _ld(res)), L["nc"]),
                _rowsum(agg, np.einsum("kji,kj->ki", np.abs(T_of(L["d"])), np.abs(res)), L["nc"]))
    t, trow, tcol = (L["ps_t"], L["ps_trow"], L["ps_tcol"]) if folded else (L["t_blk"], L["t_row"], L["t_col"])
    B = t.reshape(-1, 3, 3)
    tcol = tcol.astype(np.int64)
    return (_rowsum(tcol, np.einsum("kji,kj->ki", B.astype(LD), _ld(res)[trow]), L["nc"]),
            _rowsum(tcol, np.einsum("kji,kj->ki", np.abs(B).astype(np.float64), np.abs(res)[trow]), L["nc"]))


def _prolong10(L, w, wa, folded):
    if not L["smoothed"]:
        return np.einsum("kij,kj->ki", T_of(L["d"], LD), w[L["agg"]]), np.einsum("kij,kj->ki", np.abs(T_of(L["d"])), wa[L["agg"]])
    r, row, col = (L["ps_r"], L["ap_row"], L["ap_col"]) if folded else (L["r_blk"], L["p_row"], L["p_col"])
    B = r.reshape(-1, 3, 3)
    row = np.asarray(row, dtype=np.int64)
    return (_rowsum(row, np.einsum("kij,kj->ki", B.astype(LD), w[col]), L["n"]),
            _rowsum(row, np.einsum("kij,kj->ki", np.abs(B).astype(np.float64), wa[col]), L["n"]))


def exported_coefficients(w):
    """(a1, b, a2) from a level's exported partial sums and grid counts, in fp64 in the kernels' order (cycle_ratio's rule)."""
    gA, gB, gC = (int(x) for x in w["grids"])
    den = reduce_parts(w["pA"][0], gA)
    return (cycle_coefficient(reduce_parts(w["pA"][1], gA), den), cycle_coefficient(reduce_parts(w["pC"][0], gC), den),
            cycle_coefficient(reduce_parts(w["pB"][1], gB), reduce_parts(w["pB"][0], gB)))


def _coarse_solution(levels, W, C):
    """c1 u1 + c2 u2 as level C - 1's last launch prolongates it (long double from the exported vectors), and its magnitudes."""
    kind, w = solve_kind(levels, C), W[C]
    if kind in ("dense", "V"):
        return _ld(w["xk"]), np.abs(w["xk"])
    a1, _, a2 = exported_coefficients(w)
    ref, ab = LD(a1) * _ld(w["z1"]), abs(a1) * np.abs(w["z1"])
    if kind == "fcg2":
        ref, ab = ref + LD(a2) * _ld(w["p2"]), ab + abs(a2) * np.abs(w["p2"])
    return ref, ab


def _dot_ratio(parts, g, a, b):
    s = _ld(parts[:g]).sum()
    ref, ab = (_ld(a) * _ld(b)).sum(), float((np.abs(a) * np.abs(b)).sum())
    err = float(abs(s - ref))
    if not np.isfinite(err):
        return float("inf"), None
    return (err / (U * ab) if ab > 0 else (float("inf") if err > 0 else 0.0)), None


def stage10_kcycle(levels, W, r, z):
    """{(level, check): (error / (U abs), where)} over the steps of every level's last visit; r, z: sgo_precondition's input and
    result in the internal row order.  Check names begin with the step (restrict, product, dots, bk2, p2, last, coarsest, grids)."""
    R = {}
    last = len(levels) - 1
    for l in range(last):
        L, w, ops = levels[l], W[l], _Ops(levels, l)
        sk = solve_kind(levels, l) if l else "top"
        nu = L["nu"]
        # ---- the flexible-CG steps of this level
        if sk.startswith("fcg"):
            gA, gB, gC = (int(x) for x in w["grids"])
            R[(l, "grids")] = (0.0 if (0 < gA <= MAX_PARTS and ((0 < gB <= MAX_PARTS and 0 < gC <= MAX_PARTS) if sk == "fcg2" else gB == gC == 0))
                               else float("inf"), (gA, gB, gC))
            a1, b, _ = exported_coefficients(w)
            z1, q, bk = w["z1"], w["q"], w["bk"]
            R[(l, "product.q")] = entry_ratio(q, ops.A(_ld(z1)), ops.Aabs(np.abs(z1)))
            R[(l, "dots.z1_q")] = _dot_ratio(w["pA"][0], gA, z1, q)
            R[(l, "dots.z1_bk")] = _dot_ratio(w["pA"][1], gA, z1, bk)
            if sk == "fcg2":
                bk2, z2, p2, q2 = w["bk2"], w["z2"], w["p2"], w["q2"]
                R[(l, "bk2")] = entry_ratio(bk2, _ld(bk) - LD(a1) * _ld(q), np.abs(bk) + abs(a1) * np.abs(q))
                R[(l, "dots.q_z2")] = _dot_ratio(w["pC"][0], gC, q, z2)
                R[(l, "p2")] = entry_ratio(p2, _ld(z2) - LD(b) * _ld(z1), np.abs(z2) + abs(b) * np.abs(z1))
                R[(l, "product.q2")] = entry_ratio(q2, ops.A(_ld(p2)), ops.Aabs(np.abs(p2)))
                R[(l, "dots.p2_q2")] = _dot_ratio(w["pB"][0], gB, p2, q2)
                R[(l, "dots.p2_bk2")] = _dot_ratio(w["pB"][1], gB, p2, bk2)
        # ---- the level's last cycle: its form, right-hand side and result (_last_visit)
        if l == 0:
            kind, rhs, out = L["kind"], r, z
        elif sk == "fcg2":
            kind, rhs, out = UNFOLDED, w["bk2"], w["z2"]       # cycle': unfolded whatever the level's own form
        else:
            kind, rhs, out = L["kind"], w["bk"], (w["xk"] if sk == "V" else w["z1"])
        rhs = np.asarray(rhs, dtype=np.float64)
        rhsa = np.abs(rhs)
        cw, cwa = _coarse_solution(levels, W, l + 1)
        bkc = W[l + 1]["bk"]
        if kind == FOLDED:
            R[(l, "restrict")] = entry_ratio(bkc, *_restrict10(L, rhs, True))
            x1, x1a = ops.jac(_ld(rhs)), ops.jacabs(rhsa)
            m2, m2a = ops.sweep(x1, x1a, rhs)
            if l == 0:      # (level 0 keeps the two-sweep term: xs = w Dinv r, rs = M2 r)
                R[(l, "last.first_sweep")] = entry_ratio(w["xs"], x1, x1a)
                R[(l, "last.sweep")] = entry_ratio(w["rs"], *ops.sweep(_ld(w["xs"]), np.abs(w["xs"]), rhs))
                m2, m2a = _ld(w["rs"]), np.abs(w["rs"])
            pw, pwa = _prolong10(L, cw, cwa, True)
            R[(l, "last.out")] = entry_ratio(out, m2 + pw, m2a + pwa)
        elif kind == FOLDED2:
            xs, rs, tR = w["xs"], w["rs"], w["tR"]
            R[(l, "restrict")] = entry_ratio(bkc, *_restrict10(L, rs, True))
            R[(l, "last.first_sweep")] = entry_ratio(xs, ops.jac(_ld(rhs)), ops.jacabs(rhsa))
            R[(l, "last.resid")] = entry_ratio(rs, _ld(rhs) - ops.A(_ld(xs)), rhsa + ops.Aabs(np.abs(xs)))
            m2, m2a = ops.sweep(ops.jac(_ld(rs)), ops.jacabs(np.abs(rs)), rs)
            pw, pwa = _prolong10(L, cw, cwa, True)
            R[(l, "last.fold")] = entry_ratio(tR, _ld(xs) + m2 + pw, np.abs(xs) + m2a + pwa)
            R[(l, "last.out")] = entry_ratio(out, *ops.sweep(_ld(tR), np.abs(tR), rhs))
        else:
            if nu <= 2:     # (nu = 1: rs; nu = 2: tR, rs then holds the first post-smoothing sweep; beyond: overwritten)
                R[(l, "restrict")] = entry_ratio(bkc, *_restrict10(L, w["rs"] if nu == 1 else w["tR"], False))
            pw, pwa = _prolong10(L, cw, cwa, False)
            xs = w["xs"]
            if not L["smoothed"] and l >= 1 and L["nslot"] < UNFUSE_SLOTS:      # fused: xs is the pre-smoothing's
                xp, xpa = _ld(xs) + pw, np.abs(xs) + pwa
            else:           # in place: xs is x' itself, checked against the pre-smoothing recomputed from rhs
                x, xa, rr, rra = np.zeros((L["n"], 3), dtype=LD), np.zeros((L["n"], 3)), _ld(rhs), rhsa
                for _ in range(nu):
                    dx, dxa = ops.jac(rr), ops.jacabs(rra)
                    x, xa, rr, rra = x + dx, xa + dxa, rr - ops.A(dx), rra + ops.Aabs(dxa)
                R[(l, "last.prolong")] = entry_ratio(xs, x + pw, xa + pwa)
                xp, xpa = _ld(xs), np.abs(xs)
            if nu == 2:
                R[(l, "last.sweep")] = entry_ratio(w["rs"], *ops.sweep(xp, xpa, rhs))
                xp, xpa = _ld(w["rs"]), np.abs(w["rs"])
            elif nu > 2:
                for _ in range(nu - 1):
                    xp, xpa = ops.sweep(xp, xpa, rhs)
            R[(l, "last.out")] = entry_ratio(out, *ops.sweep(xp, xpa, rhs))
    wl = W[last]
    N = 3 * levels[last]["n"]
    inv = levels[last]["inv"][:N, :N]
    R[(last, "coarsest")] = entry_ratio(wl["xk"].reshape(N), matmul_ld(inv, wl["bk"].reshape(N, 1)).reshape(N),
                                        np.abs(inv) @ np.abs(wl["bk"].reshape(N)))
    return R


def written_vectors(levels, l):
    """The work vectors some launch of a cycle writes on level l (the others keep whatever the arena held: nothing reads them)."""
    L, last = levels[l], len(levels) - 1
    sk = solve_kind(levels, l) if l else "top"
    if l == last:
        return {"bk", "xk"} if l else set()
    forms = {"top": [L["kind"]], "V": [L["kind"]], "fcg1": [L["kind"]], "fcg2": [L["kind"], UNFOLDED]}[sk]
    out = set() if l == 0 else ({"bk", "xk"} if sk == "V" else ({"bk", "z1", "q"} | ({"bk2", "z2", "p2", "q2"} if sk == "fcg2" else set())))
    for f in forms:
        if f == FOLDED2 or (f == UNFOLDED and L["nu"] >= 2):
            out |= {"xs", "rs", "tR"}
        elif f == UNFOLDED or l == 0:
            out |= {"xs", "rs"}
    return out


def kcycle_all_zero(levels, W, z):
    """The rule case r = 0: every exported work vector the cycle writes, and z, exactly zero (and so finite); the partial sums
    that were read too."""
    bad = [(l, k) for l, w in enumerate(W) for k in sorted(written_vectors(levels, l)) if k in w and np.any(w[k] != 0.0)]
    for l, w in enumerate(W):
        if "grids" in w:
            bad += [(l, p) for p, g in zip(("pA", "pB", "pC"), w["grids"]) if np.any(w[p][:, :int(g)] != 0.0)]
    if np.any(np.asarray(z) != 0.0):
        bad.append(("z",))
    return bad


def step_of(check):
    return check.split(".")[0]


def check_kcycle(levels, W, r, z):
    """{(level, check): (ratio / C_K[step], raw ratio, where)}: a value above 1 fails."""
    return {k: ((v if v in (0.0, float("inf")) else v / C_K[step_of(k[1])]), v, at) for k, (v, at) in stage10_kcycle(levels, W, r, z).items()}


def worst_by_step(res):
    """{step: (worst raw ratio, level, check)} of a check_kcycle result."""
    w = {}
    for (l, k), (_, raw, at) in res.items():
        s = step_of(k)
        if s not in w or raw > w[s][0]:
            w[s] = (raw, l, k)
    return w


# ------------------------------------------------------------------ all applicable stages of a hierarchy
def check_hierarchy(levels, poses_xy=None, check_mask=True, stages=(1, 2, 3, 4, 5, 6, 7, 8)):
    """{(level, check): (ratio / C_stage, where)} over every applicable stage: a value above 1 fails."""
    out = {}

    def add(l, R, stage):
        c = C_STAGE.get(stage)
        for k, (v, at) in R.items():
            inv = k.endswith(("dinvF", ".dinv"))
            cc = C_STAGE["inverse"] if inv else (C_DENSE if k == "coarsest.inverse" else c)
            exact = v in (0.0, float("inf"))
            out[(l, k)] = (v if exact or cc is None else v / cc, v, at)

    for l, L in enumerate(levels[:-1]):
        Nx = levels[l + 1]
        if 1 in stages:
            add(l, stage1_partition(L), None)
        if 2 in stages:
            add(l, stage2_geometry(L, Nx, poses_xy if l == 0 else None), "geometry")
        if L["smoothed"]:
            if L["filtered"] and 3 in stages:
                add(l, stage3_filtered(L, check_mask), "filtered")
            if 4 in stages:
                add(l, stage4_transfer(L), "transfer")
            if 5 in stages:
                add(l, stage5_copies(L), None)
        if 6 in stages:
            add(l, stage6_galerkin(L, Nx), "galerkin")
        if L["smoothed"] and L["folded"] and 7 in stages:
            add(l, stage7_folded(L), "folded")
    if 8 in stages:
        add(len(levels) - 1, stage8_coarsest(levels[-1]), None)
    return out


def failures(res):
    return {k: v for k, v in res.items() if not v[0] <= 1.0}


def worst_by_stage(res):
    """{stage name: (worst raw ratio, level, check)} of a check_hierarchy result."""
    w = {}
    for (l, k), (_, raw, at) in res.items():
        s = "inverse" if k.endswith(("dinvF", ".dinv")) else k.split(".")[0].replace("pscopies", "copies")
        if s not in w or raw > w[s][0]:
            w[s] = (raw, l, k, at)
    return w
