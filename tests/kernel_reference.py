"""Per-entry reference for the level-0 entry points that never forms H (CPU only, test infrastructure).

What it computes, at the poses given, in hessian order (free vertices in ascending id, as sgo_free_ids):
b, the 3x3 diagonal blocks, plain and robust chi2, the per-edge chi2 and H x for every given x -- each with a
per-entry error bound.  The edges are processed in chunks (CHUNK at a time), so a graph of 10 M edges needs a few
hundred MB, where np_oracle.linearize's scipy H would need several GB.

Arithmetic.  The edge algebra is np_oracle's (edge_error, edge_jacobians, info_full, dcs_rho): it returns fp64 even
for long-double input, so every per-edge term -- e, A, B, the weighted products A^T W e, A^T W A, A^T W (A x_i + B x_j) --
is an fp64 value, rounded once per operation.  The per-row sums of those terms, the per-edge chi2 and the totals are
accumulated in np.longdouble (eps = 1.08e-19 on x86-64, asserted below), so the sums' own rounding is negligible and
the reference's error is that of its fp64 terms.

The bound.  Every output entry y gets  |y_kernel - y_ref| <= C * U * abs(y),  U = 2^-53 the fp64 unit roundoff and
abs(y) the sum of the absolute values of the terms that make up y, each term taken with the magnitude of the rounding
its inputs carry:

* the error e = Z^-1 (Xi^-1 Xj) is a difference of coordinates: its translation part carries the rounding of t_j - t_i
  and of the measurement at the size of the coordinates, |t_i|_1 + |t_j|_1 + |t_z|_1, its angle that of
  theta_i, theta_j, theta_z and the 2 pi of the wrap.  e_bar = |e| + those magnitudes;
* A = Rz A0 and B = Rz B0, Rz the rotation of Z^-1; the third column of A0 (d e / d theta_i) holds (t_j - t_i) rotated.
  A_bar = |Rz| (|A0| + (|t_i|_1 + |t_j|_1) in the two translation rows of that column), B_bar = |Rz| |B0|: where the
  rotations' products cancel in an entry of A, their rounding does not;
* the DCS weight w = s^2, s = 2 phi / (phi + e2), moves with the rounding of e2: |dw / de2| <= 2 w / (phi + e2), and e2
  carries U * abs(e2), so w_bar = w (1 + 2 abs(e2) / (phi + e2)) on every edge with a kernel -- saturated ones too: an
  edge whose e2 is within rounding of phi gets its w on either side of the kink at e2 = phi;
* abs(e2) = |e|^T |Omega| e_bar + U e_mag^T |Omega| e_mag (the second term: an error that is rounding and nothing else,
  e.g. an odometry edge at a dead-reckoned start, where the first term vanishes with e);

and then abs(b_i) = sum A_bar^T (w_bar |Omega|) e_bar, abs(D_i) = sum A_bar^T (w_bar |Omega|) A_bar,
abs((H x)_i) = sum A_bar^T (w_bar |Omega|) (A_bar |x_i| + B_bar |x_j|) (B for the edges' second vertex),
abs(chi2) = sum abs(e2), abs(robust chi2) = sum w_bar abs(e2).

The constant C.  These are first-order bounds of the rounding of short fp64 expressions (a product of three 3x3 factors,
a handful of sums) and of the sums over a row's edges; each contributes a small multiple of U * abs.  Both sides' rounding
counts (kernel and reference); the kernels contract to FMA and sum in their own order.  Across every case of
tests/test_gpu_kernel_reference.py the worst measured error / (U * abs) was 7.1, for H x with rows scaled
by 10^+-6 (C4 from the dead-reckoned start, after three iterations).  C = 16 is 2.3 x that, within 8 x of it.
The kernels' sums are trees (wave scans, block sums) or a few terms per lane.  A plain sequential fp64 sum over a long row
whose large terms come first can err by up to (k - 1) U abs.  The C++ oracle's row sums do this.  At C4's dead-reckoned
start, a row with two odometry edges and 66 closures that DCS has switched off reaches 33 U abs there.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import np_oracle as npo

LD = np.longdouble
assert np.finfo(LD).eps <= 1e-18, "the reference accumulates in an extended long double (x86-64: eps 1.08e-19)"

U = np.finfo(np.float64).eps / 2          # fp64 unit roundoff, 2^-53
C = 16.0
CHUNK = 1_000_000


@dataclass
class Reference:
    free: np.ndarray                      # (n,) vertex id of every hessian row
    b: np.ndarray                         # (n,3) longdouble
    b_abs: np.ndarray                     # (n,3)
    diag: np.ndarray                      # (n,3,3) longdouble
    diag_abs: np.ndarray
    chi2: LD = LD(0)
    chi2_abs: float = 0.0
    robust: LD = LD(0)
    robust_abs: float = 0.0
    e2: np.ndarray = None                 # (E,) longdouble
    e2_abs: np.ndarray = None
    hx: list = field(default_factory=list)       # (n,3) longdouble per x
    hx_abs: list = field(default_factory=list)


def edge_terms(xi, xj, meas, info, phi, x_i=(), x_j=(), e=None):
    """Per-edge fp64 terms and their magnitudes for edges with endpoint poses xi, xj (m,3).  x_i, x_j: the vectors' blocks at
    the two endpoints (zero at fixed vertices).  e: an error to use instead of edge_error's (the CPU tests' mutations)."""
    xi = np.asarray(xi, dtype=np.float64)
    xj = np.asarray(xj, dtype=np.float64)
    meas = np.asarray(meas, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    if e is None:
        e = npo.edge_error(xi, xj, meas)
    A, B = npo.edge_jacobians(xi, xj, meas)
    O = npo.info_full(info)
    Oa = np.abs(O)
    eL = e.astype(LD)
    e2 = np.einsum("ni,nij,nj->n", eL, O.astype(LD), eL)
    rho0, rho1 = npo.dcs_rho(e2.astype(np.float64), phi)
    tmag = np.abs(xi[:, :2]).sum(1) + np.abs(xj[:, :2]).sum(1)
    emag = np.empty_like(e)
    emag[:, 0] = emag[:, 1] = tmag + np.abs(meas[:, :2]).sum(1)
    emag[:, 2] = np.abs(xi[:, 2]) + np.abs(xj[:, 2]) + np.abs(meas[:, 2]) + 2.0 * np.pi
    ebar = np.abs(e) + emag
    e2_abs = np.einsum("ni,nij,nj->n", np.abs(e), Oa, ebar) + U * np.einsum("ni,nij,nj->n", emag, Oa, emag)
    # (on every edge with a kernel, saturated ones included: one whose e2 is within rounding of phi has its w computed on
    # either side of the kink at e2 = phi, where |dw / de2| jumps from 0 to 2 w / (phi + e2))
    with np.errstate(divide="ignore", invalid="ignore"):
        wbar = rho1 * (1.0 + np.where(phi >= 0, 2.0 * e2_abs / (phi + e2.astype(np.float64)), 0.0))
    W = O * rho1[:, None, None]
    Wa = Oa * wbar[:, None, None]
    # A = Rz A0 and B = Rz B0 (Rz: the rotation of Z^-1): the magnitudes are |Rz| |A0|, not |A| -- the rotations' products
    # cancel in entries of A near zero, their rounding does not
    th = npo.se2_inv(meas)[:, 2]
    Rz = np.zeros((len(th), 3, 3))
    Rz[:, 0, 0] = Rz[:, 1, 1] = np.cos(th)
    Rz[:, 1, 0] = np.sin(th)
    Rz[:, 0, 1] = -Rz[:, 1, 0]
    Rz[:, 2, 2] = 1.0
    Rzt = np.swapaxes(Rz, 1, 2)
    A0 = np.abs(Rzt @ A)
    A0[:, 0:2, 2] += tmag[:, None]
    Ab = np.abs(Rz) @ A0
    Bb = np.abs(Rz) @ np.abs(Rzt @ B)
    At, Bt, Abt, Bbt = (np.swapaxes(M, 1, 2) for M in (A, B, Ab, Bb))
    We = np.einsum("nij,nj->ni", W, e)
    Wea = np.einsum("nij,nj->ni", Wa, ebar)
    t = dict(e=e, e2=e2, e2_abs=e2_abs, rho0=rho0, rho1=rho1, wbar=wbar, A=A, B=B, W=W,
             bi=-np.einsum("nij,nj->ni", At, We), bj=-np.einsum("nij,nj->ni", Bt, We),
             bi_abs=np.einsum("nij,nj->ni", Abt, Wea), bj_abs=np.einsum("nij,nj->ni", Bbt, Wea),
             Hii=At @ W @ A, Hjj=Bt @ W @ B, Hii_abs=Abt @ Wa @ Ab, Hjj_abs=Bbt @ Wa @ Bb,
             Hij=At @ W @ B, Hij_abs=Abt @ Wa @ Bb,      # (the off-diagonal block towards the second vertex; its transpose the other way)
             yi=[], yj=[], yi_abs=[], yj_abs=[], A_abs=Ab, B_abs=Bb, e_abs=ebar)
    for a, c in zip(x_i, x_j):
        v = np.einsum("nij,nj->ni", W, np.einsum("nij,nj->ni", A, a) + np.einsum("nij,nj->ni", B, c))
        va = np.einsum("nij,nj->ni", Wa, np.einsum("nij,nj->ni", Ab, np.abs(a)) + np.einsum("nij,nj->ni", Bb, np.abs(c)))
        t["yi"].append(np.einsum("nij,nj->ni", At, v))
        t["yj"].append(np.einsum("nij,nj->ni", Bt, v))
        t["yi_abs"].append(np.einsum("nij,nj->ni", Abt, va))
        t["yj_abs"].append(np.einsum("nij,nj->ni", Bbt, va))
    return t


def _segment_sum(rows, vals, dtype):
    order = np.argsort(rows, kind="stable")
    r = rows[order]
    starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    return r[starts], np.add.reduceat(vals[order].astype(dtype), starts, axis=0)


def reference(poses, fixed, ei, ej, meas, info, phi, xs=(), chunk=CHUNK) -> Reference:
    """The reference at `poses` for the graph (arrays as sgo_set_graph_se2's) and the vectors xs ((n,3) each, hessian order)."""
    poses = np.asarray(poses, dtype=np.float64)
    hidx, free = npo.hessian_index(fixed)
    n = free.size
    V = poses.shape[0]
    E = int(np.asarray(ei).size)
    full = []
    for x in xs:
        xf = np.zeros((V, 3))
        xf[free] = np.asarray(x, dtype=np.float64).reshape(n, 3)
        full.append(xf)
    nx = len(full)
    K = 3 + 9 + 3 * nx
    acc = np.zeros((n, K), dtype=LD)
    acc_abs = np.zeros((n, K))
    e2 = np.empty(E, dtype=LD)
    e2_abs = np.empty(E)
    chi2 = robust = LD(0)
    chi2_abs = robust_abs = 0.0
    for k0 in range(0, E, chunk):
        sl = slice(k0, min(E, k0 + chunk))
        a = np.asarray(ei[sl], dtype=np.int64)
        c = np.asarray(ej[sl], dtype=np.int64)
        t = edge_terms(poses[a], poses[c], np.asarray(meas[sl]), np.asarray(info[sl]), np.asarray(phi[sl]),
                       [xf[a] for xf in full], [xf[c] for xf in full])
        e2[sl] = t["e2"]
        e2_abs[sl] = t["e2_abs"]
        chi2 += t["e2"].sum()
        robust += t["rho0"].astype(LD).sum()
        chi2_abs += float(t["e2_abs"].sum())
        robust_abs += float((t["wbar"] * t["e2_abs"]).sum())
        hi, hj = hidx[a], hidx[c]
        fi, fj = hi >= 0, hj >= 0
        m = len(a)
        vals = np.concatenate([np.concatenate([t["bi"], t["Hii"].reshape(m, 9)] + t["yi"], axis=1)[fi],
                               np.concatenate([t["bj"], t["Hjj"].reshape(m, 9)] + t["yj"], axis=1)[fj]])
        vabs = np.concatenate([np.concatenate([t["bi_abs"], t["Hii_abs"].reshape(m, 9)] + t["yi_abs"], axis=1)[fi],
                               np.concatenate([t["bj_abs"], t["Hjj_abs"].reshape(m, 9)] + t["yj_abs"], axis=1)[fj]])
        rows = np.concatenate([hi[fi], hj[fj]])
        if rows.size:
            r, s = _segment_sum(rows, vals, LD)
            acc[r] += s
            r, s = _segment_sum(rows, vabs, np.float64)
            acc_abs[r] += s
    ref = Reference(free=free, b=acc[:, 0:3], b_abs=acc_abs[:, 0:3], diag=acc[:, 3:12].reshape(n, 3, 3),
                    diag_abs=acc_abs[:, 3:12].reshape(n, 3, 3), chi2=chi2, chi2_abs=chi2_abs, robust=robust,
                    robust_abs=robust_abs, e2=e2, e2_abs=e2_abs)
    for q in range(nx):
        ref.hx.append(acc[:, 12 + 3 * q:15 + 3 * q])
        ref.hx_abs.append(acc_abs[:, 12 + 3 * q:15 + 3 * q])
    return ref


def ratio(got, ref, abs_sum) -> float:
    """max over entries of |got - ref| / (U abs_sum); an entry with abs_sum = 0 must match exactly (inf otherwise)."""
    got = np.asarray(got, dtype=LD)
    ref = np.asarray(ref, dtype=LD)
    abs_sum = np.asarray(abs_sum, dtype=np.float64)
    err = np.abs(got - ref).astype(np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(abs_sum > 0, err / (U * abs_sum), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r))


def ratios(ref: Reference, b=None, diag=None, chi2=None, robust=None, e2=None, hx=()) -> dict:
    """error / (U abs) of every given output against the reference: {output name: worst ratio}."""
    out = {}
    if b is not None:
        out["b"] = ratio(np.asarray(b).reshape(-1, 3), ref.b, ref.b_abs)
    if diag is not None:
        out["diag"] = ratio(np.asarray(diag).reshape(-1, 3, 3), ref.diag, ref.diag_abs)
    if chi2 is not None:
        out["chi2"] = ratio(chi2, ref.chi2, ref.chi2_abs)
    if robust is not None:
        out["robust_chi2"] = ratio(robust, ref.robust, ref.robust_abs)
    if e2 is not None:
        out["edge_chi2"] = ratio(e2, ref.e2, ref.e2_abs)
    for q, y in enumerate(hx):
        out[f"hx{q}"] = ratio(np.asarray(y).reshape(-1, 3), ref.hx[q], ref.hx_abs[q])
    return out


def failures(r: dict, c: float = C) -> list:
    """The outputs of a ratios() dict outside the bound C U abs."""
    return [k for k, v in r.items() if not v <= c]
