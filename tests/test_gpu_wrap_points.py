"""The angle wrap at +-pi through every kernel that forms it (sparse_gslam_amd/csrc/sgo_device.h: norm_theta; sgo_rules.h:
closure_norm_theta).  tests/wrap_cases.py holds the table of points, the cell graph that carries a point's e_theta through a kernel
bit for bit, and the cells' closed forms; tests/test_wrap_cases.py qualifies all three on the CPU.  One context on the cell graph
(340 poses) per test.

Per call site, the observable and its bar:
  k_edge_prepare, edge_error in k_linearize (group and tile)   linearize(): b_theta = -+e_theta, H_thth = 1, the theta row and column
                                  of the block otherwise 0, b_x = b_y = 0: bit for bit, no point skipped
  k_chi2, k_edge_robust, k_edge_gate   edge_chi2(), edge_robust(): fl(e_theta^2) (and weight 1) bit for bit on the identity cells;
                                  chi2() their sum within the sum's own roundings; gate_edges(): the flag is edge_chi2() > chi2_max at a
                                  chi2_max that stands between pi^2 and (pi - ulp)^2.  On the coupled cells, where the SIGN of e_theta
                                  shows in e^2: kernel_reference's bound C U abs against its long-double reference
  k_direct, k_mf_edges + k_mf_update   optimize(1) on the direct and the multifrontal path: theta of every free pose bit for bit the
                                  closed form wrap(fl(theta + b_theta)), in [-pi, pi); x, y and the fixed poses untouched
  k_pose_update                   optimize(1) with direct_rows=0 (PCG): every theta in [-pi, pi), equal to the closed form modulo 2pi
                                  within 10 d_path |dx|, the shifted cells on the declared side
  k_mf_edges<LM> + k_lm_trial     optimize_lm(1, 1e-300): the bits of optimize(1) on the multifrontal path (1 + 1e-300 is 1)
  k_lm_trial_pcg                  optimize_lm_pcg(1, 1e-300): as the PCG row
  k_dl_forms + k_dl_trial         optimize_dogleg(1): the bits of the multifrontal optimize(1) -- no damping is added while no solve
                                  has failed, the radius 1e4 holds the Gauss-Newton step and h = 0 b + 1 g is g; optimize_dogleg_pcg(1):
                                  as the PCG row (its solve is the PCG's)
  k_ov_lin + k_ov_finish          the cells appended with update_graph to a resident graph, every free pose a chain row; eight cells
                                  with a partner pose that the overlay makes a hub (k_ov_finish's other update loop): edge_chi2()
                                  bit for bit, poses as the PCG row
  k_closure_search                closure_search from one query pose with theta = 0 over poses with theta = -t for every argument t
                                  that reaches a wrap anywhere in the table: rel[2] bit for bit the host rule's
On the cells with a second, anchor edge at every free pose (wrap_cases.cells(anchored=True): no edge is a bridge, and a gate or a
hypothesis may take the cell's own edge away):
  k_fs_rhs                        candidate_gate on the anchors' graph with every cell's own edge as a candidate: P and d2 at
                                  tests/test_gpu_fsolve.py's bars against the cell's 3x3 closed form, decisions the reference's
  k_loo_edges                     edge_leave_one_out of every cell edge at tests/test_gpu_edge_loo.py's bars (its own comparison)
  k_edge_cands                    edge_joint: e_theta bit for bit the specification's, N at tests/test_gpu_edge_groups.py's bar
  batched hypotheses              optimize_hypotheses on the multifrontal path with a workspace, every cell's edge off in one
                                  hypothesis and on in the others: the unbatched loop's bits, as tests/test_gpu_hypotheses_mfront.py asks

d_path (the convention of tests/test_gpu_robust_points.py): the worst disagreement of that path's optimize(1) with the closed form on
the interior cells only, relative to |dx|, floored at 1e-14.  Any other cell may differ by 10 d_path |dx| (modulo 2pi); a cell
whose step is 0 may not move.  Every test prints what it measured; wrap_cases.MEASURED keeps it.

"Bit for bit" is wrap_cases.same: the same uint64 pattern, except that -0.0 and 0.0 count as one value (one angle, one gradient; an
assembly's sum may give either), and a NaN is never the same."""
import functools
import re

import numpy as np
import pytest

import kernel_reference as kr
import wrap_cases as wc
from sparse_gslam_amd import capi

pytestmark = pytest.mark.gpu
PI, TWO_PI = wc.PI, wc.TWO_PI
PATHS = {"direct": ({}, "direct_ldlt"), "mfront": (dict(direct_rows=1), "multifrontal_cholesky"), "pcg": (dict(direct_rows=0), "pcg")}


@functools.lru_cache(maxsize=None)
def _ref(coupled=False, anchored=False):
    """the cell graph and its closed forms (of the cells' own edges); computed once, read only"""
    C = wc.cells(coupled=coupled, anchored=anchored)
    e, b, new, dx = wc.closed_form(C)
    for a in tuple(C[:7]) + (e, b, new, dx):
        a.setflags(write=False)
    return C, e, b, new, dx


def _args(C):
    return C.poses, C.fixed, C.ei, C.ej, C.meas, C.info, C.phi


def _open(C, path="pcg"):
    opts, starts = PATHS[path]
    o = capi.Optimizer(0, **opts)
    o.set_graph(*_args(C))
    assert o.solver_description().startswith(starts), o.solver_description()
    return o


def _report(name, C, ok):
    """every cell named that is not `ok`"""
    bad = np.flatnonzero(~ok)
    return [(name, int(k), str(C.kind[k]), int(C.orient[k]), float(C.ti[k]).hex(), float(C.tj[k]).hex(), float(C.zeta[k]).hex()) for k in bad[:12]]


# ------------------------------------------------------------------ the error: linearize, chi2, the gate
@pytest.mark.parametrize("kernel", ["group", "tile"])
def test_linearize_bit_for_bit_on_every_cell(kernel, monkeypatch):
    C, e, b, new, dx = _ref()
    if kernel == "tile":
        monkeypatch.setenv("SGO_SPMV0", "tile")
    else:
        monkeypatch.delenv("SGO_SPMV0", raising=False)
    with _open(C) as o:
        gb, diag, c2, rc2 = o.linearize()
        assert np.array_equal(o.free_ids(), C.free)
    ok = wc.same(gb[:, 2], b)
    worst = np.abs(gb[:, 2] - b).max()
    print(f"k_linearize ({kernel}): {C.ti.size} cells, {int((~ok).sum())} with another b_theta than -+e_theta (largest difference {worst:.3g})")
    assert ok.all(), _report("b_theta", C, ok)
    assert np.all(gb[:, :2] == 0.0)
    assert np.all(diag[:, 2, 2] == 1.0) and np.all(diag[:, 2, :2] == 0.0) and np.all(diag[:, :2, 2] == 0.0)
    want = float(np.sum((e * e).astype(np.longdouble)))
    assert abs(c2 - want) <= kr.U * C.ti.size * want and rc2 == c2


def test_chi2_robust_and_gate_on_the_identity_cells():
    C, e, b, new, dx = _ref()
    e2 = e * e
    with _open(C) as o:
        g2 = o.edge_chi2()
        plain, robust = o.chi2()
        rho0, w = o.edge_robust()
        ok = wc.same(g2, e2)
        print(f"k_chi2: {C.ti.size} identity cells, {int((~ok).sum())} with another e^2 than fl(e_theta^2)")
        assert ok.all(), _report("edge_chi2", C, ok)
        assert np.all(wc.same(rho0, e2)) and np.all(w == 1.0)
        want = float(np.sum(e2.astype(np.longdouble)))
        assert abs(plain - want) <= kr.U * C.ti.size * want and robust == plain
        # the gate between (pi - ulp)^2 and pi^2: e_theta = -pi is gated, pi - ulp is not
        lo, hi = (PI - wc.ULP) ** 2, PI * PI
        assert lo < hi and (e2 == hi).sum() >= 10 and (e2 == lo).sum() >= 10
    # (a gate that would leave a free pose without an edge is refused: the cells with their anchors)
    A = _ref(False, True)[0]
    n = A.ti.size
    with _open(A) as o:
        g2 = o.edge_chi2()
        assert np.all(wc.same(g2[:n], e2))
        k, gated = o.gate_edges(np.arange(n, dtype=np.int32), lo)
        print(f"k_edge_gate: {k} of {n} cell edges gated at chi2_max = (pi - ulp)^2")
        assert np.array_equal(gated, g2[:n] > lo) and k == int(gated.sum()) and np.array_equal(gated, e2 > lo)


def test_the_sign_of_e_theta_in_e2_on_the_coupled_cells():
    C, e, b, new, dx = _ref(True)
    ref = kr.reference(C.poses, C.fixed.astype(bool), C.ei, C.ej, C.meas, C.info, C.phi)
    with _open(C) as o:
        g2 = o.edge_chi2()
        plain, robust = o.chi2()
        rho0, w = o.edge_robust()
        gb, diag, c2, rc2 = o.linearize()
        r = kr.ratios(ref, b=gb, diag=diag, chi2=c2, robust=rc2, e2=g2)
        s = kr.ratios(ref, chi2=plain, robust=robust, e2=rho0)
        r["sgo_chi2"], r["sgo_robust_chi2"], r["edge_robust"] = s["chi2"], s["robust_chi2"], s["edge_chi2"]
        print("coupled cells, error / (U abs) against kernel_reference (bound C = 16): " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
        per = np.abs(g2.astype(np.longdouble) - ref.e2).astype(np.float64) / (kr.C * kr.U * ref.e2_abs)
        assert not kr.failures(r), (r, _report("edge_chi2", C, per <= 1.0))
        assert np.all(w == 1.0)
    A = _ref(True, True)[0]
    n = A.ti.size
    refA = kr.reference(A.poses, A.fixed.astype(bool), A.ei, A.ej, A.meas, A.info, A.phi)
    with _open(A) as o:
        g2 = o.edge_chi2()
        assert not kr.failures(kr.ratios(refA, e2=g2))
        thr = float(np.median(g2[:n]))
        k, gated = o.gate_edges(np.arange(n, dtype=np.int32), thr)
        assert np.array_equal(gated, g2[:n] > thr) and k == int(gated.sum()) and 0 < k < n
        # the reference's decision wherever its own bound leaves no doubt
        sure = np.abs(refA.e2[:n].astype(np.float64) - thr) > kr.C * kr.U * refA.e2_abs[:n]
        assert sure.sum() >= 0.9 * n and np.array_equal(gated[sure], refA.e2[:n].astype(np.float64)[sure] > thr)


# ------------------------------------------------------------------ the update: every solver path
def _step(o, C, how="optimize"):
    o.set_poses(C.poses)
    if how == "optimize":
        d, st = o.optimize(1)
    elif how == "lm":
        d, st = o.optimize_lm(1, 1e-300)
        assert st["trials"] == [1] and st["lambda0"] == 1e-300, st
    elif how == "lm_pcg":
        d, st = o.optimize_lm_pcg(1, 1e-300)
        assert st["trials"] == [1] and st["lambda0"] == 1e-300, st
    elif how == "dogleg":
        d, st = o.optimize_dogleg(1)
        assert st["trials"] == [1] and st["step_kind"] == [0] and st["lam"] == 0.0 and st["delta0"] == 1e4, st
    else:
        d, st = o.optimize_dogleg_pcg(1)
        assert st["trials"] == [1] and st["step_kind"] == [0] and st["lam"] == 0.0 and st["delta0"] == 1e4, st
    assert d == 1, (d, o.last_error())
    return o.get_poses()


def _mod(d):
    """a difference of angles modulo 2pi, in [-pi, pi]"""
    return np.remainder(d + PI, TWO_PI) - PI


def _check_exact(name, C, P, new, free=None, fixed=None):
    free = C.free if free is None else free
    th = P[free, 2]
    ok = wc.same(th, new)
    print(f"{name}: {free.size} free poses, {int((~ok).sum())} with other bits than wrap(fl(theta + b_theta)); largest difference "
          f"modulo 2pi {np.abs(_mod(th - new)).max():.3g}")
    assert ok.all(), _report(name, C, ok)
    assert np.all((th >= -PI) & (th < PI)) and np.all(P[free, :2] == 0.0)
    fx = C.c if fixed is None else fixed
    assert np.array_equal(P[fx].view(np.uint64), C.poses[fx].view(np.uint64))


def _check_bar(name, C, P, new, dx, kinds, free=None):
    """the PCG row: in range, the closed form modulo 2pi within 10 d_path |dx| with d_path from the interior cells, the shifted cells
    on the declared side -> (d_path, the worst ratio)"""
    free = C.free if free is None else free
    th = P[free, 2]
    assert np.all((th >= -PI) & (th < PI)), _report(name + ": out of [-pi, pi)", C, (th >= -PI) & (th < PI))
    err = np.abs(_mod(th - new))
    interior = np.isin(kinds, ("interior", "update-interior"))
    assert interior.sum() >= 10
    d_path = max(1e-14, float((err[interior] / np.abs(dx[interior])).max()))
    bar = 10.0 * d_path * np.abs(dx)
    with np.errstate(divide="ignore", invalid="ignore"):           # a cell whose step is 0 has the bar 0: it must not move at all
        ratio = np.where(bar > 0, err / bar, np.where(err == 0.0, 0.0, np.inf))
    shifted = kinds == "update-shifted"
    side_ok = np.sign(th[shifted]) == np.sign(new[shifted])
    xy = np.abs(P[free, :2]).max()
    print(f"{name}: d_path {d_path:.3g} from {int(interior.sum())} interior cells; worst |theta - closed form| mod 2pi over its bar "
          f"{ratio.max():.3g} (cell {int(np.argmax(ratio))}, {kinds[int(np.argmax(ratio))]}); {int(shifted.sum())} shifted cells, "
          f"{int((~side_ok).sum())} on the wrong side; largest |x|, |y| {xy:.3g}; bit-identical to the closed form: {int(wc.same(th, new).sum())} of {free.size}")
    assert ratio.max() <= 1.0, _report(name, C, ratio <= 1.0)
    assert shifted.sum() >= 16 and side_ok.all()
    assert xy <= 10.0 * d_path
    return d_path, float(ratio.max())


@pytest.mark.parametrize("path", ["direct", "mfront"])
def test_one_iteration_bit_for_bit_on_the_factorisation_paths(path):
    C, e, b, new, dx = _ref()
    with _open(C, path) as o:
        P = _step(o, C)
        _check_exact(f"optimize(1), {path}", C, P, new)
        if path == "mfront":
            Q = _step(o, C, "lm")
            assert np.array_equal(Q.view(np.uint64), P.view(np.uint64)), _report("optimize_lm", C, wc.same(Q[C.free, 2], P[C.free, 2]))
            Q = _step(o, C, "dogleg")
            assert np.array_equal(Q.view(np.uint64), P.view(np.uint64)), _report("optimize_dogleg", C, wc.same(Q[C.free, 2], P[C.free, 2]))
            print("optimize_lm(1, 1e-300) and optimize_dogleg(1): the bits of optimize(1)")
        assert o.solver_description().startswith(PATHS[path][1])


@pytest.mark.parametrize("how", ["optimize", "lm_pcg", "dogleg_pcg"])
def test_one_iteration_on_the_pcg_path(how):
    C, e, b, new, dx = _ref()
    with _open(C, "pcg") as o:
        P = _step(o, C, how)
        _check_bar(f"{how}, pcg", C, P, new, dx, C.kind)
        assert np.array_equal(P[C.c].view(np.uint64), C.poses[C.c].view(np.uint64))
        assert o.solver_description().startswith("pcg")


# ------------------------------------------------------------------ the overlay
N_BASE, N_HUB = 8, 8


def _overlay_graph():
    """N_BASE resident cells (interior controls), then every cell of the table appended: new fixed and new free poses, the free ones
    chain rows of the overlay.  The first N_HUB exact update cells that land at +-pi get a partner: one more new free pose w at the
    free pose's angle, joined to it by an edge of error 0 exactly.  The pair's theta system is [[2, -1], [-1, 1]] (dx_v, dx_w) =
    (b_theta, 0): both move by b_theta, the cell's own closed form; w's id is not next to v's, so the overlay takes w out of the
    chain as a hub."""
    C, e, b, new, dx = _ref()
    base = np.flatnonzero(C.kind == "interior")[:N_BASE]
    n, nb = C.ti.size, base.size
    hubs = np.flatnonzero((C.kind == "update-exact") & (np.abs(np.abs(C.poses[C.free, 2] + dx) - PI) < 1e-9))[:N_HUB]
    assert nb == N_BASE and hubs.size == N_HUB and hubs.max() < n - 1
    V = 2 * nb + 2 * n + hubs.size
    poses, fixed = np.zeros((V, 3)), np.zeros(V, dtype=np.uint8)
    poses[: 2 * nb] = np.concatenate([C.poses[[C.c[k], C.free[k]]] for k in base])
    fixed[: 2 * nb : 2] = 1
    poses[2 * nb : 2 * nb + 2 * n], fixed[2 * nb : 2 * nb + 2 * n] = C.poses, C.fixed
    ei = np.r_[[2 * q + (C.ei[k] % 2) for q, k in enumerate(base)], C.ei + 2 * nb, C.free[hubs] + 2 * nb].astype(np.int32)
    w_ids = 2 * nb + 2 * n + np.arange(hubs.size)
    ej = np.r_[[2 * q + (C.ej[k] % 2) for q, k in enumerate(base)], C.ej + 2 * nb, w_ids].astype(np.int32)
    poses[w_ids, 2] = C.poses[C.free[hubs], 2]
    meas = np.r_[C.meas[base], C.meas, np.zeros((hubs.size, 3))]
    info = np.r_[C.info[base], C.info, np.tile(wc.INFO_ID, (hubs.size, 1))]
    phi = np.full(ei.size, -1.0)
    free = np.r_[np.arange(1, 2 * nb, 2), C.free + 2 * nb, w_ids]
    kinds = np.r_[C.kind[base], C.kind, np.full(hubs.size, "hub")]
    want = np.r_[new[base], new, new[hubs]]
    step = np.r_[dx[base], dx, dx[hubs]]
    e2 = np.r_[(e * e)[base], e * e, np.zeros(hubs.size)]
    return (poses, fixed, ei, ej, meas, info, phi), nb, free, kinds, want, step, e2


def test_cells_appended_as_an_overlay():
    args, nb, free, kinds, want, step, e2 = _overlay_graph()
    C = _ref()[0]
    with capi.Optimizer(0, direct_rows=0) as o:
        s = slice(None, nb)
        o.set_graph(args[0], args[1], *(a[s] for a in args[2:]))
        assert o.optimize(1)[0] == 1
        o.update_graph(*args, nb)
        desc = o.solver_description()
        assert "incremental overlay" in desc, desc
        g2 = o.edge_chi2()
        ok = wc.same(g2, e2)
        print(f"k_ov_lin: {g2.size} edges ({nb} resident), {int((~ok).sum())} with another e^2 than fl(e_theta^2); {desc.split('; incremental overlay: ')[1].split(';')[0]}")
        assert ok.all(), [(int(k), float(g2[k]).hex(), float(e2[k]).hex()) for k in np.flatnonzero(~ok)[:12]]
        o.set_poses(args[0])
        assert o.optimize(1)[0] == 1
        assert "incremental overlay" in o.solver_description()
        P = o.get_poses()
    # a view of the graph with one row per free pose, for the reports
    K = C._replace(kind=kinds, orient=np.zeros(free.size, dtype=np.int64), ti=args[0][free, 2], tj=args[0][free, 2], zeta=np.zeros(free.size))
    _check_bar("optimize(1), overlay", K, P, want, step, kinds, free=free)
    # the overlay's own account of what it built: every appended free pose a row, the eight partners hubs (k_ov_finish's other loop)
    m = re.search(r"incremental overlay: (\d+) appended rows \((\d+) hubs\), (\d+) touched rows, (\d+) appended edges", desc)
    assert m, desc
    assert (kinds == "hub").sum() == N_HUB
    assert [int(x) for x in m.groups()] == [free.size - nb, N_HUB, 0, args[2].size - nb], (desc, free.size, nb)
    fx = np.flatnonzero(args[1])
    assert np.array_equal(P[fx].view(np.uint64), args[0][fx].view(np.uint64))


# ------------------------------------------------------------------ the closure search
def test_closure_search_rel_theta_is_the_host_rules():
    t = wc.wrap_arguments(wc.POINTS)
    n = t.size
    V = n + 2
    poses, fixed = np.zeros((V, 3)), np.zeros(V, dtype=np.uint8)
    fixed[0] = 1
    poses[2:, 2] = -t                                   # theta_c - theta_j = 0 - (-t) = t, exactly
    poses[1:, 0] = 0.5 * np.arange(V - 1)
    poses[1:, 1] = 0.25
    ei, ej = np.zeros(V - 1, dtype=np.int32), np.arange(1, V, dtype=np.int32)
    meas = np.zeros((V - 1, 3))
    meas[:, :2] = poses[1:, :2]
    info, phi = np.tile(wc.INFO_ID, (V - 1, 1)), np.full(V - 1, -1.0)
    with capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(poses, fixed, ei, ej, meas, info, phi)
        assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
        ids = np.arange(2, V, dtype=np.int32)
        cnt, m2, rel, cov, sg, near = o.closure_search([1], ids, 1.0, 6.0)
    host = np.array([capi.closure_search_rule(poses[j], poses[1], np.eye(3), np.zeros((3, 3)), np.eye(3), 1.0)[0] for j in ids])
    want = np.array([wc.wrap(float(a)) for a in t])
    assert np.all(wc.same(host[:, 2], want))
    ok = wc.same(rel[0, :, 2], host[:, 2])
    print(f"k_closure_search: {n} wrap arguments, {int((~ok).sum())} with another rel[2] than the host rule's; largest difference "
          f"{np.abs(rel[0, :, 2] - host[:, 2]).max():.3g}")
    assert ok.all(), [(float(t[k]).hex(), float(rel[0, k, 2]).hex(), float(host[k, 2]).hex()) for k in np.flatnonzero(~ok)[:12]]
    assert np.abs(rel[0, :, :2] - host[:, :2]).max() <= 1e-12 * np.abs(host[:, :2]).max()


# ------------------------------------------------------------------ candidates, leave-one-out, the joint table, batched hypotheses
def _anchored_namespace(A):
    import types
    return types.SimpleNamespace(fixed=A.fixed.astype(bool), ei=A.ei, ej=A.ej, meas=A.meas, info=A.info, phi=A.phi)


def test_candidate_gate_with_every_cell_edge_as_a_candidate():
    """k_fs_rhs: the graph of the anchors alone, the cells' own edges as candidates; tests/test_gpu_fsolve.py's bars (1e-6 of
    max |Omega^-1 + P_ref| on P, 1e-6 relative on d2; an error of 0 gives d2 = 0 exactly), decisions the reference's"""
    import fsolve_reference as fr
    from oracle import np_oracle as npo
    from test_gpu_fsolve import BAR
    A, e, b, new, dx = _ref(False, True)
    n = A.ti.size
    an = slice(n, 2 * n)
    ci, cj, cm, cinfo = A.ei[:n], A.ej[:n], A.meas[:n], A.info[:n]
    # per cell: Sigma of the free pose from its anchor alone, the candidate's Jacobian over the free pose
    Aa, Ba = npo.edge_jacobians(A.poses[A.ei[an]], A.poses[A.ej[an]], A.meas[an])
    Oa = npo.info_full(A.info[an])
    Ac, Bc = npo.edge_jacobians(A.poses[ci], A.poses[cj], cm)
    ec = npo.edge_error(A.poses[ci], A.poses[cj], cm)
    assert np.all(wc.same(ec[:, 2], e))
    Pref, d2ref = np.empty((n, 3, 3)), np.empty(n)
    for k in range(n):
        Sigma = np.linalg.inv(Ba[k].T @ Oa[k] @ Ba[k])
        J = Bc[k] if A.orient[k] == 0 else Ac[k]
        Q = J @ Sigma @ J.T
        Pref[k] = 0.5 * (Q + Q.T)
        d2ref[k] = ec[k] @ np.linalg.solve(np.eye(3) + Pref[k], ec[k])
    gate = 4.0
    with capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(A.poses, A.fixed, A.ei[an], A.ej[an], A.meas[an], A.info[an], A.phi[an])
        assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
        npass, d2, P, ok = o.candidate_gate(ci, cj, cm, cinfo, gate)
    pos = d2ref > 0
    rp = max(float(np.abs(P[k] - Pref[k]).max() / np.abs(np.eye(3) + Pref[k]).max()) for k in range(n))
    rd = float(np.max(np.abs(d2[pos] - d2ref[pos]) / d2ref[pos]))
    print(f"k_fs_rhs: {n} candidates; P {rp:.3g} of max |Omega^-1 + P_ref|, d2 {rd:.3g} relative (bars {BAR:g})")
    assert rp <= BAR and rd <= BAR and np.all(d2[~pos] == 0.0)
    assert np.array_equal(ok, d2 <= gate) and npass == int(ok.sum())
    sure = np.abs(d2ref / gate - 1.0) > 1e-3
    assert sure.sum() >= 0.9 * n and np.array_equal(ok[sure], d2ref[sure] <= gate) and 0 < npass < n


def test_leave_one_out_of_every_cell_edge():
    """k_loo_edges, against loo_reference at tests/test_gpu_edge_loo.py's own bars"""
    from test_gpu_edge_loo import _compare
    A, e, b, new, dx = _ref(False, True)
    n = A.ti.size
    with _open(A, "mfront") as o:
        F, d2, red, fail = _compare("wrap cells", _anchored_namespace(A), o, np.arange(n, dtype=np.int32), min_compared=0.0)
    assert (F["redundancy"] >= 5e-3).all() and np.isfinite(d2).all()              # no cell edge is a bridge: all are compared
    assert not fail.any()                                  # (every d2 is far below the gate: max e_theta^2 / (1 + P) < 11.345)


def test_joint_table_of_the_cell_edges():
    """k_edge_cands (sgo_egroup.hip): e bit for bit the specification's, N against egroup_reference at tests/test_gpu_edge_groups.py's bar"""
    import egroup_reference as eg
    import loo_reference as lr
    import selinv_reference as sr
    A, e, b, new, dx = _ref(False, True)
    g = _anchored_namespace(A)
    # the branch, range, part and side points of orientation 0 come first in the table
    edges = np.arange(min(capi.JOINT_MAX_CANDIDATES, A.ti.size), dtype=np.int32)
    assert {"branch", "range", "part", "side"} <= set(A.kind[edges])
    S = lr.Edges(A.poses, g.fixed, g.ei, g.ej, g.meas, g.info, w=np.ones(g.ei.size))
    T = eg.table(S, edges)
    with _open(A, "mfront") as o:
        N, ge, wj = o.edge_joint(edges)
    ok = wc.same(ge[:, 2], e[edges])
    rn = np.abs(N - T["N"]).max() / np.abs(T["N"]).max()
    print(f"k_edge_cands: {edges.size} cell edges, {int((~ok).sum())} with another e_theta than the specification's; N {rn:.2e} of max |N_ref|")
    assert ok.all(), _report("edge_joint", A, np.r_[ok, np.ones(A.ti.size - edges.size, dtype=bool)])
    assert np.all(ge[:, :2] == 0.0) and np.all(wj == 1.0) and rn <= sr.DEVICE_BAR


def test_batched_hypotheses_with_every_cell_switched_off_and_on():
    """optimize_hypotheses on the multifrontal path with a workspace granted: every cell's own edge off in one hypothesis and on in
    the others; everything a hypothesis returns is, bit for bit, the unbatched loop's turn on a twin context"""
    from test_gpu_hypotheses import check_against_loop, host_loop
    A, e, b, new, dx = _ref(False, True)
    n = A.ti.size
    M = np.zeros((3, 2 * n), dtype=np.uint8)
    M[1, 0:n:2] = 1
    M[2, 1:n:2] = 1
    iters = 2
    with _open(A, "mfront") as twin:
        L = host_loop(twin, A.info, M, iters, 0.0)
    with _open(A, "mfront") as o:
        per = o.hypotheses_bytes(iters, True)
        assert per > 0
        o.set_hypotheses_workspace(3 * per)
        R = o.optimize_hypotheses(M, iters, 0.0)
        assert R["route"] == capi.HYP_BATCHED, R["route"]
    check_against_loop(R, L, iters, "wrap cells")
    th = R["poses"][:, A.free, 2]
    assert np.all((th >= -PI) & (th < PI))
    print(f"optimize_hypotheses: 3 hypotheses over {n} cells, the loop's bits; all angles in [-pi, pi)")
