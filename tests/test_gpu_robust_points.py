"""The robust kernels at their branch points, through every kernel that forms them (sparse_gslam_amd/csrc/sgo_device.h: robustify,
edge_weight<KINDS>).  tests/robust_cases.py holds the table of points, the cell graph that carries a point's e2 through a kernel
bit for bit, and the closed form of a cell in long double; tests/test_robust_cases.py qualifies all three on the CPU.

Per call site, the observable and what it is compared with:
  k_edge_robust   edge_robust() per edge         robust_reference.rho_ld within C_BOUND EPS scale, the declared side of the
                                                 threshold, (e2, 1) exactly on the quadratic side and weight 0 exactly on the cut-off one
  k_chi2          chi2()'s robust sum            one kerneled edge at a time (every other edge's information zeroed, which adds
                                                 exact zeros): that edge's rho0 within its own bound; then the whole table's sum
  k_linearize     linearize(): b, diagonal       the cell's closed form with the reference's w, per entry within
                  block (group and tile kernel)  EPS (C_BOUND Hw + 8 Ha): the weight's bound carried by |J|^T Omega |J|, plus the
                                                 assembly's own roundings (at most 8 per entry) on the sum of its terms' magnitudes
  k_direct, k_mf_edges, PCG                      poses after optimize(1) and robust_chi2[0] on the points with `solve`, against the
                                                 cell's long-double step (tolerance below)
  k_mf_edges<LM>  optimize_lm(1, 1e-300)         the bits of optimize(1) on the multifrontal path
  k_ov_lin        the kerneled edges appended with update_graph to a resident graph of anchors, kinds set on the appended ids:
                  edge_robust(), chi2(), poses after optimize(1).  (linearize() is refused while an overlay is resident: sgo.h.)
  k_loo_edges, the edge kernel of sgo_egroup.hip   edge_leave_one_out / edge_joint + edge_groups on the kerneled edges with
                  `solve`, against loo_reference / egroup_reference fed the reference's w, at test_gpu_edge_loo.py's and
                  test_gpu_edge_groups.py's own bars; a kerneled edge of weight 0 has redundancy 1 exactly, and the anchor beside
                  it has become a bridge: NaN, no decision

Tolerance of the solves: d_path is measured first -- the worst relative disagreement, per cell, of the path's optimize(1) with the
closed form on the same cells with every kind NONE (existing code against the reference), floored at 1e-14.  A kerneled cell's
pose may differ from its closed form by 10 d_path |dx| plus what the weight's bound moves of the step,
|H^-1| (|J|^T Omega |e| + |J|^T Omega |J| |dx|) C_BOUND EPS.  Every test prints what it measured; robust_cases.MEASURED keeps it."""
import functools
import types

import numpy as np
import pytest

import egroup_reference as eg
import loo_reference as lr
import robust_cases as rc
import robust_reference as rr
import selinv_reference as sr
from sparse_gslam_amd import capi

pytestmark = pytest.mark.gpu
POINTS = rc.POINTS
SOLVE = tuple(p for p in POINTS if p.solve)
LD = rc.LD
PATHS = {"direct": ({}, "direct_ldlt"), "mfront": (dict(direct_rows=1), "multifrontal_cholesky"), "pcg": (dict(direct_rows=0), "pcg")}


def _f(a):
    return np.asarray(a, dtype=LD).astype(np.float64)


def _graph_args(C, upto=None):
    s = slice(None, upto)
    return C.poses, C.fixed, C.ei[s], C.ej[s], C.meas[s], C.info[s], C.phi[s]


def _set_kinds(o, C):
    """NONE and DCS came with set_graph's phi; every other kind is set here"""
    ids = np.flatnonzero(C.kind >= rr.HUBER)
    if ids.size:
        o.set_robust_kernels(ids, C.kind[ids], C.delta[ids])


def _open(C, path="pcg"):
    opts, starts = PATHS[path]
    o = capi.Optimizer(0, **opts)
    o.set_graph(*_graph_args(C))
    assert o.solver_description().startswith(starts), o.solver_description()
    _set_kinds(o, C)
    assert o.solver_description().startswith(starts), o.solver_description()
    return o


@functools.lru_cache(maxsize=None)
def _ref(which):
    """the cells of the whole table or of its `solve` points, and the reference's pairs per point; computed once, read only"""
    pts = POINTS if which == "all" else SOLVE
    C = rc.cells(pts)
    r0, w, b0, b1 = rc.reference(pts)
    for a in (r0, w, b0, b1):
        a.setflags(write=False)
    return pts, C, r0, w, b0, b1


def _check_pairs(name, pts, C, rho0, w):
    """edge_robust()'s output on the cell graph against the table -> worst ratio per kind"""
    n = C.n_anchor
    e2a = float(rc.E_ANCHOR @ rc.OMEGA @ rc.E_ANCHOR)
    assert np.all(w[:n] == 1.0) and np.abs(rho0[:n] - e2a).max() <= rr.C_BOUND * rr.EPS * e2a      # the anchors carry no kernel
    bad, worst = rc.check([pts[t] for t in C.point], rho0[C.kedge], w[C.kedge], name)
    print(f"{name}: {C.point.size} kerneled edges ({len(pts)} points, two orientations); worst ratio to the bound per kind "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not bad, bad
    return worst


def test_edge_robust_at_every_point():
    pts, C, *_ = _ref("all")
    with _open(C) as o:
        rho0, w = o.edge_robust()
        e2 = o.edge_chi2()
    assert np.array_equal(e2[C.kedge].view(np.uint64), rc.arrays(pts)[2][C.point].view(np.uint64))   # the table's e2, bit for bit
    worst = _check_pairs("k_edge_robust", pts, C, rho0, w)
    assert set(worst) == set(rr.NAMES)


def test_chi2_one_edge_at_a_time_and_the_whole_sum():
    pts, C, r0, w, b0, b1 = _ref("all")
    n = C.n_anchor
    phi0 = np.array([pts[t].kind == rr.DCS and pts[t].d == 0.0 for t in C.point])
    worst = {}
    with _open(C) as o:
        plain, robust = o.chi2()
        e2a = float(rc.E_ANCHOR @ rc.OMEGA @ rc.E_ANCHOR)
        terms = np.r_[np.full(n, LD(e2a)), np.abs(r0[C.point])]
        want = terms.sum()
        # the table's own bounds, and the sum's roundings: E - 1 additions, each within EPS of a partial sum of the terms
        tol = b0[C.point].sum() + rr.EPS * (2 * n) * want
        print(f"k_chi2, whole sum: {float(robust)!r} against {float(want)!r}, |diff| / tol {float(abs(LD(robust) - want) / tol):.3g}")
        assert abs(LD(robust) - want) <= tol
    # One edge at a time, on the same cells with every pose fixed (an edge between fixed poses stays active for chi2 alone, and
    # its information may be zeroed) beside one free pose whose only edge has error 0: every other term of the sum is an exact zero.
    # DCS with phi = 0 stays as it is: its rho0 is an exact zero at e2 > 0, and 0 / 0 at e2 = 0.
    E = 2 * n
    args = (np.r_[C.poses, [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]], np.r_[np.ones(3 * n, dtype=np.uint8), [1, 0]].astype(np.uint8),
            np.r_[C.ei, [3 * n]].astype(np.int32), np.r_[C.ej, [3 * n + 1]].astype(np.int32), np.r_[C.meas, [[1.0, 0.0, 0.0]]],
            np.r_[C.info, [rc.OMEGA[np.triu_indices(3)]]], np.r_[C.phi, [-1.0]])
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*args)
        _set_kinds(o, C)
        quiet = np.r_[np.arange(n), C.kedge[~phi0]]
        o.set_edge_information(quiet, np.zeros((quiet.size, 6)))
        assert o.chi2()[1] == 0.0 and o.edge_chi2()[E] == 0.0
        for k in range(n):
            if phi0[k]:
                continue
            q, p = C.kedge[k], pts[C.point[k]]
            o.set_edge_information([q], C.info[[q]])
            plain, robust = o.chi2()
            o.set_edge_information([q], np.zeros((1, 6)))
            t = C.point[k]
            ratio = float(abs(LD(robust) - r0[t]) / b0[t]) if b0[t] > 0 else (0.0 if robust == float(r0[t]) else np.inf)
            worst[rr.NAMES[p.kind]] = max(worst.get(rr.NAMES[p.kind], 0.0), ratio)
            assert ratio <= 1.0, (p, robust, float(r0[t]), ratio)
    print("k_chi2, one edge at a time: worst ratio to the bound per kind " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("kernel", ["group", "tile"])
def test_linearisation_of_every_cell(kernel, monkeypatch):
    pts, C, r0, w, b0, b1 = _ref("all")
    if kernel == "tile":
        monkeypatch.setenv("SGO_SPMV0", "tile")
    else:
        monkeypatch.delenv("SGO_SPMV0", raising=False)
    with _open(C) as o:
        b, diag, c2, rc2 = o.linearize()
        assert np.array_equal(o.free_ids(), C.free)
    H, g, Ha, ga, Hw, gw = rc.cell_systems(C, pts, w)
    tolH = rr.EPS * (rr.C_BOUND * Hw + 8.0 * Ha)
    tolb = rr.EPS * (rr.C_BOUND * gw + 8.0 * ga)
    with np.errstate(invalid="ignore", divide="ignore"):
        qH = np.where(tolH > 0, np.abs(diag.astype(LD) - H) / tolH, np.where(diag == _f(H), 0.0, np.inf)).astype(np.float64)
        qb = np.where(tolb > 0, np.abs(b.astype(LD) - g) / tolb, np.where(b == _f(g), 0.0, np.inf)).astype(np.float64)
    per = {}
    for k in range(C.point.size):
        name = rr.NAMES[pts[C.point[k]].kind]
        per[name] = max(per.get(name, 0.0), float(qH[k].max()), float(qb[k].max()))
    print(f"k_linearize ({kernel}): {C.point.size} cells; worst ratio to the bound per kind " + ", ".join(f"{k} {v:.3g}" for k, v in per.items()))
    worst = np.unravel_index(np.argmax(qH.max(axis=2).max(axis=1)), (C.point.size,))[0]
    assert qH.max() <= 1.0 and qb.max() <= 1.0, (pts[C.point[worst]], C.orient[worst], diag[worst], _f(H[worst]), qH.max(), qb.max())
    want = np.abs(r0[C.point]).sum() + C.n_anchor * LD(float(rc.E_ANCHOR @ rc.OMEGA @ rc.E_ANCHOR))
    assert abs(LD(rc2) - want) <= b0[C.point].sum() + rr.EPS * (2 * C.n_anchor) * want


# ------------------------------------------------------------------ the solver paths
def _step(o, C):
    """optimize(1) from the cells' poses -> (poses, stats)"""
    o.set_poses(C.poses)
    d, st = o.optimize(1)
    assert d == 1, (d, o.last_error())
    return o.get_poses(), st


def _cell_ratio(C, P, dx, slack):
    """per cell: |pose - (start + dx)| over `slack` (n, 3), worst entry"""
    got = (P[C.free] - C.poses[C.free]).astype(LD)
    assert np.array_equal(P[C.fixed != 0].view(np.uint64), C.poses[C.fixed != 0].view(np.uint64))
    return (np.abs(got - dx) / slack).max(axis=1).astype(np.float64)


def _d_path(o_none, C, pts):
    dx, _ = rc.cell_steps(C, pts, np.ones(len(pts)))
    P, _ = _step(o_none, C)
    n = np.abs(dx).max(axis=1)[:, None]
    return max(1e-14, float(_cell_ratio(C, P, dx, n).max()))


def _solve_check(name, o, C, pts, d_path, r0, w, b0):
    dx, dw = rc.cell_steps(C, pts, w)
    P, st = _step(o, C)
    slack = 10.0 * d_path * np.abs(dx).max(axis=1)[:, None] + dw
    q = _cell_ratio(C, P, dx, slack)
    per = {}
    for k in range(C.point.size):
        nm = rr.NAMES[pts[C.point[k]].kind]
        per[nm] = max(per.get(nm, 0.0), float(q[k]))
    print(f"{name}: {C.point.size} cells, d_path {d_path:.3g}; worst ratio to the tolerance per kind " + ", ".join(f"{k} {v:.3g}" for k, v in per.items()))
    k = int(np.argmax(q))
    assert q.max() <= 1.0, (name, pts[C.point[k]], int(C.orient[k]), P[C.free[k]], _f(C.poses[C.free[k]] + dx[k]), q.max())
    want = np.abs(r0[C.point]).sum() + C.n_anchor * LD(float(rc.E_ANCHOR @ rc.OMEGA @ rc.E_ANCHOR))
    tol = b0[C.point].sum() + rr.EPS * (2 * C.n_anchor) * want
    print(f"{name}: robust_chi2[0] {st['robust_chi2'][0]!r} against {float(want)!r}, |diff| / tol {float(abs(LD(st['robust_chi2'][0]) - want) / tol):.3g}")
    assert abs(LD(st["robust_chi2"][0]) - want) <= tol
    return P, float(q.max())


@pytest.mark.parametrize("path", list(PATHS))
def test_one_iteration_on_every_path(path):
    pts, C, r0, w, b0, b1 = _ref("solve")
    with _open(rc.cells(pts, kerneled=False), path) as o_none:
        d_path = _d_path(o_none, C, pts)
    with _open(C, path) as o:
        P, worst = _solve_check(f"optimize(1), {path}", o, C, pts, d_path, r0, w, b0)
        desc = o.solver_description()
        if path == "mfront":
            # the LM instantiation of the edge kernel: a lambda below every diagonal entry's last bit is the undamped step
            o.set_poses(C.poses)
            rc_t, st_t = o.optimize_lm(1, 1e-300)
            assert rc_t == 1 and st_t["trials"] == [1] and st_t["lambda0"] == 1e-300, st_t
            assert np.array_equal(o.get_poses().view(np.uint64), P.view(np.uint64))
    assert desc.startswith(PATHS[path][1]), desc


def test_kinds_on_edges_appended_as_an_overlay():
    def grown(C):
        o = capi.Optimizer(0, direct_rows=0)
        o.set_graph(*_graph_args(C, C.n_anchor))
        assert o.optimize(1)[0] == 1
        o.update_graph(*_graph_args(C), C.n_anchor)
        assert "incremental overlay" in o.solver_description(), o.solver_description()
        o.set_robust_kernels(C.kedge, C.kind[C.kedge], C.delta[C.kedge])          # every kind, NONE and DCS too, on the appended ids
        assert "incremental overlay" in o.solver_description(), o.solver_description()
        return o

    # an overlay holds at most 64 touched resident rows (sgo_overlay.h: kOvMaxTouched): 32 points, two orientations, per context
    worst, n_cells = {}, 0
    for t0 in range(0, len(POINTS), 32):
        pts = POINTS[t0:t0 + 32]
        C = rc.cells(pts)
        r0, w, b0, b1 = rc.reference(pts)
        with grown(C) as o:
            rho0, wd = o.edge_robust()
            for k, v in _check_pairs(f"overlay, k_edge_robust, points {t0}..", pts, C, rho0, wd).items():
                worst[k] = max(worst.get(k, 0.0), v)
            plain, robust = o.chi2()
            want = np.abs(r0[C.point]).sum() + C.n_anchor * LD(float(rc.E_ANCHOR @ rc.OMEGA @ rc.E_ANCHOR))
            assert abs(LD(robust) - want) <= b0[C.point].sum() + rr.EPS * (2 * C.n_anchor) * want
        n_cells += C.point.size
    assert n_cells == 2 * len(POINTS) and set(worst) == set(rr.NAMES)
    d_path, ratio, n_cells = 0.0, 0.0, 0
    for t0 in range(0, len(SOLVE), 32):
        pts = SOLVE[t0:t0 + 32]
        C = rc.cells(pts)
        r0, w, b0, b1 = rc.reference(pts)
        with grown(rc.cells(pts, kerneled=False)) as o_none:
            d = _d_path(o_none, C, pts)
        with grown(C) as o:
            ratio = max(ratio, _solve_check(f"optimize(1), overlay (k_ov_lin), points {t0}..", o, C, pts, d, r0, w, b0)[1])
            assert "incremental overlay" in o.solver_description()
        d_path, n_cells = max(d_path, d), n_cells + C.point.size
    print(f"overlay: {n_cells} cells solved, d_path {d_path:.3g}, worst ratio to the tolerance {ratio:.3g}")
    assert n_cells == 2 * len(SOLVE)


# ------------------------------------------------------------------ leave-one-out and leave-group-out
def _edges_and_weights(pts, C, w):
    wall = np.ones(2 * C.n_anchor)
    wall[C.kedge] = _f(w[C.point])
    g = types.SimpleNamespace(fixed=C.fixed.astype(bool), ei=C.ei, ej=C.ej, meas=C.meas, info=C.info, phi=np.full(C.ei.size, -1.0))
    return g, wall


def test_leave_one_out_of_the_kerneled_edges():
    from test_gpu_edge_loo import _compare
    pts, C, r0, w, b0, b1 = _ref("solve")
    g, wall = _edges_and_weights(pts, C, w)
    zero = np.flatnonzero(wall[C.kedge] == 0.0)
    assert zero.size >= 6                                     # Tukey's and Saturated's cut-off sides, DCS with phi = 0, both orientations
    edges = np.r_[C.kedge, zero].astype(np.int32)             # (zero: the ANCHOR ids of the cells whose kerneled edge has weight 0)
    with _open(C, "mfront") as o:
        _, wd = o.edge_robust()
        F, d2, red, fail = _compare("cells", g, o, edges, w=wall, min_compared=0.0)
        assert o.solver_description().startswith("multifrontal_cholesky")
    nk = C.kedge.size
    assert np.abs(wd[C.kedge] - wall[C.kedge]).max() <= rr.C_BOUND * rr.EPS
    # a kerneled edge of weight 0 is not in H: redundancy 1 exactly, and d2 is the gate's own formula, finite
    assert np.all(red[:nk][zero] == 1.0) and np.isfinite(d2[:nk][zero]).all()
    # the anchor beside it is all that holds its pose: a bridge, which decides nothing
    assert np.all(np.abs(red[nk:]) < 1e-6) and np.isnan(d2[nk:]).all() and not fail[nk:].any()
    compared = F["redundancy"][:nk] >= 5e-3
    print(f"k_loo_edges: {int(compared.sum())} of {nk} kerneled edges compared, {zero.size} of weight 0 with their anchors as bridges")
    assert compared.sum() >= 0.8 * nk


def test_leave_group_out_of_the_kerneled_edges():
    pts, C, r0, w, b0, b1 = _ref("solve")
    g, wall = _edges_and_weights(pts, C, w)
    edges = C.kedge[: capi.JOINT_MAX_CANDIDATES].astype(np.int32)
    assert {pts[t].kind for t in C.point[: edges.size]} == set(range(10))
    S = lr.Edges(C.poses, g.fixed, g.ei, g.ej, g.meas, g.info, w=wall)
    T = eg.table(S, edges)
    M = np.eye(edges.size, dtype=np.uint8)
    with _open(C, "mfront") as o:
        _, wd = o.edge_robust()
        N, e, wj = o.edge_joint(edges)
        _, d2, dof, piv, fail = o.edge_groups(M, np.full(edges.size, eg.CHI2_99_DOF3))
    assert np.array_equal(wj.view(np.uint64), wd[edges].view(np.uint64))                    # sgo_edge_robust's weights
    assert np.abs(wj - T["w"]).max() <= rr.C_BOUND * rr.EPS and np.array_equal(e, T["e"])
    rn = np.abs(N - T["N"]).max() / np.abs(T["N"]).max()
    ref = [eg.closed_form(T["O"][[t]], T["N"][3 * t:3 * t + 3, 3 * t:3 * t + 3], T["e"][[t]], T["w"][[t]]) for t in range(edges.size)]
    d2r, pr = np.array([r["d2"] for r in ref]), np.array([r["pivot"] for r in ref])
    use = pr >= 10 * eg.MIN_PIVOT
    rd = float((np.abs(d2[use] - d2r[use]) / d2r[use]).max())
    rp = float(np.abs(piv[use] - pr[use]).max())
    print(f"egroup's edge kernel: {edges.size} kerneled edges, {int(use.sum())} single-edge groups compared; N {rn:.2e} of max |N_ref|, "
          f"d2 {rd:.2e} relative, pivot {rp:.2e} absolute")
    assert use.sum() >= 0.8 * edges.size and rn <= sr.DEVICE_BAR and rd <= sr.DEVICE_BAR and rp <= sr.DEVICE_BAR
    assert (dof == 3).all()
    zero = T["w"] == 0.0
    assert zero.sum() >= 3 and np.all(piv[zero] == 1.0)       # weight 0: I - T Nt T is the identity, the pivot 1 exactly
    decided = piv >= eg.MIN_PIVOT
    assert np.isnan(d2[~decided]).all() and not fail[~decided].any() and np.array_equal(fail, decided & (d2 > eg.CHI2_99_DOF3))
