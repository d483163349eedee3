"""The level-0 entry points and the exact preconditioners against a reference that never forms H (tests/kernel_reference.py).

sgo_linearize (b, diagonal blocks, chi2, robust chi2), sgo_edge_chi2, sgo_chi2 and sgo_hessian_apply on three vectors -- two
random ones and one whose rows are scaled by 10^+-6, so that a per-entry bound means something -- are checked entry by entry
against the reference's bound C U abs (the module docstring there).  Each case also asserts the shape it is there for: the
tile count and kind of cut of the level-0 plan (capi.plan_rows, the plan sgo_set_graph_se2 makes), which level-0 kernel ran
(kernel profile), rows longer than 64 slots, the fraction of pairs that straddle tiles.  Kinds of cut (sgo_plan.cpp,
plan_rows_tiles): "group" no tiles (the wave-group kernel k_spmv0), "block" the block-balanced cut (at most one tile per CU),
"lds" many tiles closed by the LDS budget (at least 4 per CU, uneven slot counts), "slot" the fallback cut by slot count
(tiles of nearly equal slot counts, at most 4096 rows).

Block-Jacobi (z = D^-1 r) and the single-level hierarchy of graphs of at most 400 free poses (z = H^-1 r, the Gauss-Jordan
inverse) are checked against closed forms.  A failing check reports every ratio error / bound of its case.
"""
import numpy as np
import pytest

import kernel_reference as kr
from sparse_gslam_amd import capi, synth

pytestmark = pytest.mark.gpu
C_BJ = 1.0
C_DENSE = 0.5
TILE_KERNEL = "k_spmv0t"
GROUP_KERNEL = "k_spmv0<"


def _vectors(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, 3)), rng.uniform(-1.0, 1.0, (n, 3)),
            rng.standard_normal((n, 3)) * 10.0 ** rng.choice([-6.0, 6.0], size=(n, 1))]


def _plan(g, poses=None, meas=True):
    """Tile count, kind of cut, largest row (slots), fraction of free-free pairs in two tiles, of the plan of g."""
    P = g.poses if poses is None else poses
    p = capi.plan_rows(P, g.fixed, g.ei, g.ej, meas=g.meas if meas else None)
    tb, rv, n = p["tile_row_begin"], p["row_vertex"], p["n"]
    deg = np.bincount(np.r_[g.ei, g.ej], minlength=g.V) + 1       # slots of a row: its edges + the diagonal
    out = dict(tiles=len(tb) - 1, max_row_slots=int(deg[rv].max()), row_vertex=rv)
    if out["tiles"] == 0:
        return dict(out, kind="group", straddle=0.0)
    cs = np.r_[0, np.cumsum(deg[rv])]
    slots = (cs[tb[1:]] - cs[tb[:-1]])[:-1]
    rows = np.diff(tb)
    row = np.full(g.V, -1)
    row[rv] = np.arange(n)
    ri, rj = row[g.ei], row[g.ej]
    both = (ri >= 0) & (rj >= 0)
    ti = np.searchsorted(tb, ri[both], side="right") - 1
    tj = np.searchsorted(tb, rj[both], side="right") - 1
    K = out["tiles"]
    spread = (slots.max() - slots.min()) / np.median(slots) if slots.size else 0.0
    if K <= 256:
        kind = "block"
    elif spread <= 0.35 and rows.max() <= 4096:
        kind = "slot"
    elif K >= 1024:
        kind = "lds"
    else:
        kind = "other"
    return dict(out, kind=kind, straddle=float((ti != tj).mean()), spread=float(spread))


def _kernels(opt):
    return {k for k, v in opt.kernel_profile().items() if v["launches"] > 0}


def check_level0(case, opt, g, poses=None, seed=0, values=None):
    """Every level-0 entry point of `opt` (graph g, current poses) against the reference; values: (b, diag, chi2, robust, hx)
    to compare instead of the reference's own (C5: the C++ oracle's), the bounds are the reference's either way."""
    P = opt.get_poses() if poses is None else poses
    arr = (P,) + tuple(g.arrays()[1:])
    assert np.array_equal(opt.free_ids(), np.flatnonzero(~g.fixed))
    b, diag, c2, rc2 = opt.linearize()
    e2 = opt.edge_chi2()
    sc2, src2 = opt.chi2()
    xs = _vectors(opt.n_free, seed)
    ys = [opt.hessian_apply(x) for x in xs]
    ref = kr.reference(*arr, xs=xs)
    r = kr.ratios(ref, b=b, diag=diag, chi2=c2, robust=rc2, e2=e2, hx=ys)
    s = kr.ratios(ref, chi2=sc2, robust=src2)
    r["sgo_chi2"], r["sgo_robust_chi2"] = s["chi2"], s["robust_chi2"]
    if values is not None:
        ob, od, oc2, orc2, oys = values(arr, xs)
        ref.b, ref.diag, ref.chi2, ref.robust, ref.hx = ob, od, oc2, orc2, oys
        for k, v in kr.ratios(ref, b=b, diag=diag, chi2=c2, robust=rc2, hx=ys).items():
            r["vs_oracle_" + k] = v
    bad = kr.failures(r)
    if bad and values is None:   # where the worst entry of each failing output is, and the row's edges
        got = dict(b=b, diag=diag, edge_chi2=e2, hx0=ys[0], hx1=ys[1], hx2=ys[2])
        want = dict(b=(ref.b, ref.b_abs), diag=(ref.diag, ref.diag_abs), edge_chi2=(ref.e2, ref.e2_abs),
                    **{f"hx{q}": (ref.hx[q], ref.hx_abs[q]) for q in range(3)})
        for k in set(bad) & set(got):
            G = np.asarray(got[k]).reshape(want[k][0].shape)
            err = np.abs(G - want[k][0]).astype(np.float64) / (kr.U * want[k][1])
            at = np.unravel_index(int(np.nanargmax(err)), err.shape)
            v = int(ref.free[at[0]]) if k != "edge_chi2" else int(g.ei[at[0]])
            inc = np.flatnonzero((g.ei == v) | (g.ej == v))
            r["worst_" + k] = dict(at=[int(q) for q in at], got=float(G[at]), ref=float(want[k][0][at]), abs=float(want[k][1][at]),
                                   edges=inc.tolist(), phi=g.phi[inc].tolist(), e2=ref.e2[inc].astype(np.float64).tolist())
    assert not bad, (case, r)
    return ref


# ------------------------------------------------------------------ small graphs: the wave-group kernel
def _c1_boundary():
    """C1 with closures whose phi is set so that e2 lies just below, at and just above it (the DCS scale leaves 1 there)."""
    g = synth.config("C1", info_mode="full")
    e2 = kr.reference(*g.arrays()).e2.astype(np.float64)
    close = np.flatnonzero(g.phi >= 0)
    phi = g.phi.copy()
    for k, f in zip(range(30), (1.0 - 1e-9, 1.0, 1.0 + 1e-9) * 10):
        phi[close[k]] = e2[close[k]] * f
    return synth.Graph(g.poses, g.fixed, g.ei, g.ej, g.meas, g.info, phi)


def _c1_no_kernel():
    g = synth.config("C1", info_mode="full")
    return synth.Graph(g.poses, g.fixed, g.ei, g.ej, g.meas, g.info, np.full(g.E, -1.0))


SMALL = {
    "C1_diag": lambda: synth.config("C1"),
    "C1_full": lambda: synth.config("C1", info_mode="full"),
    "C1_no_robust_kernel": _c1_no_kernel,
    "C1_phi_boundary": _c1_boundary,
}


@pytest.mark.parametrize("case", list(SMALL))
def test_small_graphs_wave_group_kernel(case):
    g = SMALL[case]()
    pl = _plan(g)
    assert pl["kind"] == "group", pl["kind"]
    with capi.Optimizer(0, direct_rows=0, profile=1) as o:
        o.set_graph(*g.arrays())
        check_level0(case, o, g)
        assert any(k.startswith(GROUP_KERNEL) for k in _kernels(o))


@pytest.mark.parametrize("kernel", ["group", "tile"])
def test_c2_both_level0_kernels(kernel, monkeypatch):
    if kernel == "tile":
        monkeypatch.setenv("SGO_SPMV0", "tile")
    g = synth.config("C2", info_mode="full")
    pl = _plan(g)
    assert pl["kind"] == ("block" if kernel == "tile" else "group"), pl
    if kernel == "tile":
        assert 50 <= pl["tiles"] <= 256 and pl["straddle"] > 0.01, pl
    with capi.Optimizer(0, direct_rows=0, profile=1) as o:
        o.set_graph(*g.arrays())
        check_level0(f"C2_{kernel}", o, g)
        used = _kernels(o)
    assert any(k.startswith(TILE_KERNEL if kernel == "tile" else GROUP_KERNEL) for k in used), used


# ------------------------------------------------------------------ the tile kernel's cuts
@pytest.mark.parametrize("lds,kind", [(6000, "lds"), (20000, "slot")])
def test_tile_cuts_on_a_cheap_graph(lds, kind, monkeypatch):
    """30 k poses / 250 k edges (above the wave-group threshold: the tile kernel by default).  SGO_TILE_LDS=6000: the LDS
    closes tiles early, about 1300 uneven tiles are taken as cut; 20000: the block-balanced cut makes more tiles than CUs
    without reaching 4 per CU, and the fallback cut by slot count takes over (tiles of nearly equal slot counts)."""
    monkeypatch.setenv("SGO_TILE_LDS", str(lds))
    g = synth.manhattan(30000, 250000, seed=8, p_random=0.2)
    pl = _plan(g)
    assert pl["kind"] == kind and pl["tiles"] >= 1000 and pl["straddle"] > 0.2, pl
    with capi.Optimizer(0, profile=1) as o:
        o.set_graph(*g.arrays())
        check_level0(f"manhattan30k_tile_lds{lds}_{kind}", o, g)
        assert any(k.startswith(TILE_KERNEL) for k in _kernels(o))


LARGE = {
    "C4": (lambda: synth.config("C4"), "block"),
    "C4_odom": (lambda: synth.config("C4", init="odom"), "block"),
    "C4r": (lambda: synth.config("C4r"), "block"),
}


@pytest.mark.parametrize("case", list(LARGE))
def test_large_graphs_at_the_start_and_at_the_gpus_own_poses(case):
    make, kind = LARGE[case]
    g = make()
    pl = _plan(g)
    assert pl["tiles"] > 0 and pl["kind"] == kind, pl
    if case == "C4_odom":   # rows ordered by spanning-tree positions, not by the (dead-reckoned) poses
        assert not np.array_equal(pl["row_vertex"], _plan(g, meas=False)["row_vertex"])
    if case == "C4r":       # random closures: long halo lists
        assert pl["straddle"] > 0.05, pl
    with capi.Optimizer(0, profile=1) as o:
        o.set_graph(*g.arrays())
        check_level0(f"{case}_start[{pl['kind']} {pl['tiles']} tiles, straddle {pl['straddle']:.3f}]", o, g)
        assert any(k.startswith(TILE_KERNEL) for k in _kernels(o))
        done, st = o.optimize(3)
        assert done == 3
        check_level0(f"{case}_after_optimize3", o, g, seed=1)


# ------------------------------------------------------------------ structural cases, under both kernels
def _base(V=3000, E=6000, seed=11):
    return synth.manhattan(V, E, seed=seed, info_mode="full")


def _with_edges(g, a, b, rng, fixed=None, poses=None):
    """g plus edges (a[k], b[k]) whose measurements are the current relative poses with noise."""
    P = g.poses if poses is None else poses
    a, b = np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32)
    ci, si = np.cos(P[a, 2]), np.sin(P[a, 2])
    dx, dy = P[b, 0] - P[a, 0], P[b, 1] - P[a, 1]
    m = np.stack([ci * dx + si * dy, -si * dx + ci * dy, P[b, 2] - P[a, 2]], axis=1) + rng.normal(0, 0.05, (a.size, 3))
    m[:, 2] = synth._wrap(m[:, 2])
    info = np.tile(np.array([400.0, 5.0, 1.0, 300.0, -2.0, 2500.0]), (a.size, 1))
    return synth.Graph(P, g.fixed if fixed is None else fixed, np.r_[g.ei, a], np.r_[g.ej, b], np.r_[g.meas, m],
                       np.r_[g.info, info], np.r_[g.phi, np.full(a.size, 1.0)])


def _hubs():
    g = _base()
    rng = np.random.default_rng(1)
    a, b = [], []
    for hub, k in ((500, 65), (1500, 130), (2500, 1000)):
        others = rng.choice(np.setdiff1d(np.arange(g.V), [hub]), size=k, replace=False)
        a += [hub] * k
        b += list(others)
    return _with_edges(g, a, b, rng)


def _duplicates():
    g = _base()
    rng = np.random.default_rng(2)
    pick = rng.choice(g.E, size=300, replace=False)
    rep = np.repeat(pick, rng.integers(1, 4, size=pick.size))
    return _with_edges(g, g.ei[rep], g.ej[rep], rng)


def _fixed():
    g = _base()
    fixed = g.fixed.copy()
    fixed[::37] = True
    both = np.flatnonzero(fixed)
    rng = np.random.default_rng(3)
    a = both[:-1][:40]
    b = both[1:][:40]
    g2 = _with_edges(g, a, b, rng, fixed=fixed)
    assert np.any(fixed[g2.ei] & fixed[g2.ej]) and np.any(fixed[g2.ei] ^ fixed[g2.ej])
    return g2


def _near_pi():
    g = _base()
    P = g.poses.copy()
    rng = np.random.default_rng(4)
    k = rng.choice(g.V, size=g.V // 3, replace=False)
    P[k, 2] = np.where(rng.random(k.size) < 0.5, np.pi - rng.uniform(0, 1e-9, k.size), -np.pi + rng.uniform(0, 1e-9, k.size))
    return synth.Graph(P, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi)


STRUCT = {"hubs_65_130_1000": _hubs, "duplicate_edges": _duplicates, "fixed_free_and_fixed_fixed": _fixed,
          "theta_near_pi": _near_pi}


@pytest.mark.parametrize("kernel", ["group", "tile"])
@pytest.mark.parametrize("case", list(STRUCT))
def test_structural_cases_under_both_kernels(case, kernel, monkeypatch):
    if kernel == "tile":
        monkeypatch.setenv("SGO_SPMV0", "tile")
    g = STRUCT[case]()
    pl = _plan(g)
    assert pl["kind"] == ("block" if kernel == "tile" else "group"), pl
    if case.startswith("hubs"):
        assert pl["max_row_slots"] > 1000, pl
    with capi.Optimizer(0, direct_rows=0, profile=1) as o:
        o.set_graph(*g.arrays())
        check_level0(f"{case}_{kernel}", o, g)
        used = _kernels(o)
    assert any(k.startswith(TILE_KERNEL if kernel == "tile" else GROUP_KERNEL) for k in used), used


def test_direct_path_graph_after_optimize():
    """A graph on the factorisation path (default direct_rows): its level-0 plan is made lazily by the first single-step entry
    point, from the poses current at that moment."""
    g = synth.manhattan(3000, 4200, seed=9, info_mode="full", phi=0.75)
    with capi.Optimizer(0, profile=1) as o:
        o.set_graph(*g.arrays())
        desc = o.solver_description()
        assert desc.startswith(("multifrontal_cholesky", "direct_ldlt")), desc
        done, st = o.optimize(3)
        assert done == 3
        P = o.get_poses()
        assert _plan(g, poses=P, meas=False)["kind"] == "group"
        check_level0("direct_path_after_optimize3", o, g, poses=P)


# ------------------------------------------------------------------ C5 at full size
@pytest.fixture(scope="module")
def c5():
    return synth.config("C5")


def test_c5_full_size(c5):
    """1 M poses / 10 M edges, cut into about 1 800 LDS-limited tiles: at the start, every entry point against the chunked
    reference's values and against the C++ oracle's (fp64, OpenMP), both within the reference's bounds; chi2 and robust chi2
    at the GPU's own poses after optimize(20) against both."""
    from oracle import c_oracle
    g = c5
    pl = _plan(g)
    assert pl["kind"] == "lds" and pl["tiles"] >= 1024, pl

    def oracle_values(arr, xs):
        ob, od, oc2, orc2 = c_oracle.linearize(*arr)
        return ob, od, oc2, orc2, [c_oracle.hessian_apply(*arr, x).reshape(-1, 3) for x in xs]

    with capi.Optimizer(0, profile=1) as o:
        o.set_graph(*g.arrays())
        check_level0(f"C5_start[{pl['kind']} {pl['tiles']} tiles, straddle {pl['straddle']:.3f}]", o, g, values=oracle_values)
        assert any(k.startswith(TILE_KERNEL) for k in _kernels(o))
        done, st = o.optimize(20)
        assert done == 20
        P = o.get_poses()
        c2, rc2 = o.chi2()
    oc2, orc2 = c_oracle.chi2(P, *g.arrays()[1:])
    ref = kr.reference(P, *g.arrays()[1:])
    r = kr.ratios(ref, chi2=c2, robust=rc2)
    r.update({"oracle_" + k: v for k, v in kr.ratios(ref, chi2=oc2, robust=orc2).items()})
    r["gpu_vs_oracle_chi2"] = abs(c2 - oc2) / (kr.U * ref.chi2_abs)
    r["gpu_vs_oracle_robust_chi2"] = abs(rc2 - orc2) / (kr.U * ref.robust_abs)
    r["gpu_stats_chi2_end"] = abs(st["chi2"][-1] - oc2) / (kr.U * ref.chi2_abs)
    assert not kr.failures(r), r


# ------------------------------------------------------------------ exact preconditioners
BJ = {"C2": lambda: synth.config("C2", info_mode="full"), "C4": lambda: synth.config("C4"), "hubs": _hubs}


@pytest.mark.parametrize("case", list(BJ))
def test_block_jacobi_is_the_inverse_of_the_diagonal_blocks(case):
    """z = D^-1 r with D the reference's diagonal blocks: per block |z - D^-1 r|_2 <= C_BJ U kappa_abs(D) |D^-1 r|_2, kappa_abs =
    |D^-1|_2 |abs(D)|_2 (the blocks' own rounding is a multiple of U abs(D)).  C_BJ = 1: the worst measured ratio is 0.28."""
    g = BJ[case]()
    with capi.Optimizer(0, solver=capi.SOLVER_PCG_BJ, direct_rows=0) as o:
        o.set_graph(*g.arrays())
        o.linearize()
        rng = np.random.default_rng(6)
        rs = [rng.standard_normal((o.n_free, 3)), rng.standard_normal((o.n_free, 3)) * 10.0 ** rng.choice([-6.0, 6.0], size=(o.n_free, 1))]
        zs = [o.precondition(r) for r in rs]
    ref = kr.reference(*g.arrays())
    D = ref.diag.astype(np.float64)
    Dinv = np.linalg.inv(D)
    kappa = np.linalg.norm(Dinv, 2, axis=(1, 2)) * np.linalg.norm(ref.diag_abs, 2, axis=(1, 2))
    worst = 0.0
    for r, z in zip(rs, zs):
        zr = np.einsum("nij,nj->ni", Dinv, r)
        worst = max(worst, float((np.linalg.norm(z - zr, axis=1) / (kr.U * kappa * np.linalg.norm(zr, axis=1))).max()))
    assert worst <= C_BJ, worst


def _dense_graph(n, dup_fixed=False):
    if not dup_fixed:
        g = synth.manhattan(n + 1, max(n, int(1.6 * n)), seed=100 + n, info_mode="full")
        assert int((~g.fixed).sum()) == n
        return g
    g = synth.manhattan(n + 20, int(1.6 * n), seed=7, info_mode="full")
    fixed = g.fixed.copy()
    fixed[np.arange(5, g.V, g.V // 19)[:19]] = True
    rng = np.random.default_rng(8)
    rep = rng.choice(g.E, size=40, replace=False)
    g2 = _with_edges(g, g.ei[rep], g.ej[rep], rng, fixed=fixed)
    assert int((~g2.fixed).sum()) == n and np.any(g2.fixed[g2.ei] & ~g2.fixed[g2.ej])
    return g2


DENSE = [(1, False), (2, False), (20, False), (25, False), (350, False), (352, False), (360, False), (384, False),
         (400, False), (200, True)]


@pytest.mark.parametrize("n,dup_fixed", DENSE)
def test_single_level_hierarchy_is_the_exact_inverse(n, dup_fixed):
    """Graphs of at most 400 free poses have a one-level hierarchy: z = H^-1 r through the Gauss-Jordan inverse on the matrix
    cores (k_dense_fill, k_gj_pivot, k_gj_step, k_dense_apply).  N = 3n covers: multiples of 32 with an odd and an even block
    count (352, 384: the parity picks the result buffer), other N of both parities (350: 33 blocks, 360: 34), N < 64 and
    N > 64 (20, 25: the first stride of k_dense_apply), the smallest (1, 2) and the largest (400), duplicate edges and fixed
    endpoints (the accumulating k_dense_fill).  Checked per column in the 2-norm: |z - H^-1 r| <= C_DENSE N U kappa_2(H) |H^-1 r|,
    with H and the reference inverse (fp64 solve, two steps of refinement, residuals in long double) from the reference.
    C_DENSE = 0.5: the worst measured ratio is 0.11 (n = 1); at n >= 350, kappa_2 ~ 1e7-1e8, the measured errors are 1e-6 of
    the bound (this normwise bound is the worst case).  An exact preconditioner makes the PCG converge in one iteration: every
    one of these graphs does (pcg_tol 1e-8)."""
    g = _dense_graph(n, dup_fixed)
    N = 3 * n
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*g.arrays())
        desc = o.solver_description()
        assert f"L0 n={n} " in desc and "L1 " not in desc and f"coarsest dense N={N};" in desc, desc
        o.linearize()
        rng = np.random.default_rng(n)
        R = rng.standard_normal((N, 16))
        Z = np.stack([o.precondition(R[:, k].reshape(n, 3)).ravel() for k in range(R.shape[1])], axis=1)
        x, it, relres = o.solve()
    eye = np.eye(N)
    ref = kr.reference(*g.arrays(), xs=[eye[:, k].reshape(n, 3) for k in range(N)])
    H = np.stack([h.reshape(-1) for h in ref.hx], axis=1)          # longdouble, column k = H e_k
    H64 = H.astype(np.float64)
    Zr = np.linalg.solve(H64, R)
    for _ in range(2):
        res = R.astype(kr.LD) - H @ Zr.astype(kr.LD)
        Zr = Zr + np.linalg.solve(H64, res.astype(np.float64))
    kappa = np.linalg.cond(H64, 2)
    worst = float((np.linalg.norm(Z - Zr, axis=0) / (N * kr.U * kappa * np.linalg.norm(Zr, axis=0))).max())
    assert worst <= C_DENSE, (worst, kappa)
    assert it == 1 and relres <= 1e-8, (it, relres)
