"""GPU parity: every kernel of the HIP path, through the C-ABI, against the CPU oracle.

Floating point (fp64) path: tolerances are stated per check.  The oracle compiles with
-ffp-contract=off, the device code contracts to FMA, and the row sums run in a different
(tree) order, so agreement is to rounding, not bitwise.
"""
import numpy as np
import pytest

from sparse_gslam_amd import capi, synth

pytestmark = pytest.mark.gpu


def _oracle():
    from oracle import c_oracle
    return c_oracle


@pytest.fixture(scope="module")
def opt():
    o = capi.Optimizer(0, pcg_tol=1e-10, pcg_maxit=200000, direct_rows=0)   # the PCG path (tests/test_gpu_direct.py covers the other)
    yield o
    o.close()


@pytest.mark.parametrize("name,kw", [("C1", dict(info_mode="full")), ("C2", dict(info_mode="full")),
                                     ("C1", dict(init="odom"))])
def test_linearize_matches_oracle(opt, name, kw):
    g = synth.config(name, **kw)
    opt.set_graph(*g.arrays())
    b, diag, c2, rc2 = opt.linearize()
    ob, od, oc2, orc2 = _oracle().linearize(*g.arrays())
    assert b.shape == ob.shape
    # tolerance: 1e-12 relative to the largest entry (sums of ~10 terms of mixed sign)
    assert np.abs(b - ob).max() <= 1e-12 * np.abs(ob).max()
    assert np.abs(diag - od).max() <= 1e-12 * np.abs(od).max()
    assert abs(c2 - oc2) <= 1e-12 * oc2 and abs(rc2 - orc2) <= 1e-12 * orc2


def test_edge_chi2_matches_oracle(opt):
    g = synth.config("C1", info_mode="full")
    opt.set_graph(*g.arrays())
    e2 = opt.edge_chi2()
    _, _, _, oe2, _, _ = _oracle().edges(g.poses[g.ei], g.poses[g.ej], g.meas, g.info, g.phi)
    assert np.abs(e2 - oe2).max() <= 1e-11 * max(1.0, np.abs(oe2).max())


def test_spmv_matches_oracle(opt):
    g = synth.config("C2", info_mode="full")
    opt.set_graph(*g.arrays())
    opt.linearize()
    x = np.random.default_rng(0).standard_normal((opt.n_free, 3))
    y = opt.hessian_apply(x)
    oy = _oracle().hessian_apply(*g.arrays(), x).reshape(-1, 3)
    assert np.abs(y - oy).max() <= 1e-12 * np.abs(oy).max()


@pytest.mark.parametrize("kernel", ["tile", "group"])
def test_both_level0_kernels_match_the_oracle(kernel, monkeypatch):
    """Small graphs (< 150 k connected pairs) take the wave-group product kernel k_spmv0, large ones the tile kernel k_spmv0t:
    both forced on C2 (SGO_SPMV0), product, solve and five GN iterations against the oracle."""
    monkeypatch.setenv("SGO_SPMV0", kernel)
    g = synth.config("C2", info_mode="full")
    with capi.Optimizer(0, pcg_tol=1e-10, direct_rows=0, profile=1) as o:
        o.set_graph(*g.arrays())
        b, _, _, _ = o.linearize()
        x = np.random.default_rng(0).standard_normal((o.n_free, 3))
        y = o.hessian_apply(x)
        oy = _oracle().hessian_apply(*g.arrays(), x).reshape(-1, 3)
        assert np.abs(y - oy).max() <= 1e-12 * np.abs(oy).max()
        sol, it, relres = o.solve()
        assert np.linalg.norm(b - o.hessian_apply(sol)) <= 1e-8 * np.linalg.norm(b)
        done, st = o.optimize(5)
        prof = o.kernel_profile()
    used = {n for n, v in prof.items() if v["launches"] > 0}
    assert ("k_spmv0t<0, 1024, false>" in used) == (kernel == "tile") and ("k_spmv0<0>" in used) == (kernel == "group"), used
    oP, ost = _oracle().gauss_newton(*g.arrays(), iters=5)
    assert done == 5
    for a, c in zip(st["chi2"], ost["chi2"]):
        assert abs(a - c) <= 1e-6 * c


def test_pcg_solves_the_normal_equations(opt):
    g = synth.config("C1", info_mode="full")
    opt.set_graph(*g.arrays())
    b, _, _, _ = opt.linearize()
    x, it, relres = opt.solve()
    assert it > 0 and relres <= 1e-10
    r = b - opt.hessian_apply(x)
    assert np.linalg.norm(r) <= 1e-8 * np.linalg.norm(b)   # true residual, not the recurrence


@pytest.mark.parametrize("name", ["C1"])
def test_gauss_newton_matches_direct_oracle(opt, name):
    g = synth.config(name, info_mode="full")
    opt.set_graph(*g.arrays())
    done, st = opt.optimize(20)
    P = opt.get_poses()
    oP, ost = _oracle().gauss_newton(*g.arrays(), iters=20, solver="direct")
    assert done == 20 == ost["iters_done"]
    # BASELINE.json north_star: final chi2 within 1e-6 relative of the direct-solver reference
    for k in range(21):
        assert abs(st["chi2"][k] - ost["chi2"][k]) <= 1e-6 * ost["chi2"][k], k
        assert abs(st["robust_chi2"][k] - ost["robust_chi2"][k]) <= 1e-6 * ost["robust_chi2"][k], k
    assert np.abs(P - oP).max() <= 1e-5


# ------------------------------------------------------------------ AMG-preconditioned solver
@pytest.fixture(scope="module")
def opt_amg():
    o = capi.Optimizer(0, solver=capi.SOLVER_PCG_AMG, pcg_tol=1e-10, pcg_maxit=5000, direct_rows=0)
    yield o
    o.close()


def test_amg_preconditioner_is_positive_and_contracts(opt_amg):
    """Default: smoothed aggregation, V-cycle -- a fixed symmetric operator (checked below).  With
    SGO_AMG_KDEPTH > 0 the K-cycle's inner flexible CG makes it a variable preconditioner, for which
    <u, M v> == <M u, v> holds only approximately; the outer flexible PCG needs <u, M u> > 0 and
    M ~ H^-1 either way."""
    g = synth.config("C2", info_mode="full")
    opt_amg.set_graph(*g.arrays())
    b, _, _, _ = opt_amg.linearize()
    rng = np.random.default_rng(5)
    u = rng.standard_normal((opt_amg.n_free, 3))
    v = rng.standard_normal((opt_amg.n_free, 3))
    Mu, Mv = opt_amg.precondition(u), opt_amg.precondition(v)
    assert (u * Mu).sum() > 0 and (v * Mv).sum() > 0
    assert abs((u * Mv).sum() - (Mu * v).sum()) <= 0.1 * abs((u * Mv).sum())
    # one preconditioned step on the actual right-hand side reduces the M-norm of the residual
    x1 = opt_amg.precondition(b)
    r1 = b - opt_amg.hessian_apply(x1)
    assert (r1 * opt_amg.precondition(r1)).sum() < (b * x1).sum()


def test_smoothed_aggregation_v_cycle_is_a_symmetric_operator(opt_amg):
    """P = (I - w D^-1 A) T, Galerkin coarse operators, one damped block-Jacobi sweep before and after
    on every level, exact dense coarsest solve: M is symmetric positive definite and linear."""
    g = synth.config("C2", info_mode="full")
    opt_amg.set_graph(*g.arrays())
    opt_amg.linearize()
    rng = np.random.default_rng(7)
    u = rng.standard_normal((opt_amg.n_free, 3))
    v = rng.standard_normal((opt_amg.n_free, 3))
    Mu, Mv = opt_amg.precondition(u), opt_amg.precondition(v)
    assert abs((u * Mv).sum() - (Mu * v).sum()) <= 1e-9 * max(abs((u * Mv).sum()), np.linalg.norm(u) * np.linalg.norm(Mv) * 1e-3)
    assert np.abs(opt_amg.precondition(2.0 * u - 3.0 * v) - (2.0 * Mu - 3.0 * Mv)).max() <= 1e-9 * np.abs(Mu).max()
    assert (u * Mu).sum() > 0 and (v * Mv).sum() > 0


def test_tentative_and_smoothed_hierarchies_solve_the_same_system(monkeypatch):
    """SGO_AMG_SMOOTH=0 keeps the plain-aggregation K-cycle of the first milestone: same solution,
    more PCG iterations."""
    g = synth.config("C2", info_mode="full")
    res = {}
    for smooth in ("1", "0"):
        monkeypatch.setenv("SGO_AMG_SMOOTH", smooth)
        with capi.Optimizer(0, solver=capi.SOLVER_PCG_AMG, pcg_tol=1e-10, pcg_maxit=5000) as o:
            o.set_graph(*g.arrays())
            o.linearize()
            res[smooth] = o.solve()
    (x1, it1, rr1), (x0, it0, rr0) = res["1"], res["0"]
    assert rr1 <= 1e-10 and rr0 <= 1e-10
    assert np.abs(x1 - x0).max() <= 1e-7 * np.abs(x0).max()
    assert it1 < it0 < 400


def test_amg_pcg_solves_the_normal_equations(opt_amg):
    g = synth.config("C2", info_mode="full")
    opt_amg.set_graph(*g.arrays())
    b, _, _, _ = opt_amg.linearize()
    x, it, relres = opt_amg.solve()
    assert 0 < it < 400 and relres <= 1e-10
    r = b - opt_amg.hessian_apply(x)
    assert np.linalg.norm(r) <= 1e-8 * np.linalg.norm(b)


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_amg_gauss_newton_matches_direct_oracle(opt_amg, name):
    g = synth.config(name, info_mode="full")
    opt_amg.set_graph(*g.arrays())
    done, st = opt_amg.optimize(20)
    P = opt_amg.get_poses()
    oP, ost = _oracle().gauss_newton(*g.arrays(), iters=20, solver="direct")
    assert done == 20 == ost["iters_done"]
    for k in range(21):
        assert abs(st["chi2"][k] - ost["chi2"][k]) <= 1e-6 * ost["chi2"][k], k
        assert abs(st["robust_chi2"][k] - ost["robust_chi2"][k]) <= 1e-6 * ost["robust_chi2"][k], k
    assert np.abs(P - oP).max() <= 1e-5


def test_tolerance_rules_at_their_boundaries():
    """The two rules that set a solve's tolerance, checked where they switch.  (1) Chain-like graphs -- fewer than 4
    Hessian blocks per free pose -- solve to pcg_tol / 10.  (2) Inside one optimize() call later solves keep the first
    solve's ABSOLUTE accuracy, never looser than pcg_tol_cap relative; pcg_tol_cap = 0 and optimize(1) keep pcg_tol."""
    def relres(g, iters=6, **kw):
        with capi.Optimizer(0, direct_rows=0, **kw) as o:
            o.set_graph(*g.arrays())
            done, st = o.optimize(iters)
            assert done == iters and set(st["pcg_converged"]) == {1}
            return np.array(st["pcg_relres"])
    V = 2000
    chain = synth.manhattan(V, int(1.45 * V), seed=31, info_mode="full")     # 2E + n < 4n
    dense = synth.manhattan(V, int(1.55 * V), seed=31, info_mode="full")     # 2E + n > 4n
    assert 2 * chain.E + (V - 1) < 4 * (V - 1) < 2 * dense.E + (V - 1)
    assert relres(chain, pcg_tol_cap=0.0).max() <= 1e-9 and relres(dense, pcg_tol_cap=0.0).max() <= 1e-8
    assert relres(dense, pcg_tol_cap=0.0).max() > 1e-9            # the denser graph is NOT solved tighter than asked
    r = relres(dense, iters=12)                                    # default cap 1e-6
    assert r[0] <= 1e-8 and r.max() <= 1e-6 and r[-1] > 1e-8       # first solve as asked, later ones absolute, capped
    r = relres(dense, iters=12, pcg_tol_cap=1e-7)
    assert r.max() <= 1e-7
    with capi.Optimizer(0, direct_rows=0) as o:                    # one iteration per call: always the relative rule
        o.set_graph(*dense.arrays())
        for _ in range(6):
            done, st = o.optimize(1)
            assert done == 1 and st["pcg_relres"][0] <= 1e-8


def test_stale_aggregation_is_rebuilt_and_the_result_still_matches(capfd):
    """From a dead-reckoned start robust-kernel re-weighting moves the strong connections within a few iterations: the
    count-based rule redoes the aggregation inside optimize() (verbose line), and the iterates still match the direct
    oracle."""
    g = synth.manhattan(V=3000, E=4500, seed=1, p_random=0.3, info_mode="diag", phi=1.0, init="odom")
    with capi.Optimizer(0, direct_rows=0, verbose=1) as o:
        o.set_graph(*g.arrays())
        done, st = o.optimize(20)
        P = o.get_poses()
    err = capfd.readouterr().err
    assert "multigrid hierarchy rebuilt before iteration" in err or "hierarchy rebuilt" in err, err[-2000:]
    oP, ost = _oracle().gauss_newton(*g.arrays(), iters=20)
    assert done == 20 == ost["iters_done"] and set(st["pcg_converged"]) == {1}
    rel = np.abs(np.array(st["chi2"]) - np.array(ost["chi2"])) / np.array(ost["chi2"])
    assert rel.max() <= 1e-6, rel.max()
    assert max(st["pcg_iters"]) < 400        # no solve ground on with a stale hierarchy


# ------------------------------------------------------------------ multi-GPU logic on one GPU
def test_rank_partial_products_sum_to_the_single_rank_product():
    """Multi-GPU scheme on one GPU: each emulated rank evaluates the level-0 product for the rows of its tile
    range only (zeros elsewhere); every row has exactly one contributing rank, so the sum over ranks -- what
    ncclAllReduce computes in the all-reduce mode -- is the full product.  A world of G ranks cuts 256 G tiles (every
    rank keeps its own 256 CUs busy), so a row's blocks are summed in another order than in the one-rank cut:
    agreement with the single-rank product to rounding, not bitwise."""
    g = synth.config("C2", info_mode="full")
    x = np.random.default_rng(3).standard_normal((int((~g.fixed).sum()), 3))
    with capi.Optimizer(0, solver=capi.SOLVER_PCG_BJ) as full:
        full.set_graph(*g.arrays())
        full.linearize()
        fy = full.hessian_apply(x)
    for world in (2, 3, 8):
        sy = np.zeros_like(fy)
        owners = np.zeros(fy.shape[0], dtype=int)
        plan = capi.plan_rows(g.poses, g.fixed, g.ei, g.ej, world)
        for r in range(world):
            with capi.Optimizer(0, solver=capi.SOLVER_PCG_BJ) as o:
                o.debug_set_shard(world, r)
                o.set_graph(*g.arrays())
                o.linearize()
                y = o.hessian_apply(x)
            nz = np.any(y != 0.0, axis=1)
            assert 0 < nz.sum() < y.shape[0]            # really a partial
            # the rows this rank wrote are the rows the host-only plan assigns to it
            free = np.flatnonzero(~g.fixed)
            mine = np.isin(free, plan["row_vertex"][plan["rank_row_begin"][r]:plan["rank_row_begin"][r + 1]])
            assert not np.any(nz & ~mine)
            owners += nz
            sy += y
        assert np.abs(sy - fy).max() <= 1e-13 * np.abs(fy).max(), world
        assert owners.max() == 1


def test_rank_partial_coarse_right_hand_sides_sum_to_the_single_rank_one(monkeypatch):
    """The other exchange of the multi-GPU cycle: each rank restricts the residual of ITS rows only and the
    partial coarse right-hand sides are all-reduced (3 n_c doubles).  Emulated ranks on one GPU: the partials sum
    to the single-rank vector (to rounding: the per-column sums are split differently).  The single-rank context is given
    the tile kernel too (a graph of C2's size would take the wave-group kernel, whose residual pass reads the fp64 blocks
    where the tile kernel's reads their fp32 copy: the comparison is between partitions, not between kernels)."""
    monkeypatch.setenv("SGO_SPMV0", "tile")
    import ctypes as C
    L = capi.lib()
    L.sgo_debug_coarse_rhs.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
    g = synth.config("C2", info_mode="full")
    n = int((~g.fixed).sum())
    r = np.random.default_rng(4).standard_normal((n, 3))

    def coarse(o):
        out = np.zeros(3 * n)
        k = L.sgo_debug_coarse_rhs(o._h, r.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)), out.size)
        assert k > 0
        return out[:k].copy()

    with capi.Optimizer(0) as full:
        full.set_graph(*g.arrays())
        full.linearize()
        fc = coarse(full)
    for world in (2, 5):
        acc = np.zeros_like(fc)
        for rk in range(world):
            with capi.Optimizer(0) as o:
                o.debug_set_shard(world, rk)
                o.set_graph(*g.arrays())
                o.linearize()
                part = coarse(o)
            assert np.abs(part).max() > 0 and not np.allclose(part, fc)
            acc += part
        assert np.abs(acc - fc).max() <= 1e-12 * np.abs(fc).max(), world


def test_single_rank_rccl_communicator_runs_the_collective_path():
    """Exercises the RCCL binding with a 1-rank communicator: dlopen, ncclCommInitRank and a real
    ncclAllReduce after every level-0 product of the solve and on chi2 (the multi-GPU code path: sharded
    products, zero fill, all-reduce, dot products on the full vectors).  The PCG scalars are summed in another
    order than on the single-GPU path, so agreement is to rounding, not bitwise."""
    g = synth.config("C2", info_mode="full")
    with capi.Optimizer(0) as a:
        a.set_graph(*g.arrays())
        da, sa = a.optimize(5)
        Pa = a.get_poses()
    with capi.Optimizer(0) as b:
        b.comm_init(1, 0, capi.comm_unique_id())
        b.set_graph(*g.arrays())
        db, sb = b.optimize(5)
        Pb = b.get_poses()
    assert da == db == 5
    assert np.abs(Pa - Pb).max() <= 1e-7
    for ca, cb in zip(sa["chi2"], sb["chi2"]):
        assert abs(ca - cb) <= 1e-9 * ca
    assert max(abs(x - y) for x, y in zip(sa["pcg_iters"], sb["pcg_iters"])) <= 2


def test_rccl_collectives_captured_into_the_hipgraph_give_the_same_iterates(monkeypatch):
    """SGO_COMM_GRAPH=1: ncclAllReduce captured into the replayed PCG graph (1-rank communicator) -- the same kernels
    and collectives in the same order as the plain-launch collective path: identical results."""
    g = synth.config("C2", info_mode="full")
    res = []
    for flag in (None, "1"):
        if flag:
            monkeypatch.setenv("SGO_COMM_GRAPH", flag)
        with capi.Optimizer(0) as o:
            o.comm_init(1, 0, capi.comm_unique_id())
            o.set_graph(*g.arrays())
            d, st = o.optimize(5)
            res.append((d, st["chi2"], st["pcg_iters"], o.get_poses()))
    assert res[0][0] == res[1][0] == 5
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert np.array_equal(res[0][3], res[1][3])


# ------------------------------------------------------------------ execution modes agree
def test_graph_replay_plain_launches_and_profile_mode_agree_bitwise():
    """hipGraph replay, plain stream launches and the event-bracketed profile mode run the same
    kernels in the same order: identical poses, chi2 history and PCG iteration counts."""
    g = synth.config("C2", info_mode="full")
    res = []
    for kw in (dict(use_graph=1), dict(use_graph=0), dict(profile=1)):
        with capi.Optimizer(0, **kw) as o:
            o.set_graph(*g.arrays())
            done, st = o.optimize(6)
            res.append((done, st["chi2"], st["pcg_iters"], o.get_poses()))
            if kw.get("profile"):
                prof = o.kernel_profile()
                # 6 GN iterations + the linearisation of the multigrid set-up
                # (the level-0 launches of the block-stream kernels are kept in slots of their own)
                assert prof["k_linearize"]["launches"] in (6, 7) and prof["k_spmv0<0>"]["ms"] > 0
                assert 0 <= o.profile_overhead_ms() < 0.1
    for r in res[1:]:
        assert r[0] == res[0][0] == 6 and r[1] == res[0][1] and r[2] == res[0][2]
        assert np.array_equal(r[3], res[0][3])


def test_both_solvers_reach_the_same_solution(opt, opt_amg):
    g = synth.config("C1", info_mode="full")
    xs = []
    for o in (opt, opt_amg):
        o.set_graph(*g.arrays())
        o.linearize()
        x, it, relres = o.solve()
        assert it > 0 and relres <= 1e-10
        xs.append(x)
    assert np.abs(xs[0] - xs[1]).max() <= 1e-7 * np.abs(xs[0]).max()
