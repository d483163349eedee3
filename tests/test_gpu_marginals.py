"""Marginal covariances of selected poses through the resident solver (sgo_marginals / sgo_solve_rhs; kernels in
sparse_gslam_amd/csrc/sgo_marginals.hip, driver in sgo_marginals.cpp), and SparseOptimizer::computeMarginals of the compat headers.

Reference: tests/marginals_reference.py -- SuperLU solves of unit columns of the robustified Hessian of oracle.np_oracle.  The
shapes are the smallest that reach each solver path (test_gpu_edge_gate.py, test_gpu_robust_kernels.py), corrupted as there, at
the oracle's 8-iteration poses.

Bar: |Sigma - Sigma_ref|_max <= 1e-6 x the block's natural scale sqrt(max |Sigma_ii| max |Sigma_jj|) -- the project's relative bar
for solver-dependent quantities; block-Jacobi PCG at 1e-8 on the CPU oracle agrees with SuperLU to 6e-10 on that scale.  A condition
on the input, not a tolerance: every reference column has |H x - e|_inf <= 1e-9, asserted on the reference alone.  Every test
prints its measured worst ratio."""
import functools
import os
import subprocess

import numpy as np
import pytest

import marginals_reference as mr
from sparse_gslam_amd import capi
from test_gpu_edge_gate import GATE, PCG, _case, _grow, _overlay_session, _same, _state
from test_gpu_robust_kernels import DIRECT, MFRONT, _mixed
from test_shim_replay import _write_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-6
PATHS = [(PCG, dict(direct_rows=0), "pcg_amg"), (MFRONT, {}, "multifrontal_cholesky"), (DIRECT, {}, "direct_ldlt")]


@functools.lru_cache(maxsize=None)
def _reference(shape, variant="dcs"):
    """graph, poses, the reference of H^-1 there; variant: dcs (what phi says) | mixed (_mixed's kinds) | gated (mixed, the gate's
    edges with zero information)"""
    g, _, P1, _, ogate = _case(*shape)
    assert g.fixed[0] and not g.fixed[1:].any()
    kind, delta = (None, None) if variant == "dcs" else _mixed(g)
    info = g.info.copy()
    if variant == "gated":
        info[ogate] = 0.0
    return g, P1, mr.Reference(mr.hessian(P1, g.fixed, g.ei, g.ej, g.meas, info, g.phi, kind, delta), g.fixed)


def _check(cov, ref, vi, vj, what):
    worst = mr.worst_ratio(cov, ref, vi, vj)
    print(f"{what}: worst |Sigma - Sigma_ref| / natural scale = {worst:.3e}; worst reference column residual = {ref.worst_residual:.3e}")
    assert ref.worst_residual <= 1e-9     # (the input condition, on the reference alone)
    assert worst <= BAR
    return worst


def test_blocks_match_the_reference_on_the_pcg_path():
    g, P1, ref = _reference(PCG)
    V = g.V
    m, l = V // 2, V - 1
    vi = [1, m, l, l, m, 0, l]
    vj = [1, m, l, m, l, m, m]       # (the last pair is the fourth again; (0, m): vertex 0 is fixed)
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(*g.arrays())
        assert opt.solver_description().startswith("pcg_amg")
        opt.set_poses(P1)
        cov = opt.marginals(vi, vj)
        solves = opt.last_marginal_solves
    assert solves == 3 * 3           # distinct free column vertices: 1, m, l
    _check(cov, ref, vi, vj, "pcg")
    assert np.array_equal(cov[5], np.zeros((3, 3)))
    assert np.array_equal(cov[3].view(np.uint64), cov[6].view(np.uint64))
    for t in range(3):
        assert np.array_equal(cov[t], cov[t].T) and np.all(np.linalg.eigvalsh(cov[t]) > 0), cov[t]
    # reference-free: Sigma_ij and Sigma_ji^T come from different solves
    mirror = np.abs(cov[3] - cov[4].T).max() / ref.scale(l, m)
    print(f"|Sigma_lm - Sigma_ml^T| / natural scale = {mirror:.3e}")
    assert mirror <= 1e-8


def test_weights_and_gating_are_in_the_hessian():
    g, P1, ref = _reference(PCG, "mixed")
    _, _, gref = _reference(PCG, "gated")
    ogate = _case(*PCG)[4]
    kind, delta = _mixed(g)
    V = g.V
    m, l = V // 2, V - 1
    vi, vj = [l, m, l], [l, m, m]
    # on the reference first: the gate shows in the last pose's block
    change = np.abs(gref.block(l, l) - ref.block(l, l)).max() / np.abs(ref.block(l, l)).max()
    assert change > 1e-3, change
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P1)
        opt.set_robust_kernels(np.arange(g.E), kind, delta)
        cov = opt.marginals(vi, vj)
        k, gated = opt.gate_edges(None, GATE)
        assert np.array_equal(gated, ogate) and k == int(ogate.sum())
        gcov = opt.marginals(vi, vj)
    _check(cov, ref, vi, vj, "mixed kinds")
    _check(gcov, gref, vi, vj, "mixed kinds, gated")
    assert np.abs(gcov[0] - cov[0]).max() / np.abs(cov[0]).max() > 1e-3


@pytest.mark.parametrize("shape,opts,path", PATHS[1:], ids=["mfront", "direct"])
def test_factorisation_paths_keep_their_path_and_their_bits(shape, opts, path):
    g, P1, ref = _reference(shape)
    V = g.V
    m, l = V // 2, V - 1
    vi, vj = [1, m, l, l, 0], [1, m, l, m, l]
    with capi.Optimizer(0, **opts) as opt, capi.Optimizer(0, **opts) as fresh:
        opt.set_graph(*g.arrays())
        opt.set_poses(P1)
        before = opt.solver_description()
        cov = opt.marginals(vi, vj)
        solves = opt.last_marginal_solves
        after = opt.solver_description()
        d, st = opt.optimize(6)
        fresh.set_graph(*g.arrays())
        fresh.set_poses(P1)
        df, sf = fresh.optimize(6)
        same_poses = np.array_equal(opt.get_poses().view(np.uint64), fresh.get_poses().view(np.uint64))
    # (the lazily built PCG structures add their own clause to the text; the path sgo_optimize_gn takes is named first)
    assert before.split(":")[0] == after.split(":")[0] == path, (before, after)
    assert solves == 9
    _check(cov, ref, vi, vj, path)
    assert np.array_equal(cov[4], np.zeros((3, 3)))
    assert d == df == 6
    assert st["chi2"] == sf["chi2"] and st["robust_chi2"] == sf["robust_chi2"]
    assert same_poses


def test_solve_rhs_is_solve_with_the_callers_right_hand_side():
    g, P1, ref = _reference(PCG)
    l = g.V - 1
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P1)
        with pytest.raises(capi.SgoError, match="sgo_linearize first"):
            opt.solve_rhs(np.zeros((opt.n_free, 3)))
        b = opt.linearize()[0]
        x0, it0, rr0 = opt.solve()
        x1, it1, rr1 = opt.solve_rhs(b)
        assert it1 == it0 and rr1 == rr0 and np.array_equal(x1.view(np.uint64), x0.view(np.uint64))
        h = int(np.flatnonzero(opt.free_ids() == l)[0])
        e = np.zeros((opt.n_free, 3))
        e[h, 0] = 1.0
        col, _, _ = opt.solve_rhs(e)
        x2, it2, _ = opt.solve()
        assert it2 == it0 and np.array_equal(x2.view(np.uint64), x0.view(np.uint64))
        bad = b.copy()
        bad[7, 1] = np.nan
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.solve_rhs(bad)
        assert capi.lib().sgo_solve_rhs(opt._h, None, None, None) == -2
        opt.marginals([l], [l])
        x3, it3, _ = opt.solve()
        assert it3 == it0 and np.array_equal(x3.view(np.uint64), x0.view(np.uint64))
    want = ref.column(l)[:, 0]
    err = np.abs(col.reshape(-1) - want).max() / np.abs(want).max()
    print(f"unit column: |x - x_ref|_max / |x_ref|_max = {err:.3e}; reference residual {ref.worst_residual:.3e}")
    assert ref.worst_residual <= 1e-9
    assert err <= BAR


REFRESH = ("k_galerkin", "k_galerkin @level0", "k_level_dinv", "k_p_values", "k_p_values @level0", "k_block_products<1, 0, 0>",
           "k_block_products<1, 0, 0> @level0", "k_block_products<0, 1, 1>", "k_block_products<0, 1, 1> @level0")


def test_the_coarse_operators_are_refreshed_once_per_call():
    g, P1, _ = _reference(PCG)
    V = g.V
    m, l = V // 2, V - 1

    def counts(opt, vi, vj):
        opt.profile_reset()
        opt.marginals(vi, vj)
        p = opt.kernel_profile()
        return {k: p.get(k, dict(launches=0))["launches"] for k in REFRESH + ("k_rhs_inject", "k_rhs_restore", "k_cov_gather", "k_linearize")}

    with capi.Optimizer(0, direct_rows=0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P1)
        one = counts(opt, [l], [l])
        three = counts(opt, [l, m, 1, l], [l, m, 1, m])
    print("one column vertex", one, "three", three)
    for k in REFRESH:    # ("k_galerkin" and "k_galerkin @level0" among them)
        assert three[k] == one[k], k
    assert sum(one[k] for k in REFRESH) > 0           # (there is a refresh to count)
    assert one["k_linearize"] == three["k_linearize"] == 1
    assert (one["k_rhs_inject"], three["k_rhs_inject"]) == (3, 9) and (one["k_cov_gather"], three["k_cov_gather"]) == (3, 9)
    assert one["k_rhs_restore"] == three["k_rhs_restore"] == 1


def test_refusals_leave_the_device_untouched():
    g, P1, _ = _reference(PCG)
    V = g.V
    # one extra vertex without any edge: not active
    arr = (np.vstack([P1, P1[-1] + 1.0]), np.append(g.fixed, False)) + tuple(g.arrays()[2:])
    L = capi.lib()
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(*arr)
        s0 = _state(opt)
        for vi, vj in (([1, V + 1], [1, 1]), ([1], [-1]), ([V], [1]), ([1], [V])):    # outside [0, V + 1); without edges
            with pytest.raises(capi.SgoError, match="rc=-2"):
                opt.marginals(vi, vj)
            assert _same(_state(opt), s0), (vi, vj)
        assert "not active" in opt.last_error() and f"vertex {V}" in opt.last_error()
        one = np.array([1], dtype=np.int32)
        out = np.full(9, 7.0)
        ip, dp = capi._ip, capi._dp
        assert L.sgo_marginals(opt._h, 1, None, ip(one), dp(out)) == -2
        assert L.sgo_marginals(opt._h, 1, ip(one), None, dp(out)) == -2
        assert L.sgo_marginals(opt._h, 1, ip(one), ip(one), None) == -2
        assert L.sgo_marginals(opt._h, -1, ip(one), ip(one), dp(out)) == -2
        assert np.all(out == 7.0) and _same(_state(opt), s0)
        assert L.sgo_marginals(opt._h, 0, None, None, None) == 0
    with capi.Optimizer(0) as opt:
        assert L.sgo_marginals(opt._h, 1, ip(one), ip(one), dp(out)) == -4      # no graph
    # the rank emulation of a multi-GPU context
    with capi.Optimizer(0, direct_rows=0, solver=capi.SOLVER_PCG_BJ) as opt:
        opt.debug_set_shard(2, 0)
        opt.set_graph(*g.arrays())
        s0 = _state(opt)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.marginals([1], [1])
        assert "multi-GPU" in opt.last_error()
        assert _same(_state(opt), s0)


def test_an_active_overlay_is_refused():
    base, steps, g, arrs, V, fixed, ids = _overlay_session()
    with capi.Optimizer(0, direct_rows=0) as opt:
        _grow(opt, base, steps, g, 6)
        assert "incremental overlay" in opt.solver_description()
        e0, c0 = opt.edge_chi2().view(np.uint64), opt.chi2()
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.marginals([1], [1])
        assert "incremental overlay" in opt.last_error()
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.solve_rhs(np.zeros((opt.n_free, 3)))
        assert np.array_equal(opt.edge_chi2().view(np.uint64), e0) and opt.chi2() == c0
        assert "incremental overlay" in opt.solver_description()


@pytest.fixture(scope="module")
def replay_marginals(tmp_path_factory):
    """replay_marginals built once, with the g++ line tests/cpp/Makefile uses for the other replays (that file has no target for it)"""
    libdir = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("replay_marginals") / "replay_marginals")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "replay_marginals.cpp"), "-L" + libdir, "-lsgo", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_compute_marginals_through_the_compat_headers(replay_marginals, tmp_path):
    g = _case(*DIRECT)[0]
    assert g.fixed[0] and not g.fixed[1:].any()       # hessian index h is vertex h + 1
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 1.0)
    env = dict(os.environ)
    for k in ("SGO_DIRECT_ROWS", "SGO_INCREMENTAL", "SGO_SOLVER"):
        env.pop(k, None)
    subprocess.check_call([replay_marginals, str(gf), str(of), "8"], env=env)
    lines = open(of).read().split("\n")
    assert int(lines[0]) == 8 and lines[1].startswith("direct_ldlt"), lines[:2]
    P = np.array([[float(v) for v in ln.split()] for ln in lines[2:2 + g.V]])
    blocks = [ln.split() for ln in lines[2 + g.V:] if ln and ln.split()[0] in ("vertex", "pairs", "container")]
    rows, cols, absent, lm = (int(v) for v in lines[2 + g.V + len(blocks)].split())
    n = g.V - 1
    assert (rows, cols, absent, lm) == (3 * n, 3 * n, 1, 0)
    assert [b[0] for b in blocks] == ["vertex"] + ["pairs"] * 5 + ["container"] * 2
    hl, hm = n - 1, (n - 1) // 2
    assert [(int(b[1]), int(b[2])) for b in blocks] == [(hl, hl), (0, 0), (hm, hm), (hl, hm), (hm, hl), (hl, hm), (0, 0), (hl, hl)]
    vi = np.array([int(b[1]) + 1 for b in blocks])
    vj = np.array([int(b[2]) + 1 for b in blocks])
    shim = np.array([[float(v) for v in b[3:]] for b in blocks]).reshape(-1, 3, 3)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        assert opt.solver_description().startswith("direct_ldlt")
        opt.set_poses(P)
        cov = opt.marginals(vi, vj)
    assert np.array_equal(shim.view(np.uint64), cov.view(np.uint64)), np.abs(shim - cov).max()
    for t in (0, 1, 2):
        assert np.array_equal(cov[t], cov[t].T) and np.all(np.linalg.eigvalsh(cov[t]) > 0)
