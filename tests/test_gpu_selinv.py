"""Marginal covariances of every pose by selected inversion of the multifrontal factor (sgo_marginals_selected; kernels in
sparse_gslam_amd/csrc/sgo_selinv.hip, driver in sgo_selinv.cpp), and its route through the compat headers' computeMarginals.

References.  On the cases of tests/mfront_cases.py (the smallest graphs that reach every panel width, gather K, tree shape and
both front-size branches): the dense inverse of the oracle's robustified Hessian at the same poses (tests/selinv_reference.py;
the CPU test tests/test_selinv_reference.py qualifies these cases with the long-double-refined inverse, here the sparse LU's fp64
columns serve: the bar is 1e-6).  On the mid-size graphs: tests/marginals_reference.py's SuperLU columns, input condition
|H x - e|_inf <= 1e-9 asserted on the reference alone, and sgo_marginals itself.

Bar: the project's own for marginals, |Sigma - Sigma_ref|_max <= 1e-6 x sqrt(max |Sigma_ii| max |Sigma_jj|).  Two results that are
both held to it against the same reference (sgo_marginals_selected and sgo_marginals) may differ by twice that.  The three cases
tests/selinv_reference.ILL_CONDITIONED lists by name (the fp64 model itself is further than 1e-8 from the inverse there) are
checked for finite entries and symmetric positive definite diagonal blocks instead.  Every test prints its measured worst ratio."""
import functools
import os
import subprocess

import numpy as np
import pytest

import marginals_reference as mref
import mfront_cases as mc
import selinv_reference as sr
import test_gpu_marginals as tgm
import test_gpu_mfront as tmf
from oracle import np_oracle as npo
from sparse_gslam_amd import capi, synth
from test_gpu_edge_gate import GATE, _case, _grow, _overlay_session, _same, _state
from test_gpu_robust_kernels import DIRECT, MFRONT, _mixed
from test_shim_replay import _write_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = sr.DEVICE_BAR
PATHS = [(MFRONT, {}, "multifrontal_cholesky"), (DIRECT, {}, "direct_ldlt"), (DIRECT, dict(direct_rows=0), "pcg_amg")]
IDS = ["mfront", "direct", "forced_pcg"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", mc.NAMES)
def test_every_stored_entry_of_every_front(name):
    c = mc.make(name)
    vi, vj = np.r_[c.ei, c.ej], np.r_[c.ej, c.ei]       # every edge in both orientations (fixed endpoints: zero blocks)
    with mc.environment(c.env), capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(*c.arrays())
        assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
        o.optimize(1)
        o.set_poses(c.poses)
        x0 = o.mfront_arrays(("X",))["X"]
        assert o.mfront_arrays(("SEL",))["SEL"].size == 0       # nothing before the first call
        D, cov = o.marginals_selected(vi, vj)
        X = o.mfront_arrays(("INFO", "FRONTS", "BND", "ELIM_VERTEX", "TARGETS", "CONTRIB", "PINV", "SEL", "X", "ARENA", "FLAGS"))
        D2, cov2 = o.marginals_selected(vi, vj)
        sel2 = o.mfront_arrays(("SEL",))["SEL"]
        nf = o.last_selected_fronts
    shape = mc.check_shape(c, X)
    assert shape and all(shape.values()), (name, shape)
    assert nf == X["FRONTS"].shape[0] and X["SEL"].size == X["ARENA"].size and not X["FLAGS"][0]
    assert np.array_equal(_bits(x0), _bits(X["X"]))                                  # the call leaves the step alone
    assert np.array_equal(_bits(D), _bits(D2)) and np.array_equal(_bits(cov), _bits(cov2)) and np.array_equal(_bits(X["SEL"]), _bits(sel2))
    E = c.ei.size
    assert np.array_equal(_bits(cov[:E]), _bits(cov[E:].transpose(0, 2, 1).copy()))  # (vi, vj) is (vj, vi) transposed, bit for bit
    assert np.array_equal(_bits(D), _bits(D.transpose(0, 2, 1).copy()))
    plan = sr.Plan(X, c.fixed)
    S = [sr.front_from_arena(X["SEL"], F) for F in plan.fronts]
    hidx, free = npo.hessian_index(c.fixed)
    V = c.poses.shape[0]
    if name in sr.ILL_CONDITIONED:
        for Sf in S:
            assert np.isfinite(np.tril(Sf)).all()
        assert np.isfinite(D).all() and np.isfinite(cov).all()
        for v in range(V):
            if hidx[v] >= 0:
                assert np.linalg.eigvalsh(D[v]).min() > 0.0, (v, D[v])
            else:
                assert not D[v].any()
        print(f"{name}: left out of the accuracy comparison (fp64 model {sr.ILL_CONDITIONED[name]:.2e} of the natural scale from the "
              "long-double inverse); finite, symmetric, positive definite")
        return
    H = mref.hessian(c.poses, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
    Sigma, _ = sr.dense_inverse(H, refine=False)
    ratio, where = sr.worst_ratio(plan, S, Sigma)
    rd = sr.block_ratio(D, np.arange(V), np.arange(V), Sigma, hidx)
    rp = sr.block_ratio(cov, vi, vj, Sigma, hidx)
    print(f"{name}: worst |S - Sigma| / natural scale: fronts {ratio:.3e} at {where}, diag {rd:.3e}, edge blocks {rp:.3e}")
    assert ratio <= BAR and rd <= BAR and rp <= BAR


@functools.lru_cache(maxsize=None)
def _sample(shape):
    """16 free vertices and 32 edges between free vertices of the shape's graph"""
    g = _case(*shape)[0]
    rng = np.random.default_rng(5)
    vs = np.sort(rng.choice(np.flatnonzero(~g.fixed), size=16, replace=False))
    ok = np.flatnonzero(~g.fixed[g.ei] & ~g.fixed[g.ej])
    es = np.sort(rng.choice(ok, size=32, replace=False))
    return vs, es


@pytest.mark.parametrize("shape,opts,path", PATHS, ids=IDS)
def test_all_poses_on_every_path(shape, opts, path):
    g, P1, ref = tgm._reference(shape)
    vs, es = _sample(shape)
    vi, vj = np.r_[vs, g.ei[es]], np.r_[vs, g.ej[es]]
    with capi.Optimizer(0, **opts) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P1)
        before = opt.solver_description()
        D, cov = opt.marginals_selected(g.ei[es], g.ej[es])
        after = opt.solver_description()
        old = opt.marginals(vi, vj)
    assert before == after and before.split(":")[0] == path, (before, after)
    new = np.concatenate([D[vs], cov])
    worst = mref.worst_ratio(new, ref, vi, vj)
    both = float(np.max(np.abs(new - old).reshape(len(vi), -1).max(1) / ref.scales(vi, vj)))
    print(f"{path}: worst |Sigma - Sigma_ref| / natural scale = {worst:.3e}; against sgo_marginals {both:.3e}; "
          f"worst reference column residual = {ref.worst_residual:.3e}")
    assert ref.worst_residual <= 1e-9     # (the input condition, on the reference alone)
    assert worst <= BAR and both <= 2 * BAR
    assert not D[g.fixed].any() and np.array_equal(D, D.transpose(0, 2, 1))
    free = np.flatnonzero(~g.fixed)
    assert np.linalg.eigvalsh(D[free]).min() > 0.0


def test_a_graph_the_analysis_refuses_returns_enothing():
    g = synth.manhattan(1000, 4000, seed=3, info_mode="full")
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        desc = opt.solver_description()
        assert "multifrontal path not used: " in desc, desc
        why = desc.split("multifrontal path not used: ")[1].split(";")[0]
        for _ in range(2):                # (the refusal is cached per set-up)
            with pytest.raises(capi.SgoError, match="rc=-1"):
                opt.marginals_selected()
            assert why in opt.last_error() and "sgo_marginals" in opt.last_error(), (why, opt.last_error())
        assert opt.solver_description() == desc
        assert opt.optimize(2)[0] == 2


@pytest.mark.parametrize("shape,opts,path", PATHS[:2], ids=IDS[:2])
def test_a_later_optimize_has_the_bits_of_a_context_that_never_called(shape, opts, path):
    g = _case(*shape)[0]
    with capi.Optimizer(0, **opts) as opt, capi.Optimizer(0, **opts) as fresh:
        for o in (opt, fresh):
            o.set_graph(*g.arrays())
            assert o.solver_description().startswith(path)
        a = [opt.optimize(5)]
        opt.marginals_selected()
        a.append(opt.optimize(5))
        b = [fresh.optimize(5), fresh.optimize(5)]
        same_poses = np.array_equal(_bits(opt.get_poses()), _bits(fresh.get_poses()))
    for (d, st), (df, sf) in zip(a, b):
        assert d == df == 5 and st["chi2"] == sf["chi2"] and st["robust_chi2"] == sf["robust_chi2"]
    assert same_poses


def test_weights_and_gating_are_in_the_matrix():
    g, P1, ref = tgm._reference(MFRONT, "mixed")
    _, _, gref = tgm._reference(MFRONT, "gated")
    ogate = _case(*MFRONT)[4]
    kind, delta = _mixed(g)
    gated_free = np.flatnonzero(ogate & ~g.fixed[g.ei] & ~g.fixed[g.ej])[:8]
    assert gated_free.size > 0
    vs = np.unique(np.r_[g.ei[gated_free], g.ej[gated_free]])
    vi, vj = np.r_[vs, g.ei[gated_free]], np.r_[vs, g.ej[gated_free]]       # (a deactivated edge's pair stays in the pattern)
    # on the reference first: the gate shows in the blocks of the gated edges' endpoints
    change = max(np.abs(gref.block(v, v) - ref.block(v, v)).max() / np.abs(ref.block(v, v)).max() for v in vs)
    assert change > 1e-3, change
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        assert opt.solver_description().startswith("multifrontal_cholesky")
        opt.set_poses(P1)
        opt.set_robust_kernels(np.arange(g.E), kind, delta)
        D, cov = opt.marginals_selected(g.ei[gated_free], g.ej[gated_free])
        k, gated = opt.gate_edges(None, GATE)
        assert np.array_equal(gated, ogate) and k == int(ogate.sum())
        gD, gcov = opt.marginals_selected(g.ei[gated_free], g.ej[gated_free])
    w = mref.worst_ratio(np.concatenate([D[vs], cov]), ref, vi, vj)
    gw = mref.worst_ratio(np.concatenate([gD[vs], gcov]), gref, vi, vj)
    print(f"mixed kinds: worst ratio {w:.3e}; gated: {gw:.3e}; reference residuals {ref.worst_residual:.3e}, {gref.worst_residual:.3e}")
    assert ref.worst_residual <= 1e-9 and gref.worst_residual <= 1e-9
    assert w <= BAR and gw <= BAR
    assert max(np.abs(gD[v] - D[v]).max() / np.abs(D[v]).max() for v in vs) > 1e-3


def _outside_pair(g):
    """two free vertices no front holds together, from the host plan: the first-eliminated pose and one its front does not list"""
    X = capi.mfront_plan_arrays(*g.arrays()[:4])
    F = X["FRONTS"][0]
    held = set(range(int(F[0]), int(F[0]) + int(F[1]) // 3)) | set(int(p) for p in X["BND"][int(F[6]):int(F[6]) + int(F[5])])
    other = next(p for p in range(int(X["INFO"][0]) - 1, -1, -1) if p not in held)
    return int(X["ELIM_VERTEX"][int(F[0])]), int(X["ELIM_VERTEX"][other])


def test_refusals_leave_the_device_and_the_outputs_untouched():
    g, P1, _ = tgm._reference(MFRONT)
    V = g.V
    arr = (np.vstack([P1, P1[-1] + 1.0]), np.append(g.fixed, False)) + tuple(g.arrays()[2:])   # one extra vertex without any edge
    a, b = _outside_pair(g)
    L = capi.lib()
    ip, dp = capi._ip, capi._dp
    one = np.array([1], dtype=np.int32)
    out, dg = np.full(9, 7.0), np.full((V + 1) * 9, 7.0)
    with capi.Optimizer(0) as opt, capi.Optimizer(0) as fresh:
        for o in (opt, fresh):
            o.set_graph(*arr)
            assert o.solver_description().startswith("multifrontal_cholesky")
        s0 = _state(opt)
        _state(fresh)                      # (the same lazily built structures on both)
        for vi, vj in (([1, V + 1], [1, 1]), ([1], [-1]), ([V], [1]), ([1], [V]), ([a], [b]), ([b, 1], [a, 1])):
            with pytest.raises(capi.SgoError, match="rc=-2"):
                opt.marginals_selected(vi, vj)
            assert _same(_state(opt), s0), (vi, vj)
        assert "outside the factor's pattern" in opt.last_error() and "sgo_marginals" in opt.last_error()
        assert f"({b}, {a})" in opt.last_error()
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.marginals_selected([V], [1])
        assert "not active" in opt.last_error() and f"vertex {V}" in opt.last_error()
        pa, pb = np.array([a], dtype=np.int32), np.array([b], dtype=np.int32)
        assert L.sgo_marginals_selected(opt._h, dp(dg), 1, ip(pa), ip(pb), dp(out)) == -2
        assert L.sgo_marginals_selected(opt._h, dp(dg), 1, None, ip(one), dp(out)) == -2
        assert L.sgo_marginals_selected(opt._h, dp(dg), 1, ip(one), None, dp(out)) == -2
        assert L.sgo_marginals_selected(opt._h, dp(dg), 1, ip(one), ip(one), None) == -2
        assert L.sgo_marginals_selected(opt._h, dp(dg), -1, ip(one), ip(one), dp(out)) == -2
        assert np.all(out == 7.0) and np.all(dg == 7.0) and _same(_state(opt), s0)
        assert np.array_equal(_bits(opt.get_poses()), _bits(arr[0]))
        # the vertex without an edge has a zero diagonal block, and asking for the diagonal alone needs no pair buffers
        assert L.sgo_marginals_selected(opt._h, dp(dg), 0, None, None, None) > 0
        assert not dg.reshape(-1, 9)[V].any() and not dg.reshape(-1, 9)[0].any() and dg.reshape(-1, 9)[1].all()
        fresh.marginals_selected()
        pairs = ([1, V // 2, V - 1], [1, V // 2, V // 2])
        assert np.array_equal(_bits(opt.marginals(*pairs)), _bits(fresh.marginals(*pairs)))
        (d, st), (df, sf) = opt.optimize(3), fresh.optimize(3)
        assert d == df == 3 and st["chi2"] == sf["chi2"]
        assert np.array_equal(_bits(opt.get_poses()), _bits(fresh.get_poses()))
    with capi.Optimizer(0) as opt:
        assert L.sgo_marginals_selected(opt._h, None, 1, ip(one), ip(one), dp(out)) == -4      # no graph
    # the rank emulation of a multi-GPU context
    with capi.Optimizer(0, direct_rows=0, solver=capi.SOLVER_PCG_BJ) as opt:
        opt.debug_set_shard(2, 0)
        opt.set_graph(*g.arrays())
        s0 = _state(opt)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.marginals_selected([1], [1])
        assert "multi-GPU" in opt.last_error()
        assert _same(_state(opt), s0)


def test_an_active_overlay_is_refused():
    base, steps, g, arrs, V, fixed, ids = _overlay_session()
    with capi.Optimizer(0, direct_rows=0) as opt:
        _grow(opt, base, steps, g, 6)
        assert "incremental overlay" in opt.solver_description()
        e0, c0 = opt.edge_chi2().view(np.uint64), opt.chi2()
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.marginals_selected([1], [1])
        assert "incremental overlay" in opt.last_error()
        assert np.array_equal(opt.edge_chi2().view(np.uint64), e0) and opt.chi2() == c0
        assert "incremental overlay" in opt.solver_description()


def test_an_indefinite_hessian_fails_and_leaves_the_outputs():
    """the failure path of test_gpu_mfront.py's indefinite graph (negated information: a pivot block fails its test, no fault)"""
    g = tmf.chain_graph(700, 150, seed=16)
    info = g.info.copy()
    info[:, [0, 3, 5]] *= -1.0
    L = capi.lib()
    one = np.array([1], dtype=np.int32)
    out, dg = np.full(9, 7.0), np.full(g.V * 9, 7.0)
    with capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)
        assert o.solver_description().startswith("multifrontal_cholesky")
        assert L.sgo_marginals_selected(o._h, capi._dp(dg), 1, capi._ip(one), capi._ip(one), capi._dp(out)) == -2
        assert "not positive definite" in o.last_error()
        assert np.all(out == 7.0) and np.all(dg == 7.0)
        rc, st = o.optimize(5)                           # as without the call: fails at iteration 0, the estimates stay
        assert rc == 0 and st["iters_done"] == 0 and np.array_equal(o.get_poses(), g.poses)
        o.set_graph(*g.arrays())
        D, _ = o.marginals_selected()
        assert np.isfinite(D).all()
        assert o.optimize(2)[0] == 2


@pytest.fixture(scope="module")
def replays(tmp_path_factory):
    """replay_marginals_all and replay_marginals, built with the g++ line test_gpu_marginals.py uses"""
    libdir = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
    d = tmp_path_factory.mktemp("replay_marginals_all")
    out = []
    for name in ("replay_marginals_all", "replay_marginals"):
        exe = str(d / name)
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L" + libdir, "-lsgo", "-Wl,-rpath," + libdir,
                               "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
        out.append(exe)
    return out


def _replay_env():
    env = dict(os.environ)
    for k in ("SGO_DIRECT_ROWS", "SGO_INCREMENTAL", "SGO_SOLVER"):
        env.pop(k, None)
    return env


def test_compute_marginals_of_every_vertex_through_the_compat_headers(replays, tmp_path):
    """the VertexContainer overload with every vertex of a chain-plus-closures graph: more than 8 distinct column vertices, so the
    shim asks sgo_marginals_selected; the blocks are that call's, bit for bit, and the reference's within the bar"""
    g = _case(*DIRECT)[0]
    assert g.fixed[0] and not g.fixed[1:].any()       # hessian index h is vertex h + 1
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 1.0)
    subprocess.check_call([replays[0], str(gf), str(of), "8"], env=_replay_env())
    lines = open(of).read().split("\n")
    assert int(lines[0]) == 8 and lines[1].startswith("direct_ldlt"), lines[:2]
    assert lines[2] == lines[1]                        # the backend description after computeMarginals
    P = np.array([[float(v) for v in ln.split()] for ln in lines[3:3 + g.V]])
    blocks = [ln.split() for ln in lines[3 + g.V:] if ln and ln.split()[0] == "block"]
    n = g.V - 1
    assert [int(b[1]) for b in blocks] == list(range(n))
    shim = np.array([[float(v) for v in b[2:]] for b in blocks]).reshape(-1, 3, 3)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P)
        D, _ = opt.marginals_selected()
    assert np.array_equal(_bits(shim), _bits(D[1:]))
    ref = mref.Reference(mref.hessian(P, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi), g.fixed)
    vs = _sample(DIRECT)[0]
    worst = mref.worst_ratio(shim[vs - 1], ref, vs, vs)
    print(f"computeMarginals(all vertices): worst ratio {worst:.3e} on 16 vertices; reference residual {ref.worst_residual:.3e}")
    assert ref.worst_residual <= 1e-9 and worst <= BAR


def test_the_existing_replay_keeps_its_route(replays, tmp_path):
    """requests with up to 8 distinct column vertices stay with sgo_marginals: replay_marginals' blocks are that call's bits"""
    g = _case(*DIRECT)[0]
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 1.0)
    subprocess.check_call([replays[1], str(gf), str(of), "8"], env=_replay_env())
    lines = open(of).read().split("\n")
    P = np.array([[float(v) for v in ln.split()] for ln in lines[2:2 + g.V]])
    blocks = [ln.split() for ln in lines[2 + g.V:] if ln and ln.split()[0] in ("vertex", "pairs", "container")]
    assert len(blocks) == 8
    vi = np.array([int(b[1]) + 1 for b in blocks])
    vj = np.array([int(b[2]) + 1 for b in blocks])
    shim = np.array([[float(v) for v in b[3:]] for b in blocks]).reshape(-1, 3, 3)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P)
        cov = opt.marginals(vi, vj)
    assert np.array_equal(_bits(shim), _bits(cov))
