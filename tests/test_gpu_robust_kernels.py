"""Robust kernels beyond DCS, set per edge on every solver path (sgo_set_robust_kernels / sgo_edge_robust; robustify in
sparse_gslam_amd/csrc/sgo_device.h).  The bars are the project's own (test_gpu_edge_gate.py): linearisation 1e-12, relative chi2
1e-6 per iterate, poses 1e-5.

The reference is the CPU oracle under the identity of tests/robust_reference.py (the robustified system is the unrobustified one
with information w Omega), with delta = 1.5 and kind = 1 + (closure index mod 9) over the closures of the three shapes
test_gpu_edge_gate.py uses to reach each path, corrupted as there, from the oracle's 8-iteration DCS poses, for 6 iterations.
Every test that depends on a branch first asserts, on the reference alone, that no edge lies within 1e-5 (relative) of a branch
threshold at any reference iterate and that both branches of every piecewise kind (DCS, Huber, Tukey, Saturated) are populated:
conditions on the input, not tolerances.  At the PCG and the multifrontal shape every iterate keeps at least 13 edges on each
side; the direct shape has 31 closures -- 3 or 4 per kind -- and the Saturated ones all leave the quadratic branch after the
first iterate, so there the two branches are required over the run's iterates taken together."""
import functools
import os
import subprocess

import numpy as np
import pytest

import robust_reference as rr
from oracle import c_oracle
from sparse_gslam_amd import capi, synth
from test_gpu_edge_gate import GATE, PCG, _case, _close, _overlay_session, _same, _state
from test_shim_replay import _write_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFRONT, DIRECT = (2500, 3400, 31, 12), (600, 630, 5, 6)
DELTA, ITERS = 1.5, 6


def _mixed(g):
    """kind = 1 + (closure index mod 9) and delta = 1.5 on the closures; the odometry edges carry no kernel"""
    cl = np.flatnonzero(g.phi >= 0)
    kind = np.zeros(g.E, dtype=np.int32)
    kind[cl] = 1 + np.arange(cl.size) % 9
    return kind, np.where(g.phi >= 0, DELTA, 1.0)


@functools.lru_cache(maxsize=None)
def _ref(shape):
    """graph, the oracle's DCS poses, kinds, deltas, the reference's poses and per-iterate sums after ITERS iterations"""
    g, bad, P1 = _case(*shape)[:3]
    kind, delta = _mixed(g)
    P, st = rr.gauss_newton(c_oracle, P1, g, kind, delta, ITERS)
    # the input conditions, on the reference alone
    assert np.isfinite(P).all() and all(a > b for a, b in zip(st["robust_chi2"], st["robust_chi2"][1:]))
    lo_any, hi_any = {k: 0 for k in rr.PIECEWISE}, {k: 0 for k in rr.PIECEWISE}
    for e2 in st["e2"]:
        for k, (lo, hi, dist) in rr.branch_report(kind, e2, delta).items():
            assert dist > 1e-5, (shape, rr.NAMES[k], dist)
            if shape != DIRECT:
                assert lo >= 13 and hi >= 13, (shape, rr.NAMES[k], lo, hi)
            lo_any[k] += lo
            hi_any[k] += hi
    assert all(lo_any[k] > 0 and hi_any[k] > 0 for k in rr.PIECEWISE), (shape, lo_any, hi_any)
    P.setflags(write=False)
    return g, P1, kind, delta, P, st


def _set_mixed(opt, g, kind, delta):
    opt.set_robust_kernels(np.arange(g.E), kind, delta)


def test_linearisation_with_mixed_kinds_matches_the_reference():
    g, P1, kind, delta, _, _ = _ref(PCG)
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(*g.arrays())
        assert opt.solver_description().startswith("pcg_amg")
        opt.set_poses(P1)
        _set_mixed(opt, g, kind, delta)
        rho0, w = opt.edge_robust()
        plain, robust = opt.chi2()
        b, diag, c2, rc2 = opt.linearize()
        x = np.random.default_rng(0).standard_normal((opt.n_free, 3))
        y = opt.hessian_apply(x)
    ob, od, oc2, orc2, or0, ow = rr.linearize(c_oracle, P1, g, kind, delta)
    oy = c_oracle.hessian_apply(P1, g.fixed, g.ei, g.ej, g.meas, g.info * ow[:, None], np.full(g.E, -1.0), x).reshape(-1, 3)
    print("rho0", np.abs(rho0 - or0).max() / np.abs(or0).max(), "w", np.abs(w - ow).max(), "b", np.abs(b - ob).max() / np.abs(ob).max(),
          "diag", np.abs(diag - od).max() / np.abs(od).max(), "y", np.abs(y - oy).max() / np.abs(oy).max())
    # (3 000 poses span several tiles: edges whose two slots lie in different tiles carry every kind)
    assert np.abs(rho0 - or0).max() <= 1e-12 * np.abs(or0).max()
    assert np.abs(w - ow).max() <= 1e-12
    for k in range(10):   # every kind is among them, with weights that differ from the DCS ones where it is not DCS
        assert (kind == k).sum() >= 1000
    assert abs(plain - oc2) <= 1e-12 * oc2 and abs(robust - orc2) <= 1e-12 * orc2
    assert abs(c2 - oc2) <= 1e-12 * oc2 and abs(rc2 - orc2) <= 1e-12 * orc2
    assert np.abs(b - ob).max() <= 1e-12 * np.abs(ob).max()
    assert np.abs(diag - od).max() <= 1e-12 * np.abs(od).max()
    assert np.abs(y - oy).max() <= 1e-12 * np.abs(oy).max()


@pytest.mark.parametrize("shape,opts,path", [(PCG, dict(direct_rows=0), "pcg_amg"), (MFRONT, {}, "multifrontal_cholesky"),
                                             (DIRECT, {}, "direct_ldlt")], ids=["pcg", "mfront", "direct"])
def test_iterates_with_mixed_kinds_match_a_fresh_context_and_the_reference(shape, opts, path):
    g, P1, kind, delta, Pr, sr = _ref(shape)
    with capi.Optimizer(0, **opts) as opt, capi.Optimizer(0, **opts) as fresh:
        opt.set_graph(*g.arrays())
        assert opt.solver_description().startswith(path), opt.solver_description()
        d0, st0 = opt.optimize(ITERS)        # (the context has optimised with DCS before the kinds change)
        assert d0 == ITERS
        opt.set_poses(P1)
        _set_mixed(opt, g, kind, delta)
        d, st = opt.optimize(ITERS)
        P = opt.get_poses()
        desc = opt.solver_description()
        fresh.set_graph(P1, *g.arrays()[1:])
        _set_mixed(fresh, g, kind, delta)
        df, sf = fresh.optimize(ITERS)
        Pf = fresh.get_poses()
    assert desc.startswith(path), desc
    assert st["seconds_setup"] == st0["seconds_setup"]   # (no set-up ran)
    assert d == ITERS and df == ITERS
    print("robust chi2", st["robust_chi2"][:ITERS + 1], sr["robust_chi2"], "poses", np.abs(P - Pf).max(), np.abs(P - Pr).max())
    _close(st, sf, ITERS)
    _close(st, sr, ITERS)
    assert np.abs(P - Pf).max() <= 1e-5 and np.abs(P - Pr).max() <= 1e-5
    if path == "pcg_amg":
        assert set(st["pcg_converged"][:ITERS]) == {1}


def test_dcs_and_none_through_the_call_are_bit_identical():
    g, P1 = _case(*PCG)[0], _case(*PCG)[2]
    cl = np.flatnonzero(g.phi >= 0)
    with capi.Optimizer(0, direct_rows=0) as opt, capi.Optimizer(0, direct_rows=0) as plain:
        opt.set_graph(P1, *g.arrays()[1:])
        plain.set_graph(P1, *g.arrays()[1:-1], np.full(g.E, -1.0))
        s_dcs, s_none = _state(opt), _state(plain)
        assert not _same(s_dcs, s_none)
        for _ in range(2):
            opt.set_robust_kernels(cl, capi.KERNEL_DCS, g.phi[cl])
            assert _same(_state(opt), s_dcs)
            opt.set_robust_kernels(cl, capi.KERNEL_NONE, 0.0)
            assert _same(_state(opt), s_none)
            opt.set_robust_kernels(cl, capi.KERNEL_HUBER, DELTA)
            s_huber = _state(opt)
            assert not _same(s_huber, s_dcs) and not _same(s_huber, s_none)
        opt.set_robust_kernels(None, np.where(g.phi >= 0, capi.KERNEL_DCS, capi.KERNEL_NONE), np.abs(g.phi))
        assert _same(_state(opt), s_dcs)


@pytest.mark.parametrize("shape,opts,path", [(PCG, dict(direct_rows=0), "pcg_amg"), (MFRONT, {}, "multifrontal_cholesky"),
                                             (DIRECT, {}, "direct_ldlt")], ids=["pcg", "mfront", "direct"])
def test_a_graph_back_at_dcs_optimises_bit_for_bit_as_one_that_never_left(shape, opts, path):
    g = _case(*shape)[0]
    cl = np.flatnonzero(g.phi >= 0)
    with capi.Optimizer(0, **opts) as opt, capi.Optimizer(0, **opts) as never:
        never.set_graph(*g.arrays())
        dn, sn = never.optimize(3)
        opt.set_graph(*g.arrays())
        opt.set_robust_kernels(cl, capi.KERNEL_TUKEY, DELTA)
        opt.set_robust_kernels(cl, capi.KERNEL_DCS, g.phi[cl])
        assert opt.solver_description().startswith(path)
        d, st = opt.optimize(3)
        assert d == dn == 3
        assert st["chi2"][:4] == sn["chi2"][:4] and st["robust_chi2"][:4] == sn["robust_chi2"][:4]
        assert np.array_equal(opt.get_poses().view(np.uint64), never.get_poses().view(np.uint64))


@pytest.mark.parametrize("incremental", [True, False], ids=["overlay", "fallback"])
def test_kinds_under_an_overlay_and_across_the_fallback(incremental, monkeypatch):
    """A kind on a resident closure before the update, a kind on the last appended closure after it: as a fresh full set-up that
    carries both.  With SGO_INCREMENTAL=0 the update is a full set-up, and the resident prefix keeps its kinds, with delta from the phi
    passed: the caller's arrays carry the kernel's delta as phi, as the compat header's do."""
    if incremental:
        monkeypatch.delenv("SGO_INCREMENTAL", raising=False)
    else:
        monkeypatch.setenv("SGO_INCREMENTAL", "0")
    base, steps, g, arrs, V, fixed, ids = _overlay_session()
    names = ("ei", "ej", "meas", "info", "phi")
    full = [arrs[k] for k in names]
    res, last = int(ids[0]), int(ids[1])
    with capi.Optimizer(0, direct_rows=0) as opt, capi.Optimizer(0, direct_rows=0) as fresh:
        opt.set_graph(*base.arrays())
        assert opt.optimize(ITERS)[0] == ITERS
        opt.set_robust_kernels([res], capi.KERNEL_TUKEY, 4.0)
        P, E_res = opt.get_poses(), base.E
        cur = [getattr(base, k).copy() for k in names]
        cur[4][res] = 4.0
        for s in steps:
            cur = [np.concatenate([a, s[k]]) for a, k in zip(cur, names)]
            P0 = np.empty((s["V"], 3))
            P0[: P.shape[0]] = P
            synth.chain_init(P0, g.meas[: g.V - 1], P.shape[0], s["V"] - 1)
            fx = np.zeros(s["V"], dtype=bool)
            fx[0] = True
            opt.update_graph(P0, fx, *cur, E_res)
            assert ("incremental overlay" in opt.solver_description()) == incremental, opt.solver_description()
            P, E_res = P0, cur[0].size
        assert E_res == full[0].size and last == E_res - 1
        opt.set_robust_kernels([last], capi.KERNEL_CAUCHY, 2.0)
        assert ("incremental overlay" in opt.solver_description()) == incremental
        r0, w = opt.edge_robust()
        fresh.set_graph(P0, fixed, *full)
        fresh.set_robust_kernels([res, last], [capi.KERNEL_TUKEY, capi.KERNEL_CAUCHY], [4.0, 2.0])
        f0, fw = fresh.edge_robust()
        dcs0, dcsw = rr.rho(rr.DCS, fresh.edge_chi2()[[res, last]], 1.0)
        assert np.abs(r0 - f0).max() <= 1e-12 * np.abs(f0).max() and np.abs(w - fw).max() <= 1e-12
        assert np.all(np.abs(fw[[res, last]] - dcsw) > 1e-3), (fw[[res, last]], dcsw)   # (the two kinds show: not the DCS weights)
        d, st = opt.optimize(ITERS)
        df, sf = fresh.optimize(ITERS)
        assert d == ITERS and df == ITERS
        _close(st, sf, ITERS)
        assert np.abs(opt.get_poses() - fresh.get_poses()).max() <= 1e-5


def test_the_gate_takes_the_edges_with_any_kernel_and_composes_with_every_kind():
    g, P1, kind, delta, _, _ = _ref(PCG)
    bad = _case(*PCG)[1]
    kind = kind.copy()
    kind[bad[0]] = capi.KERNEL_NONE          # a corrupted closure without a kernel: the gate must leave it alone
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P1)
        _set_mixed(opt, g, kind, delta)
        before = opt.edge_chi2()
        assert before[bad[0]] > GATE
        assert np.abs(before[kind != 0] / GATE - 1.0).min() > 1e-6   # (the input keeps clear of the gate's threshold)
        k, gated = opt.gate_edges(None, GATE)
        rho0, w = opt.edge_robust()
        after = opt.edge_chi2()
    assert np.array_equal(gated, (kind != capi.KERNEL_NONE) & (before > GATE))
    assert k == int(gated.sum()) and not gated[bad[0]]
    for kk in range(1, 10):
        assert gated[kind == kk].any(), rr.NAMES[kk]
    tukey = gated & (kind == capi.KERNEL_TUKEY)
    assert np.all(rho0[tukey] == 0.0) and np.all(w[tukey] == 1.0)
    assert np.all(after[gated] == 0.0) and np.all(rho0[gated] == 0.0) and np.all(w[gated] == 1.0)


def test_refusals_leave_the_device_untouched():
    g, P1 = _case(*PCG)[0], _case(*PCG)[2]
    cl = np.flatnonzero(g.phi >= 0)
    e = int(cl[3])
    refused = [([e, g.E], [2, 2], [1.0, 1.0]), ([e, -1], [2, 2], [1.0, 1.0]),                 # an id out of range
               ([e], [10], [1.0]), ([e], [-1], [1.0]),                                         # an unknown kind
               ([e], [2], [np.nan]), ([e], [4], [np.inf]), ([e], [0], [np.nan]),               # a non-finite delta
               ([e], [1], [-0.5])]                                                             # delta < 0 for DCS
    refused += [([e], [k], [dl]) for k in range(2, 10) for dl in (0.0, -1.0)]                  # delta <= 0 for any other kind
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(P1, *g.arrays()[1:])
        s0 = _state(opt)
        r0 = [a.view(np.uint64) for a in opt.edge_robust()]
        for ids, kk, dl in refused:
            with pytest.raises(capi.SgoError, match="rc=-2"):
                opt.set_robust_kernels([int(cl[5])] + ids, [capi.KERNEL_HUBER] + kk, [DELTA] + dl)   # (a valid entry first)
            assert _same(_state(opt), s0), (ids, kk, dl)
        assert _same([a.view(np.uint64) for a in opt.edge_robust()], r0)
        opt.set_robust_kernels([e], capi.KERNEL_NONE, -1.0)        # (NONE ignores its delta)
        opt.set_robust_kernels([e, e], [capi.KERNEL_HUBER, capi.KERNEL_DCS], [DELTA, g.phi[e]])   # of an id listed twice the later entry counts
        assert _same(_state(opt), s0)
    # the rank emulation of a multi-GPU context (block-Jacobi PCG: the single-step entry points need no other rank there)
    with capi.Optimizer(0, direct_rows=0, solver=capi.SOLVER_PCG_BJ) as opt:
        opt.debug_set_shard(2, 0)
        opt.set_graph(*g.arrays())
        s0 = _state(opt)
        r0 = [a.view(np.uint64) for a in opt.edge_robust()]
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.set_robust_kernels([e], capi.KERNEL_HUBER, DELTA)
        assert _same(_state(opt), s0)
        assert _same([a.view(np.uint64) for a in opt.edge_robust()], r0)


@pytest.fixture(scope="module")
def replay_robust(tmp_path_factory):
    """replay_robust built once with the g++ line of tests/cpp/Makefile"""
    libdir = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("replay_robust") / "replay_robust")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "replay_robust.cpp"), "-L" + libdir, "-lsgo", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("shape,direct_rows,path", [(MFRONT, None, "multifrontal_cholesky"), (PCG, "0", "pcg_amg")], ids=["mfront", "pcg"])
def test_huber_and_cauchy_through_the_shim_take_the_gpu_path(replay_robust, tmp_path, shape, direct_rows, path):
    """Huber on the even closures, Cauchy on the odd ones, delta = 2: with 4 500 Huber edges at the PCG shape delta = 1.5 brings one
    of them within 7e-6 of its threshold at the first reference iterate, delta = 2 keeps every iterate of both shapes 5e-5 clear."""
    shim_delta = 2.0
    g, _, P1 = _case(*shape)[:3]
    cl = np.flatnonzero(g.phi >= 0)
    kind = np.zeros(g.E, dtype=np.int32)
    kind[cl] = np.where(np.arange(cl.size) % 2 == 0, rr.HUBER, rr.CAUCHY)
    delta = np.where(g.phi >= 0, shim_delta, 1.0)
    Pr, sr = rr.gauss_newton(c_oracle, P1, g, kind, delta, ITERS)
    for e2 in sr["e2"]:
        lo, hi, dist = rr.branch_report(kind, e2, delta)[rr.HUBER]
        assert dist > 1e-5 and lo >= 13 and hi >= 13, (lo, hi, dist)
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, synth.Graph(np.array(P1), g.fixed, g.ei, g.ej, g.meas, g.info, g.phi, g.truth, dict(g.meta)), shim_delta)
    env = dict(os.environ)
    env.pop("SGO_DIRECT_ROWS", None)
    env.pop("SGO_INCREMENTAL", None)
    if direct_rows is not None:
        env["SGO_DIRECT_ROWS"] = direct_rows
    subprocess.check_call([replay_robust, str(gf), str(of), str(ITERS)], env=env)
    lines = open(of).read().split("\n")
    done, c2, rc2 = lines[0].split()
    assert lines[1].startswith(path), lines[1]          # (the GPU path, not the dense host solver)
    assert int(done) == ITERS
    assert abs(float(c2) - sr["chi2"][-1]) <= 1e-6 * sr["chi2"][-1]
    assert abs(float(rc2) - sr["robust_chi2"][-1]) <= 1e-6 * sr["robust_chi2"][-1]
    P = np.loadtxt(lines[2:2 + g.V])
    assert np.abs(P - Pr).max() <= 1e-5
