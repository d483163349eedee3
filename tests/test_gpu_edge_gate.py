"""Deactivating and gating edges on the device without a new set-up (sgo_set_edge_information / sgo_gate_edges,
sparse_gslam_amd/csrc/sgo_gate.hip): the reference's closure gate -- edge.computeError(); if (edge.chi2() > 11.345) removeEdge(&edge);
for every closure, then initializeOptimization(); optimize(20) (log_runner.cpp:182-204) -- with "removed" represented as
"information = 0" in the operand arrays the resident kernels read.  The bars are the project's own (test_gpu_incremental.py,
test_gpu_parity.py): relative chi2 1e-6 per iterate, poses 1e-5, linearisation 1e-12.

Every gate test runs the CPU oracle first (8 Gauss-Newton iterations from the initial poses) and uploads ITS poses before gating, so
that the gate's decisions do not depend on solver noise; the oracle's per-edge chi2 defines the expected set, and no closure may lie
within 1e-6 (relative) of the threshold -- a condition on the input, not a tolerance."""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from sparse_gslam_amd import capi, synth

pytestmark = pytest.mark.gpu
GATE = 11.345


def _corrupted(V, E, seed, nbad, extras=False):
    g = synth.manhattan(V, E, seed=seed, info_mode="full", phi=1.0)
    rng = np.random.default_rng(0)
    n_odom = g.meta["n_odom"]
    bad = n_odom + rng.choice(g.E - n_odom, size=nbad, replace=False)
    clean = g.meas[bad].copy()
    g.meas[bad, :2] += rng.normal(0, 3.0, (nbad, 2))
    if extras:
        # a duplicated closure (the same pair twice, only one of the two corrupted) and a corrupted closure to the fixed vertex 0
        j = g.V // 2
        z0 = synth._rel(g.truth[0:1], g.truth[j:j + 1])[0].copy()
        z0[:2] += (2.5, -3.5)
        # (the twin: the corrupted closure whose clean measurement fits the true poses best, so that the clean copy stays)
        t = int(np.argmin(c_oracle.edges(g.truth[g.ei[bad]], g.truth[g.ej[bad]], clean, g.info[bad], g.phi[bad])[3]))
        k, clean = bad[t], clean[t]
        g = synth.Graph(g.poses, g.fixed, np.append(g.ei, [g.ei[k], 0]).astype(np.int32), np.append(g.ej, [g.ej[k], j]).astype(np.int32),
                        np.vstack([g.meas, clean, z0]), np.vstack([g.info, g.info[k], g.info[k]]), np.append(g.phi, [1.0, 1.0]),
                        g.truth, dict(g.meta))
        bad = np.concatenate([[k], bad[bad != k]])   # (the twinned one first)
    return g, bad


@functools.lru_cache(maxsize=None)
def _case(V, E, seed, nbad, extras=False):
    """graph, corrupted closures, the oracle's poses after 8 iterations, its per-edge chi2 there, the edges its gate removes"""
    g, bad = _corrupted(V, E, seed, nbad, extras)
    P1, _ = c_oracle.gauss_newton(*g.arrays(), iters=8)
    e2 = c_oracle.edges(P1[g.ei], P1[g.ej], g.meas, g.info, g.phi)[3]
    closure = g.phi >= 0
    assert np.abs(e2[closure] / GATE - 1.0).min() > 1e-6   # (the input keeps clear of the threshold)
    gate = closure & (e2 > GATE)
    for a in (P1, e2, gate):
        a.setflags(write=False)
    return g, bad, P1, e2, gate


@functools.lru_cache(maxsize=None)
def _oracle_after_gate(V, E, seed, nbad, iters):
    g, _, P1, _, gate = _case(V, E, seed, nbad)
    keep = ~gate
    P2, s2 = c_oracle.gauss_newton(P1, g.fixed, g.ei[keep], g.ej[keep], g.meas[keep], g.info[keep], g.phi[keep], iters=iters)
    return P2, s2


def _reduced(g, keep):
    return g.fixed, g.ei[keep], g.ej[keep], g.meas[keep], g.info[keep], g.phi[keep]


def _close(st, ref, iters):
    assert st["iters_done"] == iters
    for k in range(iters + 1):
        assert abs(st["chi2"][k] - ref["chi2"][k]) <= 1e-6 * ref["chi2"][k], (k, st["chi2"][k], ref["chi2"][k])
        assert abs(st["robust_chi2"][k] - ref["robust_chi2"][k]) <= 1e-6 * ref["robust_chi2"][k], (k, st["robust_chi2"][k], ref["robust_chi2"][k])


PCG = (3000, 12000, 7, 12)


def test_the_decision_is_edge_chi2s_bit_for_bit():
    g, bad, P1, oe2, ogate = _case(*PCG)
    assert int(ogate.sum()) == 696 and ogate[bad].all()
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(*g.arrays())
        assert opt.solver_description().startswith("pcg_amg")
        opt.set_poses(P1)
        before = opt.edge_chi2()
        k, gated = opt.gate_edges(None, GATE)
        after = opt.edge_chi2()
        desc = opt.solver_description()
        plain, robust = opt.chi2()
    assert np.array_equal(gated, (g.phi >= 0) & (before > GATE))
    assert np.array_equal(gated, ogate)
    assert k == int(gated.sum()) == 696
    assert np.all(after[gated] == 0.0)
    assert np.array_equal(after[~gated].view(np.uint64), before[~gated].view(np.uint64))
    assert "696 edges inactive" in desc and desc.startswith("pcg_amg"), desc
    oc, orc = c_oracle.chi2(P1, *_reduced(g, ~ogate))
    assert abs(plain - oc) <= 1e-11 * oc and abs(robust - orc) <= 1e-11 * orc


def test_linearisation_of_the_gated_graph_matches_the_oracle_of_the_graph_without_the_edges():
    g, bad, P1, oe2, ogate = _case(*PCG, extras=True)
    assert ogate[bad[0]] and not ogate[g.E - 2] and ogate[g.E - 1]   # (the corrupted twin goes, the clean one stays; the closure to vertex 0 goes)
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P1)
        k, gated = opt.gate_edges(None, GATE)
        assert np.array_equal(gated, ogate) and k == int(ogate.sum())
        assert "incremental overlay" not in opt.solver_description()
        b, diag, c2, rc2 = opt.linearize()
        x = np.random.default_rng(0).standard_normal((opt.n_free, 3))
        y = opt.hessian_apply(x)
    red = (P1,) + _reduced(g, ~ogate)
    ob, od, oc2, orc2 = c_oracle.linearize(*red)
    oy = c_oracle.hessian_apply(*red, x).reshape(-1, 3)
    # 3 000 poses span several tiles: edges whose two slots lie in different tiles are among the gated ones
    assert np.abs(b - ob).max() <= 1e-12 * np.abs(ob).max()
    assert np.abs(diag - od).max() <= 1e-12 * np.abs(od).max()
    assert abs(c2 - oc2) <= 1e-12 * oc2 and abs(rc2 - orc2) <= 1e-12 * orc2
    assert np.abs(y - oy).max() <= 1e-12 * np.abs(oy).max()


@pytest.mark.parametrize("shape,opts,path", [(PCG, dict(direct_rows=0), "pcg_amg"), ((2500, 3400, 31, 12), {}, "multifrontal_cholesky"),
                                             ((600, 630, 5, 6), {}, "direct_ldlt")], ids=["pcg", "mfront", "direct"])
def test_iterates_after_the_gate_match_a_fresh_set_up_and_the_oracle(shape, opts, path):
    iters = 8
    g, bad, P1, oe2, ogate = _case(*shape)
    assert ogate[bad].all()
    P2, s2 = _oracle_after_gate(*shape, iters)
    with capi.Optimizer(0, **opts) as opt, capi.Optimizer(0, **opts) as fresh:
        opt.set_graph(*g.arrays())
        assert opt.solver_description().startswith(path), opt.solver_description()
        d0, st0 = opt.optimize(iters)       # (the context has optimised before it gates, as the reference's has)
        assert d0 == iters
        opt.set_poses(P1)
        k, gated = opt.gate_edges(None, GATE)
        assert np.array_equal(gated, ogate) and k == int(ogate.sum())
        d, st = opt.optimize(iters)
        P = opt.get_poses()
        desc = opt.solver_description()
        fresh.set_graph(P1, *_reduced(g, ~ogate))
        df, sf = fresh.optimize(iters)
        Pf = fresh.get_poses()
    assert desc.startswith(path) and f"{k} edges inactive" in desc, desc
    assert st["seconds_setup"] == st0["seconds_setup"]   # (no set-up ran)
    assert d == iters and df == iters
    _close(st, sf, iters)
    _close(st, s2, iters)
    assert np.abs(P - Pf).max() <= 1e-5 and np.abs(P - P2).max() <= 1e-5
    if path == "pcg_amg":
        assert set(st["pcg_converged"][:iters]) == {1}


def _overlay_session():
    base, steps, g = synth.append_session(1500, 4500, 2, 12, seed=21, info_mode="full", phi=1.0)
    arrs = {k: np.concatenate([getattr(base, k)] + [s[k] for s in steps]) for k in ("ei", "ej", "meas", "info", "phi")}
    V = steps[-1]["V"]
    fixed = np.zeros(V, dtype=bool)
    fixed[: base.V] = base.fixed
    # a resident closure and the last appended closure (its id lies in the overlay's list)
    res = int(np.flatnonzero(base.phi >= 0)[7])
    last = arrs["ei"].size - 1
    assert arrs["phi"][last] >= 0 and last >= base.E
    return base, steps, g, arrs, V, fixed, np.array([res, last], dtype=np.int32)


def _grow(opt, base, steps, g, iters):
    """set_graph of the base, optimize, then the two incremental updates (optimising in between) -> the poses handed to the last update"""
    names = ("ei", "ej", "meas", "info", "phi")
    opt.set_graph(*base.arrays())
    assert opt.optimize(iters)[0] == iters
    P, E_res = opt.get_poses(), base.E
    cur = [getattr(base, k) for k in names]
    P0 = None
    for n, s in enumerate(steps):
        cur = [np.concatenate([a, s[k]]) for a, k in zip(cur, names)]
        P0 = np.empty((s["V"], 3))
        P0[: P.shape[0]] = P
        synth.chain_init(P0, g.meas[: g.V - 1], P.shape[0], s["V"] - 1)
        fixed = np.zeros(s["V"], dtype=bool)
        fixed[0] = True
        opt.update_graph(P0, fixed, *cur, E_res)
        assert "incremental overlay" in opt.solver_description(), opt.solver_description()
        if n + 1 < len(steps):
            assert opt.optimize(iters)[0] == iters
            P, E_res = opt.get_poses(), cur[0].size
    return P0


def test_deactivation_and_reactivation_under_a_resident_overlay():
    iters = 6
    base, steps, g, arrs, V, fixed, ids = _overlay_session()
    keep = np.ones(arrs["ei"].size, dtype=bool)
    keep[ids] = False
    full = [arrs[k] for k in ("ei", "ej", "meas", "info", "phi")]
    with capi.Optimizer(0, direct_rows=0) as opt, capi.Optimizer(0, direct_rows=0) as fresh:
        P0 = _grow(opt, base, steps, g, iters)
        assert np.array_equal(fixed, np.arange(V) == 0)
        # 4: explicit deactivation, one edge in the resident list and one in the overlay's
        opt.set_edge_information(ids, np.zeros((2, 6)))
        desc = opt.solver_description()
        assert "incremental overlay" in desc and "2 edges inactive" in desc, desc
        assert np.all(opt.edge_chi2()[ids] == 0.0)
        d, st = opt.optimize(iters)
        P = opt.get_poses()
        fresh.set_graph(P0, fixed, *[a[keep] for a in full])
        df, sf = fresh.optimize(iters)
        assert d == iters and df == iters
        _close(st, sf, iters)
        assert np.abs(P - fresh.get_poses()).max() <= 1e-5
        assert "incremental overlay" in opt.solver_description()
        # 5: the original rows bring the edges back: as a context that never deactivated anything
        opt.set_edge_information(ids, arrs["info"][ids])
        assert "inactive" not in opt.solver_description(), opt.solver_description()
        opt.set_poses(P0)
        d, st = opt.optimize(iters)
        P = opt.get_poses()
        fresh.set_graph(P0, fixed, *full)
        df, sf = fresh.optimize(iters)
        assert d == iters and df == iters
        _close(st, sf, iters)
        assert np.abs(P - fresh.get_poses()).max() <= 1e-5
        # ... and a changed non-zero row (the original x 4) is the general use
        info4 = arrs["info"].copy()
        info4[ids] *= 4.0
        opt.set_edge_information(ids, info4[ids])
        assert "inactive" not in opt.solver_description()
        opt.set_poses(P0)
        d, st = opt.optimize(iters)
        P = opt.get_poses()
        fresh.set_graph(P0, fixed, full[0], full[1], full[2], info4, full[4])
        df, sf = fresh.optimize(iters)
        assert d == iters and df == iters
        _close(st, sf, iters)
        assert np.abs(P - fresh.get_poses()).max() <= 1e-5


def _state(opt):
    b, diag, c2, rc2 = opt.linearize()
    return [opt.edge_chi2().view(np.uint64), b.view(np.uint64), diag.view(np.uint64), np.array([c2, rc2]).view(np.uint64)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_refusals_leave_the_device_untouched():
    g, bad, P1, oe2, ogate = _case(*PCG)
    # one extra pose hanging on a single closure, corrupted so that the gate wants it
    v = g.V
    z = synth._rel(g.truth[100:101], g.truth[101:102])[0] + (4.0, -4.0, 0.0)
    arr = (np.vstack([P1, P1[101]]), np.append(g.fixed, False), np.append(g.ei, 100).astype(np.int32), np.append(g.ej, v).astype(np.int32),
           np.vstack([g.meas, z]), np.vstack([g.info, g.info[bad[0]]]), np.append(g.phi, 1.0))
    hang = g.E
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(*arr)
        s0 = _state(opt)
        assert opt.edge_chi2()[hang] > GATE
        with pytest.raises(capi.SgoError, match="rc=-2") as ex:
            opt.gate_edges(None, GATE)
        assert f"vertex {v}" in str(ex.value) and f"vertex {v}" in opt.last_error()
        assert "inactive" not in opt.solver_description()
        assert _same(_state(opt), s0)
        with pytest.raises(capi.SgoError, match="rc=-2") as ex:
            opt.set_edge_information([5, hang], np.zeros((2, 6)))
        assert f"vertex {v}" in str(ex.value)
        assert _same(_state(opt), s0)
        with pytest.raises(capi.SgoError, match="rc=-2"):     # an id equal to E
            opt.set_edge_information([3, hang + 1], np.zeros((2, 6)))
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.gate_edges([3, hang + 1], GATE)
        assert _same(_state(opt), s0)
        row = np.array([g.info[3], g.info[4]])
        row[1, 4] = np.nan
        with pytest.raises(capi.SgoError, match="rc=-2"):     # a NaN entry
            opt.set_edge_information([3, 4], row)
        assert _same(_state(opt), s0)
        assert "inactive" not in opt.solver_description()
    with capi.Optimizer(0, direct_rows=0) as opt:              # the rank emulation of a multi-GPU context
        opt.debug_set_shard(2, 0)
        opt.set_graph(*g.arrays())
        e0 = opt.edge_chi2().view(np.uint64)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.gate_edges(None, GATE)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.set_edge_information([int(bad[0])], np.zeros((1, 6)))
        assert np.array_equal(opt.edge_chi2().view(np.uint64), e0)
        assert "inactive" not in opt.solver_description()


def test_the_first_solve_after_the_gate_refreshes_the_coarse_operators(capfd, monkeypatch):
    """SGO_AMG_LAG at its default.  Observed as test_gpu_lagged_refresh.py observes kept solves (the per-iteration lines of a verbose
    context and the call's note), and through the level-1 operator itself across a single-step linearisation."""
    import amg_reference as ar
    monkeypatch.delenv("SGO_AMG_LAG", raising=False)
    g, bad, P1, oe2, ogate = _case(*PCG)
    iters = 8
    with capi.Optimizer(0, direct_rows=0, verbose=1) as opt:
        opt.set_graph(*g.arrays())
        assert opt.optimize(iters)[0] == iters
        opt.set_poses(P1)
        opt.linearize()
        A_before = ar._fetch(opt, 1, "A_BLK", np.float64)
        k, _ = opt.gate_edges(None, GATE)
        assert k == int(ogate.sum())
        opt.linearize()
        A_after = ar._fetch(opt, 1, "A_BLK", np.float64)
        capfd.readouterr()
        d, st = opt.optimize(iters)
        desc = opt.solver_description()
    err = capfd.readouterr().err
    assert A_before is not None and A_after is not None and A_before.shape == A_after.shape   # (the aggregation is kept)
    assert not np.array_equal(A_before, A_after)
    assert d == iters
    first = [ln for ln in err.split("\n") if ln.startswith("[sgo] iteration= 0\t")]
    assert len(first) == 1 and "coarse operators kept" not in first[0], err[-2000:]
    if "kept the coarse operators" in desc:
        assert int(desc.split("last sgo_optimize_gn: ")[1].split(" of ")[0]) <= iters - 1
