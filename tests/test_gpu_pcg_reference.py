"""The device-resident PCG recurrence (k_finalize's start state, k_init_scalars, k_restart_scalars, k_warm_start, k_update_xr,
k_update_p, k_set_probe and the drivers start_pcg / pcg_iteration / run_pcg) against tests/pcg_reference.py, stage by stage, on
the cases of tests/pcg_cases.py.  States come from runs capped at consecutive iteration counts (sgo_debug_pcg_run) and are read
with sgo_debug_pcg_array; every case first asserts that two runs with the same cap leave bit-identical states.  Every case
prints one JSON line of its worst error / (U abs) per constant before it asserts, and every stage's figure when one fails.
GPU-machine time of the whole file on the MI355X: 13 s for its 23 tests (4.8 s the 530 000-pose chain, 1.8 s C2's whole solve with the
cycle at every cap, 1.0 s the 303 capped runs of n = 257, at most 0.9 s the others)."""
import json

import numpy as np
import pytest

import amg_reference as ar
import pcg_cases as pc
import pcg_reference as pr
from sparse_gslam_amd import capi

pytestmark = pytest.mark.gpu

BIG = 10 ** 6
CONST_OF = dict(pq_row="dot", rr_row="dot", rz_row="dot", bb_row="dot", zq_row="dot", pq="dot", rr="dot", rz="dot", bb="dot", x="axpy", r="axpy",
                p="axpy", z="z", z0="z", xs0="xs", alpha="div", beta="div", probe_rel="div", tol2="tol", drift="drift", q="product")
CONST_OF.update({"warm.xq_row": "dot", "warm.bx_row": "dot", "warm.q": "product", "warm.x0": "warm", "warm.r0": "warm"})


def _report(name, res, **extra):
    worst = {}
    for key, v in res.items():
        k = CONST_OF.get(key.split("@")[0])
        if k and np.isfinite(v):
            worst[k] = max(worst.get(k, 0.0), getattr(v, "raw", float(v)))
    print("PCGREF " + json.dumps(dict(case=name, **{k: float(f"{v:.3g}") for k, v in worst.items()}, **extra), default=str))
    bad = pr.failures(res)
    if bad:
        print("PCGREF every stage of " + name + ": " + json.dumps({k: float(f"{float(v):.4g}") for k, v in res.items()}))
    return bad


def _open(case, monkeypatch, lanczos=True, **opts):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if lanczos:
        monkeypatch.setenv("SGO_LANCZOS", "1")
    o = capi.Optimizer(0, solver=case.solver, direct_rows=0, **opts)
    o.set_graph(*case.arrays)
    o.linearize()
    return o


def _states(o, caps, **kw):
    out = {}
    for cap in caps:
        it = o.pcg_run(cap, **kw)
        out[cap] = pr.export_state(o)
        assert it == out[cap]["S"]["iter"] == out[cap]["H"]["iter"] <= max(cap, 0) or cap == 0
    return out


def _level0(o, case):
    """(omega, whether the cycle leaves xs0 as the update wrote it: the folded form only reads it, the unfolded one corrects it in place)"""
    if case.solver != pc.AMG:
        return None, True
    info = ar._fetch(o, 0, "INFO", np.float64)
    if info is None:
        return None, True
    L = dict(zip(ar.INFO, info))
    return float(L["omega"]), int(L["kind"]) != ar.UNFOLDED


def _cycle_figures(o, states):
    """stage 4: z of the loop's own cycle against the long-double cycle of the exported hierarchy on the exported r of every given
    state (normwise, in units of the case's fp64 rounding scale: amg_reference.K_CYCLE); a single dense level is its exact inverse"""
    lv = ar.export_hierarchy(o)
    order = lv[0]["row_order"].astype(np.int64)
    out = {}
    for cap, st in states.items():
        n = st["n"]
        ri, zi = np.empty((n, 3)), np.empty((n, 3))
        ri[order], zi[order] = st["r"], st["z"]
        zr, eps = ar.cycle_scale(lv, ri)
        out[cap] = ar.cycle_ratio(zi, zr, eps)
    return out


@pytest.mark.parametrize("name", list(pc.CASES))
def test_every_stage(name, monkeypatch):
    case = pc.case(name)
    whole = name != "bj_large_chain"             # (its whole solve: thousands of iterations of block-Jacobi on 530 000 poses)
    with _open(case, monkeypatch) as o:
        desc = o.solver_description()
        assert desc.startswith("pcg_amg" if case.solver == pc.AMG else "pcg_block_jacobi"), desc
        lin = pr.export_state(o)                                   # sgo_linearize leaves the start state of a cold solve
        caps, extra = case.caps, {}
        if whole:
            # stage 7: the whole solve, and then EVERY state of it: caps 0 .. N + 1, so that the drift bound is accumulated over all N
            # iterations and every iterate behind the third is held by every stage too
            N = o.pcg_run(BIG)
            full = pr.export_state(o)
            al, be = o.lanczos()                                   # (the entry point itself: the same record)
            assert al.size == be.size == N and (full["lanczos"] is None) == (N == 0)
            if N:
                assert np.array_equal(al, full["lanczos"][:, 0]) and np.array_equal(be, full["lanczos"][:, 1])
            x, it, relres = o.solve()
            assert it == N and not pr.same_bits(full, pr.export_state(o), skip=("args",)), "sgo_solve and an uncapped sgo_debug_pcg_run differ"
            assert full["S"]["stop"] == 1 and relres == pr.relres_of(full["H"]), (full["S"], relres)
            assert np.array_equal(x, full["x"])
            caps, extra["N"] = tuple(range(0, N + 2)), N
        st = _states(o, caps)
        again = _states(o, caps[-1:])
        assert not pr.same_bits(st[caps[-1]], again[caps[-1]]), "two runs with the same cap differ"
        # (everything a start writes; q, the iteration's rows and their counts are whatever the solves in between left)
        assert not pr.same_bits(lin, st[0], skip=("H", "M", "args", "q", "counts", "row.pq", "row.rr", "row.rz", "row.zq", "row.xq", "row.bx")), \
            "sgo_linearize's start state differs from a start alone"
        omega, kept = _level0(o, case)
        res = pr.check_sequence(st, pr.Operator(case.arrays), omega=omega, xs0_kept=kept, drift=whole)
        shown = caps[:4]
        extra.update(n=case.n, iters=[st[c]["S"]["iter"] for c in shown], stops=[st[c]["S"]["stop"] for c in shown], counts=st[caps[-1]]["counts"])
        last = st[caps[-1]]
        if whole:
            res.update({k + "@N": v for k, v in pr.check_records(full).items()})
            res["uncapped=capped@N"] = pr.check_frozen(st[N], full)["frozen"]     # the uncapped solve is the run capped at N, bit for bit
            if N >= 1:   # it stopped at the FIRST passing iteration: one iteration less has not converged; its drift is held at the end
                s = st[N - 1]["S"]
                assert s["iter"] == N - 1 and s["stop"] == (2 if N > 1 else 0) and s["rr"] > s["tol2"] * s["bb"], s
                assert f"drift@{N}" in res and f"frozen@{N + 1}" in res, sorted(res)[:40]
                extra["drift_at_N"] = float(f"{res[f'drift@{N}'].raw:.3g}")
        # stage 4: the cycle inside the loop at every cap against amg_reference's stage 9 (V-cycle hierarchies and the dense single
        # level: K_CYCLE; the K-cycle, whose flexible-CG steps are nonlinear in r: K_KCYCLE)
        if case.solver == pc.AMG and "SGO_AMG_KDEPTH" not in case.env:
            cyc = _cycle_figures(o, {c: st[c] for c in caps if st[c]["S"]["iter"] == c})
            assert len(cyc) >= min(len(caps) - 1, 2)
            res.update({f"cycle@{c}": v / ar.K_CYCLE for c, v in cyc.items()})
            extra["cycle"] = max(cyc.values())
            o.pcg_run(caps[-1])
            extra["cycle_bitwise_with_sgo_precondition"] = bool(np.array_equal(o.precondition(last["r"]), last["z"]))
        elif case.solver == pc.AMG:
            kd = dict(zip(ar.INFO, ar._fetch(o, 0, "INFO", np.float64)))["kdepth"]
            assert kd > 0, kd
            cyc = _cycle_figures(o, {c: st[c] for c in caps if st[c]["S"]["iter"] == c})
            assert len(cyc) >= min(len(caps) - 1, 2)
            res.update({f"cycle@{c}": v / ar.K_KCYCLE for c, v in cyc.items()})
            extra["cycle"], extra["kdepth"] = max(cyc.values()), int(kd)
            o.pcg_run(caps[-1])
            extra["cycle_bitwise_with_sgo_precondition"] = bool(np.array_equal(o.precondition(last["r"]), last["z"]))
            assert extra["cycle_bitwise_with_sgo_precondition"], "the K-cycle in the loop and sgo_precondition differ on the same r"
    bad = _report(name, res, **extra)
    assert not bad, bad
    assert len(res) >= 20 or name == "bj_lattice_b0", sorted(res)
    # the shape the case exists for
    if "grid" in case.expect:
        assert last["counts"]["n_rr"] == case.expect["grid"] == pr.MAX_GRID and case.n > pr.BLOCK * pr.MAX_GRID, last["counts"]
        assert last["counts"]["start_bb"] == pr.MAX_GRID
    if case.expect.get("zq"):
        assert last["rows"]["zq"].size > 0 and "zq_row@1" in res
    if case.solver == pc.AMG:
        assert last["counts"]["n_zq"] == last["counts"]["n_rz"] > 0          # the multigrid's beta is the flexible one
    else:
        assert last["counts"]["n_zq"] == 0 and (any(k.startswith("z@") for k in res) or name == "bj_lattice_b0")
    if "stop" in case.expect:
        assert not st[0]["b"].any() and st[0]["S"]["stop"] == case.expect["stop"] and st[1]["S"]["iter"] == 0, st[1]["S"]
        assert "frozen@1" in res
    if "iters" in case.expect and name != "bj_lattice_b0":
        assert extra["N"] == case.expect["iters"] and st[1]["S"]["stop"] == 1 and "frozen@2" in res, (extra, desc)
    if name.startswith("bj_n"):
        g = pr.grid_for(case.n)
        assert last["counts"]["n_rr"] == g == st[0]["counts"]["start_bb"] == 8


MODES = dict(graph=dict(use_graph=1), plain_chunk1=dict(use_graph=0, pcg_chunk=1), profile=dict(profile=1))


@pytest.mark.parametrize("name", ["bj_n257", "amg_c2"])
def test_launch_modes_leave_the_same_bits(name, monkeypatch):
    """An odd cap inside the 2-iteration replay, speculative replays past the stop, plain launches one iteration at a time and the
    profiled launches: every exported array and scalar bitwise equal."""
    case = pc.case(name)
    got = {}
    for mode, opts in MODES.items():
        with _open(case, monkeypatch, lanczos=False, **opts) as o:
            got[mode] = _states(o, (1, 2, 3, 6))
    for cap in (1, 2, 3, 6):
        assert got["graph"][cap]["S"]["iter"] == cap and got["graph"][cap]["S"]["stop"] == 2, got["graph"][cap]["S"]
        for mode in ("plain_chunk1", "profile"):
            diff = pr.same_bits(got["graph"][cap], got[mode][cap])
            assert not diff, (name, cap, mode, diff)


def test_absolute_tolerance_rule(monkeypatch):
    """bb_ref below, equal to and above b.b, and so far above that the cap holds"""
    case = pc.case("bj_n86")
    op = pr.Operator(case.arrays)
    with _open(case, monkeypatch) as o:
        s0 = pr.export_state(o)
        bb, tol = s0["S"]["bb"], s0["args"]["tol"]
        opts = capi.default_opts()
        assert 0.0 < tol <= opts.pcg_tol and s0["S"]["tol2"] == tol * tol and s0["args"]["bb_ref"] == 0.0
        cap = max(opts.pcg_tol_cap, tol)
        want = {0.5: tol * tol, 1.0: tol * tol, 4.0: (tol * tol) * (4.0 * bb / bb), 1e30: cap * cap}
        for f, t2 in want.items():
            st = _states(o, (0, 1), bb_ref=f * bb)
            res = pr.check_sequence(st, op)
            assert not _report(f"bb_ref_{f}", res), pr.failures(res)
            assert st[0]["args"] == dict(tol=tol, tol_cap=cap, bb_ref=f * bb, maxit=float(opts.pcg_maxit)), st[0]["args"]
            assert st[0]["S"]["tol2"] == st[1]["S"]["tol2"] and abs(st[0]["S"]["tol2"] - t2) <= 4 * pr.U * t2, (f, st[0]["S"]["tol2"], t2)
        N = o.pcg_run(BIG, bb_ref=1e30 * bb)                       # the looser target ends the solve earlier, at its first passing iteration
        s = pr.export_state(o)["S"]
        assert s["stop"] == 1 and s["rr"] <= cap * cap * bb and N < o.pcg_run(BIG)
        o.pcg_run(N - 1, bb_ref=1e30 * bb)
        s = pr.export_state(o)["S"]
        assert s["rr"] > s["tol2"] * s["bb"] and s["stop"] == 2
        assert pr.export_state(o)["args"]["bb_ref"] == 1e30 * bb and o.pcg_run(0) == 0 and pr.export_state(o)["args"]["bb_ref"] == 0.0   # restored


def test_progress_probe(monkeypatch):
    case = pc.case("amg_c2")
    op = pr.Operator(case.arrays)
    with _open(case, monkeypatch) as o:
        omega, kept = _level0(o, case)
        N = o.pcg_run(BIG, probe_k=3)
        s = pr.export_state(o)["S"]
        rel = s["probe_rel"]
        assert N > 4 and s["stop"] == 1 and s["probe_k"] == 3 and 0.0 < rel < 1.0, s
        for side, pm in (("above", rel * (1 + 1e-9)), ("below", rel * (1 - 1e-9))):
            st = _states(o, (0, 1, 2, 3, 4), probe_k=3, probe_max=pm)
            res = pr.check_sequence(st, op, omega=omega, xs0_kept=kept, drift=False)
            assert not _report("probe_" + side, res, probe_rel=rel, stops=[st[c]["S"]["stop"] for c in sorted(st)]), pr.failures(res)
            assert st[4]["S"]["probe_max"] == pm and abs(st[3]["S"]["probe_rel"] - rel) <= 1e-12 * rel
            if side == "above":
                assert st[4]["S"]["stop"] == 2 and st[4]["S"]["iter"] == 4
            else:
                assert st[4]["S"]["stop"] == 4 and st[4]["S"]["iter"] == 3 and "frozen@4" not in res   # (cap 3 stops with 2, cap 4 with 4)
                assert pr.stop_rule(st[4]["S"]) == 4
                assert not pr.same_bits(st[3], st[4], skip=("S", "H", "M", "args")), "the probe's stop moved an array"
        assert o.pcg_run(BIG) == N and pr.export_state(o)["S"]["probe_k"] == 0                  # restored: no probe armed


def test_negative_information_breaks_down(monkeypatch):
    """p.Hp <= 0 (stop 3): sgo_solve reports it, x stays finite, nothing moves behind the flag"""
    arrays = pc.negative_information()
    case = pc.Case("negative_information", arrays, caps=(0, 1, 2))
    with _open(case, monkeypatch) as o:
        with pytest.raises(capi.SgoError, match="breakdown"):
            o.solve()
        s = pr.export_state(o)
        assert s["S"]["stop"] == 3 and s["S"]["iter"] == 0 and s["S"]["pq"] < 0.0 and np.isfinite(s["x"]).all() and not s["x"].any(), s["S"]
        st = _states(o, case.caps)
        res = pr.check_sequence(st, pr.Operator(arrays))
        assert not _report(case.name, res), pr.failures(res)
        assert "breakdown@1" in res and "frozen@2" in res


def test_warm_start(monkeypatch):
    """x_prev = x*, x* / 2 (gamma ~ 1, 2) and the three fall-backs to the cold start: x_prev = 0, -x*, x* / 8 (gamma = 8 > 4)"""
    case = pc.case("amg_c2")
    op = pr.Operator(case.arrays)
    with _open(case, monkeypatch) as o:
        omega, kept = _level0(o, case)
        xstar, Ncold, _ = o.solve()
        cold = pr.export_state(o)
        assert cold["S"]["stop"] == 1 and Ncold > 2
        for f, gamma in ((1.0, 1.0), (0.5, 2.0), (0.0, 0.0), (-1.0, 0.0), (0.125, 0.0)):
            st = _states(o, (0, 1, 2), x_prev=f * xstar)
            res = pr.check_sequence(st, op, omega=omega, xs0_kept=kept, x_prev=f * xstar, drift=False)
            g = st[0]["gamma_ref"]
            N = o.pcg_run(BIG, x_prev=f * xstar)
            assert not _report(f"warm_{f}", res, gamma=g, N=N, Ncold=Ncold, counts=st[0]["counts"]), pr.failures(res)
            assert st[0]["counts"]["n_xq"] > 0 and st[0]["counts"]["n_bx"] > 0
            if gamma:
                assert abs(g - gamma) <= 1e-6 * gamma and "warm.x0@0" in res and "warm.r0@0" in res, g
            else:
                assert g == 0.0 and not st[0]["x"].any() and np.array_equal(st[0]["r"], st[0]["b"]) and "r0=b@0" in res
                assert abs(N - Ncold) <= 1                           # the cold start's solve again
            if f == 1.0:
                assert N <= 1 and st[2]["S"]["stop"] == 1, (N, st[2]["S"])
        o.pcg_run(0)
        assert pr.export_state(o)["counts"]["n_xq"] == 0            # restored: the next start is cold


def test_warm_start_keeps_a_stop_the_start_has_set(monkeypatch):
    """b == 0 under the multigrid with a non-zero x_prev: k_init_scalars sets stop 1, k_restart_scalars(keep_stop) leaves it, gamma
    = 0 / (x_prev . H x_prev) falls back to the cold start, and nothing moves behind the flag"""
    case = pc.Case("amg_lattice_b0_warm", pc.lattice(), solver=pc.AMG, caps=(0, 1))
    xp = np.random.default_rng(3).standard_normal((case.n, 3))
    with _open(case, monkeypatch) as o:
        omega, kept = _level0(o, case)
        st = _states(o, case.caps, x_prev=xp)
        res = pr.check_sequence(st, pr.Operator(case.arrays), omega=omega, xs0_kept=kept, x_prev=xp, drift=False)
        assert not _report(case.name, res, counts=st[0]["counts"], S=st[1]["S"]), pr.failures(res)
        assert not st[0]["b"].any() and st[0]["counts"]["n_xq"] > 0 and st[0]["gamma_ref"] == 0.0
        assert st[0]["S"]["stop"] == 1 == st[1]["S"]["stop"] and st[1]["S"]["iter"] == 0 and "frozen@1" in res and "stop@0" in res
        assert not st[1]["x"].any() and o.pcg_run(BIG, x_prev=xp) == 0


def test_hooks_refuse_what_they_cannot_serve(monkeypatch):
    case = pc.case("bj_n2")
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    with capi.Optimizer(0, solver=case.solver, direct_rows=0) as o:
        o.set_graph(*case.arrays)
        with pytest.raises(capi.SgoError, match="sgo_linearize"):
            o.pcg_array("X")
        with pytest.raises(capi.SgoError, match="sgo_linearize"):
            o.pcg_run(1)
        o.linearize()
        with pytest.raises(capi.SgoError, match="hierarchy"):     # block-Jacobi: no warm start, no probe
            o.pcg_run(1, x_prev=np.zeros((2, 3)))
        with pytest.raises(capi.SgoError, match="hierarchy"):
            o.pcg_run(1, probe_k=3)
        assert o.pcg_array("XS0") is None and o.pcg_array("ZPARTS") is None and o.pcg_array("LANCZOS") is None
        assert o.pcg_array("SCALARS").dtype.itemsize == 104
        with pytest.raises(capi.SgoError, match="must be >= 0"):   # bad arguments name themselves
            o.pcg_run(-1)
        with pytest.raises(capi.SgoError, match="must be >= 0"):
            o.pcg_run(1, bb_ref=float("nan"))
        assert capi.lib().sgo_debug_pcg_array(o._h, capi.PCG_ARRAYS["X"][0], None, 8) == -2 and "capacity" in o.last_error()
        assert capi.lib().sgo_debug_pcg_array(o._h, 99, None, 0) == -2 and "unknown array" in o.last_error()


def test_hooks_refuse_a_sharded_context(monkeypatch):
    with capi.Optimizer(0, solver=capi.SOLVER_PCG_BJ) as o:      # (10 000 rows: enough level-0 work units for two ranks)
        o.debug_set_shard(2, 0)
        o.set_graph(*pc.c2())
        o.linearize()
        with pytest.raises(capi.SgoError, match="multi-GPU"):
            o.pcg_run(1)
        with pytest.raises(capi.SgoError, match="multi-GPU"):
            o.pcg_array("X")


def test_hooks_refuse_an_active_overlay():
    import overlay_cases as oc
    p = oc.plan("tile_k1")
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*p.base.arrays())
        d, _ = o.optimize(2)
        assert d == 2, o.last_error()
        u = p.updates[0]
        V, fixed, ei, ej, meas, info, phi = oc.arrays_upto(p, 1)
        o.update_graph(oc.start_poses(p, o.get_poses(), u["V"]), fixed, ei, ej, meas, info, phi, p.base.E)
        assert "incremental overlay" in o.solver_description()
        with pytest.raises(capi.SgoError, match="overlay"):
            o.pcg_run(1)
        with pytest.raises(capi.SgoError, match="overlay"):
            o.pcg_array("X")
