"""sgo_optimize_gn_hypotheses on the multifrontal path with a workspace granted (sgo_set_hypotheses_workspace; DESIGN.md section
5i-2): chains of hypotheses share every launch of one sgo_optimize_gn_until, each on its own copy of what the factorisation writes.
The bar is the sequential route's: everything a hypothesis returns but edge_chi2 is, bit for bit, the host loop's turn on a twin
context -- whatever the chunk --, a failing hypothesis fails alone, and the batched route writes nothing of the resident solver.
Without a grant nothing changes.  The oracle (host_loop, check_against_loop) is tests/test_gpu_hypotheses.py's."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from sparse_gslam_amd import capi, synth
from test_gpu_hypotheses import (CPP, DIRECT, LIBDIR, MFRONT, PCG, ROOT, bits, check_against_loop, graph, host_loop, masks7,
                                 open_ctx, rule_stop, same_bits, sentinel_outputs, untouched)

pytestmark = pytest.mark.gpu

PATH = "multifrontal_cholesky"
OUTPUTS = ("hist", "poses", "edge_chi2", "chi2", "robust_chi2", "iters_done", "stop_reason")
FACTOR = ("ARENA", "ELEM", "X", "INVD", "YINV", "FLAGS")


def batched_ctx(g, hypotheses, iters=20, slack=0, **opts):
    """a context on g whose grant holds `hypotheses` copies (+ slack bytes) for calls of `iters` iterations with edge_chi2"""
    opt = open_ctx(g, PATH, **opts)
    per = opt.hypotheses_bytes(iters, True)
    assert per > 0
    opt.set_hypotheses_workspace(hypotheses * per + slack)
    return opt


def same_outputs(A, B):
    return all(np.array_equal(A[k], B[k], equal_nan=True) for k in OUTPUTS)


@functools.lru_cache(maxsize=None)
def mf_loop(tol):
    g = graph(MFRONT)
    with open_ctx(g, PATH) as twin:
        return host_loop(twin, g.info, masks7(g), 20, tol)


@functools.lru_cache(maxsize=None)
def mf_stopping_tolerance():
    """as test_gpu_hypotheses.stopping_tolerance, from this graph's loop: 1e-6 if it makes two of the seven hypotheses stop at
    different iterations; otherwise a tolerance between two adjacent gains of the loop's own full histories that does"""
    full = mf_loop(0.0)
    assert all(l["done"] == 20 for l in full)
    gains = sorted({(l["robust"][i - 1] - l["robust"][i]) / l["robust"][i] for l in full for i in range(2, 20)})
    gains = [x for x in gains if x > 0.0]
    for tol in [1e-6] + [math.sqrt(a * b) for a, b in zip(gains, gains[1:])]:
        stops = {rule_stop(l["robust"], tol, 20) for l in full}
        if len(stops) >= 2 and min(stops) < 20:
            return tol
    raise AssertionError(f"no tolerance separates the hypotheses' stop iterations: {gains}")


@functools.lru_cache(maxsize=None)
def mf_batch(tol):
    """the seven hypotheses in ONE chain"""
    g = graph(MFRONT)
    with batched_ctx(g, 7) as opt:
        return opt.optimize_hypotheses(masks7(g), 20, tol)


def test_the_plan_has_merge_levels():
    g = graph(MFRONT)
    plan = capi.mfront_plan(g.poses, g.fixed, g.ei, g.ej)
    assert plan["qualifies"] and plan["levels"] - 1 >= 2, plan           # height >= 2: k_mf_merge runs, and on more than one level


def test_default_route_is_sequential():
    g = graph(MFRONT)
    M = masks7(g)[[0, 1, 4]]
    with open_ctx(g, PATH) as opt:
        per = opt.hypotheses_bytes(2, True)
        assert 0 < opt.hypotheses_bytes(2, False) < per
        assert opt.hypotheses_bytes(20, True) >= per
        assert opt.optimize_hypotheses(M, 2, 0.0)["route"] == capi.HYP_SEQUENTIAL          # no grant
        opt.set_hypotheses_workspace(2 * per - 1)
        assert capi.hypotheses_chunk(per, 2 * per - 1, 3) == 0
        assert opt.optimize_hypotheses(M, 2, 0.0)["route"] == capi.HYP_SEQUENTIAL          # a grant below two copies
        assert opt.hypotheses_workspace_bytes() == 0                                         # the sequential route takes no workspace
        opt.set_hypotheses_workspace(2 * per)
        assert opt.optimize_hypotheses(M, 2, 0.0)["route"] == capi.HYP_BATCHED
        opt.set_hypotheses_workspace(0)
        assert opt.optimize_hypotheses(M, 2, 0.0)["route"] == capi.HYP_SEQUENTIAL          # ... and taken back


def test_the_grant_bounds_the_allocation():
    """The workspace is chunk x per-hypothesis bytes exactly: a grant that the chain nearly fills is not exceeded by any head-room,
    and growing for a longer chain stays within the grant too."""
    g = graph(MFRONT)
    M = masks7(g)[[0, 1, 4]]
    with open_ctx(g, PATH) as opt:
        per = opt.hypotheses_bytes(2, True)
        grant = 2 * per + per // 20                                      # two copies fill 97 % of it
        opt.set_hypotheses_workspace(grant)
        assert opt.optimize_hypotheses(M, 2, 0.0)["route"] == capi.HYP_BATCHED
        assert opt.hypotheses_workspace_bytes() == 2 * per <= grant
        opt.set_hypotheses_workspace(3 * per)                            # a larger grant, filled to the byte
        assert opt.optimize_hypotheses(M, 2, 0.0)["route"] == capi.HYP_BATCHED
        assert opt.hypotheses_workspace_bytes() == 3 * per
        opt.set_hypotheses_workspace(grant)                              # a workspace already held is reused, not shrunk
        assert opt.optimize_hypotheses(M, 2, 0.0)["route"] == capi.HYP_BATCHED
        assert opt.hypotheses_workspace_bytes() == 3 * per


@pytest.mark.parametrize("stopping", [False, True])
def test_batch_equals_loop_bit_for_bit(stopping):
    tol = mf_stopping_tolerance() if stopping else 0.0
    L = mf_loop(tol)
    R = mf_batch(tol)
    assert R["route"] == capi.HYP_BATCHED
    print(f"gain_tol {tol!r}: the loop's hypotheses end after {[l['done'] for l in L]} updates")
    if stopping:
        assert len({l["done"] for l in L}) >= 2 and any(l["why"] == capi.STOP_GAIN for l in L), [l["done"] for l in L]
    else:
        assert all(l["done"] == 20 and l["why"] == capi.STOP_MAX_ITERS for l in L)
    check_against_loop(R, L, 20)
    assert not same_bits(R["poses"][0], R["poses"][4])                 # (the masks do change the answer)


@pytest.mark.parametrize("stopping", [False, True])
def test_chunking_changes_no_bit(stopping):
    g = graph(MFRONT)
    tol = mf_stopping_tolerance() if stopping else 0.0
    one = mf_batch(tol)
    with batched_ctx(g, 3, slack=100, profile=1) as opt:
        per = opt.hypotheses_bytes(20, True)
        assert capi.hypotheses_chunk(per, 3 * per + 100, 7) == 3
        opt.profile_reset()
        R = opt.optimize_hypotheses(masks7(g), 20, tol)
        chains = opt.kernel_profile()["mfront_batch"]["launches"]
        assert opt.hypotheses_workspace_bytes() == 3 * per               # within the grant: no head-room on top of it
    assert R["route"] == capi.HYP_BATCHED and chains == 3                # 3 + 3 + 1
    assert same_outputs(R, one)


def test_forty_hypotheses_and_no_aliasing():
    g = graph(MFRONT)
    two = masks7(g)[[5, 6]]
    with open_ctx(g, PATH) as twin:
        L = host_loop(twin, g.info, two, 6, 0.0)
    with batched_ctx(g, 40, iters=6) as opt:
        per = opt.hypotheses_bytes(6, True)
        small = opt.optimize_hypotheses(two, 6, 0.0)                   # the context's workspace grows for the next call ...
        assert opt.hypotheses_workspace_bytes() == 2 * per
        R = opt.optimize_hypotheses(np.tile(two, (20, 1)), 6, 0.0)
        assert opt.hypotheses_workspace_bytes() == 40 * per
        again = opt.optimize_hypotheses(two, 6, 0.0)                   # ... and is reused by this one
        assert opt.hypotheses_workspace_bytes() == 40 * per
    assert small["route"] == R["route"] == again["route"] == capi.HYP_BATCHED and R["poses"].shape[0] == 40
    for key in OUTPUTS:
        for par in (0, 1):
            a = R[key][par::2]
            assert all(np.array_equal(a[0], x, equal_nan=True) for x in a), (key, par)
        assert np.array_equal(small[key], R[key][:2], equal_nan=True) and np.array_equal(again[key], R[key][:2], equal_nan=True), key
    assert not same_bits(R["poses"][0], R["poses"][1]) and not same_bits(R["edge_chi2"][0], R["edge_chi2"][1])
    check_against_loop({k: (v[:2] if k != "route" else v) for k, v in R.items()}, L, 6)


def test_own_starting_poses():
    g = graph(MFRONT)
    M = masks7(g)[[0, 1, 4, 6]]
    P0 = np.repeat(g.poses[None], 4, axis=0)
    free = ~np.asarray(g.fixed, bool)
    for b in range(4):
        P0[b, free] += 1e-2 * np.random.default_rng(b).standard_normal((int(free.sum()), 3))
    with open_ctx(g, PATH) as twin:
        L = host_loop(twin, g.info, M, 8, 0.0, P0)
    with batched_ctx(g, 3, iters=8) as opt:                            # chains of 3 + 1: the second chain's starts are its own
        R = opt.optimize_hypotheses(M, 8, 0.0, poses0=P0)
        assert same_bits(opt.get_poses(), g.poses)
    assert R["route"] == capi.HYP_BATCHED
    check_against_loop(R, L, 8)
    assert same_bits(R["poses"][:, ~free], P0[:, ~free]) and same_bits(P0[0, ~free], g.poses[~free])   # the fixed pose comes back unchanged
    assert not same_bits(L[0]["chi2"][:1], mf_loop(0.0)[0]["chi2"][:1])                            # (the starts were used)


def test_other_kernel_kinds():
    g = graph(MFRONT)
    clo = np.arange(g.V - 1, g.E, dtype=np.int32)
    kinds = np.array([capi.KERNEL_HUBER, capi.KERNEL_CAUCHY, capi.KERNEL_TUKEY], dtype=np.int32)[(3 * np.arange(clo.size)) // clo.size]
    delta = np.where(kinds == capi.KERNEL_TUKEY, 4.0, 1.5)
    M = masks7(g)[[0, 2, 5]]
    with open_ctx(g, PATH) as twin:
        twin.set_robust_kernels(clo, kinds, delta)
        L = host_loop(twin, g.info, M, 20, 0.0)
    with batched_ctx(g, 3) as opt:
        opt.set_robust_kernels(clo, kinds, delta)
        R = opt.optimize_hypotheses(M, 20, 0.0)
    assert R["route"] == capi.HYP_BATCHED
    check_against_loop(R, L, 20)
    assert not same_bits(L[0]["robust"], mf_loop(0.0)[0]["robust"])      # (the kernels were used)


def test_a_failing_hypothesis_fails_alone():
    """One closure's information negated, as in test_gpu_hypotheses.test_a_failing_hypothesis_stays_alone: the Hessian with it is
    indefinite (a pivot test fails, a clean failure flag), without it the graph optimises as usual.  The failing hypothesis sits
    between two good ones of the same chain."""
    g = graph(MFRONT)
    info = g.info.copy()
    c = g.E - 1
    info[c, [0, 3, 5]] *= -1.0
    M = np.zeros((3, g.E), dtype=np.uint8)
    M[0, c] = 1
    M[2, [c, g.V - 1]] = 1
    args = (g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)
    with capi.Optimizer(0) as twin:
        twin.set_graph(*args)
        assert twin.solver_description().startswith(PATH)
        L = host_loop(twin, info, M, 20, 0.0)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*args)
        assert opt.solver_description().startswith(PATH)
        opt.set_hypotheses_workspace(3 * opt.hypotheses_bytes(20, True))
        R = opt.optimize_hypotheses(M, 20, 0.0)
    assert R["route"] == capi.HYP_BATCHED
    print("the loop:", [(l["done"], l["why"]) for l in L])
    assert L[1]["why"] == capi.STOP_FAILED and R["stop_reason"][1] == capi.STOP_FAILED and R["iters_done"][1] == L[1]["done"]
    for b in (0, 2):
        assert R["stop_reason"][b] == capi.STOP_MAX_ITERS and R["iters_done"][b] == 20
    check_against_loop(R, L, 20)


def test_edge_chi2_is_formed_with_the_resident_information():
    from oracle import c_oracle
    g = graph(MFRONT)
    M = masks7(g)
    held = np.array([g.V + 3, g.V + 7], dtype=np.int32)                  # two closures the context itself holds inactive
    for tol, inactive in ((0.0, False), (mf_stopping_tolerance(), False), (0.0, True)):
        if inactive:
            with batched_ctx(g, 7) as opt:
                opt.set_edge_information(held, np.zeros((2, 6)))
                R = opt.optimize_hypotheses(M, 20, tol)
            assert R["route"] == capi.HYP_BATCHED
            info = g.info.copy()
            info[held] = 0.0
        else:
            R, info = mf_batch(tol), g.info
        for b in range(M.shape[0]):
            P = R["poses"][b]
            _, _, _, oe2, _, _ = c_oracle.edges(P[g.ei], P[g.ej], g.meas, info, g.phi)
            err = np.abs(R["edge_chi2"][b] - oe2).max()
            assert err <= 1e-11 * max(1.0, np.abs(oe2).max()), (b, err)
            active = (M[b] == 0)
            s = R["edge_chi2"][b][active].sum()
            assert abs(s - R["chi2"][b]) <= g.E * 2.0 ** -53 * R["chi2"][b], (b, s, R["chi2"][b])
            if M[b].any():
                off = R["edge_chi2"][b][M[b] != 0]
                if inactive:
                    off = R["edge_chi2"][b][(M[b] != 0) & ~np.isin(np.arange(g.E), held)]
                assert (off > 0.0).all() and off.size >= 1                   # a switched-off edge reports its resident cost
            if inactive:
                assert (R["edge_chi2"][b][held] == 0.0).all()                # a context-inactive edge reports 0


def test_nothing_is_left_behind():
    """The batched route writes nothing of the resident solver (unlike the sequential one, whose factor is the last hypothesis').
    The information rows have no read-back of their own: chi2 and edge_chi2 at the unchanged poses are their witnesses."""
    g = graph(MFRONT)
    M = np.zeros((3, g.E), dtype=np.uint8)
    M[1, g.V - 1] = 1
    M[2, g.V - 1:] = 1

    def session(call):
        with batched_ctx(g, 3, iters=5) as opt:
            assert opt.optimize(3)[0] == 3

            def state():
                s = dict(poses=opt.get_poses(), chi2=np.array(opt.chi2()), edge_chi2=opt.edge_chi2(), desc=opt.solver_description(),
                         setup=opt.optimize(0)[1]["seconds_setup"])
                s.update(opt.mfront_arrays(FACTOR))
                return s

            if call:
                before = state()
                R = opt.optimize_hypotheses(M, 5, 0.0)
                assert R["route"] == capi.HYP_BATCHED
                after = state()
                for k in before:
                    if isinstance(before[k], np.ndarray) and before[k].dtype == np.float64:
                        assert same_bits(after[k], before[k]), k
                    else:
                        assert np.array_equal(after[k], before[k]), (k, before[k], after[k])
                assert not same_bits(R["poses"][0], before["poses"])      # (the hypotheses did move)
            d, st = opt.optimize(20)
            return d, st, opt.get_poses(), opt.mfront_arrays(FACTOR)

    dA, stA, PA, FA = session(True)
    dB, stB, PB, FB = session(False)
    assert dA == dB == 20
    assert same_bits(stA["chi2"], stB["chi2"]) and same_bits(stA["robust_chi2"], stB["robust_chi2"])
    assert same_bits(PA, PB)
    for k in FACTOR:
        assert np.array_equal(FA[k].view(np.uint8), FB[k].view(np.uint8)), k


def test_the_setter():
    g = graph(MFRONT)
    with open_ctx(g, PATH) as opt:
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.set_hypotheses_workspace(-1)
        assert "negative" in opt.last_error()
        per = opt.hypotheses_bytes(2, True)
        opt.set_hypotheses_workspace(2 * per)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.set_hypotheses_workspace(-(2 ** 40))                    # a refused value changes nothing
        opt.set_graph(*g.arrays())                                       # the grant survives a second set-up
        assert opt.solver_description().startswith(PATH)
        R = opt.optimize_hypotheses(masks7(g)[[0, 4]], 2, 0.0)
        assert R["route"] == capi.HYP_BATCHED
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.hypotheses_bytes(capi.SGO_MAX_ITERS + 1, True)
    gd = graph(DIRECT)
    with open_ctx(gd, "direct_ldlt") as opt:
        assert opt.hypotheses_bytes(2, True) == 0
        opt.set_hypotheses_workspace(2 ** 30)
        assert opt.optimize_hypotheses(masks7(gd)[[0, 4]], 2, 0.0)["route"] == capi.HYP_BATCHED
    gp = graph(PCG)
    with open_ctx(gp, "pcg_amg", direct_rows=0) as opt:
        assert opt.hypotheses_bytes(2, True) == 0
        opt.set_hypotheses_workspace(2 ** 30)
        M = np.zeros((2, gp.E), dtype=np.uint8)
        M[1, gp.V - 1 + 5] = 1
        assert opt.optimize_hypotheses(M, 1, 0.0)["route"] == capi.HYP_SEQUENTIAL


def test_refusals_write_nothing_with_a_grant():
    g = graph(MFRONT)
    B = 2
    with batched_ctx(g, B) as opt:
        p0 = opt.get_poses()
        v = 300
        M = np.zeros((B, g.E), dtype=np.uint8)
        M[1, (g.ei == v) | (g.ej == v)] = 1                             # hypothesis 1 takes every edge of pose 300 away
        out = sentinel_outputs(B, g.V, g.E, 20)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.optimize_hypotheses(M, 20, 0.0, out=out)
        assert "hypothesis 1" in opt.last_error() and f"vertex {v}" in opt.last_error(), opt.last_error()
        assert untouched(out) and same_bits(opt.get_poses(), p0)
        M[:] = 0
        u8, d = C.POINTER(C.c_uint8), C.POINTER(C.c_double)              # a negative count, a NULL edge_off: the binding cannot say them
        tail = (None, out["res"], out["hist"].ctypes.data_as(d), out["poses"].ctypes.data_as(d), out["edge_chi2"].ctypes.data_as(d))
        assert capi.lib().sgo_optimize_gn_hypotheses(opt._h, -1, 20, 0.0, M.ctypes.data_as(u8), *tail) == -2
        assert capi.lib().sgo_optimize_gn_hypotheses(opt._h, B, 20, 0.0, None, *tail) == -2
        assert untouched(out) and same_bits(opt.get_poses(), p0) and opt.hypotheses_workspace_bytes() == 0
        P0 = np.repeat(p0[None], B, axis=0)
        P0[1, 17, 2] = math.nan
        for kw in (dict(poses0=P0), dict(gain_tol=math.inf), dict(max_iters=-1), dict(max_iters=capi.SGO_MAX_ITERS + 1)):
            it = kw.get("max_iters", 20)
            o2 = sentinel_outputs(B, g.V, g.E, it)
            with pytest.raises(capi.SgoError, match="rc=-2"):
                opt.optimize_hypotheses(M, **{"max_iters": 20, "gain_tol": 0.0, **kw}, out=o2)
            assert untouched(o2) and same_bits(opt.get_poses(), p0), kw
        R = opt.optimize_hypotheses(np.zeros((0, g.E), dtype=np.uint8), 20, 0.0)   # B == 0: nothing to do
        assert R["route"] == capi.HYP_BATCHED and R["poses"].shape[0] == 0
    with capi.Optimizer(0, direct_rows=0) as opt:                       # the rank emulation of a multi-GPU context
        opt.debug_set_shard(2, 0)
        opt.set_hypotheses_workspace(2 ** 30)
        opt.set_graph(*g.arrays())
        assert opt.hypotheses_bytes(20, True) == 0
        p0 = opt.get_poses()
        out = sentinel_outputs(B, g.V, g.E, 20)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.optimize_hypotheses(M, 20, 0.0, out=out)
        assert "multi-GPU" in opt.last_error()
        assert untouched(out) and same_bits(opt.get_poses(), p0)


def test_an_active_overlay_is_refused_with_a_grant():
    """test_gpu_hypotheses.test_an_active_overlay_is_refused's session with a grant set: the refusal comes before the route"""
    base, steps, gg = synth.append_session(2500, 10000, 1, 16, seed=5)
    st1 = steps[0]
    arrs = [np.concatenate([getattr(base, k), st1[k]]) for k in ("ei", "ej", "meas", "info", "phi")]
    fixed = np.zeros(st1["V"], dtype=bool)
    fixed[0] = True
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_hypotheses_workspace(2 ** 30)
        opt.set_graph(*base.arrays())
        assert opt.optimize(2)[0] == 2
        P0 = np.empty((st1["V"], 3))
        P0[: base.V] = opt.get_poses()
        synth.chain_init(P0, gg.meas[: gg.V - 1], base.V, st1["V"] - 1)
        opt.update_graph(P0, fixed, *arrs, base.E)
        assert "incremental overlay" in opt.solver_description()
        assert opt.hypotheses_bytes(5, True) == 0
        p0 = opt.get_poses()
        out = sentinel_outputs(2, opt.V, opt.E, 5)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.optimize_hypotheses(np.zeros((2, opt.E), dtype=np.uint8), 5, 0.0, out=out)
        assert "overlay" in opt.last_error()
        assert untouched(out) and same_bits(opt.get_poses(), p0) and opt.hypotheses_workspace_bytes() == 0


def test_hypotheses_through_the_shim(tmp_path):
    """tests/cpp/replay_hypotheses_mfront.cpp: the graph through the g2o-compatible header with sgoSetHypothesesWorkspace, leave-one-
    out over its first five closures; what it returns is capi's answer with the same grant, bit for bit, and no estimate moved."""
    from test_shim_replay import _write_graph
    g = graph(MFRONT)
    B, iters, tol = 5, 6, 1e-3
    clo = np.arange(g.V - 1, g.V - 1 + B)
    M = np.zeros((B, g.E), dtype=np.uint8)
    M[np.arange(B), clo] = 1
    with open_ctx(g, PATH) as opt:
        grant = 3 * opt.hypotheses_bytes(iters, True)                    # chains of 3 + 2
        opt.set_hypotheses_workspace(grant)
        R = opt.optimize_hypotheses(M, iters, tol)
    assert R["route"] == capi.HYP_BATCHED
    exe = str(tmp_path / "replay_hypotheses_mfront")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(CPP, "replay_hypotheses_mfront.cpp"), "-L" + LIBDIR, "-lsgo", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 10.0)
    env = dict(os.environ)
    env.pop("SGO_DIRECT_ROWS", None)
    subprocess.check_call([exe, str(gf), str(of), str(iters), repr(tol), str(grant), str(B)], env=env)
    lines = open(of).read().split("\n")
    assert lines[0].startswith(PATH), lines[0]
    assert int(lines[1]) == B and int(lines[2]) == 0                      # hypotheses; estimates that moved
    at = 3
    for b in range(B):
        head = lines[at].split()
        assert (int(head[0]), int(head[1])) == (R["iters_done"][b], R["stop_reason"][b]), (b, head)
        assert [int(x, 16) for x in head[2:4]] == [int(x) for x in bits([R["chi2"][b], R["robust_chi2"][b]])], (b, head)
        e2 = np.array([int(x, 16) for x in lines[at + 1].split()], dtype=np.uint64)
        assert np.array_equal(e2, bits(R["edge_chi2"][b])), b
        P = np.array([int(x, 16) for x in " ".join(lines[at + 2: at + 2 + g.V]).split()], dtype=np.uint64).reshape(g.V, 3)
        assert np.array_equal(P, bits(R["poses"][b])), b
        at += 2 + g.V
