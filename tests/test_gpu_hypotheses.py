"""sgo_optimize_gn_hypotheses (include/sgo.h): the resident graph optimised once per closure hypothesis in one
call -- on the single-launch path as ONE launch of B workgroups of k_direct's batched instantiation, on every other single-GPU path
as the host loop inside the call.  The bar: on the factorisation paths everything a hypothesis returns is, bit for bit, what the
host loop { sgo_set_edge_information(zero rows); sgo_set_poses; sgo_optimize_gn_until; read back; restore } returns on a twin
context, a failing hypothesis fails alone, and the context is left as it was."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from sparse_gslam_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "sparse_gslam_amd", "csrc")

DIRECT = (600, 620, 3)            # more than 512 edges: k_direct's second edge pass runs
MFRONT = (2500, 3400, 31)
PCG = (3000, 12000, 7)
PATHS = {DIRECT: ({}, "direct_ldlt"), MFRONT: ({}, "multifrontal_cholesky"), PCG: ({"direct_rows": 0}, "pcg_amg")}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def graph(shape):
    V, E, seed = shape
    return synth.manhattan(V, E, seed=seed, info_mode="full", phi=10.0)


def open_ctx(g, path, **opts):
    opt = capi.Optimizer(0, **opts)
    opt.set_graph(*g.arrays())
    desc = opt.solver_description()
    assert desc.startswith(path), desc
    return opt


def host_loop(opt, info, masks, max_iters, tol, poses0=None):
    """The loop the call replaces, on the context `opt` whose resident rows are `info`: per hypothesis zero rows, the start, the
    optimisation, the read-back, the rows again; the resident poses at the end."""
    resident = opt.get_poses()
    out = []
    for b, off in enumerate(masks):
        ids = np.flatnonzero((off != 0) & np.any(info != 0.0, axis=1)).astype(np.int32)
        if ids.size:
            opt.set_edge_information(ids, np.zeros((ids.size, 6)))
        opt.set_poses(resident if poses0 is None else poses0[b])
        rc, st, why = opt.optimize_until(max_iters, tol)
        out.append(dict(rc=rc, done=st["iters_done"], why=why, chi2=np.array(st["chi2"]), robust=np.array(st["robust_chi2"]),
                        poses=opt.get_poses()))
        if ids.size:
            opt.set_edge_information(ids, info[ids])
    opt.set_poses(resident)
    return out


def check_against_loop(R, L, max_iters, what=""):
    """everything hypothesis b returns against the loop's turn b, bit for bit"""
    for b, l in enumerate(L):
        d = l["done"]
        tag = f"{what} hypothesis {b}"
        assert R["iters_done"][b] == d and R["stop_reason"][b] == l["why"], (tag, R["iters_done"][b], d, R["stop_reason"][b], l["why"])
        assert same_bits(R["hist"][b, : d + 1, 0], l["chi2"]), (tag, R["hist"][b, : d + 1, 0], l["chi2"])
        assert same_bits(R["hist"][b, : d + 1, 1], l["robust"]), tag
        assert np.isnan(R["hist"][b, d + 1:]).all() and R["hist"].shape == (len(L), max_iters + 1, 2), tag
        assert same_bits(R["poses"][b], l["poses"]), (tag, np.abs(R["poses"][b] - l["poses"]).max())
        assert same_bits([R["chi2"][b], R["robust_chi2"][b]], [l["chi2"][d], l["robust"][d]]), tag


def rule_stop(robust_chi2, gain_tol, max_iters):
    r = np.asarray(robust_chi2, dtype=np.float64)
    with np.errstate(all="ignore"):
        for it in range(2, max_iters):
            gain = (r[it - 1] - r[it]) / r[it]
            if gain >= 0.0 and gain < gain_tol:
                return it
    return max_iters


def masks7(g):
    """none off; each of three single closures; all closures; a random half of them; one odometry edge in mid-chain together with
    a closure, while another closure still ties the two halves"""
    V, E = g.V, g.E
    clo = np.arange(V - 1, E)
    M = np.zeros((7, E), dtype=np.uint8)
    for b, k in enumerate((clo[0], clo[len(clo) // 3], clo[-1])):
        M[1 + b, k] = 1
    M[4, clo] = 1
    M[5, clo[np.random.default_rng(1).random(clo.size) < 0.5]] = 1
    lo, hi = np.minimum(g.ei, g.ej), np.maximum(g.ei, g.ej)
    for k in sorted(range(V - 1), key=lambda k: abs(k - V // 2)):       # the odometry edge (k, k + 1) nearest the middle ...
        span = [c for c in clo if lo[c] <= k and hi[c] >= k + 1]        # ... that closures bridge
        if span:
            other = span[1] if len(span) > 1 else [c for c in clo if c != span[0]][0]
            M[6, [k, other]] = 1                                        # span[0] stays
            break
    assert M[6].sum() == 2
    return M


@functools.lru_cache(maxsize=None)
def direct_loop(tol):
    g = graph(DIRECT)
    with open_ctx(g, "direct_ldlt") as twin:
        return host_loop(twin, g.info, masks7(g), 20, tol)


@functools.lru_cache(maxsize=None)
def stopping_tolerance():
    """1e-6 if it makes two of the seven hypotheses stop at different iterations; otherwise a tolerance between two adjacent gains
    of the loop's own full histories that does"""
    full = direct_loop(0.0)
    assert all(l["done"] == 20 for l in full)
    gains = sorted({(l["robust"][i - 1] - l["robust"][i]) / l["robust"][i] for l in full for i in range(2, 20)})
    gains = [x for x in gains if x > 0.0]
    for tol in [1e-6] + [math.sqrt(a * b) for a, b in zip(gains, gains[1:])]:
        stops = {rule_stop(l["robust"], tol, 20) for l in full}
        if len(stops) >= 2 and min(stops) < 20:
            return tol
    raise AssertionError(f"no tolerance separates the hypotheses' stop iterations: {gains}")


@functools.lru_cache(maxsize=None)
def direct_batch(tol):
    g = graph(DIRECT)
    with open_ctx(g, "direct_ldlt") as opt:
        return opt.optimize_hypotheses(masks7(g), 20, tol)


@pytest.mark.parametrize("stopping", [False, True])
def test_batch_equals_loop_bit_for_bit(stopping):
    tol = stopping_tolerance() if stopping else 0.0
    L = direct_loop(tol)
    R = direct_batch(tol)
    assert R["route"] == capi.HYP_BATCHED
    print(f"gain_tol {tol!r}: the loop's hypotheses end after {[l['done'] for l in L]} updates")
    if stopping:
        assert len({l["done"] for l in L}) >= 2 and any(l["why"] == capi.STOP_GAIN for l in L), [l["done"] for l in L]
    else:
        assert all(l["done"] == 20 and l["why"] == capi.STOP_MAX_ITERS for l in L)
    check_against_loop(R, L, 20)
    assert not same_bits(R["poses"][0], R["poses"][4])                 # (the masks do change the answer)


def test_one_hypothesis_with_nothing_off_is_the_plain_until_call():
    g = graph(DIRECT)
    tol = stopping_tolerance()
    with open_ctx(g, "direct_ldlt") as fresh:
        rc, st, why = fresh.optimize_until(20, tol)
        P = fresh.get_poses()
    with open_ctx(g, "direct_ldlt") as opt:
        R = opt.optimize_hypotheses(np.zeros((1, g.E), dtype=np.uint8), 20, tol)
    d = st["iters_done"]
    assert R["route"] == capi.HYP_BATCHED and R["iters_done"][0] == d == rc and R["stop_reason"][0] == why
    assert same_bits(R["hist"][0, : d + 1, 0], st["chi2"]) and same_bits(R["hist"][0, : d + 1, 1], st["robust_chi2"])
    assert same_bits(R["poses"][0], P)


def test_own_starting_poses():
    g = graph(DIRECT)
    M = masks7(g)[[0, 1, 4, 6]]
    P0 = np.repeat(g.poses[None], 4, axis=0)
    free = ~np.asarray(g.fixed, bool)
    for b in range(4):
        P0[b, free] += 1e-2 * np.random.default_rng(b).standard_normal((int(free.sum()), 3))
    with open_ctx(g, "direct_ldlt") as twin:
        L = host_loop(twin, g.info, M, 20, 0.0, P0)
    with open_ctx(g, "direct_ldlt") as opt:
        R = opt.optimize_hypotheses(M, 20, 0.0, poses0=P0)
        assert same_bits(opt.get_poses(), g.poses)
    assert R["route"] == capi.HYP_BATCHED
    check_against_loop(R, L, 20)
    assert same_bits(R["poses"][:, ~free], P0[:, ~free]) and same_bits(P0[0, ~free], g.poses[~free])   # the fixed pose comes back unchanged
    assert not same_bits(L[0]["chi2"][:1], direct_loop(0.0)[0]["chi2"][:1])                       # (the starts were used)


def test_more_workgroups_than_compute_units_and_no_aliasing():
    g = graph(DIRECT)
    two = masks7(g)[[5, 6]]
    with open_ctx(g, "direct_ldlt") as twin:
        L = host_loop(twin, g.info, two, 6, 0.0)
    with open_ctx(g, "direct_ldlt") as opt:
        small = opt.optimize_hypotheses(two, 6, 0.0)                   # the context's workspace grows for the next call ...
        R = opt.optimize_hypotheses(np.tile(two, (150, 1)), 6, 0.0)
        again = opt.optimize_hypotheses(two, 6, 0.0)                   # ... and is reused by this one
    assert R["route"] == capi.HYP_BATCHED and R["poses"].shape[0] == 300
    for key in ("hist", "poses", "edge_chi2", "chi2", "robust_chi2", "iters_done", "stop_reason"):
        for par in (0, 1):
            a = R[key][par::2]
            assert all(np.array_equal(a[0], x, equal_nan=True) for x in a), (key, par)
        assert np.array_equal(small[key], R[key][:2], equal_nan=True) and np.array_equal(again[key], R[key][:2], equal_nan=True), key
    check_against_loop({k: (v[:2] if k != "route" else v) for k, v in R.items()}, L, 6)


def test_the_vector_in_global_memory():
    """3 n doubles of this graph exceed the kernel's LDS budget: the right-hand side / solution vector lives in global memory, one
    copy per hypothesis."""
    g = synth.manhattan(8000, 8000 - 1 + 58, seed=21, info_mode="full", init="incremental", phi=10.0)
    assert 24 * g.V > 150 * 1024
    M = np.zeros((3, g.E), dtype=np.uint8)
    M[1, g.V - 1] = 1
    M[2, [g.V + 10, g.E - 1]] = 1
    with open_ctx(g, "direct_ldlt") as twin:
        L = host_loop(twin, g.info, M, 4, 0.0)
    with open_ctx(g, "direct_ldlt") as opt:
        R = opt.optimize_hypotheses(M, 4, 0.0)
    assert R["route"] == capi.HYP_BATCHED
    check_against_loop(R, L, 4)
    assert not same_bits(R["poses"][0], R["poses"][2])


def test_other_kernel_kinds():
    g = graph(DIRECT)
    clo = np.arange(g.V - 1, g.E, dtype=np.int32)
    kinds = np.array([capi.KERNEL_HUBER, capi.KERNEL_CAUCHY, capi.KERNEL_TUKEY], dtype=np.int32)[(3 * np.arange(clo.size)) // clo.size]
    delta = np.where(kinds == capi.KERNEL_TUKEY, 4.0, 1.5)
    M = masks7(g)[[0, 2, 5]]

    def ctx():
        opt = open_ctx(g, "direct_ldlt")
        opt.set_robust_kernels(clo, kinds, delta)
        return opt

    with ctx() as twin:
        L = host_loop(twin, g.info, M, 20, 0.0)
    with ctx() as opt:
        R = opt.optimize_hypotheses(M, 20, 0.0)
    assert R["route"] == capi.HYP_BATCHED
    check_against_loop(R, L, 20)
    assert not same_bits(L[0]["robust"], direct_loop(0.0)[0]["robust"])   # (the kernels were used)


def test_a_failing_hypothesis_stays_alone():
    """One closure's information negated: the Hessian with it is indefinite (its pivot test fails, a clean failure flag), without
    it the graph optimises as usual."""
    g = graph(DIRECT)
    info = g.info.copy()
    c = g.E - 1
    info[c, [0, 3, 5]] *= -1.0
    M = np.zeros((2, g.E), dtype=np.uint8)
    M[1, c] = 1
    args = (g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)
    with capi.Optimizer(0) as twin:
        twin.set_graph(*args)
        assert twin.solver_description().startswith("direct_ldlt")
        L = host_loop(twin, info, M, 20, 0.0)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*args)
        assert opt.solver_description().startswith("direct_ldlt")
        R = opt.optimize_hypotheses(M, 20, 0.0)
    assert R["route"] >= 0
    assert R["stop_reason"][0] == capi.STOP_FAILED and R["iters_done"][0] == 0 and same_bits(R["poses"][0], g.poses)
    assert L[0]["why"] == capi.STOP_FAILED and L[0]["done"] == 0
    assert R["stop_reason"][1] == capi.STOP_MAX_ITERS and R["iters_done"][1] == 20
    check_against_loop(R, L, 20)


def test_edge_chi2_is_formed_with_the_resident_information():
    from oracle import c_oracle
    g = graph(DIRECT)
    M = masks7(g)
    held = np.array([g.V + 3, g.V + 7], dtype=np.int32)                  # two closures the context itself holds inactive
    for tol, inactive in ((0.0, False), (stopping_tolerance(), False), (0.0, True)):
        if inactive:
            with open_ctx(g, "direct_ldlt") as opt:
                opt.set_edge_information(held, np.zeros((2, 6)))
                R = opt.optimize_hypotheses(M, 20, tol)
            info = g.info.copy()
            info[held] = 0.0
        else:
            R, info = direct_batch(tol), g.info
        for b in range(M.shape[0]):
            P = R["poses"][b]
            _, _, _, oe2, _, _ = c_oracle.edges(P[g.ei], P[g.ej], g.meas, info, g.phi)
            err = np.abs(R["edge_chi2"][b] - oe2).max()
            assert err <= 1e-11 * max(1.0, np.abs(oe2).max()), (b, err)
            active = (M[b] == 0)
            s = R["edge_chi2"][b][active].sum()
            assert abs(s - R["chi2"][b]) <= g.E * 2.0 ** -53 * R["chi2"][b], (b, s, R["chi2"][b])
            if M[b].any():
                assert (R["edge_chi2"][b][M[b] != 0] > 0.0).sum() >= 1     # a switched-off edge reports what it would cost
            if inactive:
                assert (R["edge_chi2"][b][held] == 0.0).all()


@pytest.mark.parametrize("shape", [DIRECT, MFRONT])
def test_nothing_is_left_behind(shape):
    g = graph(shape)
    opts, path = PATHS[shape]
    M = np.zeros((3, g.E), dtype=np.uint8)
    M[1, g.V - 1] = 1
    M[2, g.V - 1:] = 1

    def session(call):
        with open_ctx(g, path, **opts) as opt:
            assert opt.optimize(3)[0] == 3
            before = (opt.get_poses(), opt.chi2(), opt.solver_description(), opt.optimize(0)[1]["seconds_setup"])
            if call:
                R = opt.optimize_hypotheses(M, 5, 0.0)
                assert R["route"] == (capi.HYP_BATCHED if shape == DIRECT else capi.HYP_SEQUENTIAL)
                after = (opt.get_poses(), opt.chi2(), opt.solver_description(), opt.optimize(0)[1]["seconds_setup"])
                assert same_bits(after[0], before[0]) and same_bits(list(after[1]), list(before[1]))
                assert after[2] == before[2] and after[3] == before[3], (before[2:], after[2:])
            d, st = opt.optimize(20)
            return d, st, opt.get_poses()

    dA, stA, PA = session(True)
    dB, stB, PB = session(False)
    assert dA == dB == 20
    assert same_bits(stA["chi2"], stB["chi2"]) and same_bits(stA["robust_chi2"], stB["robust_chi2"])
    assert same_bits(PA, PB)


@pytest.mark.parametrize("shape", [MFRONT, PCG])
def test_sequential_route(shape):
    g = graph(shape)
    opts, path = PATHS[shape]
    M = np.zeros((3, g.E), dtype=np.uint8)
    M[1, g.V - 1 + 5] = 1
    M[2, g.V - 1: g.V - 1 + 5] = 1
    iters = 6
    with open_ctx(g, path, **opts) as twin:
        L = host_loop(twin, g.info, M, iters, 0.0)
    with open_ctx(g, path, **opts) as opt:
        R = opt.optimize_hypotheses(M, iters, 0.0)
        assert same_bits(opt.get_poses(), g.poses)
    assert R["route"] == capi.HYP_SEQUENTIAL
    if shape == MFRONT:
        check_against_loop(R, L, iters)
    else:
        # two PCG runs of the same system: the relative bound tests/test_gpu_optimize_until.py puts on chi2 of a PCG call against the
        # same iterations computed elsewhere (line 155: max(rel) <= 1e-6)
        for b, l in enumerate(L):
            d = l["done"]
            assert R["iters_done"][b] == d
            rel = np.abs(R["hist"][b, : d + 1, 0] - l["chi2"]) / l["chi2"]
            print(f"hypothesis {b}: {d} updates, max relative chi2 difference to the loop {rel.max():.3e}")
            assert rel.max() <= 1e-6, (b, rel)
    from oracle import c_oracle
    for b in range(3):                                                   # (the per-edge values of this route: sgo_edge_chi2's)
        P = R["poses"][b]
        _, _, _, oe2, _, _ = c_oracle.edges(P[g.ei], P[g.ej], g.meas, g.info, g.phi)
        assert np.abs(R["edge_chi2"][b] - oe2).max() <= 1e-11 * max(1.0, np.abs(oe2).max())


SENTINEL = -777.25


def sentinel_outputs(B, V, E, iters):
    res = (capi.HypothesisResult * B)()
    for b in range(B):
        res[b].iters_done, res[b].stop_reason, res[b].chi2, res[b].robust_chi2 = -7, -7, SENTINEL, SENTINEL
    return dict(res=res, hist=np.full((B, max(iters + 1, 0), 2), SENTINEL), poses=np.full((B, V, 3), SENTINEL), edge_chi2=np.full((B, E), SENTINEL))


def untouched(out):
    return (all(r.iters_done == -7 and r.stop_reason == -7 and r.chi2 == SENTINEL and r.robust_chi2 == SENTINEL for r in out["res"]) and
            all((out[k] == SENTINEL).all() for k in ("hist", "poses", "edge_chi2")))


def test_refusals_write_nothing():
    import ctypes as C
    g = graph(DIRECT)
    B = 2
    with open_ctx(g, "direct_ldlt") as opt:
        p0 = opt.get_poses()
        v = 300
        M = np.zeros((B, g.E), dtype=np.uint8)
        M[1, (g.ei == v) | (g.ej == v)] = 1                             # hypothesis 1 takes every edge of pose 300 away
        out = sentinel_outputs(B, g.V, g.E, 20)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.optimize_hypotheses(M, 20, 0.0, out=out)
        assert "hypothesis 1" in opt.last_error() and f"vertex {v}" in opt.last_error(), opt.last_error()
        assert untouched(out) and same_bits(opt.get_poses(), p0)
        assert capi.hypothesis_isolated_vertex(g.fixed, g.ei, g.ej, g.info, M[1]) == v
        u8, d = C.POINTER(C.c_uint8), C.POINTER(C.c_double)              # a negative count: the binding cannot say it
        rc = capi.lib().sgo_optimize_gn_hypotheses(opt._h, -1, 20, 0.0, M.ctypes.data_as(u8), None, out["res"], out["hist"].ctypes.data_as(d),
                                                   out["poses"].ctypes.data_as(d), out["edge_chi2"].ctypes.data_as(d))
        assert rc == -2 and untouched(out) and same_bits(opt.get_poses(), p0)
        M[:] = 0
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
        opt.set_graph(*g.arrays())
        p0 = opt.get_poses()
        out = sentinel_outputs(B, g.V, g.E, 20)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.optimize_hypotheses(M, 20, 0.0, out=out)
        assert "multi-GPU" in opt.last_error()
        assert untouched(out) and same_bits(opt.get_poses(), p0)


def test_an_active_overlay_is_refused():
    base, steps, gg = synth.append_session(2500, 10000, 1, 16, seed=5)
    st1 = steps[0]
    arrs = [np.concatenate([getattr(base, k), st1[k]]) for k in ("ei", "ej", "meas", "info", "phi")]
    fixed = np.zeros(st1["V"], dtype=bool)
    fixed[0] = True
    with capi.Optimizer(0, direct_rows=0) as opt:
        opt.set_graph(*base.arrays())
        assert opt.optimize(2)[0] == 2
        P0 = np.empty((st1["V"], 3))
        P0[: base.V] = opt.get_poses()
        synth.chain_init(P0, gg.meas[: gg.V - 1], base.V, st1["V"] - 1)
        opt.update_graph(P0, fixed, *arrs, base.E)
        assert "incremental overlay" in opt.solver_description()
        p0 = opt.get_poses()
        out = sentinel_outputs(2, opt.V, opt.E, 5)
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.optimize_hypotheses(np.zeros((2, opt.E), dtype=np.uint8), 5, 0.0, out=out)
        assert "overlay" in opt.last_error()
        assert untouched(out) and same_bits(opt.get_poses(), p0)


def test_hypotheses_through_the_shim(tmp_path):
    """tests/cpp/replay_hypotheses.cpp: a VertexSE2 / EdgeSE2 graph under Gauss-Newton, sgoOptimizeHypotheses with leave-one-out
    sets over its closures; what it returns is capi's answer on the same graph, bit for bit, and no estimate moved."""
    from test_shim_replay import _write_graph
    g = synth.manhattan(120, 128, seed=12, info_mode="full", phi=10.0)
    exe = str(tmp_path / "replay_hypotheses")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(CPP, "replay_hypotheses.cpp"), "-L" + LIBDIR, "-lsgo", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 10.0)
    env = dict(os.environ)
    env.pop("SGO_DIRECT_ROWS", None)
    subprocess.check_call([exe, str(gf), str(of), "12", "1e-3"], env=env)
    lines = open(of).read().split("\n")
    assert lines[0].startswith("direct_ldlt"), lines[0]
    clo = np.arange(g.V - 1, g.E)
    B = clo.size
    assert int(lines[1]) == B and int(lines[2]) == 0                      # hypotheses; estimates that moved
    M = np.zeros((B, g.E), dtype=np.uint8)
    M[np.arange(B), clo] = 1
    with open_ctx(g, "direct_ldlt") as opt:
        R = opt.optimize_hypotheses(M, 12, 1e-3)
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
