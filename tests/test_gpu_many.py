"""sgo_optimize_gn_many (include/sgo.h): many independent pose graphs optimised by one call, the direct_ldlt
ones in ONE launch of k_direct's MANY instantiation with a workgroup per graph.  The bar: every context ends as after its own
sgo_optimize_gn_until -- checked against TWIN contexts that run exactly that, bit for bit on the factorisation paths --, a graph
whose factorisation fails fails alone, contexts on other paths take their own route inside the call, and a refusal writes nothing."""
import ctypes as C
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

# (V, E, seed, phi): more than 512 edges, so k_direct's second edge pass runs; most threads idle in every phase; another phi;
# another seed and size; a single closure, so the separator block is as small as it gets
FIVE = ((600, 620, 3, 10.0), (40, 44, 5, 10.0), (200, 230, 7, 4.0), (1000, 1030, 11, 10.0), (120, 120 - 1 + 1, 12, 10.0))
HUBER = (600, 620, 17, 10.0)          # Huber kernels on its closures: the KINDS instantiations
XG = (7000, 7010, 21, 10.0)           # 3 n doubles do not fit the LDS: the XG instantiations
MFRONT = (2500, 3400, 31, 10.0)
PCG = (300, 600, 7, 10.0)
ITERS = 20


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def graph(shape):
    V, E, seed, phi = shape
    return synth.manhattan(V, E, seed=seed, info_mode="full", phi=phi)


def open_ctx(shape, path="direct_ldlt", **opts):
    g = graph(shape)
    opt = capi.Optimizer(0, **opts)
    opt.set_graph(*g.arrays())
    if shape == HUBER:
        clo = np.arange(g.V - 1, g.E, dtype=np.int32)
        opt.set_robust_kernels(clo, np.full(clo.size, capi.KERNEL_HUBER, dtype=np.int32), np.full(clo.size, 1.5))
    assert opt.solver_description().startswith(path), opt.solver_description()
    return opt


def own_call(opt, max_iters, tol):
    """what the call replaces, on one context: its own optimize_until"""
    rc, st, why = opt.optimize_until(max_iters, tol)
    return dict(rc=rc, why=why, done=st["iters_done"], chi2=np.array(st["chi2"]), robust=np.array(st["robust_chi2"]),
                poses=opt.get_poses(), err=opt.last_error())


@functools.lru_cache(maxsize=None)
def twin(shape, tol, max_iters=ITERS):
    with open_ctx(shape) as t:
        return own_call(t, max_iters, tol)


def check_against_twin(r, opt, t, tag):
    """one context's part of the call's answer, and the context itself, against its twin's own call: bit for bit"""
    assert (r["rc"], r["stop_reason"], r["iters_done"]) == (t["rc"], t["why"], t["done"]), (tag, r["rc"], r["stop_reason"], r["iters_done"], t)
    assert same_bits(r["chi2"], t["chi2"]), (tag, r["chi2"], t["chi2"])
    assert same_bits(r["robust_chi2"], t["robust"]), tag
    assert same_bits(opt.get_poses(), t["poses"]), (tag, np.abs(opt.get_poses() - t["poses"]).max())


def rule_stop(robust_chi2, gain_tol, max_iters):
    r = np.asarray(robust_chi2, dtype=np.float64)
    with np.errstate(all="ignore"):
        for it in range(2, max_iters):
            gain = (r[it - 1] - r[it]) / r[it]
            if gain >= 0.0 and gain < gain_tol:
                return it
    return max_iters


@functools.lru_cache(maxsize=None)
def stopping_tolerance():
    """1e-6 if it makes two of the five graphs stop at different iterations; otherwise a tolerance between two adjacent gains of
    the twins' own full histories that does (as tests/test_gpu_hypotheses.py chooses its own)"""
    full = [twin(s, 0.0) for s in FIVE]
    assert all(t["done"] == ITERS for t in full)
    gains = sorted({(t["robust"][i - 1] - t["robust"][i]) / t["robust"][i] for t in full for i in range(2, ITERS)})
    gains = [x for x in gains if x > 0.0]
    for tol in [1e-6] + [math.sqrt(a * b) for a, b in zip(gains, gains[1:])]:
        stops = [rule_stop(t["robust"], tol, ITERS) for t in full]
        if len(set(stops)) >= 2 and min(stops) < ITERS:
            return tol
    raise AssertionError(f"no tolerance separates the graphs' stop iterations: {gains}")


@pytest.mark.parametrize("stopping", [False, True])
def test_mixed_structures_share_one_launch(stopping):
    tol = stopping_tolerance() if stopping else 0.0
    T = [twin(s, tol) for s in FIVE]
    print(f"gain_tol {tol!r}: the twins end after {[t['done'] for t in T]} updates")
    if stopping:
        assert len({t["done"] for t in T}) >= 2 and any(t["why"] == capi.STOP_GAIN for t in T), [t["done"] for t in T]
    else:
        assert all(t["done"] == ITERS and t["why"] == capi.STOP_MAX_ITERS for t in T)
    opts = [open_ctx(s) for s in FIVE]
    try:
        R, launches = capi.optimize_many(opts, ITERS, tol)
        assert launches == 1 and [r["in_launch"] for r in R] == [1] * 5, (launches, [r["in_launch"] for r in R])
        for k, (r, o, t) in enumerate(zip(R, opts, T)):
            check_against_twin(r, o, t, f"graph {FIVE[k]}")
            assert r["pcg_converged"][: t["done"]] == [1] * t["done"] and r["seconds_total"] > 0.0
            assert all(s > 0.0 for s in r["seconds"][: t["done"]])       # (the workgroup's own stamps)
    finally:
        for o in opts:
            o.close()
    assert not same_bits(T[0]["poses"][:40], T[1]["poses"])               # (the graphs do differ)


def test_instantiation_groups_and_the_order_of_the_contexts():
    """The five plain graphs, one with Huber kernels (KINDS) and one whose vector lives in global memory (XG), interleaved: a
    launch per distinct group, and the same bits whatever the order."""
    order = (FIVE[0], HUBER, FIVE[1], XG, FIVE[2], FIVE[3], FIVE[4])
    T = {s: twin(s, 0.0) for s in order}
    assert not same_bits(T[HUBER]["robust"], T[HUBER]["chi2"])
    for perm in (list(range(7)), [3, 6, 1, 0, 5, 2, 4]):
        shapes = [order[k] for k in perm]
        opts = [open_ctx(s) for s in shapes]
        try:
            R, launches = capi.optimize_many(opts, ITERS, 0.0)
            # the groups through the SGO_DR_INFO row of every context (which the call has marked as run), not by the sizes
            xg = [int(dict(zip(capi.DIRECT_INFO, o.direct_arrays(("INFO",))["INFO"]))["xb_global"]) for o in opts]
            assert [x for s, x in zip(shapes, xg) if s == XG] == [1] and sum(xg) == 1, xg
            groups = {(x, s == HUBER) for s, x in zip(shapes, xg)}
            assert len(groups) == 3
            assert launches == len(groups) and all(r["in_launch"] == 1 for r in R), (launches, groups)
            for s, r, o in zip(shapes, R, opts):
                check_against_twin(r, o, T[s], f"order {perm}, graph {s}")
        finally:
            for o in opts:
                o.close()


def test_more_graphs_than_compute_units():
    """300 workgroups on 256 compute units: the second wave's graphs come out as the first wave's, each as its twin."""
    shapes = [FIVE[1], FIVE[4]] * 150
    T = {s: twin(s, 0.0, 6) for s in shapes[:2]}
    opts = [open_ctx(s) for s in shapes]
    try:
        R, launches = capi.optimize_many(opts, 6, 0.0)
        assert launches == 1 and all(r["in_launch"] == 1 for r in R)
        for k, (s, r, o) in enumerate(zip(shapes, R, opts)):
            check_against_twin(r, o, T[s], f"context {k}, graph {s}")
    finally:
        for o in opts:
            o.close()


def failing_arrays():
    """A graph whose last odometry edge has zero information and no closure bridging it: the last pose's Hessian block is zero,
    its first pivot is not positive."""
    g = synth.manhattan(300, 312, seed=9, info_mode="full", phi=10.0)
    k = g.V - 2
    lo, hi = np.minimum(g.ei, g.ej)[g.V - 1:], np.maximum(g.ei, g.ej)[g.V - 1:]
    assert (g.ei[k], g.ej[k]) == (k, k + 1) and not ((lo <= k) & (hi >= k + 1)).any()
    info = g.info.copy()
    info[k] = 0.0
    return (g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)


def test_a_failure_stays_local():
    args = failing_arrays()
    with capi.Optimizer(0) as t:
        t.set_graph(*args)
        assert t.solver_description().startswith("direct_ldlt")
        bad = own_call(t, ITERS, 0.0)
    assert bad["rc"] == 0 and bad["why"] == capi.STOP_FAILED and "not positive definite" in bad["err"], bad
    opts = [open_ctx(FIVE[0]), capi.Optimizer(0), open_ctx(FIVE[2])]
    try:
        opts[1].set_graph(*args)
        R, launches = capi.optimize_many(opts, ITERS, 0.0)
        assert launches == 1 and [r["in_launch"] for r in R] == [1, 1, 1]
        assert R[1]["rc"] == 0 and R[1]["stop_reason"] == capi.STOP_FAILED
        check_against_twin(R[1], opts[1], bad, "the failing graph")
        assert opts[1].last_error() == bad["err"] and same_bits(opts[1].get_poses(), args[0])
        check_against_twin(R[0], opts[0], twin(FIVE[0], 0.0), "the neighbour before")
        check_against_twin(R[2], opts[2], twin(FIVE[2], 0.0), "the neighbour after")
        assert opts[0].last_error() == twin(FIVE[0], 0.0)["err"] and opts[2].last_error() == twin(FIVE[2], 0.0)["err"]
    finally:
        for o in opts:
            o.close()


def test_mixed_routes():
    iters = 6
    shapes = (FIVE[0], MFRONT, PCG)
    paths = ("direct_ldlt", "multifrontal_cholesky", "pcg_amg")
    kw = ({}, {}, {"direct_rows": 0})
    T = []
    for s, p, k in zip(shapes, paths, kw):
        with open_ctx(s, p, **k) as t:
            T.append(own_call(t, iters, 0.0))
    opts = [open_ctx(s, p, **k) for s, p, k in zip(shapes, paths, kw)]
    try:
        R, launches = capi.optimize_many(opts, iters, 0.0)
        assert [r["in_launch"] for r in R] == [1, 0, 0] and launches == 1
        check_against_twin(R[0], opts[0], T[0], "direct")
        check_against_twin(R[1], opts[1], T[1], "multifrontal")
        # two PCG runs of the same system: the bound tests/test_gpu_hypotheses.py puts on its sequential route's PCG path
        assert (R[2]["rc"], R[2]["stop_reason"], R[2]["iters_done"]) == (T[2]["rc"], T[2]["why"], T[2]["done"])
        rel = np.abs(np.array(R[2]["chi2"]) - T[2]["chi2"]) / T[2]["chi2"]
        print(f"PCG context: {T[2]['done']} updates, max relative chi2 difference to its own call {rel.max():.3e}")
        assert rel.max() <= 1e-6, rel
    finally:
        for o in opts:
            o.close()


def test_the_state_afterwards():
    """A second call continues as a second optimize_until does; sgo_chi2, sgo_edge_chi2 and sgo_optimize_gn_hypotheses on a
    participant work as before; the workspace does not grow."""
    shapes = FIVE[:3]
    tol = stopping_tolerance()
    opts = [open_ctx(s) for s in shapes]
    twins = [open_ctx(s) for s in shapes]
    try:
        for t in twins:
            t.optimize_until(5, 0.0)
        R, _ = capi.optimize_many(opts, 5, 0.0)
        assert opts[1].many_workspace_bytes() == 0 and opts[2].many_workspace_bytes() == 0   # (the first context owns it)
        held = opts[0].many_workspace_bytes()
        assert held > 0
        second = [own_call(t, ITERS, tol) for t in twins]
        R, launches = capi.optimize_many(opts, ITERS, tol)
        assert launches == 1
        for s, r, o, t in zip(shapes, R, opts, second):
            check_against_twin(r, o, t, f"second call, graph {s}")
        held2 = opts[0].many_workspace_bytes()                               # (longer histories: it may have grown)
        assert held2 >= held
        R3, _ = capi.optimize_many(opts, 5, 0.0)                             # the first call's arguments again: nothing allocated
        for t in twins:
            t.optimize_until(5, 0.0)
        assert opts[0].many_workspace_bytes() == held2, (held2, opts[0].many_workspace_bytes())
        g = graph(shapes[0])
        M = np.zeros((2, g.E), dtype=np.uint8)
        M[1, g.V - 1] = 1
        for o, t in zip(opts, twins):
            assert same_bits(list(o.chi2()), list(t.chi2())) and same_bits(o.edge_chi2(), t.edge_chi2())
        assert same_bits(list(opts[0].chi2()), [R3[0]["chi2"][-1], R3[0]["robust_chi2"][-1]])
        A, B = opts[0].optimize_hypotheses(M, 5, 0.0), twins[0].optimize_hypotheses(M, 5, 0.0)
        assert A["route"] == B["route"] == capi.HYP_BATCHED
        for key in ("hist", "poses", "edge_chi2", "iters_done", "stop_reason"):
            assert np.array_equal(A[key], B[key], equal_nan=True), key
        d, st = opts[0].optimize(3)                                           # the context's own calls go on as the twin's
        d2, st2 = twins[0].optimize(3)
        assert d == d2 == 3 and same_bits(st["chi2"], st2["chi2"]) and same_bits(opts[0].get_poses(), twins[0].get_poses())
    finally:
        for o in opts + twins:
            o.close()


def test_the_profile_records_each_shared_launch_once():
    """With sgo_opts.profile the first context's k_direct slot gets one sample per shared launch, with the summed bytes."""
    shapes = (FIVE[1], HUBER, FIVE[4])
    own = []
    for s in shapes:
        with open_ctx(s, profile=1) as t:
            t.optimize_until(5, 0.0)
            p = t.kernel_profile()["k_direct"]
            assert p["launches"] == 1
            own.append(p["bytes"])
    opts = [open_ctx(shapes[0], profile=1)] + [open_ctx(s) for s in shapes[1:]]
    try:
        R, launches = capi.optimize_many(opts, 5, 0.0)
        assert launches == 2 and [r["in_launch"] for r in R] == [1, 1, 1]
        p = opts[0].kernel_profile()["k_direct"]
        assert p["launches"] == 2 and p["ms"] > 0.0, p
        assert abs(p["bytes"] - sum(own)) <= 1e-12 * sum(own), (p["bytes"], own)
        assert "k_direct" not in opts[1].kernel_profile() and "k_direct" not in opts[2].kernel_profile()
    finally:
        for o in opts:
            o.close()


SENTINEL = -777.25


def test_refusals_write_nothing():
    L = capi.lib()
    shapes = FIVE[1:3]
    opts = [open_ctx(s) for s in shapes]
    sharded = capi.Optimizer(0, direct_rows=0)                          # the rank emulation of a multi-GPU context
    empty = capi.Optimizer(0)                                           # no graph
    try:
        sharded.debug_set_shard(2, 0)
        sharded.set_graph(*graph(FIVE[1]).arrays())
        before = [o.get_poses() for o in opts] + [sharded.get_poses()]

        def call(ctxs, n, max_iters=ITERS, tol=0.0, with_res=True, null_ctxs=False):
            m = max(len(ctxs), 1)
            h = (C.c_void_p * m)(*[None if o is None else o._h for o in ctxs])
            stats = [capi.Stats() for _ in range(m)]
            for st in stats:
                st.iters_done, st.seconds_total = -7, SENTINEL
            sp = (C.POINTER(capi.Stats) * m)(*[C.pointer(st) for st in stats])
            res = (capi.ManyResult * m)()
            for r in res:
                r.rc = r.stop_reason = r.in_launch = -7
            launches = C.c_int32(-7)
            rc = L.sgo_optimize_gn_many(None if null_ctxs else h, n, max_iters, tol, sp, res if with_res else None, C.byref(launches))
            untouched = (launches.value == -7 and all((r.rc, r.stop_reason, r.in_launch) == (-7, -7, -7) for r in res) and
                         all(st.iters_done == -7 and st.seconds_total == SENTINEL for st in stats))
            return rc, untouched

        cases = {
            "n < 0": dict(ctxs=opts, n=-1),
            "max_iters < 0": dict(ctxs=opts, n=2, max_iters=-1),
            "max_iters > SGO_MAX_ITERS": dict(ctxs=opts, n=2, max_iters=capi.SGO_MAX_ITERS + 1),
            "gain_tol inf": dict(ctxs=opts, n=2, tol=math.inf),
            "gain_tol nan": dict(ctxs=opts, n=2, tol=math.nan),
            "NULL ctxs": dict(ctxs=opts, n=2, null_ctxs=True),
            "NULL res": dict(ctxs=opts, n=2, with_res=False),
            "a NULL context": dict(ctxs=[opts[0], None], n=2),
            "a duplicate context": dict(ctxs=[opts[0], opts[1], opts[0]], n=3),
            "a multi-GPU context": dict(ctxs=[opts[0], sharded, opts[1]], n=3),
        }
        try:
            other = capi.Optimizer(1)                                   # a second device, where the machine has one
        except capi.SgoError:
            other = None
        if other is not None:
            other.set_graph(*graph(FIVE[1]).arrays())
            cases["contexts on different devices"] = dict(ctxs=[opts[0], other], n=2)
        for name, kw in cases.items():
            rc, untouched = call(**kw)
            assert rc == -2 and untouched, (name, rc, untouched)
        rc, untouched = call(ctxs=[opts[0], empty, opts[1]], n=3)
        assert rc == -4 and untouched, rc                                    # SGO_ENOGRAPH
        assert "no graph" in opts[0].last_error()
        for o, p in zip(opts + [sharded], before):
            assert same_bits(o.get_poses(), p)
        if other is not None:
            other.close()
        # ... and the contexts are as good as new: the call itself, now
        R, launches = capi.optimize_many(opts, ITERS, 0.0)
        for s, r, o in zip(shapes, R, opts):
            check_against_twin(r, o, twin(s, 0.0), f"after the refusals, graph {s}")
    finally:
        for o in opts + [sharded, empty]:
            o.close()


def test_many_through_the_shim(tmp_path):
    """tests/cpp/replay_many.cpp: three SparseOptimizers of VertexSE2 / EdgeSE2 graphs under Gauss-Newton through
    SparseOptimizer::sgoOptimizeMany; the estimates and return values are those of three separate optimize(12)."""
    from test_shim_replay import _write_graph
    exe = str(tmp_path / "replay_many")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(CPP, "replay_many.cpp"), "-L" + LIBDIR, "-lsgo", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    files = []
    for k, s in enumerate((FIVE[4], FIVE[1], FIVE[2])):
        g = graph(s)
        files.append(str(tmp_path / f"g{k}.txt"))
        _write_graph(files[-1], g, s[3])
    env = dict(os.environ)
    env.pop("SGO_DIRECT_ROWS", None)
    outs = {}
    for mode in ("many", "loop"):
        of = str(tmp_path / f"{mode}.txt")
        subprocess.check_call([exe, mode, "12", of] + files, env=env)
        outs[mode] = open(of).read()
    lines = outs["many"].split("\n")
    at = 0
    for s in (FIVE[4], FIVE[1], FIVE[2]):
        done, V = map(int, lines[at].split())
        assert done == 12 and V == s[0] and lines[at + 1].startswith("direct_ldlt"), lines[at: at + 2]
        P = np.array([int(x, 16) for x in " ".join(lines[at + 2: at + 2 + V]).split()], dtype=np.uint64).reshape(V, 3)
        with open_ctx(s) as o:                                           # (and capi's answer for the same graph)
            assert o.optimize(12)[0] == 12
            assert np.array_equal(P, bits(o.get_poses())), s
        at += 2 + V
    assert outs["many"] == outs["loop"]
