"""sgo_optimize_gn_until on the device (include/sgo.h): sgo_optimize_gn that ends before the first iteration
at which the gain rule holds -- decided inside k_direct on the single-launch path, by k_mf_gain_stop between the launches of the
multifrontal path, and by the host behind one small synchronisation on the PCG path (an incremental overlay included).  The bar: the
call is a PREFIX of sgo_optimize_gn(max_iters) bit for bit, it stops where the CPU oracle's history says, on the factorisation
paths it leaves the poses and the factor of sgo_optimize_gn(k*) bit for bit, and it leaves nothing behind."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from sparse_gslam_amd import capi, synth
from test_stop_rule import STOPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "sparse_gslam_amd", "csrc")

# the small graph of each path: (V, E, seed) -> (Optimizer options, what sgo_solver_description starts with).  600 / 620 has more
# than 513 edges: k_direct's second edge pass runs.
PATHS = {
    (600, 620, 3): ({}, "direct_ldlt"),
    (2500, 3400, 31): ({}, "multifrontal_cholesky"),
    (3000, 12000, 7): ({"direct_rows": 0}, "pcg_amg"),
}
SHAPES = sorted(PATHS)
FACTORED = [s for s in SHAPES if PATHS[s][1] != "pcg_amg"]
CASES = [(s, tol) for s in SHAPES for tol in sorted(STOPS[s], reverse=True)]
MF_ARRAYS = ("ARENA", "X", "INVD", "YINV", "FLAGS")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def rule_stop(robust_chi2, gain_tol, max_iters):
    """the rule in numpy, as include/sgo.h states it"""
    r = np.asarray(robust_chi2, dtype=np.float64)
    with np.errstate(all="ignore"):
        for it in range(2, max_iters):
            gain = (r[it - 1] - r[it]) / r[it]
            if gain >= 0.0 and gain < gain_tol:
                return it
    return max_iters


@functools.lru_cache(maxsize=None)
def graph(shape):
    V, E, seed = shape
    return synth.manhattan(V, E, seed=seed, info_mode="full", phi=10.0)


def run(shape, calls):
    """A fresh context on the graph; calls: ("gn", iters) or ("until", max_iters, tol) in turn.  Returns the description, per call
    (done, stats, reason), the final poses, sgo_chi2 and (multifrontal path) the factor's arrays."""
    opts, path = PATHS[shape]
    with capi.Optimizer(0, **opts) as opt:
        opt.set_graph(*graph(shape).arrays())
        desc = opt.solver_description()
        assert desc.startswith(path), desc
        res = []
        for c in calls:
            if c[0] == "gn":
                d, st = opt.optimize(c[1])
                res.append((d, st, None))
            else:
                res.append(opt.optimize_until(c[1], c[2]))
        ran = any(c[1] > 0 for c in calls)                         # (the hook has nothing to show before the first factorisation)
        mf = opt.mfront_arrays(MF_ARRAYS) if path == "multifrontal_cholesky" and ran else None
        return dict(res=res, poses=opt.get_poses(), chi2=opt.chi2(), mf=mf)


@functools.lru_cache(maxsize=None)
def plain20(shape):
    return run(shape, (("gn", 20),))


@functools.lru_cache(maxsize=None)
def until20(shape, tol):
    return run(shape, (("until", 20, tol),))


@functools.lru_cache(maxsize=None)
def plain_k(shape, k):
    return run(shape, (("gn", k),))


@functools.lru_cache(maxsize=None)
def oracle_k(shape, k):
    from oracle import c_oracle
    return c_oracle.gauss_newton(*graph(shape).arrays(), iters=k, solver="direct")


def check_prefix(A, B, k):
    """B, an until-call that stopped before iteration k, against A, the plain call's stats of the same start"""
    d, st, why = B["res"][-1]
    assert d == k == st["iters_done"] and why == capi.STOP_GAIN, (d, k, why)
    assert len(st["chi2"]) == k + 1 and len(st["robust_chi2"]) == k + 1
    assert same_bits(st["chi2"], A["chi2"][: k + 1]), (st["chi2"], A["chi2"])
    assert same_bits(st["robust_chi2"], A["robust_chi2"][: k + 1])


@pytest.mark.parametrize("shape,tol", CASES)
def test_until_is_a_prefix_of_the_plain_call(shape, tol):
    dA, stA, _ = plain20(shape)["res"][0]
    assert dA == 20
    k = rule_stop(stA["robust_chi2"], tol, 20)
    assert 2 <= k < 20
    check_prefix(stA, until20(shape, tol), k)
    other = [t for t in STOPS[shape] if t != tol][0]
    assert rule_stop(stA["robust_chi2"], other, 20) != k          # the two tolerances exercise two stop iterations


@pytest.mark.parametrize("shape,tol", CASES)
def test_sgo_chi2_after_the_call_is_the_final_value(shape, tol):
    """The final entries of the history are the sums AT the final poses: sgo_chi2 afterwards equals chi2[k*] and robust_chi2[k*].
    Bit for bit.  On the PCG path the history and sgo_chi2 come from the same two kernels, on the multifrontal path the partial sums
    are added in the same order, and on the single-launch path sgo_chi2 IS k_direct's closing pass (a call of 0 iterations): k_chi2
    forms the edge error from another sincos and adds in another order, and its sums differed from the history's in the last bits
    there (88.25417979114252 against 88.25417979114239 at k* = 8 on the 600 / 620 graph).  The same holds after the plain call of
    k* iterations, printed and asserted below.  The relative bound before the bitwise one: a sum of E <= 12 000 terms of one sign
    taken in two orders differs by less than E * 2^-53 < 2e-12 relative."""
    B = until20(shape, tol)
    k, st, _ = B["res"][0]
    C = plain_k(shape, k)
    want = [st["chi2"][k], st["robust_chi2"][k]]
    print(f"{shape} tol {tol}: after until, sgo_chi2 {B['chi2']!r} against the history's {want!r}; after the plain call of {k}: "
          f"{C['chi2']!r} against {[C['res'][0][1]['chi2'][k], C['res'][0][1]['robust_chi2'][k]]!r}")
    assert all(abs(a - b) <= 2e-12 * b for a, b in zip(B["chi2"], want)), (B["chi2"], want)
    assert same_bits(list(B["chi2"]), want), (B["chi2"], want)
    stC = C["res"][0][1]
    assert same_bits(list(C["chi2"]), [stC["chi2"][k], stC["robust_chi2"][k]]), (C["chi2"], stC["chi2"][k], stC["robust_chi2"][k])


@pytest.mark.parametrize("shape,tol", CASES)
def test_stops_where_the_oracle_does_and_at_its_estimate(shape, tol):
    k = STOPS[shape][tol]
    B = until20(shape, tol)
    d, st, why = B["res"][0]
    assert d == k and why == capi.STOP_GAIN, (d, k, why)
    oP, ost = oracle_k(shape, k)
    assert ost["iters_done"] == k
    err = np.abs(B["poses"] - oP).max()
    rel = [abs(st[key][k] - ost[key][-1]) / ost[key][-1] for key in ("chi2", "robust_chi2")]
    print(f"{shape} tol {tol}: k* {k}, max pose difference {err:.3e}, relative chi2 difference {rel[0]:.3e} / {rel[1]:.3e}")
    assert err <= 1e-6 and max(rel) <= 1e-6, (err, rel)


@pytest.mark.parametrize("shape,tol", [(s, t) for s, t in CASES if s in FACTORED])
def test_factorisation_paths_leave_what_the_plain_call_of_k_leaves(shape, tol):
    B = until20(shape, tol)
    k = B["res"][0][0]
    C = plain_k(shape, k)
    assert C["res"][0][0] == k
    assert same_bits(B["poses"], C["poses"])
    assert same_bits(B["res"][0][1]["robust_chi2"], C["res"][0][1]["robust_chi2"])
    if B["mf"] is not None:
        for name in MF_ARRAYS:
            assert B["mf"][name].size > 0 and B["mf"][name].tobytes() == C["mf"][name].tobytes(), name
        assert list(B["mf"]["FLAGS"].ravel()[:4]) == [0, 0, 0, k]


@pytest.mark.parametrize("shape", SHAPES)
def test_identities(shape):
    A = plain20(shape)
    stA = A["res"][0][1]
    Z = until20(shape, 0.0)                                       # gain_tol = 0 never stops: the plain call
    d, st, why = Z["res"][0]
    assert d == 20 and why == capi.STOP_MAX_ITERS
    assert same_bits(st["chi2"], stA["chi2"]) and same_bits(st["robust_chi2"], stA["robust_chi2"])
    assert same_bits(Z["poses"], A["poses"])
    assert stA["robust_chi2"][1] > stA["robust_chi2"][2]          # the second gain is positive: any tolerance above it stops there
    R = run(shape, (("until", 1, 1.0),))
    assert R["res"][0][0] == 1 and R["res"][0][2] == capi.STOP_MAX_ITERS and len(R["res"][0][1]["chi2"]) == 2
    assert same_bits(R["res"][0][1]["robust_chi2"], stA["robust_chi2"][:2])
    R = run(shape, (("until", 2, 1e300),))                        # at least two updates, and the closing pass decides nothing
    assert R["res"][0][0] == 2 and R["res"][0][2] == capi.STOP_MAX_ITERS
    R = run(shape, (("until", 20, 1e300),))
    assert R["res"][0][0] == 2 and R["res"][0][2] == capi.STOP_GAIN
    assert same_bits(R["res"][0][1]["robust_chi2"], stA["robust_chi2"][:3])
    R = run(shape, (("until", 0, 1.0),))
    assert R["res"][0][0] == 0 and same_bits(R["res"][0][1]["robust_chi2"], stA["robust_chi2"][:1])


@pytest.mark.parametrize("shape", FACTORED)
def test_no_stop_word_is_left_behind(shape):
    tol = min(STOPS[shape])
    k = STOPS[shape][tol]
    U = run(shape, (("until", 20, tol), ("gn", 20)))
    T = run(shape, (("gn", k), ("gn", 20)))
    assert U["res"][0][0] == k and U["res"][1][0] == 20 == T["res"][1][0]
    for key in ("chi2", "robust_chi2"):
        assert same_bits(U["res"][1][1][key], T["res"][1][1][key]), key
    assert same_bits(U["poses"], T["poses"])
    if U["mf"] is not None:
        for name in MF_ARRAYS:
            assert U["mf"][name].tobytes() == T["mf"][name].tobytes(), name


def test_overlay_session_stops_as_its_twin_says():
    """The reference's flow: the graph optimised before + a chain of new poses + one closure (sgo_update_graph_se2 leaves an
    incremental overlay resident), then the call under test on the updated graph."""
    base, steps, gg = synth.append_session(2500, 10000, 1, 16, seed=5)
    st1 = steps[0]
    arrs = [np.concatenate([getattr(base, k), st1[k]]) for k in ("ei", "ej", "meas", "info", "phi")]
    fixed = np.zeros(st1["V"], dtype=bool)
    fixed[0] = True

    def session(call):
        with capi.Optimizer(0, direct_rows=0) as opt:
            opt.set_graph(*base.arrays())
            assert opt.optimize(5)[0] == 5
            P0 = np.empty((st1["V"], 3))
            P0[: base.V] = opt.get_poses()
            synth.chain_init(P0, gg.meas[: gg.V - 1], base.V, st1["V"] - 1)
            opt.update_graph(P0, fixed, *arrs, base.E)
            desc = opt.solver_description()
            assert "incremental overlay" in desc, desc
            out = call(opt)
            return dict(res=[out], poses=opt.get_poses(), chi2=opt.chi2())

    A = session(lambda opt: opt.optimize(20) + (None,))
    dA, stA, _ = A["res"][0]
    assert dA == 20
    r = stA["robust_chi2"]
    gains = [math.nan] + [(r[i - 1] - r[i]) / r[i] for i in range(1, 21)]
    pick = None
    for k in range(3, 20):      # a tolerance between two adjacent positive gains that makes the call stop before iteration k
        if gains[k - 1] > gains[k] > 0.0:
            tol = math.sqrt(gains[k - 1] * gains[k])
            if rule_stop(r, tol, 20) == k:
                pick = (k, tol)
                break
    if pick is None:
        pytest.skip(f"the twin's history has no two adjacent positive gains that make a stop with 2 < k* < 20: {gains[1:]}")
    k, tol = pick
    B = session(lambda opt: opt.optimize_until(20, tol))
    check_prefix(stA, B, k)
    st = B["res"][0][1]
    assert same_bits(list(B["chi2"]), [st["chi2"][k], st["robust_chi2"][k]]), (B["chi2"], st["chi2"][k], st["robust_chi2"][k])


def test_refusals_leave_the_poses_untouched():
    shape = (600, 620, 3)
    g = graph(shape)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        p0 = opt.get_poses()
        for args in ((20, math.nan), (20, math.inf), (20, -math.inf), (-1, 1e-6), (capi.SGO_MAX_ITERS + 1, 1e-6)):
            with pytest.raises(capi.SgoError, match="rc=-2"):
                opt.optimize_until(*args)
            assert same_bits(opt.get_poses(), p0), args
        d, st, why = opt.optimize_until(capi.SGO_MAX_ITERS, 1e-6)     # the upper end of the range is valid
        assert 2 <= d < 20 and why == capi.STOP_GAIN
    with capi.Optimizer(0, direct_rows=0) as opt:                   # the rank emulation of a multi-GPU context
        opt.debug_set_shard(2, 0)
        opt.set_graph(*g.arrays())
        p0 = opt.get_poses()
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.optimize_until(20, 1e-6)
        assert "multi-GPU" in opt.last_error()
        assert same_bits(opt.get_poses(), p0)


def test_terminate_action_through_the_shim_on_the_device(tmp_path):
    """tests/cpp/replay_until.cpp: VertexSE2 / EdgeSE2 under Gauss-Newton plus a SparseOptimizerTerminateAction (threshold 1e-4);
    optimize(20) returns the oracle's stop iteration and leaves its estimate."""
    from test_shim_replay import _write_graph
    shape = (2500, 3400, 31)
    exe = str(tmp_path / "replay_until")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(CPP, "replay_until.cpp"), "-L" + LIBDIR, "-lsgo", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    g = graph(shape)
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 10.0)
    env = dict(os.environ)
    env.pop("SGO_DIRECT_ROWS", None)
    subprocess.check_call([exe, str(gf), str(of), "1e-4"], env=env)
    lines = open(of).read().split("\n")
    assert lines[1].startswith("multifrontal_cholesky"), lines[1]
    assert int(lines[0]) == 8 == STOPS[shape][1e-4]
    P = np.loadtxt(lines[2:2 + g.V])
    oP, _ = oracle_k(shape, 8)
    assert np.abs(P - oP).max() <= 1e-6, np.abs(P - oP).max()


def test_mixed_kernel_kinds_on_the_multifrontal_path():
    """test_gpu_robust_kernels._mixed's kinds (all nine on the closures, delta = 1.5): k_mf_gain_stop reads the robust chi2 the edge
    kernel's KINDS instantiation summed.  The call is a prefix of the plain call bit for bit, stops where the rule says on the plain
    call's history and on the reference's (robust_reference.gauss_newton; gains 1.5e-3 before the stop and 3e-5 at it, tolerance
    5e-4), and leaves the poses and sgo_chi2 of the plain call cut at that count."""
    import robust_reference as rr
    from oracle import c_oracle
    from test_gpu_robust_kernels import _mixed
    shape, tol = (2500, 3400, 31), 5e-4
    g = graph(shape)
    kind, delta = _mixed(g)

    def ctx():
        opt = capi.Optimizer(0)
        opt.set_graph(*g.arrays())
        opt.set_robust_kernels(np.arange(g.E), kind, delta)
        assert opt.solver_description().startswith("multifrontal_cholesky"), opt.solver_description()
        return opt

    with ctx() as opt:
        dA, stA = opt.optimize(20)
    assert dA == 20
    k = rule_stop(stA["robust_chi2"], tol, 20)
    _, ref = rr.gauss_newton(c_oracle, g.poses, g, kind, delta, 20)
    assert 2 <= k < 20 and k == rule_stop(ref["robust_chi2"], tol, 20), (k, stA["robust_chi2"], ref["robust_chi2"])
    with ctx() as opt:
        B = dict(res=[opt.optimize_until(20, tol)], poses=opt.get_poses(), chi2=opt.chi2())
    check_prefix(stA, B, k)
    with ctx() as opt:
        dC, stC = opt.optimize(k)
        assert dC == k and same_bits(opt.get_poses(), B["poses"]) and opt.chi2() == B["chi2"]
    assert same_bits(stC["robust_chi2"], B["res"][0][1]["robust_chi2"]) and same_bits(stC["chi2"], B["res"][0][1]["chi2"])
    assert same_bits(list(B["chi2"]), [stC["chi2"][k], stC["robust_chi2"][k]])
