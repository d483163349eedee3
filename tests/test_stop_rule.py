"""The gain rule of sgo_optimize_gn_until (rules::gain_stop, sparse_gslam_amd/csrc/sgo_rules.h; g2o's
SparseOptimizerTerminateAction): before iteration `it` with 2 <= it < max_iters the call stops iff the relative gain
(r[it - 1] - r[it]) / r[it] of the robust chi2 is in [0, gain_tol).  Here without a GPU: the exported pure function's truth table,
the stop iterations it gives on the CPU oracle's histories of the three graphs tests/test_gpu_optimize_until.py runs on the device,
and the compat header's action on the host solver."""
import math
import os
import subprocess

import pytest

from sparse_gslam_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "sparse_gslam_amd", "csrc")

# (V, E, seed) of synth.manhattan(info_mode="full", phi=10.0) -> {gain_tol: the iteration the rule stops before}; every deciding
# gain of the oracle's history is more than 1.5x away from its tolerance (the closest: 1.68x), so the device's
# rounding of chi2 (relative 1e-12 or so) cannot move a decision
STOPS = {
    (600, 620, 3): {0.5: 8, 1e-3: 12},
    (2500, 3400, 31): {5e-3: 7, 1e-4: 8},
    (3000, 12000, 7): {1e-3: 4, 1e-4: 6},
}


def walk(robust_chi2, gain_tol, max_iters):
    """the stop iteration of a history by the library's own rule"""
    for it in range(2, max_iters):
        if capi.gain_stop(robust_chi2[it - 1], robust_chi2[it], gain_tol):
            return it
    return max_iters


def test_gain_stop_truth_table():
    gs = capi.gain_stop
    assert gs(1.0005, 1.0, 1e-3) and not gs(1.002, 1.0, 1e-3)        # a positive gain below / above the tolerance
    assert gs(101.0, 100.0, 0.0100001) and not gs(101.0, 100.0, 0.01)   # gain == 0.01 exactly: the upper bound is open
    assert gs(3.0, 3.0, 1e-300) and gs(3.0, 3.0, 1.0)                 # gain exactly 0 stops for any tol > 0
    assert not gs(0.999, 1.0, 1.0) and not gs(1.0, 2.0, 1e300)        # a negative gain never stops
    for tol in (0.0, -0.0, -1.0, -math.inf):                          # tol <= 0 never stops
        assert not gs(3.0, 3.0, tol) and not gs(3.1, 3.0, tol) and not gs(2.9, 3.0, tol)
    for tol in (1e-6, 1.0, 1e300, math.inf):
        assert not gs(1.0, 0.0, tol) and not gs(0.0, 0.0, tol) and not gs(-1.0, 0.0, tol)   # cur == 0: inf or NaN
        for bad in (math.nan, math.inf, -math.inf):
            assert not gs(bad, 1.0, tol), (bad, tol)                  # (inf - 1) / 1 = inf is not < tol, inf included
            assert not gs(1.0, bad, tol), (bad, tol)
            assert not gs(bad, bad, tol)
    assert not gs(1.0, 1.0, math.nan) and not gs(2.0, 1.0, math.nan)
    assert gs(2.0, 1.0, math.inf)                                      # (the entry point refuses a non-finite tolerance itself)


@pytest.mark.parametrize("shape", sorted(STOPS))
def test_stop_iterations_on_the_cpu_oracles_histories(shape):
    from oracle import np_oracle
    V, E, seed = shape
    g = synth.manhattan(V, E, seed=seed, info_mode="full", phi=10.0)
    _, st = np_oracle.gauss_newton(*g.arrays(), iters=20)
    r = st["robust_chi2"]
    assert len(r) == 21
    for tol, k in STOPS[shape].items():
        assert walk(r, tol, 20) == k, (tol, [(r[i - 1] - r[i]) / r[i] for i in range(1, 21)])
        gain = (r[k - 1] - r[k]) / r[k]
        assert 0.0 <= 1.5 * gain < tol, (tol, gain)                   # the margin the table claims, on the side that stops ...
        for it in range(2, k):                                        # ... and on the side that does not
            gi = (r[it - 1] - r[it]) / r[it]
            assert gi < 0.0 or gi >= 1.5 * tol, (tol, it, gi)
    assert walk(r, 0.0, 20) == 20 and walk(r, 1e300, 20) == 2 and walk(r, 1.0, 2) == 2 and walk(r, 1.0, 1) == 1


def test_terminate_action_on_the_host_solver(tmp_path):
    """tests/cpp/terminate_action_host.cpp, built with the g++ line of tests/cpp/Makefile: optimize(50) with the action returns k < 50
    and leaves the estimates of optimize(k) without it; a foreign action class is refused."""
    exe = str(tmp_path / "terminate_action_host")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(CPP, "terminate_action_host.cpp"), "-L" + LIBDIR, "-lsgo", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    k, kb, diff, foreign_refused, once, removed, kc = out.stdout.split()
    assert 2 <= int(k) < 50 and int(kb) == int(k)
    assert float(diff) == 0.0
    assert foreign_refused == "1" and "only SparseOptimizerTerminateAction" in out.stderr
    assert len([ln for ln in out.stderr.split("\n") if ln.strip()]) == 1, out.stderr   # one line for the one refusal
    assert once == "1" and removed == "1"
    assert int(kc) == 2                                               # maxIterations = 1: stops after the iteration with index 1
