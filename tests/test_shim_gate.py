"""The closure gate through the g2o-compat shim without a new set-up: after removeEdge + initializeOptimization the shim finds the
device's edge records with some left out and deactivates those on the device (sgo_set_edge_information with zero rows) instead of
setting the graph up again.  tests/cpp/replay_gate.cpp follows log_runner.cpp:182-204; the CPU oracle follows the same steps."""
import os
import subprocess

import numpy as np
import pytest

from sparse_gslam_amd import synth
from test_shim_replay import _write_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "sparse_gslam_amd", "csrc")


@pytest.fixture(scope="module")
def replay_gate(tmp_path_factory):
    """replay_gate built once with the g++ line of tests/cpp/Makefile"""
    exe = str(tmp_path_factory.mktemp("replay_gate") / "replay_gate")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(CPP, "replay_gate.cpp"), "-L" + LIBDIR, "-lsgo", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_replay_gate_compiles_as_cxx14_and_links_libsgo(replay_gate):
    exe = replay_gate
    assert os.access(exe, os.X_OK)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libsgo.so" in out and "not found" not in out.split("libsgo.so")[1].split("\n")[0]


@pytest.mark.gpu
@pytest.mark.parametrize("V,E,seed,direct_rows,path", [(2500, 3400, 31, None, "multifrontal_cholesky"), (3000, 12000, 7, "0", "pcg_amg")])
@pytest.mark.parametrize("incremental", [True, False])
def test_the_gate_through_the_shim_keeps_the_set_up(replay_gate, tmp_path, V, E, seed, direct_rows, path, incremental):
    from oracle import c_oracle as co
    exe = replay_gate
    phi = 1.0
    g = synth.manhattan(V, E, seed=seed, info_mode="full", phi=phi)
    rng = np.random.default_rng(0)
    bad = g.meta["n_odom"] + rng.choice(g.E - g.meta["n_odom"], size=12, replace=False)
    g.meas[bad, :2] += rng.normal(0, 3.0, (12, 2))
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, phi)
    env = dict(os.environ)
    env.pop("SGO_DIRECT_ROWS", None)
    env.pop("SGO_INCREMENTAL", None)
    if direct_rows is not None:
        env["SGO_DIRECT_ROWS"] = direct_rows
    if not incremental:
        env["SGO_INCREMENTAL"] = "0"
    subprocess.check_call([exe, str(gf), str(of)], env=env)
    lines = open(of).read().split("\n")
    it1, c1, r1, removed, it2, c2, r2, setup1, setup2 = lines[0].split()
    desc1, desc2 = lines[1], lines[2]
    P = np.loadtxt(lines[3:3 + g.V])

    P1, s1 = co.gauss_newton(*g.arrays(), iters=20)
    assert int(it1) == 20 and abs(float(c1) - s1["chi2"][-1]) <= 1e-6 * s1["chi2"][-1]
    assert abs(float(r1) - s1["robust_chi2"][-1]) <= 1e-6 * s1["robust_chi2"][-1]
    e2 = co.edges(P1[g.ei], P1[g.ej], g.meas, g.info, g.phi)[3]
    keep = ~((g.phi >= 0) & (e2 > 11.345))
    assert int(removed) == int((~keep).sum()) > 0
    P2, s2 = co.gauss_newton(P1, g.fixed, g.ei[keep], g.ej[keep], g.meas[keep], g.info[keep], g.phi[keep], iters=20)
    assert int(it2) == 20
    assert abs(float(c2) - s2["chi2"][-1]) <= 1e-6 * s2["chi2"][-1]
    assert abs(float(r2) - s2["robust_chi2"][-1]) <= 1e-6 * s2["robust_chi2"][-1]
    assert np.abs(P - P2).max() <= 1e-6

    assert desc1.startswith(path), desc1
    if incremental:
        assert f"{int(removed)} edges inactive" in desc2 and desc2.startswith(path), desc2
        assert float(setup2) == float(setup1)       # (the context's last set-up is still the first one)
    else:
        assert "edges inactive" not in desc2, desc2   # today's route: a full set-up of the reduced graph
