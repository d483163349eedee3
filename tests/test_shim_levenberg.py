"""OptimizationAlgorithmLevenberg through the g2o-compatible header on pose graphs (tests/cpp/replay_levenberg.cpp): above the dense
host solver's size -- 1200 poses, 3597 unknowns -- optimize() is the library's sgo_optimize_lm, bit for bit; the same generator's
900-pose graph (2697 unknowns) still takes the host solver, with the trace tests/lm_reference.py gives; and with a
SparseOptimizerTerminateAction registered the large graph is refused with one line that says why."""
import os
import subprocess

import numpy as np
import pytest

import lm_reference as lr
from sparse_gslam_amd import synth
from test_shim_replay import _write_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "sparse_gslam_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("shim_lm") / "replay_levenberg")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", path,
                           os.path.join(CPP, "replay_levenberg.cpp"), "-L" + LIBDIR, "-lsgo", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return path


def _graph(V, E, sigma):
    g = synth.manhattan(V, E, seed=7, info_mode="full", init="incremental")
    g.phi[:] = -1.0
    g.poses = lr.perturbed(g, sigma)
    return g


def _run(exe, tmp_path, g, iters, *more, direct_rows=None):
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 1.0)
    env = dict(os.environ)
    env.pop("SGO_DIRECT_ROWS", None)
    if direct_rows is not None:
        env["SGO_DIRECT_ROWS"] = str(direct_rows)
    r = subprocess.run([exe, str(gf), str(of), str(iters), *more], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = open(of).read().split("\n")
    its, abi, trace_equal, poses_equal = map(int, lines[0].split())
    n = int(lines[2])
    trace = [ln.split() for ln in lines[3:3 + n]]
    _run.grown = lines[3 + n] if len(lines) > 3 + n else ""
    return its, abi, trace_equal, poses_equal, lines[1], [(float(a), float(b), int(c)) for a, b, c in trace], r.stderr


@pytest.mark.gpu
def test_a_large_pose_graph_takes_the_librarys_levenberg(exe, tmp_path):
    g = _graph(1200, 1400, 2.0)
    iters = 6
    ref = lr.levenberg(*g.arrays(), iters)
    its, abi, trace_equal, poses_equal, desc, trace, err = _run(exe, tmp_path, g, iters)
    assert desc and err == "", (desc, err)
    assert its == abi == len(trace) == iters
    assert trace_equal == 1 and poses_equal == 1
    assert [t[2] for t in trace] == ref["trials"]
    assert np.allclose([t[1] for t in trace], ref["robust_chi2"][1:], rtol=1e-6, atol=0.0)


def test_a_graph_the_host_solver_holds_stays_on_the_host_solver(exe, tmp_path):
    g = _graph(900, 1050, 1.0)
    ref = lr.levenberg(*g.arrays(), 1)
    its, abi, _, _, desc, trace, err = _run(exe, tmp_path, g, 1)
    assert desc == "" and abi == -99 and err == ""        # no context was made
    assert its == 1 and [t[2] for t in trace] == ref["trials"] == [1]
    assert abs(trace[0][0] - ref["lam"][0]) <= 1e-6 * ref["lam"][0] and abs(trace[0][1] - ref["robust_chi2"][1]) <= 1e-6 * ref["robust_chi2"][1]


def test_a_terminate_action_keeps_the_large_graph_refused(exe, tmp_path):
    g = _graph(1200, 1400, 2.0)
    its, abi, _, _, desc, trace, err = _run(exe, tmp_path, g, 6, "terminate")
    assert its == 0 and abi == -99 and desc == "" and trace == []
    lines = [ln for ln in err.split("\n") if ln.strip()]
    assert len(lines) == 1 and "SparseOptimizerTerminateAction" in lines[0] and "refusing" in lines[0], err


@pytest.mark.gpu
def test_a_graph_that_grew_under_gauss_newton_gets_a_full_set_up(exe, tmp_path):
    """On a PCG context a graph that grew by a chain and a closure carries an incremental overlay, which sgo_optimize_lm refuses: the
    Levenberg route of the header gives it the full set-up instead of refusing."""
    g = synth.manhattan(1200, 1400, seed=7, info_mode="full", init="incremental")
    g.phi[:] = -1.0
    V0 = 1180
    late = np.flatnonzero((np.maximum(g.ei, g.ej) >= V0) & (np.abs(g.ei - g.ej) > 1))
    g = g.subset(np.isin(np.arange(g.E), late[1:], invert=True))     # (the new poses' chain and one closure)
    its, abi, _, _, desc, trace, err = _run(exe, tmp_path, g, 3, "grow", str(V0), direct_rows=0)
    assert "incremental overlay" in _run.grown, _run.grown
    assert err == "" and its == 3 == len(trace) and abi == -99
    assert desc and "incremental overlay" not in desc
    assert all(a[1] >= b[1] for a, b in zip(trace, trace[1:]))
