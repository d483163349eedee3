"""OptimizationAlgorithmDogleg through the g2o-compatible header (tests/cpp/replay_dogleg.cpp, compiled here): on a pose graph the
multifrontal analysis takes optimize() is the library's sgo_optimize_dogleg, on one it refuses (four edges per pose) the header calls
sgo_optimize_dogleg_pcg instead of refusing -- in both cases the C-ABI's call bit for bit: iterations, the trace (delta, robust chi2,
trials, step kind) and the estimates.  The graphs and starts are tests/test_gpu_dogleg*.py's, whose first iterations reject trials."""
import os
import subprocess

import pytest

import lm_reference as lr
from sparse_gslam_amd import synth
from test_shim_replay import _write_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "sparse_gslam_amd", "csrc")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("shim_dogleg") / "replay_dogleg")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", path,
                           os.path.join(CPP, "replay_dogleg.cpp"), "-L" + LIBDIR, "-lsgo", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return path


def _run(exe, tmp_path, V, E, seed, sigma, iters):
    g = synth.manhattan(V, E, seed, info_mode="full", init="incremental")
    g.phi[:] = -1.0
    g.poses = lr.perturbed(g, sigma)
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 1.0)
    env = dict(os.environ)
    for k in ("SGO_DIRECT_ROWS", "SGO_INCREMENTAL", "SGO_SOLVER", "SGO_MFRONT", "SGO_MFRONT_ROWS"):
        env.pop(k, None)
    r = subprocess.run([exe, str(gf), str(of), str(iters)], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = open(of).read().split("\n")
    its, factor, abi, trace_equal, poses_equal = map(int, lines[0].split())
    n = int(lines[2])
    trace = [(float(a), float(b), int(c), int(d)) for a, b, c, d in (ln.split() for ln in lines[3:3 + n])]
    return its, factor, abi, trace_equal, poses_equal, lines[1], trace


@pytest.mark.parametrize("V,E,seed,sigma,iters,refused", [(300, 400, 2, 2.0, 8, False), (1000, 4000, 5, 1.0, 6, True)])
def test_optimize_is_the_librarys_dogleg(exe, tmp_path, V, E, seed, sigma, iters, refused):
    its, factor, abi, trace_equal, poses_equal, desc, trace = _run(exe, tmp_path, V, E, seed, sigma, iters)
    assert (factor == -1) == refused, (factor, desc)
    assert desc and (not refused or "multifrontal path not used" in desc), desc
    assert its == abi == len(trace) == iters
    assert trace_equal == 1 and poses_equal == 1
    chi2 = [t[1] for t in trace]
    assert all(a >= b for a, b in zip(chi2, chi2[1:])), chi2
    assert sum(t[2] for t in trace) > iters and trace[0][2] > 1          # (the first iteration rejects trials)
    assert all(t[3] in (0, 1, 2) for t in trace)
