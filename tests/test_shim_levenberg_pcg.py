"""OptimizationAlgorithmLevenberg through the g2o-compatible header on a pose graph the multifrontal analysis refuses
(tests/cpp/replay_levenberg_pcg.cpp): 1100 poses (3297 unknowns, above the dense host solver's size) with four edges per pose.
sgo_optimize_lm returns SGO_ENOTHING for it; the header then calls sgo_optimize_lm_pcg instead of refusing, and optimize(8) is that
call bit for bit."""
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
    path = str(tmp_path_factory.mktemp("shim_lm_pcg") / "replay_levenberg_pcg")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", path,
                           os.path.join(CPP, "replay_levenberg_pcg.cpp"), "-L" + LIBDIR, "-lsgo", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return path


@pytest.mark.gpu
def test_a_dense_large_pose_graph_takes_the_pcg_route(exe, tmp_path):
    V, E, iters = 1100, 4400, 8
    g = synth.manhattan(V, E, seed=7, info_mode="full", init="incremental")
    g.phi[:] = -1.0
    g.poses = lr.perturbed(g, 1.0)
    assert 3 * (V - 1) > 3000 and E == 4 * V
    ref = lr.levenberg(*g.arrays(), iters)
    assert ref["iters_done"] == iters
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 1.0)
    env = dict(os.environ)
    for k in ("SGO_DIRECT_ROWS", "SGO_INCREMENTAL", "SGO_SOLVER", "SGO_MFRONT", "SGO_MFRONT_ROWS"):
        env.pop(k, None)
    r = subprocess.run([exe, str(gf), str(of), str(iters)], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = open(of).read().split("\n")
    its, factor, abi, trace_equal, poses_equal = map(int, lines[0].split())
    desc, desc_abi, n = lines[1], lines[2], int(lines[3])
    trace = [(float(a), float(b), int(c)) for a, b, c in (ln.split() for ln in lines[4:4 + n])]
    assert factor == -1                                           # sgo_optimize_lm still refuses the graph
    assert its == abi == n == iters and trace_equal == 1 and poses_equal == 1
    chi2 = [t[1] for t in trace]
    assert all(a >= b for a, b in zip(chi2, chi2[1:])), chi2
    # the backend is unchanged in kind: the PCG context the graph had before, and the C-ABI context's description
    assert desc.startswith("pcg_amg") and "multifrontal path not used" in desc and desc == desc_abi, (desc, desc_abi)
    assert [t[2] for t in trace] == ref["trials"]
    assert np.allclose(chi2, ref["robust_chi2"][1:], rtol=1e-6, atol=0.0)
