"""The g2o-compat C++ shim (include/g2o/...) driven with sparse-gslam's own call sequences.

CPU part: the replay program compiles with the reference's language level (-std=c++14) against the
compat headers and links libsgo.so.  GPU part: it runs the sequences of
submap_loop_closer.cpp:205-288 and log_runner.cpp:182-204 and must agree with the CPU oracle
following the same steps (optimize(20); chi2 > 11.345 gate; optimize(20))."""
import os
import subprocess

import numpy as np
import pytest

from sparse_gslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "replay_posegraph")


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "replay_posegraph"])
    return EXE


def test_shim_compiles_as_cxx14_and_links_libsgo():
    exe = _build()
    assert os.access(exe, os.X_OK)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libsgo.so" in out and "not found" not in out.split("libsgo.so")[1].split("\n")[0]


def _write_graph(path, g, phi):
    with open(path, "w") as f:
        f.write(f"{g.V} {g.E} {phi!r}\n")
        np.savetxt(f, g.poses, fmt="%.17g")
        for k in range(g.E):
            row = [int(g.ei[k]), int(g.ej[k]), int(g.phi[k] >= 0)] + [repr(float(v)) for v in g.meas[k]] + \
                  [repr(float(v)) for v in g.info[k]]
            f.write(" ".join(map(str, row)) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("V,E", [(300, 700), (2500, 3400)])
def test_call_site_replay_matches_oracle(tmp_path, V, E):
    """The reference's call sequence through the g2o-compatible header (slc.cpp:205-288: build, initializeOptimization,
    optimize(20), chi2 gate at 11.345 with removeEdge, re-initialise, optimize(20)) on a graph that takes the multigrid
    path and on one of the size and closure density of the reference's largest (the multifrontal path)."""
    from oracle import c_oracle as co
    exe = _build()
    phi = 1.0
    g = synth.manhattan(V, E, seed=31, info_mode="full", phi=phi)
    # corrupt a few closures so that the 11.345 gate has something to remove
    rng = np.random.default_rng(0)
    bad = g.meta["n_odom"] + rng.choice(g.E - g.meta["n_odom"], size=12, replace=False)
    g.meas[bad, :2] += rng.normal(0, 3.0, (12, 2))
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, phi)
    subprocess.check_call([exe, str(gf), str(of), "gate"])
    lines = open(of).read().split("\n")
    it1, c1, r1, removed, it2, c2, r2 = lines[0].split()
    P = np.loadtxt(lines[1:1 + g.V])

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


def test_landmark_graph_types_run_on_the_host_solver():
    """The non-hot-path half of the surface (drone.cpp:146-187, graphs.cpp:9-15): user-defined 2-dof
    vertex + computeError-only edge (numeric Jacobians), Levenberg-Marquardt, push/pop/discardTop,
    updateInitialization.  Exact measurements => LM returns to the ground truth; an inconsistent
    observation raises chi2 and pop() restores the accepted estimates.  No GPU involved."""
    subprocess.check_call(["make", "-s", "-C", CPP, "landmark_graph"])
    out = subprocess.run([os.path.join(CPP, "landmark_graph")], capture_output=True, text=True, check=True).stdout.split()
    chi2_before, chi2_after, its, perr, lerr, chi2_bad, chi2_restored, dof = map(float, out)
    assert chi2_before > 10 and chi2_after < 1e-18 and 1 <= its <= 15
    assert perr < 1e-9 and lerr < 1e-9
    assert chi2_bad > 100 * max(chi2_after, 1e-20) and chi2_bad > 10
    assert chi2_restored < 1e-18
    assert dof == 7 * 3 + 20 * 2


def test_shim_container_semantics():
    """addVertex/addEdge/removeEdge/removeVertex return values, hessian order by id, upstream clear()
    semantics, push/pop, ownership -- SURVEY.md section 8(b) semantic notes (host only)."""
    subprocess.check_call(["make", "-s", "-C", CPP, "shim_semantics"])
    out = subprocess.run([os.path.join(CPP, "shim_semantics")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_cmake_find_module_resolves_g2o_to_this_backend(tmp_path):
    """cmake/FindG2O.cmake defines the variables sparse-gslam's CMakeLists consumes
    (find_package(G2O REQUIRED); G2O_*_LIBRARY list at src/sparse_gslam/CMakeLists.txt:235-243)."""
    import shutil
    if shutil.which("cmake") is None:
        pytest.skip("cmake not installed")
    build = tmp_path / "b"
    subprocess.check_call(["cmake", "-S", os.path.join(ROOT, "tests", "cmake_project"), "-B", str(build),
                           f"-DSGO_ROOT={ROOT}"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["cmake", "--build", str(build)], stdout=subprocess.DEVNULL)
    exe = build / "replay"
    assert exe.exists()
    out = subprocess.run(["ldd", str(exe)], capture_output=True, text=True).stdout
    assert "libsgo.so" in out and "not found" not in out


@pytest.mark.gpu
def test_loop_closer_growth_pattern_takes_the_incremental_update(tmp_path, monkeypatch):
    """slc.cpp:205-226 + :272-287 through the shim on a graph of the multigrid path's size: every optimize() after the first
    sees the previous graph as a prefix and goes through sgo_update_graph_se2 (the resident structures are kept); chi2 after
    each step and the final poses agree with the CPU oracle following the same steps."""
    from oracle import c_oracle as co
    monkeypatch.setenv("SGO_DIRECT_ROWS", "0")      # (graphs of this size would otherwise take the single-launch direct path)
    subprocess.check_call(["make", "-s", "-C", CPP, "replay_incremental"])
    iters, phi = 6, 1.0
    base, steps, g = synth.append_session(1500, 4500, 3, 12, seed=21, info_mode="full", phi=phi)

    def rows(ei, ej, ph, meas, info):
        return "".join(" ".join(map(str, [int(ei[k]), int(ej[k]), int(ph[k] >= 0)] + [repr(float(v)) for v in meas[k]] +
                                     [repr(float(v)) for v in info[k]])) + "\n" for k in range(len(ei)))
    sf, of = tmp_path / "s.txt", tmp_path / "o.txt"
    with open(sf, "w") as f:
        f.write(f"{base.V} {base.E} {len(steps)} {phi!r}\n")
        np.savetxt(f, base.poses, fmt="%.17g")
        f.write(rows(base.ei, base.ej, base.phi, base.meas, base.info))
        for st in steps:
            f.write(f"{st['V']} {len(st['ei'])}\n")
            f.write(rows(st["ei"], st["ej"], st["phi"], st["meas"], st["info"]))
    subprocess.check_call([os.path.join(CPP, "replay_incremental"), str(sf), str(of), str(iters)])
    lines = open(of).read().split("\n")
    # the CPU oracle through the same steps
    P, so = co.gauss_newton(*base.arrays(), iters=iters)
    arrs = [base.ei, base.ej, base.meas, base.info, base.phi]
    done, c, r = lines[0].split(" | ")[0].split()
    assert int(done) == iters and abs(float(c) - so["chi2"][-1]) <= 1e-6 * so["chi2"][-1]
    for k, st in enumerate(steps):
        arrs = [np.concatenate([a, st[n]]) for a, n in zip(arrs, ("ei", "ej", "meas", "info", "phi"))]
        P0 = np.empty((st["V"], 3))
        P0[: P.shape[0]] = P
        synth.chain_init(P0, g.meas[: g.V - 1], P.shape[0], st["V"] - 1)
        fixed = np.zeros(st["V"], dtype=bool)
        fixed[0] = True
        P, so = co.gauss_newton(P0, fixed, *arrs, iters=iters)
        head, desc = lines[k + 1].split(" | ")
        done, c, r = head.split()
        assert int(done) == iters
        assert abs(float(c) - so["chi2"][-1]) <= 1e-6 * so["chi2"][-1], (k, c, so["chi2"][-1])
        assert abs(float(r) - so["robust_chi2"][-1]) <= 1e-6 * so["robust_chi2"][-1]
        assert "incremental overlay" in desc, desc
    Pg = np.loadtxt(lines[len(steps) + 1: len(steps) + 1 + P.shape[0]])
    assert np.abs(Pg - P).max() <= 1e-6
