#!/usr/bin/env python3
"""Records what the reference's own rho-theta edge and vertex compute, for tests/test_landmark_lm.py:

    python scripts/make_golden_ref_rhotheta.py <reference checkout>     (libsgo.so built first: __graft_entry__.build())

The reference's src/g2o_bindings/{edge_se2_rhotheta,vertex_rhotheta}.cpp -- and through them ls_extractor/utils.h -- are
compiled verbatim from the checkout against the compat headers (the only stand-in is tests/ref_stub/boost/array.hpp =
std::array, for two covariance helpers the path never calls) and linked with two programs:
  tests/cpp/ref_sources_check.cpp -DSGO_REF_SOURCES   their computeError on 2000 pose / line pairs
  tests/cpp/landmark_rhotheta.cpp -DSGO_REF_SOURCES   the golden LM schedule (tests/golden/lm_landmark_graph.txt) through THEIR
                                                      computeError / oplusImpl
Both outputs go to tests/golden/ref_rhotheta.npz (`error`: 2000 x 2, `landmark_stdout`: the program's lines).  (src/graphs.cpp
is not built: graphs.h pulls in pose_with_observation.h -> Cartographer + ROS message headers; its two set-up functions are what
tests/cpp/replay_posegraph.cpp and landmark_graph.cpp spell out.)

It also checks that the reference's custom-type declarations (include/g2o_bindings/*.h) are accepted by the compat headers and
go through a Levenberg-configured SparseOptimizer (tests/cpp/ref_headers_check.cpp: subclass ABI of SURVEY.md section 2 row 6).
Nothing of the checkout is copied: the fixture holds numbers only.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLD = os.path.join(ROOT, "tests", "golden")
LIBDIR = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
LINK = ["-L" + LIBDIR, "-lsgo", "-L/opt/rocm/lib", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]


def main(ref_root: str) -> None:
    src = os.path.join(ref_root, "src")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "eigen_stub"),
           "-I" + os.path.join(ROOT, "tests", "ref_stub"), "-I" + os.path.join(src, "sparse_gslam", "include"),
           "-I" + os.path.join(src, "ls_extractor", "include")]
    with tempfile.TemporaryDirectory() as tmp:
        objs = []
        for name in ("edge_se2_rhotheta", "vertex_rhotheta"):
            o = os.path.join(tmp, name + ".o")
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-c", os.path.join(src, "sparse_gslam", "src", "g2o_bindings", name + ".cpp"),
                                   "-o", o] + inc)
            objs.append(o)
        chk = os.path.join(tmp, "ref_sources_check")
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-DSGO_REF_SOURCES", os.path.join(CPP, "ref_sources_check.cpp")] + objs + inc +
                              LINK + ["-o", chk])
        err = np.loadtxt(subprocess.run([chk], capture_output=True, text=True, check=True).stdout.splitlines())
        exe = os.path.join(tmp, "landmark_ref")
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-DSGO_REF_SOURCES", os.path.join(CPP, "landmark_rhotheta.cpp")] + objs + inc +
                              LINK + ["-o", exe])
        out = subprocess.run([exe, os.path.join(GOLD, "lm_landmark_graph.txt")], capture_output=True, text=True, check=True).stdout
        hdr = os.path.join(tmp, "ref_headers_check")
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "tests", "eigen_stub"), "-I" + os.path.join(src, "sparse_gslam", "include"),
                               os.path.join(CPP, "ref_headers_check.cpp")] + LINK + ["-o", hdr])
        r = subprocess.run([hdr], capture_output=True, text=True)
        its, chi2 = r.stdout.split()[:2]
        assert r.returncode == 0 and int(its) >= 1 and float(chi2) < 1e-12, r.stdout + r.stderr
    assert err.shape == (2000, 2)
    np.savez(os.path.join(GOLD, "ref_rhotheta.npz"), error=err, landmark_stdout=np.array(out.splitlines()))
    print(f"wrote tests/golden/ref_rhotheta.npz: {err.shape[0]} errors, {len(out.splitlines())} lines of the LM schedule; "
          f"the reference's headers passed the compat check ({its} iterations, chi2 {chi2})")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
