"""The table of robust kernels (tests/robust_reference.py, written from include/sgo.h's) against itself and against the host
robustify of the g2o-compat header's classes.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import robust_reference as rr
from oracle import np_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
EPS = np.finfo(np.float64).eps
DELTAS = (0.5, 1.5, 3.0)


def _grid():
    """e from deep inside every kind's quadratic region to far outside it, for every delta"""
    e = np.concatenate([np.geomspace(1e-3, 60.0, 400), np.random.default_rng(3).uniform(0.0, 40.0, 400)])
    return [(d, e) for d in DELTAS]


@pytest.mark.parametrize("kind", [k for k in range(10) if k != rr.DCS], ids=lambda k: rr.NAMES[k])
def test_the_weight_is_the_derivative_of_rho0(kind):
    """rho1 = d rho0 / d e by central differences with h = 1e-4 e: truncation h^2 |rho0'''| / 6 <= 1e-8 (|rho0'''| e^2 <= 1 for every
    kind here), rounding <= 4 EPS max(e, d^2) / h <= 1e-10: 1e-6 absolute on a weight in [0, 1] leaves two digits of slack.  (g2o's
    DCS pair is not a derivative pair.)  Samples within 2 h of a branch threshold are left out."""
    for d, e in _grid():
        h = 1e-4 * e
        t = rr.threshold(kind, d)
        keep = np.ones(e.size, dtype=bool) if t is None else np.abs(e - t) > 2 * h
        e, h = e[keep], h[keep]
        num = (rr.rho(kind, e + h, d)[0] - rr.rho(kind, e - h, d)[0]) / (2 * h)
        assert np.abs(num - rr.rho(kind, e, d)[1]).max() <= 1e-6, (rr.NAMES[kind], d)


@pytest.mark.parametrize("kind", rr.PIECEWISE, ids=lambda k: rr.NAMES[k])
def test_rho0_is_continuous_at_the_threshold(kind):
    """the two branches one ulp either side of the threshold: rho0's slope is at most 1 there, so the values differ by at most the
    spacing of e plus the rounding of each branch's few operations on numbers of size max(t, d^2)"""
    for d in DELTAS:
        t = float(rr.threshold(kind, d))
        lo, hi = np.nextafter(t, 0.0), np.nextafter(t, np.inf)
        r = [rr.rho(kind, np.array([x]), d)[0][0] for x in (lo, t, hi)]
        assert max(r) - min(r) <= 16 * EPS * max(t, d * d), (rr.NAMES[kind], d, r)


def test_the_dcs_row_is_the_oracles_bit_for_bit():
    rng = np.random.default_rng(5)
    e = np.concatenate([rng.uniform(0, 50, 2000), [0.0, 1.0, 0.75]])
    for phi in (0.0, 0.75, 1.0, 10.0):
        a, b = rr.rho(rr.DCS, e, phi), np_oracle.dcs_rho(e, phi)
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    a, b = rr.rho(rr.NONE, e, 1.0), np_oracle.dcs_rho(e, -1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_an_edge_without_information_has_weight_one_under_every_kind():
    for kind in range(10):
        for d in DELTAS:
            r0, w = rr.rho(kind, np.zeros(3), d)
            assert np.all(r0 == 0.0) and np.all(w == 1.0), rr.NAMES[kind]
    kinds = np.arange(10)
    r0, w = rr.rho_mixed(kinds, np.zeros(10), np.where(kinds == rr.NONE, -1.0, 1.5))
    assert np.all(r0 == 0.0) and np.all(w == 1.0)


def test_the_compat_headers_robustify_agrees_with_the_table(tmp_path):
    """Every class's host robustify on the grid, thresholds included.  Both sides evaluate the same expressions in fp64; they
    may differ in sqrt / log / exp / log1p of the two maths libraries (an ulp each) on intermediates no larger than
    m = max(e, 2 d^2, 2 s d): 4 EPS m on rho0 -- a few ulp of the operands, not of a difference that cancels -- and 4 EPS on the weight."""
    exe = str(tmp_path / "robust_kernels")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(CPP, "robust_kernels.cpp"), "-L" + LIBDIR, "-lsgo", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    rows = []
    for kind in range(rr.DCS, 10):
        for d, e in _grid():
            t = rr.threshold(kind, d)
            ee = e if t is None else np.concatenate([e, [np.nextafter(t, 0.0), t, np.nextafter(t, np.inf)]])
            rows += [(kind, d, x) for x in np.concatenate([ee, [0.0]])]
    with open(tmp_path / "s.txt", "w") as f:
        for k, d, x in rows:
            f.write(f"{k} {d!r} {float(x)!r}\n")
    subprocess.check_call([exe, str(tmp_path / "s.txt"), str(tmp_path / "o.txt")])
    got = np.loadtxt(tmp_path / "o.txt")
    kind, d, e = (np.array(c) for c in zip(*rows))
    assert got.shape == (len(rows), 3)
    r0, w = rr.rho_mixed(kind.astype(int), e, d)
    m = np.maximum(np.maximum(e, 2 * d * d), 2 * np.sqrt(e) * d)
    worst0, worst1 = np.abs(got[:, 0] - r0) / (EPS * m), np.abs(got[:, 1] - w) / EPS
    print("worst rho0 / (EPS m):", worst0.max(), " worst weight / EPS:", worst1.max())
    assert worst0.max() <= 4.0, (worst0.max(), rows[int(worst0.argmax())])
    assert worst1.max() <= 4.0, (worst1.max(), rows[int(worst1.argmax())])
    assert np.all(np.isfinite(got[:, 2]))
