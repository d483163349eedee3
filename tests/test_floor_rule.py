"""The floor rule's measure (sparse_gslam_amd/csrc/sgo_rules.h: floor_backward_error, kFloorEta).  A solve that stops short of pcg_tol
is accepted -- its step applied, sgo_stats.pcg_converged = 2 -- when the backward error of its x on the Jacobi-scaled system,
eta = |S r| / (|S^-1 x| + |S b|) with S = diag(H)^-1/2 and r = b - H x, is <= 1e-12.  Checked here against plain numpy on the CPU
oracle's systems (oracle.np_oracle.linearize): agreement with a long-double restatement, invariance under one stiff row (which let a
cut-off solve through round 6's normwise measure), strictness against the exact scaled backward error, acceptance of direct
solutions, and rejection of degenerate diagonals.  The function is compiled with g++ behind a C shim (tests/cpp/floor_shim.cpp); no
GPU, no library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle
from sparse_gslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_ETA = 1e-12
CUTOFF = 8   # PCG iterations of a solve cut off far from its solution


@pytest.fixture(scope="module")
def floor_fn(tmp_path_factory):
    so = tmp_path_factory.mktemp("floor") / "libfloor_shim.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "sparse_gslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "floor_shim.cpp"), "-o", str(so)])
    f = ctypes.CDLL(str(so)).sgo_test_floor_backward_error
    f.restype = ctypes.c_double
    f.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4

    def eta(r, x, b, dblk6):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (r, x, b, dblk6)]
        n = arrs[3].shape[0]
        assert all(a.size == 3 * n for a in arrs[:3]) and arrs[3].shape == (n, 6)
        return f(n, *(a.ctypes.data for a in arrs))
    return eta


def with_prior(g, s, j):
    """g plus one edge from the fixed pose 0 to pose j that agrees with the current poses (zero error: b is unchanged), information
    s I, no robust kernel: a stiff row of H."""
    rel = np_oracle.se2_mul(np_oracle.se2_inv(g.poses[0:1]), g.poses[j:j + 1])
    return synth.Graph(g.poses, g.fixed, np.append(g.ei, 0).astype(g.ei.dtype), np.append(g.ej, j).astype(g.ej.dtype),
                       np.vstack([g.meas, rel]), np.vstack([g.info, [[s, 0.0, 0.0, s, 0.0, s]]]), np.append(g.phi, -1.0))


def system(g):
    assert g.fixed[0]
    H, b, _, _ = np_oracle.linearize(*g.arrays())
    n = b.size // 3
    rows = 3 * np.arange(n)
    # the diagonal blocks in S0.dblk's symmetric packing [00 01 02 11 12 22]
    dblk6 = np.stack([np.asarray(H[rows + p, rows + q]).ravel() for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
    return H.tocsr(), b, dblk6


def cutoff(H, b):
    x, it = np_oracle.solve_pcg(H, b, tol=0.0, maxit=CUTOFF)
    assert it == CUTOFF
    return x


def eta_longdouble(r, x, b, dblk6):
    """The scaled backward error with |S H S| taken as 1, in long double from the same double inputs."""
    d = np.asarray(dblk6, dtype=np.longdouble)[:, [0, 3, 5]].ravel()
    r, x, b = (np.asarray(a, dtype=np.longdouble) for a in (r, x, b))
    return float(np.sqrt(np.sum(r * r / d)) / (np.sqrt(np.sum(x * x * d)) + np.sqrt(np.sum(b * b / d))))


def eta_round6(H, b, x, dblk6):
    """Round 6's normwise measure, |r| / (2 max_i |D_i|_F |x| + |b|) (with the true residual here)."""
    d = dblk6
    dmax = np.sqrt(d[:, 0] ** 2 + 2 * d[:, 1] ** 2 + 2 * d[:, 2] ** 2 + d[:, 3] ** 2 + 2 * d[:, 4] ** 2 + d[:, 5] ** 2).max()
    return np.linalg.norm(b - H @ x) / (2.0 * dmax * np.linalg.norm(x) + np.linalg.norm(b))


@pytest.fixture(scope="module")
def c2():
    return synth.config("C2")


@pytest.mark.parametrize("name", ["C1", "C2"])
@pytest.mark.parametrize("info_mode", ["diag", "full"])
def test_the_measure_agrees_with_a_long_double_reference(floor_fn, name, info_mode):
    H, b, dblk6 = system(synth.config(name, info_mode=info_mode))
    for x in (cutoff(H, b), np_oracle.solve_direct(H, b)):
        r = b - H @ x
        ref = eta_longdouble(r, x, b, dblk6)
        got = floor_fn(r, x, b, dblk6)
        assert ref > 0.0
        assert abs(got - ref) <= 1e-12 * ref, (name, info_mode, got, ref)


def test_one_stiff_row_does_not_let_a_cut_off_solve_through(floor_fn, c2):
    """C2 plus a prior-like edge of information s I on pose 5000, s = 1e8 and 1e14: the scaled measure of an 8-iteration solve stays
    within 1 % of plain C2's (1.3e-2: rejected).  Round 6's normwise measure falls in proportion to s on the same systems and accepted
    the same solve at s = 1e14 -- the reason the rule changed."""
    H0, b0, d0 = system(c2)
    x0 = cutoff(H0, b0)
    eta0 = floor_fn(b0 - H0 @ x0, x0, b0, d0)
    old0 = eta_round6(H0, b0, x0, d0)
    assert eta0 > 1e-3 and old0 > 1e-6, (eta0, old0)
    falls = []
    for s in (1e8, 1e14):
        H, b, d = system(with_prior(c2, s, 5000))
        x = cutoff(H, b)
        assert np.linalg.norm(b - H @ x) > 1e-2 * np.linalg.norm(b)   # far from its solution
        eta = floor_fn(b - H @ x, x, b, d)
        assert abs(eta - eta0) <= 0.01 * eta0, (s, eta, eta0)
        old = eta_round6(H, b, x, d)
        falls.append(old0 / old / s)
    assert abs(falls[1] / falls[0] - 1.0) <= 0.01, falls   # old0 / old = const * s
    assert old <= FLOOR_ETA < old0, (old, old0)            # s = 1e14: accepted by round 6's measure, rejected by the new one


def test_the_measure_errs_on_the_strict_side(floor_fn):
    """On C1 (3 000 unknowns: a dense eigenvalue problem is affordable) the measure is at least the exact scaled normwise backward
    error |S r| / (|S H S|_2 |S^-1 x| + |S b|): |S H S|_2 >= 1, taken as 1."""
    import scipy.linalg
    for info_mode in ("diag", "full"):
        H, b, dblk6 = system(synth.config("C1", info_mode=info_mode))
        s = 1.0 / np.sqrt(dblk6[:, [0, 3, 5]].ravel())
        A = (H.toarray() * s[:, None]) * s[None, :]
        nrm = scipy.linalg.eigvalsh(A, subset_by_index=[A.shape[0] - 1, A.shape[0] - 1])[0]
        assert nrm >= 1.0
        for x in (cutoff(H, b), np_oracle.solve_direct(H, b)):
            r = b - H @ x
            exact = np.linalg.norm(s * r) / (nrm * np.linalg.norm(x / s) + np.linalg.norm(s * b))
            assert floor_fn(r, x, b, dblk6) >= exact, info_mode


def test_a_direct_solution_is_at_the_floor(floor_fn, c2):
    """A backward-stable solver's answer passes, stiff row or not."""
    for g in (synth.config("C1"), synth.config("C1", info_mode="full"), c2, with_prior(c2, 1e14, 5000)):
        H, b, dblk6 = system(g)
        x = np_oracle.solve_direct(H, b)
        eta = floor_fn(b - H @ x, x, b, dblk6)
        assert eta <= 1e-14, eta


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
@pytest.mark.parametrize("entry", [0, 3, 5])
def test_a_degenerate_diagonal_is_not_accepted(floor_fn, bad, entry):
    H, b, dblk6 = system(synth.config("C1"))
    x = np_oracle.solve_direct(H, b)
    r = b - H @ x
    assert floor_fn(r, x, b, dblk6) <= 1e-14
    d = dblk6.copy()
    d[417, entry] = bad
    assert floor_fn(r, x, b, d) == 1.0


def test_a_non_finite_result_is_not_accepted(floor_fn):
    H, b, dblk6 = system(synth.config("C1"))
    x = np_oracle.solve_direct(H, b)
    r = b - H @ x
    for v, vec in ((np.nan, "r"), (np.inf, "r"), (np.nan, "x"), (np.nan, "b")):
        a = dict(r=r.copy(), x=x.copy(), b=b.copy())
        a[vec][100] = v
        assert floor_fn(a["r"], a["x"], a["b"], dblk6) == 1.0, (v, vec)
    z = np.zeros_like(b)
    assert floor_fn(z, z, z, dblk6) == 1.0   # (0 / 0)
