"""The case list of the PCG reference (tests/pcg_reference.py): small graphs, each with the shape it exists for, shared by the CPU
tests (fp64 model, mutations) and the GPU tests.  A case is a graph (arrays as sgo_set_graph_se2's), the solver it runs under
and the iteration caps whose states are exported; n = free poses (vertex 0 is fixed)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from sparse_gslam_amd import synth

BJ, AMG = 0, 1                       # capi.SOLVER_PCG_BJ, capi.SOLVER_PCG_AMG
SIG = np.array([synth.SIGMA_XY, synth.SIGMA_XY, synth.SIGMA_TH])
INFO = np.array([1 / SIG[0] ** 2, 0.0, 0.0, 1 / SIG[1] ** 2, 0.0, 1 / SIG[2] ** 2])


@dataclass
class Case:
    name: str
    arrays: tuple
    solver: int = BJ
    caps: tuple = (0, 1, 2, 3)
    env: dict = field(default_factory=dict)
    expect: dict = field(default_factory=dict)

    @property
    def n(self):
        return int((~np.asarray(self.arrays[1], dtype=bool)).sum())


def chain(n, seed=0, closures=None, scale=None):
    """n free poses behind a fixed one: odometry + `closures` (default n // 3) loop closures with a DCS kernel, poses near the truth.
    scale(V) -> per-vertex factors: an edge's information is multiplied by the factor of its first vertex."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    V = n + 1
    truth = synth._walk(V, rng)
    ei = np.arange(V - 1)
    ej = ei + 1
    nc = n // 3 if closures is None else closures
    if nc and V > 3:
        a = rng.integers(0, V - 2, nc)
        b = np.minimum(V - 1, a + 2 + rng.integers(0, max(V // 2, 1), nc))
        ei, ej = np.r_[ei, a], np.r_[ej, b]
    E = ei.size
    meas = synth._rel(truth[ei], truth[ej]) + rng.standard_normal((E, 3)) * SIG
    meas[:, 2] = synth._wrap(meas[:, 2])
    info = np.tile(INFO, (E, 1))
    if scale is not None:
        info = info * np.asarray(scale(V), dtype=np.float64)[ei][:, None]
    phi = np.r_[np.full(V - 1, -1.0), np.full(E - (V - 1), 1.0)]
    poses = truth + rng.standard_normal((V, 3)) * np.array([0.02, 0.02, 0.005])
    poses[0] = truth[0]
    fixed = np.zeros(V, dtype=bool)
    fixed[0] = True
    return (poses, fixed, ei.astype(np.int32), ej.astype(np.int32), meas, info, phi)


def scaled(n=86):
    """rows scaled by 10^+-6 through the information: alternating blocks of 16 vertices"""
    return chain(n, seed=5, scale=lambda V: 10.0 ** np.where((np.arange(V) // 16) % 2 == 0, 6.0, -6.0))


def lattice(n=30):
    """poses on the integer lattice along x, theta = 0, measurements exact differences: every error is exactly zero, so b == 0"""
    V = n + 1
    poses = np.zeros((V, 3))
    poses[:, 0] = np.arange(V)
    ei = np.r_[np.arange(V - 1), np.arange(0, V - 5, 3)]
    ej = np.r_[np.arange(1, V), np.arange(0, V - 5, 3) + 5]
    meas = np.zeros((ei.size, 3))
    meas[:, 0] = (ej - ei).astype(np.float64)
    fixed = np.zeros(V, dtype=bool)
    fixed[0] = True
    return (poses, fixed, ei.astype(np.int32), ej.astype(np.int32), meas, np.tile(INFO, (ei.size, 1)), np.full(ei.size, -1.0))


def negative_information():
    """one free pose on one edge of negative information: H is negative definite, p.Hp < 0 in the first iteration"""
    poses, fixed, ei, ej, meas, info, phi = chain(1, seed=9)
    return (poses, fixed, ei, ej, meas, -info, phi)


def large_chain():
    """530 000 poses, chain-like: the only shape with n > 2048 * 256 rows (kMaxGrid workgroups, second grid-stride trip)"""
    return synth.manhattan(530_000, 600_000, seed=3).arrays()


def c2():
    return synth.config("C2").arrays()


def small_amg():
    """<= 400 poses under the multigrid: a single level, inverted densely -- the preconditioner is the exact inverse"""
    return synth.manhattan(300, 900, seed=17, info_mode="full").arrays()


SIZES = (1, 2, 85, 86, 255, 256, 257)
CASES = {f"bj_n{n}": (lambda n=n: Case(f"bj_n{n}", chain(n))) for n in SIZES}
CASES["bj_scaled_rows"] = lambda: Case("bj_scaled_rows", scaled())
CASES["bj_lattice_b0"] = lambda: Case("bj_lattice_b0", lattice(), caps=(0, 1), expect=dict(stop=1, iters=0))
CASES["bj_large_chain"] = lambda: Case("bj_large_chain", large_chain(), caps=(0, 1, 2, 3), expect=dict(grid=2048))
CASES["amg_c2"] = lambda: Case("amg_c2", c2(), solver=AMG)
CASES["amg_c2_kcycle"] = lambda: Case("amg_c2_kcycle", c2(), solver=AMG, env=dict(SGO_AMG_KDEPTH="2"), expect=dict(zq=True))
CASES["amg_exact_coarse"] = lambda: Case("amg_exact_coarse", small_amg(), solver=AMG, caps=(0, 1, 2), expect=dict(iters=1))
CPU_CASES = [f"bj_n{n}" for n in SIZES] + ["bj_scaled_rows", "bj_lattice_b0"]


def case(name) -> Case:
    return CASES[name]()
