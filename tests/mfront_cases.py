"""The cases of the multifrontal stage tests: the smallest graphs that reach every tile, panel and branch boundary of
sgo_mfront.hip's kernels (CPU only: tests/test_mfront_reference.py runs the fp64 model on them, tests/test_gpu_mfront_reference.py
the device).

A case = a graph (sgo_set_graph_se2's arrays; `poses` are P0), the environment it is set up under (SGO_MFRONT_LEAF and its
like: the same for the host plan and the device) and the SHAPE it is there for: a predicate on the front table that both tests
assert, so that a change of the generators or of the nested dissection cannot silently turn a case into another one.

Graphs: a trajectory `truth`, the odometry chain and the listed closures, measurements = the true relative poses + noise, P0 =
truth + N(0.02 m, 0.02 m, 0.005 rad) on the free poses -- the state the reference re-optimises from after a closure.  The
parameters (pose counts, leaf sizes) were found by searching capi.mfront_plan_arrays on the CPU; the comment of every group
says which kernel boundary it reaches.  Front sizes come in multiples of 3, so a front has m + 1 = 16, 19, 31, 34, 49 rows
where a tile boundary is wanted at 16, 17, 31, 33, 49 (17 and 33 do not exist: m = 16 and 32 are no multiples of 3).
"""
from __future__ import annotations

import os
from contextlib import contextmanager
from dataclasses import dataclass, field

import numpy as np

from sparse_gslam_amd import synth

SIG = np.array([0.05, 0.05, 0.01])


@dataclass
class Case:
    name: str
    poses: np.ndarray
    fixed: np.ndarray
    ei: np.ndarray
    ej: np.ndarray
    meas: np.ndarray
    info: np.ndarray
    phi: np.ndarray
    env: dict = field(default_factory=dict)
    shape: object = None                  # shape(T) -> dict of what the case is there for; every value must be truthy
    why: str = ""

    def arrays(self):
        return (self.poses, self.fixed, self.ei, self.ej, self.meas, self.info, self.phi)

    def as_dict(self):
        return dict(P0=self.poses, fixed=self.fixed, ei=self.ei, ej=self.ej, meas=self.meas, info=self.info, phi=self.phi)


@contextmanager
def environment(env):
    """The case's SGO_MFRONT_* knobs for the duration of a set-up (host plan or sgo_set_graph_se2)."""
    keys = ("SGO_MFRONT_LEAF", "SGO_MFRONT_DEGREE", "SGO_MFRONT_CRIT_MFLOP")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in env.items()})
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ------------------------------------------------------------------ the front table's shape
class Table:
    """The front table in the terms the shapes are declared in."""

    def __init__(self, X):
        F = np.asarray(X["FRONTS"], dtype=np.int64)
        self.own3, self.m, self.nb = F[:, 1], F[:, 2], F[:, 5]
        self.nb3 = self.m - self.own3
        self.kids = F[:, 7:9]
        self.parent = F[:, 13]
        self.nkids = (self.kids >= 0).sum(1)
        self.levels = int(X["INFO"][3])
        self.nf = F.shape[0]
        self.child_own3 = set(int(v) for v in self.own3[self.parent >= 0])
        self.rows = set(int(v) + 1 for v in self.m)
        self.fast = (self.own3 > 0) & (self.own3 <= 144) & (self.nb3 <= 256)
        self.generic = (self.own3 > 0) & ~self.fast
        T = np.asarray(X["TARGETS"], dtype=np.int64).reshape(-1, 4)
        cnt = T[:, 3] - T[:, 2]
        self.diag_counts = set(int(v) for v in cnt[T[:, 0] == T[:, 1]])
        self.off_counts = set(int(v) for v in cnt[T[:, 0] != T[:, 1]])
        self.parts = set(int(v) & 3 for v in X["CONTRIB"])
        held = []                       # per front with two children: how many children hold each local pose
        for f in range(self.nf):
            if self.nkids[f] == 2:
                n = int(self.m[f]) // 3
                held.append(sum((np.asarray(X["PINV"][int(F[f, 9 + k]):int(F[f, 9 + k]) + n]) >= 0).astype(int) for k in range(2)))
        self.held = np.concatenate(held) if held else np.zeros(0, dtype=int)


# ------------------------------------------------------------------ graphs
def line(V, step=1.0):
    """A gently curving path: a long thin chain."""
    i = np.arange(V, dtype=np.float64)
    th = 0.3 * np.sin(i / 9.0)
    x = np.cumsum(np.r_[0.0, step * np.cos(th[:-1])])
    y = np.cumsum(np.r_[0.0, step * np.sin(th[:-1])])
    return np.stack([x, y, th], axis=1)


def lattice(k):
    """k x k grid visited row by row, alternating direction (snake odometry); heading along the row."""
    r, c = np.divmod(np.arange(k * k), k)
    c = np.where(r % 2 == 0, c, k - 1 - c)
    th = np.where(r % 2 == 0, 0.0, np.pi - 1e-3)
    return np.stack([c.astype(np.float64), r.astype(np.float64), synth._wrap(th)], axis=1)


def lattice_rungs(k, every=1):
    """The vertical neighbours of the snake: with the odometry that is just below 2 edges per pose."""
    out = []
    for r in range(k - 1):
        for c in range(0, k, every):
            a = r * k + (c if r % 2 == 0 else k - 1 - c)
            b = (r + 1) * k + (c if (r + 1) % 2 == 0 else k - 1 - c)
            if abs(a - b) > 1:
                out.append((a, b))
    return out


def graph(name, truth, closures=(), fixed=(0,), seed=1, phi=10.0, env=None, shape=None, why="", odometry=None, info_scale=None,
          outliers=()):
    """Odometry chain (or the given `odometry` pairs) + closures (i, j), full information, noise of the matching covariance."""
    rng = np.random.default_rng(seed)
    V = truth.shape[0]
    od = [(i, i + 1) for i in range(V - 1)] if odometry is None else list(odometry)
    pairs = np.array(od + list(closures), dtype=np.int64).reshape(-1, 2)
    ei, ej = pairs[:, 0], pairs[:, 1]
    E = ei.size
    a, b, c = rng.uniform(-np.pi, np.pi, E), rng.uniform(-0.2, 0.2, E), rng.uniform(-0.2, 0.2, E)
    Q = synth._euler(a, b, c)
    noise = np.einsum("nij,nj->ni", Q, rng.standard_normal((E, 3)) * SIG)
    O = np.einsum("nij,j,nkj->nik", Q, 1.0 / SIG**2, Q)
    if info_scale is not None:
        O = O * np.asarray(info_scale, dtype=np.float64)[:, None, None]
    info = np.stack([O[:, 0, 0], O[:, 0, 1], O[:, 0, 2], O[:, 1, 1], O[:, 1, 2], O[:, 2, 2]], axis=1)
    meas = synth._rel(truth[ei], truth[ej]) + noise
    for q in outliers:                                   # closures that contradict the chain: DCS switches them off
        meas[len(od) + q, :2] += 3.0
    meas[:, 2] = synth._wrap(meas[:, 2])
    ph = np.full(E, -1.0)
    ph[len(od):] = phi
    fx = np.zeros(V, dtype=bool)
    fx[list(fixed)] = True
    poses = truth + rng.standard_normal((V, 3)) * np.array([0.02, 0.02, 0.005])
    poses[fx] = truth[fx]
    poses[:, 2] = synth._wrap(poses[:, 2])
    return Case(name, poses, fx, ei.astype(np.int32), ej.astype(np.int32), meas, info, ph, dict(env or {}), shape, why)


def walk(V, ncl, seed):
    """synth's Manhattan walk and `ncl` of its revisits as closures."""
    rng = np.random.default_rng(seed)
    truth = synth._walk(V, rng)
    ci, cj, _ = synth._closure_candidates(truth, ncl, 2.0, 10)
    pick = np.sort(rng.choice(ci.size, size=min(ncl, ci.size), replace=False))
    return truth, [(int(a), int(b)) for a, b in zip(ci[pick], cj[pick])]


# ------------------------------------------------------------------ the cases
def _root(own3):
    """One leaf front that is the root, nb = 0: 1 .. 4 panels of k_mf_panels, the last one wp = own3 % 16 wide."""
    return graph(f"root_own3_{own3}", line(own3 // 3 + 1), seed=own3,
                 shape=lambda T: dict(single_front=T.nf == 1, own3=int(T.own3[0]) == own3, no_boundary=int(T.nb[0]) == 0),
                 why=f"panel widths: {own3} = {own3 // 16} x 16 + {own3 % 16}")


# chain of V poses under SGO_MFRONT_LEAF = leaf: two leaves and a root of one pose; the larger leaf has own3 = K
_CHILD = {12: (4, 8), 15: (5, 10), 18: (6, 12), 33: (11, 22), 48: (16, 33), 66: (22, 45), 96: (32, 64), 99: (33, 66), 114: (38, 76)}


def _child(K):
    """The merge's K (mf_tile_dot's 64-, 32-, 16-step bodies and its masked tail) = a child's own3."""
    leaf, V = _CHILD[K]
    return graph(f"child_own3_{K}", line(V), seed=K, env=dict(SGO_MFRONT_LEAF=leaf),
                 shape=lambda T: dict(child_with_K=K in T.child_own3, two_levels=T.levels == 2),
                 why=f"k_mf_merge K = {K} = {K // 64} x 64 + {K % 64 // 32} x 32 + {K % 32 // 16} x 16 + {K % 16}")


def _rows(rows, leaf, V):
    return graph(f"rows_{rows}", line(V), seed=rows, env=dict(SGO_MFRONT_LEAF=leaf),
                 shape=lambda T: dict(front_with_rows=rows in T.rows), why=f"a front of m + 1 = {rows} rows: row m's place in the 16-row tiles")


def _tree_shapes():
    truth, cl = walk(40, 10, 3)
    return graph("tree_shapes", truth, cl, seed=3, env=dict(SGO_MFRONT_LEAF=4),
                 shape=lambda T: dict(parent_with_one_child=bool((T.nkids == 1).any()), pose_held_by_both_children=bool((T.held == 2).any()),
                                      pose_held_by_neither=bool((T.held == 0).any()), height_4=T.levels >= 5),
                 why="k_mf_merge: one child, a pose both children hold (two terms), a pose neither holds (zeros written)")


def _no_pivots():
    V = 40
    od = [(i, i + 1) for i in range(V - 1) if i != 19]
    return graph("front_without_pivots", line(V), fixed=(0, 20), odometry=od, seed=5, env=dict(SGO_MFRONT_LEAF=20),
                 shape=lambda T: dict(front_without_pivots=bool(((T.own3 == 0) & (T.nkids == 2)).any())),
                 why="two components with a fixed pose each: the root only merges")


def _contributions():
    cl = [(10, 30)] * 9 + [(12, 40), (40, 12), (12, 40), (40, 12), (12, 40)] + [(14, 45), (45, 14)] * 2 + [(16, 50)]
    cl += [(25, j) for j in (3, 8, 37, 44, 48, 52, 55, 58)] + [(0, 33), (33, 5), (20, 33)]
    return graph("contributions", line(60), cl, fixed=(0, 33), seed=7, env=dict(SGO_MFRONT_LEAF=8),
                 shape=lambda T: dict(off_diagonal_counts={1, 4, 5, 9} <= T.off_counts, all_parts=T.parts == {0, 1, 2, 3},
                                      hub_diagonal=max(T.diag_counts) >= 9),
                 why="targets with 1, 4, 5 and 9 contributions (four are prefetched), duplicates in both orientations, a hub's "
                     "diagonal block, fixed endpoints, an edge between two fixed poses")


def _solve(own3, leaf):
    fast = own3 <= 144
    return graph(f"solve_{'fast' if fast else 'generic'}_{own3}", line(own3 // 3 + 1), seed=own3, env=dict(SGO_MFRONT_LEAF=leaf),
                 shape=lambda T: dict(own3=int(T.own3.max()) == own3, branch=bool((T.fast if fast else T.generic).any()),
                                      only=not bool((T.generic if fast else T.fast).any())),
                 why=f"k_mf_solve's {'fast' if fast else 'generic'} branch at own3 = {own3}")


def _lattice(k, generic):
    return graph(f"lattice_{k}", lattice(k), lattice_rungs(k), seed=k, env=dict(SGO_MFRONT_CRIT_MFLOP=400),
                 shape=lambda T: dict(largest_own3=int(T.own3.max()) == (150 if generic else 144), generic=bool(T.generic.any()) == generic,
                                      fast=bool(T.fast.any()), height_4=T.levels >= 5),
                 why=f"a {k} x {k} grid with snake odometry: separators of about {k} poses; " +
                     ("its largest front takes k_mf_solve's generic branch" if generic else "its largest front is the last on the fast branch"))


def _weight_1e10():
    truth, cl = walk(130, 30, 11)
    scale = np.ones(129 + len(cl))
    scale[129 + 7] = 1e10
    c = graph("closure_weight_1e10", truth, cl, seed=11, env=dict(SGO_MFRONT_LEAF=16), info_scale=scale,
              shape=lambda T: dict(levels=T.levels >= 3), why="one closure of weight 10^10: blocks of wide scaling under the explicit inverses")
    c.phi[129 + 7] = -1.0
    return c


def _rows_scaled():
    truth, cl = walk(130, 30, 12)
    E = 129 + len(cl)
    scale = np.ones(E)
    scale[:129] = 10.0 ** (6.0 * ((np.arange(129) // 5) % 2))          # the chain: runs of five edges at 1 and at 10^6
    scale[129:] = 10.0 ** (6.0 * (2 * (np.arange(E - 129) % 2) - 1))    # the closures: 10^-6 and 10^6 in turn
    return graph("rows_scaled_1e6", truth, cl, seed=12, env=dict(SGO_MFRONT_LEAF=16), info_scale=scale, phi=-1.0,
                 shape=lambda T: dict(levels=T.levels >= 3),
                 why="information scaled by 10^+-6: odometry in runs of five edges at 1 and 10^6, closures at 10^-6 and 10^6 in turn "
                     "(a chain link at 10^-6 would leave kappa(H) above 1 / U: no factorisation is expected to survive that)")


def _dcs_off():
    truth, cl = walk(130, 30, 13)
    return graph("dcs_switches_closures_off", truth, cl, seed=13, env=dict(SGO_MFRONT_LEAF=16), phi=0.5, outliers=range(0, len(cl), 3),
                 shape=lambda T: dict(levels=T.levels >= 3), why="every third closure contradicts the chain: DCS weights near zero")


def _angles_pi():
    V = 40
    truth = line(V)
    truth[:, 2] = np.pi
    truth[:, 0] = -np.arange(V)
    truth[:, 1] = 0.0
    c = graph("angles_at_pi", truth, [(3, 20), (8, 31)], seed=14, env=dict(SGO_MFRONT_LEAF=8),
              shape=lambda T: dict(levels=T.levels >= 3), why="every angle within 1e-9 of +-pi before the update: k_mf_update's normalisation")
    rng = np.random.default_rng(14)
    th = np.where(rng.random(V) < 0.5, np.pi - 1e-9 * rng.random(V), -np.pi + 1e-9 * rng.random(V))
    c.poses[~c.fixed, 2] = th[~c.fixed]
    return c


def _long_chain():
    return graph("long_thin_chain", line(1500), seed=15, shape=lambda T: dict(height_4=T.levels >= 5),
                 why="1 499 free poses in a row: the pivots fall with the distance from the fixed pose")


BUILDERS = {}
for _k in (6, 15, 18, 48, 51):
    BUILDERS[f"root_own3_{_k}"] = (_root, (_k,))
for _k in _CHILD:
    BUILDERS[f"child_own3_{_k}"] = (_child, (_k,))
BUILDERS["rows_34"] = (_rows, (34, 10, 20))
BUILDERS["tree_shapes"] = (_tree_shapes, ())
BUILDERS["front_without_pivots"] = (_no_pivots, ())
BUILDERS["contributions"] = (_contributions, ())
BUILDERS["solve_fast_144"] = (_solve, (144, 48))
BUILDERS["solve_generic_147"] = (_solve, (147, 49))
BUILDERS["lattice_48"] = (_lattice, (48, False))
BUILDERS["lattice_50"] = (_lattice, (50, True))
BUILDERS["closure_weight_1e10"] = (_weight_1e10, ())
BUILDERS["rows_scaled_1e6"] = (_rows_scaled, ())
BUILDERS["dcs_switches_closures_off"] = (_dcs_off, ())
BUILDERS["angles_at_pi"] = (_angles_pi, ())
BUILDERS["long_thin_chain"] = (_long_chain, ())
NAMES = tuple(BUILDERS)
# m + 1 of some front of some case, asserted by the tests: row m last in a tile (16), with two others (19), clamped inside a
# tile (31, 34), alone in a tile (49)
ROWS_WANTED = {16: "child_own3_12", 19: "child_own3_15", 31: "child_own3_33", 34: "rows_34", 49: "child_own3_48"}


def make(name) -> Case:
    fn, args = BUILDERS[name]
    c = fn(*args)
    assert c.name == name, (c.name, name)
    return c


def check_shape(case, X):
    """The declared shape against the front table X (host plan or device export): {property: bool}, plus the wanted row count."""
    T = Table(X)
    got = dict(case.shape(T))
    for rows, name in ROWS_WANTED.items():
        if name == case.name:
            got[f"front_with_{rows}_rows"] = rows in T.rows
    return got
