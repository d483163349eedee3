"""The cases of the direct path's stage tests: the smallest graphs that reach every branch of k_direct and of its host analysis
(CPU only: tests/test_direct_reference.py runs the fp64 model on them, tests/test_gpu_direct_reference.py the device).

A case = a graph (mfront_cases.graph's: a trajectory, the odometry chain and the listed closures, P0 = truth + noise), for the
`kinds_*` cases the robust kernels of its edges, and the SHAPE it is there for: a predicate on the plan tables (INFO and the
lists) that both tests assert, so that a change of the generators or of the elimination analysis cannot silently turn a case
into another one.  The separators are a greedy vertex cover of the non-chain pairs (highest closure degree first, ties to the
lower pose): a closure between two poses nothing else touches makes its lower endpoint a separator.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import mfront_cases as mc
import robust_reference as rr
from sparse_gslam_amd import capi

LDS_BUDGET = 150 * 1024          # sgo_direct.hip's kLdsBudget
MAX_SEP = 60                     # ... kMaxSep


@dataclass
class DCase(mc.Case):
    kind: np.ndarray = None      # per edge, robust_reference's numbering (None: DCS with phi, as the graph says)
    delta: np.ndarray = None
    refused: str = ""            # the reason the analysis must give (a plan-only case)

    def as_dict(self):
        d = super().as_dict()
        d.update(kind=self.kind, delta=self.delta)
        return d


class Table:
    """The plan tables in the terms the shapes are declared in."""

    def __init__(self, X):
        for k, v in zip(capi.DIRECT_INFO, X["INFO"]):
            setattr(self, k, int(v))
        rc = np.asarray(X["SLOT_RC"], dtype=np.int64).reshape(-1, 2)
        self.row, self.col = rc[:, 0], rc[:, 1]
        lm = np.asarray(X["LMETA"], dtype=np.int64)
        self.lslot, self.ltask = lm[:self.NL + 1], lm[self.NL + 1:]
        self.level_slots = np.diff(self.lslot)
        self.level_tasks = np.diff(self.ltask)
        self.dummy_slots = int(((self.row < 0) & (self.col >= 0)).sum())
        real = (self.row >= 0) & (self.col >= 0)
        self.column_blocks = np.bincount(self.col[real], minlength=max(self.nI, 1))
        # padding BEFORE a column inside a level (the column would straddle a multiple of 64), not only at the level's end
        self.inner_padding = bool(np.any((self.col[:-1] < 0) & (self.col[1:] >= 0))) if self.NB > 1 else False
        vr = np.asarray(X["VREC"], dtype=np.int64).reshape(-1, 4)
        vo = np.asarray(X["VOVER"], dtype=np.int64)
        self.incident = np.array([(r[:3] >= 0).sum() + (1 if r[3] >= 0 else (int(vo[-2 - r[3]]) if r[3] <= -2 else 0)) for r in vr])
        et = np.asarray(X["EDGE_TGT"], dtype=np.int64)[:self.E]
        self.e_kind, self.e_tr = et >> 30, (et >> 29) & 1
        m = np.asarray(X["MULTI"], dtype=np.int64).reshape(-1, 2)
        en = np.asarray(X["ENEXT"], dtype=np.int64)
        self.multi = []                # per pair: (target kind: 1 a slot, 2 a separator block; the transposed flags of its edges)
        for tgt, first in m:
            fl, t = [], int(first)
            while t >= 0:
                fl.append(t & 1)
                t = int(en[t >> 1])
            self.multi.append(((int(tgt) & 0xffffffff) >> 30, fl))
        tk = np.asarray(X["TK"], dtype=np.int64).reshape(-1, 4)
        self.task_contribs = tk[:, 2] - tk[:, 1]


def _case(name, truth, closures=(), shape=None, why="", kinds=None, refused="", **kw):
    g = mc.graph(name, truth, closures, shape=shape, why=why, **kw)
    c = DCase(g.name, g.poses, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi, {}, shape, why, refused=refused)
    if kinds is not None:
        c.kind, c.delta = kinds(c)
    return c


def _two_poses():
    return _case("two_poses", mc.line(2), seed=2,
                 shape=lambda T: dict(one_free_pose=T.n == 1, no_separator=T.ns == 0, one_dummy_slot=T.dummy_slots == 1 and T.column_blocks.sum() == 0,
                                      nothing_to_update=T.tasks == 0),
                 why="n = 1: the only edge has a fixed endpoint, the one column is empty (a dummy slot)")


def _chain(V):
    return _case(f"chain_{V}", mc.line(V), seed=V,
                 shape=lambda T: dict(no_separator=T.ns == 0 and T.tri == 0, root_column_empty=T.dummy_slots == 1, levels=T.NL >= 2,
                                      padded_inside_a_level=T.inner_padding or V < 65),
                 why="no closure: ns = 0, the dense phase is skipped; the root column is empty; from 65 poses on a column is padded "
                     "across a 64-slot boundary")


def _one_closure():
    return _case("one_closure", mc.line(24), [(4, 17)], seed=3, shape=lambda T: dict(one_separator=T.ns == 1, dense_target=T.tri == 6),
                 why="ns = 1: a pivot and no dense step")


def _two_seps():
    cl = [(5, 14), (5, 20), (30, 11), (30, 24), (5, 30), (30, 5)]
    return _case("two_seps", mc.line(36), cl, seed=4,
                 shape=lambda T: dict(two_separators=T.ns == 2, separator_pair_both_orientations=any(k == 2 and set(f) == {0, 1} for k, f in T.multi)),
                 why="ns = 2: one dense step; the separator pair carries closures in both orientations")


def _three_seps():
    cl = [(5, 14), (5, 20), (30, 11), (30, 24), (40, 8), (40, 22), (30, 5), (5, 40), (40, 30)]
    return _case("three_seps", mc.line(46), cl, seed=5,
                 shape=lambda T: dict(three_separators=T.ns == 3,
                                      single_separator_edges_both_orientations={0, 1} <= set(int(v) for v in T.e_tr[T.e_kind == 2])),
                 why="ns = 3: single edges between separators stored as they are and transposed")


def _multi_pairs():
    cl = [(7, 8), (8, 7),                       # three edges on a chain pair (with the odometry edge), mixed
          (12, 13),                             # two on a chain pair
          (3, 20), (20, 3), (3, 20),            # three on a sparse-separator pair
          (26, 20),                             # (keeps 20 the separator: closure degree 2)
          (20, 33), (33, 20), (33, 40), (33, 28)]   # two on a separator pair (33: closure degree 3)
    return _case("multi_pairs", mc.line(44), cl, seed=6,
                 shape=lambda T: dict(chain_pairs={2, 3} <= set(len(f) for k, f in T.multi if k == 1),
                                      mixed_orientations=all(set(f) == {0, 1} for k, f in T.multi if len(f) == 3),
                                      separator_pair=any(k == 2 for k, f in T.multi), pairs=T.nmulti >= 4),
                 why="two and three edges on a chain pair, on a sparse-separator pair and on a separator pair, in mixed orientations")


def _hub():
    V = 60
    fixed = (0, 25, 26, 41)
    cl = [(10, 30), (10, 35),                                   # pose 10: exactly 4 incident edges
          (16, 45), (16, 50), (16, 55)]                         # pose 16: exactly 5
    cl += [(20, j) for j in (2, 6, 33, 37, 44, 48, 52, 54, 57, 59)]   # pose 20: 12
    cl += [(25, 26), (0, 41), (26, 12), (38, 25), (41, 3)]       # between fixed poses (one doubles the chain edge), to fixed poses
    return _case("hub", mc.line(V), cl, fixed=fixed, seed=7,
                 shape=lambda T: dict(incident_4=4 in T.incident, incident_5=5 in T.incident, incident_12=12 in T.incident,
                                      edges_without_target=int((T.e_kind == 0).sum()) >= 8),
                 why="poses with exactly 4 (all inline), 5 (three inline, two in the overflow list) and 12 incident edges; fixed poses "
                     "mid-chain, edges to and between fixed poses")


def _disjoint(N):
    return [(4 * i + 1, 4 * i + 3) for i in range(N)]


def _seps(N):
    return _case(f"seps_{N}", mc.line(4 * N + 2), _disjoint(N), seed=N,
                 shape=lambda T: dict(separators=T.ns == N, dense_items_from_the_table=(T.ns * (T.ns - 1) // 2 > 3 * 384) == (N >= 49)),
                 why=f"{N} disjoint closures = {N} separators: the first dense step has {N * (N - 1) // 2} work items for 384 threads with "
                     "three each in registers (a fourth comes from dpl[] from 49 separators on)")


def _seps_61():
    return _case("seps_61", mc.line(4 * 61 + 2), _disjoint(61), seed=61, refused="more separators than the dense block holds",
                 why="61 separators: refused, the graph takes another path")


def _wide_column():
    N = 49
    seps = [210 + 3 * i for i in range(N)]
    cl = []
    for i, s in enumerate(seps):
        cl += [(s, 4 * i + 2), (s, 4 * i + 4)]
    return _case("wide_column", mc.line(seps[-1] + 3), cl, seed=8,
                 shape=lambda T: dict(separators=T.ns == N, column_of_49_blocks=int(T.column_blocks.max()) >= 49),
                 why="one chain segment whose poses are partners of 49 separators: its last column holds >= 49 blocks (a wave's segment)")


def _tasks_over_512():
    return _case("tasks_over_512", mc.line(1100), [(100, 700), (300, 900), (450, 1000), (205, 640)], seed=9,
                 shape=lambda T: dict(edges=T.E > 512, level_tasks=int(T.level_tasks.max()) > 512, level_slots=int(T.level_slots.max()) > 512),
                 why="E > 512, a level with more than 512 tasks and one with more than 512 slots: the loops run past the prefetched item")


def _xg_poses(above):
    """The pose count at which the vector stops fitting the LDS next to 60 separators' triangle, from the plan's own lds_bytes."""
    def info(V):
        c = mc.graph("probe", mc.line(V), _disjoint(MAX_SEP), seed=10)
        return dict(zip(capi.DIRECT_INFO, (int(v) for v in capi.direct_plan_arrays(c.fixed, c.ei, c.ej, names=("INFO",))["INFO"])))
    V = 560
    i0 = info(V)
    assert not i0["xb_global"]
    V += (LDS_BUDGET - i0["lds_bytes"]) // 24 - 4            # 24 bytes of LDS per further pose; the levels' table grows a little
    while not info(V + 1)["xb_global"]:
        V += 1
    return V + 1 if above else V


def _xg(above, kinds=None, name=None):
    V = _xg_poses(above)
    return _case(name or ("xg_above" if above else "xg_below"), mc.line(V), _disjoint(MAX_SEP), seed=10, kinds=kinds,
                 shape=lambda T: dict(separators=T.ns == MAX_SEP, vector_in_global_memory=bool(T.xb_global) == above,
                                      at_the_threshold=(T.lds_bytes + 24 > LDS_BUDGET) if not above else (T.lds_bytes + 24 * T.n > LDS_BUDGET >= T.lds_bytes + 24 * (T.n - 1))),
                 why=f"60 separators and {V - 1} free poses: the {'first' if above else 'last'} pose count whose vector "
                     f"{'lives in global memory (XG)' if above else 'still fits the LDS'}")


def _mixed_kinds(c):
    E = c.ei.size
    kinds = np.array([rr.CAUCHY, rr.HUBER, rr.GEMAN_MCCLURE, rr.WELSCH, rr.PSEUDO_HUBER, rr.DCS, rr.NONE])
    kind = kinds[np.arange(E) % kinds.size]
    delta = np.where(kind == rr.DCS, 10.0, 1.5 + 0.5 * (np.arange(E) % 3))
    return kind, delta


def _kinds_mixed():
    truth, cl = mc.walk(90, 14, 21)
    return _case("kinds_mixed", truth, cl, seed=21, kinds=_mixed_kinds,
                 shape=lambda T: dict(separators=T.ns >= 3, in_lds=not T.xb_global), why="per-edge robust kernels other than DCS (KINDS)")


def _kinds_xg():
    return _xg(True, kinds=_mixed_kinds, name="kinds_xg")


def _long_chain():
    return _case("long_chain_2048", mc.line(2049), seed=12, shape=lambda T: dict(n=T.n == 2048, no_separator=T.ns == 0, levels=T.NL == 12),
                 why="2048 free poses, no closure: the top pivots are Schur complements of 1024-pose segments")


def _from_mfront(name, builder):
    def make():
        g = builder()
        return DCase(name, g.poses, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi, {}, lambda T: dict(separators=T.ns >= 2, levels=T.NL >= 3), g.why)
    return make


BUILDERS = {"two_poses": (_two_poses, ()), "chain_3": (_chain, (3,)), "chain_65": (_chain, (65,)), "chain_130": (_chain, (130,)),
            "one_closure": (_one_closure, ()), "two_seps": (_two_seps, ()), "three_seps": (_three_seps, ()),
            "multi_pairs": (_multi_pairs, ()), "hub": (_hub, ()), "seps_48": (_seps, (48,)), "seps_49": (_seps, (49,)),
            "seps_60": (_seps, (60,)), "wide_column": (_wide_column, ()), "tasks_over_512": (_tasks_over_512, ()),
            "xg_below": (_xg, (False,)), "xg_above": (_xg, (True,)), "kinds_mixed": (_kinds_mixed, ()), "kinds_xg": (_kinds_xg, ()),
            "long_chain_2048": (_long_chain, ()),
            "weight_1e10": (_from_mfront("weight_1e10", mc._weight_1e10), ()),
            "rows_scaled_1e6": (_from_mfront("rows_scaled_1e6", mc._rows_scaled), ()),
            "angles_pi": (_from_mfront("angles_pi", mc._angles_pi), ()),
            "dcs_switches_closures_off": (_from_mfront("dcs_switches_closures_off", mc._dcs_off), ())}
NAMES = tuple(BUILDERS)
REFUSED = {"seps_61": (_seps_61, ())}
SECOND_ITERATION = ("two_seps", "multi_pairs", "seps_49")          # the GPU test also runs optimize(2) on these
_MADE = {}


def make(name) -> DCase:
    """The case (built once, shared, never modified)."""
    if name not in _MADE:
        fn, args = (BUILDERS.get(name) or REFUSED[name])
        c = fn(*args)
        assert c.name == name, (c.name, name)
        _MADE[name] = c
    return _MADE[name]


def check_shape(case, X):
    """The declared shape against the plan tables X (host plan or device export): {property: bool}."""
    return dict(case.shape(Table(X)))
