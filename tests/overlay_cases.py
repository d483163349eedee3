"""The case list of the overlay reference (tests/overlay_reference.py): resident graphs with hand-built appended parts, shared
by the CPU tests (forward model, mutations) and the GPU tests.  A plan is a resident graph, the world it was cut from and a
list of updates; an update is the poses appended ([first, V)), their odometry edges and whatever closures the case is about.
The appended poses start dead-reckoned (synth.chain_init) from the estimates current at the update, as the reference's do."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import np_oracle as npo
from sparse_gslam_amd import synth

BASE_V, BASE_E = 600, 2400


@dataclass
class Plan:
    name: str
    base: synth.Graph
    g: synth.Graph
    updates: list = field(default_factory=list)
    expect: dict = field(default_factory=dict)      # header fields the case exists for: k, nt, nx, ncol
    late: object = None                             # late(P0, edges of the last update): measurements that depend on P0
    composed: bool = True


def _world(chain, seed=7, **kw):
    base, steps, g = synth.append_session(BASE_V, BASE_E, 1, max(chain, 1), seed, closures_per_step=0, **kw)
    return base, g


class _Edges:
    def __init__(self, g, seed):
        self.g, self.rng, self.rows = g, np.random.default_rng(seed), []
        self.closure_info = g.info[g.E - 1]

    def odom(self, a, b, anchor=None):
        """odometry edges of the appended poses [a, b): (a-1, a) ... (b-2, b-1); anchor: the first one's other endpoint instead"""
        g = self.g
        for e in range(a - 1, b - 1):
            if e == a - 1 and anchor is not None:
                self.add(anchor, a, phi=-1.0, info=g.info[e])
            else:
                self.rows.append((int(g.ei[e]), int(g.ej[e]), g.meas[e], g.info[e], float(g.phi[e])))
        return self

    def add(self, i, j, phi=1.0, info=None, weight=None):
        g = self.g
        sig = np.array([synth.SIGMA_XY, synth.SIGMA_XY, synth.SIGMA_TH])
        z = synth._rel(g.truth[[i]], g.truth[[j]])[0] + self.rng.standard_normal(3) * sig
        z[2] = synth._wrap(z[2])
        inf = self.closure_info if info is None else info
        if weight is not None:
            inf = np.array([weight, 0.0, 0.0, weight, 0.0, weight])
        self.rows.append((int(i), int(j), z, np.asarray(inf, dtype=np.float64), float(phi)))
        return self

    def update(self, V, fixed_new=()):
        r = self.rows
        self.rows = []
        return dict(V=V, fixed_new=list(fixed_new), ei=np.array([t[0] for t in r], np.int32), ej=np.array([t[1] for t in r], np.int32),
                    meas=np.array([t[2] for t in r]).reshape(-1, 3), info=np.array([t[3] for t in r]).reshape(-1, 6),
                    phi=np.array([t[4] for t in r]))


def _targets(n, lo=40, hi=BASE_V - 20):
    """n distinct resident poses spread over the base"""
    return [int(v) for v in np.linspace(lo, hi, n).astype(int)]


# ------------------------------------------------------------------ the cases
def tile(k):
    base, g = _world(k)
    V0 = base.V
    E = _Edges(g, k).odom(V0, V0 + k).add(V0 + k // 2, 123)
    return Plan(f"tile_k{k}", base, g, [E.update(V0 + k)], dict(k=k, nt=2, nx=0))


def no_chain():
    base, g = _world(1)
    E = _Edges(g, 1).add(100, 480).add(42, 577).add(100, 480).add(333, 42)
    return Plan("k0_resident_closures", base, g, [E.update(base.V)], dict(k=0, nt=5, nx=0))


def fixed_anchor():
    base, g = _world(9)
    V0 = base.V
    E = _Edges(g, 2).odom(V0, V0 + 9, anchor=0)
    return Plan("nt0_chain_on_fixed_vertex", base, g, [E.update(V0 + 9)], dict(k=9, nt=0, nx=0, ncol=1))


def _hub_pairs(V0, nx):
    """nx disjoint closures (V0 + 3 q, V0 + 3 q + 2): pose 3 q + 2 becomes a hub, the chain falls into segments of two"""
    return [(V0 + 3 * q, V0 + 3 * q + 2) for q in range(nx)]


def wave(nk, nx, chain=26):
    base, g = _world(chain)
    V0 = base.V
    E = _Edges(g, 10 * nk + nx).odom(V0, V0 + chain)
    tg = _targets(nk - nx - 1)                                     # + the chain's anchor V0 - 1
    for q, v in enumerate(tg):
        if q % 2:
            E.add(v, V0 + (5 * q) % chain)
        else:
            E.add(V0 + (5 * q) % chain, v)
    for a, b in _hub_pairs(V0, nx):
        E.add(a, b)
    return Plan(f"wave_nk{nk}_nx{nx}", base, g, [E.update(V0 + chain)], dict(k=chain - nx, nt=nk - nx, nx=nx, ncol=3 * nk + 1))


def hubs_one():
    base, g = _world(12)
    V0 = base.V
    h = V0 + 7
    E = _Edges(g, 3).odom(V0, V0 + 12).add(V0 + 3, h)
    E.add(0, h).add(h, 0).add(321, h).add(h, 400).add(h, V0 + 2).add(V0 + 1, h).add(V0 + 5, 123)
    return Plan("hubs_1", base, g, [E.update(V0 + 12)], dict(k=11, nt=4, nx=1))


def hubs_eight():
    """Hubs at the earliest possible position (the third appended pose: a hub is the LATER endpoint of a non-neighbour edge) and
    at the last one, hubs that cut the chain into nine segments, hub-hub / hub-fixed / hub-resident / hub-chain edges in both
    orientations."""
    base, g = _world(24)
    V0 = base.V
    E = _Edges(g, 4).odom(V0, V0 + 24)
    for a, b in ((0, 2), (5, 23), (4, 9), (6, 14), (11, 17), (12, 19), (15, 21), (3, 7)):
        E.add(V0 + a, V0 + b)
    E.add(V0 + 9, V0 + 14).add(V0 + 23, V0 + 2).add(0, V0 + 9).add(V0 + 14, 0).add(321, V0 + 9).add(V0 + 14, 400)
    E.add(V0 + 14, V0 + 4).add(V0 + 5, V0 + 9).add(V0 + 12, 77)
    return Plan("hubs_8", base, g, [E.update(V0 + 24)], dict(k=16, nt=4, nx=8))


def multiblock(k, nk):
    base, g = _world(k)
    V0 = base.V
    E = _Edges(g, k).odom(V0, V0 + k)
    for q, v in enumerate(_targets(nk - 1)):
        E.add(V0 + (q * k) // max(nk - 1, 1), v)
    return Plan(f"multiblock_k{k}_nk{nk}", base, g, [E.update(V0 + k)], dict(k=k, nt=nk, nx=0), composed=k <= 300)


def accumulation():
    """three updates of six poses; the third closes into a pose of the first (a hub) and ends in a fixed appended pose"""
    base, g = _world(18)
    V0 = base.V
    E = _Edges(g, 5)
    u1 = E.odom(V0, V0 + 6).add(V0 + 3, 200).update(V0 + 6)
    u2 = E.odom(V0 + 6, V0 + 12).add(450, V0 + 9).update(V0 + 12)
    u3 = E.odom(V0 + 12, V0 + 18).add(V0 + 2, V0 + 15).add(V0 + 14, 200).update(V0 + 18, fixed_new=[V0 + 17])
    return Plan("accumulation", base, g, [u1, u2, u3], dict(k=16, nt=3, nx=1))


def full_information():
    base, g = _world(10, info_mode="full", phi=10.0)
    V0 = base.V
    E = _Edges(g, 6).odom(V0, V0 + 10).add(V0 + 5, 250, phi=10.0).add(90, V0 + 8, phi=10.0)
    return Plan("full_information_phi10", base, g, [E.update(V0 + 10)], dict(k=10, nt=3, nx=0))


def dcs_kink():
    """one closure whose e2 equals its phi up to rounding at the poses of the update: Z = (Xi^-1 Xj) d^-1 with d^T Omega d = phi"""
    base, g = _world(10)
    V0 = base.V
    E = _Edges(g, 7).odom(V0, V0 + 10).add(V0 + 4, 310, phi=1.0)
    up = E.update(V0 + 10)

    def late(P0, u):
        q = u["ei"].size - 1
        d = np.array([np.sqrt(u["phi"][q] / u["info"][q, 0]), 0.0, 0.0])
        rel = npo.se2_mul(npo.se2_inv(P0[u["ei"][q]]), P0[u["ej"][q]])
        u["meas"][q] = npo.se2_mul(rel, npo.se2_inv(d))
    return Plan("dcs_kink", base, g, [up], dict(k=10, nt=2, nx=0), late=late)


def heavy_closure():
    base, g = _world(10)
    V0 = base.V
    E = _Edges(g, 8).odom(V0, V0 + 10).add(V0 + 6, 150, phi=-1.0, weight=1e10).add(V0 + 2, 410)
    return Plan("closure_weight_1e10", base, g, [E.update(V0 + 10)], dict(k=10, nt=3, nx=0))


def dead_reckoned():
    """the appended chain at its chain_init start (every case's start; here with nothing else going on): odometry errors are rounding"""
    base, g = _world(12)
    V0 = base.V
    E = _Edges(g, 9).odom(V0, V0 + 12).add(V0 + 11, 20)
    return Plan("dead_reckoned_chain", base, g, [E.update(V0 + 12)], dict(k=12, nt=2, nx=0))


CASES = {}
for _k in (1, 7, 8, 9, 17):
    CASES[f"tile_k{_k}"] = (tile, (_k,))
CASES["k0_resident_closures"] = (no_chain, ())
CASES["nt0_chain_on_fixed_vertex"] = (fixed_anchor, ())
for _nk, _nx in ((21, 0), (22, 8), (42, 0), (43, 8), (64, 0), (64, 8)):
    CASES[f"wave_nk{_nk}_nx{_nx}"] = (wave, (_nk, _nx))
CASES["hubs_1"] = (hubs_one, ())
CASES["hubs_8"] = (hubs_eight, ())
CASES["multiblock_k257_nk2"] = (multiblock, (257, 2))
CASES["multiblock_k512_nk64"] = (multiblock, (512, 64))
CASES["accumulation"] = (accumulation, ())
CASES["full_information_phi10"] = (full_information, ())
CASES["dcs_kink"] = (dcs_kink, ())
CASES["closure_weight_1e10"] = (heavy_closure, ())
CASES["dead_reckoned_chain"] = (dead_reckoned, ())


def plan(name) -> Plan:
    f, a = CASES[name]
    return f(*a)


def arrays_upto(p: Plan, upto: int):
    """(V, fixed, ei, ej, meas, info, phi) of the base + the first `upto` updates"""
    parts = p.updates[:upto]
    V = parts[-1]["V"] if parts else p.base.V
    fixed = np.zeros(V, dtype=bool)
    fixed[:p.base.V] = p.base.fixed
    for u in parts:
        fixed[u["fixed_new"]] = True
    cat = lambda k: np.concatenate([getattr(p.base, k)] + [u[k] for u in parts])      # noqa: E731
    return V, fixed, cat("ei"), cat("ej"), cat("meas"), cat("info"), cat("phi")


def start_poses(p: Plan, P, V):
    """P extended to V poses: the new ones dead-reckoned from the last estimate through the odometry measurements"""
    P0 = np.empty((V, 3))
    P0[:P.shape[0]] = P
    if V > P.shape[0]:
        synth.chain_init(P0, p.g.meas[:p.g.V - 1], P.shape[0], V - 1)
    return P0


def make_case(p: Plan, P0, hpos):
    """The reference's case dict for the state after the plan's last update, given the poses handed to it."""
    V, fixed, *_ = arrays_upto(p, len(p.updates))
    app = tuple(np.concatenate([u[k] for u in p.updates]) for k in ("ei", "ej", "meas", "info", "phi"))
    b = p.base
    return dict(V0=b.V, fixed=fixed, P0=np.asarray(P0, dtype=np.float64), res=(b.ei, b.ej, b.meas, b.info, b.phi), app=app,
                hpos=np.asarray(hpos, dtype=np.int64))


def cpu_case(p: Plan, seed=0):
    """The case without a device: every update's start chained from the previous start, a random internal row order."""
    P = p.base.poses
    for q, u in enumerate(p.updates):
        P = start_poses(p, P, u["V"])
    if p.late is not None:
        p.late(P, p.updates[-1])
    hidx, free = npo.hessian_index(p.base.fixed)
    hpos = np.full(p.base.V, -1, dtype=np.int64)
    hpos[free] = np.random.default_rng(seed).permutation(free.size)
    return make_case(p, P, hpos)
