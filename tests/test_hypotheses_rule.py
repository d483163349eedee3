"""sgo_hypothesis_isolated_vertex (include/sgo.h): the mask rule of sgo_optimize_gn_hypotheses as a pure function -- no context, no
GPU -- against a numpy restatement, and the size of the result record."""
import ctypes

import numpy as np
import pytest

from sparse_gslam_amd import capi


def rule(fixed, ei, ej, info, off):
    """the lowest free vertex that an edge the mask switches off leaves without an incident edge of non-zero information, or -1"""
    fixed, ei, ej, off = np.asarray(fixed, bool), np.asarray(ei), np.asarray(ej), np.asarray(off) != 0
    live = np.any(np.asarray(info, float).reshape(-1, 6) != 0.0, axis=1)
    killed, kept = live & off, live & ~off
    deg = np.bincount(ei[kept], minlength=fixed.size) + np.bincount(ej[kept], minlength=fixed.size)
    touched = np.unique(np.concatenate([ei[killed], ej[killed]]))
    bad = [int(v) for v in touched if not fixed[v] and deg[v] == 0]
    return min(bad) if bad else -1


V = 6
CHAIN = [(k, k + 1) for k in range(V - 1)]               # edges 0 .. 4
EDGES = CHAIN + [(0, 3), (1, 5)]                         # closures 5 and 6: pose 2 and pose 4 have their chain edges only
ROW = [2.0, 0.1, 0.0, 3.0, 0.2, 5.0]


def graph(edges=EDGES, fixed=(0,), zero=()):
    ei = np.array([e[0] for e in edges], dtype=np.int32)
    ej = np.array([e[1] for e in edges], dtype=np.int32)
    info = np.tile(ROW, (len(edges), 1))
    info[list(zero)] = 0.0
    f = np.zeros(V, dtype=np.uint8)
    f[list(fixed)] = 1
    return f, ei, ej, info


def mask(n, on):
    m = np.zeros(n, dtype=np.uint8)
    m[list(on)] = 1
    return m


CASES = {
    "no edge off": (graph(), (), -1),
    "a closure off": (graph(), (6,), -1),
    "both chain edges of an interior pose off": (graph(), (1, 2), 2),
    "the same pose when it is fixed": (graph(fixed=(0, 2)), (1, 2), -1),
    "an edge whose resident information is already zero, listed": (graph(zero=(6,)), (6,), -1),
    "... and a pose that zero row no longer holds": (graph(zero=(6,)), (4,), 5),
    "... which the live closure does hold": (graph(), (4,), -1),
    "a duplicated pair with one copy off": (graph(edges=CHAIN + [(4, 5)], zero=()), (4,), -1),
    "a duplicated pair with both copies off": (graph(edges=CHAIN + [(4, 5)]), (4, 5), 5),
    "the last pose's only edge off": (graph(edges=CHAIN), (4,), 5),
    "two poses isolated: the lowest is named": (graph(edges=CHAIN), (1, 2, 4), 2),
    "a mask of non-zero bytes other than 1": (graph(edges=CHAIN), None, 1),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_rule_matches_the_numpy_restatement(name):
    (fixed, ei, ej, info), on, want = CASES[name]
    off = np.full(ei.size, 200, dtype=np.uint8) if on is None else mask(ei.size, on)
    assert rule(fixed, ei, ej, info, off) == want
    assert capi.hypothesis_isolated_vertex(fixed, ei, ej, info, off) == want


def test_rule_on_random_masks_of_a_generated_graph():
    from sparse_gslam_amd import synth
    g = synth.manhattan(80, 95, seed=4, info_mode="full", phi=10.0)
    rng = np.random.default_rng(0)
    info = g.info.copy()
    info[[83, 90]] = 0.0
    hits = 0
    for p in (0.05, 0.3, 0.6):
        for _ in range(40):
            off = (rng.random(g.E) < p).astype(np.uint8)
            want = rule(g.fixed, g.ei, g.ej, info, off)
            hits += want >= 0
            assert capi.hypothesis_isolated_vertex(g.fixed, g.ei, g.ej, info, off) == want
    assert 10 < hits < 110          # both answers occur


def test_rule_refuses_bad_arguments():
    fixed, ei, ej, info = graph()
    bad = ei.copy()
    bad[3] = V
    with pytest.raises(capi.SgoError, match="rc=-2"):
        capi.hypothesis_isolated_vertex(fixed, bad, ej, info, mask(ei.size, ()))


def test_result_record_is_24_bytes():
    assert ctypes.sizeof(capi.HypothesisResult) == 24
    assert (capi.HYP_BATCHED, capi.HYP_SEQUENTIAL) == (1, 2)
