"""The K-cycle of the resident multigrid hierarchy against tests/amg_reference.py: stage 9 (with the flexible-CG driver) end to
end, stage 10 step by step on the work vectors sgo_debug_amg_array exports after sgo_precondition.

Every case runs sgo_precondition (direct_rows=0) on two random vectors, one with rows scaled by 10^+-6
(test_gpu_kernel_reference._vectors), the zero vector (every exported vector and z exactly zero), a vector with a single
non-zero row, and the first vector again (bitwise equal: the coefficient reductions are fixed-order).  After each run the work
vectors of every level's last visit are exported and every step is checked against its own exported inputs (amg_reference's
stage 10: restrict, product, dots, bk2, p2, last, coarsest); z is compared with the long-double cycle in units of the case's fp64
rounding scale (K_KCYCLE).  The export is every level's LAST visit: the folded first cycle of a two-step level (k_up_fold with two
vectors and ratios among its launches) and every earlier visit of a level >= 2 are held by stage 9's end-to-end norm alone, not step
by step.  A case asserts the shape it exists for from the exported flags and grid counts, and prints its figures
-- the worst ratio per step with its level, and every level's shape with its largest aggregate -- before it asserts (run with -s).

The cases:
a  C2 with SGO_AMG_SMOOTH=0: tentative transfers everywhere, two flexible-CG steps on level 1.
b  GRAPH_B with SGO_AMG_SMOOTH=0, the smallest of {C2, 20k / 120k with 5 % random closures, 30k / 300k} that exports at least four
   levels: a level beyond fcg2_depth takes one step and, below the two-step level 1, is visited twice per cycle.
c  the same graph with SGO_AMG_FCG2_DEPTH = 0 (one step everywhere) and = 9 (two steps everywhere).
d  C2 with SGO_AMG_KDEPTH = 2 and = 1: smoothed, folded levels under the K-cycle -- the first cycle folded, the second unfolded.
   C2 exports three levels, so the shapes that need a sparse level 2 (the V-cycle below a K level; k_prolong_p / k_up_fold with two
   vectors and ratios) run on 30k / 300k, which exports four; what the export shows of them step by step is the second, unfolded
   cycle (k_prolong_p), see above.
e  the 20k graph with random closures at its defaults: tentative levels 0 and 1 over a smoothed level 2, a V level below a K level.
   NOT reached on the GPU: a SMOOTHED level 0 over tentative levels (k_prolong_p on level 0 taking fcg()'s ratios from a tentative
   child), the shape the issue calls production -- this graph and C4r (case g) both keep a tentative level 0 at their defaults.
   Only the "mixed" hierarchy of tests/test_amg_reference.py has it, on the CPU.
f  C4r with SGO_AMG_SMOOTH=0: the stalled level's aggregate of 627 members under k_restrict (no other case has more than 64
   members on a tentative level; every case reports max_aggregate per level).
g  C4r at its defaults: NOT reached -- its largest tentative level >= 1 has 271 096 slots, kUnfuseSlots is 400 000, and no graph of
   at most 30k poses comes near; the case asserts that figure and what is covered instead.
GRAPH_B is the 20k graph: C2 exports three levels under SGO_AMG_SMOOTH=0 (9999 -> 1406 -> 286 rows), the 20k graph four
(19999 -> 2753 -> 510 -> 113).  Measured on the MI355X: the file takes about 20 s of GPU-machine time, 5 s each for the two C4r
cases (100k poses: four exports and two long-double cycles per vector) and at most 1.7 s for every other.
"""
import json

import numpy as np
import pytest

import amg_reference as ar
from sparse_gslam_amd import capi, synth
from test_gpu_kernel_reference import _vectors

pytestmark = pytest.mark.gpu

GRAPHS = {"C2": lambda: synth.config("C2", info_mode="full"),
          "20k": lambda: synth.manhattan(20000, 120000, seed=21, p_random=0.05, info_mode="full"),
          "30k": lambda: synth.manhattan(30000, 300000, seed=12, info_mode="full"),
          "C4r": lambda: synth.config("C4r")}
GRAPH_B = "20k"
_cache = {}


def _graph(name):
    if name not in _cache:
        _cache[name] = GRAPHS[name]().arrays()
    return _cache[name]


def kcycle_vectors(o, lv, runs):
    """sgo_precondition on every (name, r) of runs against stage 9 (K_KCYCLE) and stage 10 on the exported work vectors.
    Returns (worst raw ratio per step, [(name, cycle error / eps_case, eps_case)], failures, grid counts per level)."""
    n = lv[0]["n"]
    order = lv[0]["row_order"].astype(np.int64)          # hessian row -> internal row
    worst, cyc, bad, grids = {}, [], {}, None
    for name, r in runs:
        z = o.precondition(r)
        W = ar.export_work(o, lv)
        ri, zi = np.empty((n, 3)), np.empty((n, 3))
        ri[order], zi[order] = r, z
        res = ar.check_kcycle(lv, W, ri, zi)
        for s, (raw, l, k) in ar.worst_by_step(res).items():
            if s not in worst or raw > worst[s][0]:
                worst[s] = (round(raw, 3), l, k, name)
        bad.update({(name,) + k: v for k, v in ar.failures(res).items()})
        zr, eps = ar.cycle_scale(lv, ri)
        cyc.append((name, round(ar.cycle_ratio(zi, zr, eps), 3), eps))
        grids = [[int(x) for x in w["grids"]] if "grids" in w else None for w in W]
    return worst, cyc, bad, grids


def kcycle_case(case, o, seed=0):
    """The case's vectors against stages 9 and 10; returns (levels, report).  Prints the figures, then asserts them."""
    o.linearize()
    lv = ar.export_hierarchy(o)
    desc = o.solver_description()
    assert len(lv) >= 2 and ar.has_kcycle(lv), desc
    n = lv[0]["n"]
    vec = _vectors(n, seed)
    one = np.zeros((n, 3))
    one[n // 3] = (1.0, -2.0, 0.5)
    runs = [("random", vec[0]), ("uniform", vec[1]), ("scaled", vec[2]), ("single_row", one)]
    worst, cyc, bad, grids = kcycle_vectors(o, lv, runs)
    z0 = o.precondition(vec[0])
    again = o.precondition(vec[0])
    zero = o.precondition(np.zeros((n, 3)))
    nonzero = ar.kcycle_all_zero(lv, ar.export_work(o, lv), zero)
    shape = [dict(l=l, n=L["n"], nslot=L["nslot"], smoothed=L["smoothed"], kind=L["kind"], nu=L["nu"],
                  solve=ar.solve_kind(lv, l) if l else "top", grids=grids[l],
                  max_aggregate=int(np.diff(L["mem_ptr"]).max()) if "mem_ptr" in L else 0) for l, L in enumerate(lv)]
    report = dict(case=case, desc=desc, kdepth=lv[0]["kdepth"], fcg2_depth=lv[0]["fcg2_depth"], worst=worst, cycle=cyc,
                  bitwise_repeat=bool(np.array_equal(z0, again)), zero_rule_violations=nonzero[:6], shape=shape)
    print("KCYCLE " + json.dumps(report, default=str))
    assert not bad, (case, bad)
    assert all(np.isfinite(c[1]) and c[1] <= ar.K_KCYCLE for c in cyc), (case, cyc)
    assert report["bitwise_repeat"], case
    assert not nonzero and np.isfinite(zero).all(), (case, nonzero)
    return lv, report


def _run(case, graph, monkeypatch, env=None, **kw):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*_graph(graph))
        return kcycle_case(case, o, **kw)


def _solves(lv):
    return [ar.solve_kind(lv, l) for l in range(1, len(lv))]


def _steps_ran(rep, l):
    """(first step ran, second step ran) on level l, from the exported grid counts."""
    gA, gB, gC = rep["shape"][l]["grids"]
    return gA > 0, gB > 0 and gC > 0


def test_a_tentative_everywhere_two_steps_on_level_1(monkeypatch):
    lv, rep = _run("a_C2_smooth0", "C2", monkeypatch, dict(SGO_AMG_SMOOTH="0"))
    assert len(lv) >= 3 and not any(L["smoothed"] for L in lv[:-1]), rep["desc"]
    assert _solves(lv)[0] == "fcg2" and _steps_ran(rep, 1) == (True, True), rep["shape"]


def test_b_a_level_beyond_fcg2_depth_takes_one_step_and_is_visited_twice(monkeypatch):
    lv, rep = _run("b_%s_smooth0" % GRAPH_B, GRAPH_B, monkeypatch, dict(SGO_AMG_SMOOTH="0"))
    assert len(lv) >= 4 and not any(L["smoothed"] for L in lv[:-1]), rep["desc"]
    s = _solves(lv)
    assert lv[0]["fcg2_depth"] == 1 and s[0] == "fcg2" and s[1] == "fcg1", s        # level 2: once per step of level 1
    assert _steps_ran(rep, 1) == (True, True) and _steps_ran(rep, 2) == (True, False), rep["shape"]


@pytest.mark.parametrize("depth,want", [("0", "fcg1"), ("9", "fcg2")])
def test_c_one_step_everywhere_and_two_steps_everywhere(depth, want, monkeypatch):
    lv, rep = _run("c_%s_smooth0_fcg2depth%s" % (GRAPH_B, depth), GRAPH_B, monkeypatch,
                   dict(SGO_AMG_SMOOTH="0", SGO_AMG_FCG2_DEPTH=depth))
    assert len(lv) >= 4 and lv[0]["fcg2_depth"] == int(depth), rep["desc"]
    assert all(k == want for k in _solves(lv)[:-1]), _solves(lv)
    assert all(_steps_ran(rep, l) == (True, want == "fcg2") for l in range(1, len(lv) - 1)), rep["shape"]


@pytest.mark.parametrize("graph,kdepth,fcg2", [("C2", "2", "1"), ("C2", "1", "1"), ("30k", "2", "1"), ("30k", "1", "1"), ("30k", "2", "2")])
def test_d_smoothed_folded_levels_under_the_k_cycle(graph, kdepth, fcg2, monkeypatch):
    """C2 has three levels (measured), so its level 2 is the dense one: k_prolong_fold takes level 1's two vectors and ratios, and
    level 1's second, unfolded cycle runs k_prolong_p.  30k / 300k has four (levels 1, 2 folded in two sweeps, nu = 2): kdepth = 1
    walks level 2 by the V-cycle below the K level 1; kdepth = 2 gives it one step, and with fcg2_depth = 2 two steps, whose two
    vectors and ratios level 1 prolongates with k_up_fold (its first cycle) and with k_prolong_p (its second).  Stage 10 sees each
    level's last visit, so of these only the second cycle's k_prolong_p is checked per step; the folded first cycle -- k_up_fold
    with two vectors and ratios -- reaches the test through z alone (stage 9's norm)."""
    lv, rep = _run("d_%s_kdepth%s_fcg2depth%s" % (graph, kdepth, fcg2), graph, monkeypatch,
                   dict(SGO_AMG_KDEPTH=kdepth, SGO_AMG_FCG2_DEPTH=fcg2))
    assert all(L["smoothed"] for L in lv[:-1]) and lv[0]["kdepth"] == int(kdepth) and lv[0]["fcg2_depth"] == int(fcg2), rep["desc"]
    s = _solves(lv)
    assert lv[0]["kind"] == ar.FOLDED and lv[1]["folded"] and lv[1]["kind"] in (ar.FOLDED, ar.FOLDED2), rep["shape"]
    assert s[0] == "fcg2" and _steps_ran(rep, 1) == (True, True), rep["shape"]
    if graph == "C2":
        assert s == ["fcg2", "dense"], s
    else:
        assert len(lv) == 4 and lv[2]["kind"] == ar.FOLDED2 and lv[2]["nu"] == 2, rep["shape"]
        assert s[1] == ("V" if kdepth == "1" else ("fcg2" if fcg2 == "2" else "fcg1")), s
        assert _steps_ran(rep, 2) == (kdepth == "2", kdepth == "2" and fcg2 == "2"), rep["shape"]


def test_e_default_mix_of_tentative_and_smoothed_levels(monkeypatch):
    """The 20k graph with 5 % random closures at its defaults.  Measured: levels 0 and 1 keep the tentative transfer, level 2 is
    smoothed (kdepth = 0: the V-cycle walks it, below the K level 1: coarse_solve's `l + 1 > kdepth && C.smoothed` branch).  The mix
    is asserted from the flags: at least one tentative and one smoothed level, a K level above a V level.  Level 0 is tentative
    here, so this is not the shape of a smoothed level 0 over tentative levels: no graph of this suite gives that on the GPU."""
    lv, rep = _run("e_20k_defaults", "20k", monkeypatch)
    sm = [bool(L["smoothed"]) for L in lv[:-1]]
    assert any(sm) and not all(sm) and lv[0]["kdepth"] == 0, rep["desc"]
    s = _solves(lv)
    assert "V" in s and any(k.startswith("fcg") for k in s[:s.index("V")]), s


def test_f_c4r_long_aggregate_under_k_restrict(monkeypatch):
    """No case above has an aggregate of more than 64 members on a tentative level (their largest: 50, on the 20k graph's level 0),
    and C4r at its defaults smooths its stalled level, whose 627 members then go through P.  With SGO_AMG_SMOOTH=0 that level keeps
    the tentative transfer: k_restrict sums a 627-member aggregate, and the level takes one flexible-CG step."""
    lv, rep = _run("f_C4r_smooth0", "C4r", monkeypatch, dict(SGO_AMG_SMOOTH="0"))
    big = [s for s in rep["shape"][:-1] if not s["smoothed"] and s["max_aggregate"] > 64]
    assert big and big[0]["max_aggregate"] == 627 and big[0]["solve"] == "fcg1", rep["shape"]
    assert _steps_ran(rep, big[0]["l"]) == (True, False), rep["shape"]


def test_g_c4r_largest_tentative_level_stays_below_the_unfused_path(monkeypatch):
    """C4r at its defaults, the production shape of the benchmark's C5.  Its largest tentative level >= 1 has 271 096 slots
    (measured), below kUnfuseSlots = 400 000, and no graph of at most 30k poses comes near: the unfused pre_resid / k_prolong_add
    pair of a LARGE level >= 1 is not reached by this suite.  Level 0 (2.1 M slots) runs k_prolong_add in place in every case
    with a tentative level 0, which stage 10 checks as last.prolong.  Asserted, so that a change of either figure is seen."""
    lv, rep = _run("g_C4r", "C4r", monkeypatch)
    tent = [s for s in rep["shape"][1:-1] if not s["smoothed"]]
    assert tent and max(s["nslot"] for s in tent) < ar.UNFUSE_SLOTS, rep["shape"]
    assert not rep["shape"][0]["smoothed"] and rep["shape"][0]["nslot"] >= ar.UNFUSE_SLOTS, rep["shape"]
    assert any(s["smoothed"] and s["max_aggregate"] == 627 for s in rep["shape"][:-1]), rep["shape"]
