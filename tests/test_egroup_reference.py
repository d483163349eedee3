"""The leave-group-out statistic on the CPU (tests/egroup_reference.py; no GPU): sgo_edge_group_rule -- the text k_edge_groups
compiles -- and the closed form in numpy against the explicit removal of the group in long double.

Cases: tree_shapes, contributions (fixed endpoints, duplicate pairs, an edge between two fixed poses), dcs_switches_closures_off
(weights near 0, fractional and 1 in one group: the Nt D (I - D) Nt term), angles_at_pi, long_thin_chain (bridges alone) of
tests/mfront_cases.py, and egroup_reference.cluster_graph (the motivating graph with its four-closure cluster, without a kernel and
under DCS), all at the poses after gauss_newton(20).  Groups of 1, 2, 5, 6 (m = 15, 18: either side of a 16-row tile), 11 (m = 33)
and 40 (m = 120, the cap) members are drawn with a fixed seed from closures and in-loop odometry.  A group whose REFERENCE pivot is
within a factor 10 of min_pivot = 1e-3 is borderline and not compared.  USABLE says how many groups per case and size the generator
must deliver (checked here on the CPU): at least 8 wherever the case's graph can lose that many edges at once -- a group larger
than the graph's cycle rank always disconnects it, so tree_shapes (10 loops) stops at 6, contributions (31) and
dcs_switches_closures_off (16 with the switched-off closures left out) at 11, angles_at_pi (2 loops) at 1; the 40-member groups come
from the cluster graphs (64 loops).  Every size class has at least 8 usable groups over the cases.

Bars (section 5f's convention: the worst ratio measured here against the long-double route, times 4, rounded
up to a power of two):
    d2      |d2 - ref| <= D2_BAR eps cond(K) ref        measured worst 147.9 (angles_at_pi, single edges) -> 1024
    pivot   |pivot - ref| <= PIVOT_BAR eps (1 + ||Nt||)  measured worst 18.3 (angles_at_pi) -> 128
with cond(K) and ||Nt|| from the long-double route.  The error the bars hold is the rule's own plus that of its fp64 inputs (N from
SuperLU solves with the full H), which dominates on the 40-pose chain of angles_at_pi.  Every test prints what it measured."""
import ctypes as C

import numpy as np
import pytest

import egroup_reference as eg
import loo_reference as lr
import mfront_cases as mc
from oracle import np_oracle as npo
from sparse_gslam_amd import capi

D2_BAR, PIVOT_BAR = 1024.0, 128.0
SEED = 5
CASES = ("tree_shapes", "contributions", "dcs_switches_closures_off", "angles_at_pi", "cluster", "cluster_dcs")
USABLE = {"tree_shapes": (1, 2, 5, 6), "contributions": (1, 2, 5, 6, 11), "dcs_switches_closures_off": (1, 2, 5, 6, 11),
          "angles_at_pi": (1,), "cluster": (1, 2, 5, 6, 11, 40), "cluster_dcs": (1, 2, 5, 6, 11, 40)}
_CACHE = {}


@pytest.fixture(autouse=True)
def _the_library_has_the_statistic():
    """the reference qualifies a statistic the library computes: without its entry points nothing here says anything"""
    for name in ("sgo_edge_joint", "sgo_edge_groups", "sgo_edge_group_rule"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name


def state(key):
    """(case, Edges at the poses after gauss_newton(20), a Refined of the full H): computed once, shared, never modified"""
    if key not in _CACHE:
        if key in ("cluster", "cluster_dcs"):
            c, _ = eg.cluster_graph(0.4, True) if key == "cluster_dcs" else eg.cluster_graph()
        else:
            c = mc.make(key)
        P = npo.gauss_newton(*c.arrays(), iters=20)[0]
        S = lr.Edges(P, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
        _CACHE[key] = (c, S, eg.Refined(S.H) if S.n else None)
    return _CACHE[key]


def groups(key):
    """the case's groups with their long-double references -> list of (edges, conditions, explicit or None where borderline)"""
    if ("groups", key) not in _CACHE:
        c, S, full = state(key)
        out = []
        for ks in eg.draw_groups(S, SEED):
            cond = eg.reference_conditions(S, ks, full)
            out.append((ks, cond, eg.explicit(S, ks) if cond["pivot"] >= 10 * eg.MIN_PIVOT else None))
        _CACHE[("groups", key)] = out
    return _CACHE[("groups", key)]


def rule(T):
    return capi.edge_group_rule(eg.info6(T["O"]), T["N"], T["e"], T["w"])


def test_symbols_are_bound():
    assert callable(capi.edge_group_rule) and callable(capi.Optimizer.edge_joint) and callable(capi.Optimizer.edge_groups)


@pytest.mark.parametrize("key", CASES)
def test_rule_and_closed_form_against_explicit_removal(key):
    c, S, _ = state(key)
    worst = dict(rule=0.0, closed=0.0, pivot=0.0, rel=0.0)
    usable = {}
    for ks, cond, ex in groups(key):
        if ex is None:
            continue
        T = eg.table(S, ks)
        rc, d2, piv, dof = rule(T)
        cf = eg.closed_form(T["O"], T["N"], T["e"], T["w"])
        assert rc == 0 and dof == 3 * len(ks) == ex["dof"] == cf["dof"]
        unit = eg.EPS * cond["condK"] * ex["d2"]
        worst["rule"] = max(worst["rule"], abs(d2 - ex["d2"]) / unit)
        worst["closed"] = max(worst["closed"], abs(cf["d2"] - ex["d2"]) / unit)
        worst["pivot"] = max(worst["pivot"], abs(piv - cond["pivot"]) / (eg.EPS * (1.0 + cond["normN"])),
                             abs(cf["pivot"] - cond["pivot"]) / (eg.EPS * (1.0 + cond["normN"])))
        worst["rel"] = max(worst["rel"], abs(d2 - ex["d2"]) / ex["d2"])
        assert -1e-12 <= piv <= 1.0 + 1e-12
        usable[len(ks)] = usable.get(len(ks), 0) + 1
    print(f"{key}: loops {eg.loops(S)}, usable groups by size {usable}, w in [{S.w.min():.3g}, {S.w.max():.3g}]; ratios to the units: rule "
          f"{worst['rule']:.4g}, closed form {worst['closed']:.4g}, pivot {worst['pivot']:.4g}; worst relative d2 {worst['rel']:.3g}")
    for k in USABLE[key]:
        assert usable.get(k, 0) >= 8, (key, k, usable)
    assert worst["rule"] <= D2_BAR and worst["closed"] <= D2_BAR and worst["pivot"] <= PIVOT_BAR, worst


def test_every_size_class_is_covered():
    for k in eg.SIZES:
        assert sum(k in USABLE[key] for key in CASES) >= 1, k
    assert max(eg.SIZES) == capi.JOINT_MAX_SUBSET
    # the weights of dcs_switches_closures_off: switched off, fractional and one -- and some group holds all three kinds
    _, S, _ = state("dcs_switches_closures_off")
    mixed = 0
    for ks, cond, ex in groups("dcs_switches_closures_off"):
        w = S.w[ks]
        mixed += ex is not None and (w < 1e-3).any() and ((w > 1e-3) & (w < 0.999)).any() and (w == 1.0).any()
    assert S.w.min() < 1e-6 and mixed >= 3, (S.w.min(), mixed)


def test_a_bridge_group_is_nan_and_does_not_fail():
    """long_thin_chain: every edge is a bridge; the reference's pivot is 0, the rule's is 0 up to rounding, and under the call's
    convention (pivot < min_pivot: d2 = NaN, no fail) nothing is decided"""
    c, S, full = state("long_thin_chain")
    assert eg.pool(S).size == 0 and eg.loops(S) == 0
    for ks in ([700], [10, 700, 701], list(range(300, 340))):
        T = eg.table(S, ks)
        rc, d2, piv, dof = rule(T)
        ref = eg.reference_conditions(S, ks, full)
        print(f"bridge group of {len(ks)}: rule pivot {piv:.3g}, reference pivot {ref['pivot']:.3g}")
        assert rc == 0 and dof == 3 * len(ks) and ref["pivot"] < 1e-9 and abs(piv) < 1e-6
        decided = piv >= eg.MIN_PIVOT
        d2 = d2 if decided else np.nan
        assert np.isnan(d2) and not (decided and d2 > 0.0)


@pytest.mark.parametrize("mutation", eg.MUTATIONS)
def test_mutations_are_rejected(mutation):
    """a wrong formula is told from the rule at 10 x the bar at least, on every group whose weights exercise it"""
    key = "cluster_dcs" if mutation == "w_ignored" else "dcs_switches_closures_off"
    c, S, _ = state(key)
    applies = dict(third_term_dropped=lambda w: ((w > 1e-3) & (w < 0.999)).any(), no_transpose=lambda w: (w > 1e-3).any(),
                   zero_information_kept=lambda w: True, w_ignored=lambda w: (w < 0.999).any())[mutation]
    caught = total = 0
    worst = 0.0
    for ks, cond, ex in groups(key):
        if ex is None or len(ks) < 2 or not applies(S.w[ks]):
            continue
        T = eg.table(S, ks)
        if mutation == "zero_information_kept":       # one member's information zeroed: the rule drops it, the mutant keeps it
            T["O"][0] = 0.0
            ref = eg.closed_form(T["O"][1:], T["N"][3:, 3:], T["e"][1:], T["w"][1:])
        else:
            ref = eg.closed_form(T["O"], T["N"], T["e"], T["w"])
        rc, d2, piv, dof = rule(T)
        unit = eg.EPS * cond["condK"] * abs(ref["d2"])
        assert abs(d2 - ref["d2"]) <= 2 * D2_BAR * unit, (mutation, ks)          # the rule sides with the right formula ...
        bad = eg.closed_form(T["O"], T["N"], T["e"], T["w"], mutation=mutation)
        off = abs(bad["d2"] - d2) / unit if np.isfinite(bad["d2"]) else np.inf   # ... (a mutant that breaks down is told too)
        if mutation == "zero_information_kept":
            off = max(off, np.inf if bad["dof"] != dof else 0.0)
        caught += off >= 10 * D2_BAR
        total += 1
        worst = max(worst, off)
    print(f"{mutation} on {key}: told on {caught} of {total} groups, largest distance {worst:.3g} units")
    assert total >= 8 and caught == total, (mutation, caught, total)


def test_the_motivating_cluster():
    """Four closures shifted together by 0.25 m: all pass the raw chi2 gate, three of the four pass the leave-one-out test, the group
    fails at the 0.99 quantile for 12 degrees of freedom.  Under DCS with a 0.4 m shift the singles read 4.0 / 35.4 / 6.6 / 2.2, the group 67.7."""
    c, S, full = state("cluster")
    grp = eg.CLUSTER
    one = lr.by_formulas(S, grp)
    T = eg.table(S, grp)
    rc, d2, piv, dof = rule(T)
    ex = eg.explicit(S, grp)
    print(f"raw e2 {np.round(S.e2[grp], 2)}, single d2 {np.round(one['d2'], 2)}, group d2 {d2:.6g} (explicit {ex['d2']:.6g}), pivot {piv:.4g}")
    assert (S.e2[grp] < eg.CHI2_99_DOF3).all()
    assert (one["d2"] < eg.CHI2_99_DOF3).sum() == 3
    assert rc == 0 and dof == 12 and piv >= 10 * eg.MIN_PIVOT and d2 > eg.CHI2_99_DOF12
    assert abs(d2 - 33.3) < 0.05 and abs(d2 - ex["d2"]) <= 1e-12 * ex["d2"]
    np.testing.assert_allclose(S.e2[grp], [3.1, 5.9, 1.2, 0.2], atol=0.06)
    np.testing.assert_allclose(one["d2"], [6.8, 17.6, 3.0, 1.2], atol=0.06)
    _, S1, _ = state("cluster_dcs")
    d2_dcs = rule(eg.table(S1, grp))[1]
    print(f"DCS: weights {np.round(S1.w[grp], 3)}, single d2 {np.round(lr.by_formulas(S1, grp)['d2'], 1)}, group d2 {d2_dcs:.4g}")
    np.testing.assert_allclose(lr.by_formulas(S1, grp)["d2"], [4.0, 35.4, 6.6, 2.2], atol=0.06)
    assert abs(d2_dcs - 67.7) < 0.05 and abs(d2_dcs - eg.explicit(S1, grp)["d2"]) <= 1e-12 * d2_dcs


def test_limits_of_the_formula():
    """k = 1: sgo_edge_loo_rule's closed form; w = 1: K = I - Nt; w = 0: K = I + Nt, the joint test's S"""
    done = ones = 0
    for key, (ks, cond, ex) in [(key, g) for key in ("cluster", "cluster_dcs") for g in groups(key)]:
        if ex is None:
            continue
        S = state(key)[1]
        T = eg.table(S, ks)
        k = len(ks)
        if k == 1:
            _, d2, piv, _ = rule(T)
            _, d2_loo, red, _ = capi.edge_loo_rule(eg.info6(T["O"][0]), T["N"], T["e"][0], T["w"][0])
            # (pivot bounds the redundancy, lambda_min of I - w N, from above)
            assert abs(d2 - d2_loo) <= 1e-12 * d2_loo / red and red - 1e-12 * (1.0 + cond["normN"]) <= piv <= 1.0
        if k in (5, 6):
            G = np.zeros((3 * k, 3 * k))
            for t in range(k):
                G[3 * t:3 * t + 3, 3 * t:3 * t + 3] = np.linalg.cholesky(T["O"][t])
            Nt, cv = G.T @ T["N"] @ G, G.T @ T["e"].reshape(-1)
            I = np.eye(3 * k)
            if (T["w"] == 1.0).all():     # (N was made with these weights: I - Nt is positive definite with them alone)
                _, d2, piv, _ = rule(T)
                assert abs(d2 - cv @ np.linalg.solve(I - Nt, cv)) <= 1e-10 * d2 / piv
                ones += 1
            _, d2, piv, _ = capi.edge_group_rule(eg.info6(T["O"]), T["N"], T["e"], np.zeros(k))
            Sj = np.linalg.inv(G @ G.T) + T["N"]
            ev = T["e"].reshape(-1)
            assert piv == 1.0 and abs(d2 - ev @ np.linalg.solve(Sj, ev)) <= 1e-10 * d2
        done += k in (1, 5, 6)
    assert done >= 48 and ones >= 16, (done, ones)


def test_special_cases_of_the_rule():
    c, S, _ = state("contributions")
    both_fixed = int(np.flatnonzero(S.fixed[S.ei] & S.fixed[S.ej])[0])
    ks = np.array([both_fixed, 61, 64, 70])
    T = eg.table(S, ks)
    ref = rule(T)
    assert ref[0] == 0 and ref[3] == 12 and np.isfinite(ref[1])
    # the empty group; a group of zero-information members alone
    assert capi.edge_group_rule(np.zeros((0, 6)), np.zeros((0, 0)), np.zeros((0, 3)), np.zeros(0)) == (0, 0.0, 1.0, 0)
    assert capi.edge_group_rule(np.zeros((2, 6)), T["N"][:6, :6], T["e"][:2], T["w"][:2]) == (1, 0.0, 1.0, 0)
    # a member with all-zero information is dropped: the bits of the group without it, and no degrees of freedom for it
    O = T["O"].copy()
    O[2] = 0.0
    keep = np.array([0, 1, 3])
    rows = np.repeat(np.isin(np.arange(4), keep), 3)
    a = capi.edge_group_rule(eg.info6(O), T["N"], T["e"], T["w"])
    b = capi.edge_group_rule(eg.info6(O[keep]), T["N"][np.ix_(rows, rows)], T["e"][keep], T["w"][keep])
    assert a[0] == 1 and b[0] == 0 and a[3] == b[3] == 9
    assert np.array_equal(np.array(a[1:3]).view(np.uint64), np.array(b[1:3]).view(np.uint64))
    # an information that is not positive definite: NaN, rc 2
    for bad in ([1.0, 2.0, 0.0, 1.0, 0.0, 1.0], [-1.0, 0.0, 0.0, 1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]):
        o6 = eg.info6(T["O"])
        o6[1] = bad
        rc, d2, piv, dof = capi.edge_group_rule(o6, T["N"], T["e"], T["w"])
        assert rc == 2 and np.isnan(d2) and np.isnan(piv) and dof == 12, bad
    # the edge between two fixed poses adds e^T Omega e exactly as a block of its own (N's rows are zero)
    assert np.all(T["N"][:3] == 0.0)
    alone = capi.edge_group_rule(eg.info6(T["O"][:1]), T["N"][:3, :3], T["e"][:1], T["w"][:1])
    assert alone[2] == 1.0 and abs(alone[1] - S.e2[both_fixed]) <= 1e-13 * S.e2[both_fixed]
    # above the cap, null outputs: refused
    k = capi.JOINT_MAX_SUBSET + 1
    assert capi.edge_group_rule(np.tile(eg.info6(np.eye(3)), (k, 1)), np.zeros((3 * k, 3 * k)), np.zeros((k, 3)), np.ones(k))[0] == -2
    assert capi.lib().sgo_edge_group_rule(1, capi._dp(np.ones(6)), capi._dp(np.zeros(9)), capi._dp(np.zeros(3)), capi._dp(np.ones(1)), None,
                                          C.byref(C.c_double()), None) == -2
