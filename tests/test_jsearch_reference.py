"""The greedy search's reference and the library's host rule on the CPU (tests/jsearch_reference.py; sgo_joint_greedy_rule compiles
the text k_joint_grow compiles, sgo_rules.h; no GPU).  On the cases of jsearch_reference.CASES -- tree_shapes and child_own3_33 with 48
candidates, n = 1, 2, 65 and the cap of 256 on lattice_48 --, the seeds of jsearch_reference.seeds and both threshold ladders:
  * the reference's d2_path over every prefix agrees with joint_reference.subset_d2_long (a from-scratch factorisation in long double)
    to 1e-12 relative;
  * capi.joint_greedy_rule's orders, counts and stops equal the reference's for every seed whose margins are all >= 1e-8 -- at least
    nine seeds of ten per case and ladder (jsearch_reference.DEGENERATE lists the one combination that is a tie by construction) --,
    and its d2_path and d2_ext are within RULE_BAR of the reference's;
  * the reference with q not updated, the last pivot's w dropped from C, G's transpose used or ties broken high is rejected at ten
    times the bar or by its order;
  * an exact tie goes to the lower index, a seed whose block is not positive definite gives SGO_JSTOP_NOT_PD, count 0 and NaN, a NaN
    candidate is never chosen, and the rule refuses what sgo_joint_greedy refuses.
RULE_BAR = 1e-9: cond(S) <= 2e4 on these tables and at most 120 rows, so fp64 may lose 120 x 2e4 x 1.1e-16 = 2.7e-10 of a d2; the next
power of ten (the bar tests/test_joint_reference.py sets for the reference's own fp64 Cholesky).  Every test prints what it measured."""
import os
import re

import numpy as np
import pytest

import joint_reference as jr
import jsearch_reference as js
from sparse_gslam_amd import capi

RULE_BAR = 1e-9
PREFIX_BAR = 1e-12
COMBOS = [(name, ladder) for name in js.CASES for ladder in ("q99", "tight")]


def _every(name):
    return 16 if name == "n256" else 1


def test_symbols_are_bound():
    L = capi.lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgo.h")).read()
    for name in ("sgo_joint_greedy", "sgo_joint_extend"):
        assert name in capi.SYMBOLS and hasattr(L, name) and re.search(r"\bint " + name + r"\(sgo_ctx\* ctx", src), name
    assert "sgo_joint_greedy_rule" in capi.SYMBOLS and hasattr(L, "sgo_joint_greedy_rule")
    for k, v in (("MAX_LEN", capi.JSTOP_MAX_LEN), ("NONE", capi.JSTOP_NONE), ("NOT_PD", capi.JSTOP_NOT_PD)):
        assert re.search(rf"#define SGO_JSTOP_{k}\s+{v}\b", src), k
    assert (js.STOP_MAX_LEN, js.STOP_NONE, js.STOP_NOT_PD) == (capi.JSTOP_MAX_LEN, capi.JSTOP_NONE, capi.JSTOP_NOT_PD)
    assert L.sgo_version() == 107


@pytest.mark.parametrize("name", ["tree_shapes", "child_own3_33", "n65"])
def test_the_recurrence_equals_a_from_scratch_factorisation_on_every_prefix(name):
    _, _, S, e = js.table(name)
    n = e.shape[0]
    chi = js.ladders(S, e)["q99"]
    worst, sets = 0.0, 0
    for seed in js.seeds(n):
        r = js.greedy(S, e, seed, chi)
        for k in range(r.count + 1):
            want = jr.subset_d2_long(S, e, jr.masks([r.order[:k]], n)[0])
            worst = max(worst, jr.rel(r.d2_path[k], want))
            sets += 1
        assert np.isnan(r.d2_path[r.count + 1:]).all() and r.d2_path[0] == 0.0
    print(f"{name}: incremental d2 against the long-double from-scratch value over {sets} sets: {worst:.2e}")
    assert worst <= PREFIX_BAR


def test_the_extension_values_are_the_extended_sets_d2():
    _, _, S, e = js.table("tree_shapes")
    n = e.shape[0]
    r = js.greedy(S, e, [5, 17, 2, 40], None)
    assert r.count == 4 and r.stop == js.STOP_NONE
    want = np.array([jr.subset_d2_long(S, e, jr.masks([[5, 17, 2, 40] + ([c] if c not in (5, 17, 2, 40) else [])], n)[0]) for c in range(n)])
    err = jr.rel(r.d2_ext, want)
    print(f"d2_ext of a four-candidate list against {n} from-scratch factorisations: {err:.2e}")
    assert err <= PREFIX_BAR and all(r.d2_ext[c] == r.d2_path[4] for c in (5, 17, 2, 40))


@pytest.mark.parametrize("name,ladder", COMBOS)
def test_the_rule_against_the_reference(name, ladder):
    _, _, S, e = js.table(name)
    n = e.shape[0]
    chi = js.ladders(S, e)[ladder]
    seeds = js.seeds(n, _every(name))
    qualify, worst, err, counts = 0, 1.0, 0.0, []
    for seed in seeds:
        r = js.greedy(S, e, seed, chi)
        rc, order, count, stop, path, ext = capi.joint_greedy_rule(S, e, seed, chi)
        assert rc == 1
        worst = min(worst, r.margin)
        counts.append(r.count)
        if r.margin < js.MARGIN:
            continue
        qualify += 1
        assert np.array_equal(order, r.order) and count == r.count and stop == r.stop, (seed, order, r.order)
        assert np.array_equal(np.isnan(path), np.isnan(r.d2_path)) and np.array_equal(np.isnan(ext), np.isnan(r.d2_ext))
        m = ~np.isnan(path)
        err = max(err, jr.rel(path[m], r.d2_path[m]), jr.rel(ext[~np.isnan(ext)], r.d2_ext[~np.isnan(ext)]))
        assert all(ext[c] == path[count] for c in order[:count])
    print(f"{name} / {ladder}: {qualify} of {len(seeds)} seeds with every margin >= {js.MARGIN:g} (worst margin {worst:.1e}); paths of "
          f"{min(counts)} to {max(counts)} candidates; rule / reference {err:.2e}")
    if (name, ladder) in js.DEGENERATE:
        assert worst < js.MARGIN
    else:
        assert 10 * qualify >= 9 * len(seeds)
    assert err <= RULE_BAR


@pytest.mark.parametrize("mut", js.MUTATIONS)
def test_the_comparison_rejects_a_wrong_recurrence(mut):
    _, _, S, e = js.table("tree_shapes")
    n = e.shape[0]
    if mut == "ties_high":
        St, et = _tie_table(S, e)
        allow = np.zeros(n, dtype=np.uint8)
        allow[[3, 7]] = 1
        chi = js.ladders(S, e)["q99"]
        good, bad = js.greedy(St, et, [], chi, 1, allow), js.greedy(St, et, [], chi, 1, allow, mut=mut)
        assert good.order[0] == 3 and bad.order[0] == 7
        return
    seed = [5, 17, 2, 40, 11]
    good, bad = js.greedy(S, e, seed, None), js.greedy(S, e, seed, None, mut=mut)
    gap = max(jr.rel(bad.d2_path[:6], good.d2_path[:6]), jr.rel(bad.d2_ext, good.d2_ext))
    print(f"{mut}: d2_path and d2_ext of a five-candidate list off by {gap:.2e} (NaN: a block stopped being positive definite)")
    assert not gap <= 10 * RULE_BAR


def _tie_table(S, e):
    """candidate 7 replaced by a second copy of candidate 3: their rows, columns and innovations are the same numbers"""
    n = e.shape[0]
    src = np.arange(n)
    src[7] = 3
    rows = (3 * src[:, None] + np.arange(3)[None, :]).reshape(-1)
    return np.ascontiguousarray(S[np.ix_(rows, rows)]), np.ascontiguousarray(np.asarray(e)[src])


def test_an_exact_tie_goes_to_the_lower_index():
    _, _, S, e = js.table("tree_shapes")
    n = e.shape[0]
    St, et = _tie_table(S, e)
    chi = js.ladders(S, e)["q99"]
    allow = np.zeros(n, dtype=np.uint8)
    allow[[3, 7]] = 1
    rc, order, count, stop, path, ext = capi.joint_greedy_rule(St, et, [], chi, 1, allow)
    assert rc == 1 and count == 1 and order[0] == 3 and stop == capi.JSTOP_MAX_LEN
    # ... also two steps in, where both have gone through the same updates
    rc, order, count, _, _, _ = capi.joint_greedy_rule(St, et, [20, 30], chi, 3, allow)
    r = js.greedy(St, et, [20, 30], chi, 3, allow)
    assert rc == 1 and count == r.count and np.array_equal(order, r.order) and (count < 3 or order[2] == 3)


def test_a_seed_block_that_is_not_positive_definite_ends_the_seed():
    _, _, S, e = js.table("tree_shapes")
    Sn = S.copy()
    Sn[0:3, 0:3] *= -1.0
    chi = js.ladders(S, e)["q99"]
    for seed, done in (([0], 0), ([9, 4, 0, 6], 2)):
        rc, order, count, stop, path, ext = capi.joint_greedy_rule(Sn, e, seed, chi)
        r = js.greedy(Sn, e, seed, chi)
        assert rc == 1 and stop == capi.JSTOP_NOT_PD == r.stop and count == done == r.count
        assert np.array_equal(order, r.order) and list(order[:done]) == seed[:done] and (order[done:] == -1).all()
        assert np.isnan(ext).all() and np.isnan(path[done + 1:]).all() and not np.isnan(path[:done + 1]).any()


def test_a_nan_candidate_is_never_chosen():
    _, _, S, e = js.table("tree_shapes")
    Sn = S.copy()
    Sn[12:15, 12:15] *= -1.0                                               # candidate 4: its extension value is NaN from the start
    chi = js.ladders(S, e)["q99"]
    n = e.shape[0]
    grown = 0
    for seed in ([], [20], [7]):
        rc, order, count, stop, path, ext = capi.joint_greedy_rule(Sn, e, seed, chi)
        r = js.greedy(Sn, e, seed, chi)
        assert rc == 1 and 4 not in order and np.isnan(ext[4]) and np.isnan(r.d2_ext[4])
        assert np.array_equal(order, r.order) and count == r.count and stop == r.stop
        grown = max(grown, count)
    assert grown >= 10                                                     # (the paths do grow past it)


def test_allow_and_max_len():
    _, _, S, e = js.table("tree_shapes")
    n = e.shape[0]
    chi = js.ladders(S, e)["q99"]
    rc, order, count, stop, path, ext = capi.joint_greedy_rule(S, e, [3, 8], chi, 40, np.zeros(n))
    assert (rc, count, stop) == (1, 2, capi.JSTOP_NONE) and list(order[:3]) == [3, 8, -1]
    rc, order, count, stop, _, _ = capi.joint_greedy_rule(S, e, [3, 8], chi, 2)
    assert (rc, count, stop) == (1, 2, capi.JSTOP_MAX_LEN)
    full = capi.joint_greedy_rule(S, e, [3], chi)
    barred = int(full[1][1])
    allow = np.ones(n)
    allow[barred] = 0
    rc, order, count, _, _, _ = capi.joint_greedy_rule(S, e, [3], chi, 40, allow)
    assert rc == 1 and barred not in order[:count]
    assert capi.joint_greedy_rule(S, e, [3], None)[2:4] == (1, capi.JSTOP_NONE)      # no thresholds: no growth


def test_the_rule_refuses_what_the_call_refuses():
    _, _, S, e = js.table("tree_shapes")
    n = e.shape[0]
    chi = js.ladders(S, e)["q99"]
    bad_chi = chi.copy()
    bad_chi[17] = np.inf
    row = np.full(40, -1, dtype=np.int32)
    row[[0, 2]] = 4, 5                                                     # an entry after a -1
    for seed, ch, max_len in (([n], chi, 40), ([-3], chi, 40), ([4, 9, 4], chi, 40), ([4, 9, 5], chi, 2), ([4], chi, 41), ([4], bad_chi, 40),
                              (row[None, :], chi, 40)):
        rc, order, count, stop, path, ext = capi.joint_greedy_rule(S, e, seed, ch, max_len)
        assert rc == -2 and (order == -2).all() and count == -1 and stop == -1, (seed, max_len)
