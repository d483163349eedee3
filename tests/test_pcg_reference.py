"""tests/pcg_reference.py without a GPU: a plain fp64 numpy model of the recurrence (pcg_reference.model), driven with the reference
operator on the small cases of tests/pcg_cases.py, stays under every constant; and every mutation of the model -- the defects a
converging CG hides -- is rejected at >= 10 x the bound by at least one case."""
import functools
import json

import numpy as np
import pytest

import kernel_reference as kr
import pcg_cases as pc
import pcg_reference as pr


@functools.lru_cache(maxsize=None)
def _system(name):
    """(case, operator, b, dinv) of a case: b and the block-diagonal inverse from the reference's own linearisation"""
    c = pc.case(name)
    op = pr.Operator(c.arrays)
    ref = kr.reference(*c.arrays)
    b = ref.b.astype(np.float64)
    D = ref.diag.astype(np.float64)
    inv = np.linalg.inv(D) if c.n else D
    inv = 0.5 * (inv + np.swapaxes(inv, 1, 2))
    dinv = np.stack([inv[:, 0, 0], inv[:, 0, 1], inv[:, 0, 2], inv[:, 1, 1], inv[:, 1, 2], inv[:, 2, 2]], axis=1)
    return c, op, b, dinv


def _matvec(op):
    return lambda x: op.products([x])[0][0].astype(np.float64)


def _variable(dinv):
    """a preconditioner that changes from iteration to iteration, in the K-cycle's place: the block-diagonal inverse, scaled per
    entry by a factor that depends on the iteration"""
    def M(r, k):
        w = 1.0 + 0.5 * np.cos(np.arange(r.size).reshape(r.shape) * (1.0 + k))
        return w * pr.dinv_apply(dinv, r, np.float64)[0]
    return M


def _run(name, caps=None, amg=False, **kw):
    c, op, b, dinv = _system(name)
    caps = c.caps if caps is None else caps
    states = pr.model(_matvec(op), b, dinv, caps, precond=_variable(dinv) if amg else None, **kw)
    x_prev = kw.get("x_prev")
    return pr.check_sequence(states, op, omega=kw.get("omega", 0.8), x_prev=x_prev), states


CONST_OF = dict(pq_row="dot", rr_row="dot", rz_row="dot", bb_row="dot", zq_row="dot", pq="dot", rr="dot", rz="dot", bb="dot", x="axpy", r="axpy",
                p="axpy", z="z", z0="z", xs0="xs", alpha="div", beta="div", probe_rel="div", tol2="tol", drift="drift")
CONSTANT = dict(dot=pr.C_DOT, axpy=pr.C_AXPY, z=pr.C_Z, xs=pr.C_XS, div=pr.C_DIV, tol=pr.C_TOL, drift=pr.C_DRIFT)


def _fold(worst, res, n):
    """the model's worst error / (U abs) per constant"""
    for key, v in res.items():
        st = key.split("@")[0]
        if st in CONST_OF and np.isfinite(v) and hasattr(v, "raw"):
            worst[CONST_OF[st]] = max(worst.get(CONST_OF[st], 0.0), v.raw)


def test_model_stays_under_every_constant():
    worst = {}
    for name in pc.CPU_CASES:
        c = pc.case(name)
        for amg in (False, True):
            if amg and name == "bj_lattice_b0":
                continue
            res, states = _run(name, caps=(0, 1, 2, 3, 4), amg=amg)
            assert not pr.failures(res), (name, amg, pr.failures(res))
            _fold(worst, res, c.n)
    # the bb_ref branch of the tolerance and a warm start, on one case each
    c, op, b, dinv = _system("bj_n86")
    bb = float(np.dot(b.ravel(), b.ravel()))
    for ref in (0.5 * bb, bb, 4.0 * bb, 1e30 * bb):
        res, st = _run("bj_n86", caps=(0, 1), bb_ref=ref)
        assert not pr.failures(res), (ref, pr.failures(res))
        _fold(worst, res, c.n)
    xstar = pr.model(_matvec(op), b, dinv, (400,))[400]
    assert xstar["S"]["stop"] == 1
    for f in (1.0, 0.5, 0.0, -1.0, 0.125):
        res, st = _run("bj_n86", caps=(0, 1, 2), amg=True, x_prev=f * xstar["x"])
        assert not pr.failures(res), (f, pr.failures(res))
        assert (st[0]["gamma_ref"] > 0.0) == (f in (1.0, 0.5)), (f, st[0]["gamma_ref"])
        _fold(worst, res, c.n)
    print("PCGREF model " + json.dumps({k: float(f"{v:.3g}") for k, v in worst.items()}))
    for k, v in worst.items():
        assert v <= pr.MODEL[k] * 1.005, (k, v, "pcg_reference.MODEL is out of date")
    for k, c in CONSTANT.items():       # the project's rule: 4 x the model's worst, up to a power of two, never above the provable bound
        rule = 2.0 ** np.ceil(np.log2(4.0 * pr.MODEL[k])) if pr.MODEL[k] > 0 else np.inf
        assert c == min(rule, pr.PROVABLE.get(k, np.inf)), (k, c, rule)


@pytest.mark.parametrize("name", ["bj_n1", "bj_n2", "bj_n86", "bj_n257", "bj_scaled_rows"])
def test_model_drift_over_whole_solves(name):
    """Every state of a whole solve, caps 0 .. N + 1: the drift bound accumulated over all N iterations holds the model at the end of
    the solve as it does after three iterations (its worst figures are early: the bound grows faster than the error)."""
    c, op, b, dinv = _system(name)
    N = pr.model(_matvec(op), b, dinv, (5000,))[5000]["S"]
    assert N["stop"] == 1
    res, st = _run(name, caps=tuple(range(0, N["iter"] + 2)))
    assert not pr.failures(res), pr.failures(res)
    assert f"drift@{N['iter']}" in res and f"frozen@{N['iter'] + 1}" in res
    worst = max(v.raw for k, v in res.items() if k.startswith("drift"))
    print(f"PCGREF model drift over the {N['iter']} iterations of {name}: {worst:.3g}, at the end {res['drift@%d' % N['iter']].raw:.3g}")
    assert worst <= pr.MODEL["drift"] * 1.005


def test_lattice_case_has_a_zero_right_hand_side():
    c, op, b, dinv = _system("bj_lattice_b0")
    assert not b.any()
    st = pr.model(_matvec(op), b, dinv, c.caps)
    assert st[0]["S"]["stop"] == 1 and st[1]["S"]["iter"] == 0
    assert not pr.failures(pr.check_sequence(st, op))


def test_negative_information_breaks_down_in_the_model():
    """stop 3 (p.Hp <= 0) in the CPU model: the breakdown branch of check_step"""
    arrays = pc.negative_information()
    op = pr.Operator(arrays)
    ref = kr.reference(*arrays)
    b = ref.b.astype(np.float64)
    inv = np.linalg.inv(ref.diag.astype(np.float64))
    dinv = np.stack([inv[:, 0, 0], inv[:, 0, 1], inv[:, 0, 2], inv[:, 1, 1], inv[:, 1, 2], inv[:, 2, 2]], axis=1)
    st = pr.model(_matvec(op), b, dinv, (0, 1, 2))
    assert st[1]["S"]["stop"] == 3 and st[1]["S"]["iter"] == 0 and st[1]["S"]["pq"] < 0.0
    res = pr.check_sequence(st, op)
    assert "breakdown@1" in res and "frozen@2" in res and not pr.failures(res), res


def _probe_window():
    """(probe_max between r.z / b.b and r.r / b.b at iteration 3 of bj_n86 under the variable preconditioner, r.r / b.b there)"""
    _, st = _run("bj_n86", caps=(0, 3), amg=True, probe_k=3)
    S = st[3]["S"]
    lo, hi = sorted((S["rz"] / S["bb"], S["rr"] / S["bb"]))
    assert hi > 4.0 * lo
    return float(np.sqrt(lo * hi)), S["rr"] / S["bb"]


def _mutant_runs(m):
    """the runs in which mutation m can show: (case, keyword arguments of _run)"""
    big = dict(caps=(0, 1, 2, 3, 4))
    if m == "tol2_uncapped":
        c, op, b, dinv = _system("bj_n86")
        return [("bj_n86", dict(caps=(0, 1), bb_ref=1e30 * float(np.dot(b.ravel(), b.ravel()))))]
    if m in ("gamma_above_4", "gamma_negative"):
        c, op, b, dinv = _system("bj_n86")
        xs = pr.model(_matvec(op), b, dinv, (400,))[400]["x"]
        return [("bj_n86", dict(caps=(0, 1), amg=True, x_prev=(0.125 if m == "gamma_above_4" else -1.0) * xs))]
    if m in ("plain_beta_variable_precond", "xs0_without_omega"):
        return [(n, dict(big, amg=True)) for n in ("bj_n86", "bj_n257")]
    if m == "probe_against_rz":
        return [("bj_n86", dict(caps=(0, 1, 2, 3, 4), amg=True, probe_k=3, probe_max=_probe_window()[0]))]
    if m == "stop_not_frozen":
        return [("bj_n1", dict(big)), ("bj_n2", dict(caps=tuple(range(0, 9))))]
    return [(n, dict(big)) for n in ("bj_n2", "bj_n86", "bj_n257")]


@pytest.mark.parametrize("mutation", pr.MUTATIONS)
def test_every_mutation_is_rejected(mutation):
    assert len(pr.MUTATIONS) >= 12
    worst = 0.0
    for name, kw in _mutant_runs(mutation):
        clean, _ = _run(name, **kw)
        assert not pr.failures(clean), (name, pr.failures(clean))
        res, _ = _run(name, mutate=mutation, **kw)
        worst = max([worst] + list(res.values()))
    print(f"PCGREF mutation {mutation}: worst figure {worst:.3g} x its bound")
    assert worst >= 10.0, (mutation, worst)


def test_probe_stops_the_model_on_either_side_of_the_record():
    mid, rel = _probe_window()
    _, st = _run("bj_n86", caps=(0, 1, 2, 3, 4), amg=True, probe_k=3, probe_max=rel * (1 + 1e-12))
    assert st[4]["S"]["stop"] != 4 and st[3]["S"]["probe_rel"] == rel
    res, st = _run("bj_n86", caps=(0, 1, 2, 3, 4), amg=True, probe_k=3, probe_max=rel * (1 - 1e-12))
    assert st[4]["S"]["stop"] == 4 and st[4]["S"]["iter"] == 3 and not pr.failures(res)
