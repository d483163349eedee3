"""Covariance-aware closure search: all listed poses against each query pose (sgo_closure_search; kernels in
sparse_gslam_amd/csrc/sgo_search.hip, driver in sgo_search.cpp, the pair rule in sgo_rules.h).

Reference: tests/search_reference.py -- SuperLU blocks of np_oracle's robustified Hessian AT THE DEVICE'S POSES through the block
formula (tests/test_search_reference.py qualifies it on the CPU).

Bars (derived in search_reference.py's docstring; scale = (|A|max sqrt(max |Sjj|) + |B|max sqrt(max |Scc|))^2):
    reference   |P - P_ref|max <= 9 DEVICE_BAR scale on EVERY pair, no cap; rel at 1e-12 (relative to max(1, |rel|))
    sharp       P, m2 and sigma against sgo_closure_search_rule fed the device's OWN blocks through the public API -- Sigma_jj and
                Sigma_cc from sgo_marginals_selected(diag), Sigma_jc from sgo_factor_solve on unit columns in hessian order, both
                bit-reproducible and panel-independent --: |P - P_rule|max <= RULE_BAR scale (FMA contraction), m2 and sigma at
                2 RULE_BAR scale / (u^T P u) relative.  This is what pins the gathers.
    decisions   near equals the reference's decision wherever search_reference.decided says the bar on P cannot move it; at least
                95 % of a test's pairs and 90 % of the reference's near pairs must be decided this way, asserted on the reference
                alone before the device is asked; the returned count is near.sum()
Every test prints what it measured."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mfront_cases as mc
import robust_reference as rr
import search_reference as sr
from selinv_reference import DEVICE_BAR
from sparse_gslam_amd import capi
from test_gpu_hypotheses import DIRECT, MFRONT, PCG, bits, graph, same_bits
from test_shim_replay import _write_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS, GATE = 2.0, 6.635          # metres; the 99 % quantile of chi2 with 1 degree of freedom
SENTINEL = -777.25


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _device_blocks(o, query):
    """The device's own blocks through the public API: (D (V, 3, 3) from marginals_selected, cross(c) -> (V, 3, 3) with
    cross[j][a][b] = Sigma_jc[a][b] from factor_solve on the unit columns of c in hessian order; None for a fixed c)"""
    D, _ = o.marginals_selected()
    free = o.free_ids()
    hidx = np.full(o.V, -1)
    hidx[free] = np.arange(free.size)
    cross = {}
    qs = [int(c) for c in dict.fromkeys(int(c) for c in query) if hidx[int(c)] >= 0]
    if qs:
        B = np.zeros((3 * len(qs), free.size, 3))
        for k, c in enumerate(qs):
            for b in range(3):
                B[3 * k + b, hidx[c], b] = 1.0
        X = o.factor_solve(B)
        for k, c in enumerate(qs):
            S = np.zeros((o.V, 3, 3))
            S[free] = X[3 * k:3 * k + 3].transpose(1, 2, 0)          # [hj][a][b] = X[b][hj][a]
            cross[c] = S
    return D, cross, hidx


def _sharp(o, query, ids, out, radius):
    """the worst ratios (P, m2, sigma) of the kernel's answers to sgo_closure_search_rule on the device's own blocks"""
    _, m2, rel, P, sg, _ = out
    D, cross, hidx = _device_blocks(o, query)
    worst = np.zeros(3)
    poses = o.get_poses()
    for a, c in enumerate(query):
        for b, j in enumerate(ids):
            if j == c:
                continue
            fj, fc = hidx[j] >= 0, hidx[c] >= 0
            rrel, rP, rm2, rsg = capi.closure_search_rule(poses[j], poses[c], D[j] if fj else None, cross[int(c)][j] if fj and fc else None,
                                                          D[c] if fc else None, radius)
            ref = sr.pair(poses[j], poses[c], D[j] if fj else None, cross[int(c)][j] if fj and fc else None, D[c] if fc else None, radius)
            scale, den = ref["scale"], ref["den"]
            assert np.abs(rel[a, b] - rrel).max() <= sr.RULE_BAR * max(1.0, np.abs(rrel).max()), (c, j)      # (sin and cos are the device's)
            if scale == 0.0:
                assert not P[a, b].any() and m2[a, b] == rm2 and not sg[a, b].any()
                continue
            worst[0] = max(worst[0], np.abs(P[a, b] - rP).max() / (sr.RULE_BAR * scale))
            if rm2 == 0.0 or np.isinf(rm2):
                assert m2[a, b] == rm2, (c, j, m2[a, b], rm2)
            else:
                norm = float(np.hypot(rrel[0], rrel[1]))      # (|t| carries two roundings, amplified by |t| - radius and squared)
                worst[1] = max(worst[1], abs(m2[a, b] - rm2) / rm2 / (2.0 * sr.RULE_BAR * scale / den + 8.0 * 2.0**-52 * norm / (norm - radius)))
            for k, var in enumerate((rsg[0] ** 2, rP[2, 2])):
                if var > 0.0:
                    worst[2] = max(worst[2], abs(sg[a, b, k] - rsg[k]) / rsg[k] / (2.0 * sr.RULE_BAR * scale / var))
    return worst


def _compare(name, g, o, query, ids, kind=None, delta=None, radius=RADIUS, gate=GATE, sharp=True):
    """The device's answers against the reference at the device's poses and against the rule on the device's own blocks"""
    query, ids = np.asarray(query, dtype=np.int32), np.asarray(ids, dtype=np.int32)
    S = sr.Reference(o.get_poses(), g.fixed, g.ei, g.ej, g.meas, g.info, g.phi, kind, delta)
    R = S.search(query, ids, radius, gate)
    dec = sr.decided(R, radius, gate)
    nnear = int(R["near"].sum())
    within = int(((R["norm"] <= radius) & (ids[None, :] != query[:, None])).sum())
    assert dec.mean() >= 0.95 and (dec & R["near"]).sum() >= 0.9 * nnear, (name, dec.mean(), (dec & R["near"]).sum(), nnear)
    out = o.closure_search(query, ids, radius, gate)
    count, m2, rel, P, sg, near = out
    other = ids[None, :] != query[:, None]
    dP = np.abs(P - R["P"]).reshape(query.size, ids.size, 9).max(2)
    free = other & (R["scale"] > 0.0)
    assert not dP[~free].any() and not P[~free].any()                                     # two fixed poses, or the query itself: P = 0 exactly
    rP = dP[free] / (9.0 * DEVICE_BAR * R["scale"][free])
    rrel = np.abs(rel - R["rel"]).max(2) / (sr.REL_BAR * np.maximum(1.0, np.abs(R["rel"]).max(2)))
    worst = _sharp(o, query, ids, out, radius) if sharp else np.full(3, np.nan)
    print(f"{name}: {query.size} x {ids.size} pairs, {within} within {radius} m, {nnear} near in the reference ({int(near.sum())} on the device), "
          f"decided {dec.mean():.2%} of the pairs and {(dec & R['near']).sum()} of the near ones; ratios to the bars: P against the reference "
          f"{rP.max():.3g}, rel {rrel.max():.3g}; against the rule on the device's blocks: P {worst[0]:.3g}, m2 {worst[1]:.3g}, sigma {worst[2]:.3g}")
    assert rP.max() <= 1.0 and rrel.max() <= 1.0, (name, rP.max(), rrel.max())
    if sharp:
        assert (worst <= 1.0).all(), (name, worst)
    assert np.array_equal(near[dec], R["near"][dec]), (name, np.argwhere(dec & (near != R["near"])))
    assert count == int(near.sum())
    assert np.array_equal(near, (m2 <= gate) & other)
    assert np.array_equal(bits(P), bits(P.transpose(0, 1, 3, 2).copy()))                  # exactly symmetric
    same = ~other
    assert not m2[same].any() and not rel[same].any() and not P[same].any() and not sg[same].any() and not near[same].any()
    return R, out


# ------------------------------------------------------------------ the stage cases: fixed poses inside, duplicate edges, a multi-level tree
@pytest.mark.parametrize("name", ["contributions", "tree_shapes"])
def test_cases_of_the_stage_tests(name):
    c = mc.make(name)
    V = c.poses.shape[0]
    fx = int(np.flatnonzero(c.fixed)[-1])
    with mc.environment(c.env), capi.Optimizer(0, direct_rows=1, profile=1) as o:
        o.set_graph(*c.arrays())
        assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
        assert o.optimize(20)[0] == 20
        _compare(name, c, o, [V - 1, V // 2, fx], np.arange(V))
        # a fixed query costs no solve: no substitution launch at all
        o.profile_reset()
        o.closure_search([fx], np.arange(V), RADIUS, GATE)
        prof = o.kernel_profile()
        print(f"{name}: a fixed query launched {sorted(prof)}")
        assert "k_closure_search" in prof and "k_si_panels" in prof
        assert "k_fs_forward" not in prof and "k_fs_backward" not in prof and "k_fs_rhs" not in prof
        o.profile_reset()
        o.closure_search([fx, V - 1], np.arange(V), RADIUS, GATE)
        assert "k_fs_forward" in o.kernel_profile()


# ------------------------------------------------------------------ the two factorisation paths of optimize(), each with a plan of its own kind
@functools.lru_cache(maxsize=None)
def _mfront_ids():
    """every pose the reference finds near query V - 1 at the initial poses, filled up to 200 with a default_rng(5) draw"""
    g = graph(MFRONT)
    S = sr.Reference(g.poses, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi)
    near = np.flatnonzero(S.search([g.V - 1], np.arange(g.V), RADIUS, GATE)["near"][0])
    rest = np.setdiff1d(np.arange(g.V), near)
    return np.r_[near, np.random.default_rng(5).choice(rest, 200 - near.size, replace=False)].astype(np.int32), near.size


@pytest.mark.parametrize("shape,path", [(DIRECT, "direct_ldlt"), (MFRONT, "multifrontal_cholesky")], ids=["direct", "mfront"])
def test_mid_size_graphs(shape, path):
    """six queries are 18 columns: the last one straddles the 16-column panel boundary"""
    g = graph(shape)
    V = g.V
    if shape == DIRECT:
        ids, query = np.arange(V), [V - 1, 300, 0, V // 4, (3 * V) // 4, V - 2]
    else:
        ids, nnear = _mfront_ids()
        query = [V - 1, V // 2, 0, V // 4, (3 * V) // 4, V - 2]
        print(f"{shape}: {nnear} reference-near poses of query {V - 1} among the 200 ids")
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        desc = o.solver_description()
        assert desc.startswith(path), desc
        R, out = _compare(str(shape), g, o, query, ids)
        assert o.solver_description() == desc
        within = ((R["norm"][0] <= RADIUS) & (ids != query[0])).sum()
        assert out[5][0].sum() > within, (out[5][0].sum(), within)                    # the search keeps more than the Euclidean threshold
        assert o.optimize(3)[0] == 3


# ------------------------------------------------------------------ chunks of queries
def test_more_queries_than_one_chunk_of_columns():
    """86 free queries are 258 columns: two chunks; every answer has the bits of the same query asked alone"""
    g = graph(DIRECT)
    ids = np.array([0, 5, 17, 300, 301, 598, 599, 42], dtype=np.int32)
    query = np.r_[np.arange(100, 185), 599].astype(np.int32)
    assert query.size == 86 and not g.fixed[query].any()
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.optimize(5)
        A = o.closure_search(query, ids, RADIUS, GATE)
        assert A[0] == int(A[5].sum())
        for q in (0, 4, 5, 84, 85):
            B = o.closure_search(query[[q]], ids, RADIUS, GATE)
            for a, b in zip(A[1:5], B[1:5]):
                assert same_bits(a[q], b[0]), q
            assert np.array_equal(A[5][q], B[5][0])
        alone = sum(o.closure_search(query[[q]], ids, RADIUS, GATE)[0] for q in range(query.size))
        print(f"86 queries x 8 ids: {A[0]} near pairs in one call, {alone} asked one by one")
        assert alone == A[0]


# ------------------------------------------------------------------ what a list means
def test_list_semantics():
    g = graph(MFRONT)
    V = g.V
    ids = np.r_[np.arange(0, V, 13), V - 1, V - 3].astype(np.int32)
    query = np.array([V - 1, 700, 0, 1900], dtype=np.int32)
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.optimize(5)
        A = o.closure_search(query, ids, RADIUS, GATE)
        again = o.closure_search(query, ids, RADIUS, GATE)
        for a, b in zip(A[1:5], again[1:5]):                                          # two calls, the same bits
            assert same_bits(a, b)
        assert A[0] == again[0] and np.array_equal(A[5], again[5])
        rng = np.random.default_rng(3)
        pick = rng.permutation(ids.size)[:50]                                         # a subset in another order, queries in another order
        qo = np.array([3, 0, 2, 1])
        B = o.closure_search(query[qo], ids[pick], RADIUS, GATE)
        for a, b in zip(A[1:5], B[1:5]):
            assert same_bits(a[qo][:, pick], b)
        assert np.array_equal(A[5][qo][:, pick], B[5]) and B[0] == int(B[5].sum())
        dup = o.closure_search([700, V - 1, 700], [V - 1, 26, 26, 700], RADIUS, GATE)     # duplicates are answered twice; j == c
        for f in dup[1:5]:
            assert same_bits(f[0], f[2]) and same_bits(f[:, 1], f[:, 2])
        assert dup[1][1, 0] == 0.0 and not dup[3][1, 0].any() and not dup[5][1, 0] and dup[1][0, 3] == 0.0 and not dup[5][0, 3]
        k = list(ids).index(26)
        assert same_bits(dup[1][0, 1], A[1][1, k]) and same_bits(dup[3][0, 1], A[3][1, k])
        # min_sep clears near alone
        full = o.closure_search([V - 1], None, RADIUS, GATE)
        sep = o.closure_search([V - 1], None, RADIUS, GATE, min_sep=50)
        for a, b in zip(full[1:5], sep[1:5]):
            assert same_bits(a, b)
        far = np.abs(np.arange(V) - (V - 1)) >= 50
        assert np.array_equal(sep[5][0], full[5][0] & far) and sep[0] == int(sep[5].sum()) < full[0]
        assert full[5][0][~far].any()
        print(f"query {V - 1}: {full[0]} near poses, {sep[0]} of them at least 50 poses away")


def test_a_vertex_without_an_edge_is_nan_without_ids():
    """a hand-made chain of 7 poses with a loop, vertex 4 left out: NaN row and near = 0 without ids, a refusal with ids"""
    P = np.array([[0, 0, 0], [1, 0, 0.1], [2, 0.2, 0.2], [3, 0.5, 0.2], [9, 9, 0], [3.5, 1.5, 1.2], [2.5, 2.0, 2.5]], dtype=np.float64)
    fixed = np.zeros(7, dtype=bool)
    fixed[0] = True
    ei = np.array([0, 1, 2, 3, 5, 6], dtype=np.int32)
    ej = np.array([1, 2, 3, 5, 6, 1], dtype=np.int32)
    from sparse_gslam_amd import synth
    meas = synth._rel(P[ei], P[ej])
    info = np.tile(np.array([400.0, 0, 0, 400.0, 0, 2500.0]), (6, 1))
    phi = np.full(6, -1.0)

    class G:
        pass
    g = G()
    g.fixed, g.ei, g.ej, g.meas, g.info, g.phi = fixed, ei, ej, meas, info, phi
    with capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(P, fixed, ei, ej, meas, info, phi)
        count, m2, rel, cov, sg, near = o.closure_search([6, 0], None, 1.2, GATE)
        assert np.isnan(m2[:, 4]).all() and np.isnan(rel[:, 4]).all() and np.isnan(cov[:, 4]).all() and np.isnan(sg[:, 4]).all()
        assert not near[:, 4].any() and count == int(near.sum())
        keep = np.array([0, 1, 2, 3, 5, 6])
        R = sr.Reference(P, fixed, ei, ej, meas, info, phi).search([6, 0], keep, 1.2, GATE)
        ratio = (np.abs(cov[:, keep] - R["P"]).reshape(2, 6, 9).max(2)[R["scale"] > 0] / (9 * DEVICE_BAR * R["scale"][R["scale"] > 0])).max()
        print(f"7 poses, one without an edge: P at {ratio:.3g} of the bar, near {near.astype(int).tolist()}")
        dec = sr.decided(R, 1.2, GATE)
        assert ratio <= 1.0 and dec.mean() >= 0.9 and np.array_equal(near[:, keep][dec], R["near"][dec])
        m2s = np.full(2, SENTINEL)
        for q, ids in (([6], [3, 4]), ([4], [3, 5])):
            qa, ia = np.array(q, dtype=np.int32), np.array(ids, dtype=np.int32)
            rc = capi.lib().sgo_closure_search(o._h, 1, capi._ip(qa), 2, capi._ip(ia), 0.5, GATE, 0, capi._dp(m2s), None, None, None, None)
            assert rc == -2 and "no edge" in o.last_error() and np.all(m2s == SENTINEL), (rc, o.last_error())


# ------------------------------------------------------------------ refusals
def test_the_analysis_refusing_the_graph_returns_enothing():
    g = graph(PCG)
    m2, near = np.full(8, SENTINEL), np.full(8, 7, dtype=np.uint8)
    q, ids = np.array([g.V - 1], dtype=np.int32), np.arange(8, dtype=np.int32)
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*g.arrays())
        o.optimize(2)
        for _ in range(2):
            rc = capi.lib().sgo_closure_search(o._h, 1, capi._ip(q), 8, capi._ip(ids), RADIUS, GATE, 0, capi._dp(m2), None, None, None, _u8(near))
            assert rc == -1 and "sgo_candidate_gate" in o.last_error() and "refuses" in o.last_error(), (rc, o.last_error())
            with pytest.raises(capi.SgoError, match="rc=-1"):
                o.closure_search(q, ids, RADIUS, GATE)
        assert np.all(m2 == SENTINEL) and np.all(near == 7)
        assert o.optimize(2)[0] == 2


def _raw(o, nq, query, n, ids, radius, chi2, min_sep, outs, null_m2=False):
    m2, rel, cov, sg, near = outs
    return capi.lib().sgo_closure_search(o._h, nq, None if query is None else capi._ip(query), n, None if ids is None else capi._ip(ids), radius, chi2,
                                         min_sep, None if null_m2 else capi._dp(m2), capi._dp(rel), capi._dp(cov), capi._dp(sg), _u8(near))


def _sentinels(nq, n):
    return (np.full((nq, n), SENTINEL), np.full((nq, n, 3), SENTINEL), np.full((nq, n, 9), SENTINEL), np.full((nq, n, 2), SENTINEL),
            np.full((nq, n), 7, dtype=np.uint8))


def _untouched(outs):
    return all(np.all(a == SENTINEL) for a in outs[:4]) and np.all(outs[4] == 7)


def test_refusals_leave_the_outputs_untouched():
    g = graph(DIRECT)
    nq, n = 2, 4
    outs = _sentinels(nq, n)
    q, ids = np.array([599, 300], dtype=np.int32), np.arange(n, dtype=np.int32)
    bad = lambda a, k, v: np.array([v if i == k else x for i, x in enumerate(a)], dtype=np.int32)
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.optimize(3)
        P = o.get_poses()
        refusals = [(-1, q, n, ids, RADIUS, GATE, 0, False), (nq, q, -1, ids, RADIUS, GATE, 0, False), (nq, None, n, ids, RADIUS, GATE, 0, False),
                    (nq, q, n, ids, RADIUS, GATE, 0, True), (nq, q, g.V + 1, None, RADIUS, GATE, 0, False),
                    (nq, q, n, bad(ids, 1, g.V), RADIUS, GATE, 0, False), (nq, q, n, bad(ids, 2, -1), RADIUS, GATE, 0, False),
                    (nq, bad(q, 1, g.V), n, ids, RADIUS, GATE, 0, False), (nq, bad(q, 0, -3), n, ids, RADIUS, GATE, 0, False),
                    (nq, q, n, ids, -0.5, GATE, 0, False), (nq, q, n, ids, np.inf, GATE, 0, False), (nq, q, n, ids, np.nan, GATE, 0, False),
                    (nq, q, n, ids, RADIUS, np.inf, 0, False), (nq, q, n, ids, RADIUS, np.nan, 0, False), (nq, q, n, ids, RADIUS, GATE, -1, False)]
        for a in refusals:
            assert _raw(o, *a[:7], outs, a[7]) == -2, a
            assert "sgo_closure_search" in o.last_error()
        assert _untouched(outs) and same_bits(o.get_poses(), P)
        assert _raw(o, 0, q, n, ids, RADIUS, GATE, 0, outs) == 0 and _raw(o, nq, q, 0, ids, RADIUS, GATE, 0, outs) == 0
        assert _raw(o, 0, None, 0, None, RADIUS, GATE, 0, outs, True) == 0 and _untouched(outs)
        assert _raw(o, nq, q, n, ids, 0.0, GATE, 0, outs) >= 0 and not _untouched(outs)              # radius 0 is allowed
        assert o.closure_search(q, ids, RADIUS, -1.0)[0] == 0                                         # ... and a gate nothing passes
    outs = _sentinels(nq, n)
    with capi.Optimizer(0) as o:
        assert _raw(o, nq, q, n, ids, RADIUS, GATE, 0, outs) == -4                                    # no graph
    with capi.Optimizer(0, direct_rows=0, solver=capi.SOLVER_PCG_BJ) as o:                            # a multi-GPU context's emulation
        o.debug_set_shard(2, 0)
        o.set_graph(*g.arrays())
        assert _raw(o, nq, q, n, ids, RADIUS, GATE, 0, outs) == -2 and "multi-GPU" in o.last_error()
    assert _untouched(outs)


def test_an_active_overlay_is_refused():
    from test_gpu_edge_gate import _grow, _overlay_session
    base, steps, gg = _overlay_session()[:3]
    outs = _sentinels(1, 4)
    q = np.array([3], dtype=np.int32)
    with capi.Optimizer(0, direct_rows=0) as o:
        _grow(o, base, steps, gg, 6)
        assert "incremental overlay" in o.solver_description()
        assert _raw(o, 1, q, 4, None, RADIUS, GATE, 0, outs) == -2 and "overlay" in o.last_error() and _untouched(outs)


def test_a_graph_without_a_free_pose():
    """every active vertex fixed: nothing to factorise, P = 0, m2 is 0 inside the radius and +inf outside"""
    c = mc.make("root_own3_6")
    V = c.poses.shape[0]
    with capi.Optimizer(0) as o:
        o.set_graph(c.poses, np.ones_like(c.fixed), *c.arrays()[2:])
        count, m2, rel, P, sg, near = o.closure_search([V - 1, 0], None, 1.2, GATE)
    R = sr.Reference(c.poses, np.ones_like(c.fixed), c.ei, c.ej, c.meas, c.info, c.phi).search([V - 1, 0], np.arange(V), 1.2, GATE)
    assert not P.any() and not sg.any() and np.array_equal(m2, R["m2"]) and np.isinf(m2).any() and (m2 == 0).sum() > 2
    assert np.array_equal(near, R["near"]) and count == int(near.sum()) and np.abs(rel - R["rel"]).max() <= 1e-12


def test_an_indefinite_hessian_fails_and_leaves_the_outputs():
    """the failure path of test_gpu_fsolve.py's indefinite graph (negated information: a pivot block fails its test, no fault)"""
    import test_gpu_mfront as tmf
    g = tmf.chain_graph(700, 150, seed=16)
    info = g.info.copy()
    info[:, [0, 3, 5]] *= -1.0
    outs = _sentinels(2, 4)
    q = np.array([650, 0], dtype=np.int32)
    with capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)
        assert o.solver_description().startswith("multifrontal_cholesky")
        rc = _raw(o, 2, q, 4, None, RADIUS, GATE, 0, outs)
        assert rc == -2 and "not positive definite" in o.last_error(), (rc, o.last_error())
        assert _untouched(outs)
        rc, st = o.optimize(5)                           # as without the call: fails at iteration 0, the estimates stay
        assert rc == 0 and st["iters_done"] == 0 and np.array_equal(o.get_poses(), g.poses)


# ------------------------------------------------------------------ no footprint
@pytest.mark.parametrize("shape,path", [(DIRECT, "direct_ldlt"), (MFRONT, "multifrontal_cholesky")], ids=["direct", "mfront"])
def test_a_later_optimize_has_the_bits_of_a_context_that_never_called(shape, path):
    g = graph(shape)
    with capi.Optimizer(0) as opt, capi.Optimizer(0) as fresh:
        for o in (opt, fresh):
            o.set_graph(*g.arrays())
            assert o.solver_description().startswith(path)
        a = [opt.optimize(5)]
        A = opt.closure_search([g.V - 1, 0, 300], None, RADIUS, GATE)
        B = opt.closure_search([g.V - 1, 0, 300], None, RADIUS, GATE)
        for x, y in zip(A[1:5], B[1:5]):
            assert same_bits(x, y)
        a.append(opt.optimize(20))
        b = [fresh.optimize(5), fresh.optimize(20)]
        assert same_bits(opt.get_poses(), fresh.get_poses())
        if shape == MFRONT:
            assert same_bits(opt.mfront_arrays(("X",))["X"], fresh.mfront_arrays(("X",))["X"])
    for (d, st), (df, sf) in zip(a, b):
        assert d == df and st["chi2"] == sf["chi2"] and st["robust_chi2"] == sf["robust_chi2"]


def test_marginals_selected_and_factor_solve_keep_their_bits_around_the_call():
    g = graph(DIRECT)
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.optimize(20)
        B = np.zeros((1, o.n_free, 3))
        B[0, 17, 1] = 1.0
        D0, X0 = o.marginals_selected()[0], o.factor_solve(B)
        o.closure_search([g.V - 1, 5], None, RADIUS, GATE)
        assert same_bits(o.marginals_selected()[0], D0) and same_bits(o.factor_solve(B), X0)


# ------------------------------------------------------------------ robust kernels: the weighted Hessian
def test_mixed_kernel_kinds():
    g = graph(MFRONT)
    cl = np.flatnonzero(g.phi >= 0)
    kind = np.zeros(g.E, dtype=np.int32)
    kind[cl] = np.array([rr.DCS, rr.HUBER, rr.CAUCHY, rr.TUKEY])[np.arange(cl.size) % 4]
    delta = np.where(g.phi >= 0, 1.5, 1.0)
    delta[kind == rr.DCS] = 10.0
    V = g.V
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.set_robust_kernels(np.arange(g.E), kind, delta)
        assert o.optimize(20)[0] == 20
        # the poses whose estimates lie within 10 m of a query (where the near ones are) and every 25th of the rest
        P = o.get_poses()
        query = np.array([V - 1, V // 2, V // 4, (3 * V) // 4])
        close = np.min([np.hypot(*(P[:, :2] - P[q, :2]).T) for q in query], axis=0) < 10.0
        ids = np.union1d(np.flatnonzero(close), np.arange(0, V, 25)).astype(np.int32)
        _, w = o.edge_robust()
        assert (w[cl] < 0.999).sum() >= 20, (w[cl] < 0.999).sum()
        R, out = _compare("mixed kinds", g, o, query, ids, kind=kind, delta=delta)
        # the unweighted Hessian is another answer: the bar tells the two apart
        U = sr.Reference(P, g.fixed, g.ei, g.ej, g.meas, g.info, np.full(g.E, -1.0)).search(query[:1], ids, RADIUS, GATE)
        other = ids != query[0]
        apart = (np.abs(U["P"][0] - R["P"][0]).reshape(ids.size, 9).max(1)[other] / (9 * DEVICE_BAR * R["scale"][0][other])).max()
        print(f"the unweighted Hessian's P is {apart:.3g} bars away")
        assert apart > 1.0


# ------------------------------------------------------------------ the compat headers
@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    """replay_closure_search, built with the g++ line test_gpu_edge_loo.py uses"""
    libdir = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("replay_closure_search") / "replay_closure_search")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "replay_closure_search.cpp"), "-L" + libdir, "-lsgo", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_the_call_through_the_compat_headers(replay, tmp_path):
    """SparseOptimizer::sgoClosureSearch in the place of the reference's max_match_distance filter: its shortlist is the C-ABI
    call's at the same estimates, it holds the Euclidean shortlist, and the call returns -1 where it must"""
    g = graph(DIRECT)
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 10.0)
    env = dict(os.environ)
    for k in ("SGO_DIRECT_ROWS", "SGO_INCREMENTAL", "SGO_SOLVER"):
        env.pop(k, None)
    res = subprocess.run([replay, str(gf), str(of), "8", repr(RADIUS), repr(GATE), "20"], env=env, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    lines = open(of).read().split("\n")
    assert int(lines[0]) == 8 and lines[1].startswith("direct_ldlt") and lines[2] == lines[1], lines[:3]
    P = np.array([[float(v) for v in ln.split()] for ln in lines[3:3 + g.V]])
    rows = [ln.split() for ln in lines[3 + g.V:] if ln and ln.split()[0] == "pose"]
    tail = dict(ln.split() for ln in lines[3 + g.V:] if ln and ln.split()[0] in ("count", "by_pointer", "not_active", "stale", "levenberg", "refused"))
    assert len(rows) == g.V
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P)
        count, m2, rel, _, sg, near = opt.closure_search([g.V - 1], None, RADIUS, GATE, min_sep=20)
    euclid = np.array([int(r[2]) for r in rows], dtype=bool)
    shortlist = np.array([int(r[6]) for r in rows], dtype=bool)
    # (equal values: the text carries 17 digits)
    assert np.array_equal(np.array([float(r[3]) for r in rows]), m2[0]) and np.array_equal(np.array([float(r[4]) for r in rows]), sg[0, :, 0])
    assert np.array_equal(shortlist, near[0]) and int(tail["count"]) == count == int(tail["by_pointer"])
    assert np.array_equal(euclid, np.hypot(rel[0, :, 0], rel[0, :, 1]) < RADIUS)
    far = np.abs(np.arange(g.V) - (g.V - 1)) >= 20
    assert shortlist[euclid & far].all() and not shortlist[~far].any()
    print(f"the reference's filter keeps {int((euclid & far).sum())} poses at least 20 poses away, the search {int(shortlist.sum())}")
    assert all(int(tail[k]) == -1 for k in ("not_active", "stale", "levenberg", "refused")), tail
    said = [ln for ln in res.stderr.split("\n") if "sgoClosureSearch" in ln]
    assert len(said) == 4, res.stderr
