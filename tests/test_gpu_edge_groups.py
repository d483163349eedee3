"""The leave-group-out test of clusters of resident edges (sgo_edge_joint, sgo_edge_groups; kernels k_edge_cands, k_edge_table and
k_edge_groups in sparse_gslam_amd/csrc/sgo_egroup.hip, drivers in sgo_fsolve.cpp and sgo_egroup.cpp, the rule in sgo_rules.h;
DESIGN.md section 5m).

Reference: tests/egroup_reference.py's table (SuperLU solves with np_oracle's robustified Hessian) and closed form AT THE DEVICE'S
POSES; tests/test_egroup_reference.py qualifies both against the explicit removal in long double on the CPU.  Groups as there: 1, 2,
5, 6, 11 and 40 members from closures and in-loop odometry; a group whose reference pivot is within a factor 10 of min_pivot = 1e-3 is
borderline and not compared.

Bars.  N at selinv_reference.DEVICE_BAR = 1e-6 of max |N_ref|, d2 at 1e-6 relative (tests/test_gpu_joint.py's); the cases
selinv_reference.ILL_CONDITIONED names are checked for finite values only.  Against sgo_candidate_joint on the same context:
1e-12 of max |N|.  Single-edge groups against sgo_edge_leave_one_out: 2e-6 relative.  sgo_edge_groups against sgo_edge_group_rule on
the exported table: the device contracts a b + c into one rounding, the host's compiler does not, so the two are two fp64
evaluations of one formula, each within test_egroup_reference.D2_BAR eps cond(K) of the exact value of ITS inputs -- here the same
inputs: the bar is 2 D2_BAR eps cond(K) d2, and the test prints how many groups agree bit for bit (measured: 0 to 15 of a case's 15 to
61 groups; the others within 6.8 of the unit, bar 2 048 -- the bar holds, bit equality does not).  Batch independence, repeated
calls, the snapshot, non-interference and refusals are bit for bit.  Every test prints what it measured."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import egroup_reference as eg
import loo_reference as lr
import mfront_cases as mc
import selinv_reference as sr
from oracle import np_oracle as npo
from sparse_gslam_amd import capi
from test_egroup_reference import D2_BAR, PIVOT_BAR, SEED
from test_gpu_hypotheses import DIRECT, MFRONT, bits, graph, same_bits
from test_shim_replay import _write_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = sr.DEVICE_BAR
SENTINEL = -777.25
u8p = C.POINTER(C.c_uint8)


def _case(name):
    if name in ("cluster", "cluster_dcs"):
        return eg.cluster_graph(0.4, True)[0] if name == "cluster_dcs" else eg.cluster_graph()[0]
    return mc.make(name)


def _masks(groups, edges):
    M = np.zeros((len(groups), edges.size), dtype=np.uint8)
    for b, ks in enumerate(groups):
        M[b, np.searchsorted(edges, ks)] = 1
    return M


def _listed(S, seed=SEED):
    """the groups of egroup_reference.draw_groups at S's poses whose union stays within the table's cap, and that union, sorted"""
    keep, union = [], set()
    for ks in eg.draw_groups(S, seed):
        if len(union | set(int(k) for k in ks)) > capi.JOINT_MAX_CANDIDATES:
            continue
        union |= set(int(k) for k in ks)
        keep.append(ks)
    return keep, np.array(sorted(union), dtype=np.int32)


def _reference(S, edges, groups):
    """the reference table of `edges` and every group's closed form on it"""
    T = eg.table(S, edges)
    out = []
    for ks in groups:
        t = np.searchsorted(edges, ks)
        rows = (3 * t[:, None] + np.arange(3)).reshape(-1)
        out.append(eg.closed_form(T["O"][t], T["N"][np.ix_(rows, rows)], T["e"][t], T["w"][t]))
    return T, out


def _open(c, **opts):
    o = capi.Optimizer(0, **({"direct_rows": 1} | opts))
    o.set_graph(*c.arrays())
    return o


def _rule_on_table(c, edges, ks, N, e, w):
    t = np.searchsorted(edges, ks)
    rows = (3 * t[:, None] + np.arange(3)).reshape(-1)
    return capi.edge_group_rule(c.info[np.asarray(ks)], N[np.ix_(rows, rows)], e[t], w[t])


@pytest.mark.parametrize("name", ["tree_shapes", "contributions", "dcs_switches_closures_off", "angles_at_pi", "cluster_dcs",
                                  "closure_weight_1e10", "rows_scaled_1e6"])
def test_cases_against_the_reference(name):
    c = _case(name)
    with mc.environment(c.env), _open(c) as o:
        assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
        assert o.optimize(20)[0] == 20
        S = lr.Edges(o.get_poses(), c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
        groups, edges = _listed(S)
        T, ref = _reference(S, edges, groups)
        M = _masks(groups, edges)
        chi = np.array([(1.5 if b % 2 == 0 else 0.5) * (r["d2"] if np.isfinite(r["d2"]) else 1.0) for b, r in enumerate(ref)])
        N, e, w = o.edge_joint(edges)
        nfail, d2, dof, piv, fail = o.edge_groups(M, chi)
        _, wd = o.edge_robust()
    assert np.array_equal(bits(N), bits(N.T.copy()))                          # exactly symmetric
    assert np.array_equal(dof, [r["dof"] for r in ref]) and nfail == int(fail.sum())
    assert np.array_equal(bits(w), bits(wd[edges]))                           # sgo_edge_robust's weights
    assert np.abs(e - T["e"]).max() <= 1e-9 * max(1.0, np.abs(T["e"]).max()) and np.abs(w - T["w"]).max() <= 1e-9
    if name in sr.ILL_CONDITIONED:
        assert np.isfinite(N).all() and np.isfinite(piv).all() and np.isfinite(d2[piv >= eg.MIN_PIVOT]).all()
        print(f"{name}: left out of the accuracy comparison (fp64 model above 1e-8 of the reference); N, pivot and the decided d2 finite")
        return
    rn = np.abs(N - T["N"]).max() / np.abs(T["N"]).max()
    use = np.array([r["pivot"] >= 10 * eg.MIN_PIVOT for r in ref])
    d2r, pr = np.array([r["d2"] for r in ref]), np.array([r["pivot"] for r in ref])
    rd = float((np.abs(d2[use] - d2r[use]) / d2r[use]).max())
    rp = float(np.abs(piv[use] - pr[use]).max())
    sizes = sorted(set(int(m.sum()) for m in M[use]))
    # the kernel against the rule on the device's own table
    same = 0
    worst = 0.0
    for b in np.flatnonzero(use):
        rc, rd2, rpiv, rdof = _rule_on_table(c, edges, groups[b], N, e, w)
        same += rd2 == d2[b] and rpiv == piv[b]
        worst = max(worst, abs(rd2 - d2[b]) / (eg.EPS * ref[b]["condK"] * rd2), abs(rpiv - piv[b]) / (eg.EPS * (1.0 + ref[b]["normN"])) * D2_BAR / PIVOT_BAR)
    print(f"{name}: {edges.size} edges, {int(use.sum())} of {len(groups)} groups compared (sizes {sizes}); N {rn:.2e} of max |N_ref|, d2 {rd:.2e} "
          f"relative, pivot {rp:.2e} absolute; kernel / rule: {same} of {int(use.sum())} bit for bit, worst {worst:.3g} of the unit (bar {2 * D2_BAR:g})")
    assert use.sum() >= 8 and rn <= BAR and rd <= BAR and rp <= BAR
    assert worst <= 2 * D2_BAR
    decided = piv >= eg.MIN_PIVOT
    assert np.isnan(d2[~decided]).all() and np.isfinite(d2[decided]).all() and not fail[~decided].any()
    assert np.array_equal(fail, decided & (d2 > chi))
    clear = use & (np.abs(d2r - chi) > 1e-3 * d2r)
    assert np.array_equal(fail[clear], (d2r > chi)[clear])


def test_bridges_are_nan_and_do_not_fail():
    c = mc.make("long_thin_chain")
    edges = np.array([10, 700, 701] + list(range(300, 340)), dtype=np.int32)
    lists = [[700], [10, 700, 701], list(range(300, 340)), []]
    M = _masks([np.array(k, dtype=np.int64) for k in lists], np.sort(edges))
    with mc.environment(c.env), _open(c) as o:
        assert o.optimize(20)[0] == 20
        o.edge_joint(np.sort(edges))
        nfail, d2, dof, piv, fail = o.edge_groups(M, np.zeros(4))
    print(f"bridge groups: pivots {piv[:3]}")
    assert np.isnan(d2[:3]).all() and (np.abs(piv[:3]) < 1e-6).all() and not fail.any() and nfail == 0
    assert d2[3] == 0.0 and piv[3] == 1.0 and np.array_equal(dof, [3, 9, 120, 0])


@functools.lru_cache(maxsize=None)
def _cluster_session():
    """the cluster graph at the poses a device context reaches: poses, Edges, the listed groups and edges; computed once, shared"""
    c = eg.cluster_graph()[0]
    with _open(c) as o:
        assert o.optimize(20)[0] == 20
        P = o.get_poses()
    S = lr.Edges(P, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
    groups, edges = _listed(S)
    P.setflags(write=False)
    return c, P, S, groups, edges


def test_the_motivating_cluster_fails_together():
    c, P, S, _, _ = _cluster_session()
    grp = np.array(eg.CLUSTER, dtype=np.int32)
    with _open(c) as o:
        o.set_poses(P)
        o.edge_joint(grp)
        M = np.vstack([np.ones((1, 4), dtype=np.uint8), np.eye(4, dtype=np.uint8)])
        nfail, d2, dof, piv, fail = o.edge_groups(M, np.r_[eg.CHI2_99_DOF12, np.full(4, eg.CHI2_99_DOF3)])
        _, loo, red, _, _ = o.edge_leave_one_out(grp, eg.CHI2_99_DOF3, eg.MIN_PIVOT)
        e2 = o.edge_chi2()[grp]
    print(f"raw e2 {np.round(e2, 2)}, singles {np.round(d2[1:], 2)} (leave-one-out {np.round(loo, 2)}), the group {d2[0]:.4g} at pivot {piv[0]:.3g}")
    assert (e2 < eg.CHI2_99_DOF3).all() and (d2[1:] < eg.CHI2_99_DOF3).sum() == 3
    assert fail[0] and d2[0] > eg.CHI2_99_DOF12 and abs(d2[0] - 33.3) < 0.1 and dof[0] == 12 and nfail == 2
    assert (np.abs(d2[1:] - loo) <= 2e-6 * loo).all()


def test_single_edge_groups_are_the_leave_one_out_test():
    c, P, S, _, _ = _cluster_session()
    edges = np.arange(200, 363, dtype=np.int32)                              # in-loop and tail odometry, every closure
    with _open(c) as o:
        o.set_poses(P)
        o.edge_joint(edges)
        _, d2, dof, piv, _ = o.edge_groups(np.eye(edges.size, dtype=np.uint8))
        _, loo, red, _, _ = o.edge_leave_one_out(edges, eg.CHI2_99_DOF3, eg.MIN_PIVOT)
    use = red >= 1e-2
    r = float((np.abs(d2[use] - loo[use]) / loo[use]).max())
    print(f"{int(use.sum())} of {edges.size} single-edge groups against sgo_edge_leave_one_out: {r:.2e} relative; bridges {int((red < 1e-6).sum())}")
    assert use.sum() >= 60 and r <= 2e-6 and (dof == 3).all()
    assert (piv[use] >= red[use] - 1e-6).all()                                # (the pivot bounds the redundancy from above)
    assert np.isnan(d2[red < 1e-6]).all()


def test_the_table_against_sgo_candidate_joint():
    """the listed edges offered as candidates with their own endpoints, measurements and informations: S - blockdiag(Omega^-1) = N"""
    c, P, S, groups, edges = _cluster_session()
    with _open(c) as o:
        o.set_poses(P)
        N, e, w = o.edge_joint(edges)
        Sj, ej = o.candidate_joint(c.ei[edges], c.ej[edges], c.meas[edges], c.info[edges])
    Oi = np.linalg.inv(npo.info_full(c.info[edges]))
    D = Sj.copy()
    for t in range(edges.size):
        D[3 * t:3 * t + 3, 3 * t:3 * t + 3] -= Oi[t]
    off = ~np.kron(np.eye(edges.size, dtype=bool), np.ones((3, 3), dtype=bool))
    r = np.abs(D - N).max() / np.abs(N).max()
    print(f"{edges.size} edges: S - blockdiag(Omega^-1) against N {r:.2e} of max |N|, off-diagonal blocks bit for bit: "
          f"{np.array_equal(bits(Sj[off]), bits(N[off]))}, e bit for bit: {np.array_equal(bits(e), bits(ej))}")
    assert r <= 1e-12 and np.abs(e - ej).max() <= 1e-14 * max(1.0, np.abs(e).max())


def test_a_group_does_not_depend_on_its_batch_and_two_calls_agree():
    """300 groups (more workgroups than compute units) of 0 .. 40 members: a group of 17 alone -- a launch with its own, smaller
    LDS -- has the bits it has as number 0, 150 and 299"""
    c, P, S, groups, edges = _cluster_session()
    n = edges.size
    rng = np.random.default_rng(4)
    M = np.zeros((300, n), dtype=np.uint8)
    for b, s in enumerate(np.r_[0, 40, rng.integers(0, 41, 298)]):
        M[b, rng.choice(n, size=int(s), replace=False)] = 1
    probe = np.zeros(n, dtype=np.uint8)
    probe[rng.choice(n, size=17, replace=False)] = 1
    M[[0, 150, 299]] = probe
    chi = np.full(300, 30.0)
    with _open(c) as o:
        o.set_poses(P)
        o.edge_joint(edges)
        A = o.edge_groups(M, chi)
        B = o.edge_groups(M, chi)
        one = o.edge_groups(probe[None, :], chi[:1])
        rev = o.edge_groups(M[::-1].copy(), chi)
    assert A[0] == B[0] and all(same_bits(a, b) for a, b in zip(A[1:], B[1:]))
    assert all(same_bits(a[::-1], r) for a, r in zip(A[1:], rev[1:]))
    for b in (0, 150, 299):
        assert all(np.asarray(a[b]).tobytes() == np.asarray(s[0]).tobytes() for a, s in zip(A[1:], one[1:]))
    assert np.array_equal(A[2], 3 * M.sum(1))
    print(f"300 groups: {int(np.isfinite(A[1]).sum())} decided, {A[0]} fail")


def test_the_table_is_a_snapshot_and_a_second_table():
    c, P, S, groups, edges = _cluster_session()
    M = _masks(groups, edges)
    cand = (c.ei[edges[:40]], c.ej[edges[:40]], c.meas[edges[:40]], c.info[edges[:40]])
    Mj = np.zeros((6, 40), dtype=np.uint8)
    for b in range(6):
        Mj[b, b:b + 5 * (b + 1)] = 1
    moved = P + np.random.default_rng(1).normal(0, 0.05, P.shape) * (~c.fixed)[:, None]
    with _open(c) as o:
        o.set_poses(P)
        o.candidate_joint(*cand)
        j0 = o.joint_subsets(Mj)[1]
        N0, _, _ = o.edge_joint(edges)                                        # (the candidates' table stays)
        j1 = o.joint_subsets(Mj)[1]
        g0 = o.edge_groups(M)
        o.candidate_joint(*cand)                                              # (... and so does the edges')
        g1 = o.edge_groups(M)
        o.set_poses(moved)
        assert o.optimize(2)[0] == 2
        g2 = o.edge_groups(M)
        with pytest.raises(capi.SgoError, match="rc=-2"):                     # a refused call keeps the table
            o.edge_joint(np.r_[edges[:3], edges[:1]])
        assert "twice" in o.last_error()
        g3 = o.edge_groups(M)
        j2 = o.joint_subsets(Mj)[1]
        N1, _, _ = o.edge_joint(edges)                                        # (a new table at the new poses is another one)
        g4 = o.edge_groups(M)
        assert capi.lib().sgo_edge_joint(o._h, 0, None, None, None, None) == 0                   # n == 0 drops it, and it alone
        with pytest.raises(capi.SgoError, match="rc=-2"):
            o.edge_groups(M)
        assert "no resident table" in o.last_error()
        j3 = o.joint_subsets(Mj)[1]
        o.edge_joint(edges)
        o.set_graph(*c.arrays())
        with pytest.raises(capi.SgoError, match="rc=-2"):
            o.edge_groups(M)
    for g in (g1, g2, g3):
        assert all(same_bits(a, b) for a, b in zip(g0[1:], g[1:]))
    assert same_bits(j0, j1) and same_bits(j0, j2) and same_bits(j0, j3)
    assert not np.array_equal(N0, N1) and not np.array_equal(g0[1], g4[1])


def test_a_member_with_zero_information_is_dropped():
    c, P, S, groups, edges = _cluster_session()
    ks = next(g for g in groups if len(g) == 5)
    t = np.searchsorted(edges, ks)
    with _open(c) as o:
        o.set_poses(P)
        o.set_edge_information([int(ks[2])], np.zeros((1, 6)))
        o.edge_joint(edges)
        M = np.zeros((2, edges.size), dtype=np.uint8)
        M[0, t] = 1
        M[1, np.delete(t, 2)] = 1
        _, d2, dof, piv, _ = o.edge_groups(M)
        one = np.zeros((1, edges.size), dtype=np.uint8)
        one[0, t[2]] = 1
        alone = o.edge_groups(one, [1.0])
    assert np.array_equal(dof, [12, 12]) and d2[0].tobytes() == d2[1].tobytes() and piv[0].tobytes() == piv[1].tobytes() and np.isfinite(d2[0])
    assert alone[0] == 0 and alone[1][0] == 0.0 and alone[2][0] == 0 and alone[3][0] == 1.0


@pytest.mark.parametrize("shape,path", [(DIRECT, "direct_ldlt"), (MFRONT, "multifrontal_cholesky")], ids=["direct", "mfront"])
def test_a_later_optimize_has_the_bits_of_a_context_that_never_called(shape, path):
    g = graph(shape)
    closures = np.flatnonzero(np.abs(g.ei.astype(np.int64) - g.ej) != 1)[:64].astype(np.int32)
    n = closures.size                                                        # (600 / 620 has 21 closures)
    assert n >= 16
    M = np.zeros((8, n), dtype=np.uint8)
    for b in range(8):
        M[b, (2 * b + np.arange(6)) % n] = 1
    with capi.Optimizer(0) as opt, capi.Optimizer(0) as fresh:
        for o in (opt, fresh):
            o.set_graph(*g.arrays())
            assert o.solver_description().startswith(path)
        a = [opt.optimize(5)]
        opt.edge_joint(closures)
        _, d2, _, piv, _ = opt.edge_groups(M, np.full(8, 40.0))
        a.append(opt.optimize(5))
        b = [fresh.optimize(5), fresh.optimize(5)]
        assert same_bits(opt.get_poses(), fresh.get_poses())
        if shape == MFRONT:
            assert same_bits(opt.mfront_arrays(("X",))["X"], fresh.mfront_arrays(("X",))["X"])
    assert np.isfinite(piv).all() and np.isfinite(d2[piv >= eg.MIN_PIVOT]).all()
    for (d, st), (df, sf) in zip(a, b):
        assert d == df == 5 and st["chi2"] == sf["chi2"] and st["robust_chi2"] == sf["robust_chi2"]


def test_the_table_builds_on_a_direct_rows_0_context():
    c, P, S, groups, edges = _cluster_session()
    T = eg.table(S, edges)
    with _open(c, direct_rows=0) as o:
        o.set_poses(P)
        desc = o.solver_description()
        N, e, w = o.edge_joint(edges)
        _, d2, _, piv, _ = o.edge_groups(_masks(groups, edges))
        assert o.solver_description() == desc and o.optimize(2)[0] == 2
    rn = np.abs(N - T["N"]).max() / np.abs(T["N"]).max()
    print(f"direct_rows = 0 ({desc.split(':')[0]}): N {rn:.2e} of max |N_ref|, {int((piv >= eg.MIN_PIVOT).sum())} of {len(groups)} groups decided")
    assert rn <= BAR and np.array_equal(bits(N), bits(N.T.copy()))


def test_refusals_leave_the_outputs_and_the_device_untouched():
    c, P, S, groups, edges = _cluster_session()
    L = capi.lib()
    ip, dp = capi._ip, capi._dp
    n = 4
    ok = edges[:n].copy()
    Nv, ev, wv = np.full(9 * 257 * 257, SENTINEL), np.full(3 * 257, SENTINEL), np.full(257, SENTINEL)
    d2, dof, piv, fl = np.full(3, SENTINEL), np.full(3, -7, dtype=np.int32), np.full(3, SENTINEL), np.full(3, 7, dtype=np.uint8)
    M = np.zeros((3, edges.size), dtype=np.uint8)
    M[0, :3] = M[1, 2:9] = M[2, 5:45] = 1
    big = M.copy()
    big[1, 2:43] = 1                                                          # 41 members
    chi = np.full(3, 20.0)

    def joint(cnt, ids):
        return L.sgo_edge_joint(o._h, cnt, None if ids is None else ip(np.ascontiguousarray(ids, dtype=np.int32)), dp(Nv), dp(ev), dp(wv))

    def grp(nn=edges.size, B=3, m=M, ch=chi, mp=eg.MIN_PIVOT, out=d2):
        return L.sgo_edge_groups(o._h, nn, B, None if m is None else m.ctypes.data_as(u8p), None if ch is None else dp(ch), mp,
                                 None if out is None else dp(out), ip(dof), dp(piv), fl.ctypes.data_as(u8p))

    with _open(c) as o:
        o.set_poses(P)
        assert grp() == -2 and "no resident table" in o.last_error()
        o.edge_joint(edges)
        want = o.edge_groups(M, chi)
        for cnt, ids in [(-1, ok), (n, None), (257, np.arange(257)), (n, np.r_[ok[:3], c.ei.size]), (n, np.r_[-1, ok[:3]]), (n, np.r_[ok[:3], ok[1]])]:
            assert joint(cnt, ids) == -2 and "sgo_edge_joint" in o.last_error(), (cnt, ids)
        for kw in [dict(nn=edges.size - 1), dict(B=-1), dict(m=None), dict(out=None), dict(ch=np.array([20.0, np.inf, 20.0])),
                   dict(ch=np.array([np.nan, 20.0, 20.0])), dict(mp=0.0), dict(mp=-0.5), dict(mp=1.5), dict(mp=np.nan), dict(m=big)]:
            assert grp(**kw) == -2 and "sgo_edge_groups" in o.last_error(), kw
        assert "group 1" in o.last_error() and "41" in o.last_error()
        assert np.all(Nv == SENTINEL) and np.all(ev == SENTINEL) and np.all(wv == SENTINEL)
        assert np.all(d2 == SENTINEL) and np.all(dof == -7) and np.all(piv == SENTINEL) and np.all(fl == 7)
        assert same_bits(o.get_poses(), P)
        again = o.edge_groups(M, chi)                                         # the table is kept
        assert want[0] == again[0] and all(same_bits(a, b) for a, b in zip(want[1:], again[1:]))
        assert grp(B=0) == 0 and grp(mp=1.0) >= 0 and np.all(d2 != SENTINEL)  # min_pivot = 1 is allowed
    with capi.Optimizer(0) as o:
        assert joint(n, ok) == -4                                             # no graph
    with capi.Optimizer(0, direct_rows=0, solver=capi.SOLVER_PCG_BJ) as o:    # a multi-GPU context's emulation
        o.debug_set_shard(2, 0)
        o.set_graph(*c.arrays())
        assert joint(n, ok) == -2 and "multi-GPU" in o.last_error()
    assert np.all(Nv == SENTINEL)


def test_an_active_overlay_is_refused():
    from test_gpu_edge_gate import _grow, _overlay_session
    base, steps, gg = _overlay_session()[:3]
    Nv = np.full(9 * 16, SENTINEL)
    with capi.Optimizer(0, direct_rows=0) as o:
        _grow(o, base, steps, gg, 6)
        assert "incremental overlay" in o.solver_description()
        rc = capi.lib().sgo_edge_joint(o._h, 4, capi._ip(np.arange(4, dtype=np.int32)), capi._dp(Nv), None, None)
        assert rc == -2 and "overlay" in o.last_error() and np.all(Nv == SENTINEL)


def test_an_indefinite_hessian_fails_and_keeps_the_table_and_the_outputs():
    import test_gpu_mfront as tmf
    g = tmf.chain_graph(700, 150, seed=16)
    info = g.info.copy()
    info[:, [0, 3, 5]] *= -1.0
    ids = np.arange(700, 716, dtype=np.int32)
    Nv = np.full(9 * 16 * 16, SENTINEL)
    with capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(*g.arrays())
        o.edge_joint(ids)
        M = np.ones((1, 16), dtype=np.uint8)
        want = o.edge_groups(M)
        o.set_edge_information(np.arange(g.E), info)
        rc = capi.lib().sgo_edge_joint(o._h, 16, capi._ip(ids), capi._dp(Nv), None, None)
        assert rc == -2 and "not positive definite" in o.last_error(), (rc, o.last_error())
        assert np.all(Nv == SENTINEL)
        again = o.edge_groups(M)
    assert all(same_bits(a, b) for a, b in zip(want[1:], again[1:]))


# ------------------------------------------------------------------ the compat headers
@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    """replay_edge_groups, built with the g++ line test_gpu_fsolve.py uses"""
    libdir = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("replay_edge_groups") / "replay_edge_groups")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "replay_edge_groups.cpp"), "-L" + libdir, "-lsgo", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_the_calls_through_the_compat_headers(replay, tmp_path):
    """SparseOptimizer::sgoEdgeJoint / sgoEdgeGroups return the C-ABI calls' values for 16 groups of 8 closures at the same estimates,
    and -1 with one line on std::cerr each where they must refuse"""
    g = graph(DIRECT)
    gf, of = tmp_path / "g.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 10.0)
    env = dict(os.environ)
    for k in ("SGO_DIRECT_ROWS", "SGO_INCREMENTAL", "SGO_SOLVER"):
        env.pop(k, None)
    chi = 40.0
    res = subprocess.run([replay, str(gf), str(of), "8", repr(chi), repr(eg.MIN_PIVOT), "8"], env=env, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    lines = open(of).read().split("\n")
    assert int(lines[0]) == 8 and lines[1].startswith("direct_ldlt") and lines[2] == lines[1], lines[:3]
    P = np.array([[float(v) for v in ln.split()] for ln in lines[3:3 + g.V]])
    rest = [ln.split() for ln in lines[3 + g.V:] if ln]
    rows = np.array([int(r[2]) for r in rest if r[0] == "row"], dtype=np.int32)
    grp = [r for r in rest if r[0] == "group"]
    tail = {r[0]: int(r[1]) for r in rest if r[0] in ("nfail", "not_active", "stale", "levenberg", "refused", "bad_row")}
    n = rows.size
    assert n >= 8 and len(grp) == 16
    M = np.zeros((16, n), dtype=np.uint8)
    for b in range(16):
        M[b, (b + np.arange(8)) % n] = 1
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P)
        opt.edge_joint(rows)
        nfail, d2, _, piv, fail = opt.edge_groups(M, np.full(16, chi))
    # (equal values: the text carries 17 digits; a NaN's sign and payload do not survive it)
    assert np.array_equal(np.array([float(r[2]) for r in grp]), d2, equal_nan=True) and np.array_equal(np.array([float(r[3]) for r in grp]), piv)
    assert np.array_equal(np.array([int(r[4]) for r in grp], dtype=bool), fail) and tail["nfail"] == nfail
    assert all(tail[k] == -1 for k in ("not_active", "stale", "levenberg", "refused", "bad_row")), tail
    said = [ln for ln in res.stderr.split("\n") if "sgoEdgeJoint" in ln or "sgoEdgeGroups" in ln]
    assert len(said) == 7, res.stderr                                        # (stale and levenberg: both calls refuse)


def test_mixed_kernel_kinds():
    """test_gpu_robust_kernels._mixed's kinds (all nine on the closures, delta = 1.5) set before sgo_edge_joint / sgo_edge_groups: the
    table's weights are sgo_edge_robust's and the reference's (tests/robust_reference.py), N and the groups' d2 and pivot meet the bars
    of test_cases_against_the_reference with the reference fed information w Omega.  Groups of 1, 2, 5, 6 and 11 closures (no set of
    closures disconnects the graph; how far a group is from that is the reference pivot's to say)."""
    import robust_reference as rr
    from test_gpu_robust_kernels import _mixed
    g = graph(MFRONT)
    kind, delta = _mixed(g)
    cl = np.flatnonzero(g.phi >= 0)
    edges = cl[::4][:200].astype(np.int32)
    assert set(kind[edges]) == set(range(1, 10))
    rng = np.random.default_rng(SEED)
    groups = [np.sort(rng.choice(edges, size=k, replace=False)) for k in (1, 2, 5, 6, 11) for _ in range(8)]
    M = _masks(groups, edges)
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        o.set_robust_kernels(np.arange(g.E), kind, delta)
        assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
        assert o.optimize(20)[0] == 20
        S0 = lr.Edges(o.get_poses(), g.fixed, g.ei, g.ej, g.meas, g.info, np.full(g.E, -1.0))
        w = rr.rho_mixed(kind, S0.e2, delta)[1]
        S = lr.Edges(o.get_poses(), g.fixed, g.ei, g.ej, g.meas, g.info, w=w)
        T, ref = _reference(S, edges, groups)
        N, e, wt = o.edge_joint(edges)
        chi = np.array([(1.5 if b % 2 == 0 else 0.5) * (r["d2"] if np.isfinite(r["d2"]) else 1.0) for b, r in enumerate(ref)])
        nfail, d2, dof, piv, fail = o.edge_groups(M, chi)
        _, wd = o.edge_robust()
    assert np.array_equal(bits(wt), bits(wd[edges])) and np.abs(wt - T["w"]).max() <= 1e-9
    assert (T["w"] < 0.999).sum() >= 20 and np.array_equal(bits(N), bits(N.T.copy()))
    rn = np.abs(N - T["N"]).max() / np.abs(T["N"]).max()
    use = np.array([r["pivot"] >= 10 * eg.MIN_PIVOT for r in ref])
    d2r, pr = np.array([r["d2"] for r in ref]), np.array([r["pivot"] for r in ref])
    rd = float((np.abs(d2[use] - d2r[use]) / d2r[use]).max())
    rp = float(np.abs(piv[use] - pr[use]).max())
    print(f"mixed kinds: {edges.size} closures, {int(use.sum())} of {len(groups)} groups compared, {int((T['w'] < 0.999).sum())} weights below 0.999; "
          f"N {rn:.2e} of max |N_ref|, d2 {rd:.2e} relative, pivot {rp:.2e} absolute")
    assert use.sum() >= 8 and rn <= BAR and rd <= BAR and rp <= BAR
    assert np.array_equal(dof, [r["dof"] for r in ref]) and nfail == int(fail.sum())
    decided = piv >= eg.MIN_PIVOT
    assert np.isnan(d2[~decided]).all() and np.isfinite(d2[decided]).all() and np.array_equal(fail, decided & (d2 > chi))
    clear = use & (np.abs(d2r - chi) > 1e-3 * d2r)
    assert np.array_equal(fail[clear], (d2r > chi)[clear])
