"""Joint compatibility of candidate closure sets (sgo_candidate_joint, sgo_joint_subsets, sgo_joint_pairs; kernels k_fs_gram,
k_fs_joint_table and k_joint_subsets in sparse_gslam_amd/csrc/sgo_fsolve.hip, driver in sgo_fsolve.cpp).

References.  On the cases of tests/mfront_cases.py: the table from the long-double-refined columns and its long-double Cholesky
(tests/joint_reference.py; tests/test_joint_reference.py qualifies the cases on the CPU).  On the mid-size graphs and the graph the
analysis refuses: SuperLU columns of the oracle's robustified Hessian.

Bars.  S at selinv_reference.DEVICE_BAR = 1e-6 of max |S_ref|, d2 at 1e-6 relative; the three cases selinv_reference.ILL_CONDITIONED
lists by name are checked for finite entries instead.  Symmetry, batch independence, the table's lifetime, non-interference and the
compat replay are bit for bit.  Every test prints what it measured."""
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import fsolve_reference as fr
import joint_reference as jr
import marginals_reference as mref
import mfront_cases as mc
import selinv_reference as sr
import test_gpu_mfront as tmf
from oracle import np_oracle as npo
from sparse_gslam_amd import capi
from test_gpu_edge_gate import GATE, _case, _grow, _overlay_session, _same, _state
from test_gpu_fsolve import IDS, PATHS, PCG_SLOTS, _candidates, _refused
from test_gpu_robust_kernels import DIRECT, MFRONT
from test_shim_replay import _write_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = sr.DEVICE_BAR
u8p = capi.C.POINTER(capi.C.c_uint8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _u8(a):
    return a.ctypes.data_as(u8p)


def _oinv(info):
    return np.linalg.inv(npo.info_full(info))


@functools.lru_cache(maxsize=None)
def _mc(name, k=jr.K):
    """case, candidates, the reference's e, S (long-double-refined columns), the subset masks and their d2 (long-double Cholesky), the
    gate's reference P and d2, the refinement's last correction: computed once per case and shared, never modified"""
    c = mc.make(name)
    H = mref.hessian(c.poses, c.fixed, c.ei, c.ej, c.meas, c.info, c.phi)
    cand = fr.candidates(c, k)
    R, e = fr.rhs(c.poses, c.fixed, *cand[:3])
    Xr, last = fr.refined(H, R)
    Sr = jr.joint_table(R, Xr, e, cand[3])
    M = jr.masks(jr.subsets(min(k, jr.K)), k)
    d2r = jr.all_d2(Sr, e, M, long=True)
    Pg, d2g = fr.gate(R, Xr, e, cand[3])
    for a in (e, Sr, M, d2r, Pg, d2g):
        a.setflags(write=False)
    return c, cand, e, Sr, M, d2r, Pg, d2g, last


@pytest.mark.parametrize("name", mc.NAMES)
def test_every_case_of_the_stage_tests(name):
    c, (ci, cj, meas, info), er, Sr, M, d2r, Pg, d2g, last = _mc(name)
    k = jr.K
    chi = np.where(np.arange(M.shape[0]) % 2 == 0, 1.5, 0.5) * d2r
    with mc.environment(c.env), capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(*c.arrays())
        assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
        S, e = o.candidate_joint(ci, cj, meas, info)
        npass, d2, dof, ok = o.joint_subsets(M, chi)
        _, gd2, gP, _ = o.candidate_gate(ci, cj, meas, info, GATE)
    assert np.array_equal(_bits(S), _bits(S.T.copy()))                       # exactly symmetric
    assert np.array_equal(dof, 3 * M.sum(1)) and d2[0] == 0.0 and npass == int(ok.sum())
    both = np.flatnonzero(c.fixed[ci] & c.fixed[cj])
    Oi = _oinv(info)
    for t in both:                                                           # S_tt = Omega^-1, zero cross blocks
        blk = S[3 * t:3 * t + 3].copy()
        assert np.abs(blk[:, 3 * t:3 * t + 3] - Oi[t]).max() <= 1e-14 * np.abs(Oi[t]).max()
        blk[:, 3 * t:3 * t + 3] = 0.0
        assert not blk.any()
    assert np.abs(e - er).max() <= 1e-9 * max(1.0, np.abs(er).max())
    if name in sr.ILL_CONDITIONED:
        assert np.isfinite(S).all() and np.isfinite(d2).all() and (d2 >= 0).all()
        print(f"{name}: left out of the accuracy comparison (fp64 model above 1e-8 of the reference); S and d2 finite")
        return
    rs, rd = jr.table_ratio(S, Sr), jr.rel(d2, d2r)
    # against sgo_candidate_gate on the same context: the singletons' d2 and the diagonal blocks less Omega^-1
    rg = jr.rel(d2[1:1 + k], gd2)
    rp = max(float(np.abs(S[3 * t:3 * t + 3, 3 * t:3 * t + 3] - Oi[t] - gP[t]).max() / np.abs(Oi[t] + Pg[t]).max()) for t in range(k))
    print(f"{name}: S {rs:.2e} of max |S_ref|, d2 {rd:.2e} of the reference over {M.shape[0]} subsets (largest {int(M.sum(1).max())}); "
          f"singletons / sgo_candidate_gate {rg:.2e}, diagonal blocks / its cov_pred {rp:.2e}; reference's last correction {last:.1e}")
    assert last <= 1e-12
    assert rs <= BAR and rd <= BAR
    assert rg <= BAR and rp <= BAR
    assert jr.rel(gd2, d2g) <= BAR
    assert np.array_equal(ok, d2r <= chi)                                    # (chi2_max is 1.5 or 0.5 of the reference's d2)


def _superlu_reference(P1, g, cand):
    ci, cj, meas, info = cand[:4]
    H = mref.hessian(P1, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi)
    R, e = fr.rhs(P1, g.fixed, ci, cj, meas)
    lu = spla.splu(H.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    X = lu.solve(R)
    resid = float(np.abs(H @ X - R).max() / np.abs(R).max())
    return jr.joint_table(R, X, e, info), e, resid


def _five(k, seed=11):
    """five subsets of k candidates: 2, 5, 11, 17 and min(k, 40) of them"""
    rng = np.random.default_rng(seed)
    return jr.masks([np.sort(rng.choice(k, size=s, replace=False)) for s in (2, 5, 11, min(k, 17), min(k, 40))], k)


def test_more_than_one_chunk_of_candidates():
    """90 candidates: 85 in the first chunk of columns, 5 in the second; the cross blocks between the chunks against the reference"""
    c, (ci, cj, meas, info), er, Sr, M, d2r, _, _, last = _mc("tree_shapes", 90)
    with mc.environment(c.env), capi.Optimizer(0, direct_rows=1, profile=1) as o:
        o.set_graph(*c.arrays())
        o.profile_reset()
        S, e = o.candidate_joint(ci, cj, meas, info)
        prof = o.kernel_profile()
        _, d2, _, _ = o.joint_subsets(M)
    assert prof["k_fs_gram"]["launches"] == 2 and prof["k_fs_joint_table"]["launches"] == 1, prof
    cross = np.abs(S[:255, 255:] - Sr[:255, 255:]).max() / np.abs(Sr).max()
    rs, rd = jr.table_ratio(S, Sr), jr.rel(d2, d2r)
    print(f"two chunks: S {rs:.2e}, cross blocks between the chunks {cross:.2e} of max |S_ref| (largest of them "
          f"{np.abs(Sr[:255, 255:]).max() / np.abs(Sr).max():.2e}); d2 {rd:.2e}")
    assert last <= 1e-12 and np.abs(Sr[:255, 255:]).max() > 1e-3 * np.abs(Sr).max()       # (the cross blocks are not negligible)
    assert np.array_equal(_bits(S), _bits(S.T.copy()))
    assert cross <= BAR and rs <= BAR and rd <= BAR


@functools.lru_cache(maxsize=None)
def _mid(shape):
    g, _, P1, _, _ = _case(*shape)
    cand = _candidates(g, 64)
    return (g, P1, cand) + _superlu_reference(P1, g, cand)


@pytest.mark.parametrize("shape,opts,path", PATHS, ids=IDS)
def test_the_table_on_every_path(shape, opts, path):
    g, P1, (ci, cj, meas, info, _), Sr, er, resid = _mid(shape)
    assert resid <= 1e-9
    M = _five(64)
    d2r = jr.all_d2(Sr, er, M, long=True)
    with capi.Optimizer(0, profile=1, **opts) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P1)
        before = opt.solver_description()
        opt.profile_reset()
        S, e = opt.candidate_joint(ci, cj, meas, info)
        _, d2, dof, _ = opt.joint_subsets(M)
        prof = opt.kernel_profile()
        after = opt.solver_description()
    assert before == after and before.split(":")[0] == path, (before, after)
    assert prof["k_fs_forward"]["launches"] > 0 and not any(k in prof for k in PCG_SLOTS), sorted(prof)
    assert prof["k_fs_gram"]["launches"] == 1 and prof["k_fs_joint_table"]["launches"] == 1 and prof["k_joint_subsets"]["launches"] == 1
    assert "k_fs_gate" not in prof
    rs, rd = jr.table_ratio(S, Sr), jr.rel(d2, d2r)
    print(f"{path}: S {rs:.3e} of max |S_ref|, d2 of five subsets {rd:.3e}; reference residual {resid:.1e}")
    assert np.array_equal(_bits(S), _bits(S.T.copy())) and np.array_equal(dof, 3 * M.sum(1))
    assert rs <= BAR and rd <= BAR


def test_a_graph_the_analysis_refuses_goes_through_the_pcg():
    g, P1, cand = _refused()[:3]
    ci, cj, meas, info = cand[:4]
    Sr, er, resid = _superlu_reference(P1, g, cand)
    assert resid <= 1e-9
    M = _five(16)
    d2r = jr.all_d2(Sr, er, M, long=True)
    with capi.Optimizer(0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P1)
        desc = opt.solver_description()
        assert "multifrontal path not used: " in desc, desc
        opt.profile_reset()
        S, e = opt.candidate_joint(ci, cj, meas, info)
        _, d2, _, _ = opt.joint_subsets(M)
        prof = opt.kernel_profile()
        assert opt.solver_description() == desc
        assert opt.optimize(2)[0] == 2
    assert "k_fs_forward" not in prof and "k_fs_backward" not in prof and prof["k_fs_gram"]["launches"] == 1, sorted(prof)
    assert prof["k_update_p"]["launches"] > 0
    rs, rd = jr.table_ratio(S, Sr), jr.rel(d2, d2r)
    print(f"PCG route: S {rs:.3e} of max |S_ref|, d2 of five subsets {rd:.3e}")
    assert np.array_equal(_bits(S), _bits(S.T.copy()))
    assert rs <= BAR and rd <= BAR


def test_more_than_one_chunk_on_the_pcg_route():
    g, P1, _ = _refused()[:3]
    cand = _candidates(g, 90)
    ci, cj, meas, info = cand[:4]
    Sr, er, resid = _superlu_reference(P1, g, cand)
    assert resid <= 1e-9 and np.abs(Sr[:255, 255:]).max() > 1e-3 * np.abs(Sr).max()
    with capi.Optimizer(0, profile=1) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P1)
        opt.profile_reset()
        S, e = opt.candidate_joint(ci, cj, meas, info)
        prof = opt.kernel_profile()
    assert "k_fs_forward" not in prof and prof["k_fs_gram"]["launches"] == 2, sorted(prof)
    cross = np.abs(S[:255, 255:] - Sr[:255, 255:]).max() / np.abs(Sr).max()
    rs = jr.table_ratio(S, Sr)
    print(f"PCG route, two chunks: S {rs:.3e}, cross blocks between the chunks {cross:.3e} of max |S_ref|")
    assert np.array_equal(_bits(S), _bits(S.T.copy())) and cross <= BAR and rs <= BAR


def test_a_subset_does_not_depend_on_its_batch():
    """300 subsets of 0 .. 40 candidates (more workgroups than compute units): one of 17 alone -- a launch with its own, smaller LDS --
    has the bits it has as number 0, 150 and 299; two calls agree; the pairs are symmetric and equal sgo_joint_subsets' bits"""
    c, (ci, cj, meas, info), er, Sr, _, _, _, _, _ = _mc("tree_shapes")
    k = jr.K
    rng = np.random.default_rng(4)
    lists = [np.sort(rng.choice(k, size=int(s), replace=False)) for s in np.r_[0, 40, rng.integers(0, 41, 298)]]
    probe = np.sort(rng.choice(k, size=17, replace=False))
    for b in (0, 150, 299):
        lists[b] = probe
    lists[1], lists[2] = np.zeros(0, dtype=np.int64), np.arange(40)
    M = jr.masks(lists, k)
    iu = [(s, t) for t in range(k) for s in range(t + 1)]
    Mp = jr.masks([np.unique([s, t]) for s, t in iu], k)
    with mc.environment(c.env), capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(*c.arrays())
        S, _ = o.candidate_joint(ci, cj, meas, info)
        _, d2, dof, _ = o.joint_subsets(M)
        _, d2b, _, _ = o.joint_subsets(M)
        _, alone, _, _ = o.joint_subsets(M[:1])
        pairs = o.joint_pairs()
        _, dp, _, _ = o.joint_subsets(Mp)
    assert np.array_equal(_bits(d2), _bits(d2b))
    assert all(d2[b].tobytes() == alone[0].tobytes() for b in (0, 150, 299))
    assert d2[1] == 0.0 and np.array_equal(dof, 3 * M.sum(1))
    assert np.array_equal(_bits(pairs), _bits(pairs.T.copy()))
    assert np.array_equal(_bits(np.array([pairs[s, t] for s, t in iu])), _bits(dp))
    want = jr.all_d2(S, er, M, long=True)                                    # on the device's own table: the kernel's arithmetic alone
    rd = jr.rel(d2, want)
    print(f"300 subsets: d2 {rd:.2e} of a long-double Cholesky of the device's table; pairs: {len(iu)} subsets")
    assert rd <= 1e-9


def test_the_table_is_a_snapshot_until_the_graph_changes():
    c, (ci, cj, meas, info), _, _, M, _, _, _, _ = _mc("tree_shapes")
    L = capi.lib()
    moved = c.poses + np.random.default_rng(1).normal(0, 0.05, c.poses.shape) * (~c.fixed)[:, None]
    with mc.environment(c.env), capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(*c.arrays())
        S0, _ = o.candidate_joint(ci, cj, meas, info)
        d0 = o.joint_subsets(M)[1]
        o.set_poses(moved)
        assert o.optimize(2)[0] == 2
        d1 = o.joint_subsets(M)[1]
        with pytest.raises(capi.SgoError, match="rc=-2"):                    # a refused call keeps the table
            o.candidate_joint(ci[:2], ci[:2], meas[:2], info[:2])
        assert "itself" in o.last_error()
        d2 = o.joint_subsets(M)[1]
        p2 = o.joint_pairs()
        S1, _ = o.candidate_joint(ci, cj, meas, info)                        # (a new table at the new poses is another one)
        d3 = o.joint_subsets(M)[1]
        o.set_graph(*c.arrays())
        with pytest.raises(capi.SgoError, match="rc=-2"):
            o.joint_subsets(M)
        assert "no resident table" in o.last_error()
        with pytest.raises(capi.SgoError, match="rc=-2"):
            o.joint_pairs()
        o.candidate_joint(ci, cj, meas, info)
        d4 = o.joint_subsets(M)[1]
        assert L.sgo_candidate_joint(o._h, 0, None, None, None, None, None, None) == 0          # n == 0 drops it
        with pytest.raises(capi.SgoError, match="rc=-2"):
            o.joint_subsets(M)
    assert np.array_equal(_bits(d0), _bits(d1)) and np.array_equal(_bits(d0), _bits(d2)) and np.array_equal(_bits(d0), _bits(d4))
    assert p2.shape == (jr.K, jr.K) and np.array_equal(_bits(np.diag(p2)), _bits(d0[1:1 + jr.K]))
    assert not np.array_equal(S0, S1) and not np.array_equal(d0, d3)


@pytest.mark.parametrize("shape,opts,path", PATHS[:2], ids=IDS[:2])
def test_a_later_optimize_has_the_bits_of_a_context_that_never_called(shape, opts, path):
    g, P1, (ci, cj, meas, info, _) = _mid(shape)[:3]
    M = _five(64)
    with capi.Optimizer(0, **opts) as opt, capi.Optimizer(0, **opts) as fresh:
        for o in (opt, fresh):
            o.set_graph(*g.arrays())
            assert o.solver_description().startswith(path)
        a = [opt.optimize(3)]
        opt.candidate_joint(ci, cj, meas, info)
        opt.joint_subsets(M)
        opt.joint_pairs()
        a.append(opt.optimize(8))
        b = [fresh.optimize(3), fresh.optimize(8)]
        same_poses = np.array_equal(_bits(opt.get_poses()), _bits(fresh.get_poses()))
    for (d, st), (df, sf) in zip(a, b):
        assert d == df and st["chi2"] == sf["chi2"] and st["robust_chi2"] == sf["robust_chi2"]
    assert same_poses


def test_refusals_leave_the_device_and_the_outputs_untouched():
    g, P1, (ci, cj, meas, info, _) = _mid(MFRONT)[:3]
    V = g.V
    arr = (np.vstack([P1, P1[-1] + 1.0]), np.append(g.fixed, False)) + tuple(g.arrays()[2:])   # one extra vertex without any edge
    L = capi.lib()
    ip, dp = capi._ip, capi._dp
    a1, b1 = np.array([5], dtype=np.int32), np.array([900], dtype=np.int32)
    z1, w1 = meas[:1].copy(), info[:1].copy()
    Sv, ev = np.full(9, 7.0), np.full(3, 7.0)
    big = 257
    ab, bb = np.zeros(big, dtype=np.int32), np.arange(1, big + 1, dtype=np.int32)
    zb, wb = np.tile(z1, (big, 1)), np.tile(w1, (big, 1))
    Sb, eb = np.full(9 * big * big, 7.0), np.full(3 * big, 7.0)

    def joint(a=a1, b=b1, z=z1, w=w1, cnt=1, S=Sv, e=ev):
        return L.sgo_candidate_joint(opt._h, cnt, None if a is None else ip(a), None if b is None else ip(b), None if z is None else dp(z),
                                     None if w is None else dp(w), dp(S), dp(e))

    def bad(k, v):
        x = (z1 if k < 3 else w1).copy()
        x[0, k if k < 3 else k - 3] = v
        return x

    neg = w1.copy()
    neg[0, [0, 3, 5]] *= -1.0
    semi = np.array([[1.0, 1.0, 0.0, 1.0, 0.0, 1.0]])
    M = _five(64)
    d2v, dofv, okv = np.full(5, 7.0), np.full(5, 7, dtype=np.int32), np.full(5, 7, dtype=np.uint8)
    chi = np.full(5, GATE)
    pv = np.full(64 * 64, 7.0)

    def subsets(n=64, B=5, m=M, c=chi, d=d2v):
        return L.sgo_joint_subsets(opt._h, n, B, None if m is None else _u8(m), None if c is None else dp(c), None if d is None else dp(d),
                                   ip(dofv), _u8(okv))

    def untouched():
        return (np.all(Sv == 7.0) and np.all(ev == 7.0) and np.all(Sb == 7.0) and np.all(eb == 7.0) and np.all(d2v == 7.0) and np.all(dofv == 7)
                and np.all(okv == 7) and np.all(pv == 7.0))

    with capi.Optimizer(0) as opt:
        opt.set_graph(*arr)
        assert opt.solver_description().startswith("multifrontal_cholesky")
        # no table yet
        assert subsets() == -2 and "no resident table" in opt.last_error()
        assert L.sgo_joint_pairs(opt._h, 64, dp(pv)) == -2 and "no resident table" in opt.last_error()
        opt.candidate_joint(ci, cj, meas, info)
        keep = opt.joint_subsets(M)[1]
        s0 = _state(opt)
        tries = [("count", dict(cnt=-1)), ("ci", dict(a=None)), ("cj", dict(b=None)), ("meas", dict(z=None)), ("info", dict(w=None)),
                 ("nan meas", dict(z=bad(1, np.nan))), ("inf info", dict(w=bad(3, np.inf))), ("id low", dict(a=np.array([-1], dtype=np.int32))),
                 ("id high", dict(b=np.array([V + 1], dtype=np.int32))), ("no edge", dict(b=np.array([V], dtype=np.int32))),
                 ("self", dict(b=a1)), ("negative information", dict(w=neg)), ("semi-definite information", dict(w=semi)),
                 ("257 candidates", dict(a=ab, b=bb, z=zb, w=wb, cnt=big, S=Sb, e=eb))]
        for what, kw in tries:
            assert joint(**kw) == -2, what
            assert untouched(), what
            assert _same(_state(opt), s0), what
        assert "SGO_JOINT_MAX_CANDIDATES" in opt.last_error()
        assert joint(b=np.array([V], dtype=np.int32)) == -2 and "not active" in opt.last_error() and f"vertex {V}" in opt.last_error()
        assert joint(w=neg) == -2 and "positive definite" in opt.last_error() and "candidate 0" in opt.last_error()
        # the subsets' and the pairs' own refusals
        over = M.copy()
        over[3, :] = 0
        over[3, :41] = 1
        nanchi = chi.copy()
        nanchi[2] = np.nan
        for what, kw in [("wrong n", dict(n=63)), ("B < 0", dict(B=-1)), ("null subset", dict(m=None)), ("null d2", dict(d=None)),
                         ("nan chi2", dict(c=nanchi)), ("41 candidates", dict(m=over))]:
            assert subsets(**kw) == -2, what
            assert untouched(), what
        assert "subset 3" in opt.last_error() and "41" in opt.last_error()
        assert subsets(n=63) == -2 and "63" in opt.last_error() and "64" in opt.last_error()
        assert L.sgo_joint_pairs(opt._h, 63, dp(pv)) == -2 and L.sgo_joint_pairs(opt._h, 64, None) == -2 and untouched()
        assert subsets(B=0) == 0 and subsets(B=0, m=None, d=None) == 0 and untouched()
        # every refusal kept the table; optional outputs may be null
        assert np.array_equal(_bits(opt.joint_subsets(M)[1]), _bits(keep))
        assert L.sgo_joint_subsets(opt._h, 64, 5, _u8(M), None, dp(d2v), None, None) == 0 and np.array_equal(_bits(d2v), _bits(keep))
        assert L.sgo_candidate_joint(opt._h, 1, ip(a1), ip(b1), dp(z1), dp(w1), None, None) == 1
        d2v[:] = 7.0
    with capi.Optimizer(0) as opt:
        assert joint() == -4 and subsets() == -4 and L.sgo_joint_pairs(opt._h, 64, dp(pv)) == -4          # no graph
    # the rank emulation of a multi-GPU context
    with capi.Optimizer(0, direct_rows=0, solver=capi.SOLVER_PCG_BJ) as opt:
        opt.debug_set_shard(2, 0)
        opt.set_graph(*g.arrays())
        s0 = _state(opt)
        assert joint() == -2 and "multi-GPU" in opt.last_error()
        assert _same(_state(opt), s0)
    assert untouched()


def test_a_graph_without_a_free_pose():
    """every active vertex fixed: S = blockdiag(Omega^-1) and d2 = sum of e^T Omega e"""
    c = mc.make("root_own3_6")
    ci, cj, meas, info = fr.candidates(c, k=4)
    fixed = np.ones_like(c.fixed)
    e = npo.edge_error(c.poses[ci], c.poses[cj], meas)
    each = np.einsum("ti,tij,tj->t", e, npo.info_full(info), e)
    M = jr.masks([[0], [1, 3], [0, 1, 2, 3], []], 4)
    with capi.Optimizer(0) as opt:
        opt.set_graph(c.poses, fixed, *c.arrays()[2:])
        S, ed = opt.candidate_joint(ci, cj, meas, info)
        _, d2, dof, _ = opt.joint_subsets(M)
        pairs = opt.joint_pairs()
    Oi = _oinv(info)
    want = np.zeros((12, 12))
    for t in range(4):
        want[3 * t:3 * t + 3, 3 * t:3 * t + 3] = Oi[t]
    assert np.abs(S - want).max() <= 1e-14 * np.abs(want).max() and not S[want == 0].any()
    wd = M.astype(np.float64) @ each
    assert np.abs(d2 - wd).max() <= 1e-12 * wd.max() and d2[3] == 0.0 and list(dof) == [3, 6, 12, 0]
    assert np.abs(pairs[1, 3] - (each[1] + each[3])) <= 1e-12 * wd.max() and np.abs(np.diag(pairs) - each).max() <= 1e-12 * wd.max()


def test_an_active_overlay_is_refused():
    base, steps, g, arrs, V, fixed, ids = _overlay_session()
    with capi.Optimizer(0, direct_rows=0) as opt:
        _grow(opt, base, steps, g, 6)
        assert "incremental overlay" in opt.solver_description()
        e0, c0 = opt.edge_chi2().view(np.uint64), opt.chi2()
        with pytest.raises(capi.SgoError, match="rc=-2"):
            opt.candidate_joint([1], [5], np.zeros((1, 3)), np.array([[1.0, 0, 0, 1.0, 0, 1.0]]))
        assert "incremental overlay" in opt.last_error()
        assert np.array_equal(opt.edge_chi2().view(np.uint64), e0) and opt.chi2() == c0


def test_an_indefinite_hessian_fails_and_leaves_the_outputs():
    """the failure path of test_gpu_fsolve.py's indefinite graph; a table made before on the same context's good graph is dropped by
    the new graph, and the failed call leaves none"""
    g = tmf.chain_graph(700, 150, seed=16)
    info = g.info.copy()
    info[:, [0, 3, 5]] *= -1.0
    L = capi.lib()
    a1, b1 = np.array([5], dtype=np.int32), np.array([400], dtype=np.int32)
    z1, w1 = np.zeros((1, 3)), np.array([[400.0, 0, 0, 400.0, 0, 2500.0]])
    Sv, ev = np.full(9, 7.0), np.full(3, 7.0)
    d2v = np.full(1, 7.0)
    one = np.ones((1, 1), dtype=np.uint8)
    with capi.Optimizer(0, direct_rows=1) as o:
        o.set_graph(g.poses, g.fixed, g.ei, g.ej, g.meas, info, g.phi)
        assert o.solver_description().startswith("multifrontal_cholesky")
        assert L.sgo_candidate_joint(o._h, 1, capi._ip(a1), capi._ip(b1), capi._dp(z1), capi._dp(w1), capi._dp(Sv), capi._dp(ev)) == -2
        assert "not positive definite" in o.last_error()
        assert np.all(Sv == 7.0) and np.all(ev == 7.0)
        assert L.sgo_joint_subsets(o._h, 1, 1, _u8(one), None, capi._dp(d2v), None, None) == -2 and d2v[0] == 7.0
        rc, st = o.optimize(5)                           # as without the call: fails at iteration 0, the estimates stay
        assert rc == 0 and st["iters_done"] == 0 and np.array_equal(o.get_poses(), g.poses)
        o.set_graph(*g.arrays())
        S, e = o.candidate_joint(a1, b1, z1, w1)
        assert np.isfinite(S).all() and o.joint_subsets(one)[1][0] > 0
        assert o.optimize(2)[0] == 2


# ------------------------------------------------------------------ the compat headers
@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    """replay_candidate_joint, built with the g++ line test_gpu_fsolve.py uses"""
    libdir = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("replay_candidate_joint") / "replay_candidate_joint")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "replay_candidate_joint.cpp"), "-L" + libdir, "-lsgo", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_the_joint_test_through_the_compat_headers(replay, tmp_path):
    """SparseOptimizer::sgoCandidateJoint returns the C-ABI calls' bits for the same candidates and subsets at the same estimates, and
    -1 where sgoCandidateGate returns it, for an index outside the candidates and for a subset over the cap"""
    g = _case(*DIRECT)[0]
    k = 48
    ci, cj, meas, info, _ = _candidates(g, k)
    lists = jr.subsets(k)[-8:] + [np.array([3]), np.array([], dtype=np.int64)]
    M = jr.masks(lists, k)
    chi = np.linspace(5.0, 400.0, len(lists))
    gf, cf, sf, of = tmp_path / "g.txt", tmp_path / "c.txt", tmp_path / "s.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 1.0)
    with open(cf, "w") as f:
        for t in range(k):
            f.write(f"{ci[t]} {cj[t]} " + " ".join(repr(float(v)) for v in np.r_[meas[t], info[t]]) + "\n")
    with open(sf, "w") as f:
        for b, idx in enumerate(lists):
            f.write(" ".join([repr(float(chi[b])), str(len(idx))] + [str(int(t)) for t in idx[::-1]]) + "\n")      # (any order)
    env = dict(os.environ)
    for key in ("SGO_DIRECT_ROWS", "SGO_INCREMENTAL", "SGO_SOLVER"):
        env.pop(key, None)
    subprocess.check_call([replay, str(gf), str(cf), str(of), "8", str(sf)], env=env)
    lines = open(of).read().split("\n")
    assert int(lines[0]) == 8 and lines[1].startswith("direct_ldlt") and lines[2] == lines[1], lines[:3]
    P = np.array([[float(v) for v in ln.split()] for ln in lines[3:3 + g.V]])
    rows = [ln.split() for ln in lines[3 + g.V:] if ln and ln.split()[0] == "sub"]
    tail = dict(ln.split() for ln in lines[3 + g.V:] if ln and ln.split()[0] != "sub")
    assert len(rows) == len(lists)
    shim_d2 = np.array([float(r[2]) for r in rows])
    shim_ok = np.array([int(r[3]) for r in rows], dtype=bool)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P)
        opt.candidate_joint(ci, cj, meas, info)
        npass, d2, _, ok = opt.joint_subsets(M, chi)
    assert np.array_equal(_bits(shim_d2), _bits(d2)) and np.array_equal(shim_ok, ok) and int(tail["npass"]) == npass
    assert 0 < npass < len(lists)
    assert int(tail["nodecision"]) == 0
    assert all(int(tail[key]) == -1 for key in ("unknown_vertex", "bad_index", "oversize", "stale", "levenberg"))
