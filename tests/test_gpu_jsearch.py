"""Greedy joint-compatibility search on the device (sgo_joint_greedy, sgo_joint_extend; kernel k_joint_grow in
sparse_gslam_amd/csrc/sgo_jsearch.hip, driver in sgo_jsearch.cpp).

Cases (jsearch_reference.CASES): tree_shapes and child_own3_33 (40 and 22 poses, direct_rows=1) with 48 candidates, of which 0 and 1
have fixed endpoints; n = 1, 2, 65 (one past a wave); n = 256 (the cap, every thread live) on lattice_48.  Seeds: the empty one, every
singleton (B = n), one of 39 and one of 40 candidates; 300 seeds with repeats (more than one slice).  Thresholds: the 99 % quantile of
chi2 with 3 k degrees of freedom and a tight ladder, median singleton d2 times k.

Everything is compared on the S and e sgo_candidate_joint copied out, so only this kernel's error is judged.  Orders, counts and stops
equal the long-double reference's (tests/jsearch_reference.py) for every seed whose decisions all have a margin >= 1e-8: at least nine
seeds of ten per case and ladder (jsearch_reference.DEGENERATE lists the one combination that is a tie by construction).  d2_path and
d2_ext are held to the bar against the reference's recurrence on every compared seed, against a long-double from-scratch factorisation
(joint_reference.subset_d2_long) on the final set of every compared seed, every prefix of every sixth and the extensions of one
seed, and against sgo_joint_subsets on the masks of the final sets.  At the cap the reference runs on every eighth singleton (all 256
take half a minute on the CPU); the other seeds are compared against sgo_joint_subsets and sgo_joint_extend.

The bar: the worst relative error joint_reference.subset_d2 (LAPACK, fp64) shows against subset_d2_long over the final sets of the
reference's paths on all cases, times 16 (the pivot order is not the ascending one), rounded up to a power of two, never above
selinv_reference.DEVICE_BAR = 1e-6.  Measured: NOTES.md section 43.  The contracts are bit for bit.  Every test prints what it measured."""
import contextlib
import functools
import os
import subprocess

import numpy as np
import pytest

import joint_reference as jr
import jsearch_reference as js
import mfront_cases as mc
import selinv_reference as sr
from sparse_gslam_amd import capi
from test_gpu_edge_gate import _case, _same, _state
from test_gpu_fsolve import IDS, PATHS, _candidates
from test_gpu_robust_kernels import DIRECT
from test_shim_replay import _write_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(name, ladder) for name in js.CASES for ladder in ("q99", "tight")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return all(np.array_equal(x, y) if x.dtype.kind == "i" else np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _every(name):
    return 8 if name == "n256" else 1


@functools.lru_cache(maxsize=None)
def _bar():
    """(bar, LAPACK's worst error): over the final sets of the reference's paths from every fourth seed of every case and ladder"""
    worst = 0.0
    for name in js.CASES:
        _, _, S, e = js.table(name)
        n = e.shape[0]
        for chi in js.ladders(S, e).values():
            for seed in js.seeds(n, _every(name))[::4]:
                r = js.greedy(S, e, seed, chi)
                m = jr.masks([r.order[:r.count]], n)[0]
                worst = max(worst, jr.rel(jr.subset_d2(S, e, m), jr.subset_d2_long(S, e, m)))
    bar = min(2.0 ** np.ceil(np.log2(16.0 * worst)), sr.DEVICE_BAR)
    return float(bar), worst


@contextlib.contextmanager
def _open(name, **opts):
    """a context with the case's graph on the multifrontal path, inside the case's environment"""
    c = js.table(name)[0]
    with mc.environment(c.env), capi.Optimizer(0, direct_rows=1, **opts) as o:
        o.set_graph(*c.arrays())
        assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
        yield o


@pytest.mark.parametrize("name,ladder", COMBOS)
def test_search_against_the_reference(name, ladder):
    bar, lapack = _bar()
    with _open(name) as o:
        cand = js.table(name)[1]
        S, e = o.candidate_joint(*cand)
        n = e.shape[0]
        chi = js.ladders(S, e)[ladder]
        seeds = js.seeds(n)
        got = o.joint_greedy(seeds, chi)
        again = o.joint_greedy(seeds, chi)
        order, count, stop, path, ext = got
        finals = [order[b, :count[b]] for b in range(len(seeds))]
        xd2, xext = o.joint_extend(finals)
        _, sub, _, _ = o.joint_subsets(jr.masks(finals, n))
    assert _same_bits(got, again)                                            # two calls give the same bits
    last = path[np.arange(len(seeds)), count]
    assert np.array_equal(_bits(xd2), _bits(last)) and np.array_equal(_bits(xext), _bits(ext))      # sgo_joint_extend on the returned orders
    for b, f in enumerate(finals):
        assert list(f[:len(seeds[b])]) == list(seeds[b]) and (order[b, count[b]:] == -1).all() and len(set(f)) == len(f)
        assert path[b, 0] == 0.0 and np.isnan(path[b, count[b] + 1:]).all() and not np.isnan(path[b, :count[b] + 1]).any()
        assert all(ext[b, c].tobytes() == last[b].tobytes() for c in f)      # members hold d2_path[count] bit for bit
        free = np.setdiff1d(np.arange(n), f)
        if stop[b] == capi.JSTOP_NONE:
            assert count[b] < 40 and not (ext[b, free] <= chi[count[b] + 1]).any()
        else:
            assert stop[b] == capi.JSTOP_MAX_LEN and count[b] == 40
        assert (np.diff(path[b, :count[b] + 1]) >= 0).all() and (path[b, len(seeds[b]) + 1:count[b] + 1] <= chi[len(seeds[b]) + 1:count[b] + 1]).all()
    err_sub = jr.rel(last, sub)
    # the reference on the device's own table
    every = _every(name)
    picked = [b for b in range(len(seeds)) if len(seeds[b]) != 1 or seeds[b][0] % every == 0]
    qualify, worst, err_ref, err_long, nlong = 0, 1.0, 0.0, 0.0, 0
    for i, b in enumerate(picked):
        r = js.greedy(S, e, seeds[b], chi)
        worst = min(worst, r.margin)
        if r.margin < js.MARGIN:
            continue
        qualify += 1
        assert np.array_equal(order[b], r.order) and count[b] == r.count and stop[b] == r.stop, (seeds[b], order[b], r.order)
        assert np.array_equal(np.isnan(ext[b]), np.isnan(r.d2_ext))
        err_ref = max(err_ref, jr.rel(path[b, :r.count + 1], r.d2_path[:r.count + 1]), jr.rel(ext[b], r.d2_ext))
        for k in (range(1, r.count + 1) if i % 6 == 0 else (r.count,)):
            err_long = max(err_long, jr.rel(path[b, k], jr.subset_d2_long(S, e, jr.masks([r.order[:k]], n)[0])))
            nlong += 1
    err_ext = 0.0
    if n <= 65:                                                              # the extensions of the longest path that leaves some
        b = max((b for b in range(len(seeds)) if count[b] < min(n, 40)), key=lambda t: count[t], default=None)
        if b is not None:
            free = np.setdiff1d(np.arange(n), finals[b])
            want = [jr.subset_d2_long(S, e, jr.masks([list(finals[b]) + [c]], n)[0]) for c in free]
            err_ext = jr.rel(ext[b, free], want)
    print(f"{name} / {ladder}: bar {bar:.2e} (16 x LAPACK's {lapack:.2e}, rounded up); {qualify} of {len(picked)} compared seeds qualify (worst "
          f"margin {worst:.1e}); paths of {count.min()} to {count.max()} candidates over {len(seeds)} seeds; d2_path, d2_ext / the reference's "
          f"recurrence {err_ref:.2e}; d2_path / long-double from scratch over {nlong} sets {err_long:.2e}; d2_ext / from scratch {err_ext:.2e}; "
          f"final d2 / sgo_joint_subsets {err_sub:.2e}")
    if (name, ladder) in js.DEGENERATE:
        assert worst < js.MARGIN
    else:
        assert 10 * qualify >= 9 * len(picked)
    assert err_ref <= bar and err_long <= bar and err_ext <= bar and err_sub <= bar


def test_extend_on_lists_of_every_length():
    """sgo_joint_extend as a primitive: lists of 0 to 40 candidates in any order against a long-double from-scratch factorisation and
    sgo_joint_subsets; an extension value is the extended list's own d2"""
    bar, _ = _bar()
    with _open("tree_shapes") as o:
        S, e = o.candidate_joint(*js.table("tree_shapes")[1])
        n = e.shape[0]
        rng = np.random.default_rng(3)
        lists = [list(rng.permutation(n)[:k]) for k in (0, 1, 2, 10, 17, 39, 40)]
        d2, ext = o.joint_extend(lists)
        longer = [lists[3] + [c] for c in range(n) if c not in lists[3]]
        d2l, _ = o.joint_extend(longer)
        _, sub, _, _ = o.joint_subsets(jr.masks(lists, n))
    want = np.array([jr.subset_d2_long(S, e, jr.masks([ls], n)[0]) for ls in lists])
    free = [c for c in range(n) if c not in lists[3]]
    assert d2[0] == 0.0 and np.array_equal(_bits(ext[3, free]), _bits(d2l))  # the same pivots in the same order: the same bits
    for b, ls in enumerate(lists):
        assert all(ext[b, c].tobytes() == d2[b].tobytes() for c in ls)
    single = np.array([jr.subset_d2_long(S, e, jr.masks([[c]], n)[0]) for c in range(n)])
    errs = jr.rel(d2, want), jr.rel(d2, sub), jr.rel(ext[0], single)
    print(f"lists of 0 .. 40 candidates: d2 / long double {errs[0]:.2e}, / sgo_joint_subsets {errs[1]:.2e}; the empty list's extensions / "
          f"the singletons {errs[2]:.2e} (bar {bar:.2e})")
    assert max(errs) <= bar


def test_a_seed_does_not_depend_on_its_batch():
    """300 seeds (two slices of at most 256 slabs) with repeats: a seed's results are the same bits as number 0, 150, 256 and 299, alone
    in a call of its own, and with the batch in reverse order"""
    with _open("tree_shapes", profile=1) as o:
        S, e = o.candidate_joint(*js.table("tree_shapes")[1])
        n = e.shape[0]
        chi = js.ladders(S, e)["q99"]
        rng = np.random.default_rng(4)
        seeds = [list(rng.permutation(n)[:int(k)]) for k in rng.integers(0, 4, 300)]
        probe = [7, 30]
        for b in (0, 150, 256, 299):
            seeds[b] = probe
        allow = (rng.random((300, n)) < 0.9).astype(np.uint8)
        allow[[0, 150, 256, 299]] = allow[0]
        o.profile_reset()
        got = o.joint_greedy(seeds, chi, 40, allow)
        launches = o.kernel_profile()["k_joint_grow"]["launches"]
        o.profile_reset()
        alone = o.joint_greedy([probe], chi, 40, allow[:1])
        launches1 = o.kernel_profile()["k_joint_grow"]["launches"]
        back = o.joint_greedy(seeds[::-1], chi, 40, allow[::-1])
    assert launches == 2 and launches1 == 1
    for b in (0, 150, 256, 299):
        assert _same_bits([a[b] for a in got], [a[0] for a in alone]), b
    assert _same_bits(got, [a[::-1] for a in back])
    assert got[1][0] > 2 and len(set(got[1])) > 3                            # (the searches do grow, to different lengths)


def test_allow_and_max_len():
    with _open("tree_shapes") as o:
        S, e = o.candidate_joint(*js.table("tree_shapes")[1])
        n = e.shape[0]
        chi = js.ladders(S, e)["q99"]
        seeds = [[3], [3, 8], []]
        free = o.joint_greedy(seeds, chi)
        barred = np.ones((3, n), dtype=np.uint8)
        for b in range(3):
            barred[b, free[0][b, len(seeds[b])]] = 0                         # each search's first choice
        barred[1, :] = 0
        order, count, stop, path, ext = o.joint_greedy(seeds, chi, 40, barred)
        capped = o.joint_greedy(seeds, chi, 2)
        still = o.joint_greedy([[3, 8], [5, 1]], chi, 2)
        nogrow = o.joint_greedy(seeds, None)
    for b in (0, 2):
        first = free[0][b, len(seeds[b])]
        assert first not in order[b, :count[b]] and count[b] > len(seeds[b])
        r = js.greedy(S, e, seeds[b], chi, 40, barred[b])
        assert r.margin < js.MARGIN or (np.array_equal(order[b], r.order) and stop[b] == r.stop)
    assert count[1] == 2 and stop[1] == capi.JSTOP_NONE and list(order[1, :3]) == [3, 8, -1]          # an all-zero row: no growth
    assert np.array_equal(_bits(ext[1]), _bits(nogrow[4][1]))                # ... and the list's own extension values
    for b in range(3):                                                       # a shorter search is a prefix of the longer one, bit for bit
        assert capped[1][b] == min(free[1][b], 2) and (capped[2][b] == capi.JSTOP_MAX_LEN) == (capped[1][b] == 2)
        assert np.array_equal(capped[0][b, :2], free[0][b, :2]) and np.array_equal(_bits(capped[3][b, :3]), _bits(free[3][b, :3]))
    assert list(still[1]) == [2, 2] and list(still[2]) == [capi.JSTOP_MAX_LEN] * 2                    # max_len = seed length
    assert list(nogrow[1]) == [1, 2, 0] and list(nogrow[2]) == [capi.JSTOP_NONE] * 3


def test_an_exact_tie_goes_to_the_lower_index():
    """candidates 3 and 7 are the same candidate listed twice"""
    c, (ci, cj, meas, info), _, _ = js.table("tree_shapes")
    ci, cj, meas, info = ci.copy(), cj.copy(), meas.copy(), info.copy()
    ci[7], cj[7], meas[7], info[7] = ci[3], cj[3], meas[3], info[3]
    with _open("tree_shapes") as o:
        S, e = o.candidate_joint(ci, cj, meas, info)
        n = e.shape[0]
        chi = js.ladders(S, e)["q99"]
        allow = np.zeros((2, n), dtype=np.uint8)
        allow[:, [3, 7]] = 1
        order, count, stop, path, ext = o.joint_greedy([[], [20, 30]], chi, 40, allow)
    identical = np.array_equal(_bits(S[9:12]), _bits(S[21:24])) and np.array_equal(_bits(e[3]), _bits(e[7]))
    print(f"the duplicated candidate's rows of the device's table are {'the same bits' if identical else 'NOT the same bits'}")
    want = [js.greedy(S, e, s, chi, 40, allow[0]).order[len(s)] for s in ([], [20, 30])]
    assert order[0, 0] == want[0] and order[1, 2] == want[1]
    if identical:
        assert order[0, 0] == 3 and order[1, 2] in (3, -1)                   # (-1: neither copy passes the threshold after 20 and 30)


def test_refusals_write_nothing_and_keep_the_table():
    L = capi.lib()
    ip, dp = capi._ip, capi._dp
    u8p = capi.C.POINTER(capi.C.c_uint8)
    with _open("tree_shapes") as o:
        n = 48
        seed = js.lists([[4, 9], [2]])
        out = dict(order=np.full((2, 40), 7, dtype=np.int32), count=np.full(2, 7, dtype=np.int32), stop=np.full(2, 7, dtype=np.int32),
                   path=np.full((2, 41), 7.0), ext=np.full((2, n), 7.0), d2=np.full(2, 7.0))
        chi = np.concatenate([[0.0], np.linspace(10.0, 400.0, 40)])
        allow = np.ones((2, n), dtype=np.uint8)

        def greedy(n_=n, B=2, s=seed, c=chi, max_len=40, order=out["order"], count=out["count"]):
            return L.sgo_joint_greedy(o._h, n_, B, None if s is None else ip(s), allow.ctypes.data_as(u8p), None if c is None else dp(c), max_len,
                                      None if order is None else ip(order), None if count is None else ip(count), ip(out["stop"]), dp(out["path"]),
                                      dp(out["ext"]))

        def extend(n_=n, B=2, s=seed, d2=out["d2"], ext=out["ext"]):
            return L.sgo_joint_extend(o._h, n_, B, None if s is None else ip(s), None if d2 is None else dp(d2), None if ext is None else dp(ext))

        def untouched():
            return all(np.all(v == 7) for v in out.values())

        assert greedy() == -2 and "no resident table" in o.last_error() and extend() == -2 and untouched()
        S, e = o.candidate_joint(*js.table("tree_shapes")[1])
        M = jr.masks(jr.subsets(n), n)
        keep = o.joint_subsets(M)[1]
        s0 = _state(o)

        def row(*v):
            r = seed.copy()
            r[1, :len(v)] = v
            return r

        after = seed.copy()
        after[1, 5] = 11                                                     # an entry after a -1
        bad = chi.copy()
        bad[23] = np.nan
        tries = [("wrong n", dict(n_=47)), ("B < 0", dict(B=-1)), ("null seed", dict(s=None)), ("null order", dict(order=None)),
                 ("null count", dict(count=None)), ("entry high", dict(s=row(n))), ("entry low", dict(s=row(-2))), ("twice", dict(s=row(5, 6, 5))),
                 ("after a -1", dict(s=after)), ("max_len below the seed", dict(max_len=1)), ("max_len above the cap", dict(max_len=41)),
                 ("negative max_len", dict(max_len=-1)), ("nan chi2", dict(c=bad))]
        for what, kw in tries:
            assert greedy(**kw) == -2, what
            assert untouched() and _same(_state(o), s0), what
        assert "chi2_max[23]" in o.last_error()
        assert greedy(s=row(5, 6, 5)) == -2 and "candidate 5 twice" in o.last_error() and "list 1" in o.last_error()
        for what, kw in [("wrong n", dict(n_=49)), ("B < 0", dict(B=-1)), ("null lists", dict(s=None)), ("null d2", dict(d2=None)),
                         ("null d2_ext", dict(ext=None)), ("entry high", dict(s=row(n))), ("twice", dict(s=row(1, 1))), ("after a -1", dict(s=after))]:
            assert extend(**kw) == -2, what
            assert untouched() and _same(_state(o), s0), what
        assert greedy(B=0) == 0 and greedy(B=0, s=None, order=None, count=None) == 0 and extend(B=0, s=None, d2=None, ext=None) == 0 and untouched()
        assert np.array_equal(_bits(o.joint_subsets(M)[1]), _bits(keep))     # every refusal kept the table
        # optional outputs may be null; the return value is B
        assert L.sgo_joint_greedy(o._h, n, 2, ip(seed), None, dp(chi), 40, ip(out["order"]), ip(out["count"]), None, None, None) == 2
        assert extend() == 2 and list(out["order"][1, :1]) == [2] and out["count"].min() >= 1
        o.set_graph(*js.table("tree_shapes")[0].arrays())                    # a new graph drops the table
        assert greedy() == -2 and "no resident table" in o.last_error()
    with capi.Optimizer(0) as o:
        assert greedy() == -4 and extend() == -4                             # no graph


@pytest.mark.parametrize("shape,opts,path", PATHS[:2], ids=IDS[:2])
def test_the_search_touches_neither_a_later_optimize_nor_the_subsets(shape, opts, path):
    g = _case(*shape)[0]
    ci, cj, meas, info, _ = _candidates(g, 64)
    rng = np.random.default_rng(2)
    M = jr.masks([np.sort(rng.choice(64, size=s, replace=False)) for s in (2, 5, 11, 17, 40)], 64)
    chi = np.concatenate([[0.0], js.chi2_dist.ppf(0.99, 3 * np.arange(1, 41))])
    with capi.Optimizer(0, **opts) as opt, capi.Optimizer(0, **opts) as fresh:
        for o in (opt, fresh):
            o.set_graph(*g.arrays())
            assert o.solver_description().startswith(path)
        a = [opt.optimize(3)]
        opt.candidate_joint(ci, cj, meas, info)
        before = opt.joint_subsets(M)[1]
        order, count, _, _, _ = opt.joint_greedy([[t] for t in range(64)], chi)
        opt.joint_extend([order[b, :count[b]] for b in range(64)])
        after = opt.joint_subsets(M)[1]
        a.append(opt.optimize(8))
        b = [fresh.optimize(3), fresh.optimize(8)]
        same_poses = np.array_equal(_bits(opt.get_poses()), _bits(fresh.get_poses()))
    assert np.array_equal(_bits(before), _bits(after))
    for (d, st), (df, sf) in zip(a, b):
        assert d == df and st["chi2"] == sf["chi2"] and st["robust_chi2"] == sf["robust_chi2"]
    assert same_poses


# ------------------------------------------------------------------ the compat headers
@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    """replay_joint_search, built with the g++ line test_gpu_joint.py uses"""
    libdir = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("replay_joint_search") / "replay_joint_search")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "replay_joint_search.cpp"), "-L" + libdir, "-lsgo", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_the_search_through_the_compat_headers(replay, tmp_path):
    """SparseOptimizer::sgoJointGreedy and sgoJointExtend return the C-ABI calls' bits for the same candidates and seeds at the same
    estimates, and -1 where sgoCandidateJoint returns it, for a seed the call refuses and for a max_len below a seed's length"""
    g = _case(*DIRECT)[0]
    k = 48
    ci, cj, meas, info, _ = _candidates(g, k)
    seeds = [[], [3], [5, 1], [40, 2, 17]] + [[t] for t in range(8, 14)]
    chi = np.concatenate([[0.0], js.chi2_dist.ppf(0.99, 3 * np.arange(1, 41))])
    gf, cf, sf, of = tmp_path / "g.txt", tmp_path / "c.txt", tmp_path / "s.txt", tmp_path / "o.txt"
    _write_graph(gf, g, 1.0)
    with open(cf, "w") as f:
        for t in range(k):
            f.write(f"{ci[t]} {cj[t]} " + " ".join(repr(float(v)) for v in np.r_[meas[t], info[t]]) + "\n")
    with open(sf, "w") as f:
        f.write("12 " + " ".join(repr(float(v)) for v in chi) + "\n")
        for s in seeds:
            f.write(" ".join([str(len(s))] + [str(t) for t in s]) + "\n")
    env = dict(os.environ)
    for key in ("SGO_DIRECT_ROWS", "SGO_INCREMENTAL", "SGO_SOLVER"):
        env.pop(key, None)
    subprocess.check_call([replay, str(gf), str(cf), str(of), "8", str(sf)], env=env)
    lines = open(of).read().split("\n")
    assert int(lines[0]) == 8 and lines[1].startswith("direct_ldlt") and lines[2] == lines[1], lines[:3]
    P = np.array([[float(v) for v in ln.split()] for ln in lines[3:3 + g.V]])
    rest = [ln for ln in lines[3 + g.V:] if ln]
    paths = [ln.split(" | ") for ln in rest if ln.startswith("path ")]
    exts = [ln.split(" | ") for ln in rest if ln.startswith("ext ")]
    tail = dict(ln.split() for ln in rest if not ln.startswith(("path ", "ext ")))
    assert len(paths) == len(exts) == len(seeds)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        opt.set_poses(P)
        opt.candidate_joint(ci, cj, meas, info)
        order, count, stop, path, ext = opt.joint_greedy(seeds, chi, 12)
        d2, xext = opt.joint_extend([order[b, :count[b]] for b in range(len(seeds))])
    for b in range(len(seeds)):
        head = paths[b][0].split()
        assert int(head[2]) == stop[b] and int(head[3]) == count[b] and [int(t) for t in head[4:]] == list(order[b, :count[b]])
        assert np.array_equal(_bits([float(v) for v in paths[b][1].split()]), _bits(path[b, :count[b] + 1]))
        assert np.array_equal(_bits([float(v) for v in paths[b][2].split()]), _bits(ext[b]))
        assert np.array_equal(_bits([float(exts[b][0].split()[2])]), _bits(d2[b:b + 1]))
        assert np.array_equal(_bits([float(v) for v in exts[b][1].split()]), _bits(xext[b]))
    assert count.max() > 4 and int(tail["searches"]) == len(seeds) == int(tail["nogrowth"])
    assert all(int(tail[key]) == -1 for key in ("unknown_vertex", "bad_index", "twice", "short_max_len", "stale", "levenberg"))
