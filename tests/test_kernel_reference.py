"""The per-entry reference of the level-0 entry points (tests/kernel_reference.py) against both CPU oracles, and its
sensitivity: the checker accepts the C++ oracle's outputs and rejects each of a list of small, realistic mutations of them.
No GPU."""
import numpy as np
import pytest

import kernel_reference as kr
from oracle import c_oracle, np_oracle as npo
from sparse_gslam_amd import synth

CASES = {"C1_diag": ("C1", {}), "C1_full": ("C1", dict(info_mode="full")), "C2": ("C2", dict(info_mode="full")),
         "C2_odom": ("C2", dict(init="odom"))}


def _vectors(n):
    rng = np.random.default_rng(0)
    return [rng.standard_normal((n, 3)), rng.standard_normal((n, 3)) * 10.0 ** rng.choice([-6.0, 6.0], size=(n, 1))]


def _oracle(arr, xs):
    b, d, c2, rc2 = c_oracle.linearize(*arr)
    _, _, _, e2, _, _ = c_oracle.edges(arr[0][arr[2]], arr[0][arr[3]], arr[4], arr[5], arr[6])
    return dict(b=b, diag=d, chi2=c2, robust=rc2, e2=e2, hx=[c_oracle.hessian_apply(*arr, x).reshape(-1, 3) for x in xs])


def _diag_blocks(H, n):
    """The 3x3 diagonal blocks of a scipy H."""
    k = 3 * np.arange(n)[:, None, None]
    r = np.broadcast_to(k + np.arange(3)[:, None], (n, 3, 3)).ravel()
    c = np.broadcast_to(k + np.arange(3)[None, :], (n, 3, 3)).ravel()
    return np.asarray(H.tocsr()[r, c]).reshape(n, 3, 3)


@pytest.fixture(scope="module")
def c2():
    g = synth.config("C2", info_mode="full")
    arr = g.arrays()
    n = int((~g.fixed).sum())
    xs = _vectors(n)
    ref = kr.reference(*arr, xs=xs)
    return g, arr, xs, ref, _oracle(arr, xs)


def test_long_double_is_extended():
    assert np.finfo(np.longdouble).eps <= 1e-18


@pytest.mark.parametrize("case", list(CASES))
def test_reference_agrees_with_both_oracles_within_its_bounds(case):
    name, kw = CASES[case]
    g = synth.config(name, **kw)
    arr = g.arrays()
    n = int((~g.fixed).sum())
    xs = _vectors(n)
    ref = kr.reference(*arr, xs=xs)
    assert ref.free.size == n and np.array_equal(ref.free, np.flatnonzero(~g.fixed))
    o = _oracle(arr, xs)
    rc = kr.ratios(ref, b=o["b"], diag=o["diag"], chi2=o["chi2"], robust=o["robust"], e2=o["e2"], hx=o["hx"])
    assert not kr.failures(rc), ("c_oracle", rc)
    H, b, c2, rc2 = npo.linearize(*arr)
    _, _, e2 = npo.chi2(g.poses, g.ei, g.ej, g.meas, g.info, g.phi)
    rn = kr.ratios(ref, b=b.reshape(-1, 3), diag=_diag_blocks(H, n), chi2=c2, robust=rc2, e2=e2,
                   hx=[(H @ x.ravel()).reshape(-1, 3) for x in xs])
    assert not kr.failures(rn), ("np_oracle", rn)
    # the chunked accumulation is the one-pass accumulation
    small = kr.reference(*arr, xs=xs, chunk=97)
    assert kr.ratio(small.b, ref.b, ref.b_abs) <= 0.01 and kr.ratio(small.hx[1], ref.hx[1], ref.hx_abs[1]) <= 0.01


def _rejected(ref, **got):
    return kr.failures(kr.ratios(ref, **got))


def test_the_oracles_outputs_are_accepted(c2):
    g, arr, xs, ref, o = c2
    assert _rejected(ref, b=o["b"], diag=o["diag"], chi2=o["chi2"], robust=o["robust"], e2=o["e2"], hx=o["hx"]) == []


def _terms(g, k, xs=(), e=None):
    hidx, _ = npo.hessian_index(g.fixed)
    xf = []
    for x in xs:
        f = np.zeros((g.V, 3))
        f[hidx >= 0] = x
        xf.append(f)
    i, j = g.ei[k:k + 1], g.ej[k:k + 1]
    return kr.edge_terms(g.poses[i], g.poses[j], g.meas[k:k + 1], g.info[k:k + 1], g.phi[k:k + 1],
                         [f[i] for f in xf], [f[j] for f in xf], e=e), hidx[g.ei[k]], hidx[g.ej[k]]


def test_a_dropped_edge_of_small_contribution_is_rejected(c2):
    g, arr, xs, ref, o = c2
    fi = ~g.fixed[g.ei] & ~g.fixed[g.ej]
    t = kr.edge_terms(g.poses[g.ei], g.poses[g.ej], g.meas, g.info, g.phi)
    size = np.where(fi, np.abs(t["Hii"]).sum(axis=(1, 2)), np.inf)
    k = int(np.argmin(size))
    assert t["rho1"][k] < 1e-3         # a closure DCS has all but switched off
    keep = np.arange(g.E) != k
    sub = g.subset(keep).arrays()
    m = _oracle(sub, xs)
    bad = _rejected(ref, b=m["b"], diag=m["diag"], hx=m["hx"])
    assert {"b", "diag", "hx0", "hx1"} <= set(bad), bad


def test_an_untransposed_off_diagonal_block_is_rejected(c2):
    g, arr, xs, ref, o = c2
    fi = ~g.fixed[g.ei] & ~g.fixed[g.ej]
    t = kr.edge_terms(g.poses[g.ei], g.poses[g.ej], g.meas, g.info, g.phi)
    Hij = np.swapaxes(t["A"], 1, 2) @ t["W"] @ t["B"]
    asym = np.where(fi, np.abs(Hij - np.swapaxes(Hij, 1, 2)).max(axis=(1, 2)), -1)
    cand = np.flatnonzero(asym > 0)
    k = int(cand[np.argsort(asym[cand])[cand.size // 2]])      # a pair of median asymmetry
    hidx, _ = npo.hessian_index(g.fixed)
    i, j = hidx[g.ei[k]], hidx[g.ej[k]]
    hx = [y.copy() for y in o["hx"]]
    for y, x in zip(hx, xs):
        y[i] += (Hij[k].T - Hij[k]) @ x[j]      # row i reads its twin's block untransposed
    assert _rejected(ref, hx=hx) == ["hx0", "hx1"]


def test_blocks_rounded_to_fp32_are_rejected(c2):
    g, arr, xs, ref, o = c2
    H, _, _, _ = npo.linearize(*arr)
    H32 = H.copy()
    H32.data = H32.data.astype(np.float32).astype(np.float64)
    assert _rejected(ref, diag=o["diag"].astype(np.float32), hx=[(H32 @ x.ravel()).reshape(-1, 3) for x in xs]) == \
        ["diag", "hx0", "hx1"]
    # one block alone: a diagonal block, and the off-diagonal block of one pair in one row's product
    d = o["diag"].copy()
    d[1234] = d[1234].astype(np.float32)
    assert _rejected(ref, diag=d) == ["diag"]
    fi = ~g.fixed[g.ei] & ~g.fixed[g.ej]
    k = int(np.flatnonzero(fi)[4321])
    t, i, j = _terms(g, k)
    Hij = t["A"][0].T @ t["W"][0] @ t["B"][0]
    hx = [y.copy() for y in o["hx"]]
    for y, x in zip(hx, xs):
        y[i] += (Hij.astype(np.float32) - Hij) @ x[j]
    assert _rejected(ref, hx=hx) == ["hx0", "hx1"]


def test_a_dcs_weight_of_s_instead_of_s_squared_is_rejected(c2):
    g, arr, xs, ref, o = c2
    t = kr.edge_terms(g.poses[g.ei], g.poses[g.ej], g.meas, g.info, g.phi)
    fi = ~g.fixed[g.ei] & ~g.fixed[g.ej]
    k = int(np.flatnonzero(fi & (g.phi >= 0) & (t["rho1"] > 0.5) & (t["rho1"] < 0.9))[0])   # a mildly down-weighted closure
    tk, i, j = _terms(g, k, xs)
    f = 1.0 / np.sqrt(tk["rho1"][0]) - 1.0          # w = s instead of s^2: every W-linear term times 1/s
    b, d = o["b"].copy(), o["diag"].copy()
    b[i] += f * tk["bi"][0]
    b[j] += f * tk["bj"][0]
    d[i] += f * tk["Hii"][0]
    d[j] += f * tk["Hjj"][0]
    hx = [y.copy() for y in o["hx"]]
    for q, y in enumerate(hx):
        y[i] += f * tk["yi"][q][0]
        y[j] += f * tk["yj"][q][0]
    s = np.sqrt(tk["rho1"][0])
    robust = o["robust"] + (s - s * s) * float(tk["e2"][0])
    assert _rejected(ref, b=b, diag=d, hx=hx, robust=robust) == ["b", "diag", "robust_chi2", "hx0", "hx1"]


def test_an_edge_error_without_the_theta_wrap_is_rejected(c2):
    g, arr, xs, ref, o = c2
    e = npo.edge_error(g.poses[g.ei], g.poses[g.ej], g.meas)
    raw = g.poses[g.ej, 2] - g.poses[g.ei, 2] - g.meas[:, 2]
    fi = ~g.fixed[g.ei] & ~g.fixed[g.ej]
    k = int(np.flatnonzero(fi & (g.phi < 0) & (np.abs(raw - e[:, 2]) > np.pi))[0])   # an odometry edge across +-pi
    em = e[k:k + 1].copy()
    em[0, 2] = raw[k]
    t0, i, j = _terms(g, k)
    t1, _, _ = _terms(g, k, e=em)
    e2 = o["e2"].copy()
    e2[k] = float(t1["e2"][0])
    b = o["b"].copy()
    b[i] += t1["bi"][0] - t0["bi"][0]
    b[j] += t1["bj"][0] - t0["bj"][0]
    chi2 = o["chi2"] + float(t1["e2"][0] - t0["e2"][0])
    assert _rejected(ref, e2=e2, b=b, chi2=chi2) == ["b", "chi2", "edge_chi2"]


def test_two_rows_swapped_in_hessian_order_are_rejected(c2):
    g, arr, xs, ref, o = c2
    swap = np.arange(ref.free.size)
    swap[[700, 701]] = [701, 700]
    assert _rejected(ref, b=o["b"][swap], diag=o["diag"][swap], hx=[y[swap] for y in o["hx"]]) == ["b", "diag", "hx0", "hx1"]
