"""The overlay reference (tests/overlay_reference.py) on the CPU: it accepts its own fp64 forward model on every case of the
list (tests/overlay_cases.py), and rejects that model with one thing wrong -- each mutation at >= 10 C of the stage it belongs to."""
import json

import numpy as np
import pytest

import overlay_cases as oc
import overlay_reference as ovr

_CACHE = {}


def _vectors(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, 3)), rng.uniform(-1.0, 1.0, (n, 3)),
            rng.standard_normal((n, 3)) * 10.0 ** rng.choice([-6.0, 6.0], size=(n, 1))]


def _case(name):
    """(plan, case, vectors, step at the touched rows): made once per case and left unchanged"""
    if name not in _CACHE:
        p = oc.plan(name)
        case = oc.cpu_case(p)
        n = int((~p.base.fixed).sum())
        nt = ovr.structure(case)["nt"]
        _CACHE[name] = (p, case, _vectors(n, 1), np.random.default_rng(2).standard_normal(3 * nt) * 0.01)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(oc.CASES))
def test_reference_accepts_the_forward_model(name):
    p, case, xs, xt = _case(name)
    X = ovr.forward(case, xs=xs, xt=xt)
    for key, want in p.expect.items():
        assert int(X["HDR"][["k", "nt", "ncol", "nnz", "nx"].index(key)]) == want, (key, X["HDR"])
    R = ovr.check(case, X)
    w = ovr.worst_by_stage(R)
    if p.composed:
        c = ovr.composed(case, X["M"], X["b"], X["tv"])
        w["composed"] = max(v[0] for v in c.values())
    print(json.dumps(dict(case=name, hdr=[int(v) for v in X["HDR"]], **{k: round(v, 3) for k, v in w.items()})))
    assert not ovr.failures(R), ovr.failures(R)
    assert len(R) >= 12
    if p.composed:
        assert w["composed"] <= ovr.K_OV, c


MUTATIONS = [("side_swap", "structure", "hubs_1"), ("un_transposed", "lin", "tile_k9"), ("tile_skip", "pivot", "tile_k17"),
             ("back_short", "solve", "tile_k9"), ("nz_missing", "structure", "hubs_8"), ("no_sym", "schur", "hubs_8"),
             ("g_sign", "rhs", "tile_k7"), ("no_stx_w", "m", "hubs_8"), ("xn_no_hubs", "finish", "hubs_8"),
             ("dot_share", "dot", "wave_nk21_nx0"), ("mx_wrong_row", "operator", "tile_k8"), ("hub_earlier", "structure", "hubs_1")]


@pytest.mark.parametrize("mut,stage,name", MUTATIONS)
def test_reference_rejects_a_mutated_model(mut, stage, name):
    p, case, xs, xt = _case(name)
    X = ovr.forward(case, mut=mut, xs=xs, xt=xt)
    s = ovr.scaled(ovr.check(case, X))
    worst = max(v for k, v in s.items() if ovr.stage_of(k) == stage)
    assert worst >= 10.0, (mut, stage, {k: v for k, v in s.items() if v > 1.0})


def test_edge_terms_off_diagonal_block_is_the_oracle_s():
    """kernel_reference.edge_terms' A^T W B is np_oracle.linearize's off-diagonal block, its magnitude bounds it"""
    from oracle import np_oracle as npo
    p, case, _, _ = _case("hubs_1")
    t = ovr.edge_terms(case)
    ei, ej, meas, info, phi = case["app"]
    H, _, _, _ = npo.linearize(case["P0"], case["fixed"], ei, ej, meas, info, phi)
    hidx, _ = npo.hessian_index(case["fixed"])
    q = 0                                     # (the anchor edge: the only appended edge between its two poses)
    blk = H[3 * hidx[ei[q]]:3 * hidx[ei[q]] + 3, 3 * hidx[ej[q]]:3 * hidx[ej[q]] + 3].toarray()
    assert np.allclose(blk, t["Hij"][q], rtol=1e-13, atol=0)
    assert (np.abs(t["Hij"]) <= t["Hij_abs"] * (1 + 1e-12)).all()


def test_long_double_edge_algebra_is_np_oracle_s():
    """the composed check's long-double system of the appended edges against np_oracle.linearize (fp64 terms, fp64 sums)"""
    from oracle import np_oracle as npo
    for name in ("hubs_8", "full_information_phi10", "dcs_kink"):
        p, case, _, _ = _case(name)
        ei, ej, meas, info, phi = case["app"]
        H, b, _, _ = npo.linearize(case["P0"], case["fixed"], ei, ej, meas, info, phi)
        hidx, _ = npo.hessian_index(case["fixed"])
        av, tv, M = ovr.appended_system_ld(case)
        ix = (3 * hidx[np.r_[av, tv]][:, None] + np.arange(3)[None, :]).ravel()
        Hd = H[ix][:, ix].toarray()
        got = M.astype(np.float64)
        assert np.abs(got[:, :-1] - Hd).max() <= 1e-11 * np.abs(Hd).max()
        assert np.abs(got[:, -1] - b[ix]).max() <= 1e-11 * max(np.abs(b[ix]).max(), 1.0)
