"""The incremental overlay's kernels (k_ov_lin, k_ov_solve, k_ov_ax, k_ov_finish and the host's overlay_build) against the
stage-by-stage reference of tests/overlay_reference.py, on the case list of tests/overlay_cases.py: tile boundaries of the
elimination, empty sides, the wave boundaries of the right-hand sides, hubs, multi-block launches, accumulated updates and
the arithmetic edges.  Every case prints one JSON line of its worst error / (U abs) per stage before it asserts.
GPU-machine time of the whole file on the MI355X: 1.8 s for its 22 cases (0.3 s the first, 0.02 - 0.12 s the others)."""
import json

import numpy as np
import pytest

import amg_reference as ar
import overlay_cases as oc
import overlay_reference as ovr
from oracle import np_oracle as npo
from sparse_gslam_amd import capi

pytestmark = pytest.mark.gpu


def _vectors(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, 3)), rng.uniform(-1.0, 1.0, (n, 3)),
            rng.standard_normal((n, 3)) * 10.0 ** rng.choice([-6.0, 6.0], size=(n, 1))]


def _run(name):
    """The plan on the device: (plan, case, exported arrays + hook results, solver description)."""
    p = oc.plan(name)
    base = p.base
    hidx, free = npo.hessian_index(base.fixed)
    n = free.size
    with capi.Optimizer(0, direct_rows=0) as o:
        o.set_graph(*base.arrays())
        d, _ = o.optimize(4)
        assert d == 4, o.last_error()
        o.linearize()
        hpos = np.full(base.V, -1, dtype=np.int64)
        hpos[free] = ar._fetch(o, 0, "ROW_ORDER", np.int32)          # the internal row of every resident free pose
        with pytest.raises(capi.SgoError):                           # no overlay yet: the hooks refuse
            ovr.export_overlay(o, ["HDR"])
        P, E_res = o.get_poses(), base.E
        for q, u in enumerate(p.updates):
            last = q == len(p.updates) - 1
            P0 = oc.start_poses(p, P, u["V"])
            if last and p.late is not None:
                p.late(P0, u)
            V, fixed, ei, ej, meas, info, phi = oc.arrays_upto(p, q + 1)
            o.update_graph(P0, fixed, ei, ej, meas, info, phi, E_res)
            desc = o.solver_description()
            assert "incremental overlay" in desc, desc
            E_res = ei.size
            if not last:
                d, _ = o.optimize(4)
                assert d == 4, o.last_error()
                P = o.get_poses()
        case = oc.make_case(p, P0, hpos)
        xs = _vectors(n, 1)
        with pytest.raises(capi.SgoError):                           # the operator needs the linearisation
            ovr.overlay_apply(o, xs[0])
        b = ovr.overlay_linearize(o, n)
        X = ovr.export_overlay(o)
        X["b"] = b
        X["apply"] = [(x,) + ovr.overlay_apply(o, x) for x in xs]
        d, _ = o.optimize(1)
        assert d == 1, o.last_error()
        X2 = ovr.export_overlay(o, ["HDR", "Y", "WX", "XT"])
        # optimize(1) linearised at the same poses: the same values, bit for bit (fixed summation orders)
        assert np.array_equal(X2["Y"], X["Y"]) and np.array_equal(X2["WX"], X["WX"])
        X["XT"], X["P1"] = X2["XT"], o.get_poses()
    return p, case, X, desc


@pytest.mark.parametrize("name", list(oc.CASES))
def test_overlay_stages(name):
    p, case, X, desc = _run(name)
    hdr = dict(zip(("k", "nt", "ncol", "nnz", "nx"), (int(v) for v in X["HDR"])))
    R = ovr.check(case, X)
    w = ovr.worst_by_stage(R)
    comp = None
    if p.composed:
        tv = ovr.structure(case)["tv"]
        comp = ovr.composed(case, X["M"], X["b"], tv)
        w["composed"] = max(v[0] for v in comp.values())
    print(json.dumps(dict(case=name, hdr=hdr, **{k: float(f"{v:.4g}") for k, v in w.items()})))
    for key, want in p.expect.items():
        assert hdr[key] == want, (key, hdr, desc)
    assert f"({hdr['nx']} hubs), {hdr['nt']} touched rows" in desc, desc
    assert len(R) >= 12 or hdr["k"] == 0
    assert not ovr.failures(R), ovr.failures(R)
    if p.composed:
        assert w["composed"] <= ovr.K_OV, comp
