"""Every stage of one Gauss-Newton iteration of k_direct on the device against tests/direct_reference.py, on the cases of
tests/direct_cases.py: the smallest graphs that reach the dummy slot, the padded columns, zero to 60 separators (dense work items
from registers and, from 49 on, from dpl[]), multi-edge pairs in every orientation, the overflow lists, a column of 49 blocks,
loops past the prefetched item, the vector in LDS and in global memory either side of the threshold (XG), per-edge robust kernels
on both (KINDS, XG x KINDS) and blocks of wide scaling.

Per case: a DEBUG RUN (SGO_DIRECT_DEBUG when the graph is set), optimize(1), sgo_debug_direct_array's arrays; the declared shape
from the DEVICE's tables, those tables equal to the host plan's, then the stage checks; and a production run of the same case,
whose poses, history, ESCR, WD and WO must equal the debug run's bit for bit -- that ties the instantiation that dumps to the one
that ships.  Three cases also run optimize(2) and check its second iteration from the poses a separate optimize(1) left: it is
the first to need the clear of the separator triangle.  A failure prints every ratio of its case.

The UNTIL and BATCH instantiations get no dump: tests/test_gpu_optimize_until.py and tests/test_gpu_hypotheses.py hold them bit
for bit to the plain instantiation, and the plain instantiation is what this module pins."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import direct_cases as dc
import direct_reference as dr
from sparse_gslam_amd import capi

pytestmark = pytest.mark.gpu
SNAPSHOTS = ("A_WD", "A_WO", "A_SD", "A_XB", "F_SD", "F_XB", "D_SD", "D_PINV", "D_BS", "X")


@contextmanager
def debug_run(on):
    """SGO_DIRECT_DEBUG for the duration of a set-up."""
    old = os.environ.pop("SGO_DIRECT_DEBUG", None)
    try:
        if on:
            os.environ["SGO_DIRECT_DEBUG"] = "1"
        yield
    finally:
        os.environ.pop("SGO_DIRECT_DEBUG", None)
        if old is not None:
            os.environ["SGO_DIRECT_DEBUG"] = old


def run(c, iters, debug, P0=None, names=None):
    """(X as direct_reference.check takes it for the LAST iteration of optimize(iters), the call's stats) from the device."""
    arrs = list(c.arrays())
    if P0 is not None:
        arrs[0] = P0
    with capi.Optimizer(0) as o:
        with debug_run(debug):
            o.set_graph(*arrs)
        if c.kind is not None:
            o.set_robust_kernels(None, c.kind, c.delta)
        desc = o.solver_description()
        assert desc.startswith("direct_ldlt"), desc
        with pytest.raises(capi.SgoError, match="no sgo_optimize_gn has run"):
            o.direct_arrays(("X",))
        done, st = o.optimize(iters)
        assert done == iters, (done, o.last_error())
        X = o.direct_arrays(names)
        X["P1"] = o.get_poses()
    X["hist"] = (st["chi2"][iters - 1], st["robust_chi2"][iters - 1], st["chi2"][iters], st["robust_chi2"][iters])
    return X, st


def check_and_report(name, c, X, P0=None):
    case = c.as_dict() if P0 is None else dict(c.as_dict(), P0=P0)
    R = dr.check(case, X)
    print(dr.report(name, R))
    print("worst_by_stage", name, {k: float(f"{v:.4g}") for k, v in dr.worst_by_stage(R).items()})
    assert not dr.failures(R), dr.report(name, R)


@pytest.mark.parametrize("name", dc.NAMES)
def test_direct_stages(name):
    c = dc.make(name)
    plan = capi.direct_plan_arrays(c.fixed, c.ei, c.ej)
    X, st = run(c, 1, True)
    shape = dc.check_shape(c, X)
    assert shape and all(shape.values()), (name, shape)
    for k in capi.DIRECT_PLAN_ARRAYS:
        assert np.array_equal(X[k], plan[k]), (name, k)
    assert all(X[k].size == plan_size for k, plan_size in (("A_SD", int(plan["INFO"][6])), ("X", 3 * int(plan["INFO"][0])))), name
    check_and_report(name, c, X)
    # the production instantiation: no snapshot, everything else bit for bit
    Y, sp = run(c, 1, False, names=("ESCR", "ZSC", "WD", "WO") + SNAPSHOTS)
    assert all(Y[k].size == 0 for k in SNAPSHOTS), {k: Y[k].size for k in SNAPSHOTS}
    real = (X["SLOT_RC"][:, 0] >= 0) & (X["SLOT_RC"][:, 1] >= 0)
    multi = (X["EDGE_TGT"][:int(X["INFO"][4])] >> 30) == 3
    E = multi.size
    assert np.array_equal(Y["P1"], X["P1"]) and Y["hist"] == X["hist"] and np.array_equal(sp["chi2"], st["chi2"]), name
    assert np.array_equal(Y["ESCR"].reshape(27, E)[:18], X["ESCR"].reshape(27, E)[:18]), name
    assert np.array_equal(Y["ESCR"].reshape(27, E)[18:, multi], X["ESCR"].reshape(27, E)[18:, multi]), name
    assert np.array_equal(Y["ZSC"], X["ZSC"]) and np.array_equal(Y["WD"][:, :9], X["WD"][:, :9]), name
    assert np.array_equal(Y["WO"][real, :9], X["WO"][real, :9]), name


@pytest.mark.parametrize("name", dc.SECOND_ITERATION)
def test_second_iteration_stages(name):
    """optimize(2) in a debug run leaves its SECOND iteration's arrays; P0 of that iteration = what a separate optimize(1) leaves
    (tests/test_gpu_direct.py pins that continuation bit for bit).  The separator triangle of this iteration was cleared by the
    first one's pass after the back substitution: a stale entry fails the assembly's exact zeros or the forward stage."""
    c = dc.make(name)
    first, _ = run(c, 1, False, names=("INFO",))
    X, st = run(c, 2, True)
    assert int(X["INFO"][2]) >= 2
    check_and_report(name + " (second iteration)", c, X, P0=first["P1"])


def test_hook_refuses_a_graph_on_another_path():
    c = dc.make("seps_61")
    with capi.Optimizer(0) as o:
        o.set_graph(*c.arrays())
        desc = o.solver_description()
        assert not desc.startswith("direct_ldlt") and "direct path not used: " + c.refused in desc, desc
        o.optimize(1)
        with pytest.raises(capi.SgoError, match="not on the direct path"):
            o.direct_arrays(("X",))


def test_hook_refuses_an_unknown_array_and_a_closing_pass_alone():
    c = dc.make("one_closure")
    with capi.Optimizer(0) as o:
        o.set_graph(*c.arrays())
        o.optimize(0)                                   # (the closing chi2 pass alone: nothing to export)
        with pytest.raises(capi.SgoError, match="no sgo_optimize_gn has run"):
            o.direct_arrays(("WD",))
        o.optimize(1)
        assert o.direct_arrays(("WD",))["WD"].shape == (22, 10)
        rc = capi.lib().sgo_debug_direct_array(o._h, 99, None, 0)
        assert rc == -2 and "unknown array" in o.last_error(), (rc, o.last_error())
