"""The kernels of sgo_factor_solve and sgo_candidate_gate on the device against tests/fsolve_reference.check / check_gate, on the
cases of tests/mfront_cases.py -- the three selinv_reference.ILL_CONDITIONED lists included: the stage bounds carry no condition of H.

Per case: sgo_set_graph_se2 (the path must be the multifrontal one), optimize(1), the case's poses again; sgo_factor_solve with the
35 right-hand sides of tests/test_gpu_fsolve.py (two panels and a tail of 3) and ONE export of the factor it made and of the
panel after each pass; column 20 alone; then sgo_candidate_gate and the export of its last chunk.  Every test prints its ratios."""
import numpy as np
import pytest

import fsolve_reference as fr
import mfront_cases as mc
import test_fsolve_reference as tfr
from sparse_gslam_amd import capi

pytestmark = pytest.mark.gpu
EXPORT = ("INFO", "FRONTS", "BND", "PINV", "ELIM_VERTEX", "ARENA", "YINV", "FS_Y", "FS_X", "FLAGS")


@pytest.mark.parametrize("name", mc.NAMES)
def test_fsolve_stages(name):
    c, H, cand, _, _, B = tfr.inputs(name)
    n = H.shape[0] // 3
    Bd = np.ascontiguousarray(B.T).reshape(tfr.NRHS, n, 3)
    with mc.environment(c.env):
        plan = capi.mfront_plan_arrays(*c.arrays()[:4])
        with capi.Optimizer(0, direct_rows=1) as o:
            o.set_graph(*c.arrays())
            assert o.solver_description().startswith("multifrontal_cholesky"), o.solver_description()
            o.optimize(1)
            o.set_poses(c.poses)
            Xs = o.factor_solve(Bd)
            A = o.mfront_arrays(EXPORT)
            x20 = o.factor_solve(Bd[20])
            npass, d2, P, ok = o.candidate_gate(*cand, 11.345)
            G = o.mfront_arrays(("ELIM_VERTEX", "FS_X", "FLAGS"))
    for k in set(EXPORT) & set(capi.MFRONT_PLAN_ARRAYS):
        assert np.array_equal(A[k], plan[k]), (name, k)
    assert not A["FLAGS"][0] and not G["FLAGS"][0]
    R = fr.check(c.as_dict(), A, B, Xs, x20)
    R.update(fr.check_gate(c.as_dict(), G, cand, d2, P))
    print(fr.report(name, R))
    print("worst_by_stage", name, {k: float(f"{v:.4g}") for k, v in fr.worst_by_stage(R).items()})
    assert not fr.failures(R), fr.report(name, R)
    assert npass == int(ok.sum()) and np.array_equal(ok, d2 <= 11.345)
