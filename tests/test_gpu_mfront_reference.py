"""Every stage of one multifrontal Gauss-Newton iteration on the device against tests/mfront_reference.py, on the cases of
tests/mfront_cases.py: the smallest graphs that reach the panel tails, the merge's K bodies and tail, row m's places in a tile,
the prefetched and the streamed contributions, both branches of k_mf_solve (asserted from the front table: solve_fast_144 and
lattice_48 on the fast one, solve_generic_147 and lattice_50 on the generic one) and blocks of wide scaling.

Per case: sgo_set_graph_se2 (the path must be the multifrontal one), optimize(1), sgo_debug_mfront_array's arrays; the declared
shape from the DEVICE's front table, that table equal to the host plan's, then the stage checks.  A failure prints every ratio
of its case."""
import numpy as np
import pytest

import mfront_cases as mc
import mfront_reference as mr
from sparse_gslam_amd import capi

pytestmark = pytest.mark.gpu


def run_case(c):
    """X as mfront_reference.check takes it, from the device."""
    with mc.environment(c.env):
        plan = capi.mfront_plan_arrays(*c.arrays()[:4])
        with capi.Optimizer(0, direct_rows=1) as o:
            o.set_graph(*c.arrays())
            desc = o.solver_description()
            assert desc.startswith("multifrontal_cholesky"), desc
            with pytest.raises(capi.SgoError, match="no sgo_optimize_gn has run"):
                o.mfront_arrays(("X",))
            done, st = o.optimize(1)
            assert done == 1, (done, o.last_error())
            X = o.mfront_arrays()
            X["P1"] = o.get_poses()
    X["hist"] = (st["chi2"][0], st["robust_chi2"][0], st["chi2"][1], st["robust_chi2"][1])
    return plan, X


@pytest.mark.parametrize("name", mc.NAMES)
def test_mfront_stages(name):
    c = mc.make(name)
    plan, X = run_case(c)
    shape = mc.check_shape(c, X)
    assert shape and all(shape.values()), (name, shape)
    for k in capi.MFRONT_PLAN_ARRAYS:
        assert np.array_equal(X[k], plan[k]), (name, k)
    R = mr.check(c.as_dict(), X)
    print(mr.report(name, R))
    print("worst_by_stage", name, {k: float(f"{v:.4g}") for k, v in mr.worst_by_stage(R).items()})
    assert not mr.failures(R), mr.report(name, R)


def test_hook_refuses_a_graph_on_another_path():
    c = mc.make("root_own3_18")
    with capi.Optimizer(0) as o:                      # (without direct_rows=1 the single-launch path takes a graph this small)
        o.set_graph(*c.arrays())
        assert o.solver_description().startswith("direct_ldlt")
        o.optimize(1)
        with pytest.raises(capi.SgoError, match="not on the multifrontal path"):
            o.mfront_arrays(("X",))


@pytest.mark.parametrize("V,closures,seed", [(2, 0, 1), (3, 1, 2), (17, 2, 3), (64, 5, 4), (65, 0, 5), (300, 10, 6)])
def test_direct_step_meets_the_composed_bound(V, closures, seed):
    """k_direct's step from the poses alone (its stages, from sgo_debug_direct_array's export, and this residual with the kernel's
    own factor in the last term: tests/test_gpu_direct_reference.py): x = P1 (-) P0 after optimize(1), on test_gpu_direct.py's size ladder, held to the
    composed bound of the multifrontal reference -- |b - H x| <= C U (abs(b) + abs(H x) + |L| |L^T| |x|), C the composed stage's,
    L the dense Cholesky factor of np_oracle's H in hessian order (the reference's own: the kernel's factor is not exported) --
    plus U abs(H (|P1| + 2 pi on the angles)) for having read x through the rounded poses."""
    import kernel_reference as kr
    from oracle import np_oracle as npo
    from sparse_gslam_amd import synth
    g = synth.manhattan(V, V - 1 + closures, seed=seed, info_mode="full", init="odom", phi=10.0)
    with capi.Optimizer(0) as o:
        o.set_graph(*g.arrays())
        assert o.solver_description().startswith("direct_ldlt"), o.solver_description()
        done, _ = o.optimize(1)
        assert done == 1
        P1 = o.get_poses()
    hidx, free = npo.hessian_index(g.fixed)
    x = P1[free] - g.poses[free]
    x[:, 2] -= 2 * np.pi * np.round(x[:, 2] / (2 * np.pi))
    pa = np.abs(P1[free])
    pa[:, 2] += 2 * np.pi
    ref = kr.reference(g.poses, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi, xs=[x, pa])
    H = npo.linearize(*g.arrays())[0].toarray()
    La = np.abs(np.linalg.cholesky(H))
    llt = (La @ (La.T @ np.abs(x).ravel())).reshape(-1, 3)
    den = mr.C_STAGE["composed"] * (ref.b_abs + ref.hx_abs[0] + llt) + ref.hx_abs[1]
    r, at = mr.entry_ratio(ref.b - ref.hx[0], np.zeros_like(ref.b), den)
    print(f"direct V={V}: |b - H x| / (U bound) = {r:.3g} at {at}")
    assert r <= 1.0, (r, at)
