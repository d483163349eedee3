"""BASELINE.json configs with random long-range closures on the HIP path: C4 with p_random = 0.05
("C4r", 100k poses / 1M edges) and C5 (1M poses / 10M edges, 5 % random closures), SURVEY.md
section 8(d).

A sparse direct factorisation of these graphs fills in catastrophically (expander-like closures), so
the reference values are the CPU oracle's own block-Jacobi PCG at 1e-10 ("PCG-vs-PCG"): at full size
for C4r (tests/golden/C4r_pcg.npz, scripts/make_golden_large.py, about 15 minutes of one core) and at
a size the oracle finishes for the C5 generator arguments (tests/golden/C5_50000_pcg.npz).  At C5's full
size the checks are the size-independent ones: every solve converged, the TRUE residual of a solve
(b - H x through sgo_hessian_apply, not the recurrence), first-order optimality |J^T rho| and the
robust objective both falling, and the exact-measurement graph returning to ground truth.

Tolerances: chi2 per GN iteration 1e-6 relative (BASELINE.json); poses 1e-4 m / rad (two fp64 solvers
on kappa(H) ~ 1e8 systems); true residual 1e-7 |b| for pcg_tol = 1e-8.
"""
import hashlib
import os

import numpy as np
import pytest

from sparse_gslam_amd import capi, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def graph_digest(g):
    h = hashlib.sha256()
    for a in g.arrays():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _check_against(f, g, st, P, done):
    assert str(f["digest"]) == graph_digest(g), "generator drift: the graph is not the one the fixture was made from"
    assert done == int(f["iters"])
    for k in range(done + 1):
        assert abs(st["chi2"][k] - f["chi2"][k]) <= 1e-6 * f["chi2"][k], (k, st["chi2"][k], f["chi2"][k])
        assert abs(st["robust_chi2"][k] - f["robust_chi2"][k]) <= 1e-6 * f["robust_chi2"][k], k
    assert np.abs(P[::50] - f["poses_stride50"]).max() <= 1e-4
    assert np.abs(P.sum(axis=0) - f["pose_sum"]).max() <= 1e-3 * max(1.0, np.abs(f["pose_sum"]).max())


def test_c4_random_closures_full_size_matches_pcg_oracle():
    """configs[3] variant p_random = 0.05 at full size against the oracle's PCG (PCG-vs-PCG)."""
    f = np.load(os.path.join(GOLDEN, "C4r_pcg.npz"))
    g = synth.config("C4r")
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        done, st = opt.optimize(20)
        P = opt.get_poses()
    assert set(st["pcg_converged"]) == {1}
    _check_against(f, g, st, P, done)


def test_c5_generator_reduced_size_matches_pcg_oracle():
    """configs[4]'s generator arguments (seed 5, 5 % random closures, 10 edges per pose) at 50k poses /
    500k edges, where the CPU oracle's PCG finishes: per-iteration chi2 and poses."""
    f = np.load(os.path.join(GOLDEN, "C5_50000_pcg.npz"))
    g = synth.config("C5", V=int(f["V"]), E=int(f["E"]))
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        done, st = opt.optimize(20)
        P = opt.get_poses()
    assert set(st["pcg_converged"]) == {1}
    _check_against(f, g, st, P, done)


def _true_relres(opt):
    b, _, _, _ = opt.linearize()
    x, it, relres = opt.solve()
    r = b - opt.hessian_apply(x)
    return float(np.linalg.norm(r) / np.linalg.norm(b)), float(np.linalg.norm(b)), it, relres


@pytest.mark.parametrize("name", ["C4r", "C5"])
def test_full_size_optimality_and_true_residual(name):
    """Size-independent checks at full size (C5: 1M poses / 10M edges on ONE GPU): every PCG solve
    converged; the true residual of a solve at the start and at the end; |J^T rho| (= |b|, the gradient
    of the robustified objective) and the robust chi2 fall over optimize(20); results are written to
    gpurun_out/ for profiles/."""
    g = synth.config(name)
    with capi.Optimizer(0) as opt:
        opt.set_graph(*g.arrays())
        rr0, g0, it0, _ = _true_relres(opt)
        done, st = opt.optimize(20)
        rr1, g1, it1, _ = _true_relres(opt)
        P = opt.get_poses()
    assert done == 20 and set(st["pcg_converged"]) == {1}, st["pcg_iters"]
    assert np.isfinite(P).all()
    assert rr0 <= 1e-7 and rr1 <= 1e-7, (rr0, rr1)
    assert st["robust_chi2"][-1] < st["robust_chi2"][0]
    assert g1 <= 0.2 * g0, (g0, g1)      # first-order optimality: GN + DCS converges linearly; the gradient norm fell >= 5x
    out = os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"large_config_{name}.txt"), "w") as fh:
        fh.write(f"{name}: V={g.V} E={g.E} done={done}\n"
                 f"true relres of a solve: start {rr0:.3e} ({it0} PCG its), end {rr1:.3e} ({it1} PCG its)\n"
                 f"|J^T rho|: {g0:.6e} -> {g1:.6e}\n"
                 f"robust chi2: {st['robust_chi2'][0]:.9e} -> {st['robust_chi2'][-1]:.9e}\n"
                 f"chi2: {st['chi2'][0]:.9e} -> {st['chi2'][-1]:.9e}\n"
                 f"pcg iterations: {st['pcg_iters']}\n"
                 f"GN iteration ms: {[round(1e3 * s, 1) for s in st['seconds']]}\nsetup s: {st['seconds_setup']:.2f}\n")


def test_c5_full_size_noise_free_graph_returns_to_truth():
    """C5's graph with exact measurements: chi2 = 0 at the ground truth and GN from a perturbed start
    returns there (solver independent), at 1M poses / 10M edges."""
    kw = dict(synth.CONFIGS["C5"])
    g = synth.manhattan(**kw, sigma_xy=0.0, sigma_th=0.0, init="truth")
    rng = np.random.default_rng(3)
    start = g.poses + rng.normal(0, 0.02, g.poses.shape)
    start[0] = g.poses[0]
    with capi.Optimizer(0) as opt:
        opt.set_graph(start, g.fixed, g.ei, g.ej, g.meas, g.info, g.phi)
        c0, _ = opt.chi2()
        done, st = opt.optimize(8)
        P = opt.get_poses()
    assert done == 8 and c0 > 1e4
    assert st["chi2"][-1] <= 1e-12 * c0
    assert np.abs(P[:, :2] - g.truth[:, :2]).max() <= 1e-6
