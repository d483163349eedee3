"""numpy reference of sgo_optimize_lm (include/sgo.h): g2o 2020.5.29's Levenberg-Marquardt schedule, as
oracle/np_lm_oracle.py::levenberg states it for the landmark graph, on the pose-graph oracle's own building blocks --
np_oracle.linearize, chi2, oplus and solve_direct, imported and not copied.  TEST INFRASTRUCTURE ONLY.

levenberg() returns the per-iteration trace the C-ABI returns and, beyond it, one record per TRIAL (lambda of the trial, cur, tmp,
scale, rho, accepted), which tests/test_gpu_lm.py needs for its input condition and its tolerances.  The three keyword arguments
after `lambda_init` are the schedule's constants; tests/test_lm_reference.py mutates each to show that the comparisons notice."""
import math

import numpy as np
import scipy.sparse as sp

import robust_reference as rr
from oracle import np_oracle

STOP_MAX_ITERS, STOP_TRIALS, STOP_ZERO_GAIN, STOP_LAMBDA = 0, 1, 2, 3
MAX_TRIALS = 10


def _system(kind, delta):
    """-> (chi2(poses, ...) -> plain, robust;  linearize(poses, ...) -> H, b) of the graph: np_oracle's own with phi, or -- with
    kinds (sgo_set_robust_kernels) -- through robust_reference's identity: chi2 = sum rho0, and the system is the unrobustified one
    with information w Omega.  The schedule does not know the difference."""
    if kind is None:
        return (lambda P, fixed, ei, ej, meas, info, phi: np_oracle.chi2(P, ei, ej, meas, info, phi)[:2],
                lambda P, fixed, ei, ej, meas, info, phi: np_oracle.linearize(P, fixed, ei, ej, meas, info, phi)[:2])
    kind = np.asarray(kind)

    def pairs(P, ei, ej, meas, info):
        plain, _, e2 = np_oracle.chi2(P, ei, ej, meas, info, np.full(len(ei), -1.0))
        r0, w = rr.rho_mixed(kind, e2, delta)
        return plain, float(r0.sum()), w

    def chi2(P, fixed, ei, ej, meas, info, phi):
        return pairs(P, ei, ej, meas, info)[:2]

    def linearize(P, fixed, ei, ej, meas, info, phi):
        w = pairs(P, ei, ej, meas, info)[2]
        return np_oracle.linearize(P, fixed, ei, ej, meas, np.asarray(info) * w[:, None], np.full(len(ei), -1.0))[:2]
    return chi2, linearize


def levenberg(poses, fixed, ei, ej, meas, info, phi, iters, lambda_init=0.0, *, kind=None, delta=None, upper=2.0 / 3.0, eps=1e-3,
              reset_nu=True):
    """kind, delta: per-edge kinds and parameters as sgo_set_robust_kernels takes them (phi is then not read)."""
    poses = np.array(poses, dtype=np.float64, copy=True)
    out = dict(lam=[], trials=[], records=[], stop_reason=STOP_MAX_ITERS, lambda0=None)
    chi2_of, linearize_of = _system(kind, delta)
    plain0, cur = chi2_of(poses, fixed, ei, ej, meas, info, phi)
    out["chi2"], out["robust_chi2"] = [plain0], [cur]
    lam, nu, ok, done = 0.0, 2.0, True, 0
    for it in range(iters):
        if not ok:
            break
        H, b = linearize_of(poses, fixed, ei, ej, meas, info, phi)
        if it == 0:
            lam = lambda_init if lambda_init > 0 else 1e-5 * float(np.max(np.abs(H.diagonal())))
            nu = 2.0
            out["lambda0"] = lam
        plain = out["chi2"][-1]
        rho, q = 0.0, 0
        while True:
            x = np_oracle.solve_direct(H + lam * sp.identity(H.shape[0], format="csc"), b)
            ok2 = bool(np.all(np.isfinite(x)))
            tmp, tmp_plain, scale, trial = float("inf"), float("inf"), eps, poses
            if ok2:
                trial = np_oracle.oplus(poses, fixed, x)
                tmp_plain, tmp = chi2_of(trial, fixed, ei, ej, meas, info, phi)
                scale += float(x @ (lam * x + b))
            rho = (cur - tmp) / scale
            accepted = rho > 0 and math.isfinite(tmp) and ok2
            out["records"].append(dict(it=it, lam=lam, cur=cur, tmp=tmp, scale=scale, rho=rho, accepted=accepted))
            if accepted:
                lam *= max(1.0 / 3.0, min(1.0 - (2 * rho - 1) ** 3, upper))
                if reset_nu:
                    nu = 2.0
                cur, plain, poses = tmp, tmp_plain, trial
            else:
                lam *= nu
                nu *= 2
                if not math.isfinite(lam):
                    q += 1
                    break
            q += 1
            if not (rho < 0 and q < MAX_TRIALS):
                break
        done += 1
        out["lam"].append(lam)
        out["robust_chi2"].append(cur)
        out["chi2"].append(plain)
        out["trials"].append(q)
        if q == MAX_TRIALS or rho == 0 or not math.isfinite(lam):
            ok = False
            out["stop_reason"] = STOP_TRIALS if q == MAX_TRIALS else (STOP_ZERO_GAIN if rho == 0 else STOP_LAMBDA)
    out["iters_done"] = done
    out["poses"] = poses
    return out


def perturbed(g, sigma, seed=1):
    """tests/test_gpu_lm.py's starts: poses 1 .. V - 1 perturbed with default_rng(seed) -- theta by N(0, sigma), then x and y."""
    rng = np.random.default_rng(seed)
    P = g.poses.copy()
    V = P.shape[0]
    P[1:, 2] += rng.normal(0.0, sigma, V - 1)
    P[1:, :2] += rng.normal(0.0, sigma, (V - 1, 2))
    return P
