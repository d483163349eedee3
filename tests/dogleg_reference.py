"""numpy reference of sgo_optimize_dogleg / sgo_optimize_dogleg_pcg (include/sgo.h): g2o 2020.5.29's
OptimizationAlgorithmDogleg::solve on the pose-graph oracle's own building blocks -- np_oracle.linearize, chi2, oplus and
solve_direct, imported and not copied; mixed kernels through lm_reference._system.  TEST INFRASTRUCTURE ONLY.

The schedule.  At iteration 0 of a call delta = delta_init (<= 0: 1e4), lambda = 1e-7, was_pd = True.  Per iteration, at the accepted
poses: H, b the robustified system; h_sd = alpha b with alpha = b.b / b.Hb; h_gn solves H h_gn = b (a solve that fails -- here: a
solution that is not finite; SuperLU knows no "not positive definite" -- sets was_pd = False and lambda *= 10, ends the call beyond
1e3 (STOP_DAMPING) and is repeated on H + lambda I; a success with was_pd False is followed by lambda = max(1e-12, lambda / 5)).
Trials until one is accepted or 100 have run: |h_gn| < delta: h = h_gn (GN); else |h_sd| > delta: h = (delta / |h_sd|) h_sd (SD);
else h = h_sd + beta (h_gn - h_sd) with d = h_gn - h_sd, c = h_sd.d, s2 = |h_sd|^2, D = sqrt(c^2 + |d|^2 (delta^2 - s2)),
beta = (-c + D) / |d|^2 if c <= 0 else (delta^2 - s2) / (c + D) (DL).  L = -h.Hh + 2 b.h (|L| < 1e-12: 1e-12);
rho = (cur - tmp) / L; accepted iff rho > 0 and tmp finite; rho > 0.75: delta = max(delta, 3 |h|); rho < 0.25: delta *= 0.5; a tmp or
rho that is not finite counts as rho = -inf.  100 rejected trials end the call (STOP_TRIALS; the iteration is counted).

dogleg() returns the per-iteration trace the C-ABI returns and one record per TRIAL: kind, delta (before the trial), cur, tmp, L,
rho, the norms of h_gn, h_sd and h, the six forms {b.b, b.g, g.g, b.Hb, b.Hg, g.Hg} the rules take, delta_after, accepted.  The
keyword arguments after `delta_init` are the schedule's constants; tests/test_dogleg_reference.py mutates each to show that the
comparisons notice."""
import math

import numpy as np
import scipy.sparse as sp

import lm_reference as lr
from oracle import np_oracle

STOP_MAX_ITERS, STOP_TRIALS, STOP_DAMPING = 0, 1, 2
STEP_GN, STEP_SD, STEP_DL = 0, 1, 2
KIND_LETTER = "GSD"
MAX_TRIALS = 100


def pattern(ref):
    """the trials as the issue's table writes them: one letter per trial (G = GN step, D = blend, S = scaled Cauchy), iterations
    separated by blanks"""
    out, t = [], 0
    for q in ref["trials"]:
        out.append("".join(KIND_LETTER[r["kind"]] for r in ref["records"][t:t + q]))
        t += q
    return " ".join(out)


def choose_step(h_gn, h_sd, rad, beta_by_sign=True):
    """the step of one trial from the two vectors and the trust region -> (kind, h)"""
    gn_norm, sd_norm = float(np.linalg.norm(h_gn)), float(np.linalg.norm(h_sd))
    if gn_norm < rad:
        return STEP_GN, h_gn
    if sd_norm > rad:
        return STEP_SD, (rad / sd_norm) * h_sd
    d = h_gn - h_sd
    c, d2, s2 = float(h_sd @ d), float(d @ d), float(h_sd @ h_sd)
    D = math.sqrt(c * c + d2 * (rad * rad - s2))
    beta = (-c + D) / d2 if (c <= 0 or not beta_by_sign) else (rad * rad - s2) / (c + D)
    return STEP_DL, h_sd + beta * d


def decide(cur, tmp, L, h_norm, rad, lo=0.25, hi=0.75, grow=3.0):
    """the decision of one trial -> (rho, accepted, the trust region after it)"""
    if abs(L) < 1e-12:
        L = 1e-12
    rho = (cur - tmp) / L
    if not (math.isfinite(tmp) and math.isfinite(rho)):
        rho = -math.inf
    if rho > hi:
        rad = max(rad, grow * h_norm)
    elif rho < lo:
        rad *= 0.5
    return rho, rho > 0, rad


def dogleg(poses, fixed, ei, ej, meas, info, phi, iters, delta_init=0.0, *, kind=None, delta=None, lo=0.25, hi=0.75, grow=3.0,
           beta_by_sign=True):
    """kind, delta: per-edge kinds and parameters as sgo_set_robust_kernels takes them (phi is then not read)."""
    poses = np.array(poses, dtype=np.float64, copy=True)
    out = dict(delta=[], trials=[], step_kind=[], records=[], stop_reason=STOP_MAX_ITERS, solves=0, lam=0.0)
    chi2_of, linearize_of = lr._system(kind, delta)
    plain, cur = chi2_of(poses, fixed, ei, ej, meas, info, phi)
    out["chi2"], out["robust_chi2"] = [plain], [cur]
    rad = delta_init if delta_init > 0 else 1e4
    out["delta0"] = rad
    lam, was_pd, done = 1e-7, True, 0
    for it in range(iters):
        H, b = linearize_of(poses, fixed, ei, ej, meas, info, phi)
        Hb = H @ b
        bb, bHb = float(b @ b), float(b @ Hb)
        alpha = bb / bHb
        h_sd = alpha * b
        while True:                                       # the one solve of the iteration, damped only after a failure
            Hs = H if was_pd else H + lam * sp.identity(H.shape[0], format="csc")
            if not was_pd:
                out["lam"] = lam
            h_gn = np_oracle.solve_direct(Hs, b)
            out["solves"] += 1
            solved = bool(np.all(np.isfinite(h_gn)))
            was_pd = was_pd and solved
            if solved:
                if not was_pd:
                    lam = max(1e-12, lam / 5.0)
                break
            lam *= 10.0
            if lam > 1e3:
                out["stop_reason"] = STOP_DAMPING
                break
        if out["stop_reason"] == STOP_DAMPING:
            break
        Hg = H @ h_gn
        forms = [bb, float(b @ h_gn), float(h_gn @ h_gn), bHb, float(b @ Hg), float(h_gn @ Hg)]
        gn_norm, sd_norm = float(np.linalg.norm(h_gn)), float(np.linalg.norm(h_sd))
        q, accepted, step = 0, False, -1
        while q < MAX_TRIALS and not accepted:
            step, h = choose_step(h_gn, h_sd, rad, beta_by_sign)
            L = float(-(h @ (H @ h)) + 2.0 * (b @ h))
            if abs(L) < 1e-12:
                L = 1e-12
            trial = np_oracle.oplus(poses, fixed, h)
            tmp_plain, tmp = chi2_of(trial, fixed, ei, ej, meas, info, phi)
            h_norm = float(np.linalg.norm(h))
            rec = dict(it=it, kind=step, delta=rad, cur=cur, tmp=tmp, L=L, gn_norm=gn_norm, sd_norm=sd_norm, h_norm=h_norm,
                       forms=list(forms))
            rho, accepted, rad = decide(cur, tmp, L, h_norm, rad, lo, hi, grow)
            rec.update(rho=rho, accepted=accepted, delta_after=rad)
            out["records"].append(rec)
            q += 1
            if accepted:
                cur, plain, poses = tmp, tmp_plain, trial
        done += 1
        out["delta"].append(rad)
        out["robust_chi2"].append(cur)
        out["chi2"].append(plain)
        out["trials"].append(q)
        out["step_kind"].append(step if accepted else -1)
        if not accepted:
            out["stop_reason"] = STOP_TRIALS
            break
    out["iters_done"] = done
    out["trials_total"] = sum(out["trials"])
    out["poses"] = poses
    return out
