// sgo_lm_pcg.cpp -- sgo_optimize_lm_pcg and sgo_lm_pcg_trace (include/sgo.h): g2o's Levenberg-Marquardt
// schedule with every trial's (H + lambda I) x = b solved by the context's PCG -- multigrid- or block-Jacobi-preconditioned --, so no
// graph is refused for its size or density.  sgo_lm.h has the chain of one attempt.  The call borrows the PCG machinery the way
// sgo_marginals does: ensure_amg (a context on a factorisation path builds its row plan and hierarchy on first use), the per-call
// fields of a solve at their defaults -- cold start, no soft cap, no progress probe, no lagged keep, tol_cap off, so start_pcg
// refreshes the hierarchy unconditionally --, and every solve at pcg_tol * tol_scale relative to its own right-hand side.
// Where the solve gets the shift: k_finalize<LM> writes S0.dblk, S0.dinv, the start vectors and the smoother's first sweep
// xs = omega Dinv b from dgb's diagonal + lambda; the level-0 passes of the preconditioner read their diagonal blocks from S0.dblk
// (the fp32 copy holds the off-diagonal blocks only, which the shift does not touch); amg_update re-forms P's smoothing, A P, P~ and
// the Galerkin products from level 0's blocks (BsrDev: a diagonal slot refers to S0.dblk) and its dinv, every coarse level's dinv
// from the products, and the dense inverse from the coarsest product.
// The decision stays on the device (k_lm_decide, rules::lm_trial); the host says only whether the solve succeeded -- it reads the
// PCG's scalars anyway -- and reads the state once per trial.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "sgo_ctx.h"
#include "sgo_lm.h"
#include "sgo_rules.h"

using namespace sgo;

namespace {

// what the call changes of the context's solve state beyond RestoreCall's fields, put back whatever happens
struct RestoreSolveState {
  sgo_ctx* c;
  double tol_cap;
  int pcg_pred;
  explicit RestoreSolveState(sgo_ctx* c_) : c(c_), tol_cap(c_->tol_cap), pcg_pred(c_->pcg_pred) {}
  ~RestoreSolveState() {
    c->tol_cap = tol_cap;
    c->pcg_pred = pcg_pred;
    // the level-0 diagonal and the coarse operators are those of H + lambda I of the last trial: as after sgo_set_poses
    c->linearized = false;
    c->hier.ref_valid = false;
  }
};

}  // namespace

extern "C" {

int sgo_optimize_lm_pcg(sgo_ctx* c, int32_t max_iters, double lambda_init, sgo_lm_stats* out) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if ((rc = lm_check_args(c, "sgo_optimize_lm_pcg", max_iters, lambda_init))) return rc;
    if (out) {
      std::memset(out, 0, sizeof(*out));
      out->iters_requested = max_iters;
    }
    if (c->n == 0) return SGO_ENOTHING;
    const double t0 = wall_s();
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_amg(c))) return rc;
    read_call_knobs(c);
    RestoreCall restore_call(c);
    RestoreSolveState restore_solve(c);
    c->call = sgo_ctx::CallState();
    c->hier.probe_k = 0;
    c->hier.probe_max = 0.0;
    c->tol_cap = 0.0;
    sgo_ctx::Lm& Z = c->lm;
    Z.pcg_iters.clear();
    Z.solve_stop.clear();
    const size_t V3 = 3 * (size_t)c->V;
    if ((rc = grow_device(c, &Z.d_trial, &Z.trial_cap, V3)) || (rc = grow_device(c, &Z.d_scratch, &Z.scratch_cap, kLmScratchDoubles)) ||
        (rc = grow_device(c, &Z.d_state, &Z.state_cap, (size_t)1)))
      return rc;
    double *chi0 = Z.d_scratch, *chi_trial = Z.d_scratch + 2, *partials = Z.d_scratch + 4;
    const int grid = lm_grid(c->n);
    LmState S;
    int attempt = 0;
    HIP_TRY(c, hipMemcpyAsync(Z.d_trial, c->d_poses, sizeof(double) * V3, hipMemcpyDeviceToDevice, c->stream));   // (the fixed poses' entries)
    if ((rc = lm_chi2(c, c->d_poses, chi0))) return rc;
    for (;;) {
      // H and b at the accepted poses again: a rejected trial leaves no rounding behind
      {
        Scope sc(c, K_LINEARIZE, 128.0 * c->S0.ncs + 72.0 * c->S0.nu + 72.0 * c->n);
        launch_linearize(c->stream, c->S0, 0, c->S0.ngrp, c->es, c->d_poses, c->d_dgb);
      }
      if (attempt == 0) {
        launch_lm_lambda0_rows(c->stream, c->n, c->d_dgb, partials);
        launch_lm_begin(c->stream, nullptr, partials, grid, chi0, lambda_init, max_iters, Z.d_state);
      }
      if (max_iters > 0) {
        int fgrid = 0;
        {
          Scope sc(c, K_FINALIZE, (72.0 + 48.0 + 48.0 + 6 * 24.0) * c->n);
          launch_finalize(c->stream, c->S0, 0, c->n, c->d_dgb, c->d_b, c->d_x, c->d_r, c->d_z, c->d_p, c->amg ? amg_xs0(c->amg) : nullptr,
                          c->amg ? amg_omega(c->amg) : 0.0, c->d_partials, &fgrid, &Z.d_state->lambda);
        }
        if ((rc = start_pcg(c, fgrid)) || (rc = run_pcg(c))) return rc;
        const PcgScalars P = *c->h_S;
        bool ok = P.stop == 1;
        int how = SGO_LM_SOLVE_CONVERGED;
        if (!ok) {
          double eta = 1.0;
          if ((rc = solve_at_floor(c, &ok, &eta))) return rc;
          how = ok ? SGO_LM_SOLVE_FLOOR : -P.stop;
        }
        Z.pcg_iters.push_back(P.iter);
        Z.solve_stop.push_back(how);
        launch_lm_trial_pcg(c->stream, c->n, c->d_free_id, Z.d_state, ok ? 1 : 0, c->d_poses, c->d_x, c->d_b, Z.d_trial, partials);
        if ((rc = lm_chi2(c, Z.d_trial, chi_trial))) return rc;
        launch_lm_decide(c->stream, nullptr, ok ? 1 : 0, partials, grid, chi_trial, attempt, max_iters, Z.d_state);
        launch_lm_commit(c->stream, Z.d_state, attempt, (int)V3, Z.d_trial, c->d_poses);
        ++attempt;
      }
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(&S, Z.d_state, sizeof(S), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      if (S.stop || S.it >= max_iters) break;
    }
    prof_flush(c);
    if (out) {
      out->iters_done = S.it;
      out->trials_total = S.trials_total;
      out->stop_reason = S.stop_reason;
      out->sync_rounds = attempt;
      out->lambda0 = S.lambda0;
      std::copy(S.h_lambda, S.h_lambda + S.it, out->lambda);
      std::copy(S.h_rob, S.h_rob + S.it + 1, out->robust_chi2);
      std::copy(S.h_plain, S.h_plain + S.it + 1, out->chi2);
      std::copy(S.h_trials, S.h_trials + S.it, out->trials);
      out->seconds_total = wall_s() - t0;
    }
    return S.it;
  } SGO_CATCH(c)
}

int sgo_lm_pcg_trace(sgo_ctx* c, int32_t cap, int32_t* pcg_iters, int32_t* solve_stop) {
  if (!c) return SGO_EINVAL;
  if (cap < 0) {
    c->err = "sgo_lm_pcg_trace: negative capacity";
    return SGO_EINVAL;
  }
  const sgo_ctx::Lm& Z = c->lm;
  const size_t k = std::min((size_t)cap, Z.pcg_iters.size());
  if (pcg_iters) std::copy(Z.pcg_iters.begin(), Z.pcg_iters.begin() + k, pcg_iters);
  if (solve_stop) std::copy(Z.solve_stop.begin(), Z.solve_stop.begin() + k, solve_stop);
  return (int)Z.pcg_iters.size();
}

}  // extern "C"
