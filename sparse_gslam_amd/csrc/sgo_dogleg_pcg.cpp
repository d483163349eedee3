// sgo_dogleg_pcg.cpp -- sgo_optimize_dogleg_pcg (include/sgo.h): the dogleg schedule of sgo_dogleg.h with the one
// solve of an iteration done by the context's PCG, so no graph is refused for its size or density.  The call borrows the PCG
// machinery exactly as sgo_optimize_lm_pcg does (sgo_lm_pcg.cpp: ensure_amg, the per-call fields of a solve at their defaults, a
// hierarchy refreshed by start_pcg, a cold solve at pcg_tol * tol_scale relative to its own right-hand side, solve_ok = converged or
// at the floating-point floor) -- but once per ITERATION: k_finalize<LM> reads a damping word that is 0.0 until a solve has failed,
// and the trials that follow a rejection are light chains (k_dl_trial, chi2, k_dl_decide, k_lm_commit) on the vectors the solve left.
// The host reads the state once per solve, and once per group of kDlLightTrials re-trials while an iteration stays open.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "sgo_ctx.h"
#include "sgo_dogleg.h"
#include "sgo_rules.h"

using namespace sgo;

namespace {

// what the call changes of the context's solve state beyond RestoreCall's fields, put back whatever happens (as sgo_lm_pcg.cpp)
struct RestoreSolveState {
  sgo_ctx* c;
  double tol_cap;
  int pcg_pred;
  explicit RestoreSolveState(sgo_ctx* c_) : c(c_), tol_cap(c_->tol_cap), pcg_pred(c_->pcg_pred) {}
  ~RestoreSolveState() {
    c->tol_cap = tol_cap;
    c->pcg_pred = pcg_pred;
    // the level-0 diagonal and the coarse operators are those of the last solve: as after sgo_set_poses
    c->linearized = false;
    c->hier.ref_valid = false;
  }
};

}  // namespace

extern "C" {

int sgo_optimize_dogleg_pcg(sgo_ctx* c, int32_t max_iters, double delta_init, sgo_dogleg_stats* out) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if ((rc = lm_check_args(c, "sgo_optimize_dogleg_pcg", max_iters, delta_init, "delta_init"))) return rc;
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
    if ((rc = dl_buffers(c))) return rc;
    sgo_ctx::Dl& Y = c->dl;
    double* const trial = c->lm.d_trial;
    const size_t V3 = 3 * (size_t)c->V;
    double *bv = Y.d_vec, *gv = Y.d_vec + V3;
    double *chi0 = Y.d_scratch, *chi_trial = Y.d_scratch + 2, *vparts = Y.d_scratch + 4, *fparts = vparts + 3 * (size_t)kMaxPartials;
    DlState* const st = Y.d_state;
    DlState S;
    int attempt = 0, rounds = 0;
    auto trial_chain = [&]() -> int {
      launch_dl_trial(c->stream, nullptr, c->n, c->d_free_id, st, c->d_poses, bv, gv, trial);
      const int r = lm_chi2(c, trial, chi_trial);
      if (r) return r;
      launch_dl_decide(c->stream, nullptr, false, chi_trial, attempt, max_iters, st);
      launch_lm_commit(c->stream, &st->lm, attempt, (int)V3, trial, c->d_poses);
      ++attempt;
      return SGO_OK;
    };
    auto read_state = [&]() -> int {
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(&S, st, sizeof(S), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      ++rounds;
      return SGO_OK;
    };
    if ((rc = lm_chi2(c, c->d_poses, chi0))) return rc;
    launch_dl_begin(c->stream, nullptr, chi0, delta_init, max_iters, st);
    if (max_iters == 0 && (rc = read_state())) return rc;
    while (max_iters > 0) {
      {
        Scope sc(c, K_LINEARIZE, 128.0 * c->S0.ncs + 72.0 * c->S0.nu + 72.0 * c->n);
        launch_linearize(c->stream, c->S0, 0, c->S0.ngrp, c->es, c->d_poses, c->d_dgb);
      }
      int fgrid = 0;
      {
        Scope sc(c, K_FINALIZE, (72.0 + 48.0 + 48.0 + 6 * 24.0) * c->n);
        launch_finalize(c->stream, c->S0, 0, c->n, c->d_dgb, c->d_b, c->d_x, c->d_r, c->d_z, c->d_p, c->amg ? amg_xs0(c->amg) : nullptr,
                        c->amg ? amg_omega(c->amg) : 0.0, c->d_partials, &fgrid, &st->lm.lambda);
      }
      if ((rc = start_pcg(c, fgrid)) || (rc = run_pcg(c))) return rc;
      bool ok = c->h_S->stop == 1;
      if (!ok) {
        double eta = 1.0;
        if ((rc = solve_at_floor(c, &ok, &eta))) return rc;
      }
      const int nv = launch_dl_vectors_rows(c->stream, c->n, c->d_free_id, c->d_b, c->d_x, bv, gv, vparts);
      const int nf = launch_dl_forms(c->stream, c->el, nullptr, c->d_poses, bv, gv, fparts);
      launch_dl_prepare(c->stream, nullptr, ok ? 1 : 0, vparts, nv, fparts, nf, st);
      if ((rc = trial_chain()) || (rc = read_state())) return rc;
      while (!S.lm.stop && S.phase == kDlOpen) {
        for (int k = 0; k < kDlLightTrials; ++k)
          if ((rc = trial_chain())) return rc;
        if ((rc = read_state())) return rc;
      }
      if (S.lm.stop) break;
    }
    prof_flush(c);
    if (out) dl_fill_stats(S, rounds, wall_s() - t0, out);
    return S.lm.it;
  } SGO_CATCH(c)
}

}  // extern "C"
