// sgo_dogleg.cpp -- sgo_optimize_dogleg (include/sgo.h): the host driver of the chains sgo_dogleg.h describes, on
// the multifrontal factor.  The plan is selinv_plan's, as for sgo_optimize_lm, so sgo_optimize_gn keeps its path: the call writes
// the factor's arrays, the scratch d_hist / d_dres / d_partials, the call's own buffers and the poses.
// Also the two pure rules and what both routes share (the buffers, the stats).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "sgo_ctx.h"
#include "sgo_dogleg.h"
#include "sgo_rules.h"

using namespace sgo;

namespace sgo {

// the trial poses (sgo_optimize_lm's buffer), b and g by vertex [2][V][3] zeroed (the fixed poses' entries stay zero), the scratch and
// the state
int dl_buffers(sgo_ctx* c) {
  sgo_ctx::Lm& Z = c->lm;
  sgo_ctx::Dl& Y = c->dl;
  const size_t V3 = 3 * (size_t)c->V;
  int rc;
  if ((rc = grow_device(c, &Z.d_trial, &Z.trial_cap, V3)) || (rc = grow_device(c, &Y.d_vec, &Y.vec_cap, 2 * V3)) ||
      (rc = grow_device(c, &Y.d_scratch, &Y.scratch_cap, kDlScratchDoubles)) || (rc = grow_device(c, &Y.d_state, &Y.state_cap, (size_t)1)))
    return rc;
  HIP_TRY(c, hipMemsetAsync(Y.d_vec, 0, sizeof(double) * 2 * V3, c->stream));
  HIP_TRY(c, hipMemcpyAsync(Z.d_trial, c->d_poses, sizeof(double) * V3, hipMemcpyDeviceToDevice, c->stream));   // (the fixed poses' entries)
  return SGO_OK;
}

void dl_fill_stats(const DlState& S, int rounds, double seconds, sgo_dogleg_stats* out) {
  const int it = S.lm.it;
  out->iters_done = it;
  out->trials_total = S.lm.trials_total;
  out->solves = S.solves;
  out->stop_reason = S.lm.stop_reason;
  out->sync_rounds = rounds;
  out->delta0 = S.delta0;
  std::copy(S.lm.h_lambda, S.lm.h_lambda + it, out->delta);
  std::copy(S.lm.h_rob, S.lm.h_rob + it + 1, out->robust_chi2);
  std::copy(S.lm.h_plain, S.lm.h_plain + it + 1, out->chi2);
  std::copy(S.lm.h_trials, S.lm.h_trials + it, out->trials);
  std::copy(S.h_kind, S.h_kind + it, out->step_kind);
  out->lambda = S.lambda_used;
  out->seconds_total = seconds;
}

}  // namespace sgo

extern "C" {

int sgo_dogleg_step_rule(double delta, const double forms[6], double* a, double* c, double* step_norm, double* linear_gain) {
  if (!forms || !a || !c || !step_norm || !linear_gain) return SGO_EINVAL;
  return rules::dogleg_step(delta, forms, a, c, step_norm, linear_gain);
}

int sgo_dogleg_trial_rule(double cur, double trial, double linear_gain, double step_norm, double* delta) {
  if (!delta) return SGO_EINVAL;
  return rules::dogleg_trial(cur, trial, linear_gain, step_norm, delta);
}

int sgo_optimize_dogleg(sgo_ctx* c, int32_t max_iters, double delta_init, sgo_dogleg_stats* out) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if ((rc = lm_check_args(c, "sgo_optimize_dogleg", max_iters, delta_init, "delta_init"))) return rc;
    if (out) {
      std::memset(out, 0, sizeof(*out));
      out->iters_requested = max_iters;
    }
    if (c->n == 0) return SGO_ENOTHING;
    const double t0 = wall_s();
    HIP_TRY(c, hipSetDevice(c->device));
    Mfront* m = nullptr;
    if ((rc = selinv_plan(c, &m, "sgo_optimize_dogleg", "sgo_optimize_dogleg_pcg or sgo_optimize_gn")) || (rc = lm_diag_prepare(c, m)))
      return rc;
    const MfDev& D = m->dev;
    if ((rc = dl_buffers(c))) return rc;
    sgo_ctx::Dl& Y = c->dl;
    double* const trial = c->lm.d_trial;
    const size_t V3 = 3 * (size_t)c->V;
    double *bv = Y.d_vec, *gv = Y.d_vec + V3;
    double *chi0 = Y.d_scratch, *chi_trial = Y.d_scratch + 2, *vparts = Y.d_scratch + 4, *fparts = vparts + 3 * (size_t)kMaxPartials;
    DlState* const st = Y.d_state;
    DlState S;
    int attempt = 0, rounds = 0;
    auto trial_chain = [&](bool gated) -> int {   // one trial of the open iteration: what a rejected trial costs again
      launch_dl_trial(c->stream, gated ? D.flags : nullptr, D.n, D.elim_vertex, st, c->d_poses, bv, gv, trial);
      const int r = lm_chi2(c, trial, chi_trial);
      if (r) return r;
      launch_dl_decide(c->stream, D.flags, gated, chi_trial, attempt, max_iters, st);
      launch_lm_commit(c->stream, &st->lm, attempt, (int)V3, trial, c->d_poses);
      ++attempt;
      return SGO_OK;
    };
    {
      Scope sc(c, K_LM, mfront_bytes(m, c->E, max_iters), true);
      HIP_TRY(c, hipMemsetAsync(D.flags, 0, sizeof(int) * 8, c->stream));
      if ((rc = lm_chi2(c, c->d_poses, chi0))) return rc;
      launch_dl_begin(c->stream, D.flags, chi0, delta_init, max_iters, st);
      for (;;) {
        int queued = max_iters;
        if (rounds > 0) {
          queued = max_iters - S.lm.it;
          if (S.phase == kDlOpen) {
            for (int k = 0; k < kDlLightTrials; ++k)
              if ((rc = trial_chain(false))) return rc;
            --queued;   // (the open iteration is the light chains')
          }
          launch_dl_resume(c->stream, D.flags, st);
        }
        for (int a = 0; a < queued; ++a) {
          mfront_lm_edges(m, c->stream, c->el, c->d_poses, c->d_hist, c->d_dres);
          mfront_lm_solve(m, c->stream, &st->lm, c->d_hist, c->d_dres);
          const int nv = launch_dl_vectors_mf(c->stream, D, m->lm_diag, bv, gv, vparts);
          const int nf = launch_dl_forms(c->stream, c->el, D.flags, c->d_poses, bv, gv, fparts);
          launch_dl_prepare(c->stream, D.flags, 1, vparts, nv, fparts, nf, st);
          if ((rc = trial_chain(true))) return rc;
        }
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&S, st, sizeof(S), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        ++rounds;
        if (S.lm.stop) break;
      }
      launch_lm_finish(c->stream, D);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    m->sel_ran = false;   // (the factor's arrays are those of the last solve)
    c->linearized = false;
    if (out) dl_fill_stats(S, rounds, wall_s() - t0, out);
    return S.lm.it;
  } SGO_CATCH(c)
}

}  // extern "C"
