// sgo_lm.cpp -- sgo_optimize_lm (include/sgo.h): the host driver of the attempts sgo_lm.h describes.  The plan is
// selinv_plan's -- the resident multifrontal plan, or one analysed once per set-up for a graph whose optimize() takes the
// single-launch or the PCG path --, so sgo_optimize_gn keeps its path: the call writes the factor's arrays, which every
// factorisation recomputes from the poses, the scratch d_hist / d_dres / d_partials, and the poses.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "sgo_ctx.h"
#include "sgo_lm.h"
#include "sgo_rules.h"

using namespace sgo;

namespace {

// The free poses' diagonal targets on the device, once per plan: a pose's diagonal block collects contributions in its own front and
// in every descendant front that holds it as a boundary pose.
int lm_prepare(sgo_ctx* c, Mfront* m) {
  if (m->lm_diag.ptr) return SGO_OK;
  const MfPlan& P = m->plan;
  std::vector<int> ptr((size_t)P.n + 1, 0), pos;
  for (const MfFront& F : P.fronts)
    for (int t = F.tgt0; t < F.tgt1; ++t) {
      const MfTarget& T = P.targets[(size_t)t];
      if (T.li != T.lj) continue;
      const int p = T.li < F.own ? F.e0 + T.li : P.bnd[(size_t)F.bnd_off + (size_t)(T.li - F.own)];
      pos.push_back(p);
      ++ptr[(size_t)p + 1];
    }
  for (int p = 0; p < P.n; ++p) ptr[(size_t)p + 1] += ptr[(size_t)p];
  std::vector<int> tgt(std::max<size_t>(pos.size(), 1), 0), fill(ptr.begin(), ptr.end() - 1);
  size_t k = 0;
  for (const MfFront& F : P.fronts)   // (the same walk: the targets of a pose in ascending order)
    for (int t = F.tgt0; t < F.tgt1; ++t)
      if (P.targets[(size_t)t].li == P.targets[(size_t)t].lj) tgt[(size_t)fill[(size_t)pos[k++]]++] = t;
  int *d_ptr = nullptr, *d_tgt = nullptr;
  int rc;
  if ((rc = upload(c, &d_ptr, ptr)) || (rc = upload(c, &d_tgt, tgt))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the host vectors above go out of scope)
  m->lm_diag.ptr = d_ptr;
  m->lm_diag.tgt = d_tgt;
  return SGO_OK;
}

}  // namespace

namespace sgo {

int lm_diag_prepare(sgo_ctx* c, Mfront* m) { return lm_prepare(c, m); }

// (plain, robust) chi2 at `poses` into out2 by the very launches sgo_chi2 makes on this context, so that the call's history and
// sgo_chi2 after it agree to the bit whatever path optimize() takes
int lm_chi2(sgo_ctx* c, double* poses, double* out2) {
  if (c->direct) {
    const hipError_t he = direct_optimize(c->direct, c->stream, c->el, poses, 0, out2, c->d_dres, nullptr);
    if (he != hipSuccess) {
      c->err = std::string("k_direct launch: ") + hipGetErrorString(he);
      return SGO_EHIP;
    }
    return SGO_OK;
  }
  int grid = 0;
  launch_chi2(c->stream, c->el, 0, c->el.E, poses, nullptr, c->d_partials, &grid, nullptr);
  launch_reduce2(c->stream, c->d_partials, grid, out2);
  return SGO_OK;
}

int lm_check_args(sgo_ctx* c, const char* name, int32_t max_iters, double lambda_init, const char* what) {
  const std::string who(name);
  if (max_iters < 0 || max_iters > SGO_MAX_ITERS) {
    c->err = who + ": max_iters must be in [0, SGO_MAX_ITERS]";
    return SGO_EINVAL;
  }
  if (!std::isfinite(lambda_init)) {
    c->err = who + ": " + what + " is not finite";
    return SGO_EINVAL;
  }
  if (c->ov.active) {
    c->err = who + ": the resident graph carries an incremental overlay (call sgo_set_graph_se2)";
    return SGO_EINVAL;
  }
  if (multi_gpu_context(c)) {
    c->err = who + ": not available in a multi-GPU context (call sgo_optimize_gn)";
    return SGO_EINVAL;
  }
  return SGO_OK;
}

}  // namespace sgo

extern "C" {

int sgo_lm_trial_rule(double cur, double trial, double scale, int solve_ok, double* lambda, double* nu) {
  if (!lambda || !nu) return SGO_EINVAL;
  return rules::lm_trial(cur, trial, scale, solve_ok, lambda, nu);
}

int sgo_optimize_lm(sgo_ctx* c, int32_t max_iters, double lambda_init, sgo_lm_stats* out) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if ((rc = lm_check_args(c, "sgo_optimize_lm", max_iters, lambda_init))) return rc;
    if (out) {
      std::memset(out, 0, sizeof(*out));
      out->iters_requested = max_iters;
    }
    if (c->n == 0) return SGO_ENOTHING;
    const double t0 = wall_s();
    HIP_TRY(c, hipSetDevice(c->device));
    Mfront* m = nullptr;
    if ((rc = selinv_plan(c, &m, "sgo_optimize_lm", "sgo_optimize_lm_pcg or sgo_optimize_gn")) || (rc = lm_prepare(c, m))) return rc;
    const MfDev& D = m->dev;
    sgo_ctx::Lm& Z = c->lm;
    const size_t V3 = 3 * (size_t)c->V;
    if ((rc = grow_device(c, &Z.d_trial, &Z.trial_cap, V3)) || (rc = grow_device(c, &Z.d_scratch, &Z.scratch_cap, kLmScratchDoubles)) ||
        (rc = grow_device(c, &Z.d_state, &Z.state_cap, (size_t)1)))
      return rc;
    double *chi0 = Z.d_scratch, *chi_trial = Z.d_scratch + 2, *partials = Z.d_scratch + 4;
    const int grid = lm_grid(D.n);
    LmState S;
    int attempt = 0, rounds = 0;
    {
      Scope sc(c, K_LM, mfront_bytes(m, c->E, max_iters), true);
      HIP_TRY(c, hipMemsetAsync(D.flags, 0, sizeof(int) * 8, c->stream));
      HIP_TRY(c, hipMemcpyAsync(Z.d_trial, c->d_poses, sizeof(double) * V3, hipMemcpyDeviceToDevice, c->stream));   // (the fixed poses' entries)
      if ((rc = lm_chi2(c, c->d_poses, chi0))) return rc;
      for (;;) {
        const int queued = attempt == 0 ? std::max(max_iters, 1) : max_iters - S.it;
        for (int a = 0; a < queued; ++a, ++attempt) {
          mfront_lm_edges(m, c->stream, c->el, c->d_poses, c->d_hist, c->d_dres);
          if (attempt == 0) {
            launch_lm_lambda0(c->stream, D, m->lm_diag, partials);
            launch_lm_begin(c->stream, D.flags, partials, grid, chi0, lambda_init, max_iters, Z.d_state);
          }
          mfront_lm_solve(m, c->stream, Z.d_state, c->d_hist, c->d_dres);
          launch_lm_trial(c->stream, D, m->lm_diag, Z.d_state, c->d_poses, Z.d_trial, partials);
          if ((rc = lm_chi2(c, Z.d_trial, chi_trial))) return rc;
          launch_lm_decide(c->stream, D.flags, 1, partials, grid, chi_trial, attempt, max_iters, Z.d_state);
          launch_lm_commit(c->stream, Z.d_state, attempt, (int)V3, Z.d_trial, c->d_poses);
        }
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&S, Z.d_state, sizeof(S), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        ++rounds;
        if (S.stop || S.it >= max_iters) break;
      }
      launch_lm_finish(c->stream, D);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    m->sel_ran = false;   // (the factor's arrays are those of H + lambda I of the last trial now)
    c->linearized = false;
    if (out) {
      out->iters_done = S.it;
      out->trials_total = S.trials_total;
      out->stop_reason = S.stop_reason;
      out->sync_rounds = rounds;
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

}  // extern "C"
