// sgo_lm.h -- sgo_optimize_lm (include/sgo.h): Levenberg-Marquardt with g2o's schedule on the multifrontal
// factor.  One ATTEMPT -- one trial of one iteration -- is a uniform chain of launches that needs no answer from the host:
//   k_mf_edges       the elements at the accepted poses (sgo_mfront.hip's own kernel)
//   k_lm_lambda0,    first attempt of a call: max |diag(H)| from the elements, then lambda_0, nu and the starting chi2 into the
//   k_lm_begin       device state
//   k_mf_merge, k_mf_panels<LM>, k_mf_solve per level: (H + lambda I) x = b, lambda read from the state
//   k_lm_trial       trial poses = poses (+) x into a second pose buffer, partial sums of x . (lambda x + b)
//   chi2 at the trial poses by the launches sgo_chi2 makes on this context (so that the history is sgo_chi2's to the bit)
//   k_lm_decide      one wave: rules::lm_trial, the trace, the stop word
//   k_lm_commit      trial poses -> poses when the trial was accepted
// The host queues as many attempts as iterations remain, reads the state once, and repeats while iterations remain and nothing
// has stopped; after a stop every queued launch of the multifrontal path's and of this file's kernels returns on the stop word
// (flags[0], as after sgo_optimize_gn_until's), which k_lm_finish clears.  The chi2 launches are sgo_chi2's own kernels, which know
// no stop word: the attempts queued behind a stop still run them -- at most max_iters - 1 passes over the edges into scratch.
// No atomics, vector stores only, every sum in a fixed order.
#pragma once
#include <hip/hip_runtime.h>

#include "sgo_mfront_dev.h"

namespace sgo {

// flags[0] after a stop: the value sgo_optimize_gn_until's launches return on (kMfStopped, sgo_mfront.hip)
constexpr int kLmStopWord = 3;

struct LmState {
  double lambda, nu;          // the damping and its growth factor for the NEXT trial
  double cur, cur_plain;      // robust / plain chi2 at the accepted poses
  double lambda0;
  int it, q;                  // iterations counted; trials of the running iteration
  int stop, stop_reason;      // stop: the call has ended (SGO_LM_STOP_*)
  int trials_total;
  int commit_at;              // the attempt whose trial poses k_lm_commit copies (-1: none yet)
  double h_lambda[SGO_MAX_ITERS], h_rob[SGO_MAX_ITERS + 1], h_plain[SGO_MAX_ITERS + 1];
  int h_trials[SGO_MAX_ITERS];
};

// scratch of one call: [0 .. 1] chi2 at the accepted poses of the call's start, [2 .. 3] at the trial poses, then the partial
// sums / maxima [kMaxPartials]
constexpr size_t kLmScratchDoubles = 4 + (size_t)kMaxPartials;

void launch_lm_lambda0(hipStream_t s, const MfDev& M, const LmDiagDev& G, double* partials);
void launch_lm_begin(hipStream_t s, const MfDev& M, const double* partials, int nparts, const double* chi2, double lambda_init, int max_iters,
                     LmState* st);
void launch_lm_trial(hipStream_t s, const MfDev& M, const LmDiagDev& G, const LmState* st, const double* poses, double* trial_poses,
                     double* partials);
void launch_lm_decide(hipStream_t s, const MfDev& M, const double* partials, int nparts, const double* chi2_trial, int attempt, int max_iters,
                      LmState* st);
void launch_lm_commit(hipStream_t s, const LmState* st, int attempt, int V3, const double* trial_poses, double* poses);
void launch_lm_finish(hipStream_t s, const MfDev& M);
int lm_grid(int n);   // the grid of k_lm_lambda0 / k_lm_trial = their partials

}  // namespace sgo
