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
// flags: the multifrontal path's flag words (the stop word goes into flags[0]; flags[0] and flags[2] are the trial's solve failures),
// or nullptr on the PCG route, whose host reads the state after every trial and hands the solve's outcome in as solve_ok
void launch_lm_begin(hipStream_t s, int* flags, const double* partials, int nparts, const double* chi2, double lambda_init, int max_iters,
                     LmState* st);
void launch_lm_trial(hipStream_t s, const MfDev& M, const LmDiagDev& G, const LmState* st, const double* poses, double* trial_poses,
                     double* partials);
void launch_lm_decide(hipStream_t s, int* flags, int solve_ok, const double* partials, int nparts, const double* chi2_trial, int attempt,
                      int max_iters, LmState* st);
void launch_lm_commit(hipStream_t s, const LmState* st, int attempt, int V3, const double* trial_poses, double* poses);
void launch_lm_finish(hipStream_t s, const MfDev& M);
int lm_grid(int n);   // the grid of k_lm_lambda0 / k_lm_trial = their partials

// ---- the PCG route (sgo_optimize_lm_pcg, sgo_lm_pcg.cpp): one attempt is
//   k_linearize         H and b at the accepted poses into dgb (sgo_kernels.hip's own kernel)
//   k_lm_lambda0_rows,  first attempt of a call: max |diag(H)| over the rows of dgb, then k_lm_begin as above
//   k_finalize<LM>      the level-0 diagonal blocks, their inverses and the PCG start state of H + lambda I, lambda read from the state
//   start_pcg, run_pcg  the hierarchy refreshed for H + lambda I, the cold solve at pcg_tol relative to its own |b| (sgo_solve.cpp)
//   k_lm_trial_pcg      trial poses = poses (+) x, partial sums of x . (lambda x + b) from d_x and d_b
//   chi2 at the trial poses, k_lm_decide (solve_ok from the host's reading of the solve), k_lm_commit
// and one read of the state: the PCG reads its scalars on the host anyway.
// dgb: [n][9] the rows' diagonal blocks (upper triangle) and right-hand sides; -> the workgroups' maxima of |d[0]|, |d[3]|, |d[5]|
void launch_lm_lambda0_rows(hipStream_t s, int n, const double* dgb, double* partials);
// free_id: row -> vertex (k_pose_update's map); x, b: the solve's solution and right-hand side in row order
void launch_lm_trial_pcg(hipStream_t s, int n, const int* free_id, const LmState* st, int solve_ok, const double* poses, const double* x,
                         const double* b, double* trial_poses, double* partials);

}  // namespace sgo

// the host side both routes share (sgo_lm.cpp)
struct sgo_ctx;
namespace sgo {
// the argument checks of sgo_optimize_lm, sgo_optimize_lm_pcg and the dogleg calls (`name` and the third argument's name `what` in the
// error text): SGO_EINVAL with nothing changed
int lm_check_args(sgo_ctx* c, const char* name, int32_t max_iters, double lambda_init, const char* what = "lambda_init");
// (plain, robust) chi2 at `poses` into out2 by the very launches sgo_chi2 makes on this context
int lm_chi2(sgo_ctx* c, double* poses, double* out2);
// the free poses' diagonal targets (LmDiagDev) of the plan on the device, once per plan (sgo_optimize_dogleg shares them)
int lm_diag_prepare(sgo_ctx* c, Mfront* m);
}  // namespace sgo
