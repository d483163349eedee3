// sgo_dogleg.h -- sgo_optimize_dogleg and sgo_optimize_dogleg_pcg (include/sgo.h): Powell's dogleg with g2o's
// schedule.  One ITERATION solves the undamped H g = b once; every TRIAL of it is a blend a b + c g of two fixed vectors.
// The iteration chain, which needs no answer from the host on the factor route:
//   k_mf_edges, per level k_mf_merge, k_mf_panels<LM>, k_mf_solve     (factor route: sgo_lm.h's launches; lambda read from the state,
//                                                                      0.0 while no solve has failed: d + 0.0 is d)
//   k_linearize, k_finalize<LM>, start_pcg, run_pcg                   (PCG route: sgo_lm.h's; the host reads the solve's outcome)
//   k_dl_vectors    b and g per vertex [V][3] (fixed poses stay zero); the workgroups' partial sums of b.b, b.g, g.g
//   k_dl_forms      one lane per edge: u = A b_i + B b_j, v = A g_i + B g_j; partial sums of w u'Omega u, w u'Omega v, w v'Omega v
//   k_dl_prepare    one wave: the ordered sums into the state; a failed solve becomes the damping step instead
//   k_dl_trial      rules::dogleg_step from the state's delta, trial poses = poses (+) (a b + c g) into the second pose buffer
//   chi2 at the trial poses by the launches sgo_chi2 makes (lm_chi2)
//   k_dl_decide     one wave: rules::dogleg_trial, the trace, delta, the stop word, the phase
//   k_lm_commit     sgo_lm.hip's: trial poses -> poses for the trial that was accepted
// A rejection leaves the phase at kDlOpen and puts the stop word into flags[0]: every later launch of the round that is this
// file's or the multifrontal path's returns.  The host then queues LIGHT trial chains -- k_dl_trial, chi2, k_dl_decide,
// k_lm_commit, gated by the phase alone --, k_dl_resume (one wave: clears the word once the iteration is closed) and the remaining
// iteration chains.  No atomics, vector stores only, every sum in a fixed order.
#pragma once
#include <hip/hip_runtime.h>

#include "sgo_lm.h"

namespace sgo {

constexpr int kDlClosed = 0;   // between iterations: the next chain solves
constexpr int kDlOpen = 1;     // b, g and the six forms are those of the accepted poses: trials run
constexpr int kDlResolve = 2;  // the solve failed: the next chain repeats it on H + lambda I
constexpr int kDlLightTrials = 8;   // light trial chains per round

struct DlState {
  // lambda: the word k_mf_panels<LM> / k_finalize<LM> add (0.0 while was_pd); cur, cur_plain, it, q, stop, stop_reason, trials_total,
  // commit_at, h_rob, h_plain, h_trials as sgo_lm.h has them; h_lambda: delta after iteration k; nu, lambda0 unused
  LmState lm;
  double delta, delta0;
  double damping;             // g2o's _currentLambda
  double lambda_used;         // the last damping a solve used (0: none)
  double forms[6];            // b.b, b.g, g.g, b.Hb, b.Hg, g.Hg at the accepted poses
  double step_norm, gain;     // of the trial k_dl_trial has formed
  int kind;                   // ... and its kind
  int was_pd, phase, solves;
  int h_kind[SGO_MAX_ITERS];
};

// scratch of one call: [0 .. 1] chi2 at the call's start, [2 .. 3] at the trial poses, then k_dl_vectors' and k_dl_forms' partial
// sums [3][kMaxPartials] each
constexpr size_t kDlScratchDoubles = 4 + 6 * (size_t)kMaxPartials;

void launch_dl_begin(hipStream_t s, int* flags, const double* chi2, double delta_init, int max_iters, DlState* st);
// b re-formed from the element records and g from the fronts' x, by elimination position; -> grid = the partial sums per row
int launch_dl_vectors_mf(hipStream_t s, const MfDev& M, const LmDiagDev& G, double* bv, double* gv, double* partials);
// ... from the solve's right-hand side and solution in row order; free_id: row -> vertex
int launch_dl_vectors_rows(hipStream_t s, int n, const int* free_id, const double* b, const double* x, double* bv, double* gv, double* partials);
// flags: the multifrontal path's words or nullptr (PCG route)
int launch_dl_forms(hipStream_t s, const EdgeListDev& el, const int* flags, const double* poses, const double* bv, const double* gv,
                    double* partials);
void launch_dl_prepare(hipStream_t s, int* flags, int solve_ok, const double* vparts, int nv, const double* fparts, int nf, DlState* st);
// gate: the flag words whose stop word the launch returns on, or nullptr (light chains, PCG route); row_vertex: [n] the free poses
void launch_dl_trial(hipStream_t s, const int* gate, int n, const int* row_vertex, DlState* st, const double* poses, const double* bv,
                     const double* gv, double* trial_poses);
void launch_dl_decide(hipStream_t s, int* flags, bool gated, const double* chi2_trial, int attempt, int max_iters, DlState* st);
void launch_dl_resume(hipStream_t s, int* flags, DlState* st);

}  // namespace sgo

// the host side both routes share (sgo_dogleg.cpp)
struct sgo_ctx;
namespace sgo {
// the call's buffers, grown on demand: the trial poses (sgo_optimize_lm's, the fixed poses' entries copied), b and g by vertex
// (zeroed: the fixed poses' entries stay zero), the scratch and the state
int dl_buffers(sgo_ctx* c);
void dl_fill_stats(const DlState& S, int rounds, double seconds, sgo_dogleg_stats* out);
}  // namespace sgo
