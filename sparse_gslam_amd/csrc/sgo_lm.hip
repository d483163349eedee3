// sgo_lm.hip -- the kernels of sgo_optimize_lm that are not the multifrontal path's own (sgo_lm.h has the chain; DESIGN.md section
// 5n): g2o's OptimizationAlgorithmLevenberg::solve -- computeLambdaInit, the trial loop's update / computeScale / gain ratio, push and
// discardTop or pop -- on the device, around the factorisation of H + lambda I.
//   k_lm_lambda0   one lane per free pose: its three diagonal sums of H from the elements, in k_mf_panels' contribution order; the
//                  workgroups' maxima of their absolute values
//   k_lm_begin     one wave: lambda_0, nu = 2, the starting chi2 and the zeroed counters into LmState
//   k_lm_trial     one lane per free pose: trial pose = pose (+) x, and x . (lambda x + b) with b re-formed from the elements (the
//                  factorisation has consumed the right-hand-side row), summed per workgroup
//   k_lm_decide    one wave: the sum of those partial sums in mf_chi2_sum's order, rules::lm_trial, the trace, the stop word; a failed
//                  factorisation (flags[0] == 1) or substitution (flags[2]) is solve_ok = 0, and both words are cleared
//   k_lm_commit    trial poses -> poses, for the attempt k_lm_decide accepted
//   k_lm_finish    one wave: clears the stop word
//   k_lm_lambda0_rows, k_lm_trial_pcg   the PCG route's (sgo_optimize_lm_pcg; sgo_lm.h has that chain):
//                  max |diag(H)| over the rows of the linearisation; trial poses and x . (lambda x + b) from the solve's x and b
// Streaming kernels at the launch floor for the graphs the multifrontal analysis admits (3 n doubles read and written per attempt,
// against a factorisation of the whole arena); no atomics, vector stores only, every sum in a fixed order.
#include <algorithm>

#include "sgo_device.h"
#include "sgo_internal.h"
#include "sgo_lm.h"
#include "sgo_rules.h"

namespace sgo {
namespace {

__global__ __launch_bounds__(kBlock) void k_lm_lambda0(MfDev M, LmDiagDev G, double* __restrict__ partials) {
  __shared__ double sm[kWavesPerBlock];
  double mx = 0.0;
  for (int p = blockIdx.x * kBlock + threadIdx.x; p < M.n; p += gridDim.x * kBlock) {
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = G.ptr[p]; k < G.ptr[p + 1]; ++k) lm_target_terms(M, G.tgt[k], acc);
    mx = fmax(mx, fmax(fabs(acc[0]), fmax(fabs(acc[3]), fabs(acc[5]))));   // D's upper triangle by rows: the diagonal is 0, 3, 5
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kWavesPerBlock; ++k) mx = fmax(mx, sm[k]);
    partials[blockIdx.x] = mx;
  }
}

__global__ __launch_bounds__(64) void k_lm_begin(int* __restrict__ flags, const double* __restrict__ partials, int nparts,
                                                 const double* __restrict__ chi2, double lambda_init, int max_iters,
                                                 LmState* __restrict__ st) {
  double mx = 0.0;
  for (int q = threadIdx.x; q < nparts; q += 64) mx = fmax(mx, partials[q]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (threadIdx.x != 0) return;
  const double lambda0 = lambda_init > 0.0 ? lambda_init : 1e-5 * mx;
  st->lambda = st->lambda0 = lambda0;
  st->nu = 2.0;
  st->cur_plain = st->h_plain[0] = chi2[0];
  st->cur = st->h_rob[0] = chi2[1];
  st->it = st->q = st->trials_total = 0;
  st->commit_at = -1;
  st->stop = max_iters == 0 ? 1 : 0;
  st->stop_reason = SGO_LM_STOP_MAX_ITERS;
  if (max_iters == 0 && flags) flags[0] = kLmStopWord;
}

__global__ __launch_bounds__(kBlock) void k_lm_trial(MfDev M, LmDiagDev G, const LmState* __restrict__ st, const double* __restrict__ poses,
                                                     double* __restrict__ trial_poses, double* __restrict__ partials) {
  const int f0 = M.flags[0];
  if (f0 == kLmStopWord) return;
  const bool solve_ok = f0 == 0 && M.flags[2] == 0;   // (set by the launches before this one: every workgroup sees the same values)
  const double lambda = st->lambda;
  double acc[1] = {0.0};
  for (int p = blockIdx.x * kBlock + threadIdx.x; p < M.n; p += gridDim.x * kBlock) {
    const size_t v = 3 * (size_t)M.elim_vertex[p], o = 3 * (size_t)p;
    const double x[3] = {M.x[o], M.x[o + 1], M.x[o + 2]};
    double t[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = G.ptr[p]; k < G.ptr[p + 1]; ++k) lm_target_terms(M, G.tgt[k], t);
    acc[0] += x[0] * (lambda * x[0] + t[6]) + x[1] * (lambda * x[1] + t[7]) + x[2] * (lambda * x[2] + t[8]);
    if (solve_ok) {
      trial_poses[v] = poses[v] + x[0];
      trial_poses[v + 1] = poses[v + 1] + x[1];
      trial_poses[v + 2] = norm_theta(poses[v + 2] + x[2]);
    }
  }
  block_sum_store<1>(acc, partials, kMaxPartials);
}

// flags: the multifrontal path's words, nullptr on the PCG route (sgo_lm.h); solve_ok: what the host says of the trial's solve (the
// factor route hands in 1: its failures are the flag words')
__global__ __launch_bounds__(64) void k_lm_decide(int* __restrict__ flags, int solve_ok, const double* __restrict__ partials, int nparts,
                                                  const double* __restrict__ chi2_trial, int attempt, int max_iters,
                                                  LmState* __restrict__ st) {
  const int f0 = flags ? flags[0] : 0;
  if (f0 == kLmStopWord) return;
  double s = 0.0;
  for (int q = threadIdx.x; q < nparts; q += 64) s += partials[q];
  s = wave_sum(s);
  if (threadIdx.x != 0) return;
  if (flags) {
    solve_ok = solve_ok && f0 == 0 && flags[2] == 0;
    flags[0] = flags[1] = flags[2] = 0;
  }
  double lambda = st->lambda, nu = st->nu;
  const int code = rules::lm_trial(st->cur, chi2_trial[1], s + 1e-3, solve_ok, &lambda, &nu);
  st->lambda = lambda;
  st->nu = nu;
  const int q = ++st->q;
  ++st->trials_total;
  if (code == rules::kLmAccept) {
    st->cur_plain = chi2_trial[0];
    st->cur = chi2_trial[1];
    st->commit_at = attempt;
  }
  const bool lambda_bad = !(lambda - lambda == 0.0);
  if (code == rules::kLmRetry && q < rules::kLmMaxTrials && !lambda_bad) return;   // the iteration tries again
  const int it = st->it++;
  st->h_lambda[it] = lambda;
  st->h_rob[it + 1] = st->cur;
  st->h_plain[it + 1] = st->cur_plain;
  st->h_trials[it] = q;
  st->q = 0;
  int reason = -1;
  if (q == rules::kLmMaxTrials) reason = SGO_LM_STOP_TRIALS;
  else if (code == rules::kLmZeroGain) reason = SGO_LM_STOP_ZERO_GAIN;
  else if (lambda_bad) reason = SGO_LM_STOP_LAMBDA;
  else if (it + 1 == max_iters) reason = SGO_LM_STOP_MAX_ITERS;
  if (reason >= 0) {
    st->stop = 1;
    st->stop_reason = reason;
    if (flags) flags[0] = kLmStopWord;
  }
}

// ---- the PCG route (sgo_lm.h)
__global__ __launch_bounds__(kBlock) void k_lm_lambda0_rows(int n, const double* __restrict__ dgb, double* __restrict__ partials) {
  __shared__ double sm[kWavesPerBlock];
  double mx = 0.0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const double* d = dgb + 9 * (size_t)i;
    mx = fmax(mx, fmax(fabs(d[0]), fmax(fabs(d[3]), fabs(d[5]))));   // D's upper triangle by rows: the diagonal is 0, 3, 5
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kWavesPerBlock; ++k) mx = fmax(mx, sm[k]);
    partials[blockIdx.x] = mx;
  }
}

// One lane per free row: the trial pose of its vertex (k_pose_update's map and arithmetic, into the second pose buffer) when the
// solve succeeded, and the row's share of x . (lambda x + b), summed per workgroup in block_sum_store's order.
__global__ __launch_bounds__(kBlock) void k_lm_trial_pcg(int n, const int* __restrict__ free_id, const LmState* __restrict__ st, int solve_ok,
                                                         const double* __restrict__ poses, const double* __restrict__ x,
                                                         const double* __restrict__ b, double* __restrict__ trial_poses,
                                                         double* __restrict__ partials) {
  const double lambda = st->lambda;
  double acc[1] = {0.0};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const size_t v = 3 * (size_t)free_id[i], o = 3 * (size_t)i;
    const double x0 = x[o], x1 = x[o + 1], x2 = x[o + 2];
    acc[0] += x0 * (lambda * x0 + b[o]) + x1 * (lambda * x1 + b[o + 1]) + x2 * (lambda * x2 + b[o + 2]);
    if (solve_ok) {
      trial_poses[v] = poses[v] + x0;
      trial_poses[v + 1] = poses[v + 1] + x1;
      trial_poses[v + 2] = norm_theta(poses[v + 2] + x2);
    }
  }
  block_sum_store<1>(acc, partials, kMaxPartials);
}

__global__ __launch_bounds__(kBlock) void k_lm_commit(const LmState* __restrict__ st, int attempt, int V3, const double* __restrict__ trial_poses,
                                                      double* __restrict__ poses) {
  if (st->commit_at != attempt) return;   // (rejected, or a launch queued behind the stop)
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < V3; i += gridDim.x * kBlock) poses[i] = trial_poses[i];
}

__global__ __launch_bounds__(64) void k_lm_finish(MfDev M) {
  if (threadIdx.x == 0 && M.flags[0] == kLmStopWord) M.flags[0] = 0;
}

}  // namespace

int lm_grid(int n) { return std::max(1, std::min((n + kBlock - 1) / kBlock, kMaxPartials)); }

void launch_lm_lambda0(hipStream_t s, const MfDev& M, const LmDiagDev& G, double* partials) {
  hipLaunchKernelGGL(k_lm_lambda0, dim3(lm_grid(M.n)), dim3(kBlock), 0, s, M, G, partials);
}
void launch_lm_begin(hipStream_t s, int* flags, const double* partials, int nparts, const double* chi2, double lambda_init, int max_iters,
                     LmState* st) {
  hipLaunchKernelGGL(k_lm_begin, dim3(1), dim3(64), 0, s, flags, partials, nparts, chi2, lambda_init, max_iters, st);
}
void launch_lm_trial(hipStream_t s, const MfDev& M, const LmDiagDev& G, const LmState* st, const double* poses, double* trial_poses,
                     double* partials) {
  hipLaunchKernelGGL(k_lm_trial, dim3(lm_grid(M.n)), dim3(kBlock), 0, s, M, G, st, poses, trial_poses, partials);
}
void launch_lm_decide(hipStream_t s, int* flags, int solve_ok, const double* partials, int nparts, const double* chi2_trial, int attempt,
                      int max_iters, LmState* st) {
  hipLaunchKernelGGL(k_lm_decide, dim3(1), dim3(64), 0, s, flags, solve_ok, partials, nparts, chi2_trial, attempt, max_iters, st);
}
void launch_lm_commit(hipStream_t s, const LmState* st, int attempt, int V3, const double* trial_poses, double* poses) {
  hipLaunchKernelGGL(k_lm_commit, dim3(std::max(1, std::min((V3 + kBlock - 1) / kBlock, kMaxGrid))), dim3(kBlock), 0, s, st, attempt, V3,
                     trial_poses, poses);
}
void launch_lm_finish(hipStream_t s, const MfDev& M) { hipLaunchKernelGGL(k_lm_finish, dim3(1), dim3(64), 0, s, M); }
void launch_lm_lambda0_rows(hipStream_t s, int n, const double* dgb, double* partials) {
  hipLaunchKernelGGL(k_lm_lambda0_rows, dim3(lm_grid(n)), dim3(kBlock), 0, s, n, dgb, partials);
}
void launch_lm_trial_pcg(hipStream_t s, int n, const int* free_id, const LmState* st, int solve_ok, const double* poses, const double* x,
                         const double* b, double* trial_poses, double* partials) {
  hipLaunchKernelGGL(k_lm_trial_pcg, dim3(lm_grid(n)), dim3(kBlock), 0, s, n, free_id, st, solve_ok, poses, x, b, trial_poses, partials);
}

}  // namespace sgo
