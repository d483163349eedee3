// sgo_dogleg.hip -- the kernels of sgo_optimize_dogleg / sgo_optimize_dogleg_pcg that are not the solver paths' own (sgo_dogleg.h has
// the chains): g2o's OptimizationAlgorithmDogleg::solve on the device, around ONE undamped solve per iteration.
//   k_dl_begin          one wave: delta_0, the damping, the starting chi2 and the zeroed counters into DlState
//   k_dl_vectors_mf     one lane per free pose (elimination position): b re-formed from the elements as k_lm_trial does, g from the
//                       fronts' x; both to [V][3] by vertex; the workgroups' partial sums of b.b, b.g, g.g
//   k_dl_vectors_rows   the same from the PCG's d_b and d_x through free_id
//   k_dl_forms          one lane per edge, the same kernel on both routes (H is never read as stored): u = A b_i + B b_j,
//                       v = A g_i + B g_j through sgo_device.h's edge arithmetic; partial sums of w u'Omega u, w u'Omega v, w v'Omega v
//   k_dl_prepare        one wave: the six ordered sums into the state and the iteration opened; a failed solve (flags[0] == 1 or 2,
//                       flags[2], the host's solve_ok == 0, a g.g that is not finite) is the damping step instead
//   k_dl_trial          one lane per free pose: rules::dogleg_step from the state's delta (every lane the same statement on the same
//                       operands), trial pose = pose (+) (a b + c g), the GN step copied; lane 0 of workgroup 0 records the step
//   k_dl_decide         one wave: rules::dogleg_trial, the trace, delta, the stop word, the phase
//   k_dl_resume         one wave, after a round's light trial chains: clears the stop word when the iteration is closed
// Streaming kernels (k_dl_forms reads what k_chi2 reads plus 12 doubles of the two vectors per edge); no atomics, vector stores
// only, every sum in a fixed order.
#include <algorithm>

#include "sgo_device.h"
#include "sgo_dogleg.h"
#include "sgo_internal.h"
#include "sgo_rules.h"

namespace sgo {
namespace {

__global__ __launch_bounds__(64) void k_dl_begin(int* __restrict__ flags, const double* __restrict__ chi2, double delta_init, int max_iters,
                                                 DlState* __restrict__ st) {
  if (threadIdx.x != 0) return;
  st->lm.lambda = 0.0;
  st->lm.nu = 0.0;
  st->lm.lambda0 = 0.0;
  st->lm.cur_plain = st->lm.h_plain[0] = chi2[0];
  st->lm.cur = st->lm.h_rob[0] = chi2[1];
  st->lm.it = st->lm.q = st->lm.trials_total = 0;
  st->lm.commit_at = -1;
  st->lm.stop = max_iters == 0 ? 1 : 0;
  st->lm.stop_reason = SGO_DL_STOP_MAX_ITERS;
  st->delta = st->delta0 = delta_init > 0.0 ? delta_init : rules::kDlDeltaInit;
  st->damping = rules::kDlLambdaInit;
  st->lambda_used = 0.0;
  st->step_norm = st->gain = 0.0;
  st->kind = -1;
  st->was_pd = 1;
  st->phase = kDlClosed;
  st->solves = 0;
  if (max_iters == 0 && flags) flags[0] = kLmStopWord;
}

__global__ __launch_bounds__(kBlock) void k_dl_vectors_mf(MfDev M, LmDiagDev G, double* __restrict__ bv, double* __restrict__ gv,
                                                          double* __restrict__ partials) {
  if (M.flags[0]) return;   // the stop word, or a failed factorisation: k_dl_prepare reads neither vector's sums then
  double acc[3] = {0.0, 0.0, 0.0};
  for (int p = blockIdx.x * kBlock + threadIdx.x; p < M.n; p += gridDim.x * kBlock) {
    const size_t v = 3 * (size_t)M.elim_vertex[p], o = 3 * (size_t)p;
    const double x[3] = {M.x[o], M.x[o + 1], M.x[o + 2]};
    double t[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = G.ptr[p]; k < G.ptr[p + 1]; ++k) lm_target_terms(M, G.tgt[k], t);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      bv[v + q] = t[6 + q];
      gv[v + q] = x[q];
    }
    acc[0] += t[6] * t[6] + t[7] * t[7] + t[8] * t[8];
    acc[1] += t[6] * x[0] + t[7] * x[1] + t[8] * x[2];
    acc[2] += x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  }
  block_sum_store<3>(acc, partials, kMaxPartials);
}

__global__ __launch_bounds__(kBlock) void k_dl_vectors_rows(int n, const int* __restrict__ free_id, const double* __restrict__ b,
                                                            const double* __restrict__ x, double* __restrict__ bv, double* __restrict__ gv,
                                                            double* __restrict__ partials) {
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const size_t v = 3 * (size_t)free_id[i], o = 3 * (size_t)i;
    const double b0 = b[o], b1 = b[o + 1], b2 = b[o + 2], x0 = x[o], x1 = x[o + 1], x2 = x[o + 2];
    bv[v] = b0; bv[v + 1] = b1; bv[v + 2] = b2;
    gv[v] = x0; gv[v + 1] = x1; gv[v + 2] = x2;
    acc[0] += b0 * b0 + b1 * b1 + b2 * b2;
    acc[1] += b0 * x0 + b1 * x1 + b2 * x2;
    acc[2] += x0 * x0 + x1 * x1 + x2 * x2;
  }
  block_sum_store<3>(acc, partials, kMaxPartials);
}

// J y = A y_i + B y_j for the edge's Jacobians: A's third row is (0, 0, -1), B's (0, 0, 1), B02 = B12 = 0
__device__ __forceinline__ void dl_jac_apply(const EdgeJac& J, const double* __restrict__ yi, const double* __restrict__ yj, double (&u)[3]) {
  u[0] = ((J.A00 * yi[0] + J.A01 * yi[1]) + J.A02 * yi[2]) + (J.B00 * yj[0] + J.B01 * yj[1]);
  u[1] = ((J.A10 * yi[0] + J.A11 * yi[1]) + J.A12 * yi[2]) + (J.B10 * yj[0] + J.B11 * yj[1]);
  u[2] = yj[2] - yi[2];
}

template <bool KINDS>
__global__ __launch_bounds__(kBlock) void k_dl_forms(EdgeListDev el, const int* __restrict__ flags, const double* __restrict__ poses,
                                                     const double* __restrict__ bv, const double* __restrict__ gv,
                                                     double* __restrict__ partials) {
  if (flags && flags[0]) return;
  const size_t ns = (size_t)el.E;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < el.E; e += gridDim.x * kBlock) {
    EdgeOperands p;
    edge_operands(el, ns, e, poses, p);
    double sz, cz, er[3];
    sincos(p.zt, &sz, &cz);
    edge_error(p, sz, cz, er);
    EdgeWeight W;
    edge_weight<KINDS>(el, ns, e, er, W);
    EdgeJac J;
    edge_jacobians(p, sz, cz, J);
    const size_t i3 = 3 * (size_t)el.vi[e], j3 = 3 * (size_t)el.vj[e];
    double u[3], v[3];
    dl_jac_apply(J, bv + i3, bv + j3, u);
    dl_jac_apply(J, gv + i3, gv + j3, v);
    const double ou[3] = {(W.o00 * u[0] + W.o01 * u[1]) + W.o02 * u[2], (W.o01 * u[0] + W.o11 * u[1]) + W.o12 * u[2],
                          (W.o02 * u[0] + W.o12 * u[1]) + W.o22 * u[2]};
    const double ov[3] = {(W.o00 * v[0] + W.o01 * v[1]) + W.o02 * v[2], (W.o01 * v[0] + W.o11 * v[1]) + W.o12 * v[2],
                          (W.o02 * v[0] + W.o12 * v[1]) + W.o22 * v[2]};
    acc[0] += W.w * ((u[0] * ou[0] + u[1] * ou[1]) + u[2] * ou[2]);
    acc[1] += W.w * ((v[0] * ou[0] + v[1] * ou[1]) + v[2] * ou[2]);
    acc[2] += W.w * ((v[0] * ov[0] + v[1] * ov[1]) + v[2] * ov[2]);
  }
  block_sum_store<3>(acc, partials, kMaxPartials);
}

__global__ __launch_bounds__(64) void k_dl_prepare(int* __restrict__ flags, int solve_ok, const double* __restrict__ vparts, int nv,
                                                   const double* __restrict__ fparts, int nf, DlState* __restrict__ st) {
  const int f0 = flags ? flags[0] : 0;
  if (f0 == kLmStopWord) return;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int q = threadIdx.x; q < nv; q += 64) s[k] += vparts[(size_t)k * kMaxPartials + q];
    for (int q = threadIdx.x; q < nf; q += 64) s[3 + k] += fparts[(size_t)k * kMaxPartials + q];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = wave_sum(s[k]);
  if (threadIdx.x != 0) return;
  if (flags) {
    solve_ok = solve_ok && f0 == 0 && flags[2] == 0;
    flags[0] = flags[1] = flags[2] = 0;
  }
  solve_ok = solve_ok && s[2] - s[2] == 0.0;   // (a solution that is not finite)
  ++st->solves;
  if (!st->was_pd) st->lambda_used = st->lm.lambda;   // (what this solve added, whether it succeeded or not)
  if (!solve_ok) {
    st->was_pd = 0;
    st->damping *= rules::kDlLambdaFactor;
    if (st->damping > rules::kDlLambdaMax) {
      st->damping = rules::kDlLambdaMax;
      st->lm.stop = 1;
      st->lm.stop_reason = SGO_DL_STOP_DAMPING;
    } else {
      st->lm.lambda = st->damping;
      st->phase = kDlResolve;
    }
    if (flags) flags[0] = kLmStopWord;
    return;
  }
  if (!st->was_pd) {
    st->damping = st->damping / (0.5 * rules::kDlLambdaFactor);
    if (st->damping < rules::kDlLambdaMin) st->damping = rules::kDlLambdaMin;
    st->lm.lambda = st->damping;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) st->forms[k] = s[k];
  st->lm.q = 0;
  st->phase = kDlOpen;
}

__global__ __launch_bounds__(kBlock) void k_dl_trial(const int* __restrict__ gate, int n, const int* __restrict__ row_vertex,
                                                     DlState* __restrict__ st, const double* __restrict__ poses,
                                                     const double* __restrict__ bv, const double* __restrict__ gv,
                                                     double* __restrict__ trial_poses) {
  if (gate && gate[0] == kLmStopWord) return;
  if (st->lm.stop || st->phase != kDlOpen) return;
  double a, c, step_norm, gain;
  const int kind = rules::dogleg_step(st->delta, st->forms, &a, &c, &step_norm, &gain);
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const size_t v = 3 * (size_t)row_vertex[i];
    double h[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) h[q] = kind == rules::kDlGn ? gv[v + q] : a * bv[v + q] + c * gv[v + q];
    trial_poses[v] = poses[v] + h[0];
    trial_poses[v + 1] = poses[v + 1] + h[1];
    trial_poses[v + 2] = norm_theta(poses[v + 2] + h[2]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // (fields no lane of this launch reads)
    st->kind = kind;
    st->step_norm = step_norm;
    st->gain = gain;
  }
}

__global__ __launch_bounds__(64) void k_dl_decide(int* __restrict__ flags, int gated, const double* __restrict__ chi2_trial, int attempt,
                                                  int max_iters, DlState* __restrict__ st) {
  if (threadIdx.x != 0) return;
  if (gated && flags[0] == kLmStopWord) return;
  if (st->lm.stop || st->phase != kDlOpen) return;
  double delta = st->delta;
  const int accepted = rules::dogleg_trial(st->lm.cur, chi2_trial[1], st->gain, st->step_norm, &delta);
  st->delta = delta;
  const int q = ++st->lm.q;
  ++st->lm.trials_total;
  if (accepted) {
    st->lm.cur_plain = chi2_trial[0];
    st->lm.cur = chi2_trial[1];
    st->lm.commit_at = attempt;
  } else if (q < rules::kDlMaxTrials) {
    if (flags) flags[0] = kLmStopWord;   // the iteration stays open: the round's later launches return, the host queues light trials
    return;
  }
  const int it = st->lm.it++;
  st->lm.h_lambda[it] = delta;
  st->lm.h_rob[it + 1] = st->lm.cur;
  st->lm.h_plain[it + 1] = st->lm.cur_plain;
  st->lm.h_trials[it] = q;
  st->h_kind[it] = accepted ? st->kind : -1;
  st->lm.q = 0;
  st->phase = kDlClosed;
  int reason = -1;
  if (!accepted) reason = SGO_DL_STOP_TRIALS;
  else if (it + 1 == max_iters) reason = SGO_DL_STOP_MAX_ITERS;
  if (reason >= 0) {
    st->lm.stop = 1;
    st->lm.stop_reason = reason;
    if (flags) flags[0] = kLmStopWord;
  }
}

__global__ __launch_bounds__(64) void k_dl_resume(int* __restrict__ flags, DlState* __restrict__ st) {
  if (threadIdx.x != 0) return;
  if (st->lm.stop || st->phase == kDlOpen) {
    flags[0] = kLmStopWord;
    return;
  }
  st->phase = kDlClosed;   // (kDlResolve: the next chain is the repeated solve)
  flags[0] = 0;
}

inline int dl_grid(int n) { return std::max(1, std::min((n + kBlock - 1) / kBlock, kMaxPartials)); }

}  // namespace

void launch_dl_begin(hipStream_t s, int* flags, const double* chi2, double delta_init, int max_iters, DlState* st) {
  hipLaunchKernelGGL(k_dl_begin, dim3(1), dim3(64), 0, s, flags, chi2, delta_init, max_iters, st);
}
int launch_dl_vectors_mf(hipStream_t s, const MfDev& M, const LmDiagDev& G, double* bv, double* gv, double* partials) {
  const int grid = dl_grid(M.n);
  hipLaunchKernelGGL(k_dl_vectors_mf, dim3(grid), dim3(kBlock), 0, s, M, G, bv, gv, partials);
  return grid;
}
int launch_dl_vectors_rows(hipStream_t s, int n, const int* free_id, const double* b, const double* x, double* bv, double* gv, double* partials) {
  const int grid = dl_grid(n);
  hipLaunchKernelGGL(k_dl_vectors_rows, dim3(grid), dim3(kBlock), 0, s, n, free_id, b, x, bv, gv, partials);
  return grid;
}
int launch_dl_forms(hipStream_t s, const EdgeListDev& el, const int* flags, const double* poses, const double* bv, const double* gv,
                    double* partials) {
  const int grid = dl_grid(el.E);
  if (el.kinds) hipLaunchKernelGGL(k_dl_forms<true>, dim3(grid), dim3(kBlock), 0, s, el, flags, poses, bv, gv, partials);
  else hipLaunchKernelGGL(k_dl_forms<false>, dim3(grid), dim3(kBlock), 0, s, el, flags, poses, bv, gv, partials);
  return grid;
}
void launch_dl_prepare(hipStream_t s, int* flags, int solve_ok, const double* vparts, int nv, const double* fparts, int nf, DlState* st) {
  hipLaunchKernelGGL(k_dl_prepare, dim3(1), dim3(64), 0, s, flags, solve_ok, vparts, nv, fparts, nf, st);
}
void launch_dl_trial(hipStream_t s, const int* gate, int n, const int* row_vertex, DlState* st, const double* poses, const double* bv,
                     const double* gv, double* trial_poses) {
  hipLaunchKernelGGL(k_dl_trial, dim3(dl_grid(n)), dim3(kBlock), 0, s, gate, n, row_vertex, st, poses, bv, gv, trial_poses);
}
void launch_dl_decide(hipStream_t s, int* flags, bool gated, const double* chi2_trial, int attempt, int max_iters, DlState* st) {
  hipLaunchKernelGGL(k_dl_decide, dim3(1), dim3(64), 0, s, flags, gated && flags ? 1 : 0, chi2_trial, attempt, max_iters, st);
}
void launch_dl_resume(hipStream_t s, int* flags, DlState* st) { hipLaunchKernelGGL(k_dl_resume, dim3(1), dim3(64), 0, s, flags, st); }

}  // namespace sgo
