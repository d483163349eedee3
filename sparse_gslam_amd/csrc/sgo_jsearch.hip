// sgo_jsearch.hip -- the kernel behind sgo_joint_greedy / sgo_joint_extend (include/sgo.h): greedy growth of
// a jointly compatible candidate set on the resident table of sgo_candidate_joint, with no from-scratch factorisation.
//   k_joint_grow   one workgroup per seed, thread c owns candidate c.  The ordered pivots t_1 .. t_k are the steps of a
//                  block-pivoted Cholesky of S: every candidate that is not a pivot keeps its partly eliminated block
//                  C_c = S_cc - W_c^T W_c and q_c = e_c - W_c^T z in registers, its W_c (3 k x 3) in a per-workgroup slab of global
//                  scratch laid out [row][3 n], so that the lanes' 24-byte reads of one row are contiguous.
// One step with pivot p: thread p takes G = chol(C_p), z+ = G^-1 q_p and puts them into LDS while all threads copy W_p's three
// columns there; after the barrier every other candidate reads W_p and G as broadcasts, forms R = S_pc - W_p^T W_c against its own
// columns, w = G^-1 R, C_c -= w^T w, q_c -= w^T z+ and appends w to its columns (rules::jgrow_update, sgo_rules.h: the text the
// host compiles for sgo_joint_greedy_rule).  The forced pivots of the seed and the chosen ones are iterations of ONE loop and run
// the same instructions: sgo_joint_extend on a returned order repeats sgo_joint_greedy's bits.
// A free step chooses the smallest v_c = d2 + q_c^T C_c^-1 q_c among the candidates that are allowed, finite and at most
// chi2_max[k + 1], ties to the lower c: a butterfly over the wave's lanes on the pair (v, c), then thread 0 over the four waves'
// pairs in LDS.  The order on pairs is total and exact, so the result does not depend on the reduction's shape.  No atomics.
// A workgroup's slab is its own: a column of W is written by its candidate's thread and read back by that thread, except the
// pivot's columns, which all threads read after a barrier (workgroup scope).  Vector stores only.
// Bounds: a step costs a thread 9 m multiply-adds and m 24-byte loads for m rows so far, the whole path of k pivots 13.5 k^2 n
// multiply-adds per seed: 5.5 Mflop at the caps (n = 256, k = 40), against 40 steps x 216 candidates x (3 k)^3 / 3 for the
// from-scratch route.  The chain is latency-bound: k steps, each a barrier, a 3 x 3 Cholesky of one thread and a row loop whose
// loads rules::jgrow_update issues six rows at a time.
// Measurements: NOTES.md section 43.
#include <algorithm>

#include "sgo_internal.h"
#include "sgo_mfront_dev.h"
#include "sgo_rules.h"

namespace sgo {
namespace {

__global__ __launch_bounds__(kJointThreads) void k_joint_grow(JointGrowDev A) {
  __shared__ double Wp[3 * SGO_JOINT_MAX_SUBSET][3];   // the pivot's columns
  __shared__ double Gz[9];                             // its factor G6, then z+
  __shared__ double wv[kJointThreads / 64];            // the waves' best pairs
  __shared__ int wc[kJointThreads / 64];
  __shared__ int pick[2];                              // the chosen candidate (-1: none); the pivot's block is not positive definite
  const int c = threadIdx.x, lane = c & 63, wave = c >> 6, n = A.n;
  const size_t b = (size_t)A.b0 + blockIdx.x, ld = 3 * (size_t)n;
  const bool live = c < n;
  const double* __restrict__ S = A.table;
  const double* __restrict__ ev = A.table + ld * ld;
  double* __restrict__ W = A.slabs + (size_t)blockIdx.x * A.slab;   // [3 max_len][3 n]
  const int* __restrict__ seed = A.seed + b * SGO_JOINT_MAX_SUBSET;
  int* __restrict__ order = A.order + b * SGO_JOINT_MAX_SUBSET;
  double* __restrict__ path = A.d2_path + b * (SGO_JOINT_MAX_SUBSET + 1);
  const double nan = __builtin_nan("");
  const bool allowed = live && (!A.allow || A.allow[b * n + c] != 0);

  double C6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
  if (live) {
    const double* __restrict__ r = S + 3 * (size_t)c * ld + 3 * (size_t)c;
    C6[0] = r[0], C6[1] = r[ld], C6[2] = r[ld + 1], C6[3] = r[2 * ld], C6[4] = r[2 * ld + 1], C6[5] = r[2 * ld + 2];
    q[0] = ev[3 * c], q[1] = ev[3 * c + 1], q[2] = ev[3 * c + 2];
  }
  bool pivot = false;
  double d2 = 0.0;
  int k = 0, stop = SGO_JSTOP_MAX_LEN;
  if (c == 0) path[0] = 0.0;
  for (; k < A.max_len; ++k) {
    const int m = 3 * k;
    int p = seed[k];   // (-1 behind the seed)
    if (p < 0) {
      // a free step: the smallest eligible extension value, ties to the lower candidate
      double v = __builtin_inf();
      int vc = 0x7fffffff;
      if (allowed && !pivot && A.chi2) {
        const double t = rules::jgrow_value(d2, C6, q);
        if (t - t == 0.0 && t <= A.chi2[k + 1]) {
          v = t;
          vc = c;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oc = __shfl_xor(vc, off);
        if (rules::jgrow_better(ov, oc, v, vc)) {
          v = ov;
          vc = oc;
        }
      }
      if (lane == 0) {
        wv[wave] = v;
        wc[wave] = vc;
      }
      __syncthreads();
      if (c == 0) {
#pragma unroll
        for (int w = 1; w < kJointThreads / 64; ++w)
          if (rules::jgrow_better(wv[w], wc[w], v, vc)) {
            v = wv[w];
            vc = wc[w];
          }
        pick[0] = vc == 0x7fffffff ? -1 : vc;
      }
      __syncthreads();
      p = pick[0];
      if (p < 0) {
        stop = SGO_JSTOP_NONE;
        break;
      }
    }
    // the pivot's factor and its columns into LDS
    if (c == p) {
      double G6[6], zp[3] = {0.0, 0.0, 0.0};
      const bool ok = rules::jgrow_chol3(C6, G6);
      if (ok) rules::jgrow_solve3(G6, q[0], q[1], q[2], zp);
#pragma unroll
      for (int t = 0; t < 6; ++t) Gz[t] = G6[t];
#pragma unroll
      for (int t = 0; t < 3; ++t) Gz[6 + t] = zp[t];
      pick[1] = ok ? 0 : 1;
    }
    for (int i = c; i < 3 * m; i += kJointThreads) Wp[i / 3][i % 3] = W[(size_t)(i / 3) * ld + 3 * (size_t)p + i % 3];
    __syncthreads();
    if (pick[1]) {   // (only a seed's pivot: a free one had a finite value through the same factor)
      stop = SGO_JSTOP_NOT_PD;
      break;
    }
    double G6[6], zp[3];
#pragma unroll
    for (int t = 0; t < 6; ++t) G6[t] = Gz[t];
#pragma unroll
    for (int t = 0; t < 3; ++t) zp[t] = Gz[6 + t];
    if (c == p) pivot = true;
    if (live && !pivot) rules::jgrow_update(G6, zp, S + 3 * (size_t)p * ld + 3 * (size_t)c, ld, &Wp[0][0], 3, W + 3 * (size_t)c, ld, m, C6, q);
    d2 += (zp[0] * zp[0] + zp[1] * zp[1]) + zp[2] * zp[2];
    if (c == 0) {
      order[k] = p;
      path[k + 1] = d2;
    }
    __syncthreads();   // (Wp, Gz and pick are rewritten by the next step; the appended rows are the workgroup's to read)
  }
  // k pivots done.  A seed that failed leaves NaN from there on.
  const bool failed = stop == SGO_JSTOP_NOT_PD;
  if (c == 0) {
    A.count[b] = k;
    A.stop[b] = stop;
  }
  for (int t = k + c; t < SGO_JOINT_MAX_SUBSET; t += kJointThreads) {
    order[t] = -1;
    path[t + 1] = nan;
  }
  if (live) A.d2_ext[b * n + c] = failed ? nan : pivot ? d2 : rules::jgrow_value(d2, C6, q);
}

}  // namespace

void launch_joint_grow(hipStream_t s, const JointGrowDev& A, int count) {
  SGO_LAUNCH(k_joint_grow, dim3(count), dim3(kJointThreads), 0, s, A);
}

}  // namespace sgo
