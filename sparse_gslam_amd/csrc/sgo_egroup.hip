// sgo_egroup.hip -- the kernels behind sgo_edge_joint and sgo_edge_groups (include/sgo.h): the leave-group-out
// test of clusters of RESIDENT edges -- what the joint test would say about a cluster had it never been inserted.
//   k_edge_cands    one thread per listed edge: the edge as a candidate's record source (endpoints, rows of its poses, inverse
//                   measurement and information copied out of the resident edge list on the device) and its kernel weight from
//                   edge_weight<KINDS>.  From here on the columns H^-1 J^T and their Gram blocks are sgo_candidate_joint's
//                   (k_fs_rhs, the factor substitution or the PCG route, k_fs_gram: sgo_fsolve.hip)
//   k_edge_table    N = (G + G^T) / 2, one triangle computed and mirrored (no Omega^-1 on the diagonal: the rule adds the
//                   information itself), then e, w, Omega's upper triangle per edge and the factorisation's failure flag
//   k_edge_groups   one workgroup per group: the member row compacted by ballot and prefix count as k_joint_subsets does it (a member
//                   with all-zero information is left out), then rules::edge_group (sgo_rules.h: the text the host compiles too) as
//                   16 x 16 workers over two packed lower triangles in LDS: G_t and Nt = G^T N G blockwise, the pivots of
//                   I - T Nt T, K with its Nt D (I - D) Nt product, the Cholesky of K that carries c along; then the decision
// No atomics; every sum has a fixed ascending order; an element of a stage is one thread's.  Vector stores only.
// Bounds: a group of k members (m = 3 k) reads 9 k^2 / 2 + 10 k doubles of the table (gathered 3 x 3 blocks out of L2: 24-byte runs)
// and holds m (m + 1) + m doubles of LDS (118 KB at k = 40: one workgroup per CU there, five at k = 8).  The two factorisations are
// 2 m barrier-separated steps of a shrinking trailing update -- latency-bound for small groups (m steps of about one LDS round
// trip), m^3 / 3 multiply-adds over 256 threads for large ones; the K product adds m^3 / 2 where some 0 < w < 1.  Measurements:
// NOTES.md section 44.
#include <algorithm>

#include "sgo_device.h"
#include "sgo_internal.h"
#include "sgo_mfront_dev.h"
#include "sgo_rules.h"

namespace sgo {
namespace {

template <bool KINDS>
__global__ __launch_bounds__(kBlock) void k_edge_cands(int n, EdgeListDev el, const int* __restrict__ ids, const int* __restrict__ vrow,
                                                       const double* __restrict__ poses, int* __restrict__ vi, int* __restrict__ vj,
                                                       int* __restrict__ row, double* __restrict__ zinv, double* __restrict__ info,
                                                       double* __restrict__ w) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const int k = ids[t];
  const size_t ns = (size_t)el.E, nd = (size_t)n;
  const int a = el.vi[k], b = el.vj[k];
  vi[t] = a;
  vj[t] = b;
  row[2 * t] = vrow[a];
  row[2 * t + 1] = vrow[b];
#pragma unroll
  for (int q = 0; q < 3; ++q) zinv[q * nd + t] = el.zinv[q * ns + k];
#pragma unroll
  for (int q = 0; q < 6; ++q) info[q * nd + t] = el.info[q * ns + k];
  EdgeOperands p;
  edge_operands(el, ns, k, poses, p);
  double sz, cz, e[3];
  sincos(p.zt, &sz, &cz);
  edge_error(p, sz, cz, e);
  EdgeWeight Wt;
  edge_weight<KINDS>(el, ns, k, e, Wt);
  w[t] = Wt.w;
}

// One thread per block pair s <= t: N_st = (G_st + G_ts^T) / 2, stored at both places (N is exactly symmetric); the diagonal block's
// thread stores the edge's e, w and Omega; then the factorisation's failure flag
__global__ __launch_bounds__(kBlock) void k_edge_table(FsCandDev C, const double* __restrict__ w, const double* __restrict__ G,
                                                       const int* __restrict__ flags, double* __restrict__ table) {
  const int n = C.n;
  const int s = blockIdx.x * kBlock + threadIdx.x, t = blockIdx.y;
  const size_t ld = 3 * (size_t)n, ns = (size_t)n;
  double* __restrict__ ev = table + ld * ld;
  double* __restrict__ wv = ev + ld;
  double* __restrict__ ov = wv + ns;
  if (s == 0 && t == 0) ov[6 * ns] = flags ? (double)flags[0] : 0.0;
  if (s > t || t >= n) return;
  double P[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) P[a][b] = 0.5 * (G[(3 * (size_t)s + a) * ld + 3 * (size_t)t + b] + G[(3 * (size_t)t + b) * ld + 3 * (size_t)s + a]);
  if (s == t) {
    // (the lower triangle's values, mirrored: the diagonal block is symmetric bit for bit)
    P[0][1] = P[1][0];
    P[0][2] = P[2][0];
    P[1][2] = P[2][1];
    const double* rec = C.rec + (size_t)kFsRec * t;
    ev[3 * (size_t)t] = rec[0];
    ev[3 * (size_t)t + 1] = rec[1];
    ev[3 * (size_t)t + 2] = rec[2];
    wv[t] = w[t];
#pragma unroll
    for (int q = 0; q < 6; ++q) ov[6 * (size_t)t + q] = C.info[q * ns + t];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      table[(3 * (size_t)s + a) * ld + 3 * (size_t)t + b] = P[a][b];
      table[(3 * (size_t)t + b) * ld + 3 * (size_t)s + a] = P[a][b];
    }
}

struct WorkgroupSync {
  __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

// out: [groups][kEgOut] = d2, pivot, dof, the decision.  A group's arithmetic depends on the table and its member row alone: the
// packed triangles have no leading dimension, so neither the launch's LDS size nor the group's place in the grid moves anything.
__global__ __launch_bounds__(kJointThreads) void k_edge_groups(const double* __restrict__ table, int n, const uint8_t* __restrict__ mask,
                                                               const double* __restrict__ chi2_max, double min_pivot, int kmax,
                                                               double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double eg_ws[];   // rules::edge_group_ws_doubles(kmax)
  __shared__ int idx[SGO_JOINT_MAX_SUBSET];
  __shared__ int wcnt[kJointThreads / 64];
  __shared__ double res[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t b = blockIdx.x;
  const size_t ld = 3 * (size_t)n;
  const double* __restrict__ ev = table + ld * ld;
  const double* __restrict__ wv = ev + ld;
  const double* __restrict__ ov = wv + n;
  bool on = tid < n && mask[b * n + tid] != 0;
  if (on) {   // a member with all-zero information is no member
    const double* o = ov + 6 * (size_t)tid;
    on = !(o[0] == 0.0 && o[1] == 0.0 && o[2] == 0.0 && o[3] == 0.0 && o[4] == 0.0 && o[5] == 0.0);
  }
  const unsigned long long bal = __ballot(on);
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int base = 0, cnt = 0;
#pragma unroll
  for (int q = 0; q < kJointThreads / 64; ++q) {
    if (q < wave) base += wcnt[q];
    cnt += wcnt[q];
  }
  const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
  if (on && pos < SGO_JOINT_MAX_SUBSET) idx[pos] = tid;
  double* o = out + (size_t)kEgOut * b;
  if (cnt > SGO_JOINT_MAX_SUBSET || cnt > kmax) {   // (the driver refuses such a group before the launch)
    if (tid == 0) {
      o[0] = o[1] = __builtin_nan("");
      o[2] = 3.0 * cnt;
      o[3] = 0.0;
    }
    return;
  }
  __syncthreads();
  rules::edge_group(cnt, idx, table, ld, ev, wv, ov, eg_ws, tid >> 4, tid & 15, 16, WorkgroupSync(), &res[0], &res[1]);
  if (tid == 0) {
    double d2 = res[0];
    const double pivot = res[1];
    const bool decided = pivot >= min_pivot;   // (a bridge cluster's test is 0 / 0; not finite: nothing is decided either)
    if (!decided) d2 = __builtin_nan("");
    o[0] = d2;
    o[1] = pivot;
    o[2] = 3.0 * cnt;
    o[3] = (decided && chi2_max && d2 > chi2_max[b]) ? 1.0 : 0.0;
  }
}

}  // namespace

void launch_edge_cands(hipStream_t s, const FsCandDev& C, const EdgeListDev& el, const int* ids, const int* vrow, const double* poses, int* vi, int* vj,
                       int* row, double* zinv, double* info, double* w) {
  const dim3 grid((C.n + kBlock - 1) / kBlock);
  if (el.kinds) SGO_LAUNCH(k_edge_cands<true>, grid, dim3(kBlock), 0, s, C.n, el, ids, vrow, poses, vi, vj, row, zinv, info, w);
  else SGO_LAUNCH(k_edge_cands<false>, grid, dim3(kBlock), 0, s, C.n, el, ids, vrow, poses, vi, vj, row, zinv, info, w);
}
void launch_edge_table(hipStream_t s, const FsCandDev& C, const double* w, const double* G, const int* flags, double* table) {
  SGO_LAUNCH(k_edge_table, dim3((C.n + kBlock - 1) / kBlock, C.n), dim3(kBlock), 0, s, C, w, G, flags, table);
}
void launch_edge_groups(hipStream_t s, const double* table, int n, const uint8_t* mask, const double* chi2_max, double min_pivot, int count, int kmax,
                        double* out) {
  const size_t lds = sizeof(double) * rules::edge_group_ws_doubles(std::max(kmax, 1));
  SGO_LAUNCH(k_edge_groups, dim3(count), dim3(kJointThreads), lds, s, table, n, mask, chi2_max, min_pivot, kmax, out);
}
bool edge_groups_prepare_device() {
  const int lds = (int)(sizeof(double) * rules::edge_group_ws_doubles(SGO_JOINT_MAX_SUBSET));
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_edge_groups), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

}  // namespace sgo
