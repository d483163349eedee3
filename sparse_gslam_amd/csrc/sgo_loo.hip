// sgo_loo.hip -- the kernel behind sgo_edge_leave_one_out (include/sgo.h): for every listed resident edge,
// what sgo_candidate_gate would say about it had it never been inserted, from ONE selected inversion of the factor.
//   k_loo_edges   one lane per listed edge: operands, error, weight and Jacobians (sgo_device.h's layers; the Jacobians as k_mf_edges
//                 forms them), Sigma_ii, Sigma_jj and Sigma_ij straight from the selected inverse's arena through the edge's
//                 descriptor (LooEdgeDev, sgo_mfront_dev.h), P = 1/2 (Q + Q^T) with Q = [A B] Sigma [A B]^T, then the pure rule
//                 rules::edge_loo (sgo_rules.h: the text the host compiles too) and the decision
//   k_loo_count   the workgroups' counts of failing edges, added in a fixed order
// Nothing of Sigma crosses to the host.  No atomics: the count goes through block_sum_store and one ordered final sum.  Vector
// stores only.
// Bounds: the kernel is gather-bound.  An edge reads 21 doubles of Sigma (6 + 6 + 9) at addresses the elimination order scatters
// over the arena -- with 8-byte loads out of column-major fronts that is up to 21 separate 64-byte requests per lane, served by L2
// (the arena has just been written by k_si_panels) --, 15 doubles of its own record in SoA order (coalesced when the ids ascend), and
// two poses; it writes 12 doubles.  The arithmetic (about 500 flops and 8 sweeps of 3 rotations, a dozen divisions and square roots)
// is double-rate-limited only when the gathers hit; one wave per 64 edges leaves most CUs idle below ~16 000 edges, where the
// launch floor is the cost.  Measurements: NOTES.md section 42.
#include <algorithm>

#include "sgo_device.h"
#include "sgo_internal.h"
#include "sgo_mfront_dev.h"
#include "sgo_rules.h"

namespace sgo {
namespace {

// B[a][b] = Sigma(row pose, column pose)[a][b] of the descriptor pr = (front, local row pose, local column pose, transposed), as
// k_si_result reads it: the stored block has the rows of the pose eliminated later
__device__ __forceinline__ void loo_block(const MfDev& M, const MfSelDev& Z, int4 pr, double (&B)[3][3]) {
  const MfFrontDev F = M.fronts[pr.x];
  const double* __restrict__ S = Z.S + F.off;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      int row = 3 * pr.y + (pr.w ? b : a), col = 3 * pr.z + (pr.w ? a : b);
      if (row < col) {   // (a diagonal block: the other triangle is the mirror)
        const int s = row;
        row = col;
        col = s;
      }
      B[a][b] = S[(size_t)col * F.ld + row];
    }
}
// the diagonal block of elimination position p (symmetric: one triangle is stored)
__device__ __forceinline__ void loo_diag(const MfDev& M, const MfSelDev& Z, int p, double (&B)[3][3]) {
  const MfFrontDev F = M.fronts[Z.pos_front[p]];
  const double* __restrict__ S = Z.S + F.off;
  const int l = 3 * (p - F.e0);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) B[a][b] = B[b][a] = S[(size_t)(l + a) * F.ld + l + b];
}

// Q += X S Y^T for 3 x 3 matrices
__device__ __forceinline__ void loo_xsyt(const double (&X)[3][3], const double (&S)[3][3], const double (&Y)[3][3], double (&Q)[3][3]) {
  double XS[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) XS[a][b] = X[a][0] * S[0][b] + X[a][1] * S[1][b] + X[a][2] * S[2][b];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) Q[a][b] += XS[a][0] * Y[b][0] + XS[a][1] * Y[b][1] + XS[a][2] * Y[b][2];
}

template <bool KINDS>
__global__ __launch_bounds__(kBlock) void k_loo_edges(MfDev M, MfSelDev Z, const LooEdgeDev* __restrict__ desc, EdgeListDev el,
                                                      const double* __restrict__ poses, int n, const int* __restrict__ ids, double chi2_max,
                                                      double min_redundancy, double* __restrict__ out, double* __restrict__ partials) {
  const bool failed = desc && M.flags[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) out[(size_t)kLooOut * n] = failed ? (double)M.flags[0] : 0.0;
  const size_t ns = (size_t)el.E;
  double acc[1] = {0.0};
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n && !failed; t += gridDim.x * kBlock) {
    const int k = ids ? ids[t] : t;
    EdgeOperands p;
    edge_operands(el, ns, k, poses, p);
    double sz, cz, e[3];
    sincos(p.zt, &sz, &cz);
    edge_error(p, sz, cz, e);
    EdgeWeight Wt;
    edge_weight<KINDS>(el, ns, k, e, Wt);
    // the Jacobians as k_mf_edges forms them
    double si, ci;
    sincos(p.ti, &si, &ci);
    const double ddx = p.xj - p.xi, ddy = p.yj - p.yi;
    const double a02 = -si * ddx + ci * ddy, a12 = -ci * ddx - si * ddy;
    const double A[3][3] = {{cz * (-ci) - sz * si, cz * (-si) - sz * (-ci), cz * a02 - sz * a12},
                            {sz * (-ci) + cz * si, sz * (-si) + cz * (-ci), sz * a02 + cz * a12},
                            {0.0, 0.0, -1.0}};
    const double B[3][3] = {{cz * ci - sz * (-si), cz * si - sz * ci, 0.0}, {sz * ci + cz * (-si), sz * si + cz * ci, 0.0}, {0.0, 0.0, 1.0}};
    // Q = A Sii A^T + A Sij B^T + B Sij^T A^T + B Sjj B^T; a fixed endpoint drops out
    double Q[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (desc) {
      const LooEdgeDev d = desc[k];
      double S[3][3];
      if (d.pi >= 0) {
        loo_diag(M, Z, d.pi, S);
        loo_xsyt(A, S, A, Q);
      }
      if (d.pj >= 0) {
        loo_diag(M, Z, d.pj, S);
        loo_xsyt(B, S, B, Q);
      }
      if (d.pair.x >= 0) {
        loo_block(M, Z, d.pair, S);
        double St[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) St[a][b] = S[b][a];
        loo_xsyt(A, S, B, Q);
        loo_xsyt(B, St, A, Q);
      }
    }
    double P[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) P[3 * a + b] = 0.5 * (Q[a][b] + Q[b][a]);
    const double info[6] = {Wt.o00, Wt.o01, Wt.o02, Wt.o11, Wt.o12, Wt.o22};
    double d2, red, cov[9];
    rules::edge_loo(info, P, e, Wt.w, &d2, &red, cov);
    // a bridge's test is 0 / 0: below min_redundancy (or not finite) nothing is decided
    if (!(red >= min_redundancy)) {
      const double nan = __builtin_nan("");
      d2 = nan;
#pragma unroll
      for (int q = 0; q < 9; ++q) cov[q] = nan;
    }
    const bool fail = red >= min_redundancy && d2 > chi2_max;
    double* o = out + (size_t)kLooOut * t;
    o[0] = d2;
    o[1] = red;
#pragma unroll
    for (int q = 0; q < 9; ++q) o[2 + q] = cov[q];
    o[11] = fail ? 1.0 : 0.0;
    acc[0] += fail ? 1.0 : 0.0;
  }
  block_sum_store<1>(acc, partials, kMaxPartials);
}

__global__ __launch_bounds__(kBlock) void k_loo_count(const double* __restrict__ partials, int nparts, double* __restrict__ count) {
  const double s = block_reduce_parts(partials, nparts);   // (whole numbers below 2^31: exact)
  if (threadIdx.x == 0) *count = s;
}

}  // namespace

void launch_loo_edges(hipStream_t s, const MfDev& M, const MfSelDev& Z, const LooEdgeDev* desc, const EdgeListDev& el, const double* poses, int n,
                      const int* ids, double chi2_max, double min_redundancy, double* out, double* partials) {
  const int grid = grid_for(n, kBlock);
  if (el.kinds) SGO_LAUNCH(k_loo_edges<true>, dim3(grid), dim3(kBlock), 0, s, M, Z, desc, el, poses, n, ids, chi2_max, min_redundancy, out, partials);
  else SGO_LAUNCH(k_loo_edges<false>, dim3(grid), dim3(kBlock), 0, s, M, Z, desc, el, poses, n, ids, chi2_max, min_redundancy, out, partials);
  hipLaunchKernelGGL(k_loo_count, dim3(1), dim3(kBlock), 0, s, (const double*)partials, grid, out + (size_t)kLooOut * n + 1);
}

}  // namespace sgo
