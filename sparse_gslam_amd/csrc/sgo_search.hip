// sgo_search.hip -- the kernels behind sgo_closure_search (include/sgo.h): for a chunk of query poses c and
// every listed pose j, whether c can be excluded from lying within `radius` of j once the covariance of their relative pose is taken
// into account, from ONE selected inversion (Sigma_jj, Sigma_cc in place) and one panel solve (Sigma_jc = rows of H^-1 E_c).
//   k_cs_unit          the unit columns of the chunk's free queries at their elimination positions, into the zeroed panel
//   k_closure_search   one lane per listed vertex j: pose j and Sigma_jj ONCE (the diagonal block straight from the selected inverse's
//                      arena through pos_front, 6 doubles), then a loop over the chunk's queries, whose poses, Sigma_cc, positions
//                      and columns the workgroup has staged in LDS; Sigma_jc is three runs of three contiguous doubles of the
//                      query's three columns of X; the pair rule rules::closure_search (sgo_rules.h: the text the host compiles
//                      too), the decision, and stores in field-major order [field][query][listed vertex], which coalesce
//   k_cs_count         the workgroups' counts of near pairs, added in a fixed order
// Nothing of Sigma crosses to the host.  No atomics: the count goes through block_sum_store and one ordered final sum.  Vector
// stores only.
// Bounds (REASONING, not measurement; measurements: NOTES.md section 48).  Per listed vertex the kernel reads 24 bytes of pose, 8
// of indices and the 6 doubles of Sigma_jj at addresses the elimination order scatters over the arena (up to 6 separate 64-byte
// requests per lane, served by L2: k_si_panels has just written the arena) -- the expensive access, paid once, not per query.  Per PAIR
// it reads 72 bytes of X (rows 3 p_j .. 3 p_j + 2 of three columns: neighbouring lanes hit neighbouring rows only where the ids'
// elimination positions are neighbours, so this too is a gather, of 24-byte runs, out of a panel the backward pass has just
// written) and writes 13 doubles coalesced; the query's 80 bytes come from LDS as a broadcast.  The arithmetic is about 250 flops,
// two square roots and two divisions per pair after one sincos per listed vertex.  With one wave per 64 listed vertices most CUs are
// idle below ~16 000 listed vertices (DESIGN.md section 5k's argument for k_loo_edges), where the launch floor is the cost; a chunk of
// many queries lengthens each lane's loop and not the grid.
#include <algorithm>

#include "sgo_device.h"
#include "sgo_internal.h"
#include "sgo_mfront_dev.h"
#include "sgo_rules.h"

namespace sgo {
namespace {

// the diagonal block of elimination position p, row-major (symmetric: one triangle is stored), as loo_diag of sgo_loo.hip reads it
__device__ __forceinline__ void cs_diag(const MfDev& M, const MfSelDev& Z, int p, double* B) {
  const MfFrontDev F = M.fronts[Z.pos_front[p]];
  const double* __restrict__ S = Z.S + F.off;
  const int l = 3 * (p - F.e0);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) B[3 * a + b] = B[3 * b + a] = S[(size_t)(l + a) * F.ld + l + b];
}

__global__ __launch_bounds__(kBlock) void k_cs_unit(int cq, const CsQueryDev* __restrict__ queries, int n3, double* __restrict__ panel) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= 3 * cq) return;
  const CsQueryDev q = queries[i / 3];
  const int b = i % 3;
  if (q.z >= 0) panel[(size_t)(q.z + b) * n3 + 3 * (size_t)q.y + b] = 1.0;
}

__global__ __launch_bounds__(kBlock) void k_closure_search(MfDev M, MfSelDev Z, bool factor, const int* __restrict__ vpos,
                                                           const double* __restrict__ poses, int n, const int* __restrict__ ids, int cq,
                                                           const CsQueryDev* __restrict__ queries, const double* __restrict__ X, int n3, double radius,
                                                           double chi2_max, int min_sep, double* __restrict__ out, double* __restrict__ partials) {
  __shared__ double q_pose[kCsChunkQueries][3];
  __shared__ double q_cov[kCsChunkQueries][9];
  __shared__ CsQueryDev q_desc[kCsChunkQueries];
  const bool failed = factor && M.flags[0];
  const size_t plane = (size_t)cq * n;   // one field of the chunk
  if (blockIdx.x == 0 && threadIdx.x == 0) out[(size_t)kCsOut * plane] = failed ? (double)M.flags[0] : 0.0;
  if (!failed)
    for (int q = threadIdx.x; q < cq; q += kBlock) {
      const CsQueryDev d = queries[q];
      q_desc[q] = d;
#pragma unroll
      for (int a = 0; a < 3; ++a) q_pose[q][a] = poses[3 * (size_t)d.x + a];
      if (d.y >= 0) cs_diag(M, Z, d.y, q_cov[q]);
    }
  __syncthreads();
  double acc[1] = {0.0};
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n && !failed; t += gridDim.x * kBlock) {
    const int j = ids ? ids[t] : t;
    const int pj = vpos[j];
    const double xj[3] = {poses[3 * (size_t)j], poses[3 * (size_t)j + 1], poses[3 * (size_t)j + 2]};
    double Sjj[9];
    if (pj >= 0) cs_diag(M, Z, pj, Sjj);
    for (int q = 0; q < cq; ++q) {
      const CsQueryDev d = q_desc[q];
      double m2, rel[3], P[9], sg[2];
      if (pj == -2) {   // a vertex without an edge (only without ids): nothing is known about it
        const double nan = __builtin_nan("");
        m2 = rel[0] = rel[1] = rel[2] = sg[0] = sg[1] = nan;
#pragma unroll
        for (int e = 0; e < 9; ++e) P[e] = nan;
      } else if (j == d.x) {   // the query itself: exact zeros, not the rounding of A = -B
        m2 = rel[0] = rel[1] = rel[2] = sg[0] = sg[1] = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) P[e] = 0.0;
      } else {
        const double xc[3] = {q_pose[q][0], q_pose[q][1], q_pose[q][2]};
        double Scc[9], Sjc[9];
        const bool fj = pj >= 0, fc = d.y >= 0;
        if (fc)
#pragma unroll
          for (int e = 0; e < 9; ++e) Scc[e] = q_cov[q][e];
        if (fj && fc)   // Sigma_jc[a][b]: row 3 p_j + a of the query's column b
#pragma unroll
          for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int a = 0; a < 3; ++a) Sjc[3 * a + b] = X[(size_t)(d.z + b) * n3 + 3 * (size_t)pj + a];
        rules::closure_search(xj, xc, fj, fc, Sjj, Sjc, Scc, radius, rel, P, &m2, sg);
      }
      const int sep = j > d.x ? j - d.x : d.x - j;
      const bool near = m2 <= chi2_max && j != d.x && sep >= min_sep;
      double* o = out + (size_t)q * n + t;
      o[0] = m2;
      o[plane] = rel[0]; o[2 * plane] = rel[1]; o[3 * plane] = rel[2];
      o[4 * plane] = P[0]; o[5 * plane] = P[1]; o[6 * plane] = P[2]; o[7 * plane] = P[4]; o[8 * plane] = P[5]; o[9 * plane] = P[8];
      o[10 * plane] = sg[0]; o[11 * plane] = sg[1];
      o[12 * plane] = near ? 1.0 : 0.0;
      acc[0] += near ? 1.0 : 0.0;
    }
  }
  block_sum_store<1>(acc, partials, kMaxPartials);
}

__global__ __launch_bounds__(kBlock) void k_cs_count(const double* __restrict__ partials, int nparts, double* __restrict__ count) {
  const double s = block_reduce_parts(partials, nparts);   // (whole numbers below 2^53: exact)
  if (threadIdx.x == 0) *count = s;
}

}  // namespace

void launch_cs_unit(hipStream_t s, int cq, const CsQueryDev* queries, int n3, double* panel) {
  SGO_LAUNCH(k_cs_unit, dim3((3 * cq + kBlock - 1) / kBlock), dim3(kBlock), 0, s, cq, queries, n3, panel);
}

void launch_closure_search(hipStream_t s, const MfDev& M, const MfSelDev& Z, bool factor, const int* vpos, const double* poses, int n, const int* ids,
                           int cq, const CsQueryDev* queries, const double* X, int n3, double radius, double chi2_max, int min_sep, double* out,
                           double* partials) {
  const int grid = grid_for(n, kBlock);
  SGO_LAUNCH(k_closure_search, dim3(grid), dim3(kBlock), 0, s, M, Z, factor, vpos, poses, n, ids, cq, queries, X, n3, radius, chi2_max, min_sep, out,
             partials);
  hipLaunchKernelGGL(k_cs_count, dim3(1), dim3(kBlock), 0, s, (const double*)partials, grid, out + (size_t)kCsOut * cq * n + 1);
}

}  // namespace sgo
