// sgo_marginals.hip -- the kernels behind sgo_marginals / sgo_solve_rhs (include/sgo.h): blocks of H^-1 as columns solved with the
// resident level-0 PCG machinery.  The solve reads its right-hand side from the `b` slots of the linearisation's dgb records
// ([n][9]: the diagonal block's upper triangle, then b; k_finalize makes the start state from them), so a column is solved by
// putting another right-hand side there and keeping the linearisation's own aside:
//   k_rhs_inject    dgb's b := a unit column or the caller's vector (internal row order); the first injection of a call saves b
//   k_rhs_restore   dgb's b := what was saved
//   k_cov_gather    after the solve of unit column k of one column vertex: the rows of d_x that the listed pairs ask for into
//                   column k of their 3x3 result blocks; with the third column a diagonal pair's block becomes (S + S^T) / 2
// Streaming kernels, one lane per row or per pair, vector stores only, no atomics: every output has one writer.
#include "sgo_internal.h"

namespace sgo {
namespace {

// save (optional, [n][3]) receives the b the records hold; src (optional, [n][3], internal row order) is the new right-hand side,
// without it e_{3 unit_row + unit_k}
__global__ __launch_bounds__(kBlock) void k_rhs_inject(int n, double* __restrict__ dgb, double* __restrict__ save,
                                                       const double* __restrict__ src, int unit_row, int unit_k) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    double* b = dgb + 9 * (size_t)i + 6;
    const size_t o = 3 * (size_t)i;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (save) save[o + q] = b[q];
      b[q] = src ? src[o + q] : (i == unit_row && q == unit_k ? 1.0 : 0.0);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_rhs_restore(int n, double* __restrict__ dgb, const double* __restrict__ save) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    double* b = dgb + 9 * (size_t)i + 6;
#pragma unroll
    for (int q = 0; q < 3; ++q) b[q] = save[3 * (size_t)i + q];
  }
}

// Items [q0, q1) of `order` are the pairs of one column vertex (internal row col_row); pair t wants the rows of internal row
// pair_row[t] (>= 0: the host lists no pair with a fixed vertex).  x = H^-1 e_{3 col_row + k}: cov[t][a][k] = x[3 pair_row[t] + a].
// With k == 2 the block is complete (columns 0 and 1 were stored by the launches before, in stream order, by this pair's lane).
__global__ __launch_bounds__(kBlock) void k_cov_gather(int q0, int q1, const int* __restrict__ order, const int* __restrict__ pair_row,
                                                       int col_row, int k, int n, const double* __restrict__ x, double* __restrict__ cov) {
  for (int q = q0 + blockIdx.x * kBlock + threadIdx.x; q < q1; q += gridDim.x * kBlock) {
    const int t = order[q], row = pair_row[t];
    if (row < 0 || row >= n) continue;
    double* S = cov + 9 * (size_t)t;
#pragma unroll
    for (int a = 0; a < 3; ++a) S[3 * a + k] = x[3 * (size_t)row + a];
    if (k == 2 && row == col_row) {
      const double s01 = 0.5 * (S[1] + S[3]), s02 = 0.5 * (S[2] + S[6]), s12 = 0.5 * (S[5] + S[7]);
      S[1] = S[3] = s01;
      S[2] = S[6] = s02;
      S[5] = S[7] = s12;
    }
  }
}

}  // namespace

void launch_rhs_inject(hipStream_t s, int n, double* dgb, double* save, const double* src, int unit_row, int unit_k) {
  SGO_LAUNCH(k_rhs_inject, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, n, dgb, save, src, unit_row, unit_k);
}
void launch_rhs_restore(hipStream_t s, int n, double* dgb, const double* save) {
  SGO_LAUNCH(k_rhs_restore, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, n, dgb, save);
}
void launch_cov_gather(hipStream_t s, int q0, int q1, const int* order, const int* pair_row, int col_row, int k, int n, const double* x,
                       double* cov) {
  SGO_LAUNCH(k_cov_gather, dim3(grid_for(q1 - q0, kBlock)), dim3(kBlock), 0, s, q0, q1, order, pair_row, col_row, k, n, x, cov);
}

}  // namespace sgo
