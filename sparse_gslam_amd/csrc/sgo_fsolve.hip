// sgo_fsolve.hip -- forward and backward substitution through the resident multifrontal factor for panels of 16 right-hand sides
// (sgo_factor_solve, sgo_candidate_gate of include/sgo.h; driver in sgo_fsolve.cpp).  The factorisation
// (sgo_mfront.hip) leaves L11 over L21 of every front in ARENA and the explicit inverses of the 16 x 16 diagonal blocks' factors in
// YINV; nothing else is needed:
//   k_fs_rhs       the right-hand-side panel [columns][3 n] by elimination position: the caller's columns permuted from the hessian
//                  order, or, per candidate edge, e, A, B from the one statement of the edge arithmetic (sgo_device.h) and A^T / B^T
//                  at the rows of its two poses
//   k_fs_forward   one launch per level, bottom-up, grid (fronts of the level) x (panels): t = the front's own rows of the panel plus
//                  its children's boundary updates (extend-add map, child 0 before child 1), then per block J of 16 own columns,
//                  ascending: y_J = L_JJ^-1 t_J (YINV), t_R -= L_RJ y_J for every row R after J.  y goes to the panel, the boundary
//                  rows to the front's update buffer [3 nb][16].  (k_mf_panels carries ONE right-hand side as row m of the front.)
//   k_fs_backward  one launch per level, top-down: x_J = L_JJ^-T (y_J - L_RJ^T x_R), the boundary rows of x read by bnd as k_mf_solve
//                  does; the contraction over R is split over the eight waves in fixed shares and added in wave order
//   k_fs_gate      per candidate: Q = R^T W from at most six rows of W, P = (Q + Q^T) / 2, S = Omega^-1 + P (cofactors),
//                  d2 = e^T S^-1 e by a 3 x 3 Cholesky; d2, P, the decision and the factorisation's failure flag in one buffer
// and the joint table of a candidate SET (sgo_candidate_joint / sgo_joint_subsets / sgo_joint_pairs):
//   k_fs_gram         per chunk of columns: G_st = [A_s B_s] W_t[rows of i_s, j_s] for ALL candidates s against the chunk's t
//   k_fs_joint_table  S = blockdiag(Omega^-1) + (G + G^T) / 2, one triangle computed and mirrored; e; the failure flag
//   k_joint_subsets   one workgroup per subset of the resident table: d2 = e_s^T (S_ss)^-1 e_s by a Cholesky in LDS
// All products run on the fp64 matrix cores (v_mfma_f64_16x16x4_f64: lane (lr, lk) = (lane & 15, lane >> 4) holds A[lr][lk] and
// B[lk][lr] of a step and the results D[lk + 4 q][lr]); a column of the panel is a column of B and of D in every product, so a
// right-hand side's solution does not depend on what shares its panel.  Operands beyond a tail are masked to zero on both sides,
// rows beyond a front are clamped and not stored.  No atomics; every sum has a fixed order.  The panel of a front sits in LDS
// (16 x m doubles, up to 131 KB: L is streamed from global memory / L2, 16 columns at a time).
// Bounds: a pass reads the arena once per panel of 16 columns -- the traffic of k_mf_solve's pass per panel; the per-front chain of
// barrier-separated blocks is latency, as in k_si_panels.  Measurements: NOTES.md section 36.
#include <algorithm>

#include "sgo_device.h"
#include "sgo_internal.h"
#include "sgo_mfront_dev.h"

namespace sgo {
namespace {

// what edge_operands reads of an edge list, for the candidates
struct CandSrc {
  const int* vi;
  const int* vj;
  const double* zinv;
};

// GATE 1: one thread per candidate of [t0, t1) -- record, then A^T / B^T into the (zeroed) panel; GATE 2: the record alone
// (sgo_candidate_joint needs every candidate's record before the first chunk's columns are contracted); GATE 0: one thread per
// entry of the caller's columns src[ncols][3 n] (hessian order) -> panel[ncols][3 n] (elimination position).
template <int GATE>
__global__ __launch_bounds__(kBlock) void k_fs_rhs(FsCandDev C, int t0, int t1, const double* __restrict__ poses, const double* __restrict__ src,
                                                   const int* __restrict__ pos_h, int ncols, int n3, double* __restrict__ panel) {
  if (GATE) {
    const int t = t0 + blockIdx.x * kBlock + threadIdx.x;
    if (t >= t1) return;
    const CandSrc s = {C.vi, C.vj, C.zinv};
    EdgeOperands p;
    edge_operands(s, (size_t)C.n, t, poses, p);
    double sz, cz, e[3];
    sincos(p.zt, &sz, &cz);
    edge_error(p, sz, cz, e);
    EdgeJac J;
    edge_jacobians(p, sz, cz, J);
    double* rec = C.rec + (size_t)kFsRec * t;
    rec[0] = e[0]; rec[1] = e[1]; rec[2] = e[2];
    rec[3] = J.A00; rec[4] = J.A01; rec[5] = J.A02; rec[6] = J.A10; rec[7] = J.A11; rec[8] = J.A12;
    rec[9] = J.B00; rec[10] = J.B01; rec[11] = J.B10; rec[12] = J.B11;
    if (GATE == 2) return;
    const int ri = C.row[2 * t], rj = C.row[2 * t + 1];
    double* col = panel + 3 * (size_t)(t - t0) * n3;   // column a of R: row a of A at the rows of i, row a of B at the rows of j
    if (ri >= 0) {
      double* q = col + 3 * (size_t)ri;
      q[0] = J.A00; q[1] = J.A01; q[2] = J.A02;
      q += n3;
      q[0] = J.A10; q[1] = J.A11; q[2] = J.A12;
      q += n3;
      q[0] = 0.0; q[1] = 0.0; q[2] = -1.0;
    }
    if (rj >= 0) {
      double* q = col + 3 * (size_t)rj;
      q[0] = J.B00; q[1] = J.B01; q[2] = 0.0;
      q += n3;
      q[0] = J.B10; q[1] = J.B11; q[2] = 0.0;
      q += n3;
      q[0] = 0.0; q[1] = 0.0; q[2] = 1.0;
    }
  } else {
    const long long tot = (long long)ncols * n3;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < tot; i += (long long)gridDim.x * kBlock) {
      const int c = (int)(i / n3), r = (int)(i % n3);
      panel[i] = src[(size_t)c * n3 + 3 * (size_t)pos_h[r / 3] + r % 3];
    }
  }
}

__global__ __launch_bounds__(kMfThreads) void k_fs_forward(MfDev M, MfSelDev Z, MfFsDev Fs, int lvl0, double* __restrict__ Yg,
                                                          double* __restrict__ Ug, int n3) {
  extern __shared__ double T[];   // the front's rows of the panel: column c at T + c * ldp
  if (M.flags[0]) return;
  const int f = M.level_front[lvl0 + blockIdx.x];
  const MfFrontDev F = M.fronts[f];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const int m = F.m, s3 = F.own3, ld = F.ld, nb3 = m - s3;
  if (m == 0) return;
  const int ldp = (m + 2) | 1;
  double* __restrict__ Yp = Yg + (size_t)blockIdx.y * kMfPanel * n3 + 3 * (size_t)F.e0;
  double* __restrict__ Up = Ug + (size_t)blockIdx.y * Fs.U3 * kMfPanel;
  for (int i = tid; i < kMfPanel * m; i += kMfThreads) {
    const int c = i / m, r = i - c * m;
    T[c * ldp + r] = r < s3 ? Yp[(size_t)c * n3 + r] : 0.0;
  }
  __syncthreads();
  // the children's updates, child 0 before child 1 (a child's boundary poses are distinct local poses of this front)
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (F.kid[k] < 0) continue;
    const MfFrontDev C = M.fronts[F.kid[k]];
    const int cb3 = C.m - C.own3;
    const int* __restrict__ cm = Z.cmap + Z.cmap_off[F.kid[k]];
    const double* __restrict__ Uc = Up + (size_t)Fs.uoff[F.kid[k]] * kMfPanel;
    for (int i = tid; i < kMfPanel * cb3; i += kMfThreads) {
      const int r = i >> 4, c = i & 15;
      T[c * ldp + 3 * cm[r / 3] + r % 3] += Uc[i];
    }
    __syncthreads();
  }
  const double* __restrict__ A = M.arena + F.off;
  const double* __restrict__ Yi = M.yinv + 3 * (size_t)F.e0 * kMfPanel;
  for (int k0 = 0; k0 < s3; k0 += kMfPanel) {
    const int wp = min(kMfPanel, s3 - k0), rb = k0 + wp, nR = m - rb;
    // y_J = L_JJ^-1 t_J, in place (one wave: its loads of t_J are complete before the product's results are stored)
    if (wave == 0) {
      mf_d4 acc = {0.0, 0.0, 0.0, 0.0};
      double av[4], bv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = lk + 4 * s;
        const bool kv = k < wp;
        av[s] = (kv && lr < wp) ? Yi[(size_t)(k0 + lr) * kMfPanel + k] : 0.0;
        bv[s] = kv ? T[lr * ldp + k0 + k] : 0.0;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = lk + 4 * q;
        if (row < wp) T[lr * ldp + k0 + row] = acc[q];
      }
    }
    __syncthreads();
    // t_R -= L_RJ y_J, a tile of 16 rows per wave
    for (int rt = wave; rt < ((nR + 15) >> 4); rt += kMfNW) {
      const int r = rb + 16 * rt + lr;
      const bool rv = r < m;
      mf_d4 acc = {0.0, 0.0, 0.0, 0.0};
      double av[4], bv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = lk + 4 * s;
        const bool kv = k < wp;
        av[s] = (kv && rv) ? A[(size_t)(k0 + min(k, wp - 1)) * ld + min(r, m - 1)] : 0.0;
        bv[s] = kv ? T[lr * ldp + k0 + k] : 0.0;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * rt + lk + 4 * q;
        if (row < nR) T[lr * ldp + rb + row] -= acc[q];
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < kMfPanel * s3; i += kMfThreads) {
    const int c = i / s3, r = i - c * s3;
    Yp[(size_t)c * n3 + r] = T[c * ldp + r];
  }
  double* __restrict__ Uf = Up + (size_t)Fs.uoff[f] * kMfPanel;
  for (int i = tid; i < kMfPanel * nb3; i += kMfThreads) Uf[i] = T[(i & 15) * ldp + s3 + (i >> 4)];
}

__global__ __launch_bounds__(kMfThreads) void k_fs_backward(MfDev M, int lvl0, const double* __restrict__ Yg, double* __restrict__ Xg, int n3) {
  extern __shared__ double T[];                         // own rows: y, then x as the blocks finish; boundary rows: x
  __shared__ double part[kMfNW][kMfPanel * kMfPanel];   // the waves' shares of L_RJ^T x_R
  if (M.flags[0]) return;
  const MfFrontDev F = M.fronts[M.level_front[lvl0 + blockIdx.x]];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const int m = F.m, s3 = F.own3, ld = F.ld;
  if (s3 == 0) return;
  const int ldp = (m + 2) | 1;
  const double* __restrict__ Yp = Yg + (size_t)blockIdx.y * kMfPanel * n3 + 3 * (size_t)F.e0;
  double* __restrict__ Xp = Xg + (size_t)blockIdx.y * kMfPanel * n3;
  for (int i = tid; i < kMfPanel * m; i += kMfThreads) {
    const int c = i / m, r = i - c * m;
    T[c * ldp + r] = r < s3 ? Yp[(size_t)c * n3 + r] : Xp[(size_t)c * n3 + 3 * (size_t)M.bnd[F.bnd_off + (r - s3) / 3] + (r - s3) % 3];
  }
  __syncthreads();
  const double* __restrict__ A = M.arena + F.off;
  const double* __restrict__ Yi = M.yinv + 3 * (size_t)F.e0 * kMfPanel;
  for (int k0 = ((s3 - 1) / kMfPanel) * kMfPanel; k0 >= 0; k0 -= kMfPanel) {
    const int wp = min(kMfPanel, s3 - k0), rb = k0 + wp, nR = m - rb;
    {
      const int steps = (nR + 3) >> 2, per = (steps + kMfNW - 1) / kMfNW;
      const int st1 = min(steps, (wave + 1) * per);
      mf_d4 acc = {0.0, 0.0, 0.0, 0.0};
      const double* __restrict__ col = A + (size_t)(k0 + min(lr, wp - 1)) * ld + rb;
      for (int st = wave * per; st < st1; ++st) {
        const int k = 4 * st + lk;
        const bool kv = k < nR;
        const int kc = min(k, nR - 1);
        const double a = (kv && lr < wp) ? col[kc] : 0.0;
        const double b = kv ? T[lr * ldp + rb + kc] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) part[wave][(lk + 4 * q) * kMfPanel + lr] = acc[q];
    }
    __syncthreads();
    if (wave == 0) {
      double av[4], v[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = lk + 4 * s;   // (row k of y_J - L_RJ^T x_R, column lr: a product's result layout is the next one's operand layout)
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < kMfNW; ++w) sum += part[w][k * kMfPanel + lr];
        v[s] = k < wp ? T[lr * ldp + k0 + k] - sum : 0.0;
        av[s] = (k < wp && lr < wp) ? Yi[(size_t)(k0 + k) * kMfPanel + lr] : 0.0;   // (L_JJ^-T)[lr][k]
      }
      mf_d4 x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) x = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], v[s], x, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = lk + 4 * q;
        if (row < wp) T[lr * ldp + k0 + row] = x[q];
      }
    }
    __syncthreads();   // (the next block reads this one's x as part of its x_R, and part again)
  }
  for (int i = tid; i < kMfPanel * s3; i += kMfThreads) {
    const int c = i / s3, r = i - c * s3;
    Xp[(size_t)c * n3 + 3 * (size_t)F.e0 + r] = T[c * ldp + r];
  }
}

// out: [n][kFsOut] = d2, P (9, row-major), the decision; then one double: the factorisation's failure flag (flags == nullptr: 0)
__global__ __launch_bounds__(kBlock) void k_fs_gate(FsCandDev C, int t0, int t1, const double* __restrict__ W, int n3, double chi2_max,
                                                    const int* __restrict__ flags, double* __restrict__ out) {
  const int t = t0 + blockIdx.x * kBlock + threadIdx.x;
  if (t == t0) out[(size_t)kFsOut * C.n] = flags ? (double)flags[0] : 0.0;
  if (t >= t1) return;
  const double* rec = C.rec + (size_t)kFsRec * t;
  const double e[3] = {rec[0], rec[1], rec[2]};
  double Q[3][3];
  fs_candidate_q(rec, C.row + 2 * t, W + 3 * (size_t)(t - t0) * n3, n3, Q);
  double P[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) P[a][b] = 0.5 * (Q[a][b] + Q[b][a]);
  // Omega^-1 by cofactors
  const size_t ns = (size_t)C.n;
  const double o00 = C.info[t], o01 = C.info[ns + t], o02 = C.info[2 * ns + t], o11 = C.info[3 * ns + t], o12 = C.info[4 * ns + t],
               o22 = C.info[5 * ns + t];
  const double c00 = o11 * o22 - o12 * o12, c01 = o02 * o12 - o01 * o22, c02 = o01 * o12 - o02 * o11;
  const double c11 = o00 * o22 - o02 * o02, c12 = o01 * o02 - o00 * o12, c22 = o00 * o11 - o01 * o01;
  const double idet = 1.0 / (o00 * c00 + o01 * c01 + o02 * c02);
  const double s00 = c00 * idet + P[0][0], s10 = c01 * idet + P[1][0], s20 = c02 * idet + P[2][0];
  const double s11 = c11 * idet + P[1][1], s21 = c12 * idet + P[2][1], s22 = c22 * idet + P[2][2];
  // d2 = |L^-1 e|^2, S = L L^T (S not positive definite: NaN, which does not pass)
  const double l00 = sqrt(s00), l10 = s10 / l00, l20 = s20 / l00;
  const double l11 = sqrt(s11 - l10 * l10), l21 = (s21 - l20 * l10) / l11;
  const double l22 = sqrt(s22 - l20 * l20 - l21 * l21);
  const double z0 = e[0] / l00, z1 = (e[1] - l10 * z0) / l11, z2 = (e[2] - l20 * z0 - l21 * z1) / l22;
  const double d2 = z0 * z0 + z1 * z1 + z2 * z2;
  double* o = out + (size_t)kFsOut * t;
  o[0] = d2;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) o[1 + 3 * a + b] = P[a][b];
  o[10] = d2 <= chi2_max ? 1.0 : 0.0;
}

// One thread per block G_st: candidate s of all n (x), candidate t of the chunk [t0, t1) (y), whose three columns of H^-1 R are W's
// columns 3 (t - t0) ...; G: raw [3 n][3 n], every block written once over the chunks of a call
__global__ __launch_bounds__(kBlock) void k_fs_gram(FsCandDev C, int t0, int t1, const double* __restrict__ W, int n3, double* __restrict__ G) {
  const int s = blockIdx.x * kBlock + threadIdx.x, t = t0 + blockIdx.y;
  if (s >= C.n || t >= t1) return;
  double Q[3][3];
  fs_candidate_q(C.rec + (size_t)kFsRec * s, C.row + 2 * s, W + 3 * (size_t)(t - t0) * n3, n3, Q);
  const size_t ld = 3 * (size_t)C.n;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) G[(3 * (size_t)s + a) * ld + 3 * (size_t)t + b] = Q[a][b];
}

// One thread per block pair s <= t: S_st = (G_st + G_ts^T) / 2, stored at both places (S is exactly symmetric); the diagonal block
// adds Omega^-1 by cofactors as k_fs_gate does and the thread stores e_s; then the factorisation's failure flag
__global__ __launch_bounds__(kBlock) void k_fs_joint_table(FsCandDev C, const double* __restrict__ G, const int* __restrict__ flags,
                                                           double* __restrict__ table) {
  const int n = C.n;
  const int s = blockIdx.x * kBlock + threadIdx.x, t = blockIdx.y;
  const size_t ld = 3 * (size_t)n;
  if (s == 0 && t == 0) table[ld * ld + ld] = flags ? (double)flags[0] : 0.0;
  if (s > t || t >= n) return;
  double P[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) P[a][b] = 0.5 * (G[(3 * (size_t)s + a) * ld + 3 * (size_t)t + b] + G[(3 * (size_t)t + b) * ld + 3 * (size_t)s + a]);
  if (s == t) {
    const size_t ns = (size_t)n;
    const double o00 = C.info[t], o01 = C.info[ns + t], o02 = C.info[2 * ns + t], o11 = C.info[3 * ns + t], o12 = C.info[4 * ns + t],
                 o22 = C.info[5 * ns + t];
    const double c00 = o11 * o22 - o12 * o12, c01 = o02 * o12 - o01 * o22, c02 = o01 * o12 - o02 * o11;
    const double c11 = o00 * o22 - o02 * o02, c12 = o01 * o02 - o00 * o12, c22 = o00 * o11 - o01 * o01;
    const double idet = 1.0 / (o00 * c00 + o01 * c01 + o02 * c02);
    // (the lower triangle's values, mirrored: P is symmetric bit for bit, so the block is)
    const double s00 = c00 * idet + P[0][0], s10 = c01 * idet + P[1][0], s20 = c02 * idet + P[2][0];
    const double s11 = c11 * idet + P[1][1], s21 = c12 * idet + P[2][1], s22 = c22 * idet + P[2][2];
    P[0][0] = s00; P[1][0] = s10; P[2][0] = s20; P[1][1] = s11; P[2][1] = s21; P[2][2] = s22;
    P[0][1] = s10; P[0][2] = s20; P[1][2] = s21;
    const double* rec = C.rec + (size_t)kFsRec * t;
    double* e = table + ld * ld + 3 * (size_t)t;
    e[0] = rec[0]; e[1] = rec[1]; e[2] = rec[2];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      table[(3 * (size_t)s + a) * ld + 3 * (size_t)t + b] = P[a][b];
      table[(3 * (size_t)t + b) * ld + 3 * (size_t)s + a] = P[a][b];
    }
}

// One workgroup per subset of the resident table: the selected candidates ascending (a mask row compacted by ballot and prefix
// count, or the pair number decoded), S_ss's lower triangle over the row e_s gathered into LDS (leading dimension odd: a row's
// elements, and a column's, fall in distinct banks), then a right-looking Cholesky that carries e_s along as row m -- after step k
// row m holds e_s - L[:, :k] z[:k] --, so z_k = row m's entry k over L_kk and d2 = sum z_k^2, added in ascending k by one thread.
// Step k, one barrier: every thread takes r = 1 / sqrt(a_kk) itself (a_kk is final since step k - 1's barrier; a_kk not above
// zero: NaN, which spreads to d2) and element (i, j), k < j <= i <= m, loses (a_ik r) (a_jk r); column k stays unscaled, nobody reads it again
// but z_k.  Thread (ty, tx) of 16 x 16 owns the elements i = ty mod 16, j = tx mod 16 of the trailing block: an element's updates
// are its own thread's, in ascending k.  No atomics.  A subset's arithmetic depends on the table and its index list alone: not on
// the launch's LDS size (rows_cap sets the leading dimension, which moves nothing but addresses), its place in the grid or the batch.
template <bool PAIRS>
__global__ __launch_bounds__(kJointThreads) void k_joint_subsets(const double* __restrict__ table, int n, const uint8_t* __restrict__ mask, int b0,
                                                                 int rows_cap, double* __restrict__ d2) {
  extern __shared__ double Lm[];   // [rows_cap + 1][ld], then zz [rows_cap]
  __shared__ int idx[SGO_JOINT_MAX_SUBSET];
  __shared__ int wcnt[kJointThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tx = tid & 15, ty = tid >> 4;
  const long long b = (long long)b0 + blockIdx.x;
  const int ld = rows_cap | 1;
  double* __restrict__ zz = Lm + (size_t)(rows_cap + 1) * ld;
  int cnt, ps = 0, pt = 0;
  if (PAIRS) {
    // b = pt (pt + 1) / 2 + ps, ps <= pt
    pt = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while ((long long)pt * (pt + 1) / 2 > b) --pt;
    while ((long long)(pt + 1) * (pt + 2) / 2 <= b) ++pt;
    ps = (int)(b - (long long)pt * (pt + 1) / 2);
    cnt = ps == pt ? 1 : 2;
    if (tid == 0) {
      idx[0] = ps;
      idx[1] = pt;
    }
  } else {
    const bool on = tid < n && mask[(size_t)b * n + tid] != 0;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int base = 0;
    cnt = 0;
#pragma unroll
    for (int w = 0; w < kJointThreads / 64; ++w) {
      if (w < wave) base += wcnt[w];
      cnt += wcnt[w];
    }
    const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
    if (on && pos < SGO_JOINT_MAX_SUBSET) idx[pos] = tid;
  }
  const int m = 3 * cnt;
  if (cnt > SGO_JOINT_MAX_SUBSET || m > rows_cap) {   // (the driver refuses such a subset before the launch)
    if (tid == 0) d2[b] = __builtin_nan("");
    return;
  }
  __syncthreads();
  const size_t ldS = 3 * (size_t)n;
  const double* __restrict__ ev = table + ldS * ldS;
  for (int i = ty; i <= m; i += 16) {
    const double* __restrict__ src = i < m ? table + (3 * (size_t)idx[i / 3] + i % 3) * ldS : ev;
    for (int j = tx; j <= i && j < m; j += 16) Lm[i * ld + j] = src[3 * (size_t)idx[j / 3] + j % 3];
  }
  __syncthreads();
  for (int k = 0; k < m; ++k) {
    const double akk = Lm[k * ld + k];
    const double r = akk > 0.0 ? 1.0 / sqrt(akk) : __builtin_nan("");
    const int i0 = k + 1 + ((ty - (k + 1)) & 15), j0 = k + 1 + ((tx - (k + 1)) & 15);   // the first i >= k + 1 with i mod 16 == ty
    for (int i = i0; i <= m; i += 16) {
      const double li = Lm[i * ld + k] * r;
      for (int j = j0; j <= i && j < m; j += 16) Lm[i * ld + j] -= li * (Lm[j * ld + k] * r);
    }
    __syncthreads();
  }
  if (tid < m) {
    const double akk = Lm[tid * ld + tid];
    const double z = Lm[m * ld + tid] * (akk > 0.0 ? 1.0 / sqrt(akk) : __builtin_nan(""));
    zz[tid] = z * z;
  }
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int k = 0; k < m; ++k) sum += zz[k];
    if (PAIRS) {
      d2[(size_t)ps * n + pt] = sum;
      d2[(size_t)pt * n + ps] = sum;
    } else {
      d2[b] = sum;
    }
  }
}

}  // namespace

void launch_fs_rhs_columns(hipStream_t s, int ncols, int n3, const double* src, const int* pos_h, double* panel) {
  const long long tot = (long long)ncols * n3;
  const int grid = (int)std::max<long long>(1, std::min<long long>((tot + kBlock - 1) / kBlock, 4096));
  SGO_LAUNCH((k_fs_rhs<0>), dim3(grid), dim3(kBlock), 0, s, FsCandDev(), 0, 0, (const double*)nullptr, src, pos_h, ncols, n3, panel);
}
void launch_fs_rhs_candidates(hipStream_t s, const FsCandDev& C, int t0, int t1, const double* poses, int n3, double* panel) {
  SGO_LAUNCH((k_fs_rhs<1>), dim3((t1 - t0 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, C, t0, t1, poses, (const double*)nullptr, (const int*)nullptr,
             3 * (t1 - t0), n3, panel);
}
void launch_fs_records(hipStream_t s, const FsCandDev& C, const double* poses) {
  SGO_LAUNCH((k_fs_rhs<2>), dim3((C.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, C, 0, C.n, poses, (const double*)nullptr, (const int*)nullptr, 0, 0,
             (double*)nullptr);
}
void launch_fs_forward(hipStream_t s, const MfDev& M, const MfSelDev& Z, const MfFsDev& Fs, int lvl0, int count, int panels, size_t lds, double* Y,
                       double* U, int n3) {
  SGO_LAUNCH(k_fs_forward, dim3(count, panels), dim3(kMfThreads), lds, s, M, Z, Fs, lvl0, Y, U, n3);
}
void launch_fs_backward(hipStream_t s, const MfDev& M, int lvl0, int count, int panels, size_t lds, const double* Y, double* X, int n3) {
  SGO_LAUNCH(k_fs_backward, dim3(count, panels), dim3(kMfThreads), lds, s, M, lvl0, Y, X, n3);
}
void launch_fs_gate(hipStream_t s, const FsCandDev& C, int t0, int t1, const double* W, int n3, double chi2_max, const int* flags, double* out) {
  SGO_LAUNCH(k_fs_gate, dim3((t1 - t0 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, C, t0, t1, W, n3, chi2_max, flags, out);
}
void launch_fs_gram(hipStream_t s, const FsCandDev& C, int t0, int t1, const double* W, int n3, double* G) {
  SGO_LAUNCH(k_fs_gram, dim3((C.n + kBlock - 1) / kBlock, t1 - t0), dim3(kBlock), 0, s, C, t0, t1, W, n3, G);
}
void launch_fs_joint_table(hipStream_t s, const FsCandDev& C, const double* G, const int* flags, double* table) {
  SGO_LAUNCH(k_fs_joint_table, dim3((C.n + kBlock - 1) / kBlock, C.n), dim3(kBlock), 0, s, C, G, flags, table);
}
void launch_joint_subsets(hipStream_t s, const double* table, int n, const uint8_t* mask, int b0, int count, int rows_cap, double* d2) {
  const size_t lds = joint_lds_bytes(rows_cap);
  if (mask) SGO_LAUNCH((k_joint_subsets<false>), dim3(count), dim3(kJointThreads), lds, s, table, n, mask, b0, rows_cap, d2);
  else SGO_LAUNCH((k_joint_subsets<true>), dim3(count), dim3(kJointThreads), lds, s, table, n, mask, b0, rows_cap, d2);
}
bool joint_prepare_device() {
  const int lds = (int)joint_lds_bytes(3 * SGO_JOINT_MAX_SUBSET);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_joint_subsets<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&k_joint_subsets<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}
bool fs_prepare_device() {
  const int lds = (int)sizeof(double) * kMfPanel * ((kMfMaxDim + 2) | 1);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fs_forward), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fs_backward), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

}  // namespace sgo
