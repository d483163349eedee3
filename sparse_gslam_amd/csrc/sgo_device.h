// sgo_device.h -- device-side helpers shared by the HIP translation units (the arithmetic of EdgeSE2,
// wave64 reductions, the wavefront segmented scan, the XCD-aware group walk and its frame, the arithmetic of the
// multigrid cycle).
#pragma once
#include "sgo_internal.h"

namespace sgo {
namespace {

constexpr double kPi = 3.14159265358979323846;

// g2o::normalize_theta, branch structure and roundings kept literal (result in [-pi, pi)).  The product m 2 pi and the
// subtraction are two roundings, as in the host statements (oracle/, numpy, sgo_rules.h on an x86-64 baseline host): fused into
// one FMA the result differs wherever m 2 pi is inexact (from |m| = 11 on; 3e-11 at t = 1e6), and near an odd multiple of pi it can land
// on the other side of the branch (tests/wrap_cases.py has such points).  Contraction is switched off for this body alone.
__device__ __forceinline__ double norm_theta(double t) {
#pragma clang fp contract(off)
  if (t >= -kPi && t < kPi) return t;
  double m = floor(t / (2 * kPi));
  t = t - m * 2 * kPi;
  if (t >= kPi) t -= 2 * kPi;
  if (t < -kPi) t += 2 * kPi;
  return t;
}

// ---------------------------------------------------------------------------- the arithmetic of EdgeSE2
// One statement of what every edge kernel evaluates, in layers: operands -> computeError -> Omega e, e^2 and the robust
// kernel's weight -> the Jacobians of linearizeOplus -> one side's terms of constructQuadraticForm.  k_chi2 stops after the
// weight; k_linearize and k_ov_lin take all of it (edge_side_terms).  Three kernels share the first layers and keep
// a contraction of their own, because each rounds differently from edge_side:
//   k_direct (sgo_direct.hip)        error from its one sincos, weight, Jacobians; then both sides at once, with the
//                                    Jacobians' constant 0 / +-1 entries folded by hand
//   k_mf_edges (sgo_mfront.hip)      error, weight; generic 3x3 loops over A, B, Ow A, Ow B; the gradient as -w (A^T (Omega e))
//   k_row_strength (sgo_kernels.hip) error; e^2 summed entry by entry, generic 3x3 loops, Ow R as w (Omega R)
// The last two also write the Jacobians' entries out themselves: with full 3x3 arrays under generic loops the compiler
// shares products between entries (A01 = B10, A10 = B01, ...) only when it sees the expressions in place, and through
// edge_jacobians it emits other multiplies (7 more in each), which the byte-for-byte equality of a refactor rules out.

// Src: EdgeListDev or EdgeSlotsDev, k an edge or a compact slot of it, ns the component stride of its zinv / info.
// Poses and inverse measurement of edge k.
struct EdgeOperands {
  double xi, yi, ti, xj, yj, tj;                // poses of vertices()[0] and [1]
  double zx, zy, zt;                            // cached inverse measurement
};
template <class Src>
__device__ __forceinline__ void edge_operands(const Src& s, size_t ns, int k, const double* __restrict__ poses, EdgeOperands& p) {
  const int vi = s.vi[k], vj = s.vj[k];
  p.xi = poses[3 * (size_t)vi]; p.yi = poses[3 * (size_t)vi + 1]; p.ti = poses[3 * (size_t)vi + 2];
  p.xj = poses[3 * (size_t)vj]; p.yj = poses[3 * (size_t)vj + 1]; p.tj = poses[3 * (size_t)vj + 2];
  p.zx = s.zinv[k]; p.zy = s.zinv[ns + k]; p.zt = s.zinv[2 * ns + k];
}

// EdgeSE2::computeError with the cached inverse measurement Zi:
//   e = toVector( Zi * (Xi^-1 * Xj) ),  SE2 algebra literal (g2o SE2::operator* / inverse).
// tin = norm_theta(-ti) with its sine and cosine s1, c1 come from the caller; sz, cz: sine and cosine of zt.
__device__ __forceinline__ void edge_error_sc(const EdgeOperands& p, double tin, double s1, double c1, double sz, double cz,
                                              double (&e)[3]) {
  const double ix = c1 * (-p.xi) - s1 * (-p.yi);
  const double iy = s1 * (-p.xi) + c1 * (-p.yi);
  const double dx = ix + c1 * p.xj - s1 * p.yj;
  const double dy = iy + s1 * p.xj + c1 * p.yj;
  const double dth = norm_theta(tin + p.tj);
  e[0] = p.zx + cz * dx - sz * dy;
  e[1] = p.zy + sz * dx + cz * dy;
  e[2] = norm_theta(p.zt + dth);
}
__device__ __forceinline__ void edge_error(const EdgeOperands& p, double sz, double cz, double (&e)[3]) {
  const double tin = norm_theta(-p.ti);
  double s1, c1;
  sincos(tin, &s1, &c1);
  edge_error_sc(p, tin, s1, c1, sz, cz, e);
}

// RobustKernelDCS::robustify; phi < 0: no kernel.
__device__ __forceinline__ void dcs(double e2, double phi, double* rho0, double* rho1) {
  double r0 = e2, r1 = 1.0;
  if (phi >= 0.0) {
    const double scale = (2.0 * phi) / (phi + e2);
    if (!(scale >= 1.0)) {
      r0 = scale * e2 * scale;
      r1 = scale * scale;
    }
  }
  *rho0 = r0;
  *rho1 = r1;
}

// RobustKernel::robustify for an edge's kind (sgo_internal.h: RobustKind) and parameter d = phi: rho0 and the weight rho1 of
// e2 = e^T Omega e as g2o's robust_kernel_impl.cpp has them (include/sgo.h lists the pairs); rho2 is not formed, g2o's
// robustInformation is rho1 Omega.  kRobustDcs is dcs() itself.  The other kinds come with d > 0 (sgo_set_robust_kernels checks);
// an edge without information has e2 = 0, for which every kind gives rho0 = 0 and weight 1.
__device__ __forceinline__ void robustify(int kind, double e2, double d, double* rho0, double* rho1) {
  if (kind == kRobustDcs) {
    dcs(e2, d, rho0, rho1);
    return;
  }
  double r0 = e2, r1 = 1.0;
  if (d > 0.0) {
    const double d2 = d * d;
    switch (kind) {
      case kRobustHuber:
        if (!(e2 <= d2)) {
          const double s = sqrt(e2);
          r0 = 2.0 * s * d - d2;
          r1 = d / s;
        }
        break;
      case kRobustPseudoHuber: {
        const double a = sqrt(1.0 + e2 / d2);
        r0 = 2.0 * d2 * (a - 1.0);
        r1 = 1.0 / a;
        break;
      }
      case kRobustCauchy: {
        const double a = 1.0 + e2 / d2;
        r0 = d2 * log(a);
        r1 = 1.0 / a;
        break;
      }
      case kRobustGemanMcClure: {
        const double a = 1.0 / (1.0 + e2);
        r0 = e2 * a;
        r1 = a * a;
        break;
      }
      case kRobustWelsch: {
        const double a = exp(-e2 / d2);
        r0 = d2 * (1.0 - a);
        r1 = a;
        break;
      }
      case kRobustFair: {
        const double a = sqrt(e2) / d;
        r0 = 2.0 * d2 * (a - log1p(a));
        r1 = 1.0 / (1.0 + a);
        break;
      }
      case kRobustTukey:
        if (sqrt(e2) <= d) {
          const double u = 1.0 - e2 / d2;
          r0 = d2 * (1.0 - u * u * u) / 3.0;
          r1 = u * u;
        } else {
          r0 = d2 / 3.0;
          r1 = 0.0;
        }
        break;
      case kRobustSaturated:
        if (!(e2 <= d2)) {
          r0 = d2;
          r1 = 0.0;
        }
        break;
      default: break;
    }
  }
  *rho0 = r0;
  *rho1 = r1;
}
// KINDS: the graph holds kinds other than kRobustDcs (EdgeListDev::kinds), and the kind is read where phi is.  Without it the
// kernels are the instruction sequences of a graph that knows DCS only.
template <bool KINDS, class Src>
__device__ __forceinline__ void edge_robustify(const Src& s, int k, double e2, double* rho0, double* rho1) {
  if (KINDS) robustify(s.kind[k], e2, s.phi[k], rho0, rho1);
  else dcs(e2, s.phi[k], rho0, rho1);
}

// The information's upper triangle, Omega e (unscaled), e^2 = e^T Omega e, and the robust kernel's rho0 and weight w = rho1.
// (The information is loaded here, after the error, not with the operands: held across the error's sincos it costs
// k_chi2 a step of occupancy.)
struct EdgeWeight {
  double o00, o01, o02, o11, o12, o22, oe0, oe1, oe2, e2, rho0, w;
};
template <bool KINDS, class Src>
__device__ __forceinline__ void edge_weight(const Src& s, size_t ns, int k, const double (&e)[3], EdgeWeight& W) {
  W.o00 = s.info[k]; W.o01 = s.info[ns + k]; W.o02 = s.info[2 * ns + k];
  W.o11 = s.info[3 * ns + k]; W.o12 = s.info[4 * ns + k]; W.o22 = s.info[5 * ns + k];
  W.oe0 = W.o00 * e[0] + W.o01 * e[1] + W.o02 * e[2];
  W.oe1 = W.o01 * e[0] + W.o11 * e[1] + W.o12 * e[2];
  W.oe2 = W.o02 * e[0] + W.o12 * e[1] + W.o22 * e[2];
  W.e2 = e[0] * W.oe0 + e[1] * W.oe1 + e[2] * W.oe2;
  edge_robustify<KINDS>(s, k, W.e2, &W.rho0, &W.w);
}

// EdgeSE2::linearizeOplus: A = d e / d x_i = Rz a, B = d e / d x_j = Rz b (rows: error components), with Rz of the
// inverse measurement.  The entries not held are constant: A's third row is (0, 0, -1), B's (0, 0, 1), B02 = B12 = 0.
struct EdgeJac {
  double A00, A01, A02, A10, A11, A12, B00, B01, B10, B11;
};
__device__ __forceinline__ void edge_jacobians(double si, double ci, double sz, double cz, double ddx, double ddy, EdgeJac& J) {
  const double a02 = -si * ddx + ci * ddy, a12 = -ci * ddx - si * ddy;
  J.A00 = cz * (-ci) - sz * si; J.A01 = cz * (-si) - sz * (-ci); J.A02 = cz * a02 - sz * a12;
  J.A10 = sz * (-ci) + cz * si; J.A11 = sz * (-si) + cz * (-ci); J.A12 = sz * a02 + cz * a12;
  J.B00 = cz * ci - sz * (-si); J.B01 = cz * si - sz * ci;
  J.B10 = sz * ci + cz * (-si); J.B11 = sz * si + cz * ci;
}
__device__ __forceinline__ void edge_jacobians(const EdgeOperands& p, double sz, double cz, EdgeJac& J) {
  double si, ci;
  sincos(p.ti, &si, &ci);
  edge_jacobians(si, ci, sz, cz, p.xj - p.xi, p.yj - p.yi, J);
}

// BaseBinaryEdge::constructQuadraticForm for the row on one side of the edge (dir 0: vertices()[0], row Jacobian R = A;
// dir 1: vertices()[1], R = B; column Jacobian C the other one), with robustInformation Ow = w Omega and Omega e scaled
// by w:  T = Ow R,  D = R^T T (symmetric packing 00 01 02 11 12 22),  g = R^T (Ow e).
struct EdgeSide {
  double R00, R01, R02, R10, R11, R12, R22;   // third row (0, 0, R22)
  double C00, C01, C02, C10, C11, C12, C22;
  double T00, T01, T02, T10, T11, T12, T20, T21, T22;
  double D[6], g[3];
};
__device__ __forceinline__ void edge_side(const EdgeWeight& W, const EdgeJac& J, bool dir, EdgeSide& S) {
  const double w = W.w;
  const double w00 = w * W.o00, w01 = w * W.o01, w02 = w * W.o02, w11 = w * W.o11, w12 = w * W.o12, w22 = w * W.o22;
  const double oe0 = W.oe0 * w, oe1 = W.oe1 * w, oe2 = W.oe2 * w;
  S.R00 = dir ? J.B00 : J.A00; S.R01 = dir ? J.B01 : J.A01; S.R02 = dir ? 0.0 : J.A02;
  S.R10 = dir ? J.B10 : J.A10; S.R11 = dir ? J.B11 : J.A11; S.R12 = dir ? 0.0 : J.A12;
  S.R22 = dir ? 1.0 : -1.0;
  S.C00 = dir ? J.A00 : J.B00; S.C01 = dir ? J.A01 : J.B01; S.C02 = dir ? J.A02 : 0.0;
  S.C10 = dir ? J.A10 : J.B10; S.C11 = dir ? J.A11 : J.B11; S.C12 = dir ? J.A12 : 0.0;
  S.C22 = dir ? -1.0 : 1.0;
  // T = Ow * R  (3x3), R has zero entries (2,0),(2,1)
  S.T00 = w00 * S.R00 + w01 * S.R10; S.T01 = w00 * S.R01 + w01 * S.R11; S.T02 = w00 * S.R02 + w01 * S.R12 + w02 * S.R22;
  S.T10 = w01 * S.R00 + w11 * S.R10; S.T11 = w01 * S.R01 + w11 * S.R11; S.T12 = w01 * S.R02 + w11 * S.R12 + w12 * S.R22;
  S.T20 = w02 * S.R00 + w12 * S.R10; S.T21 = w02 * S.R01 + w12 * S.R11; S.T22 = w02 * S.R02 + w12 * S.R12 + w22 * S.R22;
  S.D[0] = S.R00 * S.T00 + S.R10 * S.T10;
  S.D[1] = S.R00 * S.T01 + S.R10 * S.T11;
  S.D[2] = S.R00 * S.T02 + S.R10 * S.T12;
  S.D[3] = S.R01 * S.T01 + S.R11 * S.T11;
  S.D[4] = S.R01 * S.T02 + S.R11 * S.T12;
  S.D[5] = S.R02 * S.T02 + S.R12 * S.T12 + S.R22 * S.T22;
  S.g[0] = S.R00 * oe0 + S.R10 * oe1;
  S.g[1] = S.R01 * oe0 + S.R11 * oe1;
  S.g[2] = S.R02 * oe0 + S.R12 * oe1 + S.R22 * oe2;
}
// the off-diagonal block towards the other endpoint, row-major:  R^T Ow C = T^T C  (T^T because Ow is symmetric)
__device__ __forceinline__ void edge_block(const EdgeSide& S, double (&blk)[9]) {
  blk[0] = S.T00 * S.C00 + S.T10 * S.C10; blk[1] = S.T00 * S.C01 + S.T10 * S.C11; blk[2] = S.T00 * S.C02 + S.T10 * S.C12 + S.T20 * S.C22;
  blk[3] = S.T01 * S.C00 + S.T11 * S.C10; blk[4] = S.T01 * S.C01 + S.T11 * S.C11; blk[5] = S.T01 * S.C02 + S.T11 * S.C12 + S.T21 * S.C22;
  blk[6] = S.T02 * S.C00 + S.T12 * S.C10; blk[7] = S.T02 * S.C01 + S.T12 * S.C11; blk[8] = S.T02 * S.C02 + S.T12 * S.C12 + S.T22 * S.C22;
}
// All layers for edge (or slot) k of s, seen from the row on side `dir`.  The caller adds S.D, subtracts S.g and, where it
// wants the block, calls edge_block.
template <bool KINDS, class Src>
__device__ __forceinline__ void edge_side_terms(const Src& s, size_t ns, int k, const double* __restrict__ poses, bool dir, EdgeSide& S) {
  EdgeOperands p;
  edge_operands(s, ns, k, poses, p);
  double sz, cz, e[3];
  sincos(p.zt, &sz, &cz);
  edge_error(p, sz, cz, e);
  EdgeWeight W;
  edge_weight<KINDS>(s, ns, k, e, W);
  EdgeJac J;
  edge_jacobians(p, sz, cz, J);
  edge_side(W, J, dir, S);
}

// v of lane l (wave-uniform)
__device__ __forceinline__ double readlane_d(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum(double v);   // (below, with the DPP helpers)

// Block-wide sums of N values; thread 0 stores them to out[i * stride + blockIdx.x].
template <int N>
__device__ __forceinline__ void block_sum_store(double (&v)[N], double* out, int stride) {
  __shared__ double sm[N][kWavesPerBlock];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = wave_sum(v[i]);
    if (lane == 0) sm[i][w] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double s = sm[i][0];
#pragma unroll
      for (int k = 1; k < kWavesPerBlock; ++k) s += sm[i][k];
      out[(size_t)i * stride + blockIdx.x] = s;
    }
  }
}

// Deterministic sum of nparts partials by one block (fixed order), result in every thread.
__device__ __forceinline__ double block_reduce_parts(const double* parts, int nparts) {
  __shared__ double sm2[kWavesPerBlock];
  __shared__ double res;
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kBlock) s += parts[i];
  s = wave_sum(s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm2[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = sm2[0];
#pragma unroll
    for (int k = 1; k < kWavesPerBlock; ++k) t += sm2[k];
    res = t;
  }
  __syncthreads();
  return res;
}

// N such sums at once (same summation order as block_reduce_parts for each of them, so the values
// are bit-identical) with ONE LDS exchange: 2 barriers instead of 3 N.  parts[c] == nullptr gives 0.
template <int N>
__device__ __forceinline__ void block_reduce_parts_n(const double* const (&parts)[N], const int (&cnt)[N],
                                                     double (&out)[N]) {
  __shared__ double smn[N][kWavesPerBlock];
  double s[N];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    s[c] = 0.0;
    if (parts[c])
      for (int i = threadIdx.x; i < cnt[c]; i += kBlock) s[c] += parts[c][i];
  }
#pragma unroll
  for (int c = 0; c < N; ++c) s[c] = wave_sum(s[c]);
  __syncthreads();  // readers of an earlier call are done with smn
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < N; ++c) smn[c][threadIdx.x >> 6] = s[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; ++c) {
    double t = smn[c][0];
#pragma unroll
    for (int k = 1; k < kWavesPerBlock; ++k) t += smn[c][k];
    out[c] = t;
  }
}

// Inclusive segmented scan over the wave: lanes with equal `row` that are contiguous form a
// segment; after the scan the LAST lane of a segment holds the segment sum.
//
// Cross-lane traffic goes through DPP moves on the vector ALU, not through ds_bpermute: the LDS crossbar
// is what the tile kernel's staging and the 40-odd permutes of a shuffle-based scan would otherwise
// share (measured: SQ_WAIT_INST_LDS 18 % of the wave cycles of k_spmv0t with __shfl_up).  Steps 1, 2, 4, 8
// stay inside a row of 16 lanes (row_shr); the carries into rows 1 / 3 and then 2 / 3 come from lane 15 / 47
// and lane 31 (row_bcast15 / row_bcast31).  The two carry steps rely on what every caller guarantees:
// the keys of the ACTIVE lanes are non-decreasing along the wave (slots sorted by target), so a lane whose
// key equals that of the last lane of the previous row(s) belongs to a segment that spans everything in
// between.  Inactive lanes carry unique negative keys and never match.
// (Full row mask: bound_ctrl makes the lanes without a source lane read 0, so no lane keeps `old` and the compiler has no
// destination to initialise -- two moves per double and step less.  A key of 0 can then match row 0 at the start of a row
// of 16 lanes, where the value that comes with it is 0 as well: nothing is added.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_int(int old, int v) {
  if (ROW_MASK == 0xF) return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xF, false);
}
// key of the next lane (lane 63: 0), by a wavefront shift on the vector ALU instead of a permute through the LDS crossbar
__device__ __forceinline__ int next_lane_key(int key) { return __builtin_amdgcn_update_dpp(0, key, 0x130, 0xF, 0xF, true); }
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_double(double v) {
  const int lo = dpp_int<CTRL, ROW_MASK>(0, __double2loint(v)), hi = dpp_int<CTRL, ROW_MASK>(0, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
// Sum over the wave, the same in every lane: an inclusive scan by DPP moves on the vector ALU (the total ends up in lane
// 63) and two v_readlane.  (The shuffle tree it replaces went through ds_bpermute: twelve LDS-crossbar round trips in a
// dependent chain of six, in the prologue of every kernel that re-reduces partial sums and at the end of every kernel
// that leaves some.)
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_double<0x111, 0xF>(v);   // row_shr:1
  v += dpp_double<0x112, 0xF>(v);   // row_shr:2
  v += dpp_double<0x114, 0xF>(v);   // row_shr:4
  v += dpp_double<0x118, 0xF>(v);   // row_shr:8
  v += dpp_double<0x142, 0xA>(v);   // row_bcast15 into rows 1 and 3
  v += dpp_double<0x143, 0xC>(v);   // row_bcast31 into rows 2 and 3
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

template <int N, int CTRL, int ROW_MASK>
__device__ __forceinline__ void seg_scan_step(int row, double (&v)[N]) {
  constexpr int kNoKey = (int)0x80000000;   // lanes without a source lane see a key no lane has
  // (v += f u with f = 1.0 / 0.0 instead of a select and an add: one fused multiply-add, bit-identical for finite u)
  const double f = dpp_int<CTRL, ROW_MASK>(kNoKey, row) == row ? 1.0 : 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double u = dpp_double<CTRL, ROW_MASK>(v[i]);
    v[i] = fma(f, u, v[i]);
  }
}
template <int N>
__device__ __forceinline__ void seg_scan(int row, double (&v)[N]) {
  seg_scan_step<N, 0x111, 0xF>(row, v);   // row_shr:1
  seg_scan_step<N, 0x112, 0xF>(row, v);   // row_shr:2
  seg_scan_step<N, 0x114, 0xF>(row, v);   // row_shr:4
  seg_scan_step<N, 0x118, 0xF>(row, v);   // row_shr:8
  seg_scan_step<N, 0x142, 0xA>(row, v);   // row_bcast15 into rows 1 and 3
  seg_scan_step<N, 0x143, 0xC>(row, v);   // row_bcast31 into rows 2 and 3
}
// After seg_scan: this lane is the last of its segment and holds the segment's sums (inactive lanes, key < 0: never).
__device__ __forceinline__ bool segment_end(int key, int lane) {
  const int kn = next_lane_key(key);
  return key >= 0 && (lane == 63 || kn != key);
}

// Row-major 3x3 block of LOGICAL slot k of a level's operator: from the slot-indexed pair-SoA array on
// the coarse levels; on level 0 through ref[] from the symmetric storage (diagonal blocks in symmetric
// packing, off-diagonal blocks stored once and transposed for the other endpoint's row).
__device__ __forceinline__ void load_block(const BsrDev& A, size_t k, double (&b)[9]) {
  // All three sources fill nine named scalars and ONE sequence of stores hands them to the caller's array.  (With a store
  // sequence per branch the optimiser merges the branches' last stores into one store through a phi of POINTERS -- b[8] on
  // two paths, b[7] on the third -- and the caller's array can then no longer live in registers: the Galerkin products,
  // k_p_values and k_block_norms went through scratch memory for it.)
  double v0, v1, v2, v3, v4, v5, v6, v7, v8;
  if (A.ref == nullptr) {
    const size_t ns = (size_t)A.nslot;
    v0 = A.blk[blk_at(0, k, ns)]; v1 = A.blk[blk_at(1, k, ns)]; v2 = A.blk[blk_at(2, k, ns)];
    v3 = A.blk[blk_at(3, k, ns)]; v4 = A.blk[blk_at(4, k, ns)]; v5 = A.blk[blk_at(5, k, ns)];
    v6 = A.blk[blk_at(6, k, ns)]; v7 = A.blk[blk_at(7, k, ns)]; v8 = A.blk[blk_at(8, k, ns)];
  } else {
    const int r = A.ref[k];
    if (r < 0) {
      const double* d = A.dblk + 6 * (size_t)(~r);
      v0 = d[0]; v1 = d[1]; v2 = d[2];
      v3 = v1; v4 = d[3]; v5 = d[4];
      v6 = v2; v7 = v5; v8 = d[5];
    } else {
      const size_t u = (size_t)(r >> 1), nu = (size_t)A.nus;
      const double2* __restrict__ bp = reinterpret_cast<const double2*>(A.ublk);
      const double2 p0 = bp[u], p1 = bp[nu + u], p2 = bp[2 * nu + u], p3 = bp[3 * nu + u];
      const bool tr = r & 1;
      // stored row-major p0.x p0.y p1.x | p1.y p2.x p2.y | p3.x p3.y ublk8 ; transposed: swap (1,3) (2,6) (5,7)
      v0 = p0.x; v4 = p2.x; v8 = A.ublk8[u];
      v1 = tr ? p1.y : p0.y; v3 = tr ? p0.y : p1.y;
      v2 = tr ? p3.x : p1.x; v6 = tr ? p1.x : p3.x;
      v5 = tr ? p3.y : p2.y; v7 = tr ? p2.y : p3.y;
    }
  }
  b[0] = v0; b[1] = v1; b[2] = v2; b[3] = v3; b[4] = v4; b[5] = v5; b[6] = v6; b[7] = v7; b[8] = v8;
}

// Map (block, wave) -> first group and stride so that XCD x (blocks with blockIdx % 8 == x under
// the observed round-robin dispatch; speed only, never correctness) walks the contiguous band
// [x * ngrp / 8, (x + 1) * ngrp / 8) of groups.
// (nblocks: the workgroups that walk -- a multiple of 8; block: this workgroup's index among them.  NB, B: int or unsigned
// as the caller has them, so that a built-in index keeps its unsigned shift.  WAVES: the waves of a workgroup)
template <int WAVES = kWavesPerBlock, class NB, class B>
__device__ __forceinline__ void group_walk_b(int ngrp, NB nblocks, B block, int* first, int* last, int* stride) {
  const int xcd = block & 7, slot = block >> 3, per_xcd = nblocks >> 3;
  const int lo = (int)(((long long)ngrp * xcd) >> 3), hi = (int)(((long long)ngrp * (xcd + 1)) >> 3);
  *first = lo + slot * WAVES + (threadIdx.x >> 6);
  *last = hi;
  *stride = per_xcd * WAVES;
}
__device__ __forceinline__ void group_walk(int ngrp, int* first, int* last, int* stride) {
  group_walk_b(ngrp, gridDim.x, blockIdx.x, first, last, stride);
}

// The frame of a row-group walk inside a replayed PCG iteration, where a launch is a chain of dependent memory round trips:
// the cursor requests its wave's FIRST group's bounds when it is made -- before the kernel waits for the stop flag --, so
// that the two round trips overlap; the later groups' bounds are read as the walk reaches them (group_bounds, in a loop
// for (bool first = true; gc.g < gc.gend; gc.g += gc.gstride, first = false) that ends in seg_scan and segment_end).
// (restrict_groups, k_prolong_p, k_prolong_fold, k_up_fold, k_restrict in sgo_amg.hip, spmv0_groups below; k_spmv in
// sgo_kernels.hip spells the cursor out.  base: the walk covers the groups [base, base + ngrp).  The set-up and refresh
// kernels -- k_linearize, k_galerkin, k_filtered_diag, k_p_values, k_block_products -- have no stop flag to overlap the
// request with: they take group_walk and segment_end only.)
// Kernel arguments: the command processor places the leading PLAIN parameters of a kernel (pointers and scalars, up to 14
// dwords) in SGPRs before the first wave starts; whatever stands behind the first by-value struct is loaded from the
// argument block, one more round trip at the head of the chain (NOTES.md section 49).  So a kernel of
// the replayed iteration takes what its first round of requests needs -- the stop flag's address, the group array and its
// extent -- as leading parameters and hands THOSE to group_cursor; the launch wrappers copy them out of the structs, which
// stay complete.
struct GroupCursor {
  int g, gend, gstride;   // this wave's group, the end of its XCD's band, the stride
  int gb0, ge0;           // the first group's bounds
};
template <int WAVES = kWavesPerBlock, class NB, class B>
__device__ __forceinline__ GroupCursor group_cursor(const int* __restrict__ grp, int ngrp, NB nblocks, B block, int base = 0) {
  GroupCursor c = {0, 0, 0, 0, 0};
  group_walk_b<WAVES>(ngrp, nblocks, block, &c.g, &c.gend, &c.gstride);
  c.g += base;
  c.gend += base;
  if (c.g < c.gend) {
    c.gb0 = grp[c.g];
    c.ge0 = grp[c.g + 1];
  }
  return c;
}
__device__ __forceinline__ void group_bounds(const GroupCursor& c, const int* __restrict__ grp, bool first, int& gb, int& ge) {
  gb = first ? c.gb0 : grp[c.g];
  ge = first ? c.ge0 : grp[c.g + 1];
}

// ---------------------------------------------------------------------------- the arithmetic of the multigrid cycle
// One statement of what the cycle's kernels share, in layers: coefficients -> coarse operand -> 3x3 block products -> rigid-body
// transfer -> block-Jacobi pieces.  Loops, loads and epilogues stay in the kernels.  k_spmv keeps its own copy (reason there).
// K-cycle coefficients (Notay's flexible-CG steps per level): c = sum(num) / sum(den) of per-workgroup partial sums that
// every workgroup re-reduces in the same fixed order; not positive or not finite gives 0.  (k_prolong_fold calls only this.)
__device__ __forceinline__ double cycle_ratio(double den, double num) {
  return (den > 0.0 && isfinite(den) && isfinite(num)) ? num / den : 0.0;
}
// c1 = ratio r1 (no numerator: 1), c2 = ratio r2 when use2 (otherwise 0): all partial sums in ONE block reduction; none at
// all for the plain V-cycle's unscaled correction.  Callers build a ratio full or leave it default, and a second vector
// always comes with its ratio (fcg in sgo_amg.hip): a denominator alone, or use2 with an empty r2 (c2 = 0 here), is made by nobody.
// (k_prolong_p, k_up_fold, k_prolong_add, k_prolong_rows in sgo_amg.hip; ratios2 in sgo_kernels.hip is k_spmv's own copy.)
__device__ __forceinline__ void cycle_coefficients(const SpmvRatio& r1, const SpmvRatio& r2, bool use2, double& c1, double& c2) {
  c1 = 1.0;
  c2 = 0.0;
  if (!r1.num && !use2) return;
  const double* const parts[4] = {r1.num ? r1.den : nullptr, r1.num, (use2 && r2.num) ? r2.den : nullptr,
                                  use2 ? r2.num : nullptr};
  const int cnt[4] = {r1.n_den, r1.n_num, r2.n_den, r2.n_num};
  double v[4];
  block_reduce_parts_n<4>(parts, cnt, v);
  if (r1.num) c1 = cycle_ratio(v[0], v[1]);
  if (use2) c2 = cycle_ratio(v[2], v[3]);
}

// The coarse correction a level prolongates, itself the flexible-CG combination of the child level's two steps:
//   w = c1 u1[a .. a+2] (+ c2 u2[a .. a+2] when there is a second step)        (a = 3 x the coarse node)
// (k_prolong_p, k_prolong_fold, k_up_fold, k_prolong_add, k_prolong_rows)
__device__ __forceinline__ void coarse_operand(const double* __restrict__ u1, const double* __restrict__ u2, double c1, double c2,
                                               size_t a, double (&w)[3]) {
  w[0] = c1 * u1[a]; w[1] = c1 * u1[a + 1]; w[2] = c1 * u1[a + 2];
  if (u2) {
    w[0] += c2 * u2[a]; w[1] += c2 * u2[a + 1]; w[2] += c2 * u2[a + 2];
  }
}

// acc[0..2] += B x for a row-major 3x3 block B  (k_prolong_p, k_prolong_fold, k_up_fold, k_prolong_rows; tile_slot)
__device__ __forceinline__ void block_mul_acc(const double (&b)[9], const double (&x)[3], double* acc) {
  acc[0] += b[0] * x[0] + b[1] * x[1] + b[2] * x[2];
  acc[1] += b[3] * x[0] + b[4] * x[1] + b[5] * x[2];
  acc[2] += b[6] * x[0] + b[7] * x[1] + b[8] * x[2];
}
// the same with the block as a coarse level's pair-SoA storage hands it over: component pairs 01 23 45 67 and 8  (k_up_fold)
__device__ __forceinline__ void block_mul_acc(double2 p0, double2 p1, double2 p2, double2 p3, double b8, const double (&x)[3], double* acc) {
  acc[0] += p0.x * x[0] + p0.y * x[1] + p1.x * x[2];
  acc[1] += p1.y * x[0] + p2.x * x[1] + p2.y * x[2];
  acc[2] += p3.x * x[0] + p3.y * x[1] + b8 * x[2];
}
// acc[0..2] += B^T r  (restrict_groups: the restriction with the transfer's transpose)
__device__ __forceinline__ void block_tmul_acc(const double (&b)[9], const double (&r)[3], double* acc) {
  acc[0] += b[0] * r[0] + b[3] * r[1] + b[6] * r[2];
  acc[1] += b[1] * r[0] + b[4] * r[1] + b[7] * r[2];
  acc[2] += b[2] * r[0] + b[5] * r[1] + b[8] * r[2];
}

// The tentative transfer: a node at lever arm d = (d_x, d_y) from its aggregate's centre moves with the aggregate's rigid
// motion, T(d) = [[1, 0, -d_y], [0, 1, d_x], [0, 0, 1]] (sgo_amg.hip's header).
//   x += T(d) w             (k_prolong_add, k_prolong_rows)
__device__ __forceinline__ void rigid_add(double dx, double dy, const double (&w)[3], double* x) {
  x[0] += w[0] - dy * w[2]; x[1] += w[1] + dx * w[2]; x[2] += w[2];
}
//   acc[0..2] += T(d)^T r   (k_restrict)
__device__ __forceinline__ void rigid_t_acc(double dx, double dy, const double (&r)[3], double* acc) {
  acc[0] += r[0]; acc[1] += r[1]; acc[2] += -dy * r[0] + dx * r[1] + r[2];
}
//   B T(d) keeps B's first two columns; its third column is m = -d_y col0 + d_x col1 + col2
//   (k_galerkin; k_filtered_diag and k_p_values accumulate it as it stands: block_rigid_acc)
__device__ __forceinline__ void block_rigid_col(const double (&b)[9], double dx, double dy, double (&m)[3]) {
  m[0] = -dy * b[0] + dx * b[1] + b[2];
  m[1] = -dy * b[3] + dx * b[4] + b[5];
  m[2] = -dy * b[6] + dx * b[7] + b[8];
}
__device__ __forceinline__ void block_rigid_acc(const double (&b)[9], double dx, double dy, double* acc) {
  acc[0] += b[0]; acc[1] += b[1]; acc[2] += -dy * b[0] + dx * b[1] + b[2];
  acc[3] += b[3]; acc[4] += b[4]; acc[5] += -dy * b[3] + dx * b[4] + b[5];
  acc[6] += b[6]; acc[7] += b[7]; acc[8] += -dy * b[6] + dx * b[7] + b[8];
}
//   acc += T(d_i)^T M with M = B T(d_j) = [col0 col1 m]: M's first two rows as they are, the third row
//   -d_y row0 + d_x row1 + row2  -- together T_i^T B T_j, one term of the Galerkin sum  (k_galerkin)
__device__ __forceinline__ void rigid_t_block_acc(const double (&b)[9], const double (&m)[3], double dx, double dy, double* acc) {
  acc[0] += b[0]; acc[1] += b[1]; acc[2] += m[0];
  acc[3] += b[3]; acc[4] += b[4]; acc[5] += m[1];
  acc[6] += -dy * b[0] + dx * b[3] + b[6]; acc[7] += -dy * b[1] + dx * b[4] + b[7];
  acc[8] += -dy * m[0] + dx * m[1] + m[2];
}

// The block-Jacobi smoother's pieces; symmetric 3x3 blocks in the packing 00 01 02 11 12 22.
//   o = omega Dinv v        (k_up_fold: operand and both sweeps; spmv0_groups' and k_spmv0t's Jacobi epilogue)
__device__ __forceinline__ void dinv_apply(const double* __restrict__ di, double omega, const double (&v)[3], double (&o)[3]) {
  o[0] = omega * (di[0] * v[0] + di[1] * v[1] + di[2] * v[2]);
  o[1] = omega * (di[1] * v[0] + di[3] * v[1] + di[4] * v[2]);
  o[2] = omega * (di[2] * v[0] + di[4] * v[1] + di[5] * v[2]);
}
//   Dinv = D^-1 by cofactors; a determinant that is zero or not finite gives the zero block (the row is then not smoothed)
//   (k_finalize for level 0, k_level_dinv for the coarse levels)
__device__ __forceinline__ void dinv_from_block(const double (&d)[6], double* __restrict__ di) {
  const double d00 = d[0], d01 = d[1], d02 = d[2], d11 = d[3], d12 = d[4], d22 = d[5];
  const double c00 = d11 * d22 - d12 * d12, c01 = d02 * d12 - d01 * d22, c02 = d01 * d12 - d02 * d11;
  const double c11 = d00 * d22 - d02 * d02, c12 = d01 * d02 - d00 * d12, c22 = d00 * d11 - d01 * d01;
  const double det = d00 * c00 + d01 * c01 + d02 * c02;
  const double id = (det != 0.0 && isfinite(det)) ? 1.0 / det : 0.0;
  di[0] = c00 * id; di[1] = c01 * id; di[2] = c02 * id; di[3] = c11 * id; di[4] = c12 * id; di[5] = c22 * id;
}

// The leading parameters of the kernels that run spmv0_groups: S = a.S; grp / grow / gown / gtr = A's; [ulo, uhi) the
// wave groups to walk (a.u0, a.u1, or all of A.ngrp when a.u1 == 0), worked out by the launch wrapper.
struct Spmv0Head {
  const PcgScalars* S;
  const int *grp, *grow, *gown, *gtr;
  int ulo, uhi;
};
// Body of the wave-group level-0 product k_spmv0 (sgo_kernels.hip; modes and storage described there): the first
// `nblocks` workgroups of a launch walk the groups -- the launch may carry workgroups with another job behind them
// (sgo_amg.hip: the folded cycle's level-0 pass and its restriction in one launch).
// h: what the first round of requests needs, as the kernel received it in its leading parameters (Spmv0Head above).
template <int MODE>
__device__ __forceinline__ void spmv0_groups(const Spmv0Head& h, const Sym0Dev& A, const Spmv0Args& a, int nblocks) {
  // On the graphs that take this kernel a launch is a chain of dependent round trips (~0.3 us each on top of the 1.8-us
  // node of a replayed hipGraph: scripts/micro/graph_floor.hip), so the chain is kept short: the first group's descriptors
  // are requested before the stop flag is waited for, a slot's column with its meta byte, and the row's own data (diagonal
  // block, operand, right-hand side, block-diagonal inverse) before the segmented scan instead of after it.
  const int lane = threadIdx.x & 63;
  const size_t nu = (size_t)A.nus;
  const double2* __restrict__ bp = reinterpret_cast<const double2*>(A.ublk);
  double dotacc[2] = {0.0, 0.0};
  GroupCursor gc = group_cursor(h.grp, h.uhi - h.ulo, nblocks, blockIdx.x, h.ulo);
  int f_r0 = 0, f_ob = 0, f_tb = 0;
  if (gc.g < gc.gend) {
    f_r0 = h.grow[gc.g]; f_ob = h.gown[gc.g]; f_tb = h.gtr[gc.g];
  }
  if (h.S && h.S->stop) return;
  for (bool first = true; gc.g < gc.gend; gc.g += gc.gstride, first = false) {
    int gb, ge;
    group_bounds(gc, h.grp, first, gb, ge);
    const int r0 = first ? f_r0 : h.grow[gc.g];
    int ob = first ? f_ob : h.gown[gc.g], tb = first ? f_tb : h.gtr[gc.g];
    double acc[3] = {0.0, 0.0, 0.0};
    int row = -1 - lane;
    for (int kb = gb; kb < ge; kb += 64) {
      const int k = kb + lane;
      const bool active = k < ge;
      const int m = active ? (int)A.meta[k] : (kSlotNoBlock << 6);
      const int cj = active ? A.col[k] : 0;
      const int type = m >> 6;
      const unsigned long long omask = __ballot(type == kSlotOwned), tmask = __ballot(type == kSlotTransposed);
      const int orank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(omask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)omask, 0u));
      const int trank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(tmask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)tmask, 0u));
      int idx = ob + orank;
      const bool tr = type == kSlotTransposed;
      if (tr) idx = A.tref[tb + trank];
      ob += __popcll(omask);
      tb += __popcll(tmask);
      if (active) row = r0 + (m & 63);
      if (type != kSlotNoBlock) {
        const size_t c = 3 * (size_t)cj;
        const double x0 = a.x[c], x1 = a.x[c + 1], x2 = a.x[c + 2];
        const double2 p0 = bp[idx], p1 = bp[nu + idx], p2 = bp[2 * nu + idx], p3 = bp[3 * nu + idx];
        const double b8 = A.ublk8[idx];
        // row-major b0..b8 = p0.x p0.y p1.x | p1.y p2.x p2.y | p3.x p3.y b8 ; transposed: swap (1,3) (2,6) (5,7)
        const double m01 = tr ? p1.y : p0.y, m02 = tr ? p3.x : p1.x;
        const double m10 = tr ? p0.y : p1.y, m12 = tr ? p3.y : p2.y;
        const double m20 = tr ? p1.x : p3.x, m21 = tr ? p2.y : p3.y;
        acc[0] += p0.x * x0 + m01 * x1 + m02 * x2;
        acc[1] += m10 * x0 + p2.x * x1 + m12 * x2;
        acc[2] += m20 * x0 + m21 * x1 + b8 * x2;
      }
    }
    // the row's own data, requested by every lane of the row (one address per row) before the scan
    double dd0 = 0, dd1 = 0, dd2 = 0, dd3 = 0, dd4 = 0, dd5 = 0, s0 = 0, s1 = 0, s2 = 0, rb0 = 0, rb1 = 0, rb2 = 0;
    double di[6] = {0, 0, 0, 0, 0, 0};
    if (row >= 0) {
      const size_t o = 3 * (size_t)row;
      const double* dd = A.dblk + 6 * (size_t)row;
      dd0 = dd[0]; dd1 = dd[1]; dd2 = dd[2]; dd3 = dd[3]; dd4 = dd[4]; dd5 = dd[5];
      s0 = a.x[o]; s1 = a.x[o + 1]; s2 = a.x[o + 2];
      if (MODE != S0_AX) {
        rb0 = a.b[o]; rb1 = a.b[o + 1]; rb2 = a.b[o + 2];
      }
      if (MODE == S0_JACOBI) {
#pragma unroll
        for (int q = 0; q < 6; ++q) di[q] = A.dinv[6 * (size_t)row + q];
      }
    }
    seg_scan<3>(row, acc);
    if (segment_end(row, lane)) {
      const size_t o = 3 * (size_t)row;
      double o0 = acc[0] + dd0 * s0 + dd1 * s1 + dd2 * s2;
      double o1 = acc[1] + dd1 * s0 + dd3 * s1 + dd4 * s2;
      double o2 = acc[2] + dd2 * s0 + dd4 * s1 + dd5 * s2;
      if (MODE != S0_AX) {
        const double t[3] = {rb0 - o0, rb1 - o1, rb2 - o2};
        if (MODE == S0_JACOBI) {
          double sw[3];
          dinv_apply(di, a.omega, t, sw);
          o0 = s0 + sw[0]; o1 = s1 + sw[1]; o2 = s2 + sw[2];
        } else {
          o0 = t[0]; o1 = t[1]; o2 = t[2];
        }
      }
      a.y[o] = o0; a.y[o + 1] = o1; a.y[o + 2] = o2;
      if (a.dotA) dotacc[0] += a.dotA[o] * o0 + a.dotA[o + 1] * o1 + a.dotA[o + 2] * o2;
      if (a.dotA2) dotacc[1] += a.dotA2[o] * o0 + a.dotA2[o + 1] * o1 + a.dotA2[o + 2] * o2;
    }
  }
  if (a.partials) block_sum_store<2>(dotacc, a.partials, kMaxPartials);
}

}  // namespace
}  // namespace sgo
