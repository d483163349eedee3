// sgo_amg.hip -- rigid-body smoothed-aggregation multigrid preconditioner for the GN Hessian.
//
// Why it exists: the block-Jacobi PCG that BASELINE.json's north_star names needs 8 000+
// iterations per GN iteration on the 10k-pose graph and does not reach 1e-8 in 20 000 on the
// 100k-pose graph (profiles/r01_bj_c4_kernel_stats.csv), because the pose-graph Hessian is a
// vector-Laplacian-like operator whose low-energy modes are near-rigid motions of large parts
// of the trajectory.  This preconditioner keeps block-Jacobi as the smoother and adds a
// coarse-grid hierarchy that represents exactly those modes:
//   * nodes are aggregated by strength of connection (greedy root-node aggregation on
//     Frobenius norms of the 3x3 blocks, threshold theta) -- structure built on the host once
//     per sgo_set_graph_se2 (like g2o's symbolic analysis, once per optimize());
//   * the tentative prolongator T is the rigid-body one: an aggregate moves as a rigid body
//     (u_x, u_y, w) about its centre c, so node i at p_i gets T(p_i - c) u with
//     T(d) = [[1,0,-d_y],[0,1,d_x],[0,0,1]] -- the three rigid motions of SE(2) are represented
//     exactly on every level (they are the null space of every edge's Jacobian pair);
//   * the prolongator used is T smoothed by one damped block-Jacobi step, P = (I - w D^-1 H) T
//     (smoothed aggregation); a level whose smoothed coarse operator would be too dense keeps T;
//   * coarse operators are Galerkin products P^T H P, recomputed on the device every GN
//     iteration (values change, structure does not) from product lists the host made at set-up:
//     one lane per block product in target order, wavefront segmented scan per target block --
//     no atomics, bitwise reproducible;
//   * cycle: V-cycle with one damped block-Jacobi sweep before and after (levels that keep T: K-cycle,
//     two flexible-CG steps per level, Notay's AGMG scheme, with the prolongation and the FCG vector
//     updates fused into the SpMV-type launches k_spmv<4..6>); the coarsest level (<= 400 nodes) is
//     solved with an explicit dense inverse recomputed every GN iteration (blocked Gauss-Jordan).
// All launches go to the caller's stream with fixed pointers, so a whole PCG iteration
// including the cycle is captured into one hipGraph.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "sgo_amg.h"
#include "sgo_amg_host.h"
#include "sgo_sort.h"
#include "sgo_comm.h"
#include "sgo_device.h"

namespace sgo {

namespace {

// --------------------------------------------------------------------------------- kernels
// Frobenius norm of every slot's block (strength of connection input).
__global__ __launch_bounds__(kBlock) void k_block_norms(BsrDev A, double* __restrict__ w) {
  for (int k = blockIdx.x * kBlock + threadIdx.x; k < A.nslot; k += gridDim.x * kBlock) {
    double b[9];
    load_block(A, (size_t)k, b);
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) s += b[c] * b[c];
    w[k] = sqrt(s);
  }
}

// Level-0 node positions from the pose array: pos[h] = poses[free_id[h]].xy
__global__ __launch_bounds__(kBlock) void k_positions0(int n, const int* __restrict__ free_id,
                                                       const double* __restrict__ poses, double* __restrict__ pos) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const size_t v = 3 * (size_t)free_id[i];
    pos[2 * (size_t)i] = poses[v];
    pos[2 * (size_t)i + 1] = poses[v + 1];
  }
}

// Aggregate centres and lever arms: one wave per aggregate (lanes stride over the members, wave-wide sums in a fixed
// order).  An aggregate may hold hundreds of members -- the last level of a stalled hierarchy collapses into one --
// which one thread per aggregate walked serially (57 us per launch on C4 with random closures, 24 us on C4).
__global__ __launch_bounds__(kBlock) void k_centres(int nc, const int* __restrict__ mem_ptr, const int* __restrict__ mem,
                                                    const double* __restrict__ pos, double* __restrict__ cpos,
                                                    double* __restrict__ d) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), nwaves = gridDim.x * kWavesPerBlock;
  for (int a = wave; a < nc; a += nwaves) {
    const int lo = mem_ptr[a], hi = mem_ptr[a + 1];
    double sx = 0.0, sy = 0.0;
    for (int t = lo + lane; t < hi; t += 64) {
      const int i = mem[t];
      sx += pos[2 * (size_t)i];
      sy += pos[2 * (size_t)i + 1];
    }
    sx = wave_sum(sx);   // (the total, in every lane)
    sy = wave_sum(sy);
    const double inv = 1.0 / (double)(hi - lo);
    const double cx = sx * inv, cy = sy * inv;
    if (lane == 0) {
      cpos[2 * (size_t)a] = cx;
      cpos[2 * (size_t)a + 1] = cy;
    }
    for (int t = lo + lane; t < hi; t += 64) {
      const int i = mem[t];
      d[2 * (size_t)i] = pos[2 * (size_t)i] - cx;
      d[2 * (size_t)i + 1] = pos[2 * (size_t)i + 1] - cy;
    }
  }
}

// Galerkin product: coarse slot s gets sum over its fine slots k=(i,j) of T_i^T B_k T_j.
// One lane per contribution, contributions sorted by coarse slot, segmented scan by coarse slot.
struct GalerkinMap {
  int n = 0;              // contributions (= fine slots)
  int ngrp = 0;
  const int* src = nullptr;  // fine slot of contribution t
  const int* tgt = nullptr;  // coarse slot of contribution t
  const int* grp = nullptr;  // wave groups aligned to coarse-slot boundaries
};
// Multi-GPU (row-owner mode): only the fine slots of the rows [row0, row1) contribute (row1 == 0: all); the ranks'
// partial coarse operators are summed by an all-reduce.
__global__ __launch_bounds__(kBlock) void k_galerkin(BsrDev F, BsrDev C, GalerkinMap g, const double* __restrict__ d, int row0, int row1) {
  const int lane = threadIdx.x & 63;
  const size_t ncs = (size_t)C.nslot;
  int gi, gend, gstride;
  group_walk(g.ngrp, &gi, &gend, &gstride);
  for (; gi < gend; gi += gstride) {
    const int gb = g.grp[gi], ge = g.grp[gi + 1];
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int key = -1 - lane;
    for (int t = gb + lane; t < ge; t += 64) {
      key = g.tgt[t];
      const int k = g.src[t];
      const int i = F.row[k], j = F.col[k];
      if (row1 > 0 && (i < row0 || i >= row1)) continue;
      const double dxi = d[2 * (size_t)i], dyi = d[2 * (size_t)i + 1];
      const double dxj = d[2 * (size_t)j], dyj = d[2 * (size_t)j + 1];
      double b[9], m[3];
      load_block(F, (size_t)k, b);
      block_rigid_col(b, dxj, dyj, m);          // M = B T_j
      rigid_t_block_acc(b, m, dxi, dyi, acc);   // C += T_i^T M
    }
    seg_scan<9>(key, acc);
    if (segment_end(key, lane)) {
#pragma unroll
      for (int c = 0; c < 9; ++c) C.blk[blk_at(c, key, ncs)] = acc[c];
    }
  }
}

// ------------------------------------------------------------------ smoothed aggregation
// Prolongator smoothed by one damped block-Jacobi step, P = (I - w D^-1 A) T, and the Galerkin
// operator A_c = P^T A P formed in two sparse products (AP = A P, then P^T AP).  The sparsity of
// P, AP and A_c and the list of block products behind every entry are fixed by the graph and the
// aggregation: the set-up lists them once (amg_create), sorted by target entry, and the numeric
// phase of every GN iteration is three segmented-sum kernels of the k_galerkin kind.
struct ProdMap {
  int n = 0;                 // products
  int ngrp = 0;
  const int* a = nullptr;    // left operand of product t
  const int* b = nullptr;    // right operand
  const int* tgt = nullptr;  // target entry (non-decreasing in t)
  const int* grp = nullptr;  // wave groups aligned to target boundaries
};
struct PDev {
  int np = 0;                // blocks of P
  int stream_nt = 1;         // the transfer kernels read r_blk / t_blk with non-temporal loads (large levels: the stream must
                             // not displace the level-0 matrix from the Infinity Cache); small levels (0) stay in L2 between cycles
  int* rowptr = nullptr;     // [n + 1] entries of fine row i: [rowptr[i], rowptr[i+1]), coarse cols ascending
  int* row = nullptr;        // [np]
  int* col = nullptr;        // [np]
  double* blk = nullptr;     // [np][9]: the copy the block products GATHER from (one 72-byte record each)
  // The two streamed copies are indexed by GLOBAL entry / position numbers; in multi-GPU row-owner mode (level 0) they hold
  // this rank's rows' entries only: allocated for the rank's range, base pointers shifted, pair strides r_n / t_n and
  // component-8 base pointers of their own (as Sym0Dev::ublk).
  // They are fp32 (the transfers are inside the preconditioner; the Galerkin products gather the fp64 records of blk):
  // quads (0..3), (4..7) as two float4 per entry + component 8, i.e. two 16-byte loads and one 4-byte load per lane.
  int r_n = 0;               // quad stride of r_blk (= np; the rank's entries in row-owner mode)
  float* r_blk = nullptr;    // quad-SoA: the copy the prolongation STREAMS (row order,
                             // non-temporal loads: read once per cycle, must not push the level-0 matrix out of the MALL)
  float* r_blk8 = nullptr;
  int* r_grp = nullptr;      // wave groups over the entries aligned to fine rows (prolongation)
  int r_ngrp = 0;
  ProdMap val;               // a = fine slot k = (i, j), tgt = entry (i, agg(j))
  // the same entries grouped by coarse column, with their own copy of the blocks, so that the
  // restriction streams too: position t holds entry t_idx[t]
  int* t_pos = nullptr;      // [np] position of entry e in column order
  int* t_row = nullptr;      // [np] fine row at position t
  int* t_col = nullptr;      // [np] coarse column at position t
  int t_n = 0;               // entries in the column-ordered copy = its quad stride (= np; the rank's rows' entries in row-owner mode)
  float* t_blk = nullptr;    // quad-SoA: column order, streamed by the restriction (non-temporal loads)
  float* t_blk8 = nullptr;
  int* t_grp = nullptr;      // wave groups over the positions aligned to columns
  int t_ngrp = 0;
  int* t_long = nullptr;     // [t_nlong][2] position ranges of the columns longer than kLongColumn entries (the last level of a
  int t_nlong = 0;           // stalled hierarchy: thousands of fine rows in two aggregates): one WORKGROUP each (k_restrict_p_long)
  int nap = 0;               // blocks of AP
  double* apblk = nullptr;   // [nap][9]
  ProdMap ap;                // a = fine slot (i, j), b = P entry (j, c), tgt = AP entry (i, c)
  ProdMap rap;               // a = P entry (i, a), b = AP entry (i, c), tgt = coarse slot (a, c), c >= a only
  int* rap_mirror = nullptr; // [coarse slots] slot (c, a) of an upper slot (a, c): gets the transposed block (-1: none)
  bool local_lists = false;  // row-owner mode: val / ap / rap list THIS rank's rows' products only (targets of P^T A P without
                             // any are not visited: the caller zeroes the coarse blocks first)
  // FILTERED smoothing (SaHost::filtered): P = (I - w D_F^-1 A_F) T with the operator of the strong connections.  val lists
  // the kept slots only; the diagonal block and its inverse come from here instead of from the level's operator
  const unsigned char* strong = nullptr;   // [nslot]
  double* dF = nullptr;                    // [n][9] D_F, row-major (k_filtered_diag; NOT symmetric on the coarse levels, see there)
  double* dinvF = nullptr;                 // [n][9] its inverse
  int* f_grp = nullptr;                    // wave groups over the level's slots aligned to rows (level 0's logical view has none)
  int f_ngrp = 0;
};

// entry e of a streamed fp32 copy of P (quad-SoA): two 16-byte loads and one 4-byte load per lane; non-temporal on the
// large levels (read once per cycle: the stream must not push the level-0 matrix out of the Infinity Cache)
typedef double sgo_d2 __attribute__((ext_vector_type(2)));
typedef float sgo_f4 __attribute__((ext_vector_type(4)));
constexpr int kLongColumn = 512;   // entries of a P column from which a workgroup instead of a wave restricts it
__device__ __forceinline__ void load9_pairs(const float* __restrict__ base, const float* __restrict__ base8, size_t e, size_t n,
                                            double (&v)[9], bool nt) {
  const sgo_f4* __restrict__ bp = reinterpret_cast<const sgo_f4*>(base);
  sgo_f4 q0, q1;
  float f8;
  if (nt) {
    q0 = __builtin_nontemporal_load(bp + e);
    q1 = __builtin_nontemporal_load(bp + n + e);
    f8 = __builtin_nontemporal_load(base8 + e);
  } else {
    q0 = bp[e];
    q1 = bp[n + e];
    f8 = base8[e];
  }
  v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w; v[8] = f8;
}
__device__ __forceinline__ void load9(const double* __restrict__ base, size_t e, double (&v)[9]) {
#pragma unroll
  for (int c = 0; c < 9; ++c) v[c] = base[9 * e + c];
}

// Diagonal blocks of the FILTERED operator A_F (smoothing the tentative transfer with the strong connections only, SaHost in
// sgo_amg_host.h).  A weak block A_ij is dropped TOGETHER WITH its share of the diagonal block: every edge's contribution to row
// i annihilates the rigid motions, A_ii^e T(p_i) + A_ij^e T(p_j) = 0 with T(p) = [[1,0,-p_y],[0,1,p_x],[0,0,1]], hence
// A_ii^e = -A_ij^e G_ji with G_ji = T(p_j) T(p_i)^-1 = T(p_j - p_i) -- which holds for the assembled blocks and, because the
// transfers reproduce the rigid motions exactly, for the Galerkin operators of the coarse levels too.  So
//     D_F,i = D_i + sum over the weak slots k = (i, j) of A_k T(p_j - p_i)
// is the diagonal block the strong connections alone would have assembled (anchored rows keep their anchor: an edge to a fixed
// vertex has no off-diagonal block to be weak), and A_F T = 0 in the interior exactly as A T = 0: the smoothed columns keep
// representing the rigid motions.  D_F is NOT symmetrised: on level 0 every term A_k T(p_j - p_i) = -A_ii^e is symmetric, but a
// coarse level's operator is a sum of elements over up to four nodes each (a fine edge seen through the smoothed transfer), only
// the SUM over an element's nodes is symmetric, and the symmetric part alone does not keep the row sums: A_F T = O(1e-5 |D|)
// instead of 0, the next level's transfer then misses the rigid motions by as much -- five orders of magnitude above the weak
// connections' own energy -- and the cycle stalls (measured on a numpy prototype of the whole hierarchy, 20k poses from a
// dead-reckoned start: 141 PCG iterations with the symmetrised block, 36 without; the tentative transfer: 266).  D_F is only a
// recipe for P; the coarse operator P^T A P is symmetric whatever it is.
// One lane per slot, rows in wave groups, segmented scan per row; the row's last lane adds D_i and inverts (general 3x3).
// Rows [row0, row1) only when row1 > 0.
__global__ __launch_bounds__(kBlock) void k_filtered_diag(BsrDev F, const int* __restrict__ grp, int ngrp, const unsigned char* __restrict__ strong,
                                                          const double* __restrict__ pos, double* __restrict__ dF, double* __restrict__ dinvF,
                                                          int row0, int row1) {
  const int lane = threadIdx.x & 63;
  int gi, gend, gstride;
  group_walk(ngrp, &gi, &gend, &gstride);
  for (; gi < gend; gi += gstride) {
    const int gb = grp[gi], ge = grp[gi + 1];
    double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // [9]: the row's kept off-diagonal slots (counted)
    int key = -1 - lane;
    for (int k = gb + lane; k < ge; k += 64) {
      const int i = F.row[k];
      if (row1 > 0 && (i < row0 || i >= row1)) {
        key = -1 - lane;
        continue;
      }
      key = i;
      const int j = F.col[k];
      if (j == i) continue;
      if (strong[k]) {
        acc[9] += 1.0;
        continue;
      }
      const double dx = pos[2 * (size_t)j] - pos[2 * (size_t)i], dy = pos[2 * (size_t)j + 1] - pos[2 * (size_t)i + 1];
      double b[9];
      load_block(F, (size_t)k, b);
      block_rigid_acc(b, dx, dy, acc);   // A_k T(p_j - p_i)
    }
    seg_scan<10>(key, acc);
    if (segment_end(key, lane)) {
      double d[9];
      load_block(F, (size_t)F.rowptr[key], d);   // the diagonal slot comes first in its row
      // (a row without any kept connection keeps its whole diagonal block: with everything lumped D_F would be the row sum of
      // the rigid motions -- zero up to rounding in the interior -- and its "inverse" noise.  Its inverse is written as ZERO, like
      // an unsafe row's below: k_p_values still lists the row's diagonal slot, and with D_F = D that term alone would make
      // P_i = (1 - omega_p) T_i -- a row that no longer reproduces the rigid motions (both neighbours heavy hubs, or every
      // closure switched off by DCS: exactly the start the filter exists for).  With a zero inverse the row stays T_i.)
      const double keep = acc[9] > 0.0 ? 1.0 : 0.0;
      // How much of the row's stiffness the dropped connections carried: L = -acc is the sum of their (positive semi-definite)
      // shares of the diagonal block, and trace(D^-1 L) bounds the largest eigenvalue of D^-1 L.  "Negligible" is judged by
      // Frobenius norms; with full information matrices a block's norm can be dominated by one direction (the rotation's, with
      // its lever arms) while the dropped connections carry most of another -- D_F is then nearly singular there and the
      // smoothed row blows up (seen: 150 k poses / 900 k edges, full information, from a dead-reckoned start: PCG broke down
      // in the sixth Gauss-Newton iteration).  Such a row is not smoothed at all: its inverse is written as zero, which
      // k_p_values turns into the tentative row T_i -- the rigid motions stay reproduced exactly.
      const double* dv = F.dinv + 6 * (size_t)key;
      const double tr = -(dv[0] * acc[0] + dv[1] * (acc[1] + acc[3]) + dv[2] * (acc[2] + acc[6]) + dv[3] * acc[4] + dv[4] * (acc[5] + acc[7]) +
                          dv[5] * acc[8]);
      const bool unsafe = !(tr <= 0.5);   // (also when tr is not finite)
#pragma unroll
      for (int c = 0; c < 9; ++c) d[c] += keep * acc[c];
      // inverse by cofactors: inv[r][c] = cof[c][r] / det
      const double c00 = d[4] * d[8] - d[5] * d[7], c01 = d[5] * d[6] - d[3] * d[8], c02 = d[3] * d[7] - d[4] * d[6];
      const double c10 = d[2] * d[7] - d[1] * d[8], c11 = d[0] * d[8] - d[2] * d[6], c12 = d[1] * d[6] - d[0] * d[7];
      const double c20 = d[1] * d[5] - d[2] * d[4], c21 = d[2] * d[3] - d[0] * d[5], c22 = d[0] * d[4] - d[1] * d[3];
      const double det = d[0] * c00 + d[1] * c01 + d[2] * c02;
      const double id = (det != 0.0 && isfinite(det) && keep != 0.0 && !unsafe) ? 1.0 / det : 0.0;
      double* o = dF + 9 * (size_t)key;
#pragma unroll
      for (int c = 0; c < 9; ++c) o[c] = d[c];
      double* di = dinvF + 9 * (size_t)key;
      di[0] = c00 * id; di[1] = c10 * id; di[2] = c20 * id;
      di[3] = c01 * id; di[4] = c11 * id; di[5] = c21 * id;
      di[6] = c02 * id; di[7] = c12 * id; di[8] = c22 * id;
    }
  }
}

// P_e = [e is the own-aggregate entry] T_i - w D_i^-1 sum_{k in e} A_k T_col(k)
// (filtered smoothing, P.dF != nullptr: the listed slots are the kept ones, D_F in place of D_i -- also for the diagonal slot's
// own term)
// (multi-GPU, row-owner mode: the entries of the rows [row0, row1) only; row1 == 0: all)
// (grp = P.val.grp, ngrp = P.val.ngrp: the first requests, leading parameters)
__global__ __launch_bounds__(kBlock) void k_p_values(const int* __restrict__ grp, int ngrp, BsrDev F, PDev P, const int* __restrict__ agg,
                                                     const double* __restrict__ d, double omega_p, int row0, int row1) {
  const int lane = threadIdx.x & 63;
  int gi, gend, gstride;
  group_walk(ngrp, &gi, &gend, &gstride);
  for (; gi < gend; gi += gstride) {
    const int gb = grp[gi], ge = grp[gi + 1];
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int key = -1 - lane;
    for (int t = gb + lane; t < ge; t += 64) {
      key = P.val.tgt[t];
      const int k = P.val.a[t];
      if (row1 > 0) {
        const int i = F.row[k];
        if (i < row0 || i >= row1) {
          key = -1 - lane;
          continue;
        }
      }
      const int j = F.col[k];
      const double dxj = d[2 * (size_t)j], dyj = d[2 * (size_t)j + 1];
      double b[9];
      load_block(F, (size_t)k, b);
      if (P.dF && k == F.rowptr[j]) {   // the diagonal slot of a filtered level (column j = its own row)
        const double* f = P.dF + 9 * (size_t)j;
#pragma unroll
        for (int c = 0; c < 9; ++c) b[c] = f[c];
      }
      block_rigid_acc(b, dxj, dyj, acc);   // A_k T_col(k)
    }
    seg_scan<9>(key, acc);
    if (segment_end(key, lane)) {
      const size_t i = (size_t)P.row[key];
      double o[9];
      if (P.dinvF) {   // filtered smoothing: the general 3x3 inverse of D_F
        const double* di = P.dinvF + 9 * i;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          o[c] = -omega_p * (di[0] * acc[c] + di[1] * acc[3 + c] + di[2] * acc[6 + c]);
          o[3 + c] = -omega_p * (di[3] * acc[c] + di[4] * acc[3 + c] + di[5] * acc[6 + c]);
          o[6 + c] = -omega_p * (di[6] * acc[c] + di[7] * acc[3 + c] + di[8] * acc[6 + c]);
        }
      } else {
        const double* di = F.dinv + 6 * i;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          o[c] = -omega_p * (di[0] * acc[c] + di[1] * acc[3 + c] + di[2] * acc[6 + c]);
          o[3 + c] = -omega_p * (di[1] * acc[c] + di[3] * acc[3 + c] + di[4] * acc[6 + c]);
          o[6 + c] = -omega_p * (di[2] * acc[c] + di[4] * acc[3 + c] + di[5] * acc[6 + c]);
        }
      }
      if (P.col[key] == agg[i]) {
        o[0] += 1.0; o[4] += 1.0; o[8] += 1.0;
        o[2] += -d[2 * i + 1];
        o[5] += d[2 * i];
      }
      const size_t tp = (size_t)P.t_pos[key];
#pragma unroll
      for (int c = 0; c < 9; ++c) P.blk[9 * (size_t)key + c] = o[c];
      {
        const sgo_f4 q0 = {(float)o[0], (float)o[1], (float)o[2], (float)o[3]}, q1 = {(float)o[4], (float)o[5], (float)o[6], (float)o[7]};
        sgo_f4* rq = reinterpret_cast<sgo_f4*>(P.r_blk);
        sgo_f4* tq = reinterpret_cast<sgo_f4*>(P.t_blk);
        rq[key] = q0;
        rq[(size_t)P.r_n + key] = q1;
        tq[tp] = q0;
        tq[(size_t)P.t_n + tp] = q1;
        P.r_blk8[key] = (float)o[8];
        P.t_blk8[tp] = (float)o[8];
      }
    }
  }
}

// out_t = sum over the products of target t of  X(a) * Y(b)   (TRANSPOSE_X: X(a)^T * Y(b))
// X blocks: the logical slots of a level's operator XA (X_BSR; load_block) or plain records X[nx][9];
// Y plain [ny][9]; out plain or pair-SoA (a BsrDev's blk).
// (C4 level 0: 13 M products of A P in 445 us, 3 M of P^T A P in 170 us.  Measured in round 3 and dropped: a second copy of
// the level-0 blocks as 72-byte records for the gathers of A -- 434 us, and the linearisation pays 19 us for writing it:
// lanes of a target share their A blocks, the pair-SoA image is not what costs; records of P / A P padded to 80 bytes so
// that a record is five 16-byte-aligned loads instead of nine 8-byte ones -- A P 474 us, P^T A P 165 us: bytes, not load
// instructions, are what the gathers pay for.)
template <bool X_BSR, bool TRANSPOSE_X, bool OUT_BSR>
__global__ __launch_bounds__(kBlock) void k_block_products(const int* __restrict__ grp, int ngrp, ProdMap mp, BsrDev XA,
                                                           const double* __restrict__ X, const double* __restrict__ Y,
                                                           double* __restrict__ out, size_t nout, const int* __restrict__ mirror,
                                                           const int* __restrict__ rowof, int row0, int row1, int keep_key) {
  const int lane = threadIdx.x & 63;
  int gi, gend, gstride;
  group_walk(ngrp, &gi, &gend, &gstride);   // (grp = mp.grp, ngrp = mp.ngrp: leading parameters)
  int ngb = 0, nge = 0;   // the next group's bounds are requested while the current group is worked on
  if (gi < gend) {
    ngb = grp[gi];
    nge = grp[gi + 1];
  }
  for (; gi < gend; gi += gstride) {
    const int gb = ngb, ge = nge;
    if (gi + gstride < gend) {
      ngb = grp[gi + gstride];
      nge = grp[gi + gstride + 1];
    }
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int key = -1 - lane;
    for (int t = gb + lane; t < ge; t += 64) {
      key = mp.tgt[t];
      const size_t ia = (size_t)mp.a[t], ib = (size_t)mp.b[t];
      // multi-GPU, row-owner mode: only the products whose left operand lives in one of this rank's fine rows (rowof[a]).
      // keep_key (P^T A P, summed over ranks afterwards): a target without any owned product still stores the zero it
      // owes the all-reduce; otherwise (A P: a target's products all sit in one row) it is another rank's and is skipped
      if (row1 > 0) {
        const int i = rowof[ia];
        if (i < row0 || i >= row1) {
          if (!keep_key) key = -1 - lane;
          continue;
        }
      }
      // (the right operand first: its address is known from the index triple, while the left operand of A P hangs on a
      // chain of its own -- slot -> reference -> block; requested behind that chain it was one dependent round trip more)
      double x[9], y[9];
      load9(Y, ib, y);
      if (X_BSR) load_block(XA, ia, x);
      else load9(X, ia, x);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (TRANSPOSE_X) acc[3 * r + c] += x[r] * y[c] + x[3 + r] * y[3 + c] + x[6 + r] * y[6 + c];
          else acc[3 * r + c] += x[3 * r] * y[c] + x[3 * r + 1] * y[3 + c] + x[3 * r + 2] * y[6 + c];
        }
    }
    seg_scan<9>(key, acc);
    if (segment_end(key, lane)) {
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        if (OUT_BSR) out[blk_at(c, (size_t)key, nout)] = acc[c];
        else out[9 * (size_t)key + c] = acc[c];
      }
      if (OUT_BSR && mirror) {   // symmetric target matrix: the block's transpose goes to the mirrored slot
        const int mk = mirror[key];
        if (mk >= 0) {
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) out[blk_at(3 * c + r, (size_t)mk, nout)] = acc[3 * r + c];
        }
      }
    }
  }
}

// rc[a] = sum over the entries e of column a of P_e^T r[row(e)]   (column-ordered copy of P)
// Multi-GPU: only the fine rows [row0, row1) contribute (row1 == 0: all) -- the partial coarse right-hand sides of
// the ranks are then summed by an all-reduce of 3 n_c doubles instead of all-reducing the fine residual.
// The first nb_main workgroups walk the wave groups; columns longer than kLongColumn entries are left to the workgroups
// behind them, ONE WORKGROUP each in the same launch (every thread a few entries, all of them requested at once; wave sums,
// then the wave totals added in a fixed order): a single wave walking such a column stride by stride is a chain of ~70
// dependent round trips (C5's last level: 4 350 entries per column, 109 us), a launch of its own costs 4 us per cycle.
// (block: this workgroup's index within the restriction's part of the launch)
// (S, t_grp = P.t_grp, t_ngrp = P.t_ngrp, nb_main: what the first round of requests needs, from the kernel's leading parameters)
__device__ __forceinline__ void restrict_groups(const PcgScalars* S, const int* __restrict__ t_grp, int t_ngrp, int nb_main,
                                                const PDev& P, const double* __restrict__ r, double* __restrict__ rc,
                                                int row0, int row1, int block) {
  const int lane = threadIdx.x & 63;
  const size_t np = (size_t)P.t_n;
  if (block >= nb_main) {   // a long column
    if (S && S->stop) return;
    __shared__ double sm[kWavesPerBlock][3];
    const int lc = block - nb_main;
    const int gb = P.t_long[2 * lc], ge = P.t_long[2 * lc + 1];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int t = gb + (int)threadIdx.x; t < ge; t += kBlock) {
      const size_t i = (size_t)P.t_row[t];
      if (row1 > 0 && ((int)i < row0 || (int)i >= row1)) continue;
      const double ri[3] = {r[3 * i], r[3 * i + 1], r[3 * i + 2]};
      double b[9];
      load9_pairs(P.t_blk, P.t_blk8, (size_t)t, np, b, P.stream_nt != 0);
      block_tmul_acc(b, ri, acc);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double v = wave_sum(acc[q]);
      if (lane == 0) sm[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      double v = sm[0][threadIdx.x];
      for (int w = 1; w < kWavesPerBlock; ++w) v += sm[w][threadIdx.x];
      rc[3 * (size_t)P.t_col[gb] + threadIdx.x] = v;
    }
    return;
  }
  GroupCursor gc = group_cursor(t_grp, t_ngrp, nb_main, block);
  if (S && S->stop) return;
  for (bool first = true; gc.g < gc.gend; gc.g += gc.gstride, first = false) {
    int gb, ge;
    group_bounds(gc, t_grp, first, gb, ge);
    if (P.t_nlong > 0 && ge - gb > kLongColumn) continue;   // a long column: the workgroups at the end of the grid
    double acc[3] = {0.0, 0.0, 0.0};
    int key = -1 - lane;
    for (int t = gb + lane; t < ge; t += 64) {
      key = P.t_col[t];
      const size_t i = (size_t)P.t_row[t];
      if (row1 > 0 && ((int)i < row0 || (int)i >= row1)) continue;
      const double ri[3] = {r[3 * i], r[3 * i + 1], r[3 * i + 2]};
      double b[9];
      load9_pairs(P.t_blk, P.t_blk8, (size_t)t, np, b, P.stream_nt != 0);
      block_tmul_acc(b, ri, acc);
    }
    seg_scan<3>(key, acc);
    if (segment_end(key, lane)) {
      rc[3 * (size_t)key] = acc[0];
      rc[3 * (size_t)key + 1] = acc[1];
      rc[3 * (size_t)key + 2] = acc[2];
    }
  }
}
__global__ __launch_bounds__(kBlock) void k_restrict_p(const PcgScalars* S, const int* __restrict__ t_grp, int t_ngrp, int nb_main,
                                                       PDev P, const double* __restrict__ r, double* __restrict__ rc, int row0,
                                                       int row1) {
  restrict_groups(S, t_grp, t_ngrp, nb_main, P, r, rc, row0, row1, (int)blockIdx.x);
}
// The folded cycle's two level-0 launches that read the same right-hand side and do not depend on each other -- the
// Jacobi pass of the wave-group kernel (M2 r, workgroups [0, nb_spmv)) and the restriction with P~^T (the workgroups
// behind them) -- as ONE launch: on the graphs that fold level 0 a launch costs more than what it moves.
// (The leading parameters are the Jacobi pass's, the longer chain of the two: Spmv0Head, sgo_device.h.  The restriction finds
// its group array in P: there is no room for it among the preloaded dwords.)
__global__ __launch_bounds__(kBlock, 4) void k_jacobi0_restrict(const PcgScalars* __restrict__ S, const int* __restrict__ grp,
                                                                 const int* __restrict__ grow, const int* __restrict__ gown,
                                                                 const int* __restrict__ gtr, int ulo, int uhi, int nb_spmv, int nb_main,
                                                                 Sym0Dev A, Spmv0Args a, PDev P, double* __restrict__ rc) {
  if ((int)blockIdx.x < nb_spmv) spmv0_groups<S0_JACOBI>(Spmv0Head{S, grp, grow, gown, gtr, ulo, uhi}, A, a, nb_spmv);
  else restrict_groups(S, P.t_grp, P.t_ngrp, nb_main, P, a.b, rc, 0, 0, (int)blockIdx.x - nb_spmv);
}
// r_c = P^T r on the stream
void launch_restrict_p(hipStream_t s, const PDev& P, const double* r, double* rc, const PcgScalars* S, int row0, int row1) {
  const int nb = grid_for(P.t_ngrp, kWavesPerBlock);
  SGO_LAUNCH(k_restrict_p, dim3(nb + P.t_nlong), dim3(kBlock), 0, s, S, (const int*)P.t_grp, P.t_ngrp, nb, P, r, rc, row0, row1);
}

// x_i += sum over the entries e of row i of P_e (c1 u1 + c2 u2)[col(e)]  (+ xadd_i)
// (S, r_grp = P.r_grp, r_ngrp = P.r_ngrp: the first round of requests, leading parameters)
__global__ __launch_bounds__(kBlock) void k_prolong_p(const PcgScalars* S, const int* __restrict__ r_grp, int r_ngrp, int n, PDev P,
                                                      const double* __restrict__ u1, SpmvRatio r1,
                                                      const double* __restrict__ u2, SpmvRatio r2,
                                                      double* __restrict__ x,
                                                      const double* __restrict__ xadd, int row0, int row1) {
  GroupCursor gc = group_cursor(r_grp, r_ngrp, gridDim.x, blockIdx.x);
  if (S && S->stop) return;
  double c1, c2;
  cycle_coefficients(r1, r2, u2 != nullptr, c1, c2);
  // one lane per entry (entries are sorted by fine row), wavefront segmented sum per row
  const int lane = threadIdx.x & 63;
  const size_t np = (size_t)P.r_n;
  for (bool first = true; gc.g < gc.gend; gc.g += gc.gstride, first = false) {
    int gb, ge;
    group_bounds(gc, r_grp, first, gb, ge);
    double acc[3] = {0.0, 0.0, 0.0};
    int key = -1 - lane;
    for (int e = gb + lane; e < ge; e += 64) {
      key = P.row[e];
      if (row1 > 0 && (key < row0 || key >= row1)) {   // multi-GPU: another rank's row
        key = -1 - lane;
        continue;
      }
      double w[3], b[9];
      coarse_operand(u1, u2, c1, c2, 3 * (size_t)P.col[e], w);
      load9_pairs(P.r_blk, P.r_blk8, (size_t)e, np, b, P.stream_nt != 0);
      block_mul_acc(b, w, acc);
    }
    seg_scan<3>(key, acc);
    if (segment_end(key, lane)) {
      const size_t o = 3 * (size_t)key;
      if (xadd) {
        acc[0] += xadd[o]; acc[1] += xadd[o + 1]; acc[2] += xadd[o + 2];
      }
      x[o] += acc[0]; x[o + 1] += acc[1]; x[o + 2] += acc[2];
    }
  }
}

__device__ __forceinline__ int find_sorted(const int* __restrict__ v, int lo, int hi, int key) {   // position of key in v[lo, hi) or -1
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int x = v[mid];
    if (x == key) return mid;
    if (x < key) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

// ------------------------------------------------------------------ folded V-cycle
// One damped block-Jacobi sweep before and after the coarse correction, S = I - w D^-1 A, first sweep from zero:
//   x1 = w D^-1 r;  r1 = r - A x1 = S^T r;  e = P B_c P^T r1;  z = S (x1 + e) + w D^-1 r
//      = [x1 + w D^-1 r1]  +  (S P) B_c (S P)^T r
// i.e. the multiplicative cycle IS an additive one with the transfer operator P~ = S P = P - w D^-1 (A P) -- whose
// blocks follow from A P, which the Galerkin product makes anyway -- and the two-sweep term M2 r = x1 + w D^-1 (r - A x1),
// which does not depend on the coarse correction.  A level then costs two launches on the critical path of the cycle
// (restriction with P~^T, prolongation with P~) instead of four (sweep + residual, restriction, prolongation, sweep):
// on level 0 (small graphs only, see amg_create) the M2 term is the level-0 Jacobi pass -- one pass instead of residual pass +
// sweep --; on the coarser levels it is folded into the prolongation launch (k_up_fold: the row's slots of A and its entries of P~ in one list).
// Same preconditioner in exact arithmetic (B_c: the coarser levels' cycle, recursively the same), symmetric as before
// (restriction and prolongation read the same rounded fp32 values of P~).
struct FoldDev {   // pattern of P~ (= that of A P); arrays addressed by GLOBAL A P entry numbers f (row-owner mode: shifted)
  int f_lo = 0, f_hi = 0;      // entries held (this rank's rows' in row-owner mode)
  const int* row = nullptr;    // fine row of entry f
  const int* col = nullptr;    // coarse column of entry f
  int* ap2p = nullptr;         // entry of P at the same (row, column), -1: none
  int* st_pos = nullptr;       // position of f in column order, 0-based within the entries held
};
struct UpDev {     // levels >= 1: per row its slots of A, then its entries of P~, as ONE row-major list
  int n = 0, ngrp = 0;
  const int* row = nullptr;
  const int* idx = nullptr;    // slot k >= 0, or ~f for entry f of P~
  const int* col = nullptr;    // column of the slot / coarse column of the entry
  const int* grp = nullptr;    // wave groups aligned to rows
};

__global__ __launch_bounds__(kBlock) void k_fold_match(FoldDev F, const int* __restrict__ p_rowptr, const int* __restrict__ p_col,
                                                       unsigned long long* __restrict__ keys) {
  for (int f = F.f_lo + blockIdx.x * kBlock + threadIdx.x; f < F.f_hi; f += gridDim.x * kBlock) {
    const int i = F.row[f], c = F.col[f];
    F.ap2p[f] = find_sorted(p_col, p_rowptr[i], p_rowptr[i + 1], c);
    keys[f - F.f_lo] = ((unsigned long long)(unsigned)c << 32) | (unsigned)(f - F.f_lo);   // (column, row-major rank): sorted = column order
  }
}
__global__ __launch_bounds__(kBlock) void k_fold_unpack(FoldDev F, const unsigned long long* __restrict__ sorted, int* __restrict__ t_row,
                                                        int* __restrict__ t_col) {
  const int nf = F.f_hi - F.f_lo;
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < nf; t += gridDim.x * kBlock) {
    const unsigned long long k = sorted[t];
    const int f = F.f_lo + (int)(unsigned)(k & 0xffffffffull);
    F.st_pos[f] = t;
    t_col[t] = (int)(k >> 32);
    t_row[t] = F.row[f];
  }
}
// ptr[c] = first position of column c in the sorted keys (c = 0 .. nc; ptr[nc] = nf)
__global__ __launch_bounds__(kBlock) void k_fold_colptr(const unsigned long long* __restrict__ sorted, int nf, int nc, int* __restrict__ ptr) {
  for (int c = blockIdx.x * kBlock + threadIdx.x; c <= nc; c += gridDim.x * kBlock) {
    const unsigned long long key = (unsigned long long)(unsigned)c << 32;
    int lo = 0, hi = nf;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sorted[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    ptr[c] = lo;
  }
}
// the wave groups longer than kLongColumn (single long columns): their ranges, in any order (one workgroup each later on); ranges
// holds 2 x ngrp ints
__global__ __launch_bounds__(kBlock) void k_long_groups(const int* __restrict__ grp, int ngrp, int* __restrict__ count, int* __restrict__ ranges) {
  for (int g = blockIdx.x * kBlock + threadIdx.x; g < ngrp; g += gridDim.x * kBlock) {
    const int b = grp[g], e = grp[g + 1];
    if (e - b > kLongColumn) {
      const int q = atomicAdd(count, 1);
      ranges[2 * q] = b;
      ranges[2 * q + 1] = e;
    }
  }
}
// UpDev of a level >= 1: u_ptr[i] = the row's slots of A + its entries of P~ before row i; then the list itself
__global__ __launch_bounds__(kBlock) void k_u_ptr(int n, const int* __restrict__ a_rowptr, const int* __restrict__ ap_rowptr, int* __restrict__ u_ptr) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i <= n; i += gridDim.x * kBlock) u_ptr[i] = a_rowptr[i] + ap_rowptr[i];
}
__global__ __launch_bounds__(kBlock) void k_u_fill(int n, const int* __restrict__ a_rowptr, const int* __restrict__ a_col,
                                                   const int* __restrict__ ap_rowptr, const int* __restrict__ ap_col, const int* __restrict__ u_ptr,
                                                   int* __restrict__ u_row, int* __restrict__ u_idx, int* __restrict__ u_col) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    int q = u_ptr[i];
    for (int k = a_rowptr[i]; k < a_rowptr[i + 1]; ++k, ++q) {
      u_row[q] = i;
      u_idx[q] = k;
      u_col[q] = a_col[k];
    }
    for (int f = ap_rowptr[i]; f < ap_rowptr[i + 1]; ++f, ++q) {
      u_row[q] = i;
      u_idx[q] = ~f;
      u_col[q] = ap_col[f];
    }
  }
}

// P~_f = P_(row, col) - w D_row^-1 (A P)_f : the row-ordered and the column-ordered fp32 copies the folded cycle streams
__global__ __launch_bounds__(kBlock) void k_ptilde_values(FoldDev F, const double* __restrict__ apblk, const double* __restrict__ pblk,
                                                          const double* __restrict__ dinv, double omega, PDev PS) {
  for (int f = F.f_lo + blockIdx.x * kBlock + threadIdx.x; f < F.f_hi; f += gridDim.x * kBlock) {
    const size_t i = (size_t)F.row[f];
    const int e = F.ap2p[f];
    const size_t tp = (size_t)F.st_pos[f];
    const double* di = dinv + 6 * i;
    double a[9], o[9];
    load9(apblk, (size_t)f, a);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o[c] = -omega * (di[0] * a[c] + di[1] * a[3 + c] + di[2] * a[6 + c]);
      o[3 + c] = -omega * (di[1] * a[c] + di[3] * a[3 + c] + di[4] * a[6 + c]);
      o[6 + c] = -omega * (di[2] * a[c] + di[4] * a[3 + c] + di[5] * a[6 + c]);
    }
    if (e >= 0) {
#pragma unroll
      for (int c = 0; c < 9; ++c) o[c] += pblk[9 * (size_t)e + c];
    }
    const sgo_f4 q0 = {(float)o[0], (float)o[1], (float)o[2], (float)o[3]}, q1 = {(float)o[4], (float)o[5], (float)o[6], (float)o[7]};
    sgo_f4* rq = reinterpret_cast<sgo_f4*>(PS.r_blk);
    sgo_f4* tq = reinterpret_cast<sgo_f4*>(PS.t_blk);
    rq[f] = q0;
    rq[(size_t)PS.r_n + f] = q1;
    tq[tp] = q0;
    tq[(size_t)PS.t_n + tp] = q1;
    PS.r_blk8[f] = (float)o[8];
    PS.t_blk8[tp] = (float)o[8];
  }
}

// Level 0: z_i = y_i + sum over the entries f of row i of P~_f (c1 u1 + c2 u2)[col(f)]; optional partials of dotA . z, dotA2 . z
// (P: the view of P~ -- row / col / r_grp / r_blk of the folded operator; single GPU: multi-GPU runs keep level 0 unfolded).
// Workgroups of 1024 threads: the consumer of the dot products re-reduces one partial sum per WORKGROUP in every one of its
// own workgroups, so there should be a few hundred of them.
constexpr int kFoldThreads = 1024;
__global__ __launch_bounds__(kFoldThreads) void k_prolong_fold(const PcgScalars* S, const int* __restrict__ r_grp, int r_ngrp, PDev P,
                                                               const double* __restrict__ u1, SpmvRatio r1,
                                                               const double* __restrict__ u2, SpmvRatio r2, const double* __restrict__ y,
                                                               double* __restrict__ out, const double* __restrict__ dotA,
                                                               const double* __restrict__ dotA2, double* __restrict__ partials) {
  constexpr int NW = kFoldThreads / 64;
  __shared__ double sm[4][NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  GroupCursor gc = group_cursor<NW>(r_grp, r_ngrp, gridDim.x, blockIdx.x);   // (= P.r_grp, P.r_ngrp: leading parameters)
  if (S && S->stop) return;
  double c1 = 1.0, c2 = 0.0;
  // cycle_coefficients (sgo_device.h) with a reduction of its own: 1024 threads, and sm is shared with the dot products below
  if (r1.num || u2) {
    const double* const parts[4] = {r1.num ? r1.den : nullptr, r1.num, (u2 && r2.num) ? r2.den : nullptr, u2 ? r2.num : nullptr};
    const int cnt[4] = {r1.n_den, r1.n_num, r2.n_den, r2.n_num};
    double v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double t = 0.0;
      if (parts[c])
        for (int i = threadIdx.x; i < cnt[c]; i += kFoldThreads) t += parts[c][i];
      t = wave_sum(t);
      if (lane == 0) sm[c][wave] = t;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double t = sm[c][0];
#pragma unroll 1
      for (int k = 1; k < NW; ++k) t += sm[c][k];   // (not unrolled: 64 LDS reads in flight would set the kernel's register count)
      v[c] = t;
    }
    __syncthreads();
    if (r1.num) c1 = cycle_ratio(v[0], v[1]);
    if (u2) c2 = cycle_ratio(v[2], v[3]);
  }
  const size_t np = (size_t)P.r_n;
  double dotacc[2] = {0.0, 0.0};
  for (bool first = true; gc.g < gc.gend; gc.g += gc.gstride, first = false) {
    int gb, ge;
    group_bounds(gc, r_grp, first, gb, ge);
    double acc[3] = {0.0, 0.0, 0.0};
    int key = -1 - lane;
    for (int e = gb + lane; e < ge; e += 64) {
      key = P.row[e];
      double w[3], b[9];
      coarse_operand(u1, u2, c1, c2, 3 * (size_t)P.col[e], w);
      load9_pairs(P.r_blk, P.r_blk8, (size_t)e, np, b, P.stream_nt != 0);
      block_mul_acc(b, w, acc);
    }
    // the row's own term is requested before the scan (one dependent round trip less)
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    if (key >= 0) {
      const size_t o = 3 * (size_t)key;
      y0 = y[o]; y1 = y[o + 1]; y2 = y[o + 2];
    }
    seg_scan<3>(key, acc);
    if (segment_end(key, lane)) {
      const size_t o = 3 * (size_t)key;
      const double o0 = y0 + acc[0], o1 = y1 + acc[1], o2 = y2 + acc[2];
      out[o] = o0; out[o + 1] = o1; out[o + 2] = o2;
      if (dotA) dotacc[0] += dotA[o] * o0 + dotA[o + 1] * o1 + dotA[o + 2] * o2;
      if (dotA2) dotacc[1] += dotA2[o] * o0 + dotA2[o + 1] * o1 + dotA2[o + 2] * o2;
    }
  }
  if (partials) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const double t = wave_sum(dotacc[i]);
      if (lane == 0) sm[i][wave] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        double t = sm[i][0];
#pragma unroll
        for (int k = 1; k < NW; ++k) t += sm[i][k];
        partials[(size_t)i * kMaxPartials + blockIdx.x] = t;
      }
    }
  }
}

// Levels >= 1: out_i = M2 b |_i + sum_f P~_f (c1 u1 + c2 u2)[col(f)],  M2 b = x1 + w D^-1 (b - A x1), x1 = w D^-1 b
// (the operand of a slot (i, j) is made on the fly from b_j and D_j^-1: nothing but b and the coarse solution is read)
__global__ __launch_bounds__(kBlock) void k_up_fold(const PcgScalars* S, const int* __restrict__ grp, int ngrp, BsrDev A, UpDev U,
                                                    PDev PS, const double* __restrict__ b, double omega,
                                                    const double* __restrict__ u1, SpmvRatio r1, const double* __restrict__ u2,
                                                    SpmvRatio r2, double* __restrict__ out, const double* __restrict__ xadd) {
  GroupCursor gc = group_cursor(grp, ngrp, gridDim.x, blockIdx.x);   // (= U.grp, U.ngrp: leading parameters)
  if (S && S->stop) return;
  double c1, c2;
  cycle_coefficients(r1, r2, u2 != nullptr, c1, c2);
  const int lane = threadIdx.x & 63;
  const size_t ns = (size_t)A.nslot, np = (size_t)PS.r_n;
  for (bool first = true; gc.g < gc.gend; gc.g += gc.gstride, first = false) {
    int gb, ge;
    group_bounds(gc, grp, first, gb, ge);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // [0..2] A x1, [3..5] P~ e
    int key = -1 - lane;
    for (int t = gb + lane; t < ge; t += 64) {
      key = U.row[t];
      const int idx = U.idx[t];
      const size_t j = (size_t)U.col[t];
      if (idx >= 0) {
        const size_t k = (size_t)idx;
        const double bj[3] = {b[3 * j], b[3 * j + 1], b[3 * j + 2]};
        double x[3];
        dinv_apply(A.dinv + 6 * j, omega, bj, x);
        const double2* __restrict__ bp = reinterpret_cast<const double2*>(A.blk);
        const double2 p0 = bp[k], p1 = bp[ns + k], p2 = bp[2 * ns + k], p3 = bp[3 * ns + k];
        const double b8 = A.blk[8 * ns + k];
        block_mul_acc(p0, p1, p2, p3, b8, x, acc);
      } else {
        const size_t f = (size_t)(~idx);
        double w[3], q[9];
        coarse_operand(u1, u2, c1, c2, 3 * j, w);
        load9_pairs(PS.r_blk, PS.r_blk8, f, np, q, false);
        block_mul_acc(q, w, acc + 3);
      }
    }
    // the row's own right-hand side and block-diagonal inverse, requested before the scan
    double bi[3] = {0.0, 0.0, 0.0}, di[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (key >= 0) {
      const size_t i = (size_t)key;
      bi[0] = b[3 * i]; bi[1] = b[3 * i + 1]; bi[2] = b[3 * i + 2];
#pragma unroll
      for (int q = 0; q < 6; ++q) di[q] = A.dinv[6 * i + q];
    }
    seg_scan<6>(key, acc);
    if (segment_end(key, lane)) {
      const size_t o = 3 * (size_t)key;
      // x1 + w D^-1 (b - A x1) = w D^-1 (2 b - A x1) evaluated as the cycle does: x1 first, then the residual's sweep
      const double res[3] = {bi[0] - acc[0], bi[1] - acc[1], bi[2] - acc[2]};
      double x[3], sw[3];
      dinv_apply(di, omega, bi, x);
      dinv_apply(di, omega, res, sw);
      double o0 = x[0] + sw[0] + acc[3];
      double o1 = x[1] + sw[1] + acc[4];
      double o2 = x[2] + sw[2] + acc[5];
      if (xadd) {   // (an outer sweep's iterate the folded cycle corrects)
        o0 += xadd[o]; o1 += xadd[o + 1]; o2 += xadd[o + 2];
      }
      out[o] = o0; out[o + 1] = o1; out[o + 2] = o2;
    }
  }
}

// dinv of a coarse level from its diagonal slots (first slot of each row)
// (n = A.n, rowptr = A.rowptr: the first request, leading parameters)
__global__ __launch_bounds__(kBlock) void k_level_dinv(int n, const int* __restrict__ rowptr, BsrDev A) {
  const size_t ns = (size_t)A.nslot;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const int k0 = rowptr[i];
    // symmetrise (the Galerkin sum is symmetric up to rounding)
    const double d[6] = {A.blk[blk_at(0, k0, ns)], 0.5 * (A.blk[blk_at(1, k0, ns)] + A.blk[blk_at(3, k0, ns)]),
                         0.5 * (A.blk[blk_at(2, k0, ns)] + A.blk[blk_at(6, k0, ns)]), A.blk[blk_at(4, k0, ns)],
                         0.5 * (A.blk[blk_at(5, k0, ns)] + A.blk[blk_at(7, k0, ns)]), A.blk[blk_at(8, k0, ns)]};
    dinv_from_block(d, A.dinv + 6 * (size_t)i);
  }
}

// rc[a] = sum_{i in a} T_i^T r_i : one lane per member (members sorted by aggregate), wavefront
// segmented scan per aggregate -- one dependent load chain instead of a serial member loop.
__global__ __launch_bounds__(kBlock) void k_restrict(int ngrp, const int* __restrict__ grp, const int* __restrict__ mem,
                                                     const int* __restrict__ agg, const double* __restrict__ d,
                                                     const double* __restrict__ r, double* __restrict__ rc,
                                                     const PcgScalars* S, int row0, int row1) {
  const int lane = threadIdx.x & 63;
  GroupCursor gc = group_cursor(grp, ngrp, gridDim.x, blockIdx.x);
  if (S && S->stop) return;
  for (bool first = true; gc.g < gc.gend; gc.g += gc.gstride, first = false) {
    int gb, ge;
    group_bounds(gc, grp, first, gb, ge);
    double acc[3] = {0.0, 0.0, 0.0};
    int key = -1 - lane;
    for (int t = gb + lane; t < ge; t += 64) {
      const int i = mem[t];
      key = agg[i];
      if (row1 > 0 && (i < row0 || i >= row1)) continue;
      const double ri[3] = {r[3 * (size_t)i], r[3 * (size_t)i + 1], r[3 * (size_t)i + 2]};
      rigid_t_acc(d[2 * (size_t)i], d[2 * (size_t)i + 1], ri, acc);
    }
    seg_scan<3>(key, acc);
    if (segment_end(key, lane)) {
      rc[3 * (size_t)key] = acc[0];
      rc[3 * (size_t)key + 1] = acc[1];
      rc[3 * (size_t)key + 2] = acc[2];
    }
  }
}

// x_i += T_i (c1 u1 + c2 u2)[agg(i)]   (u2 may be null; scalars as in k_spmv's fused modes)
__global__ __launch_bounds__(kBlock) void k_prolong_add(int n, const int* __restrict__ agg, const double* __restrict__ d,
                                                        const double* __restrict__ u1, SpmvRatio r1,
                                                        const double* __restrict__ u2, SpmvRatio r2,
                                                        double* __restrict__ x, const PcgScalars* S,
                                                        const double* __restrict__ xadd, int row0, int row1) {
  if (S && S->stop) return;
  double c1, c2;
  cycle_coefficients(r1, r2, u2 != nullptr, c1, c2);
  const int ilo = row1 > 0 ? row0 : 0, ihi = row1 > 0 ? row1 : n;
  for (int i = ilo + blockIdx.x * kBlock + threadIdx.x; i < ihi; i += gridDim.x * kBlock) {
    const size_t o = 3 * (size_t)i;
    double w[3];
    coarse_operand(u1, u2, c1, c2, 3 * (size_t)agg[i], w);
    if (xadd) {
      w[0] += xadd[o]; w[1] += xadd[o + 1];
      x[o + 2] += xadd[o + 2];
    }
    rigid_add(d[2 * (size_t)i], d[2 * (size_t)i + 1], w, x + o);
  }
}

// Row-owner mode: the prolongated coarse correction on a LIST of rows -- the copies of the neighbours' boundary rows this rank
// keeps -- so that the post-smoothing sweep finds x1 + P e there without an exchange: the coarse solution is replicated, the
// boundary rows' entries of P travel once per Gauss-Newton iteration (the gathered records P.blk), and x1 = omega Dinv r on these
// rows is kept current by the repeated recurrences (k_update_xr_rows).  The records are rounded to the fp32 values the owner's
// k_prolong_p streams, so only the order of a row's few additions differs from the owner's result.  P.np == 0: tentative
// transfer (aggregate + lever arm, as k_prolong_add).
__global__ __launch_bounds__(kBlock) void k_prolong_rows(int nrows, const int* __restrict__ rows, PDev P, const int* __restrict__ agg,
                                                         const double* __restrict__ d, const double* __restrict__ u1, SpmvRatio r1,
                                                         const double* __restrict__ u2, SpmvRatio r2, double* __restrict__ x,
                                                         const PcgScalars* S) {
  if (S && S->stop) return;
  double c1, c2;
  cycle_coefficients(r1, r2, u2 != nullptr, c1, c2);
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < nrows; t += gridDim.x * kBlock) {
    const size_t i = (size_t)rows[t], o = 3 * i;
    if (P.np > 0) {
      double acc[3] = {0.0, 0.0, 0.0};
      for (int e = P.rowptr[i]; e < P.rowptr[i + 1]; ++e) {
        double w[3], b[9];
        coarse_operand(u1, u2, c1, c2, 3 * (size_t)P.col[e], w);
        const double* bl = P.blk + 9 * (size_t)e;
#pragma unroll
        for (int q = 0; q < 9; ++q) b[q] = (double)(float)bl[q];
        block_mul_acc(b, w, acc);
      }
      x[o] += acc[0]; x[o + 1] += acc[1]; x[o + 2] += acc[2];
    } else {
      double w[3];
      coarse_operand(u1, u2, c1, c2, 3 * (size_t)agg[i], w);
      rigid_add(d[2 * i], d[2 * i + 1], w, x + o);
    }
  }
}

// Coarsest level: explicit dense inverse, recomputed every GN iteration by a blocked in-place
// Gauss-Jordan (SPD, no pivoting) spread over many workgroups: for pivot block K (32 x 32)
//   P = inv(A_KK);  A_Kj <- P A_Kj (j != K);  A_ij <- A_ij - A_iK A_Kj (i, j != K);
//   A_iK <- -A_iK P (i != K);  A_KK <- P.
// The matrix is stored row-major with leading dimension Np = N rounded up to 32 and an identity
// on the padding, so every tile is full.  One launch per pivot block (k_gj_step).
// (64 x 64 blocks with 1024 threads -- half the sequential block steps -- were measured in round 3: much slower, C2 1.71 ->
// 2.77 ms and C4 4.84 -> 5.86 ms per GN iteration: the 64 elimination steps of a pivot block with sixteen waves at every
// barrier cost more than the launches they save.)
constexpr int kGjB = 32;

// The coarse levels' slots are unique per (row, col) (the host lists them so): one thread per slot stores its
// 3x3 block, no accumulation.  M was zeroed by the caller.
__global__ __launch_bounds__(kBlock) void k_dense_fill_unique(BsrDev A, int Np, double* __restrict__ M) {
  const int N = 3 * A.n;
  for (int k = blockIdx.x * kBlock + threadIdx.x; k < A.nslot; k += gridDim.x * kBlock) {
    const int r = A.row[k], c = A.col[k];
    double b[9];
    load_block(A, (size_t)k, b);
#pragma unroll
    for (int e = 0; e < 9; ++e) M[(size_t)(3 * r + e / 3) * Np + 3 * c + e % 3] = b[e];
  }
  for (int i = N + blockIdx.x * kBlock + threadIdx.x; i < Np; i += gridDim.x * kBlock) M[(size_t)i * Np + i] = 1.0;
}
__global__ __launch_bounds__(kBlock) void k_dense_fill(BsrDev A, int Np, double* __restrict__ M) {
  // one thread per block row, slots added in order: level 0 can hold several slots for the same
  // (row, col) -- duplicate edges, and the zero blocks of fixed-column slots that alias the
  // diagonal -- so the fill must accumulate, and a row-exclusive sequential sum keeps it
  // deterministic.  M was zeroed by the caller.
  const int N = 3 * A.n;
  for (int r = blockIdx.x * kBlock + threadIdx.x; r < A.n; r += gridDim.x * kBlock) {
    for (int k = A.rowptr[r]; k < A.rowptr[r + 1]; ++k) {
      const int c = A.col[k];
      double b[9];
      load_block(A, (size_t)k, b);
#pragma unroll
      for (int e = 0; e < 9; ++e) M[(size_t)(3 * r + e / 3) * Np + 3 * c + e % 3] += b[e];
    }
  }
  for (int i = N + blockIdx.x * kBlock + threadIdx.x; i < Np; i += gridDim.x * kBlock) M[(size_t)i * Np + i] = 1.0;
}

// 1 / x by the hardware reciprocal and two Newton steps (the IEEE division is a chain of ~12 dependent instructions on
// the critical path of every elimination step of the pivot-block inverse)
__device__ __forceinline__ double gj_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}

// P = inv(A_KK) by scalar Gauss-Jordan (one workgroup, one thread per matrix element: the element
// lives in a register, only the pivot row / column travel through LDS; 2 barriers per step)
__global__ __launch_bounds__(kGjB * kGjB) void k_gj_pivot(double* __restrict__ M, int Np, int kb, double* __restrict__ P,
                                                          int* __restrict__ fail) {
  __shared__ double a2[2][kGjB][kGjB + 1];   // ping-pong: one barrier per elimination step
  const int i = threadIdx.x / kGjB, j = threadIdx.x % kGjB, base = kb * kGjB;
  double v = M[(size_t)(base + i) * Np + base + j];
  a2[0][i][j] = v;
  __syncthreads();
  // TWO pivots per elimination step (the 2 x 2 pivot block of an SPD matrix is inverted in closed form): 16 barrier-separated
  // steps instead of 32 -- the steps, not their arithmetic, are what the inverse costs
  for (int k = 0; k < kGjB; k += 2) {
    double (*a)[kGjB + 1] = a2[(k >> 1) & 1];
    const double pa = a[k][k], pb = a[k][k + 1], pd = a[k + 1][k + 1];
    const double det = pa * pd - pb * pb;
    if (threadIdx.x == 0 && (!(pa > 0.0) || !(det > 0.0) || !isfinite(det))) *fail = 1;
    const double id = (det != 0.0) ? gj_rcp(det) : 0.0;
    const double p00 = pd * id, p01 = -pb * id, p11 = pa * id;
    const double a0j = a[k][j], a1j = a[k + 1][j], ai0 = a[i][k], ai1 = a[i][k + 1];
    const double t0 = ai0 * p00 + ai1 * p01, t1 = ai0 * p01 + ai1 * p11;
    if (i == k) v = (j == k) ? p00 : ((j == k + 1) ? p01 : p00 * a0j + p01 * a1j);
    else if (i == k + 1) v = (j == k) ? p01 : ((j == k + 1) ? p11 : p01 * a0j + p11 * a1j);
    else if (j == k) v = -t0;
    else if (j == k + 1) v = -t1;
    else v = v - (t0 * a0j + t1 * a1j);
    a2[((k >> 1) + 1) & 1][i][j] = v;
    __syncthreads();
  }
  P[threadIdx.x] = v;
}

// Z = X * Y for 32x32 fp64 tiles held in LDS, on the matrix cores: wave w of the workgroup's four makes the 16x16 quadrant
// (w >> 1, w & 1) in eight v_mfma_f64_16x16x4_f64 steps -- two LDS reads per lane and step, where the scalar loop (one row
// x four columns per thread) read five per k: the tile products of a block step were LDS-bandwidth-bound, ~5 us of its
// 17 with two or three workgroups per CU.  Operand lane maps: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col =
// lane & 15]; result register q of a lane is row (lane >> 4) + 4 q, column lane & 15.
typedef double sgo_d4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void tile_mm(const double (*X)[kGjB + 1], const double (*Y)[kGjB + 1], double (*Z)[kGjB + 1]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i0 = 16 * (w >> 1), j0 = 16 * (w & 1), lr = lane & 15, lk = lane >> 4;
  sgo_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < kGjB / 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[i0 + lr][4 * s + lk], Y[4 * s + lk][j0 + lr], acc, 0, 0, 0);
#pragma unroll
  for (int q = 0; q < 4; ++q) Z[i0 + lk + 4 * q][j0 + lr] = acc[q];
}

// One Gauss-Jordan block step K = kb is ONE launch over all 32x32 tiles, reading the matrix of the previous
// step (Min) and writing the next one (Mout) -- ping-pong, so that no tile is read after another workgroup
// has overwritten it and no panel kernel has to run first:
//   (K, K)            <- P                       (P = inv(A_KK), made by the previous launch)
//   (K, j), j != K    <- P A_Kj
//   (i, K), i != K    <- -A_iK P
//   (i, j) elsewhere  <- A_ij - A_iK (P A_Kj)    (the row-panel product recomputed per tile: two tile
//                                                 products instead of one buy half the launches)
// and the workgroup that finishes the next diagonal block (K+1, K+1) inverts it in LDS straight away and
// leaves it in Pout.  The 32 elimination steps of that inverse are the critical path of the whole inversion
// (one sequential 32x32 inverse per block step), so they ping-pong between two LDS tiles: step k reads tile
// k & 1 and writes the other one, ONE barrier per step.
__global__ __launch_bounds__(kBlock) void k_gj_step(const double* __restrict__ Min, double* __restrict__ Mout, int Np, int kb,
                                                    const double* __restrict__ Pin, double* __restrict__ Pout,
                                                    int* __restrict__ fail) {
  __shared__ double X[kGjB][kGjB + 1], Y[kGjB][kGjB + 1], Z[kGjB][kGjB + 1];
  const int t = threadIdx.x, K0 = kb * kGjB;
  const int bj = blockIdx.x, bi = blockIdx.y;
  const int r = t >> 3, c0 = (t & 7) * 4;
  double v[4];
  double* dst = Mout + (size_t)(bi * kGjB + r) * Np + bj * kGjB + c0;
  if (bi == kb && bj == kb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = Pin[r * kGjB + c0 + q];
    return;
  }
  // Everything this tile reads from global memory is requested up front -- the operands of the first product, the
  // column-panel tile of the second and the tile itself -- so that a block step is ONE memory round trip deep instead
  // of three (the step's launch is a dependent chain on the critical path of the whole inversion).
  const bool general = bi != kb && bj != kb;
  double x1[4], y1[4], x2[4] = {0, 0, 0, 0}, sv[4] = {0, 0, 0, 0};
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int e = t + m * kBlock, i = e / kGjB, j = e % kGjB;
    if (bj == kb) {
      x1[m] = Min[(size_t)(bi * kGjB + i) * Np + K0 + j];
      y1[m] = Pin[e];
    } else {
      x1[m] = Pin[e];
      y1[m] = Min[(size_t)(K0 + i) * Np + bj * kGjB + j];
    }
    if (general) x2[m] = Min[(size_t)(bi * kGjB + i) * Np + K0 + j];
  }
  if (general) {
    const double* src = Min + (size_t)(bi * kGjB + r) * Np + bj * kGjB + c0;
#pragma unroll
    for (int q = 0; q < 4; ++q) sv[q] = src[q];
  }
  // first product: Z = P A_Kj (row panel and general tiles) or A_iK P (column panel)
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int e = t + m * kBlock;
    X[e / kGjB][e % kGjB] = x1[m];
    Y[e / kGjB][e % kGjB] = y1[m];
  }
  __syncthreads();
  tile_mm(X, Y, Z);
  __syncthreads();
  if (bi == kb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = Z[r][c0 + q];
    return;
  }
  if (bj == kb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = -Z[r][c0 + q];
    return;
  }
  // general tile: A_ij - A_iK (P A_Kj): the second product's right operand is Z as it lies; X takes A_iK, Y the product
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int e = t + m * kBlock;
    X[e / kGjB][e % kGjB] = x2[m];
  }
  __syncthreads();
  tile_mm(X, Z, Y);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[q] = v[q] = sv[q] - Y[r][c0 + q];
  if (bi != kb + 1 || bj != kb + 1) return;
  // next pivot block: Pout = inv(A_K'K') by scalar Gauss-Jordan
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) X[r][c0 + q] = v[q];
  __syncthreads();
  for (int k = 0; k < kGjB; k += 2) {   // two pivots per step (see k_gj_pivot)
    double (*rd)[kGjB + 1] = ((k >> 1) & 1) ? Y : X;
    double (*wr)[kGjB + 1] = ((k >> 1) & 1) ? X : Y;
    const double pa = rd[k][k], pb = rd[k][k + 1], pd = rd[k + 1][k + 1];
    const double ar0 = rd[r][k], ar1 = rd[r][k + 1];
    double a0c[4], a1c[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      a0c[q] = rd[k][c0 + q];
      a1c[q] = rd[k + 1][c0 + q];
    }
    const double det = pa * pd - pb * pb;
    if (t == 0 && (!(pa > 0.0) || !(det > 0.0) || !isfinite(det))) *fail = 1;
    const double id = (det != 0.0) ? gj_rcp(det) : 0.0;
    const double p00 = pd * id, p01 = -pb * id, p11 = pa * id;
    const double t0 = ar0 * p00 + ar1 * p01, t1 = ar0 * p01 + ar1 * p11;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + q;
      if (r == k) v[q] = (c == k) ? p00 : ((c == k + 1) ? p01 : p00 * a0c[q] + p01 * a1c[q]);
      else if (r == k + 1) v[q] = (c == k) ? p01 : ((c == k + 1) ? p11 : p01 * a0c[q] + p11 * a1c[q]);
      else if (c == k) v[q] = -t0;
      else if (c == k + 1) v[q] = -t1;
      else v[q] = v[q] - (t0 * a0c[q] + t1 * a1c[q]);
      wr[r][c0 + q] = v[q];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) Pout[r * kGjB + c0 + q] = v[q];
}

// x = inv * b : one wave per row (inv is symmetric; row reads are coalesced)
__global__ __launch_bounds__(kBlock) void k_dense_apply(int N, int Np, const double* __restrict__ inv,
                                                       const double* __restrict__ b, double* __restrict__ x,
                                                       const PcgScalars* S) {
  const int lane = threadIdx.x & 63;
  int i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  // the first row's first stride is requested before the stop flag is waited for
  double a0 = 0.0, b0 = 0.0;
  if (i < N && lane < N) {
    a0 = inv[(size_t)i * Np + lane];
    b0 = b[lane];
  }
  if (S && S->stop) return;
  for (bool first = true; i < N; i += gridDim.x * kWavesPerBlock, first = false) {
    const double* row = inv + (size_t)i * Np;
    double s = first ? a0 * b0 : 0.0;
    // four strides per trip, all eight loads requested before the first product (as a plain loop the compiler waits for
    // every stride's pair of loads before it requests the next: eleven dependent round trips for N = 750)
    int j = lane + (first ? 64 : 0);
    for (; j + 192 < N; j += 256) {
      const double r0 = row[j], r1 = row[j + 64], r2 = row[j + 128], r3 = row[j + 192];
      const double c0 = b[j], c1 = b[j + 64], c2 = b[j + 128], c3 = b[j + 192];
      s += r0 * c0;
      s += r1 * c1;
      s += r2 * c2;
      s += r3 * c3;
    }
    {
      const bool h0 = j < N, h1 = j + 64 < N, h2 = j + 128 < N;
      const double r0 = h0 ? row[j] : 0.0, r1 = h1 ? row[j + 64] : 0.0, r2 = h2 ? row[j + 128] : 0.0;
      const double c0 = h0 ? b[j] : 0.0, c1 = h1 ? b[j + 64] : 0.0, c2 = h2 ? b[j + 128] : 0.0;
      s += r0 * c0;
      s += r1 * c1;
      s += r2 * c2;
    }
    s = wave_sum(s);
    if (lane == 0) x[i] = s;
  }
}

// partials[0][blk] = sum z.a ; partials[1][blk] = sum z.b (b optional)
__global__ __launch_bounds__(kBlock) void k_dots2(int n, const double* __restrict__ z, const double* __restrict__ a,
                                                  const double* __restrict__ b, double* __restrict__ partials,
                                                  const PcgScalars* S) {
  if (S && S->stop) return;
  double acc[2] = {0.0, 0.0};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    acc[0] += z[i] * a[i];
    if (b) acc[1] += z[i] * b[i];
  }
  block_sum_store<2>(acc, partials, kMaxPartials);
}

// --------------------------------------------------------------------------------- product lists on the device
// The patterns of P, A P and P^T A P come from the host (a per-row sort of a few distinct columns each); the lists of
// block products behind every entry -- 13 M + 3 M triples on C4 level 0, the bulk of the symbolic phase's time and of
// the set-up's upload -- are made here from the patterns: one thread per TARGET entry walks its candidates in the order
// the host lists them (A P: the slots k of row i in ascending order, each contributing the entry of P row col(k) in
// column c if it has one; P^T A P: the entries t of column a of P in ascending order, each contributing the entry of
// A P row row(t) in column c) -- first counting, then, after a prefix sum over the targets, writing.
struct ApPattern {
  int f_lo = 0;                    // targets [f_lo, nap) are listed (row-owner mode: this rank's rows' entries; the arrays
                                   // indexed by a target are then allocated for that range and shifted)
  int nap = 0;
  const int* ap_row = nullptr;     // [nap] fine row of target f
  const int* ap_col = nullptr;     // [nap] coarse column of target f (ascending within a row)
  const int* ap_rowptr = nullptr;  // [n + 1]
};
// Eight lanes per target: lane q of a target's group takes the candidates q, q + 8, ... of the walk, the matches of one
// round are ranked by a ballot (candidate order = lane order within a round), so the list keeps the host's order while
// the walk -- a chain of dependent index loads and a binary search per candidate -- is eight times shorter.
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_ap_list(ApPattern ap, const int* __restrict__ a_rowptr, const int* __restrict__ a_col,
                                                    const int* __restrict__ p_rowptr, const int* __restrict__ p_col,
                                                    int* __restrict__ cnt_or_ptr, int* __restrict__ la, int* __restrict__ lb,
                                                    int* __restrict__ lt) {
  const int lane = threadIdx.x & 63, sub = lane & 7, g8 = lane >> 3;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), nwaves = gridDim.x * kWavesPerBlock;
  for (int f0 = ap.f_lo + wave * 8; f0 < ap.nap; f0 += nwaves * 8) {
    const int f = f0 + g8;
    const bool valid = f < ap.nap;
    const int i = valid ? ap.ap_row[f] : 0, c = valid ? ap.ap_col[f] : 0;
    int k = valid ? a_rowptr[i] + sub : 0;
    const int kend = valid ? a_rowptr[i + 1] : 0;
    int out = (FILL && valid) ? cnt_or_ptr[f] : 0;
    while (__any(k < kend)) {
      int e = -1;
      if (k < kend) {
        const int j = a_col[k];
        e = find_sorted(p_col, p_rowptr[j], p_rowptr[j + 1], c);
      }
      const unsigned long long m = __ballot(e >= 0);
      const unsigned sm = (unsigned)(m >> (8 * g8)) & 0xFFu;
      if (FILL && e >= 0) {
        const int pos = out + __popc(sm & ((1u << sub) - 1u));
        la[pos] = k;
        lb[pos] = e;
        lt[pos] = f;
      }
      out += __popc(sm);
      k += 8;
    }
    if (!FILL && valid && sub == 0) cnt_or_ptr[f] = out;
  }
}
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_rap_list(int nslot_c, const int* __restrict__ c_row, const int* __restrict__ c_col,
                                                     const int* __restrict__ t_ptr, const int* __restrict__ t_row,
                                                     const int* __restrict__ t_idx, ApPattern ap, int* __restrict__ cnt_or_ptr,
                                                     int* __restrict__ la, int* __restrict__ lb, int* __restrict__ lt) {
  const int lane = threadIdx.x & 63, sub = lane & 7, g8 = lane >> 3;
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), nwaves = gridDim.x * kWavesPerBlock;
  for (int s0 = wave * 8; s0 < nslot_c; s0 += nwaves * 8) {
    const int sl = s0 + g8;
    const bool valid = sl < nslot_c;
    const int a = valid ? c_row[sl] : 0, c = valid ? c_col[sl] : 0;
    const bool upper = valid && c >= a;   // upper triangle only: the lower one is mirrored by the numeric kernel
    int t = upper ? t_ptr[a] + sub : 0;
    const int tend = upper ? t_ptr[a + 1] : 0;
    int out = (FILL && valid) ? cnt_or_ptr[sl] : 0;
    while (__any(t < tend)) {
      int f = -1;
      if (t < tend) {
        const int i = t_row[t];
        f = find_sorted(ap.ap_col, ap.ap_rowptr[i], ap.ap_rowptr[i + 1], c);
      }
      const unsigned long long m = __ballot(f >= 0);
      const unsigned sm = (unsigned)(m >> (8 * g8)) & 0xFFu;
      if (FILL && f >= 0) {
        const int pos = out + __popc(sm & ((1u << sub) - 1u));
        la[pos] = t_idx[t];
        lb[pos] = f;
        lt[pos] = sl;
      }
      out += __popc(sm);
      t += 8;
    }
    if (!FILL && valid && sub == 0) cnt_or_ptr[sl] = out;
  }
}
// Exclusive prefix sum of n ints in place (v[n] receives the total): blocks of kScanChunk elements summed, the block
// sums scanned by one workgroup, the blocks rescanned with their offsets.
constexpr int kScanChunk = 4096;
__global__ __launch_bounds__(kBlock) void k_scan_sums(const int* __restrict__ v, int n, int* __restrict__ sums) {
  __shared__ int sm[kBlock];
  const int base = blockIdx.x * kScanChunk;
  int acc = 0;
  for (int q = threadIdx.x; q < kScanChunk && base + q < n; q += kBlock) acc += v[base + q];
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = sm[0];
}
__global__ __launch_bounds__(kBlock) void k_scan_top(int* __restrict__ sums, int nb) {   // one workgroup; sums[nb] = total
  __shared__ int sm[kBlock];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += kBlock) {
    const int q = base + threadIdx.x;
    const int x = q < nb ? sums[q] : 0;
    sm[threadIdx.x] = x;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {   // Hillis-Steele inclusive scan
      const int y = (int)threadIdx.x >= off ? sm[threadIdx.x - off] : 0;
      __syncthreads();
      sm[threadIdx.x] += y;
      __syncthreads();
    }
    if (q < nb) sums[q] = carry + sm[threadIdx.x] - x;
    __syncthreads();
    if (threadIdx.x == 0) carry += sm[kBlock - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}
__global__ __launch_bounds__(kBlock) void k_scan_apply(int* __restrict__ v, int n, const int* __restrict__ sums, int nb) {
  // kScanChunk = 16 per thread: every thread scans its 16 consecutive elements, the threads' totals are scanned in LDS
  __shared__ int sm[kBlock];
  const int base = blockIdx.x * kScanChunk + threadIdx.x * (kScanChunk / kBlock);
  int x[kScanChunk / kBlock], tot = 0;
#pragma unroll
  for (int q = 0; q < kScanChunk / kBlock; ++q) {
    x[q] = base + q < n ? v[base + q] : 0;
    tot += x[q];
  }
  sm[threadIdx.x] = tot;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {
    const int y = (int)threadIdx.x >= off ? sm[threadIdx.x - off] : 0;
    __syncthreads();
    sm[threadIdx.x] += y;
    __syncthreads();
  }
  int run = sums[blockIdx.x] + sm[threadIdx.x] - tot;
#pragma unroll
  for (int q = 0; q < kScanChunk / kBlock; ++q) {
    if (base + q < n) v[base + q] = run;
    run += x[q];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) v[n] = sums[nb];
}
// The same in ONE launch of one workgroup for short lists: every thread scans a contiguous piece, the pieces' totals are scanned in LDS.
constexpr int kScanSmall = 32768;
__global__ __launch_bounds__(1024) void k_scan_small(int* __restrict__ v, int n) {
  __shared__ int sm[1024];
  const int per = (n + 1023) / 1024, b = threadIdx.x * per, e = min(n, b + per);
  int tot = 0;
  for (int q = b; q < e; ++q) tot += v[q];
  sm[threadIdx.x] = tot;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int y = (int)threadIdx.x >= off ? sm[threadIdx.x - off] : 0;
    __syncthreads();
    sm[threadIdx.x] += y;
    __syncthreads();
  }
  int run = sm[threadIdx.x] - tot;
  for (int q = b; q < e; ++q) {
    const int x = v[q];
    v[q] = run;
    run += x;
  }
  if (threadIdx.x == 1023) v[n] = sm[1023];
}
// Wave groups over the segments [ptr[f], ptr[f+1]): whole segments packed up to 64 items, a longer segment its own group (the rule
// of the level-0 row groups in sgo_structure.cpp), applied independently to chunks of kGroupChunk segments -- a chunk starts a new
// group; one thread per chunk keeps the serial walk short.  A group is recorded by its start; a list is closed by its total.  The
// grouping never changes WHICH terms a segmented sum has, only their association order inside the wavefront segmented scan (its DPP
// steps are tied to the lanes' positions) -- which is why a level's lists are grouped here and nowhere else, whichever producer made
// its patterns (tests/test_gpu_device_setup.py: the two hierarchies are bit-identical).
// All the lists of a level in two launches (GroupBatch, below): the lists' chunks are numbered through, every list followed by one
// pseudo-chunk that holds its closing element; pass 1 counts a chunk's groups, pass 2 (after a prefix sum) writes them.
constexpr int kGroupChunk = 256;
constexpr int kMaxGroupJobs = 12;
struct GroupJobsDev {
  const int* ptr[kMaxGroupJobs];
  int nseg[kMaxGroupJobs];
  int total[kMaxGroupJobs];
  int chunk0[kMaxGroupJobs + 1];   // first global chunk of list j (its pseudo-chunk is chunk0[j + 1] - 1)
  int njobs;
};
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_group_jobs(GroupJobsDev J, int* __restrict__ cnt_or_off, int* __restrict__ out) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= J.chunk0[J.njobs]) return;
  int j = 0;
  while (c >= J.chunk0[j + 1]) ++j;
  const int local = c - J.chunk0[j];
  if (c == J.chunk0[j + 1] - 1) {   // the list's closing element
    if (FILL) out[cnt_or_off[c]] = J.total[j];
    else cnt_or_off[c] = 1;
    return;
  }
  const int* __restrict__ ptr = J.ptr[j];
  const int nseg = J.nseg[j], s0 = local * kGroupChunk, s1 = min(nseg, s0 + kGroupChunk);
  int o = FILL ? cnt_or_off[c] : 0, cur = 0, start = ptr[s0];
  bool open = false;
  for (int f = s0; f < s1; ++f) {
    const int b = ptr[f], len = ptr[f + 1] - b;
    if (open && cur + len > 64) {
      if (FILL) out[o] = start;
      ++o;
      open = false;
      cur = 0;
    }
    if (!open) {
      start = b;
      open = true;
    }
    cur += len;
    if (cur >= 64) {
      if (FILL) out[o] = start;
      ++o;
      open = false;
      cur = 0;
    }
  }
  if (open) {
    if (FILL) out[o] = start;
    ++o;
  }
  if (!FILL) cnt_or_off[c] = o;
}
__global__ void k_gather_ints(const int* __restrict__ src, GroupJobsDev J, int* __restrict__ dst) {
  const int j = threadIdx.x;
  if (blockIdx.x == 0 && j <= J.njobs) dst[j] = src[J.chunk0[j]];
}

// --------------------------------------------------------------------------------- host
template <class T>
T* dev_alloc(DevArena* pool, size_t count) {
  return (T*)pool->take(std::max<size_t>(count, 1) * sizeof(T));
}
template <class T>
T* dev_upload(DevArena* pool, const std::vector<T>& v, hipStream_t s) {
  T* p = dev_alloc<T>(pool, v.size());
  if (p && !v.empty()) hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
  return p;
}

int* dev_upload(DevArena* pool, const UVec& v, hipStream_t s) {
  int* d = dev_alloc<int>(pool, v.n);
  if (d && v.n) hipMemcpyAsync(d, v.p, v.n * sizeof(int), hipMemcpyHostToDevice, s);
  return d;
}

}  // namespace

// one level of the hierarchy on the device
struct AmgLevel {
  BsrDev A;                 // operator of this level (level 0 aliases the context's matrix)
  int spmv_grid = 0;
  // transfer to the next level (absent on the coarsest)
  int nc = 0;
  int* agg = nullptr;
  int* mem_ptr = nullptr;
  int* mem = nullptr;
  int* mem_grp = nullptr;   // wave groups over the member list, aligned to aggregates
  int mem_ngrp = 0;
  double* pos = nullptr;    // [n][2]
  double* d = nullptr;      // [n][2] lever arms
  GalerkinMap gal;
  bool smoothed = false;    // transfer by the smoothed prolongator P (below) instead of the tentative one
  PDev P;
  // folded cycle (see "folded V-cycle" above): the transfer operator P~ = (I - w D^-1 A) P as a PDev VIEW (row / col /
  // r_* / t_* of P~'s pattern, the one of A P), its pattern bookkeeping, and on levels >= 1 the merged list of k_up_fold
  bool fold = false;
  PDev PS;
  FoldDev F;
  UpDev U;
  // work vectors [n][3]
  double *xs = nullptr, *rs = nullptr;                     // smoother state of the cycle
  double* tR = nullptr;                                    // second residual buffer of multi-sweep smoothing
  double *bk = nullptr, *xk = nullptr, *z1 = nullptr, *z2 = nullptr, *q = nullptr;  // K-cycle FCG (levels >= 1)
  double *bk2 = nullptr, *p2 = nullptr, *q2 = nullptr;     // residual after the first FCG step; second direction; A p2
  double *pA = nullptr, *pB = nullptr, *pC = nullptr;      // [2][kMaxPartials] each
  int gA = 0, gB = 0, gC = 0;   // partial sums the last fcg() left in pA / pB / pC (fixed by the level's size; read by the test hook only)
};

// Level 0 of a multi-GPU run (the coarser levels are replicated on every rank), as one value:
//   single     one GPU: every unit, every row;
//   allreduce  the cycle's two level-0 passes evaluate the work units [u0, u1) (= the rows [row0, row1)) only; the ranks' partial
//              coarse right-hand sides are summed over `comm`, the post-smoothing pass's result is summed as a whole -- or, with
//              `part`, all-gathered by rank slices;
//   owner      row-owner mode (sgo_internal.h): all level-0 work on the owned rows of the partition `part`, boundary exchanges.
// A collective that fails is recorded here (the cycle is captured into a graph and has no way to return it): amg_comm_failed.
struct Shard0 {
  enum Mode { single, allreduce, owner } mode = single;
  int u0 = 0, u1 = 0, row0 = 0, row1 = 0;   // (0, 0: all)
  int G = 1;                        // owner: the ranks that share the level-0 passes (the profile books 1 / G of their bytes)
  Comm* comm = nullptr;             // sums over the ranks (rank emulation, sgo_debug_set_shard: no live communicator, a no-op)
  const HaloDev* part = nullptr;    // owner: the partition; allreduce: the rank slices product vectors are gathered by (optional)
  bool failed = false;
  void reduce(hipStream_t s, double* buf, size_t count) {   // in-place sum over the ranks
    std::string e;
    if (comm && !comm->allreduce_f64(buf, count, s, &e)) failed = true;
  }
  void exchange(hipStream_t s, double* data, int width, const int* idx, int idx_max) {   // owner: records of the boundary rows
    std::string e;
    if (comm && !halo_exchange(*part, s, data, width, idx, idx_max, HaloScalars(), &e)) failed = true;
  }
  void gather(hipStream_t s, double* vec) {   // every rank's slice of a [n][3] vector to every rank
    std::string e;
    if (!halo_gather_slices(*part, s, vec, 3, &e)) failed = true;
  }
};

struct Amg {
  AmgConfig cfg;
  AmgProf prof;
  Sym0Dev S0;               // level-0 operator in symmetric storage (lv[0].A is its logical view)
  Tile0Dev T0;              // ... and its tile view
  Shard0 shard;
  long long level0_bytes = 0;   // device bytes of the level-0 transfer data (P blocks, A P blocks, product lists)
  DevArena* pool = nullptr;   // the caller's arena (not owned)
  std::vector<AmgLevel> lv;
  const double* d_poses = nullptr;
  const int* d_free_id = nullptr;
  int kdepth = 1 << 20;  // levels <= kdepth use the K-cycle (two FCG steps), deeper ones a V-cycle (amg_create: AmgConfig::kdepth)
  // Levels <= this take two FCG steps, deeper K-cycle levels one.  Two steps everywhere visit level l 2^l times:
  // on hierarchies of six levels (C4 with 5 % random closures: 100k -> 11k -> 2.5k -> 897 -> 627 -> 1) that is ~150
  // coarse launches per PCG iteration.  Two steps on level 1 only keep the PCG counts within 3-9 % (C4r 580 -> 597
  // over optimize(20)) at a third of the launches: C4r 22.5 -> 10.8 ms per GN iteration, 30k-pose graphs 1.2-1.3 x
  // (scripts/kcycle_sweep.py, profiles/r02_kcycle_sweep.txt); one step everywhere is faster still on average but
  // needs 40-50 % more iterations and doubles the worst solve.
  int fcg2_depth = 1;   // (amg_create: AmgConfig::fcg2_depth)
  // coarsest dense inverse (row-major, leading dimension Np = N rounded up to 32)
  int N = 0, Np = 0;
  double* inv = nullptr;
  double* inv0 = nullptr;  // ping-pong buffers of the block Gauss-Jordan; `inv` is the one the last step writes
  double* inv1 = nullptr;
  double* gjP[2] = {nullptr, nullptr};   // [32][32] inverse of the current / next pivot block
  int* d_fail = nullptr;
  std::string desc;
  AmgKeptAgg kept;   // host copies of every level's aggregates (a rebuild may keep them: AmgConfig::keep_agg)
};

namespace {

struct Scope {
  const AmgProf& p;
  Scope(const AmgProf& p_, int kid, double bytes) : p(p_) {
    if (p.begin) p.begin(p.user, kid, bytes);
  }
  ~Scope() {
    if (p.end) p.end(p.user);
  }
};

double bytes_spmv(const BsrDev& A) { return 80.0 * A.nslot + 48.0 * A.n; }

// Values of the operator of level l+1 from those of level l (lever arms L.d must be current):
// tentative prolongator: one Galerkin pass; smoothed: P values, AP = A P, A_c = P^T AP.
// Multi-GPU, row-owner mode (level 0 only; the coarser levels are replicated): every rank makes the entries of P and of
// A P of its own fine rows -- A P needs the P rows of the neighbours' boundary rows: one exchange of 72-byte records --
// and its rows' share of P^T A P; the ranks' partial coarse operators are summed by an all-reduce of the level-1 blocks.
void launch_coarse_operator(Amg* m, hipStream_t s, AmgLevel& L, AmgLevel& C, bool level0) {
  Shard0& sh = m->shard;
  const bool own = level0 && sh.mode == Shard0::owner;
  const int row0 = own ? sh.row0 : 0, row1 = own ? sh.row1 : 0;
  if (!L.smoothed) {
    {
      Scope sc(m->prof, level0 ? K_GALERKIN0 : K_GALERKIN, (72.0 + 16.0 + 32.0) * L.A.nslot + 72.0 * C.A.nslot);
      SGO_LAUNCH(k_galerkin, dim3(grid_for(L.gal.ngrp, kWavesPerBlock)), dim3(kBlock), 0, s, L.A, C.A, L.gal, L.d, row0, row1);
    }
    if (own) sh.reduce(s, C.A.blk, 9 * (size_t)C.A.nslot);
    return;
  }
  PDev& P = L.P;
  if (P.dF) {   // filtered smoothing: the diagonal blocks of the strong connections' operator first
    Scope sc(m->prof, level0 ? K_SA_P0 : K_SA_P, (72.0 + 9.0 + 16.0) * L.A.nslot + 144.0 * L.A.n);
    SGO_LAUNCH(k_filtered_diag, dim3(grid_for(P.f_ngrp, kWavesPerBlock)), dim3(kBlock), 0, s, L.A, (const int*)P.f_grp, P.f_ngrp, P.strong,
               (const double*)L.pos, P.dF, P.dinvF, row0, row1);
  }
  {
    Scope sc(m->prof, level0 ? K_SA_P0 : K_SA_P, (72.0 + 12.0 + 16.0) * P.val.n + 80.0 * P.r_n);
    SGO_LAUNCH(k_p_values, dim3(grid_for(P.val.ngrp, kWavesPerBlock)), dim3(kBlock), 0, s, (const int*)P.val.grp, P.val.ngrp, L.A, P,
               (const int*)L.agg, (const double*)L.d, m->cfg.omega_p, row0, row1);
  }
  if (own) sh.exchange(s, P.blk, 9, sh.part->pent, sh.part->pemax);
  {
    Scope sc(m->prof, level0 ? K_SA_AP0 : K_SA_AP, 156.0 * P.ap.n + 72.0 * P.nap);
    SGO_LAUNCH((k_block_products<true, false, false>), dim3(grid_for(P.ap.ngrp, kWavesPerBlock)), dim3(kBlock), 0, s,
               (const int*)P.ap.grp, P.ap.ngrp, P.ap, L.A, (const double*)nullptr, (const double*)P.blk, P.apblk, (size_t)P.nap, (const int*)nullptr,
               (const int*)L.A.row, row0, P.local_lists ? 0 : row1, 0);   // (local lists hold this rank's products only: no filter)
  }
  if (L.fold) {
    Scope sc(m->prof, level0 ? K_PTILDE0 : K_PTILDE, (72.0 + 36.0 + 72.0 + 12.0 + 72.0) * (L.F.f_hi - L.F.f_lo));
    SGO_LAUNCH(k_ptilde_values, dim3(grid_for((long long)(L.F.f_hi - L.F.f_lo), kBlock)), dim3(kBlock), 0, s, L.F, (const double*)P.apblk,
               (const double*)P.blk, (const double*)L.A.dinv, m->cfg.omega, L.PS);
  }
  if (P.local_lists) hipMemsetAsync(C.A.blk, 0, sizeof(double) * 9 * (size_t)C.A.nslot, s);   // targets this rank has no product for
  {
    Scope sc(m->prof, level0 ? K_SA_RAP0 : K_SA_RAP, 156.0 * P.rap.n + 72.0 * C.A.nslot);
    SGO_LAUNCH((k_block_products<false, true, true>), dim3(grid_for(P.rap.ngrp, kWavesPerBlock)), dim3(kBlock), 0, s,
               (const int*)P.rap.grp, P.rap.ngrp, P.rap, BsrDev(), (const double*)P.blk, (const double*)P.apblk, C.A.blk, (size_t)C.A.nslot, (const int*)P.rap_mirror,
               (const int*)P.row, row0, P.local_lists ? 0 : row1, 1);
  }
  if (own) sh.reduce(s, C.A.blk, 9 * (size_t)C.A.nslot);
}

// The coarse solution of level l as seen by its parent: xk (dense level) or the flexible-CG
// combination c1 z1 + c2 p2 whose scalars are ratios of the partial sums the FCG SpMVs left
// in pA / pB (never materialised: the consumers apply it on the fly).
struct CoarseSol {
  const double *u1 = nullptr, *u2 = nullptr;
  SpmvRatio c1, c2;
};
// The K-cycle's second step: the cycle runs for rhs - c sub, which its first launch forms on the fly and stores to `out`.
struct RhsSub { const double* sub; SpmvRatio c; double* out; };
// Partial sums of vec . z (and vec2 . z) asked of the cycle's last launch (vec == nullptr: none).
struct DotReq { const double *vec = nullptr, *vec2 = nullptr; double* parts = nullptr; };

// The form of level l's cycle and its sweeps per side.  Folded (see "folded V-cycle"): one sweep per side, inside the transfer P~.
// Two sweeps per side = one explicit sweep around the folded cycle: S E S with E the folded cycle's error propagator.
struct CycleForm { int nu; enum { unfolded, folded, folded_in_two_sweeps } kind; };
CycleForm cycle_form(const Amg* m, int l, bool rhs_sub, bool dots) {
  const AmgLevel& L = m->lv[l];
  CycleForm f{(l > 0 && L.tR && L.smoothed) ? std::max(1, m->cfg.nu_coarse) : 1, CycleForm::unfolded};
  if (!L.fold || rhs_sub) return f;
  if (l == 0) {   // multi-GPU runs keep level 0 unfolded
    if (m->shard.mode == Shard0::single) f.kind = CycleForm::folded;
  } else if (!dots) {   // a cycle that must deliver dot products on a level >= 1 is unfolded
    if (f.nu == 1) f.kind = CycleForm::folded;
    if (f.nu == 2) f.kind = CycleForm::folded_in_two_sweeps;
  }
  return f;
}

// Whether the set-up folds level l, whose share of A P (the pattern of P~) holds nf entries.  Level 0 is folded only where it is itself
// launch-bound: P~ has the pattern of A P, twice the entries of P, and on large graphs streaming it twice per cycle costs what the
// saved launch and pass bring -- C4: restriction + prolongation 14 + 20 us with P~ against 11 + 9 us with P.  Multi-GPU row-owner
// runs keep level 0 unfolded as well.  (A level with too many long columns is not folded after all: long_columns.)
bool fold_level(const Amg* m, int l, int nf) {
  return m->cfg.fold && nf > 0 && (l > 0 || (m->shard.mode != Shard0::owner && m->lv[0].A.n <= m->cfg.fold0_rows));
}

CoarseSol coarse_solve(Amg* m, hipStream_t s, int l, const PcgScalars* S);

// ---- steps shared by the levels
// C.bk = P^T res (P~^T: `folded`; sums over the aggregates for a tentative transfer).  Level 0 of a multi-GPU run: from this rank's
// rows only -- a partial coarse right-hand side, which the caller all-reduces (3 n_c doubles instead of the residual's 3 n).
void restrict_level(Amg* m, hipStream_t s, int l, const double* res, const PcgScalars* S, bool folded = false) {
  AmgLevel& L = m->lv[l];
  AmgLevel& C = m->lv[l + 1];
  const int row0 = l == 0 ? m->shard.row0 : 0, row1 = l == 0 ? m->shard.row1 : 0;
  if (l == 0 && m->shard.mode == Shard0::owner && L.smoothed && L.P.local_lists)
    hipMemsetAsync(C.bk, 0, sizeof(double) * 3 * (size_t)C.A.n, s);   // coarse rows none of this rank's rows reaches
  if (L.smoothed) {
    const PDev& P = folded ? L.PS : L.P;
    Scope sc(m->prof, l == 0 ? K_RESTRICT_P0 : K_RESTRICT_P, 44.0 * P.t_n + 24.0 * L.A.n + 24.0 * L.nc);
    launch_restrict_p(s, P, res, C.bk, S, row0, row1);
  } else {
    Scope sc(m->prof, l == 0 ? K_RESTRICT0 : K_RESTRICT, 40.0 * L.A.n + 24.0 * L.nc);
    SGO_LAUNCH(k_restrict, dim3(grid_for(L.mem_ngrp, kWavesPerBlock)), dim3(kBlock), 0, s, L.mem_ngrp, L.mem_grp, L.mem, L.agg, L.d, res, C.bk, S, row0, row1);
  }
}
// out = x' + omega Dinv (b - A x'), one Jacobi sweep on a coarse level: x' = x, or with `cs` x + T (coarse solution) for the
// tentative transfer T, gathered on the fly (SPMV_JACOBI_P).  Returns the grid (of the dot products' partial sums).
int jacobi_sweep(Amg* m, hipStream_t s, AmgLevel& L, const double* x, const double* b, double* out, const PcgScalars* S,
                 const DotReq& dots = DotReq(), const CoarseSol* cs = nullptr) {
  SpmvArgs a{};
  a.x = x; a.b = b; a.y = out; a.omega = m->cfg.omega; a.S = S;
  if (dots.vec) { a.dotA = dots.vec; a.dotA2 = dots.vec2; a.partials = dots.parts; }
  if (cs) {
    a.agg = L.agg; a.d = L.d; a.u1 = cs->u1; a.u2 = cs->u2; a.c1 = cs->c1; a.c2 = cs->c2;
    Scope sc(m->prof, K_SPMV_JACOBI_P, 80.0 * L.A.nslot + 140.0 * L.A.n + 48.0 * L.nc);
    return launch_spmv_ex(s, L.A, SPMV_JACOBI_P, a);
  }
  Scope sc(m->prof, K_SPMV_JACOBI, 80.0 * L.A.nslot + 120.0 * L.A.n);
  return launch_spmv_ex(s, L.A, SPMV_JACOBI, a);
}

// ---- level 0: symmetric storage (tile or wave-group kernel, fp32 or fp64 blocks), three multi-GPU modes (Shard0)
// One level-0 pass of the cycle (S0_RESID or S0_JACOBI) over this rank's 1 / `ranks` of the work, booked as what launches: the
// tile kernel reads the fp32 copy of the blocks whenever there is one, the wave-group kernel never.  Returns the grid.
int pass0(Amg* m, hipStream_t s, int mode, const Spmv0Args& a, int ranks = 1) {
  const bool tile = m->T0.ntile > 0, f32 = tile && m->S0.fblk != nullptr;
  const int kid = mode == S0_RESID ? (tile ? (f32 ? K_SPMV0T_RESID_F32 : K_SPMV0T_RESID) : K_SPMV0_RESID)
                                   : (tile ? (f32 ? K_SPMV0T_JACOBI_F32 : K_SPMV0T_JACOBI) : K_SPMV0_JACOBI);
  Scope sc(m->prof, kid, bytes_spmv0(m->S0, mode, f32) / ranks);
  return launch_spmv0_any(s, m->S0, m->T0, mode, a);
}
// xs = omega Dinv rhs, the first sweep from zero (normally left by the producer of rhs: AmgXs0)
void first_sweep0(Amg* m, hipStream_t s, const double* rhs, AmgXs0 xs0) {
  if (xs0 != AmgXs0::compute) return;
  const Shard0& sh = m->shard;
  const bool own = sh.mode == Shard0::owner;   // (its owned rows; every other mode: all rows)
  const size_t r0 = own ? sh.row0 : 0;
  Scope sc(m->prof, K_DOT, 96.0 * m->lv[0].A.n);
  launch_precond_bj(s, own ? sh.row1 - sh.row0 : m->lv[0].A.n, m->S0.dinv + 6 * r0, rhs + 3 * r0, m->lv[0].xs + 3 * r0, m->cfg.omega);
}
// The first sweep, then the residual rs = rhs - H xs in one pass over the stored blocks.  Multi-GPU: this rank's units only -- the
// residual stays a per-rank partial (this rank's rows), which is all the restriction reads.
void presmooth0(Amg* m, hipStream_t s, const double* rhs, const PcgScalars* S, AmgXs0 xs0) {
  AmgLevel& L = m->lv[0];
  Shard0& sh = m->shard;
  first_sweep0(m, s, rhs, xs0);
  // row-owner mode: the neighbours' boundary rows of xs (unless the caller keeps them current itself)
  if (sh.mode == Shard0::owner && xs0 != AmgXs0::ready_with_halo) sh.exchange(s, L.xs, 3, sh.part->bnd, sh.part->bmax);
  if (sh.mode == Shard0::allreduce && !sh.part) hipMemsetAsync(L.rs, 0, sizeof(double) * 3 * (size_t)L.A.n, s);
  Spmv0Args a{};
  a.x = L.xs; a.b = rhs; a.y = L.rs; a.S = S; a.u0 = sh.u0; a.u1 = sh.u1;
  if (sh.mode == Shard0::single || a.u1 > a.u0) pass0(m, s, S0_RESID, a, sh.G);
}
// xs += P (coarse solution), a launch of its own on level 0 (fused into the sweep, the extra gathers would cost more than the
// launch).  Row-owner mode: on the owned rows, and on this rank's copies of the neighbours' boundary rows (k_prolong_rows: the
// coarse solution is replicated, so the corrected xs needs no exchange).
void prolong0(Amg* m, hipStream_t s, const CoarseSol& cs, const PcgScalars* S) {
  AmgLevel& L = m->lv[0];
  const Shard0& sh = m->shard;
  const bool own = sh.mode == Shard0::owner;
  const int row0 = own ? sh.row0 : 0, row1 = own ? sh.row1 : 0;
  if (L.smoothed) {
    Scope sc(m->prof, K_PROLONG_P0, 44.0 * L.P.r_n + 52.0 * L.A.n);
    SGO_LAUNCH(k_prolong_p, dim3(grid_for(L.P.r_ngrp, kWavesPerBlock)), dim3(kBlock), 0, s, S, (const int*)L.P.r_grp, L.P.r_ngrp, L.A.n, L.P,
               cs.u1, cs.c1, cs.u2, cs.c2, L.xs, (const double*)nullptr, row0, row1);
  } else {
    Scope sc(m->prof, K_PROLONG0, 68.0 * L.A.n);
    SGO_LAUNCH(k_prolong_add, dim3(grid_for(own ? row1 - row0 : L.A.n, kBlock)), dim3(kBlock), 0, s, L.A.n, L.agg, L.d, cs.u1, cs.c1,
                       cs.u2, cs.c2, L.xs, S, (const double*)nullptr, row0, row1);
  }
  if (own && sh.part->nhalo > 0) {
    const HaloDev& H = *sh.part;
    SGO_LAUNCH(k_prolong_rows, dim3(grid_for(H.nhalo, kBlock)), dim3(kBlock), 0, s, H.nhalo, H.halo_rows, L.smoothed ? L.P : PDev(),
               (const int*)L.agg, (const double*)L.d, cs.u1, cs.c1, cs.u2, cs.c2, L.xs, S);
  }
}
// out = xs + omega Dinv (rhs - H xs) on the symmetric storage, with the dot products.  Returns the grid of their partial sums.
int postsmooth0(Amg* m, hipStream_t s, const double* rhs, double* out, const DotReq& dots, const PcgScalars* S) {
  AmgLevel& L = m->lv[0];
  Shard0& sh = m->shard;
  Spmv0Args b{};
  b.x = L.xs; b.b = rhs; b.y = out; b.omega = m->cfg.omega; b.S = S; b.u0 = sh.u0; b.u1 = sh.u1;
  if (sh.mode != Shard0::allreduce) {
    // single GPU | row-owner mode, this rank's tiles: the dot products ride on the kernel -- there as per-workgroup partials of the
    // OWNED rows (the caller exchanges their sums)
    if (dots.vec) { b.dotA = dots.vec; b.dotA2 = dots.vec2; b.partials = dots.parts; }
    return pass0(m, s, S0_JACOBI, b, sh.G);
  }
  // all-reduce mode: this rank's rows, zeros elsewhere, all-reduce (or the ranks' slices gathered: one contributor per row, no
  // zero fill), then the dot products on the full vector (replicated)
  if (!sh.part) hipMemsetAsync(out, 0, sizeof(double) * 3 * (size_t)L.A.n, s);
  if (b.u1 > b.u0) pass0(m, s, S0_JACOBI, b);
  if (sh.part) sh.gather(s, out);
  else sh.reduce(s, out, 3 * (size_t)L.A.n);
  if (!dots.vec) return 0;
  const int grid = grid_for(3LL * L.A.n, kBlock);
  Scope sc(m->prof, K_DOT, 72.0 * L.A.n);
  SGO_LAUNCH(k_dots2, dim3(grid), dim3(kBlock), 0, s, 3 * L.A.n, (const double*)out, dots.vec, dots.vec2, dots.parts, S);
  return grid;
}
// out = cycle(0, rhs) in the folded form (see "folded V-cycle"; single GPU): restriction with P~^T of the right-hand side itself,
// coarse solve, prolongation with P~ onto the two-sweep term M2 rhs = xs + omega Dinv (rhs - H xs), the level-0 Jacobi pass (into
// rs).  (That pass does not depend on the coarse levels; running it BESIDE them on a second stream -- a parallel branch of the captured
// hipGraph -- was measured: the fork and join cost 25 us per PCG iteration on this runtime, C2 1.45 -> 1.95 ms per GN iteration.)
int cycle0_fold(Amg* m, hipStream_t s, const double* rhs, double* out, const DotReq& dots, const PcgScalars* S, AmgXs0 xs0) {
  AmgLevel& L = m->lv[0];
  AmgLevel& C = m->lv[1];
  first_sweep0(m, s, rhs, xs0);
  Spmv0Args b{};
  b.x = L.xs; b.b = rhs; b.y = L.rs; b.omega = m->cfg.omega; b.S = S;
  if (m->T0.ntile == 0) {   // wave-group kernel: the pass and the restriction in one launch
    const int nb_spmv = grid_for(m->S0.ngrp, kWavesPerBlock), nb_main = grid_for(L.PS.t_ngrp, kWavesPerBlock);
    Scope sc(m->prof, K_JACOBI0_RESTRICT, bytes_spmv0(m->S0, S0_JACOBI) + 44.0 * L.PS.t_n + 24.0 * L.A.n + 24.0 * L.nc);
    SGO_LAUNCH(k_jacobi0_restrict, dim3(nb_spmv + nb_main + L.PS.t_nlong), dim3(kBlock), 0, s, b.S, (const int*)m->S0.grp, (const int*)m->S0.grow,
               (const int*)m->S0.gown, (const int*)m->S0.gtr, b.u1 > 0 ? b.u0 : 0, b.u1 > 0 ? b.u1 : m->S0.ngrp, nb_spmv, nb_main, m->S0, b, L.PS,
               C.bk);
  } else {
    pass0(m, s, S0_JACOBI, b);
    restrict_level(m, s, 0, rhs, S, true);
  }
  const CoarseSol cs = coarse_solve(m, s, 0, S);
  // (the dot products' partial sums are re-reduced by every workgroup of the consumer: a few hundred of them, not thousands)
  const int grid = std::min(grid_for(L.PS.r_ngrp, kFoldThreads / 64), 512);
  Scope sc(m->prof, K_PROLONG_FOLD0, 44.0 * L.PS.r_n + 72.0 * L.A.n);
  SGO_LAUNCH(k_prolong_fold, dim3(grid), dim3(kFoldThreads), 0, s, S, (const int*)L.PS.r_grp, L.PS.r_ngrp, L.PS, cs.u1, cs.c1, cs.u2,
             cs.c2, (const double*)L.rs, out, dots.vec, dots.vec2, dots.vec ? dots.parts : nullptr);
  return grid;
}
// out = cycle(0, rhs), the whole preconditioner: pre-smoothing from zero + residual, restriction, coarse solve (dense inverse, a
// V-cycle or flexible-CG steps), prolongation, post-smoothing.  Partial sums of dots.vec . out (and dots.vec2 . out): returns their grid.
int cycle0(Amg* m, hipStream_t s, const double* rhs, double* out, const DotReq& dots, const PcgScalars* S, AmgXs0 xs0) {
  if (cycle_form(m, 0, false, dots.vec).kind == CycleForm::folded) return cycle0_fold(m, s, rhs, out, dots, S, xs0);
  presmooth0(m, s, rhs, S, xs0);
  restrict_level(m, s, 0, m->lv[0].rs, S);
  m->shard.reduce(s, m->lv[1].bk, 3 * (size_t)m->lv[1].A.n);   // the ranks' partials (each from its own fine rows) -> their sum
  const CoarseSol cs = coarse_solve(m, s, 0, S);
  prolong0(m, s, cs, S);
  return postsmooth0(m, s, rhs, out, dots, S);
}

// ---- levels >= 1: BsrDev; transfer by the smoothed P with nu sweeps per side, or by the tentative one fused into the sweeps
// xs = omega Dinv rhs (first sweep from zero), rs = rhs - A xs on a coarse level.  One fused launch (the gathered operand is
// omega Dinv[col] rhs[col]: 72 B per slot) where a launch costs more than the level's data; on a LARGE level (C5's first coarse
// levels: millions of slots) the sweep from zero as a vector kernel of its own and a plain residual pass that gathers 24 B per slot.
constexpr int kUnfuseSlots = 400000;   // (swept on C5 / C4r: 10^6 87.0 / 64.4 M edge-Jacobians/s, 4 10^5 89.4 / 65.3, 1.5 10^5 89.9 / 64.8, 5 10^4 90.3 / 63.4)
void pre_resid(Amg* m, hipStream_t s, AmgLevel& L, const double* rhs, const PcgScalars* S) {
  SpmvArgs a{};
  a.b = rhs; a.y = L.rs; a.omega = m->cfg.omega; a.S = S;
  if (L.A.nslot >= kUnfuseSlots) {
    {
      Scope sc(m->prof, K_DOT, 96.0 * L.A.n);
      launch_precond_bj(s, L.A.n, L.A.dinv, rhs, L.xs, m->cfg.omega);
    }
    a.x = L.xs;
    Scope sc(m->prof, K_SPMV_RESID, 80.0 * L.A.nslot + 72.0 * L.A.n);
    launch_spmv_ex(s, L.A, SPMV_RESID, a);
    return;
  }
  a.y2 = L.xs;
  Scope sc(m->prof, K_SPMV_PRE_RESID, 80.0 * L.A.nslot + 120.0 * L.A.n);
  launch_spmv_ex(s, L.A, SPMV_PRE_RESID, a);
}
// nu pre-smoothing sweeps from zero (accumulated in xs); returns the residual they leave (rs or tR).  With `sub` the first launch
// also forms the right-hand side.
const double* presmooth(Amg* m, hipStream_t s, AmgLevel& L, const double* rhs, const RhsSub* sub, int nu, const PcgScalars* S) {
  if (sub) {
    SpmvArgs a{};
    a.b = rhs; a.y = L.rs; a.y2 = L.xs; a.omega = m->cfg.omega; a.S = S; a.bsub = sub->sub; a.c1 = sub->c; a.b_out = sub->out;
    Scope sc(m->prof, K_SPMV_PRE_RESID_S, 80.0 * L.A.nslot + 168.0 * L.A.n);
    launch_spmv_ex(s, L.A, SPMV_PRE_RESID_S, a);
  } else {
    pre_resid(m, s, L, rhs, S);
  }
  // further sweeps (levels walked by the V-cycle only): sweep s applied to the residual of sweep s-1 gives the next correction
  // (accumulated into xs) and the next residual (rs <-> tR)
  double* res = L.rs;
  for (int sw = 1; sw < nu; ++sw) {
    SpmvArgs a{};
    a.b = res; a.y = (res == L.rs) ? L.tR : L.rs; a.y2 = L.xs; a.omega = m->cfg.omega; a.S = S;
    Scope sc(m->prof, K_SPMV_PRE_RESID_ACC, 80.0 * L.A.nslot + 144.0 * L.A.n);
    launch_spmv_ex(s, L.A, SPMV_PRE_RESID_ACC, a);
    res = a.y;
  }
  return res;
}
// out = the post-smoothed xs + P (coarse solution) for the right-hand side rhs: the smoothed P as a launch of its own and nu sweeps |
// the tentative one unfused on a large level | fused into the sweep.  Returns the grid of the last kernel (the dot products').
int prolong_postsmooth(Amg* m, hipStream_t s, AmgLevel& L, const double* rhs, double* out, const CoarseSol& cs, int nu,
                       const DotReq& dots, const PcgScalars* S) {
  if (L.smoothed) {
    {
      Scope sc(m->prof, K_PROLONG_P, 80.0 * L.P.np + 52.0 * L.A.n);
      SGO_LAUNCH(k_prolong_p, dim3(grid_for(L.P.r_ngrp, kWavesPerBlock)), dim3(kBlock), 0, s, S, (const int*)L.P.r_grp, L.P.r_ngrp, L.A.n, L.P,
                 cs.u1, cs.c1, cs.u2, cs.c2, L.xs, (const double*)nullptr, 0, 0);
    }
    const double* x = L.xs;   // the first nu - 1 sweeps through the two residual buffers (free by now)
    for (int sw = 1; sw < nu; ++sw) {
      double* dst = (x == L.rs) ? L.tR : L.rs;
      jacobi_sweep(m, s, L, x, rhs, dst, S);
      x = dst;
    }
    return jacobi_sweep(m, s, L, x, rhs, out, S, dots);
  }
  if (L.A.nslot < kUnfuseSlots) return jacobi_sweep(m, s, L, L.xs, rhs, out, S, dots, &cs);
  // a large level: the prolongation as a vector kernel of its own (same arithmetic, in place), then a plain sweep that gathers
  // 24 B per slot instead of x, the aggregate number, the coarse vectors and the lever arm (68-92 B)
  {
    Scope sc(m->prof, K_PROLONG, 52.0 * L.A.n + 48.0 * L.nc);
    SGO_LAUNCH(k_prolong_add, dim3(grid_for(L.A.n, kBlock)), dim3(kBlock), 0, s, L.A.n, L.agg, L.d, cs.u1, cs.c1, cs.u2, cs.c2, L.xs, S,
               (const double*)nullptr, 0, 0);
  }
  return jacobi_sweep(m, s, L, L.xs, rhs, out, S, dots);
}
// out = cycle(l, rhs) in the folded form: restriction with P~^T of the right-hand side itself, coarse solve, and one launch for
// the prolongation with P~ onto the two-sweep term M2 rhs (+ xadd).
int cycle_coarse_fold(Amg* m, hipStream_t s, int l, const double* rhs, double* out, const PcgScalars* S, const double* xadd = nullptr) {
  AmgLevel& L = m->lv[l];
  restrict_level(m, s, l, rhs, S, true);
  const CoarseSol cs = coarse_solve(m, s, l, S);
  Scope sc(m->prof, K_UP_FOLD, 80.0 * L.A.nslot + 44.0 * L.PS.r_n + 100.0 * L.A.n);
  const int grid = grid_for(L.U.ngrp, kWavesPerBlock);
  SGO_LAUNCH(k_up_fold, dim3(grid), dim3(kBlock), 0, s, S, (const int*)L.U.grp, L.U.ngrp, L.A, L.U, L.PS, rhs, m->cfg.omega, cs.u1, cs.c1,
             cs.u2, cs.c2, out, xadd);
  return grid;
}
// out = cycle(l, rhs'), l >= 1: rhs' = rhs - c sub with `sub` (the K-cycle's second step).  Pre-smoothing from zero + residual,
// restriction, coarse solve, prolongation fused into the post-smoothing launch where the transfer is the tentative one.  Partial
// sums of dots.vec . out on request; returns the grid of the last kernel.
int cycle_coarse(Amg* m, hipStream_t s, int l, const double* rhs, double* out, const PcgScalars* S, const RhsSub* sub = nullptr,
                 const DotReq& dots = DotReq()) {
  AmgLevel& L = m->lv[l];
  const CycleForm f = cycle_form(m, l, sub != nullptr, dots.vec != nullptr);
  if (f.kind == CycleForm::folded) return cycle_coarse_fold(m, s, l, rhs, out, S);
  if (f.kind == CycleForm::folded_in_two_sweeps) {
    pre_resid(m, s, L, rhs, S);                            // xs = omega Dinv rhs, rs = rhs - A xs
    cycle_coarse_fold(m, s, l, L.rs, L.tR, S, L.xs);       // tR = xs + cycle(rs)
    return jacobi_sweep(m, s, L, L.tR, rhs, out, S);
  }
  const double* res = presmooth(m, s, L, rhs, sub, f.nu, S);
  restrict_level(m, s, l, res, S);
  const CoarseSol cs = coarse_solve(m, s, l, S);
  return prolong_postsmooth(m, s, L, sub ? sub->out : rhs, out, cs, f.nu, dots, S);
}

// Two flexible-CG steps on level l for A x = bk (Notay's K-cycle), with the vector updates
// fused into the neighbouring SpMV-type launches:
//   z1 = cycle(bk);               q = A z1            -> pA = (z1.q, z1.bk)     a1 = pA[1]/pA[0]
//   z2 = cycle(bk - a1 q) [bk2];  q = A (z2 - b z1)   -> pC = (q.z2), b = pC[0]/pA[0]; p2 = z2 - b z1
//                                                        pB = (p2.q, p2.bk2)      a2 = pB[1]/pB[0]
//   x = a1 z1 + a2 p2   (returned as a CoarseSol)
CoarseSol fcg(Amg* m, hipStream_t s, int l, const PcgScalars* S) {
  AmgLevel& L = m->lv[l];
  cycle_coarse(m, s, l, L.bk, L.z1, S);
  int gA;
  {
    SpmvArgs a{};
    a.x = L.z1; a.y = L.q; a.dotA = L.z1; a.dotB = L.z1; a.dotC = L.bk; a.partials = L.pA; a.S = S;
    Scope sc(m->prof, K_SPMV_AX, bytes_spmv(L.A));
    gA = launch_spmv_ex(s, L.A, SPMV_AX, a);
  }
  L.gA = gA;
  L.gB = L.gC = 0;  // the second step has not run (the export's "0: that step did not run")
  CoarseSol cs;
  cs.u1 = L.z1;
  cs.c1 = SpmvRatio{L.pA + kMaxPartials, gA, L.pA, gA};
  if (l > m->fcg2_depth) return cs;  // one FCG step only (steepest descent in the cycle's direction)
  const RhsSub sub{L.q, cs.c1, L.bk2};
  const int gC = cycle_coarse(m, s, l, L.bk, L.z2, S, &sub, DotReq{L.q, nullptr, L.pC});
  int gB;
  {
    SpmvArgs a{};
    a.x = L.z2; a.x2 = L.z1; a.x_out = L.p2; a.y = L.q2; a.dotC = L.bk2; a.partials = L.pB; a.S = S;
    a.c1 = SpmvRatio{L.pC, gC, L.pA, gA};
    Scope sc(m->prof, K_SPMV_AX_C, 80.0 * L.A.nslot + 120.0 * L.A.n);
    gB = launch_spmv_ex(s, L.A, SPMV_AX_C, a);
  }
  L.gB = gB;
  L.gC = gC;
  cs.u2 = L.p2;
  cs.c2 = SpmvRatio{L.pB + kMaxPartials, gB, L.pB, gB};
  return cs;
}
// The coarse solve for the right-hand side C.bk of level l + 1, as the parent level sees it.
CoarseSol coarse_solve(Amg* m, hipStream_t s, int l, const PcgScalars* S) {
  AmgLevel& C = m->lv[l + 1];
  CoarseSol cs;
  cs.u1 = C.xk;
  if (l + 1 == (int)m->lv.size() - 1) {
    Scope sc(m->prof, K_DENSE_APPLY, 8.0 * m->N * m->N);
    SGO_LAUNCH(k_dense_apply, dim3(grid_for(m->N, kWavesPerBlock)), dim3(kBlock), 0, s, m->N, m->Np, m->inv, C.bk, C.xk, S);
  } else if (l + 1 > m->kdepth && C.smoothed) {  // V-cycle below the K-cycle depth (a tentative transfer always gets the K-cycle)
    cycle_coarse(m, s, l + 1, C.bk, C.xk, S);
  } else {
    cs = fcg(m, s, l + 1, S);
  }
  return cs;
}

}  // namespace

int amg_num_levels(const Amg* m) { return m ? (int)m->lv.size() : 0; }
bool amg_has_filtered(const Amg* m) {
  if (m)
    for (const AmgLevel& L : m->lv)
      if (L.smoothed && L.P.dF) return true;
  return false;
}
long long amg_level0_bytes(const Amg* m) { return m ? m->level0_bytes : 0; }
bool amg_coarsest_not_spd(Amg* m, hipStream_t s) {
  int f = 0;
  if (!m || !m->d_fail) return false;
  if (hipMemcpyAsync(&f, m->d_fail, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return false;
  if (hipStreamSynchronize(s) != hipSuccess) return false;
  return f != 0;
}
void amg_describe(const Amg* m, std::string* out) { *out = m ? m->desc : ""; }
void amg_kept_aggregates(const Amg* m, AmgKeptAgg* out) {
  if (m && out) *out = m->kept;
}

void amg_destroy(Amg* m) {
  if (!m) return;
  delete m;   // the device memory belongs to the caller's arena
}


int amg_update(Amg* m, hipStream_t s, std::string* err) {
  const int last = (int)m->lv.size() - 1;
  {
    AmgLevel& L0 = m->lv[0];
    Scope sc(m->prof, K_POSITIONS0, 40.0 * L0.A.n);
    SGO_LAUNCH(k_positions0, dim3(grid_for(L0.A.n, kBlock)), dim3(kBlock), 0, s, L0.A.n, m->d_free_id, m->d_poses,
                       L0.pos);
  }
  for (int l = 0; l < last; ++l) {
    AmgLevel& L = m->lv[l];
    AmgLevel& C = m->lv[l + 1];
    {
      Scope sc(m->prof, K_CENTRES, 36.0 * L.A.n);
      SGO_LAUNCH(k_centres, dim3(grid_for(L.nc, kWavesPerBlock)), dim3(kBlock), 0, s, L.nc, L.mem_ptr, L.mem, L.pos, C.pos, L.d);
    }
    launch_coarse_operator(m, s, L, C, l == 0);
    {
      Scope sc(m->prof, K_LEVEL_DINV, 120.0 * C.A.n);
      SGO_LAUNCH(k_level_dinv, dim3(grid_for(C.A.n, kBlock)), dim3(kBlock), 0, s, C.A.n, (const int*)C.A.rowptr, C.A);
    }
  }
  {
    Scope sc(m->prof, K_DENSE_INVERT, 8.0 * m->Np * m->Np);
    const int nb = m->Np / kGjB;
    hipMemsetAsync(m->inv0, 0, sizeof(double) * (size_t)m->Np * m->Np, s);
    hipMemsetAsync(m->d_fail, 0, sizeof(int), s);
    if (last > 0)
      SGO_LAUNCH(k_dense_fill_unique, dim3(grid_for(m->lv[last].A.nslot, kBlock)), dim3(kBlock), 0, s, m->lv[last].A, m->Np, m->inv0);
    else   // level 0 can hold several slots per (row, col): duplicate edges
      SGO_LAUNCH(k_dense_fill, dim3(grid_for(m->lv[last].A.n, kBlock)), dim3(kBlock), 0, s, m->lv[last].A, m->Np, m->inv0);
    SGO_LAUNCH(k_gj_pivot, dim3(1), dim3(kGjB * kGjB), 0, s, m->inv0, m->Np, 0, m->gjP[0], m->d_fail);
    for (int kb = 0; kb < nb; ++kb) {   // the result of step kb lands in buffer (kb + 1) & 1: m->inv after the last one
      const double* src = (kb & 1) ? m->inv1 : m->inv0;
      double* dst = (kb & 1) ? m->inv0 : m->inv1;
      SGO_LAUNCH(k_gj_step, dim3(nb, nb), dim3(kBlock), 0, s, src, dst, m->Np, kb, (const double*)m->gjP[kb & 1],
                 m->gjP[(kb + 1) & 1], m->d_fail);
    }
  }
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) {
    if (err) *err = std::string("amg_update: a kernel launch failed: ") + hipGetErrorString(le);
    return SGO_EHIP;
  }
  return SGO_OK;
}

void amg_set_shard(Amg* m, Comm* comm, int u0, int u1, int row0, int row1, const HaloDev* slices) {
  m->shard.mode = Shard0::allreduce;
  m->shard.u0 = u0; m->shard.u1 = u1; m->shard.row0 = row0; m->shard.row1 = row1;
  m->shard.comm = comm;
  m->shard.part = slices;
}
bool amg_comm_failed(const Amg* m) { return m && m->shard.failed; }
// Test hook: the coarse right-hand side the first half of a level-0 cycle produces from r (first sweep from zero,
// residual pass, restriction; where level 0 has the folded transfer, its restriction of r itself: the same vector in exact
// arithmetic) -- with a shard set, this rank's PARTIAL coarse right-hand side: the cycle's steps short of the all-reduce.
int amg_debug_coarse_rhs(Amg* m, hipStream_t s, const double* r, double* out_dev, int cap3) {
  if (!m || m->lv.size() < 2) return 0;
  const int n3c = 3 * m->lv[1].A.n;
  if (cap3 < n3c) return -1;
  if (m->lv[0].fold) {
    restrict_level(m, s, 0, r, nullptr, true);
  } else {
    presmooth0(m, s, r, nullptr, AmgXs0::compute);
    restrict_level(m, s, 0, m->lv[0].rs, nullptr);
  }
  hipMemcpyAsync(out_dev, m->lv[1].bk, sizeof(double) * n3c, hipMemcpyDeviceToDevice, s);
  return n3c;
}
namespace {
// The logical slots' blocks as [nslot][9] records (load_block: level 0 through its references into the symmetric storage).  With
// fblk: the off-diagonal blocks from the fp32 copy the preconditioner's level-0 tile passes read (diagonal blocks stay fp64 there).
__global__ __launch_bounds__(kBlock) void k_debug_blocks(BsrDev A, const float* __restrict__ fblk, const float* __restrict__ fblk8,
                                                         double* __restrict__ out) {
  for (int k = blockIdx.x * kBlock + threadIdx.x; k < A.nslot; k += gridDim.x * kBlock) {
    double b[9];
    load_block(A, (size_t)k, b);
    if (fblk && A.ref && A.ref[k] >= 0) {
      const int r = A.ref[k];
      const size_t u = (size_t)(r >> 1), nu = (size_t)A.nus;
      double v[9];
      for (int c = 0; c < 8; ++c) v[c] = (double)fblk[4 * ((size_t)(c >> 2) * nu + u) + (c & 3)];
      v[8] = (double)fblk8[u];
      for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) b[3 * p + q] = (r & 1) ? v[3 * q + p] : v[3 * p + q];
    }
    for (int c = 0; c < 9; ++c) out[9 * (size_t)k + c] = b[c];
  }
}
}  // namespace

// Test hook (sgo_debug_amg_array, sgo.h): array `what` of level `level` of the resident hierarchy, exactly as the next cycle and the
// next amg_update read it -- device memory copied as stored; the one gather is a level's logical blocks (k_debug_blocks).  Returns the
// array's size in bytes and copies it when cap_bytes suffices, 0 when the level has no such array, < 0 on error.  Single GPU only.
long long amg_debug_array(Amg* m, hipStream_t s, int level, int what, void* out, long long cap_bytes) {
  if (!m || level < 0 || level >= (int)m->lv.size()) return 0;
  if (m->shard.mode != Shard0::single) return SGO_EINVAL;
  const int last = (int)m->lv.size() - 1;
  AmgLevel& L = m->lv[level];
  const PDev& P = L.P;
  const PDev& PS = L.PS;
  const bool transfer = level < last, sm = transfer && L.smoothed, fo = sm && L.fold;
  const size_t n = (size_t)L.A.n, ns = (size_t)L.A.nslot, nc = transfer ? (size_t)L.nc : 0;
  const size_t nsc = transfer ? (size_t)m->lv[level + 1].A.nslot : 0;
  const void* src = nullptr;
  size_t bytes = 0;
  auto arr = [&](bool have, const void* p, size_t count, size_t elem) {
    if (have && p) {
      src = p;
      bytes = count * elem;
    }
  };
  const size_t I = sizeof(int), F = sizeof(float), Dd = sizeof(double);
  const bool f32 = level == 0 && m->T0.ntile > 0 && m->S0.fblk != nullptr;   // (pass0's rule)
  switch (what) {
    case SGO_AMG_INFO: {
      const CycleForm cf = cycle_form(m, level, false, false);
      const double v[SGO_AMG_INFO_COUNT] = {(double)n, (double)ns, (double)nc, sm ? 1.0 : 0.0, (sm && P.dF) ? 1.0 : 0.0, fo ? 1.0 : 0.0,
                                            transfer ? (double)cf.kind : 0.0, transfer ? (double)cf.nu : 0.0, m->cfg.omega, m->cfg.omega_p,
                                            sm ? (double)P.np : 0.0, sm ? (double)P.nap : 0.0, sm ? (double)P.val.n : 0.0,
                                            sm ? (double)P.ap.n : 0.0, sm ? (double)P.rap.n : 0.0, (double)(last + 1), f32 ? 1.0 : 0.0,
                                            (double)m->N, (double)m->Np, sm ? (double)P.t_nlong : 0.0, fo ? (double)PS.t_nlong : 0.0,
                                            (double)m->kdepth, m->cfg.theta_filter, (double)nsc, (double)m->fcg2_depth};
      if (cap_bytes >= (long long)sizeof v) std::memcpy(out, v, sizeof v);
      return (long long)sizeof v;
    }
    case SGO_AMG_A_ROWPTR: arr(true, L.A.rowptr, n + 1, I); break;
    case SGO_AMG_A_COL: arr(true, L.A.col, ns, I); break;
    case SGO_AMG_A_BLK:
    case SGO_AMG_A_BLK_F32: {
      if (what == SGO_AMG_A_BLK_F32 && !f32) return 0;
      const long long need = (long long)(9 * ns * Dd);
      if (cap_bytes < need) return need;
      double* tmp = nullptr;
      if (hipMalloc(&tmp, (size_t)need) != hipSuccess) return SGO_ENOMEM;
      SGO_LAUNCH(k_debug_blocks, dim3(grid_for((long long)ns, kBlock)), dim3(kBlock), 0, s, L.A,
                 what == SGO_AMG_A_BLK_F32 ? (const float*)m->S0.fblk : (const float*)nullptr, (const float*)m->S0.fblk8, tmp);
      hipError_t e = hipMemcpyAsync(out, tmp, (size_t)need, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      hipFree(tmp);
      return e == hipSuccess ? need : (long long)SGO_EHIP;
    }
    case SGO_AMG_A_DINV: arr(true, L.A.dinv, 6 * n, Dd); break;
    case SGO_AMG_POS: arr(true, L.pos, 2 * n, Dd); break;
    case SGO_AMG_D: arr(transfer, L.d, 2 * n, Dd); break;
    case SGO_AMG_AGG: arr(transfer, L.agg, n, I); break;
    case SGO_AMG_MEM_PTR: arr(transfer, L.mem_ptr, nc + 1, I); break;
    case SGO_AMG_MEM: arr(transfer, L.mem, n, I); break;
    case SGO_AMG_P_ROWPTR: arr(sm, P.rowptr, n + 1, I); break;
    case SGO_AMG_P_ROW: arr(sm, P.row, (size_t)P.np, I); break;
    case SGO_AMG_P_COL: arr(sm, P.col, (size_t)P.np, I); break;
    case SGO_AMG_P_BLK: arr(sm, P.blk, 9 * (size_t)P.np, Dd); break;
    case SGO_AMG_P_RBLK: arr(sm, P.r_blk, 9 * (size_t)P.r_n, F); break;   // quads [2][np][4], then component 8 [np]
    case SGO_AMG_P_TBLK: arr(sm, P.t_blk, 9 * (size_t)P.t_n, F); break;
    case SGO_AMG_P_TPOS: arr(sm, P.t_pos, (size_t)P.np, I); break;
    case SGO_AMG_P_TROW: arr(sm, P.t_row, (size_t)P.np, I); break;
    case SGO_AMG_P_TCOL: arr(sm, P.t_col, (size_t)P.np, I); break;
    case SGO_AMG_STRONG: arr(sm && P.dF, P.strong, ns, 1); break;
    case SGO_AMG_DF: arr(sm, P.dF, 9 * n, Dd); break;
    case SGO_AMG_DINVF: arr(sm, P.dinvF, 9 * n, Dd); break;
    case SGO_AMG_AP_A: arr(sm, P.ap.a, (size_t)P.ap.n, I); break;
    case SGO_AMG_AP_B: arr(sm, P.ap.b, (size_t)P.ap.n, I); break;
    case SGO_AMG_AP_TGT: arr(sm, P.ap.tgt, (size_t)P.ap.n, I); break;
    case SGO_AMG_AP_BLK: arr(sm, P.apblk, 9 * (size_t)P.nap, Dd); break;
    case SGO_AMG_PS_ROW: arr(fo, PS.row, (size_t)PS.np, I); break;
    case SGO_AMG_PS_COL: arr(fo, PS.col, (size_t)PS.np, I); break;
    case SGO_AMG_PS_RBLK: arr(fo, PS.r_blk, 9 * (size_t)PS.r_n, F); break;
    case SGO_AMG_PS_TBLK: arr(fo, PS.t_blk, 9 * (size_t)PS.t_n, F); break;
    case SGO_AMG_PS_TROW: arr(fo, PS.t_row, (size_t)PS.np, I); break;
    case SGO_AMG_PS_TCOL: arr(fo, PS.t_col, (size_t)PS.np, I); break;
    case SGO_AMG_PS_STPOS: arr(fo, L.F.st_pos, (size_t)PS.np, I); break;
    case SGO_AMG_INV: arr(level == last, m->inv, (size_t)m->Np * m->Np, Dd); break;
    // the cycle's work vectors as the last amg_apply left them (a level >= 2 is visited several times per cycle: its LAST visit)
    case SGO_AMG_W_XS: arr(true, L.xs, 3 * n, Dd); break;
    case SGO_AMG_W_RS: arr(true, L.rs, 3 * n, Dd); break;
    case SGO_AMG_W_TR: arr(true, L.tR, 3 * n, Dd); break;
    case SGO_AMG_W_BK: arr(level > 0, L.bk, 3 * n, Dd); break;
    case SGO_AMG_W_XK: arr(level > 0, L.xk, 3 * n, Dd); break;
    case SGO_AMG_W_Z1: arr(level > 0, L.z1, 3 * n, Dd); break;
    case SGO_AMG_W_Q: arr(level > 0, L.q, 3 * n, Dd); break;
    case SGO_AMG_W_BK2: arr(level > 0, L.bk2, 3 * n, Dd); break;
    case SGO_AMG_W_Z2: arr(level > 0, L.z2, 3 * n, Dd); break;
    case SGO_AMG_W_P2: arr(level > 0, L.p2, 3 * n, Dd); break;
    case SGO_AMG_W_Q2: arr(level > 0, L.q2, 3 * n, Dd); break;
    case SGO_AMG_W_PA: arr(level > 0, L.pA, 2 * (size_t)kMaxPartials, Dd); break;
    case SGO_AMG_W_PB: arr(level > 0, L.pB, 2 * (size_t)kMaxPartials, Dd); break;
    case SGO_AMG_W_PC: arr(level > 0, L.pC, 2 * (size_t)kMaxPartials, Dd); break;
    case SGO_AMG_W_GRIDS: {
      if (level == 0) return 0;
      const int g[3] = {L.gA, L.gB, L.gC};
      if (cap_bytes >= (long long)sizeof g) std::memcpy(out, g, sizeof g);
      return (long long)sizeof g;
    }
    default: return SGO_EINVAL;
  }
  if (!src || bytes == 0) return 0;
  if (cap_bytes < (long long)bytes) return (long long)bytes;
  if (hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return SGO_EHIP;
  return (long long)bytes;
}
double* amg_xs0(Amg* m) { return (m && m->lv.size() > 1) ? m->lv[0].xs : nullptr; }
double amg_omega(const Amg* m) { return m ? m->cfg.omega : 0.0; }

int amg_apply(Amg* m, hipStream_t s, const double* r, double* z, const double* dotvec, double* partials,
              const PcgScalars* S, const double* dotvec2, AmgXs0 xs0) {
  if (m->lv.size() == 1) {  // single (dense) level: z = H^-1 r
    {
      Scope sc(m->prof, K_DENSE_APPLY, 8.0 * m->N * m->N);
      SGO_LAUNCH(k_dense_apply, dim3(grid_for(m->N, kWavesPerBlock)), dim3(kBlock), 0, s, m->N, m->Np, m->inv, r, z, S);
    }
    if (!dotvec) return 0;
    const int grid = grid_for(m->N, kBlock);
    Scope sc(m->prof, K_DOT, 24.0 * m->N);
    SGO_LAUNCH(k_dots2, dim3(grid), dim3(kBlock), 0, s, m->N, (const double*)z, dotvec, dotvec2, partials, S);
    return grid;
  }
  return cycle0(m, s, r, z, DotReq{dotvec, dotvec2, partials}, S, xs0);
}

// v[0..n) counts -> exclusive prefix sums in place, v[n] = total (device, on the stream); `sums` holds n / kScanChunk + 2 ints
void dev_scan_exclusive(hipStream_t s, int* v, int n, int* sums) {
  if (n <= kScanSmall) {   // one workgroup, one launch (the set-up's scans are mostly this small: three launches each were a third of its launches)
    SGO_LAUNCH(k_scan_small, dim3(1), dim3(1024), 0, s, v, n);
    return;
  }
  const int nb = (n + kScanChunk - 1) / kScanChunk;
  SGO_LAUNCH(k_scan_sums, dim3(std::max(nb, 1)), dim3(kBlock), 0, s, (const int*)v, n, sums);
  SGO_LAUNCH(k_scan_top, dim3(1), dim3(kBlock), 0, s, sums, nb);
  SGO_LAUNCH(k_scan_apply, dim3(std::max(nb, 1)), dim3(kBlock), 0, s, v, n, (const int*)sums, nb);
}
// The configuration amg_create works with for a level-0 operator of n rows / nslot logical slots: the caller's
// values, the environment overrides and the size-dependent choices.
AmgConfig amg_effective_config(const AmgConfig& cfg_in, int n, int nslot) {
  AmgConfig cfg = cfg_in;
  // A sweep on a coarse level is a 5-10 us launch whatever the graph; it pays when a PCG iteration is
  // dominated by level 0 (C4: 31 instead of 39 iterations, 9.7 instead of 10.6 ms) and costs a few
  // per cent on graphs whose level 0 is itself launch-bound (10k / 40k: 2.67 instead of 2.51 ms).
  cfg.nu_coarse = nslot >= 600000 ? 2 : 1;   // (with the folded cycle, scripts/nu_sweep.py: 30k / 300k 2.38 -> 2.31, 50k / 500k 3.00 -> 2.84 ms per GN
                                             // iteration with two sweeps; 20k / 200k 1.81 -> 1.91, C2 1.24 -> 1.36)
  if (const char* e = std::getenv("SGO_AMG_SMOOTH")) cfg.smooth = std::atoi(e) != 0;
  if (const char* e = std::getenv("SGO_AMG_LISTS")) cfg.lists_on_device = std::string(e) != "host";
  if (const char* e = std::getenv("SGO_AMG_THETA_FILTER")) cfg.theta_filter = std::atof(e);
  if (const char* e = std::getenv("SGO_AMG_FILTER")) cfg.filtered_smoothing = cfg.filtered_smoothing && std::atoi(e) != 0;   // (can only switch it off)
  // (experiment knobs of scripts/param_sweep.py.  Round 3, folded cycle, optimize(20) on C4 / C2 / C3s: omega 0.7 / 0.8 / 0.9 /
  // 1.0 -> 473 / 442 / 422 / 1015 PCG iterations on C4 (0.9 is 3-5 % better on every shape of scripts/robustness.py, 1.0 is
  // past the cliff: the default keeps its margin); omega_p 0.5 / 0.66 / 0.8 / 1.0 -> 486 / 442 / 557 / 809; theta 0.01 / 0.02 /
  // 0.04 -> C2 387 / 391 / 285, C3s 598 / 549 / 499, but on C4 theta 0.04 makes the smoothed level-0 operator too dense, the
  // hierarchy falls back to the tentative transfer with stagnating levels (100k -> 13k -> 4.6k -> 2.6k -> 2.0k) and needs
  // 175 iterations for the first solve instead of 30; 0.025 / 0.03 keep the smoothed transfer on C4 but its denser coarse
  // operators double the time (85 -> 159 / 167 ms), and 10k poses / 100k edges goes 354 -> 552 / 748 iterations: the
  // threshold is not a free parameter)
  if (const char* e = std::getenv("SGO_AMG_OMEGA")) cfg.omega = std::atof(e);
  if (const char* e = std::getenv("SGO_AMG_OMEGA_P")) cfg.omega_p = std::atof(e);
  if (const char* e = std::getenv("SGO_AMG_THETA")) cfg.theta = cfg.theta_coarse = std::atof(e);
  if (const char* e = std::getenv("SGO_AMG_FOLD")) cfg.fold = std::atoi(e) != 0;
  if (const char* e = std::getenv("SGO_AMG_FOLD0_ROWS")) cfg.fold0_rows = std::atoi(e);
  cfg.fold = cfg.fold && cfg.smooth && cfg.lists_on_device;
  // (the folded cycle folds ONE sweep per side into the transfers -- two would need the pattern of A A P; a second sweep is
  // one explicit sweep around it, see cycle_form().  One sweep everywhere was measured on C4: five coarse launches instead of
  // nine, but 27.9 instead of 22.1 PCG iterations, 5.07 against 4.59 ms per GN iteration)
  if (const char* e = std::getenv("SGO_AMG_NU")) {
    cfg.nu_coarse = std::max(1, std::atoi(e));
    cfg.nu_from_env = true;   // (amg_create then leaves the count alone: finish_coarsest)
  }
  // With the smoothed prolongator a V-cycle needs ~1.4x the PCG iterations of the K-cycle (C4: 39 vs
  // 27) at less than half the launches per iteration: V is the default there, K for the tentative one.
  if (cfg.smooth) cfg.kdepth = 0;
  if (const char* e = std::getenv("SGO_AMG_KDEPTH")) cfg.kdepth = std::atoi(e);
  if (const char* e = std::getenv("SGO_AMG_FCG2_DEPTH")) cfg.fcg2_depth = std::atoi(e);
  // larger graphs afford a larger dense coarsest level (its inverse costs O(N^3) once per GN
  // iteration, one K-cycle level less halves the coarse-level launches of every PCG iteration).  A SMALLER dense level
  // (one more sparse level) was measured in round 3: the dense inverse gets cheaper but the cycle weaker -- stopping at
  // <= 128 instead of <= 400 nodes: C2 19.6 -> 25.4 PCG iterations (1.76 -> 1.98 ms per GN iteration), C4 22.1 -> 26.5
  // (4.81 -> 5.82 ms); <= 48: C4 30.7 iterations (6.24 ms)
  cfg.coarsest_nodes = std::min(1000, std::max(cfg.coarsest_nodes, n / 1500));
  return cfg;
}

struct AmgHostL0 {
  HostCoarse hc;
  bool ready = false;
  bool agg_only = false;      // hc holds the aggregation only (agg, visit_c, nc; nc == 0: level 0 cannot be coarsened)
  double theta_used = 0.0;
};

#include "sgo_amg_dev.inc"

// Level 0's host analysis made AHEAD of amg_create: amg_host_l0_run is what a helper thread executes once the
// strength weights `w` of the level-0 slots (logical order of H0) are on the host; amg_create(..., pre0) then skips its
// own strength kernel, aggregation and symbolic phase for level 0.  `scratch` is used by the run (and must not be
// touched by anybody else meanwhile).
AmgHostL0* amg_host_l0_new() { return new AmgHostL0(); }
void amg_host_l0_free(AmgHostL0* p) { delete p; }
bool amg_host_l0_ready(const AmgHostL0* p) { return p && p->ready; }
bool amg_host_l0_agg_only(const AmgHostL0* p) { return p && p->ready && p->agg_only; }
void amg_host_l0_run(AmgHostL0* p, const HostLevel& H0, const std::vector<double>& w, const AmgConfig& cfg_in, ChunkArena* scratch, bool agg_only) {
  try {
    const AmgConfig cfg = amg_effective_config(cfg_in, H0.n, H0.nslot);
    if (H0.n <= cfg.coarsest_nodes || 1 >= cfg.max_levels) return;   // amg_create will not coarsen level 0 at all
    if (agg_only) {   // the patterns follow on the device (amg_create with device patterns)
      p->hc.nc = host_aggregate(H0, w, cfg, 0, scratch, p->hc.agg, p->hc.visit_c, &p->theta_used);
      p->agg_only = true;
      p->ready = true;
      return;
    }
    host_coarsen(H0, w, cfg, 0, scratch, p->hc);
    p->ready = p->hc.err.empty();
  } catch (...) {
    p->ready = false;   // amg_create does the work itself (and reports what fails there)
  }
}

namespace {

// ============================================================================================ the level assembler
// The wave-group lists of one level, made as ONE batch: every list's count pass and scan first, one synchronisation for all the group
// counts (they size the lists), then the fill passes -- a level has up to a dozen lists, and on the small levels of a hierarchy the
// set-up's time IS its host round trips.
enum GroupId { G_MEM, G_VAL, G_R, G_T, G_C, G_F, G_GAL, G_ST, G_PSR, G_U, G_APL, G_RAPL, G_COUNT };
struct GroupBatch {
  struct Job {
    const int* ptr = nullptr;
    int nseg = 0, total = 0;
    bool on = false;
    const int** grp = nullptr;   // where run() leaves the list and its group count: the owner's fields
    int* ngrp = nullptr;
  };
  Job job[G_COUNT];
  template <class IntPtr>   // (the owners' fields are int* or const int*)
  void add(GroupId id, const int* ptr, int nseg, int total, IntPtr* grp, int* ngrp) {
    job[id] = Job{ptr, nseg, total, true, (const int**)grp, ngrp};
  }
  // all the pending lists (k_group_jobs): two launches, a scan and one synchronisation; the lists go to the hierarchy's arena and
  // their addresses to the owners the jobs were added with
  bool run(DevSetup& D) {
    GroupJobsDev J;
    int ids[kMaxGroupJobs];
    J.njobs = 0;
    J.chunk0[0] = 0;
    for (int g = 0; g < G_COUNT; ++g) {
      const Job& j = job[g];
      if (!j.on) continue;
      const int q = J.njobs++;
      ids[q] = g;
      J.ptr[q] = j.ptr;
      J.nseg[q] = j.nseg;
      J.total[q] = j.total;
      J.chunk0[q + 1] = J.chunk0[q] + (j.nseg + kGroupChunk - 1) / kGroupChunk + 1;   // (+ the pseudo-chunk of the closing element)
    }
    if (J.njobs == 0) return D.ok;
    const int nch = J.chunk0[J.njobs];
    int* off = D.talloc<int>((size_t)nch + 1);
    int* d_first = D.talloc<int>(kMaxGroupJobs + 1);
    if (!D.ok) return false;
    const dim3 grid((nch + kBlock - 1) / kBlock), block(kBlock);
    SGO_LAUNCH((k_group_jobs<false>), grid, block, 0, D.s, J, off, (int*)nullptr);
    D.scan(off, nch);
    if (!D.ok) return false;
    SGO_LAUNCH(k_gather_ints, dim3(1), dim3(64), 0, D.s, (const int*)off, J, d_first);   // (off[nch] = everything)
    int h_first[kMaxGroupJobs + 1] = {};
    if (hipMemcpyAsync(h_first, d_first, sizeof(int) * (size_t)(J.njobs + 1), hipMemcpyDeviceToHost, D.s) != hipSuccess) D.ok = false;
    if (!D.sync()) return false;
    int* out = D.alloc<int>((size_t)std::max(h_first[J.njobs], 1));
    if (!D.ok) return false;
    SGO_LAUNCH((k_group_jobs<true>), grid, block, 0, D.s, J, off, out);
    for (int q = 0; q < J.njobs; ++q) {
      Job& j = job[ids[q]];
      *j.grp = out + h_first[q];
      *j.ngrp = h_first[q + 1] - h_first[q] - 1;
      j.on = false;
    }
    return D.ok;
  }
};

// The work vectors of level l (the coarser levels: the K-cycle's too, and its partial sums)
bool alloc_work(Amg* m, hipStream_t s, int l) {
  AmgLevel& L = m->lv[l];
  const int n3 = 3 * L.A.n;
  L.spmv_grid = grid_for(L.A.ngrp, kWavesPerBlock);
  L.xs = dev_alloc<double>(m->pool, n3);
  L.rs = dev_alloc<double>(m->pool, n3);
  L.tR = dev_alloc<double>(m->pool, n3);
  if (!L.pos) L.pos = dev_alloc<double>(m->pool, 2 * (size_t)L.A.n);
  if (!L.xs || !L.rs || !L.tR || !L.pos) return false;
  if (l == 0) return true;
  L.bk = dev_alloc<double>(m->pool, n3);
  L.xk = dev_alloc<double>(m->pool, n3);
  L.z1 = dev_alloc<double>(m->pool, n3);
  L.z2 = dev_alloc<double>(m->pool, n3);
  L.q = dev_alloc<double>(m->pool, n3);
  L.bk2 = dev_alloc<double>(m->pool, n3);
  L.p2 = dev_alloc<double>(m->pool, n3);
  L.q2 = dev_alloc<double>(m->pool, n3);
  L.pA = dev_alloc<double>(m->pool, 2 * (size_t)kMaxPartials);
  L.pB = dev_alloc<double>(m->pool, 2 * (size_t)kMaxPartials);
  L.pC = dev_alloc<double>(m->pool, 2 * (size_t)kMaxPartials);
  if (!L.bk || !L.xk || !L.z1 || !L.z2 || !L.q || !L.bk2 || !L.p2 || !L.q2 || !L.pA || !L.pB || !L.pC) return false;
  hipMemsetAsync(L.pA, 0, sizeof(double) * 2 * kMaxPartials, s);
  hipMemsetAsync(L.pB, 0, sizeof(double) * 2 * kMaxPartials, s);
  hipMemsetAsync(L.pC, 0, sizeof(double) * 2 * kMaxPartials, s);
  return true;
}

// A host-made coarsening step (host_coarsen's, or the set-up pipeline's level-0 result) as the DevCoarse the assembler takes.  Row-owner
// level 0 (`own`: this rank's rows [row0, row1)): the P entries, their value products and the A P entries of the rank's rows only --
// allocated for those ranges, base pointers shifted so that global numbers address them -- and the rank's own column order of its
// entries.  One synchronisation at the end: the host vectors, the rank-local ones made here included, may go away after it.
bool upload_coarse(DevSetup& D, const HostCoarse& hc, int n, const HaloDev* own, DevCoarse& o) {
  auto keep = [&](const auto& v) {   // into the hierarchy's arena
    auto* d = dev_upload(D.pool, v, D.s);
    if (!d) D.ok = false;
    return d;
  };
  auto temp = [&](const std::vector<int>& v) {   // used by the set-up only: into the temporary arena
    int* d = dev_upload(D.tmp, v, D.s);
    if (!d) D.ok = false;
    return d;
  };
  auto range = [&](const int* host, int lo, int hi) -> int* {   // host[lo, hi) into the hierarchy's arena, addressed by global numbers
    int* d = D.alloc<int>((size_t)(hi - lo));
    if (!d) return nullptr;
    if (hi > lo) hipMemcpyAsync(d, host + lo, sizeof(int) * (size_t)(hi - lo), hipMemcpyHostToDevice, D.s);
    return d - lo;
  };
  const SaHost& sa = hc.sa;
  const HostLevel& Hc = hc.Hc;
  const int nc = hc.nc;
  o.nc = nc;
  o.smooth = hc.smooth;
  o.filtered = sa.filtered;
  o.agg = keep(hc.agg);
  o.mem_ptr = keep(hc.mem_ptr);
  o.mem = keep(hc.mem);
  o.nslot_c = Hc.nslot;
  o.c_rowptr = keep(Hc.rowptr);
  o.c_row = keep(Hc.row);
  o.c_col = keep(Hc.col);
  std::vector<int> t_pos, t_row, t_col, t_idx, t_ptr;   // row-owner level 0: the rank's column order (live until the synchronisation)
  if (!hc.smooth) {
    o.gal_src = keep(hc.order);
    o.gal_tgt = keep(hc.tgt);
    o.gal_cptr = temp(hc.cptr);
  } else {
    if (own && !sa.lists_on_device) {
      o.err = "amg_create: the row-owner mode needs the device-made product lists (SGO_AMG_LISTS=host is single-GPU only)";
      return false;
    }
    const int r0 = own ? own->row0 : 0, r1 = own ? own->row1 : n;
    o.local = own != nullptr;
    o.np = (int)sa.p_row.size();
    o.e_lo = sa.p_rowptr[r0];
    o.e_hi = sa.p_rowptr[r1];
    o.v_lo = sa.val_rowptr[r0];
    o.nval = sa.val_rowptr[r1] - o.v_lo;
    o.nap = sa.nap;
    o.f_lo = own ? sa.ap_rowptr[r0] : 0;
    o.f_hi = own ? sa.ap_rowptr[r1] : sa.nap;
    o.n_ap_prod = sa.n_ap_prod;
    o.n_rap_prod = sa.n_rap_prod;
    if (sa.filtered) o.strong = keep(sa.strong);
    o.p_rowptr = keep(sa.p_rowptr);
    o.p_row = keep(sa.p_row);
    o.p_col = keep(sa.p_col);
    o.val_ptr = temp(sa.val_ptr);
    o.val_src = range(sa.val_src.p, o.v_lo, o.v_lo + o.nval);
    o.val_tgt = range(sa.val_tgt.p, o.v_lo, o.v_lo + o.nval);
    if (own) {
      // this rank's rows' entries in column order (what the restriction streams and what P^T A P is listed from)
      t_pos.assign((size_t)(o.e_hi - o.e_lo), 0);
      t_ptr.assign((size_t)nc + 1, 0);
      for (int a = 0; a < nc; ++a) {
        for (int t = sa.t_ptr[a]; t < sa.t_ptr[a + 1]; ++t) {
          const int i = sa.t_row[t];
          if (i < r0 || i >= r1) continue;
          const int e = sa.t_idx[t];
          t_pos[(size_t)(e - o.e_lo)] = (int)t_row.size();
          t_row.push_back(i);
          t_col.push_back(a);
          t_idx.push_back(e);
        }
        t_ptr[(size_t)a + 1] = (int)t_row.size();
      }
      o.t_pos = range(t_pos.data() - o.e_lo, o.e_lo, o.e_hi);
      o.t_row = keep(t_row);
      o.t_col = keep(t_col);
      o.t_ptr = temp(t_ptr);
      o.t_idx = temp(t_idx);
    } else {
      o.t_pos = keep(sa.t_pos);
      o.t_row = keep(sa.t_row);
      o.t_col = keep(sa.t_col);
      o.t_ptr = temp(sa.t_ptr);
      if (sa.lists_on_device) o.t_idx = temp(sa.t_idx);
    }
    if (sa.lists_on_device) {
      o.ap_rowptr = temp(sa.ap_rowptr);
      o.ap_col = range(sa.ap_col.p, o.f_lo, o.f_hi);
      o.ap_row = range(sa.ap_row.p, o.f_lo, o.f_hi);
    } else {   // SGO_AMG_LISTS=host: the host's lists, ready-made
      const UVec* a[2] = {&sa.ap_a, &sa.rap_a};
      const UVec* b[2] = {&sa.ap_b, &sa.rap_b};
      const UVec* tgt[2] = {&sa.ap_tgt, &sa.rap_tgt};
      const std::vector<int>* ptr[2] = {&sa.ap_ptr, &sa.rap_ptr};
      for (int w = 0; w < 2; ++w) {
        o.lists[w].a = keep(*a[w]);
        o.lists[w].b = keep(*b[w]);
        o.lists[w].tgt = keep(*tgt[w]);
        o.lists[w].ptr = temp(*ptr[w]);
      }
    }
    o.rap_mirror = keep(sa.rap_mirror);
  }
  if (!D.ok) {
    o.err = "amg_create: out of device memory";
    return false;
  }
  if (!D.sync()) {
    o.err = "amg_create: upload failed";
    return false;
  }
  return true;
}

// ---- the steps of assemble_level, in its order.  Each returns the failure's message, empty on success.  lv[l] is theirs to fill; the
// next level C stays assemble_level's local until every step has run.
const char kOom[] = "amg_create: out of device memory";

// The next level's shell -- structure from the producer; blocks, diagonal inverses and positions allocated -- and what lv[l] holds of
// its aggregates
std::string next_level_shell(Amg* m, DevSetup& D, int l, const DevCoarse& dc, GroupBatch& gb, AmgLevel& C) {
  AmgLevel& L = m->lv[l];
  const int n = L.A.n, nc = dc.nc;
  L.nc = nc;
  L.agg = dc.agg;
  L.mem_ptr = dc.mem_ptr;
  L.mem = dc.mem;
  L.d = D.alloc<double>(2 * (size_t)n);
  C.A.n = nc;
  C.A.nslot = dc.nslot_c;
  C.A.row = dc.c_row;
  C.A.col = dc.c_col;
  C.A.rowptr = dc.c_rowptr;
  C.A.blk = D.alloc<double>(9 * (size_t)dc.nslot_c);
  C.A.dinv = D.alloc<double>(6 * (size_t)nc);
  C.pos = D.alloc<double>(2 * (size_t)nc);
  if (!D.ok) return kOom;
  gb.add(G_MEM, dc.mem_ptr, nc, n, &L.mem_grp, &L.mem_ngrp);
  gb.add(G_C, dc.c_rowptr, nc, dc.nslot_c, &C.A.grp, &C.A.ngrp);
  return std::string();
}

// The two streamed fp32 copies of a transfer's n blocks, numbered from lo: the row-ordered one addressed by global entry numbers, the
// column-ordered one by the positions held
void streamed_copies(DevSetup& D, PDev& P, size_t n, int lo) {
  float* rb = D.alloc<float>(9 * n + 4);
  float* tb = D.alloc<float>(9 * n + 4);
  if (!D.ok) return;
  P.stream_nt = n >= 200000 ? 1 : 0;   // 2 x 72 B per block streamed per cycle: below ~30 MB it may stay cached
  P.r_n = P.t_n = (int)n;
  P.r_blk = rb - 4 * (size_t)lo;
  P.r_blk8 = rb + 8 * n - lo;
  P.t_blk = tb;
  P.t_blk8 = tb + 8 * n;
}

// The arrays of the smoothed transfer P: its pattern and value products from the producer, its blocks, the two streamed fp32 copies
// and the blocks of A P (base pointers shifted so that global numbers address what is held), the filtered operator's diagonals
std::string transfer_arrays(Amg* m, DevSetup& D, int l, const DevCoarse& dc, GroupBatch& gb) {
  AmgLevel& L = m->lv[l];
  PDev& P = L.P;
  const int n = L.A.n;
  const int r0 = dc.local ? m->shard.row0 : 0, r1 = dc.local ? m->shard.row1 : n;   // the rows whose entries are held
  const size_t ne = (size_t)(dc.e_hi - dc.e_lo), nf = (size_t)(dc.f_hi - dc.f_lo);   // entries of P and of A P held
  L.smoothed = true;
  P.local_lists = dc.local;
  if (dc.filtered) {
    P.dF = D.alloc<double>(9 * (size_t)n);
    P.dinvF = D.alloc<double>(9 * (size_t)n);
    P.strong = dc.strong;
    gb.add(G_F, L.A.rowptr, n, L.A.nslot, &P.f_grp, &P.f_ngrp);
  }
  P.np = dc.np;
  P.rowptr = dc.p_rowptr;
  P.row = dc.p_row;
  P.col = dc.p_col;
  P.blk = D.alloc<double>(9 * (size_t)dc.np);
  P.val.n = dc.nval;
  P.val.a = dc.val_src;
  P.val.tgt = dc.val_tgt;
  P.t_pos = dc.t_pos;
  P.t_row = dc.t_row;
  P.t_col = dc.t_col;
  streamed_copies(D, P, ne, dc.e_lo);
  P.nap = dc.nap;
  double* ab = D.alloc<double>(9 * nf);
  if (!D.ok) return kOom;
  P.apblk = ab - 9 * (size_t)dc.f_lo;
  P.rap_mirror = dc.rap_mirror;
  gb.add(G_VAL, dc.val_ptr + dc.e_lo, (int)ne, dc.v_lo + dc.nval, &P.val.grp, &P.val.ngrp);
  gb.add(G_R, dc.p_rowptr + r0, r1 - r0, dc.e_hi, &P.r_grp, &P.r_ngrp);
  gb.add(G_T, dc.t_ptr, dc.nc, (int)ne, &P.t_grp, &P.t_ngrp);
  if (l == 0) m->level0_bytes += (long long)(72 * (size_t)dc.np + 72 * ne + 72 * nf + 8 * (size_t)dc.nval + 12 * ne + 8 * nf);
  return std::string();
}

// The folded cycle's pattern bookkeeping of P~ (the pattern of A P) -- which entry of P sits at the same place, the column order (a
// device radix sort of (column, row-major rank) keys), its wave groups -- the two streamed fp32 copies of the view PS, and on levels
// >= 1 the slots of A and the entries of P~ of every row as one list (k_up_fold)
std::string fold_bookkeeping(Amg* m, DevSetup& D, int l, const DevCoarse& dc, GroupBatch& gb) {
  hipStream_t s = D.s;
  AmgLevel& L = m->lv[l];
  const PDev& P = L.P;
  const int n = L.A.n, nc = dc.nc;
  const int r0 = dc.local ? m->shard.row0 : 0, r1 = dc.local ? m->shard.row1 : n;
  const size_t nf = (size_t)(dc.f_hi - dc.f_lo);
  FoldDev& Fd = L.F;
  Fd.f_lo = dc.f_lo;
  Fd.f_hi = dc.f_hi;
  Fd.row = dc.ap_row;
  Fd.col = dc.ap_col;
  int* a2p = D.alloc<int>(nf);
  int* stp = D.alloc<int>(nf);
  u64* keys = D.talloc<u64>(nf);
  u64* sorted = D.talloc<u64>(nf);
  int bits = 33;
  while (bits < 64 && (1ull << (bits - 32)) <= (u64)nc) ++bits;
  int* st_row = D.alloc<int>(nf);
  int* st_col = D.alloc<int>(nf);
  int* st_ptr = D.alloc<int>((size_t)nc + 1);
  PDev& PS = L.PS;
  PS = PDev();
  streamed_copies(D, PS, nf, dc.f_lo);
  if (!D.ok) return kOom;
  Fd.ap2p = a2p - dc.f_lo;
  Fd.st_pos = stp - dc.f_lo;
  SGO_LAUNCH(k_fold_match, dim3(grid_for((long long)nf, kBlock)), dim3(kBlock), 0, s, Fd, (const int*)P.rowptr, (const int*)P.col, keys);
  if (!D.sort(keys, sorted, nf, bits)) return "amg_create: device sort failed";
  SGO_LAUNCH(k_fold_unpack, dim3(grid_for((long long)nf, kBlock)), dim3(kBlock), 0, s, Fd, (const u64*)sorted, st_row, st_col);
  SGO_LAUNCH(k_fold_colptr, dim3(grid_for((long long)nc + 1, kBlock)), dim3(kBlock), 0, s, (const u64*)sorted, (int)nf, nc, st_ptr);
  PS.np = (int)nf;
  PS.row = dc.ap_row;
  PS.col = dc.ap_col;
  PS.t_row = st_row;
  PS.t_col = st_col;
  gb.add(G_ST, st_ptr, nc, (int)nf, &PS.t_grp, &PS.t_ngrp);
  gb.add(G_PSR, dc.ap_rowptr + r0, r1 - r0, dc.f_hi, &PS.r_grp, &PS.r_ngrp);
  if (l > 0) {
    const int un = L.A.nslot + (int)nf;
    int* u_ptr = D.alloc<int>((size_t)n + 1);
    int* u_row = D.alloc<int>((size_t)un);
    int* u_idx = D.alloc<int>((size_t)un);
    int* u_col = D.alloc<int>((size_t)un);
    if (!D.ok) return kOom;
    SGO_LAUNCH(k_u_ptr, dim3(grid_for((long long)n + 1, kBlock)), dim3(kBlock), 0, s, n, (const int*)L.A.rowptr, (const int*)dc.ap_rowptr, u_ptr);
    SGO_LAUNCH(k_u_fill, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, n, (const int*)L.A.rowptr, (const int*)L.A.col, (const int*)dc.ap_rowptr,
               (const int*)dc.ap_col, (const int*)u_ptr, u_row, u_idx, u_col);
    UpDev& U = L.U;
    U.n = un;
    U.row = u_row;
    U.idx = u_idx;
    U.col = u_col;
    gb.add(G_U, u_ptr, n, un, &U.grp, &U.ngrp);
  }
  if (l == 0) m->level0_bytes += (long long)(72 * nf + 28 * nf);
  return std::string();
}

// One pass of a product list from the patterns -- w == 0: A P, w == 1: P^T A P; the count pass leaves every target's count at ptr, the
// fill pass (ptr scanned) the products at la / lb / lt
template <bool FILL>
void launch_product_list(hipStream_t s, int w, const ApPattern& ap, const AmgLevel& L, const AmgLevel& C, const DevCoarse& dc, int nseg, int* ptr,
                         int* la, int* lb, int* lt) {
  const dim3 grid(grid_for(8LL * nseg, kBlock)), block(kBlock);   // eight lanes per target
  if (w == 0)
    SGO_LAUNCH((k_ap_list<FILL>), grid, block, 0, s, ap, (const int*)L.A.rowptr, (const int*)L.A.col, (const int*)L.P.rowptr,
               (const int*)L.P.col, ptr, la, lb, lt);
  else
    SGO_LAUNCH((k_rap_list<FILL>), grid, block, 0, s, dc.nslot_c, (const int*)C.A.row, (const int*)C.A.col, (const int*)dc.t_ptr,
               (const int*)L.P.t_row, (const int*)dc.t_idx, ap, ptr, la, lb, lt);
}

// The product lists of A P and P^T A P: the producer's ready-made ones, or made here from the patterns
std::string product_lists(Amg* m, DevSetup& D, int l, const DevCoarse& dc, GroupBatch& gb, const AmgLevel& C) {
  hipStream_t s = D.s;
  AmgLevel& L = m->lv[l];
  PDev& P = L.P;
  char line[160];
  std::snprintf(line, sizeof line, "(P %d%s, AP %d blocks; %d + %d products) ", P.np, dc.filtered ? " filtered" : "", P.nap, (int)dc.n_ap_prod,
                (int)dc.n_rap_prod);
  m->desc += line;
  ProdMap* maps[2] = {&P.ap, &P.rap};
  const GroupId gid[2] = {G_APL, G_RAPL};
  const long long nprod[2] = {dc.n_ap_prod, dc.n_rap_prod};
  const int nseg[2] = {dc.f_hi - dc.f_lo, dc.nslot_c};
  if (dc.lists[0].a) {   // ready-made: grouped with the level's batch
    for (int w = 0; w < 2; ++w) {
      maps[w]->n = (int)nprod[w];
      maps[w]->a = dc.lists[w].a;
      maps[w]->b = dc.lists[w].b;
      maps[w]->tgt = dc.lists[w].tgt;
      gb.add(gid[w], dc.lists[w].ptr, nseg[w], (int)nprod[w], &maps[w]->grp, &maps[w]->ngrp);
    }
    return std::string();
  }
  // from the patterns: count per target, prefix sum, fill (A P, then P^T A P); both lists' totals behind one synchronisation
  ApPattern ap;
  ap.ap_row = dc.ap_row;
  ap.ap_col = dc.ap_col;
  ap.ap_rowptr = dc.ap_rowptr;
  ap.f_lo = dc.f_lo;
  ap.nap = dc.f_hi;
  int* ptrs[2] = {nullptr, nullptr};   // [nseg + 1] each, from the first target held
  int* ptr[2] = {nullptr, nullptr};    // ... addressed by global target numbers
  for (int w = 0; w < 2; ++w) {
    ptrs[w] = D.talloc<int>((size_t)nseg[w] + 1);
    int* sums = D.talloc<int>((size_t)nseg[w] / kScanChunk + 3);
    if (!D.ok) return kOom;
    ptr[w] = w == 0 ? ptrs[w] - dc.f_lo : ptrs[w];
    launch_product_list<false>(s, w, ap, L, C, dc, nseg[w], ptr[w], nullptr, nullptr, nullptr);
    dev_scan_exclusive(s, ptrs[w], nseg[w], sums);
  }
  int totals[2] = {-1, -1};
  D.read2(ptrs[0] + nseg[0], ptrs[1] + nseg[1], &totals[0], &totals[1]);
  if (!D.ok) return "amg_create: product-list kernels failed";
  for (int w = 0; w < 2; ++w) {
    const int total = totals[w];
    // (whole ranges: exactly the patterns' count; a rank's own rows: at most that)
    if ((!dc.local && total != nprod[w]) || total < 0 || total > nprod[w])
      return "amg_create: internal error (device product lists: " + std::to_string(total) + " products, the patterns say " +
             std::to_string(nprod[w]) + ")";
    int* la = D.alloc<int>((size_t)std::max(total, 1));
    int* lb = D.alloc<int>((size_t)std::max(total, 1));
    int* lt = D.alloc<int>((size_t)std::max(total, 1));
    if (!D.ok) return kOom;
    launch_product_list<true>(s, w, ap, L, C, dc, nseg[w], ptr[w], la, lb, lt);
    maps[w]->n = total;
    maps[w]->a = la;
    maps[w]->b = lb;
    maps[w]->tgt = lt;
    gb.add(gid[w], ptrs[w], nseg[w], total, &maps[w]->grp, &maps[w]->ngrp);
    if (l == 0) m->level0_bytes += 12LL * total;   // (the lists made here: the level-0 bytes have never counted ready-made ones)
  }
  return std::string();
}

// The long columns of the two column-ordered copies (P's and, folded, P~'s), behind the wave groups: one synchronisation for both counts
std::string long_columns(Amg* m, DevSetup& D, int l, bool fold_here) {
  hipStream_t s = D.s;
  AmgLevel& L = m->lv[l];
  PDev &P = L.P, &PS = L.PS;
  int* d_cnt = D.talloc<int>(2);
  int* t_ranges = D.alloc<int>(2 * (size_t)std::max(P.t_ngrp, 1));
  int* st_ranges = nullptr;
  if (!D.ok) return kOom;
  hipMemsetAsync(d_cnt, 0, 2 * sizeof(int), s);
  SGO_LAUNCH(k_long_groups, dim3(grid_for((long long)P.t_ngrp, kBlock)), dim3(kBlock), 0, s, (const int*)P.t_grp, P.t_ngrp, d_cnt, t_ranges);
  if (fold_here) {
    st_ranges = D.alloc<int>(2 * (size_t)std::max(PS.t_ngrp, 1));
    if (!D.ok) return kOom;
    SGO_LAUNCH(k_long_groups, dim3(grid_for((long long)PS.t_ngrp, kBlock)), dim3(kBlock), 0, s, (const int*)PS.t_grp, PS.t_ngrp, d_cnt + 1, st_ranges);
  }
  int nl[2] = {0, 0};
  D.read2(d_cnt, d_cnt + 1, &nl[0], &nl[1]);
  if (!D.ok) return "amg_create: set-up kernels failed";
  P.t_nlong = nl[0];
  P.t_long = nl[0] ? t_ranges : nullptr;
  if (fold_here) {
    constexpr int kLongCap = 4096;   // a level with more long columns than this is not folded
    PS.t_long = st_ranges;
    PS.t_nlong = nl[1];
    L.fold = nl[1] <= kLongCap;
  }
  return std::string();
}

// The one level assembler: a coarsening step's DevCoarse, whichever producer made it, into the transfer data of lv[l] -- P and its
// streamed fp32 copies, the folded cycle's bookkeeping, the product lists, every wave-group list of the level in one batch (each step
// adds its lists with the fields they go to), the long columns -- and the structure of the next level lv[l + 1].  Returns the
// failure's message, empty on success.
std::string assemble_level(Amg* m, DevSetup& D, int l, const DevCoarse& dc) {
  GroupBatch gb;
  AmgLevel C;
  const bool fold_here = dc.smooth && fold_level(m, l, dc.f_hi - dc.f_lo);
  std::string e = next_level_shell(m, D, l, dc, gb, C);
  if (e.empty() && dc.smooth) e = transfer_arrays(m, D, l, dc, gb);
  if (e.empty() && fold_here) e = fold_bookkeeping(m, D, l, dc, gb);
  if (e.empty() && dc.smooth) e = product_lists(m, D, l, dc, gb, C);
  if (!e.empty()) return e;
  if (!dc.smooth) {   // tentative transfer: the Galerkin map
    AmgLevel& L = m->lv[l];
    L.gal.n = L.A.nslot;
    L.gal.src = dc.gal_src;
    L.gal.tgt = dc.gal_tgt;
    gb.add(G_GAL, dc.gal_cptr, dc.nslot_c, L.A.nslot, &L.gal.grp, &L.gal.ngrp);
  }
  if (!gb.run(D)) return kOom;
  if (dc.smooth) e = long_columns(m, D, l, fold_here);
  if (!e.empty()) return e;
  m->lv.push_back(C);   // invalidates lv[l]'s address: no step holds a reference across this
  return std::string();
}

// Multi-GPU row-owner mode, level 0, between its assembly and its first values: the entries of P in every rank's boundary rows -- what
// A P of a neighbour's rows gathers from this rank's P -- and exchange buffers large enough for them.  nullptr or the failure's message.
const char* boundary_entries(hipStream_t s, DevArena* pool, const AmgHalo& halo, const std::vector<int>& p_rowptr) {
  std::vector<std::vector<int>> pe((size_t)halo.G);
  int pemax = 1;
  for (int q = 0; q < halo.G; ++q) {
    for (int t = 0; t < halo.bmax; ++t) {
      const int r = halo.bnd_host[(size_t)q * halo.bmax + t];
      if (r < 0) break;
      for (int e = p_rowptr[r]; e < p_rowptr[r + 1]; ++e) pe[q].push_back(e);
    }
    pemax = std::max(pemax, (int)pe[q].size());
  }
  std::vector<int> flat((size_t)halo.G * pemax, -1);
  for (int q = 0; q < halo.G; ++q) std::copy(pe[q].begin(), pe[q].end(), flat.begin() + (size_t)q * pemax);
  int* d_pe = dev_upload(pool, flat, s);
  if (!d_pe || hipStreamSynchronize(s) != hipSuccess) return "amg_create: out of device memory";
  halo.dev->pemax = pemax;
  halo.dev->pent = d_pe;
  if (halo.reserve && !halo.reserve(halo.user, (size_t)kHaloScalars + 9 * (size_t)pemax)) return "amg_create: out of device memory (exchange buffers)";
  return nullptr;
}

// The first values of level l + 1 (its strengths need them): positions, centres and lever arms, the Galerkin operator, the diagonal
// inverses.  No synchronisation: the next level's strengths are read behind its own, the hierarchy's last level behind amg_create's.
void level_values(Amg* m, hipStream_t s, int l) {
  AmgLevel& L = m->lv[l];
  AmgLevel& C = m->lv[l + 1];
  const int n = L.A.n, nc = C.A.n;
  if (l == 0) SGO_LAUNCH(k_positions0, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, n, m->d_free_id, m->d_poses, L.pos);
  SGO_LAUNCH(k_centres, dim3(grid_for(nc, kWavesPerBlock)), dim3(kBlock), 0, s, nc, L.mem_ptr, L.mem, L.pos, C.pos, L.d);
  launch_coarse_operator(m, s, L, C, l == 0);
  if (l + 1 < m->cfg.max_levels) SGO_LAUNCH(k_level_dinv, dim3(grid_for(C.A.n, kBlock)), dim3(kBlock), 0, s, C.A.n, (const int*)C.A.rowptr, C.A);
}

double ms_since(std::chrono::steady_clock::time_point t) {
  return 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
}

// The strengths of connection of a level from its current values: the block norms of its nslot slots, on the device (temporary arena;
// dev_coarsen takes them from there) and in w on the host, behind one synchronisation.  nullptr: failed, the message in err.
double* level_strengths(DevSetup& D, const BsrDev& A, int nslot, std::vector<double>& w, std::string& err) {
  w.resize((size_t)nslot);
  double* d_w = D.talloc<double>((size_t)std::max(nslot, 1));
  if (!d_w) {
    err = kOom;
    return nullptr;
  }
  SGO_LAUNCH(k_block_norms, dim3(grid_for(nslot, kBlock)), dim3(kBlock), 0, D.s, A, d_w);
  hipMemcpyAsync(w.data(), d_w, sizeof(double) * (size_t)nslot, hipMemcpyDeviceToHost, D.s);
  if (!D.sync()) {
    err = "amg_create: strength kernel failed";
    return nullptr;
  }
  return d_w;
}

// The aggregates a rebuild keeps for level l of n nodes (AmgConfig::keep_agg), where they fit; nullptr: none
const AmgKeptAgg* kept_aggregates(const Amg* m, int l, int n) {
  const AmgKeptAgg* k = m->cfg.keep_agg;
  return k && l < (int)k->agg.size() && (int)k->agg[l].size() == n ? k : nullptr;
}

bool refuse(DevCoarse& dc, const char* msg) {   // a producer's failure
  dc.err = msg;
  return false;
}

// The two producers of level l's DevCoarse.  Both return false on a failure (the message in dc.err), set dc.stop where the level
// cannot be coarsened further, and leave the host copies of the aggregates (h_agg) and of the next level's visiting order (h_visit_c)
// and the milliseconds of the host's aggregation (t_host_agg).
//
// On the host: host_coarsen's result -- or, for level 0, the one the set-up pipeline's helper thread made ahead (pre0) -- uploaded.
// `hc` is the HostCoarse it came from (the helper thread's, or hc_own).
bool coarsen_on_host(Amg* m, DevSetup& D, int l, const HostLevel& H, ChunkArena* scratch, AmgHostL0* pre0, const AmgHalo* halo, bool verbose,
                     HostCoarse& hc_own, HostCoarse*& hc, std::vector<int>& h_agg, std::vector<int>& h_visit_c, double& t_host_agg, DevCoarse& dc) {
  const int n = m->lv[l].A.n;
  hc = &hc_own;
  if (l == 0 && pre0 && pre0->ready && !pre0->agg_only) {
    hc = &pre0->hc;   // made ahead on the helper thread, from the same structure and the strengths at the same poses
  } else {
    // strength of connection from the current values of this level
    std::vector<double> w;
    if (l == 0 && halo) {
      if (!halo->w0 || (int)halo->w0->size() != H.nslot) return refuse(dc, "amg_create: row-owner mode needs the level-0 strength weights");
      w = *halo->w0;
    } else if (!level_strengths(D, m->lv[l].A, H.nslot, w, dc.err)) {
      return false;
    }
    if (const AmgKeptAgg* k = kept_aggregates(m, l, n)) {
      hc_own.agg = k->agg[l];
      hc_own.visit_c = k->visit_c[l];
      hc_own.nc = k->nc[l];
      hc_own.reuse_agg = true;
    }
    host_coarsen(H, w, m->cfg, l, scratch, hc_own);
  }
  if (!hc->err.empty()) return refuse(dc, hc->err.c_str());
  if (hc->stop) {
    dc.stop = true;
    return true;
  }
  if (verbose)
    std::fprintf(stderr, "[sgo] amg level %d: host aggregation + coarse structure %.1f ms (aggregate %.1f, sort %.1f; n=%d -> %d)%s\n", l,
                 hc->t_all, hc->t_agg, hc->t_sort, n, hc->nc, hc == &hc_own ? "" : " [made ahead on the helper thread]");
  h_agg = hc->agg;
  h_visit_c = hc->visit_c;
  t_host_agg = hc->t_agg;
  return upload_coarse(D, *hc, n, l == 0 && halo ? halo->dev : nullptr, dc);
}

// On the device: dev_coarsen from given aggregates -- kept ones, the helper thread's (level 0, pre0), or the host's (greedy along the
// trajectory, sgo_amg_host.cpp: from this level's strengths and its pattern, which for a coarse level is copied back into Hown, a few
// integers per slot) -- or, given none (AmgPatterns::device_aggregation), from the device's own.
bool coarsen_on_device(Amg* m, DevSetup& D, int l, const HostLevel& H0, HostLevel& Hown, AmgPatterns patterns, ChunkArena* scratch,
                       AmgHostL0* pre0, std::vector<double>& h_w, std::vector<int>& h_agg, std::vector<int>& h_visit_c, double& t_host_agg,
                       DevCoarse& dc) {
  hipStream_t s = D.s;
  const BsrDev& A = m->lv[l].A;
  const int n = A.n;
  int given_nc = 0;
  double given_theta = (l == 0 ? m->cfg.theta : m->cfg.theta_coarse) * m->cfg.theta_scale;
  double* d_w = nullptr;
  if (const AmgKeptAgg* k = kept_aggregates(m, l, n)) {
    h_agg = k->agg[l];
    h_visit_c = k->visit_c[l];
    given_nc = k->nc[l];
  } else if (l == 0 && pre0 && pre0->ready && pre0->agg_only) {
    // level 0's aggregation was made ahead on the helper thread (sgo_set_graph_se2's pipeline), from the same structure and the
    // strengths at the same poses
    h_agg = pre0->hc.agg;
    h_visit_c = pre0->hc.visit_c;
    given_nc = pre0->hc.nc;
    given_theta = pre0->theta_used;
    dc.stop = given_nc == 0;
  } else if (patterns == AmgPatterns::device) {
    if (l > 0) {
      Hown.n = n;
      Hown.nslot = A.nslot;
      Hown.rowptr.resize((size_t)n + 1);
      Hown.col.resize((size_t)A.nslot);
      Hown.row.clear();
      hipMemcpyAsync(Hown.rowptr.data(), A.rowptr, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, s);
      hipMemcpyAsync(Hown.col.data(), A.col, sizeof(int) * (size_t)A.nslot, hipMemcpyDeviceToHost, s);
    }
    const HostLevel& H = l == 0 ? H0 : Hown;
    if (!(d_w = level_strengths(D, A, H.nslot, h_w, dc.err))) return false;
    const auto tA = std::chrono::steady_clock::now();
    given_nc = host_aggregate(H, h_w, m->cfg, l, scratch, h_agg, h_visit_c, &given_theta);
    t_host_agg = ms_since(tA);
    dc.stop = given_nc == 0;
  }
  if (dc.stop) return true;
  int* given = nullptr;   // (none: dev_coarsen aggregates)
  if (!h_agg.empty() && !(given = dev_upload(D.tmp, h_agg, s))) return refuse(dc, kOom);
  if (!dev_coarsen(D, A, m->cfg, l, given, given_nc, given_theta, d_w, dc)) return dc.err.empty() ? refuse(dc, "amg_create: device set-up failed") : false;
  if (!dc.stop && h_agg.empty()) {   // (the device's aggregates)
    h_agg.resize((size_t)n);
    if (hipMemcpyAsync(h_agg.data(), dc.agg, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s) != hipSuccess || !D.sync())
      return refuse(dc, "amg_create: device set-up failed");
  }
  return true;
}

// Behind the last level: the dense inverse's buffers for it, the sweeps per coarse level, the description's tail.  Returns the
// failure's message, empty on success.
std::string finish_coarsest(Amg* m, hipStream_t s) {
  if (hipStreamSynchronize(s) != hipSuccess) return "amg_create: set-up kernels failed";
  const int last = (int)m->lv.size() - 1;
  // last == 0: the whole graph is at most coarsest_nodes large (or cannot be coarsened) and is
  // "solved" by the dense inverse directly -- the preconditioner is then exact (1-2 PCG iterations)
  if (last == 0 && m->lv[0].A.n > 1024) return "amg_create: graph not coarsenable; use the block-Jacobi solver";
  m->N = 3 * m->lv[last].A.n;
  m->Np = (m->N + kGjB - 1) / kGjB * kGjB;
  if (m->N > 3072) return "amg_create: coarsest level too large (" + std::to_string(m->N) + " unknowns)";
  m->inv0 = dev_alloc<double>(m->pool, (size_t)m->Np * m->Np);
  m->inv1 = dev_alloc<double>(m->pool, (size_t)m->Np * m->Np);
  m->gjP[0] = dev_alloc<double>(m->pool, kGjB * kGjB);
  m->gjP[1] = dev_alloc<double>(m->pool, kGjB * kGjB);
  m->inv = ((m->Np / kGjB) & 1) ? m->inv1 : m->inv0;
  m->d_fail = dev_alloc<int>(m->pool, 1);
  if (!m->inv0 || !m->inv1 || !m->d_fail || !m->gjP[0] || !m->gjP[1]) return kOom;
  hipMemsetAsync(m->d_fail, 0, sizeof(int), s);
  // Two sweeps per coarse level (amg_effective_config) pay while the coarse levels are small next to level 0.  A hierarchy
  // whose level 1 holds more than a quarter of level 0's blocks -- filtered transfers along the trajectory: aggregates of three
  // poses whose rows keep all their closures, C4 from a dead-reckoned start: 1.15 M of 2.1 M -- pays four bandwidth-bound
  // passes per level for them: one sweep there (measured: 23.3 -> 20.9 ms per Gauss-Newton iteration at that start; C4's usual
  // hierarchy, level 1 at 6 %, keeps two: 4.06 against 4.45 ms with one).
  if (last >= 1 && !m->cfg.nu_from_env && 4LL * m->lv[1].A.nslot > (long long)m->lv[0].A.nslot) m->cfg.nu_coarse = 1;
  m->cfg.keep_agg = nullptr;   // (the caller's object: only read during this set-up)
  char line[160];
  std::snprintf(line, sizeof line, "coarsest dense N=%d; theta=%.3g omega=%.2f nu=%d", m->N,
                m->cfg.theta * m->cfg.theta_scale, m->cfg.omega, m->cfg.nu_coarse);
  m->desc += line;
  return std::string();
}

}  // namespace

Amg* amg_create(hipStream_t s, const BsrDev& A0, const Sym0Dev& S0, const Tile0Dev& T0, const HostLevel& H0, const double* d_poses,
                const int* d_free_id, const AmgConfig& cfg_in, const AmgProf& prof, std::string* err, ChunkArena* scratch, DevArena* arena,
                DevArena* tmp_arena, AmgPatterns patterns, AmgHostL0* pre0, const AmgHalo* halo) {
  Amg* m = new Amg();
  if (halo) {   // row-owner mode
    const HaloDev& H = *halo->dev;
    m->shard.mode = Shard0::owner;
    m->shard.u0 = H.u0; m->shard.u1 = H.u1; m->shard.row0 = H.row0; m->shard.row1 = H.row1;
    m->shard.G = H.G;
    m->shard.comm = H.comm;
    m->shard.part = halo->dev;
  }
  m->pool = arena;
  m->S0 = S0;
  m->T0 = T0;
  m->cfg = amg_effective_config(cfg_in, A0.n, A0.nslot);
  const bool on_host = patterns == AmgPatterns::host;
  if (!on_host) m->cfg.lists_on_device = true;   // (the device producer makes patterns only; folding stays as amg_effective_config decided)
  m->kdepth = m->cfg.kdepth;
  m->fcg2_depth = m->cfg.fcg2_depth;
  m->prof = prof;
  m->d_poses = d_poses;
  m->d_free_id = d_free_id;
  auto fail = [&](const std::string& msg) -> Amg* {
    if (err) *err = msg;
    amg_destroy(m);
    return nullptr;
  };
  if (halo && !on_host) return fail("amg_create: the row-owner mode needs the host patterns");
  const bool verbose = std::getenv("SGO_VERBOSE") != nullptr;
  AmgLevel L0;
  L0.A = A0;
  m->lv.push_back(L0);
  char line[160];
  HostLevel Hown;   // structure of a level l > 0 that the host coarsens or aggregates: the host producer's, or copied back from the device
  std::vector<double> h_w;
  for (int l = 0;; ++l) {
    const int n = m->lv[l].A.n;
    std::snprintf(line, sizeof line, "L%d n=%d slots=%d; ", l, n, m->lv[l].A.nslot);
    m->desc += line;
    if (!alloc_work(m, s, l)) return fail(kOom);
    if (n <= m->cfg.coarsest_nodes || l + 1 >= m->cfg.max_levels) break;

    const auto tL = std::chrono::steady_clock::now();
    tmp_arena->rewind();   // (the previous level's temporaries: every later user is queued behind their last kernel)
    DevSetup D{s, m->pool, tmp_arena};
    DevCoarse dc;
    HostCoarse hc_own;
    HostCoarse* hc = nullptr;            // the host producer's result
    std::vector<int> h_agg, h_visit_c;   // host copies of the aggregates (AmgConfig::keep_agg) and of the next level's visiting order
    double t_host_agg = 0.0;
    const bool made = on_host ? coarsen_on_host(m, D, l, l == 0 ? H0 : Hown, scratch, pre0, halo, verbose, hc_own, hc, h_agg, h_visit_c, t_host_agg, dc)
                              : coarsen_on_device(m, D, l, H0, Hown, patterns, scratch, pre0, h_w, h_agg, h_visit_c, t_host_agg, dc);
    if (!made) return fail(dc.err);
    if (dc.stop) break;   // cannot coarsen further
    const double t_coarsen = ms_since(tL);
    m->kept.agg.push_back(std::move(h_agg));
    m->kept.visit_c.push_back(h_visit_c);
    m->kept.nc.push_back(dc.nc);
    const std::string e = assemble_level(m, D, l, dc);
    if (!e.empty()) return fail(e);
    if (l == 0 && halo && dc.smooth)
      if (const char* be = boundary_entries(s, m->pool, *halo, hc->sa.p_rowptr)) return fail(be);
    level_values(m, s, l);
    if (verbose)
      std::fprintf(stderr, "[sgo] amg level %d, patterns on the %s: %.2f ms (of which the host's aggregation %.2f), assembly %.2f ms, "
                   "%d synchronisations (n=%d -> %d, %s)\n", l, on_host ? "host" : "device", t_coarsen, t_host_agg, ms_since(tL) - t_coarsen,
                   D.syncs, n, dc.nc, dc.smooth ? (dc.filtered ? "filtered smoothing" : "smoothed") : "tentative");
    if (on_host) Hown = std::move(hc->Hc);
    Hown.visit = std::move(h_visit_c);   // (the order in which the next level's aggregation visits its nodes: along the trajectory)
  }
  const std::string e = finish_coarsest(m, s);
  if (!e.empty()) return fail(e);
  return m;
}

}  // namespace sgo
