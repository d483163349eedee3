// sgo_gate.hip -- the kernels behind sgo_gate_edges / sgo_set_edge_information / sgo_set_robust_kernels / sgo_edge_robust
// (include/sgo.h): the chi2 gate of log_runner.cpp:182-189 on the device, and an edge's information, or its robust kernel (kind
// and parameter), rewritten in every array that holds a copy of it.
//
// "Removed" is "information = 0": such an edge adds nothing to chi2, to the right-hand side or to any Hessian block, and DCS gives
// it weight 1, so every resident structure (row plan, tiles, elimination trees, overlay, multigrid patterns) stays valid and no
// kernel of the solve changes.  The copies of an edge's information:
//   EdgeListDev::info  (c->el)           k_chi2, k_direct, k_mf_edges, k_row_strength
//   EdgeSlotsDev::info (c->es)           k_linearize: one copy per compact slot of the edge (k_slot_expand made them)
//   OverlayDev::el.info                  the overlay kernels, for the edges an incremental update appended
// The robust kernel's pair (phi, kind) has the same three homes -- EdgeListDev::phi / kind, EdgeSlotsDev::phi / kind,
// OverlayDev::el.phi / kind -- and the same two sweeps (k_edge_kernel_scatter, k_slot_kernel_refresh).
// Streaming kernels, one lane per item, vector stores only, no atomics; the gate's count goes through block_sum_store /
// block_reduce_parts like every other reduction here.
#include <algorithm>

#include "sgo_device.h"
#include "sgo_internal.h"

namespace sgo {
namespace {

// e^T Omega e of edge k of `el` at the current poses: the very sequence chi2_range (sgo_kernels.hip) evaluates, so the
// gate's decision is sgo_edge_chi2's value compared with chi2_max, bit for bit
__device__ __forceinline__ double gate_e2(const EdgeListDev& el, int k, const double* __restrict__ poses) {
  EdgeOperands p;
  edge_operands(el, (size_t)el.E, k, poses, p);
  double sz, cz, e[3];
  sincos(p.zt, &sz, &cz);
  edge_error(p, sz, cz, e);
  EdgeWeight W;
  edge_weight<false>(el, (size_t)el.E, k, e, W);   // (e2 alone: the kernel's pair is never formed)
  return W.e2;
}

// Item t is edge ids[t] (ids == nullptr: edge t, and only edges with a kernel, phi >= 0, are gated); ids below el.E are the
// resident list's, the others the overlay list's first el2.cnt.  flag[t] = chi2 > chi2_max; partials[block] = the block's count.
// Reads the graph, writes flag and partials only.
__global__ __launch_bounds__(kBlock) void k_edge_gate(EdgeListDev el, EdgeListDev el2, int n, const int* __restrict__ ids,
                                                      const double* __restrict__ poses, double chi2_max,
                                                      unsigned char* __restrict__ flag, double* __restrict__ partials) {
  double acc[1] = {0.0};
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
    const int id = ids ? ids[t] : t;
    bool hit = false;
    if (id >= 0 && id < el.E) {
      if (ids || el.phi[id] >= 0.0) hit = gate_e2(el, id, poses) > chi2_max;
    } else if (id >= el.E && id - el.E < el2.cnt) {
      const int k = id - el.E;
      if (ids || el2.phi[k] >= 0.0) hit = gate_e2(el2, k, poses) > chi2_max;
    }
    flag[t] = hit ? 1 : 0;
    acc[0] += hit ? 1.0 : 0.0;
  }
  block_sum_store<1>(acc, partials, kMaxPartials);
}
__global__ __launch_bounds__(kBlock) void k_gate_count(const double* __restrict__ partials, int nparts, int* __restrict__ count) {
  const double s = block_reduce_parts(partials, nparts);   // (whole numbers below 2^31: exact)
  if (threadIdx.x == 0) *count = (int)s;
}

// The six SoA components of the listed edges from rows[n][6] (upper triangles, the caller's layout), in the resident list
// (stride el.E) or the overlay's (stride el2.E, its capacity); mark[id] = 1 for the resident ones when the per-slot copies
// exist (k_slot_info_refresh).  The host lists every id once.
__global__ __launch_bounds__(kBlock) void k_edge_info_scatter(int n, const int* __restrict__ ids, const double* __restrict__ rows,
                                                              EdgeListDev el, EdgeListDev el2, unsigned char* __restrict__ mark) {
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
    const int id = ids[t];
    const double* r = rows + 6 * (size_t)t;
    if (id >= 0 && id < el.E) {
      const size_t E = (size_t)el.E;
#pragma unroll
      for (int q = 0; q < 6; ++q) el.info[q * E + (size_t)id] = r[q];
      if (mark) mark[id] = 1;
    } else if (id >= el.E && id - el.E < el2.cnt) {
      const size_t E2 = (size_t)el2.E, k = (size_t)(id - el.E);
#pragma unroll
      for (int q = 0; q < 6; ++q) el2.info[q * E2 + k] = r[q];
    }
  }
}

// dead[id] = the edge's information is all zero, over both lists (ids as above): what the host's bookkeeping starts from
__global__ __launch_bounds__(kBlock) void k_edge_dead_flags(EdgeListDev el, EdgeListDev el2, unsigned char* __restrict__ dead) {
  const int n = el.E + el2.cnt;
  for (int id = blockIdx.x * kBlock + threadIdx.x; id < n; id += gridDim.x * kBlock) {
    const bool base = id < el.E;
    const double* info = base ? el.info : el2.info;
    const size_t stride = (size_t)(base ? el.E : el2.E), k = (size_t)(base ? id : id - el.E);
    bool zero = true;
#pragma unroll
    for (int q = 0; q < 6; ++q) zero = zero && info[q * stride + k] == 0.0;
    dead[id] = zero ? 1 : 0;
  }
}

// One sweep over the compact slots: a slot whose edge (eidx: slot -> edge of the resident list) is marked takes its six
// information components from the edge list -- the information part of k_slot_expand (sgo_kernels.hip).
__global__ __launch_bounds__(kBlock) void k_slot_info_refresh(int ncs, const int* __restrict__ eidx, const unsigned char* __restrict__ mark,
                                                              EdgeListDev el, EdgeSlotsDev es) {
  const size_t ns = (size_t)es.stride, E = (size_t)el.E;
  for (int k = blockIdx.x * kBlock + threadIdx.x; k < ncs; k += gridDim.x * kBlock) {
    if (es.flags[k] & kSlotNoEdge) continue;
    const int e = eidx[k];
    if (e < 0 || e >= el.E || !mark[e]) continue;
#pragma unroll
    for (int q = 0; q < 6; ++q) es.info[q * ns + (size_t)k] = el.info[q * E + (size_t)e];
  }
}

// The robust kernel of the listed edges -- parameter delta[t] into phi, kind[t] (a RobustKind byte) beside it --, in the resident
// list or the overlay's; mark[id] = 1 for the resident ones when the per-slot copies exist.  The host lists every id once.
__global__ __launch_bounds__(kBlock) void k_edge_kernel_scatter(int n, const int* __restrict__ ids, const double* __restrict__ delta,
                                                                const unsigned char* __restrict__ kind, EdgeListDev el, EdgeListDev el2,
                                                                unsigned char* __restrict__ mark) {
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
    const int id = ids[t];
    if (id >= 0 && id < el.E) {
      el.phi[id] = delta[t];
      el.kind[id] = kind[t];
      if (mark) mark[id] = 1;
    } else if (id >= el.E && id - el.E < el2.cnt) {
      el2.phi[id - el.E] = delta[t];
      el2.kind[id - el.E] = kind[t];
    }
  }
}
// The robust-kernel part of k_slot_expand for the slots of marked edges (as k_slot_info_refresh).
__global__ __launch_bounds__(kBlock) void k_slot_kernel_refresh(int ncs, const int* __restrict__ eidx, const unsigned char* __restrict__ mark,
                                                                EdgeListDev el, EdgeSlotsDev es) {
  for (int k = blockIdx.x * kBlock + threadIdx.x; k < ncs; k += gridDim.x * kBlock) {
    if (es.flags[k] & kSlotNoEdge) continue;
    const int e = eidx[k];
    if (e < 0 || e >= el.E || !mark[e]) continue;
    es.phi[k] = el.phi[e];
    es.kind[k] = el.kind[e];
  }
}

// rho0[id], w[id] of every edge over both lists at the current poses: the sequence chi2_range evaluates, with the pair stored
// instead of summed (either pointer may be null).
template <bool KINDS>
__device__ __forceinline__ void robust_range(const EdgeListDev& el, int cnt, const double* __restrict__ poses, double* __restrict__ rho0,
                                             double* __restrict__ w) {
  for (int k = blockIdx.x * kBlock + threadIdx.x; k < cnt; k += gridDim.x * kBlock) {
    EdgeOperands p;
    edge_operands(el, (size_t)el.E, k, poses, p);
    double sz, cz, e[3];
    sincos(p.zt, &sz, &cz);
    edge_error(p, sz, cz, e);
    EdgeWeight W;
    edge_weight<KINDS>(el, (size_t)el.E, k, e, W);
    if (rho0) rho0[k] = W.rho0;
    if (w) w[k] = W.w;
  }
}
template <bool KINDS>
__global__ __launch_bounds__(kBlock) void k_edge_robust(EdgeListDev el, EdgeListDev el2, const double* __restrict__ poses,
                                                        double* __restrict__ rho0, double* __restrict__ w) {
  robust_range<KINDS>(el, el.E, poses, rho0, w);
  if (el2.cnt > 0) robust_range<KINDS>(el2, el2.cnt, poses, rho0 ? rho0 + el.E : nullptr, w ? w + el.E : nullptr);
}

}  // namespace

void launch_edge_kernel_scatter(hipStream_t s, int n, const int* ids, const double* delta, const unsigned char* kind, const EdgeListDev& el,
                                const EdgeListDev* el2, unsigned char* mark) {
  SGO_LAUNCH(k_edge_kernel_scatter, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, n, ids, delta, kind, el, el2 ? *el2 : EdgeListDev(), mark);
}
void launch_slot_kernel_refresh(hipStream_t s, int ncs, const int* eidx, const unsigned char* mark, const EdgeListDev& el,
                                const EdgeSlotsDev& es) {
  SGO_LAUNCH(k_slot_kernel_refresh, dim3(grid_for(ncs, kBlock)), dim3(kBlock), 0, s, ncs, eidx, mark, el, es);
}
void launch_edge_robust(hipStream_t s, const EdgeListDev& el, const EdgeListDev* el2, const double* poses, double* rho0, double* w) {
  const EdgeListDev l2 = el2 ? *el2 : EdgeListDev();
  const int grid = grid_for(std::max(el.E, l2.cnt), kBlock);
  if (el.kinds) SGO_LAUNCH(k_edge_robust<true>, dim3(grid), dim3(kBlock), 0, s, el, l2, poses, rho0, w);
  else SGO_LAUNCH(k_edge_robust<false>, dim3(grid), dim3(kBlock), 0, s, el, l2, poses, rho0, w);
}

void launch_edge_gate(hipStream_t s, const EdgeListDev& el, const EdgeListDev* el2, int n, const int* ids, const double* poses,
                      double chi2_max, unsigned char* flag, double* partials, int* count) {
  const int grid = grid_for(n, kBlock);
  SGO_LAUNCH(k_edge_gate, dim3(grid), dim3(kBlock), 0, s, el, el2 ? *el2 : EdgeListDev(), n, ids, poses, chi2_max, flag, partials);
  SGO_LAUNCH(k_gate_count, dim3(1), dim3(kBlock), 0, s, partials, grid, count);
}
void launch_edge_dead_flags(hipStream_t s, const EdgeListDev& el, const EdgeListDev* el2, unsigned char* dead) {
  const EdgeListDev l2 = el2 ? *el2 : EdgeListDev();
  SGO_LAUNCH(k_edge_dead_flags, dim3(grid_for(el.E + l2.cnt, kBlock)), dim3(kBlock), 0, s, el, l2, dead);
}
void launch_edge_info_scatter(hipStream_t s, int n, const int* ids, const double* rows, const EdgeListDev& el, const EdgeListDev* el2,
                              unsigned char* mark) {
  SGO_LAUNCH(k_edge_info_scatter, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, n, ids, rows, el, el2 ? *el2 : EdgeListDev(), mark);
}
void launch_slot_info_refresh(hipStream_t s, int ncs, const int* eidx, const unsigned char* mark, const EdgeListDev& el,
                              const EdgeSlotsDev& es) {
  SGO_LAUNCH(k_slot_info_refresh, dim3(grid_for(ncs, kBlock)), dim3(kBlock), 0, s, ncs, eidx, mark, el, es);
}

}  // namespace sgo
