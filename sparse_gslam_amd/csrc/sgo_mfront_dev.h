// sgo_mfront_dev.h -- what the multifrontal path's two device sources share: the device image of the plan and the resident
// factorisation (sgo_mfront.hip makes and fills it; sgo_selinv.hip reads the factor for the selected inversion, sgo_fsolve.hip for
// the multi-right-hand-side substitution) and the opaque Mfront behind sgo_mfront.h.  Not for the host-only sources.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "sgo_mfront.h"

struct sgo_ctx;

namespace sgo {

constexpr int kMfNW = kMfThreads / 64;
constexpr int kElemStride = 28;   // kMfElem padded to 16-byte multiples

struct MfFrontDev {
  int e0, own3, m, ld;
  long long off;
  int nb, bnd_off;
  int kid[2];
  int pinv_off[2];   // child k: pinv[pinv_off[k] + local pose] = its index among the child's boundary poses, -1: not there
  int tgt0, tgt1;
  int parent;
};

struct MfDev {
  int n = 0, E = 0, nfront = 0;
  const MfFrontDev* fronts = nullptr;
  const int* level_front = nullptr;
  const int* bnd = nullptr;
  const int* pinv = nullptr;
  const int2* mtile = nullptr;   // k_mf_merge's work list: (front, tile row | tile column << 16), level by level
  const MfTarget* targets = nullptr;
  const int* contrib = nullptr;
  const int* elim_vertex = nullptr;
  double* arena = nullptr;
  double* elem = nullptr;      // [E][kElemStride]
  double* x = nullptr;         // [3 n] by elimination position
  double* invd = nullptr;      // [3 n] 1 / L[c][c] of every eliminated scalar row (k_mf_panels), for the substitution
  double* yinv = nullptr;      // [3 n][16] row i of the inverse of its 16 x 16 diagonal block's factor (zeros right of the diagonal)
  double* partials = nullptr;  // [2][kMaxPartials]
  long long* dbg = nullptr;    // diagnostic runs (SGO_MFRONT_DEBUG): [nfront][8] s_memtime cycles of the factor kernel's phases
  int* flags = nullptr;        // [0] fail (1 not positive definite, 2 non-finite update)  [1] iteration of the failure
                               // [2] a back-substitution produced a non-finite value  [3] updates applied
};

typedef double mf_d4 __attribute__((ext_vector_type(4)));

// The batched instantiations of sgo_mfront.hip's kernels (mfront_optimize_batch): blockIdx.y is the hypothesis, which works on copy
// blockIdx.y of everything mfront_optimize writes -- the strides, in doubles, from one copy to the next -- while the plan's tables
// stay shared.  The partial sums stride by 2 kMaxPartials doubles, the flags by 8 ints, the DirectResult by one.
struct MfBatch {
  size_t elem, x, yinv, arena;   // MfDev's arrays (invd strides like x)
  size_t info, poses, hist;      // the information rows [6][E], the poses [V][3], the history [iters + 1][2]
  int2* brief;                   // [B] {updates applied, failure code}: what the host reads of a hypothesis' DirectResult
};
struct MfSingle {};              // the unbatched instantiations take nothing

// Hypothesis blockIdx.y's view of a batched kernel's arguments; el / poses / hist / res: those the kernel has (nullptr: not one of its).
template <class P = double*, class H = double*, class R = DirectResult*>
__device__ __forceinline__ void mf_slice(const MfBatch& bt, MfDev& M, EdgeListDev* el = nullptr, P* poses = nullptr, H* hist = nullptr,
                                         R* res = nullptr) {
  const size_t b = blockIdx.y;
  M.elem += b * bt.elem;
  M.x += b * bt.x;
  M.invd += b * bt.x;
  M.yinv += b * bt.yinv;
  M.arena += b * bt.arena;
  M.partials += b * (2 * (size_t)kMaxPartials);
  M.flags += b * 8;
  if (el) el->info += b * bt.info;
  if (poses) *poses += b * bt.poses;
  if (hist) *hist += b * bt.hist;
  if (res) *res += b;
}

// The selected inversion's share of the device image (sgo_selinv.hip, sgo_selinv.cpp): made by the first sgo_marginals_selected
// on the graph, out of the same per-graph arena.
struct MfSelDev {
  double* S = nullptr;            // the second arena: front f's selected inverse at fronts[f].off, the front's own layout
  const int* cmap = nullptr;      // the plan's extend-add maps: child boundary pose -> local pose of the parent
  const int* cmap_off = nullptr;  // [nfront] where front f's map starts (a root: 0, unused)
  const int2* gtile = nullptr;    // k_si_gather's work list: (front, tile row | tile column << 16) of the boundary block, level by level
  const int* pos_front = nullptr; // [n] elimination position -> the front that owns it
};

// Where the selected inverse holds a resident edge's three blocks (sgo_edge_leave_one_out; made on the host once per plan):
// pair = sgo_marginals_selected's descriptor of the block (vertices()[0], vertices()[1]) -- (front, local row pose, local column
// pose, transposed); front < 0: an endpoint is fixed, no block --, pi / pj = the endpoints' elimination positions (-1: fixed), whose
// diagonal blocks sit in the fronts that own them (MfSelDev::pos_front).  Duplicate edges of a pair, in either orientation, name the
// same stored block and differ in `transposed` alone.
struct LooEdgeDev {
  int4 pair;
  int pi, pj;
};
constexpr int kLooOut = 12;       // per listed edge: d2, redundancy, cov_loo (9, row-major), fail

// The multi-right-hand-side substitution's share (sgo_fsolve.hip, sgo_fsolve.cpp): made by the first sgo_factor_solve /
// sgo_candidate_gate on the graph, out of the same per-graph arena.
struct MfFsDev {
  const int* uoff = nullptr;      // [nfront] first row of front f's boundary rows in a panel's update buffer [U3][16]
  const int* pos_h = nullptr;     // [n] elimination position -> hessian index
  int U3 = 0;                     // boundary scalar rows of all fronts
};
// The candidates of one sgo_candidate_gate call on the device (n: their number = the component stride of zinv / info)
constexpr int kFsRec = 13;        // per-candidate record: e (3), A00 A01 A02 A10 A11 A12, B00 B01 B10 B11
constexpr int kFsOut = 11;        // per-candidate result: d2, P (9), the decision
constexpr int kFsChunkPanels = 16;   // panels of 16 columns per pass over the factor (bounds the scratch: 2 x 256 x 3 n doubles + updates)
struct FsCandDev {
  int n = 0;
  const int* vi = nullptr;
  const int* vj = nullptr;
  const int* row = nullptr;       // [n][2] the pose's place in a right-hand side (elimination position; hessian index on the PCG route), -1: fixed
  const double* zinv = nullptr;   // [3][n]
  const double* info = nullptr;   // [6][n]
  double* rec = nullptr;          // [n][kFsRec]
};

// Q = [A_s B_s] W[rows of i_s, j_s] (3 x 3): candidate s' record against three columns `col` of W = H^-1 R (column b at col + b n3;
// rows[0], rows[1]: the rows of its poses, -1 for a fixed endpoint, which drops out).  The one statement of this arithmetic: k_fs_gate takes a
// candidate's own columns, k_fs_gram every other candidate's.
__device__ __forceinline__ void fs_candidate_q(const double* rec, const int* rows, const double* col, int n3, double (&Q)[3][3]) {
  const double A[3][3] = {{rec[3], rec[4], rec[5]}, {rec[6], rec[7], rec[8]}, {0.0, 0.0, -1.0}};
  const double B[3][3] = {{rec[9], rec[10], 0.0}, {rec[11], rec[12], 0.0}, {0.0, 0.0, 1.0}};
  const int ri = rows[0], rj = rows[1];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    double wi[3] = {0.0, 0.0, 0.0}, wj[3] = {0.0, 0.0, 0.0};
    if (ri >= 0)
#pragma unroll
      for (int r = 0; r < 3; ++r) wi[r] = col[(size_t)b * n3 + 3 * (size_t)ri + r];
    if (rj >= 0)
#pragma unroll
      for (int r = 0; r < 3; ++r) wj[r] = col[(size_t)b * n3 + 3 * (size_t)rj + r];
#pragma unroll
    for (int a = 0; a < 3; ++a)
      Q[a][b] = ((A[a][0] * wi[0] + A[a][1] * wi[1]) + A[a][2] * wi[2]) + ((B[a][0] * wj[0] + B[a][1] * wj[1]) + B[a][2] * wj[2]);
  }
}

// sgo_optimize_lm's share (sgo_lm.hip, sgo_lm.cpp): the free poses' diagonal targets, made by the first call on the plan out of the
// same per-graph arena -- elimination position p's targets tgt[ptr[p] .. ptr[p + 1]), ascending: the fronts in post-order, which is
// k_mf_panels' contribution order.
struct LmDiagDev {
  const int* ptr = nullptr;   // [n + 1]
  const int* tgt = nullptr;
};
// a pose's diagonal terms of the elements: the six entries of D and the three of b of every contribution to target t, added to acc
// (k_lm_lambda0, k_lm_trial; k_dl_vectors of sgo_dogleg.hip)
__device__ __forceinline__ void lm_target_terms(const MfDev& M, int t, double (&acc)[9]) {
  const MfTarget T = M.targets[t];
  for (int c = T.c0; c < T.c1; ++c) {
    const int w = M.contrib[c];
    const double* el = M.elem + (size_t)kElemStride * (w >> 2);
    const int side = w & 1;
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[q] += el[6 * side + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[6 + q] += el[21 + 3 * side + q];
  }
}

// The joint table of sgo_candidate_joint (sgo_fsolve.hip): S [3 n][3 n] row-major, then e [n][3], then one double: the
// factorisation's failure flag
constexpr int kJointThreads = 256;   // k_joint_subsets' workgroup: 16 x 16 over a trailing block; one thread per candidate of a mask
inline size_t joint_table_doubles(int n) { return 9 * (size_t)n * n + 3 * (size_t)n + 1; }

struct Mfront {
  MfPlan plan;
  MfrontInfo info;
  MfDev dev;
  void* buf = nullptr;
  std::vector<int> level_lds;        // dynamic LDS of the panel launch of every level
  std::vector<int> level_solve_lds;  // ... of the substitution launch
  std::vector<int> mtile_ptr;        // k_mf_merge's tiles of level h: [mtile_ptr[h], mtile_ptr[h + 1])
  size_t n_pinv = 0;                 // entries of dev.pinv
  bool ran = false;                  // an mfront_optimize with iters > 0 has filled elem, the arena, x, invd and yinv
  // selected inversion
  MfSelDev sel;
  bool sel_ready = false;            // sel's arrays exist
  bool sel_ran = false;              // a selected inversion has filled sel.S (and mfront_factorize the factor's arrays)
  std::vector<int> gtile_ptr;        // k_si_gather's tiles of level h: [gtile_ptr[h], gtile_ptr[h + 1])
  std::vector<int> pos_front;        // host copy of sel.pos_front
  // leave-one-out test of the resident edges (sgo_loo.cpp): where sel.S holds every edge's blocks, once per plan
  const LooEdgeDev* loo = nullptr;   // [loo_E]
  int loo_E = -1;                    // the edges the descriptors were made for (-1: none yet)
  // multi-right-hand-side substitution
  MfFsDev fs;
  bool fs_ready = false;             // fs's arrays and sel.cmap / sel.cmap_off exist
  const double *fs_Y = nullptr, *fs_X = nullptr;   // the last call's last chunk after the forward / backward pass (the context's scratch)
  int fs_cols = 0;                   // its columns (0: no call yet)
  // Levenberg-Marquardt
  LmDiagDev lm_diag;                 // (ptr == nullptr: not made yet)
};

// ---- kernels of the selected inversion (sgo_selinv.hip), one launch each; the host driver is sgo_selinv.cpp ----
void launch_si_gather(hipStream_t s, const MfDev& M, const MfSelDev& Z, int t0, int t1);
void launch_si_panels(hipStream_t s, const MfDev& M, const MfSelDev& Z, int lvl0, int count, size_t lds);
// out: [V][9] diagonal blocks by vertex id, then [npairs][9], then one double: the factorisation's failure flag.  pairs[t] =
// (front, local row pose, local column pose, transpose), front < 0: the zero block.  The caller has zeroed out.
void launch_si_result(hipStream_t s, const MfDev& M, const MfSelDev& Z, int V, int npairs, const int4* pairs, double* out);
bool si_prepare_device();   // the panel kernel's dynamic LDS; false: the device does not grant it


// ---- what the calls that work through the factor share (sgo_selinv.cpp) ----
// The plan: the resident one, or one analysed for these calls (once per set-up; a refusal is cached too: SGO_ENOTHING, the reason
// in the context's error text, which names `who` and points to `instead`).
int selinv_plan(sgo_ctx* c, Mfront** out, const char* who, const char* instead);
int mfront_maps_prepare(sgo_ctx* c, Mfront* m);   // sel.cmap / sel.cmap_off on the device, once per plan
// The two phases sgo_marginals_selected and sgo_edge_leave_one_out share: selinv_prepare makes the selected inversion's own device
// arrays (once per plan; `who` for the error text), selinv_run queues the factor phase at the current poses and the top-down
// selected inversion, after which sel.S holds every front's selected inverse (dev.flags[0] != 0: the factorisation failed and the
// later launches did nothing).  selinv_positions: hessian index -> elimination position; selinv_pair: sgo_marginals_selected's
// descriptor of the block with the rows of position pi and the columns of pj, false when no front holds both.
int selinv_prepare(sgo_ctx* c, Mfront* m, const char* who);
int selinv_run(sgo_ctx* c, Mfront* m);
std::vector<int> selinv_positions(const sgo_ctx* c, const Mfront* m);
bool selinv_pair(const Mfront* m, int pi, int pj, int4* out);

// ---- the leave-one-out kernel (sgo_loo.hip); the host driver is sgo_loo.cpp ----
// out: [n][kLooOut], then the factorisation's failure flag, then the count of failing edges; partials: [kMaxPartials].  ids ==
// nullptr: edges 0 .. n-1.  desc == nullptr: a graph without a free pose (every P is zero; M, Z and flags are not read).
void launch_loo_edges(hipStream_t s, const MfDev& M, const MfSelDev& Z, const LooEdgeDev* desc, const EdgeListDev& el, const double* poses, int n,
                      const int* ids, double chi2_max, double min_redundancy, double* out, double* partials);

// ---- kernels of the multi-right-hand-side substitution (sgo_fsolve.hip), one launch each; the host driver is sgo_fsolve.cpp ----
void launch_fs_rhs_columns(hipStream_t s, int ncols, int n3, const double* src, const int* pos_h, double* panel);
void launch_fs_rhs_candidates(hipStream_t s, const FsCandDev& C, int t0, int t1, const double* poses, int n3, double* panel);   // panel: zeroed
void launch_fs_records(hipStream_t s, const FsCandDev& C, const double* poses);   // every candidate's record, no panel
void launch_fs_forward(hipStream_t s, const MfDev& M, const MfSelDev& Z, const MfFsDev& Fs, int lvl0, int count, int panels, size_t lds, double* Y,
                       double* U, int n3);
void launch_fs_backward(hipStream_t s, const MfDev& M, int lvl0, int count, int panels, size_t lds, const double* Y, double* X, int n3);
void launch_fs_gate(hipStream_t s, const FsCandDev& C, int t0, int t1, const double* W, int n3, double chi2_max, const int* flags, double* out);
bool fs_prepare_device();   // the two substitution kernels' dynamic LDS
// What the calls that substitute through the factor share (sgo_fsolve.cpp): fs_prepare makes the substitution's own device arrays
// (once per plan); fs_scratch hands out one chunk's scratch for `panels` panels -- the panel after the forward pass (it holds the
// right-hand sides before), after the backward pass, and the fronts' update buffers --; fs_passes queues both passes over the factor
// for the panels whose right-hand sides sit in S.Y (ncols of their columns are in use), after which S.X holds H^-1 of them.
struct FsScratch {
  double *Y = nullptr, *X = nullptr, *U = nullptr;
};
int fs_prepare(sgo_ctx* c, Mfront* m, const char* who);
int fs_scratch(sgo_ctx* c, int n3, int U3, int panels, FsScratch* S);
void fs_passes(sgo_ctx* c, Mfront* m, const FsScratch& S, int panels, int ncols);

// ---- the closure search's kernels (sgo_search.hip); the host driver is sgo_search.cpp ----
constexpr int kCsOut = 13;   // per pair: m2, rel (3), cov_rel's upper triangle by rows (6), sigma (2), near
constexpr int kCsChunkQueries = kFsChunkPanels * kMfPanel / 3;   // queries per pass over the factor: three columns each, packed
// A chunk's queries on the device: (vertex id, elimination position or -1 for a fixed pose, the first of its three columns in
// the chunk's panel or -1 for a fixed pose, unused)
typedef int4 CsQueryDev;
// panel (zeroed) <- the unit columns of the chunk's free queries at their elimination positions
void launch_cs_unit(hipStream_t s, int cq, const CsQueryDev* queries, int n3, double* panel);
// out: [kCsOut][cq][n] (field, query, listed vertex), then the factorisation's failure flag, then the count of near pairs;
// partials: [kMaxPartials].  vpos[v]: vertex v's elimination position, -1 for a fixed active vertex, -2 for one without an edge.
// ids == nullptr: vertices 0 .. n-1.  factor == false: a graph without a free pose (M, Z and X are not read).  X: the chunk's
// columns H^-1 E after fs_passes (column k at X + k n3, rows by elimination position).
void launch_closure_search(hipStream_t s, const MfDev& M, const MfSelDev& Z, bool factor, const int* vpos, const double* poses, int n, const int* ids,
                           int cq, const CsQueryDev* queries, const double* X, int n3, double radius, double chi2_max, int min_sep, double* out,
                           double* partials);

// ---- the joint table of a candidate set and its subsets (sgo_candidate_joint / sgo_joint_subsets / sgo_joint_pairs) ----
// G[3 s + a][3 t + b] = Q_st[a][b] for every candidate s of C and the candidates t of [t0, t1), whose columns are W
void launch_fs_gram(hipStream_t s, const FsCandDev& C, int t0, int t1, const double* W, int n3, double* G);
// table = S (symmetrised G + blockdiag(Omega^-1)), e, the failure flag (flags == nullptr: 0)
void launch_fs_joint_table(hipStream_t s, const FsCandDev& C, const double* G, const int* flags, double* table);
// d2 of `count` subsets of the table of n candidates, one workgroup each: mask rows [count][n], or (mask == nullptr) the one- and
// two-element subsets number b0 .. b0 + count of the pairs' triangle, written to both places of d2 [n][n].  rows_cap: the scalar
// rows the dynamic LDS holds.
void launch_joint_subsets(hipStream_t s, const double* table, int n, const uint8_t* mask, int b0, int count, int rows_cap, double* d2);
bool joint_prepare_device();   // the subset kernel's dynamic LDS
inline size_t joint_lds_bytes(int rows) { return sizeof(double) * (size_t)(rows + 1) * (size_t)(rows | 1) + sizeof(double) * (size_t)std::max(rows, 1); }
// what sgo_joint_subsets, sgo_joint_pairs and the search's calls refuse alike: no resident table, n not the table's (sgo_fsolve.cpp)
int joint_table_check(sgo_ctx* c, const char* name, int32_t n);

// ---- the greedy search on the joint table (sgo_joint_greedy / sgo_joint_extend; kernel in sgo_jsearch.hip, driver in sgo_jsearch.cpp) ----
// One workgroup per seed of a slice, each with its own slab of W [3 max_len][3 n].  A slice holds at most kJointGrowSlabs slabs (one
// per compute unit) and at most kJointGrowScratchBytes of them: 256 slabs at the caps are 256 x 3 x 40 x 3 x 256 x 8 = 180 MiB.
constexpr int kJointGrowSlabs = 256;
constexpr size_t kJointGrowScratchBytes = (size_t)192 << 20;
inline size_t joint_grow_slab_doubles(int n, int max_len) { return std::max<size_t>(9 * (size_t)max_len * (size_t)n, 1); }
inline int joint_grow_slice(int n, int max_len, int B) {
  const size_t fit = kJointGrowScratchBytes / (sizeof(double) * joint_grow_slab_doubles(n, max_len));
  return (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(fit, kJointGrowSlabs), (size_t)std::max(B, 1)));
}
struct JointGrowDev {
  const double* table = nullptr;   // S, e, the flag (joint_table_doubles)
  int n = 0, max_len = 0, b0 = 0;  // candidates; pivots at most; the slice's first seed
  const int* seed = nullptr;       // [B][SGO_JOINT_MAX_SUBSET], -1 padded
  const uint8_t* allow = nullptr;  // [B][n] or nullptr: all
  const double* chi2 = nullptr;    // [SGO_JOINT_MAX_SUBSET + 1] by count, or nullptr: no growth
  double* slabs = nullptr;         // [slice][slab]
  size_t slab = 0;                 // doubles per slab
  int *order = nullptr, *count = nullptr, *stop = nullptr;   // [B][SGO_JOINT_MAX_SUBSET], [B], [B]
  double *d2_path = nullptr, *d2_ext = nullptr;              // [B][SGO_JOINT_MAX_SUBSET + 1], [B][n]
};
void launch_joint_grow(hipStream_t s, const JointGrowDev& A, int count);   // seeds A.b0 .. A.b0 + count, count <= the slice

// ---- the resident-edge table and its groups (sgo_edge_joint / sgo_edge_groups; kernels in sgo_egroup.hip, drivers in sgo_fsolve.cpp
// and sgo_egroup.cpp) ----
// The table: N [3 n][3 n] row-major, e [n][3], w [n], Omega's upper triangle [n][6], then one double: the factorisation's failure flag
inline size_t edge_table_doubles(int n) { return 9 * (size_t)n * n + 10 * (size_t)n + 1; }
constexpr int kEgOut = 4;   // per-group result: d2, pivot, dof, the decision
// The listed resident edges as candidates' records, filled on the device: endpoints, rows (vrow[v]: vertex v's place in a
// right-hand side, -1 for a fixed one), inverse measurement and information in C's arrays (stride C.n), the kernel weights in w
void launch_edge_cands(hipStream_t s, const FsCandDev& C, const EdgeListDev& el, const int* ids, const int* vrow, const double* poses, int* vi, int* vj,
                       int* row, double* zinv, double* info, double* w);
// table = N (G symmetrised, one triangle computed and mirrored), e, w, Omega, the failure flag (flags == nullptr: 0)
void launch_edge_table(hipStream_t s, const FsCandDev& C, const double* w, const double* G, const int* flags, double* table);
// `count` groups of the table of n edges, one workgroup each: member rows mask [count][n]; out [count][kEgOut].  kmax: the members
// the dynamic LDS holds.
void launch_edge_groups(hipStream_t s, const double* table, int n, const uint8_t* mask, const double* chi2_max, double min_pivot, int count, int kmax,
                        double* out);
bool edge_groups_prepare_device();   // the group kernel's dynamic LDS

}  // namespace sgo
