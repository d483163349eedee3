// sgo_mfront.h -- the mid-size path: optimize(iters) through a MULTIFRONTAL sparse Cholesky factorisation spread over the
// chip, for graphs between the single-launch direct path (sgo_direct.h: <= 60 separator poses, one workgroup) and the
// multigrid PCG (whose iteration is eight or more launch-floor-bound kernels below ~10^5 rows: DESIGN.md section 7,
// "mid-size regime").  This is the regime of the reference's own largest graphs -- a few thousand keyframe poses with a
// closure every few poses (mit-killian: 5 489 poses / 7 629 edges), re-optimised after every accepted closure
// (src/sparse_gslam/src/submap_loop_closer.cpp:286-287) through g2o's sparse Cholesky (src/sparse_gslam/src/graphs.cpp:19).
//
//   * Host, once per sgo_set_graph_se2 (the counterpart of g2o's symbolic analysis): nested dissection of the free poses --
//     rows in Hilbert order of the initial positions (or in id order, whichever gives the cheaper tree), index bisection,
//     separator = a MINIMUM vertex cover of the cut (Koenig's theorem on the bipartite cut graph), leaves of <= 32 poses --,
//     the fronts' row structures, the assembly lists (every edge goes to the front of its first-eliminated endpoint) and the
//     extend-add maps, the fronts of equal height gathered into levels.
//   * Device, per Gauss-Newton iteration: two launches per LEVEL of the tree for the factorisation -- a parent's matrix is
//     gathered tile by tile from its children by many workgroups, the children's Schur complements formed on the fly on the
//     fp64 matrix cores (v_mfma_f64_16x16x4_f64: no update matrix is stored); then one workgroup per front adds the edges'
//     terms and factorises the own columns left-looking in 16-column panels, with the right-hand side as the front's last
//     ROW, so the forward substitution rides along --, one launch per level for the backward substitution, one for the edges
//     (error, Jacobians, 6x6 element and chi2), one for the update.  No atomics on floating-point data; every sum has a fixed
//     order.
// A graph qualifies when the critical path of its tree (the largest front of every level) is short enough and no front
// outgrows a workgroup's LDS panel; otherwise the caller keeps the multigrid PCG (C2's Manhattan world with four edges per
// pose has 580-row fronts and 0.24 Gflop on the critical path: not for one workgroup per front).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "sgo_direct.h"
#include "sgo_internal.h"

namespace sgo {

constexpr int kMfPanel = 16;          // panel width (= the MFMA tile)
constexpr int kMfThreads = 512;       // workgroup of the factor / solve kernels
constexpr int kMfMaxDim = 1023;       // largest front (scalar rows incl. the right-hand side row): the LDS panel is kMfMaxDim + 1 rows x 16 columns
constexpr int kMfElem = 27;           // per-edge terms: D_ii (6) D_jj (6) H_ij (9) b_i (3) b_j (3)

struct MfFront {            // one front; the fronts are numbered in post-order (children before parents)
  int e0 = 0;               // first elimination position of its own poses
  int own = 0, nb = 0;      // own poses, boundary poses
  int bnd_off = 0;          // boundary: elimination positions bnd[bnd_off .. + nb), ascending
  int kid[2] = {-1, -1};
  int map_off[2] = {0, 0};  // child k: cmap[map_off[k] + i] = local pose index (own first, then boundary) of the child's boundary pose i
  int parent = -1;
  int height = 0;
  int tgt0 = 0, tgt1 = 0;   // assembly targets
  int ld = 0;               // leading dimension of the front's matrix (column-major, rows 0 .. 3 (own + nb) incl. the right-hand side row)
  long long off = 0;        // its place in the arena (doubles)
};

struct MfTarget {           // one 3x3 block of a front that original edges contribute to
  int li, lj;               // local pose indices, li >= lj
  int c0, c1;               // contributions contrib[c0 .. c1): edge << 2 | part
};                          // part 0: D_ii + b_i (diagonal target of vertices()[0]); 1: D_jj + b_j; 2: H_ij as stored (row i, column j); 3: its transpose

struct MfPlan {
  int n = 0;
  int order_kind = 0;                 // 0: Hilbert order of the initial positions, 1: vertex id order
  std::vector<int> elim_vertex;       // [n] elimination position -> vertex id
  std::vector<MfFront> fronts;
  std::vector<int> bnd, cmap;
  std::vector<MfTarget> targets;
  std::vector<int> contrib;
  std::vector<int> level_ptr, level_front;   // fronts of height h: level_front[level_ptr[h] .. level_ptr[h + 1]), largest first
  // figures of merit
  int height = 0, max_dim = 0, max_own = 0, max_bnd = 0;
  double flops = 0.0, crit_flops = 0.0;      // multiply-adds x 2 of the partial factorisations: all fronts / the largest front of every level
  int crit_panels = 0;                       // 16-column panels on the critical path
  long long arena_doubles = 0;
};

struct MfLimits {
  int max_rows = 65536;
  int leaf = 32;
  double max_crit_flops = 80e6;
  long long max_arena_bytes = (long long)1 << 30;
  double max_degree = 2.5;           // edges between free poses per free pose: above it the graph is refused unanalysed
  int both_orders_rows = 8192;       // up to this size both row orders are analysed, above it only the Hilbert order
  int only_kind = -1;                // >= 0: analyse this row order alone (the caller knows which one wins on this graph's kind)
};

// Host analysis.  false with *why set: the graph does not qualify.
bool mfront_analyze(int V, int n, const int* free_id, const double* poses, int E, const int* ei, const int* ej, const MfLimits& lim,
                    MfPlan* plan, std::string* why);

// The front table in plain columns (sgo_debug_mfront_array / sgo_mfront_plan_array, SGO_MF_FRONTS of include/sgo.h):
// e0, own3, m, ld, off, nb, bnd_off, kid[0], kid[1], pinv_off[0], pinv_off[1], tgt0, tgt1, parent
constexpr int kMfFrontCols = 14;
void mfront_tables(const MfPlan& plan, std::vector<long long>* fronts, std::vector<int>* pinv);
// The limits sgo_set_graph_se2 analyses with: the defaults and the environment's SGO_MFRONT_LEAF / _CRIT_MFLOP / _DEGREE.
void mfront_env_limits(MfLimits* lim);
// One array of a host plan by its SGO_MF_* number (the plan's share: INFO .. ELIM_VERTEX): bytes, copied when cap_bytes holds
// them; SGO_EINVAL for any other array.
long long mfront_plan_array(const MfPlan& plan, int E, int what, void* out, long long cap_bytes);

struct Mfront;   // opaque: plan + device arrays

struct MfrontInfo {
  int n = 0, fronts = 0, height = 0, max_dim = 0, max_own = 0, max_bnd = 0, order_kind = 0, crit_panels = 0;
  double flops = 0.0, crit_flops = 0.0;
  size_t arena_bytes = 0;
};

// nullptr with *why set: the graph does not qualify; nullptr with *err set: HIP failure.
// Device arrays come out of `arena` (the context's per-graph arena: rewound, not freed, by the next set-up -- the reference
// re-initialises after every closure).  *order_hint (in / out, -1: none): the row order the previous graph of this context
// chose; when the new graph has about as many poses that order is analysed alone.
Mfront* mfront_create(hipStream_t s, DevArena* arena, int V, int n, const int* free_id, const double* poses, int E, const int* ei,
                      const int* ej, int max_rows, int* order_hint, std::string* why, std::string* err);
void mfront_destroy(Mfront* m);
const MfrontInfo& mfront_info(const Mfront* m);
// iters x { edges + chi2, factorise (levels up), substitute (levels down), update } + the closing chi2 on the stream; outputs
// as direct_optimize (d_hist[2 (iters + 1)], DirectResult: done / fail / fail_iter / stamps).  until != nullptr
// (sgo_optimize_gn_until): one more single-wave launch per iteration from the third on applies rules::gain_stop with *until on the
// device; after a stop the call's remaining launches return at once, and the arena, x, invd, yinv and the flags are those of the
// plain call of as many iterations (the elements: those at the final poses).
hipError_t mfront_optimize(Mfront* m, hipStream_t s, const EdgeListDev& el, double* d_poses, int iters, double* d_hist,
                           DirectResult* d_res, const double* until = nullptr);
double mfront_bytes(const Mfront* m, int E, int iters);
// sgo_optimize_gn_hypotheses on this path when the caller has granted the memory (sgo_set_hypotheses_workspace): L.B hypotheses of
// the resident graph as ONE chain of launches -- mfront_optimize's in until-mode, every grid x L.B, the kernels' batched
// instantiations (always with the gain rule; gain_tol <= 0 never stops).  Hypothesis b works on copy b of everything mfront_optimize
// writes -- elem, x, invd, yinv, the partial sums, the flags, the arena, its information rows, poses, history and DirectResult --
// in one workspace of the caller's laid out by mfront_batch_layout (offsets in bytes, strides in doubles from one hypothesis to the
// next; bytes = B x per_hypothesis whatever B is); the plan's tables are shared and the resident image is not written.  It obeys
// its own flags word: after a failure or a stop its workgroups return at once, no host read inside the chain.  The caller puts
// the masks [B][E] at o_off and, with own_poses, the starting poses [B][V][3] at o_poses before the call; after it, it reads hist
// [B][iters + 1][2] at o_hist, {updates applied, DirectResult::fail} [B] at o_brief, the poses at o_poses and, if asked for (in the
// layout too), e^T Omega e with the resident rows [B][E] at o_echi2.  The arithmetic, the grids in x and the order of every sum are
// mfront_optimize's: hypothesis b is bit for bit that call on the graph with its rows zeroed.
struct MfBatchLayout {
  int B = 0, V = 0, E = 0;
  size_t hist_stride = 0;
  size_t s_elem = 0, s_x = 0, s_yinv = 0, s_arena = 0, s_info = 0, s_poses = 0;
  size_t o_off = 0, o_info = 0, o_poses = 0, o_hist = 0, o_echi2 = 0, o_brief = 0, o_res = 0, o_elem = 0, o_x = 0, o_invd = 0, o_yinv = 0,
         o_partials = 0, o_flags = 0, o_arena = 0;
  size_t per_hypothesis = 0, bytes = 0;
};
MfBatchLayout mfront_batch_layout(const Mfront* m, int V, int B, int iters, bool want_edge_chi2);
hipError_t mfront_optimize_batch(Mfront* m, hipStream_t s, const EdgeListDev& el, const double* d_poses_res, bool own_poses,
                                 const MfBatchLayout& L, char* ws, int iters, double gain_tol, bool want_edge_chi2);
// The factor phase of one iteration alone, at the current poses: edges (elements, chi2 partials), then merge and panels per level --
// mfront_optimize's own launches up to and excluding the substitution and the update.  Clears the failure flags first; x is untouched.
hipError_t mfront_factorize(Mfront* m, hipStream_t s, const EdgeListDev& el, const double* d_poses, double* d_hist, DirectResult* d_res);
// sgo_optimize_lm's two shares of one attempt (sgo_lm.h): k_mf_edges at the accepted poses (elements; d_hist / d_res: scratch), and
// merge, panels and substitution per level for (H + lambda I) x = b with lambda read from *st on the device.  Both obey the flags
// word and neither clears it.
struct LmState;
struct DlState;   // (sgo_dogleg.h: the state of sgo_optimize_dogleg, which solves through the same two shares)
void mfront_lm_edges(Mfront* m, hipStream_t s, const EdgeListDev& el, const double* d_poses, double* d_hist, DirectResult* d_res);
void mfront_lm_solve(Mfront* m, hipStream_t s, const LmState* st, double* d_hist, DirectResult* d_res);
// Test hook (sgo_debug_mfront_array): one resident array as stored after the last mfront_optimize or selected inversion;
// SGO_ENOTHING before the first (SGO_MF_SEL: 0 bytes before the first selected inversion; SGO_MF_FS_Y / _X: before the first
// multi-right-hand-side substitution).
long long mfront_debug_array(const Mfront* m, hipStream_t s, int what, void* out, long long cap_bytes);

}  // namespace sgo
