// sgo_direct.h -- the small-graph path: optimize(iters) of a pose graph of the size the reference itself
// produces (intel-lab: ~1k poses and a few tens of closures, slc.cpp:205-288) as ONE kernel launch of one
// workgroup -- linearisation, a sparse block LDL^T in nested-dissection order, the update and chi2 of every
// Gauss-Newton iteration -- instead of ~150 launches per iteration of the multigrid PCG, whose fixed costs
// (a dense coarsest inverse, 8 launches per PCG iteration) dominate at this size.
#pragma once
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "sgo_internal.h"

namespace sgo {

struct Direct;   // opaque: elimination plan + device arrays

struct DirectInfo {
  int n = 0;         // free poses
  int n_chain = 0;   // ... eliminated level by level (cyclic reduction of the trajectory's chain segments)
  int n_sep = 0;     // ... separators (a vertex cover of the non-chain edges), factorised as one dense block in LDS
  int levels = 0;    // sparse elimination levels (height of the elimination tree below the separators)
  int slots = 0;     // stored off-diagonal blocks of the sparse columns (incl. fill and padding)
  int contributions = 0;   // Schur-complement block products per factorisation
  size_t lds_bytes = 0;
};

// Result of one direct_optimize call (pinned host memory, filled by the kernel).
struct DirectResult {
  int done;          // Gauss-Newton updates applied
  int fail;          // 0 ok; 1 a pivot block was not positive definite; 2 non-finite update
  int fail_iter;
  int pad;
  unsigned long long cycles;     // shader clock cycles (s_memtime) between the first and the last stamp
  unsigned long long phase[8];   // wall_clock64 of the LAST iteration: start, edges done, assembled, sparse forward done,
                                 // separators eliminated, separators solved, sparse backward done, poses updated
  unsigned long long stamp[2 * SGO_MAX_ITERS + 4];   // wall_clock64 (100 MHz) at the start of iteration k [2k] and
                                                     // after its assembly [2k + 1]; the closing chi2 pass starts at
                                                     // [2 iters] and ends at [2 iters + 1]; after a failure in
                                                     // iteration k the call ends at [2k + 2]
};

// Host analysis, then the upload of what it made.  nullptr with *why set: the graph does not qualify (too many separators / levels /
// rows; the caller uses the multigrid path); nullptr with *err set: HIP failure.
Direct* direct_create(hipStream_t s, DevArena* arena, int V, int n, const int* free_id, int E, const int* ei, const int* ej,
                      int max_rows, std::string* why, std::string* err);
void direct_destroy(Direct* d);
const DirectInfo& direct_info(const Direct* d);

// iters x { chi2, linearise, factorise, solve, update } + the final chi2 on the stream; d_hist[2 (iters + 1)] gets
// (chi2, robust chi2) at the start of every iteration and at the end; d_res is a device DirectResult.
// until != nullptr (sgo_optimize_gn_until): the kernel ends the call before the first iteration at which rules::gain_stop holds for
// *until and leaves d_res, the history and the poses as a call of that many iterations does.
hipError_t direct_optimize(Direct* d, hipStream_t s, const EdgeListDev& el, double* d_poses, int iters, double* d_hist,
                           DirectResult* d_res, const double* until = nullptr);
// sgo_optimize_gn_hypotheses on this path: B hypotheses of the resident graph as ONE launch of B workgroups of the batched
// instantiation of the same kernel (always with the gain rule; gain_tol <= 0 never stops).  Workgroup b works on copy b of everything
// the kernel writes; the copies live in one workspace of the caller's, laid out by direct_batch_layout (offsets in bytes, strides
// in doubles from one hypothesis to the next).  The caller puts the masks [B][E] at o_off and, with own_poses, the starting poses
// [B][V][3] at o_poses before the call; after it, it reads hist [B][iters + 1][2] at o_hist, {updates applied, DirectResult::fail}
// [B] at o_brief, the poses at o_poses and, if asked for, e^T Omega e with the resident rows [B][E] at o_echi2.
struct DirectBatchLayout {
  int B = 0, V = 0, E = 0;
  size_t hist_stride = 0;
  size_t s_Wd = 0, s_Wo = 0, s_escr = 0, s_zsc = 0, s_xbg = 0, s_info = 0, s_poses = 0;
  size_t o_off = 0, o_info = 0, o_poses = 0, o_hist = 0, o_echi2 = 0, o_brief = 0, o_res = 0, o_Wd = 0, o_Wo = 0, o_escr = 0, o_zsc = 0, o_xbg = 0;
  size_t bytes = 0;
};
DirectBatchLayout direct_batch_layout(const Direct* d, int V, int B, int iters);
hipError_t direct_optimize_batch(Direct* d, hipStream_t s, const EdgeListDev& el, const double* d_poses_res, bool own_poses,
                                 const DirectBatchLayout& L, char* ws, int iters, double gain_tol, bool want_edge_chi2);
// sgo_optimize_gn_many on this path: n DIFFERENT graphs, one workgroup each, in one launch of the MANY instantiation of the same
// kernel per group of graphs that share its compile-time flags (the vector in global memory or in LDS, kernel kinds or DCS alone:
// at most four groups, one for the usual homogeneous call; a group of more than kDirectManyGrid graphs takes further launches).
// Workgroup b reads everything -- plan, edge list, outputs, iters, gain_tol -- from record b of a job table in device memory.
//   direct_many_table     fills the caller's host table [n][kDirectJobBytes] (pinned: the caller uploads it in ONE copy), the
//                         records of a group next to each other, and lists the launches; item i writes to ITS d_hist
//                         [2 (iters + 1)] and d_res whatever its place in the table.  Marks every item's Direct as run.
//   direct_optimize_many  one of those launches, on the table's device copy (so that the caller can bracket each launch).
// direct_joins_many: false for a Direct whose debug dump is on (SGO_DIRECT_DEBUG): it keeps its own launch.
constexpr size_t kDirectJobBytes = 288;
constexpr int kDirectManyGrid = 65535;
struct DirectManyItem {
  Direct* d;
  const EdgeListDev* el;
  double* d_poses;
  double* d_hist;
  DirectResult* d_res;
};
struct DirectManyTable {
  struct Launch {
    int group, first, count;   // xb_global | kinds << 1; records [first, first + count) of the table
    size_t lds_bytes;          // the largest of its jobs
    double bytes;              // algorithmic bytes, summed (profile table)
  };
  std::vector<Launch> launches;
};
bool direct_joins_many(const Direct* d);
void direct_many_table(int n, const DirectManyItem* items, int iters, double gain_tol, char* h_jobs, DirectManyTable* T);
hipError_t direct_optimize_many(hipStream_t s, const DirectManyTable::Launch& L, const char* d_jobs);
// What a batched launch of either factorisation path (this one, sgo_mfront.h) needs before it starts, one launch of k_hyp_prepare:
// hypothesis b's information rows at info_b + b info_stride ([6][E]: 0 where off[b][E] is set, info_res elsewhere) and, with
// poses_res != nullptr (the caller gave no starting poses), its copy of the resident poses at poses_b + b poses_stride.
void launch_hyp_prepare(hipStream_t s, int B, int E, int V, const double* info_res, const unsigned char* off, double* info_b, size_t info_stride,
                        const double* poses_res, double* poses_b, size_t poses_stride);
// Test hooks (include/sgo.h, SGO_DR_*; size-query convention of the other hooks).  direct_plan_array: one table of the host
// analysis alone -- no stream, no arena; SGO_ENOTHING with *why set when the graph does not qualify.  direct_debug_array: the
// same tables read back from the device and what the last direct_optimize left; SGO_ENOTHING before the first with iters > 0.
long long direct_plan_array(int V, int n, const int* free_id, int E, const int* ei, const int* ej, int max_rows, int what, void* out,
                            long long cap_bytes, std::string* why);
long long direct_debug_array(const Direct* d, hipStream_t s, int what, void* out, long long cap_bytes);
// algorithmic bytes of one call (profile table)
double direct_bytes(const Direct* d, int E, int iters);

}  // namespace sgo
