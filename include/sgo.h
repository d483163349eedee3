/* sgo.h -- C-ABI of the MI355X-native SE(2) pose-graph optimiser (libsgo.so).
 *
 * This is the drop-in boundary under sparse-gslam's g2o call sites.  The reference drives a
 * g2o::SparseOptimizer (src/sparse_gslam/include/graphs.h:31-40) configured as
 *   OptimizationAlgorithmGaussNewton + BlockSolver<BlockSolverTraits<3,3>> + LinearSolverEigen
 * (src/sparse_gslam/src/graphs.cpp:17-23) through
 *   initializeOptimization(); optimize(20); computeActiveErrors();
 * (src/sparse_gslam/src/submap_loop_closer.cpp:286-288, src/sparse_gslam/src/log_runner.cpp:203-204).
 * The C++ mirror of that API (include/g2o/...) marshals the pointer graph into the flat arrays
 * below at initializeOptimization() and calls these entry points; INTEGRATION.md shows the
 * binding a maintainer adds.
 *
 * Conventions
 *   - plain pointers and sizes, caller-owned buffers, no exceptions, no torch types;
 *   - every function returning int returns >= 0 on success and a negative SGO_E* code on
 *     failure; sgo_last_error() gives the text;
 *   - one sgo_ctx is thread-compatible (one thread at a time, like one g2o::SparseOptimizer,
 *     serialised by the caller's boost::shared_mutex, graphs.h:21,32); different contexts are
 *     independent (own HIP stream and device buffers, no global mutable state);
 *   - all arithmetic is fp64 (g2o number_t = double).
 *
 * Array layout at the boundary (host memory)
 *   poses[V][3]  x, y, theta of vertex id v (ids dense from 0: drone.cpp:64,121; slc.cpp:212)
 *   fixed[V]     1 = VertexSE2::setFixed(true) (drone.cpp:66,75) -> excluded from the system
 *   ei[E], ej[E] vertex ids of EdgeSE2::vertices()[0], [1]   (slc.cpp:214-215, 279-280)
 *   meas[E][3]   EdgeSE2::setMeasurement(SE2(x,y,theta))      (slc.cpp:217, 275)
 *   info[E][6]   EdgeSE2::information(), upper triangle o11,o12,o13,o22,o23,o33 (slc.cpp:216, 276)
 *   phi[E]       DCS parameter of the edge's robust kernel (RobustKernelDCS::setDelta,
 *                slc.cpp:57; attached slc.cpp:283); < 0 = no robust kernel (odometry edges)
 */
#ifndef SGO_H_
#define SGO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGO_VERSION 107          /* 0.1.7: (later additions under the same number, no signature changed: sgo_set_edge_information, sgo_gate_edges; sgo_set_robust_kernels, sgo_edge_robust, SGO_KERNEL_*; sgo_solve_rhs, sgo_marginals; sgo_marginals_selected, SGO_MF_SEL; sgo_direct_plan_array, sgo_debug_direct_array, SGO_DR_*); sgo_stats.pcg_converged may be 2 (a solve accepted at the floating-point floor of its system), the incremental overlay keeps 64 touched + hub rows, SGO_AMG_SETUP (no signature changed); 0.1.6: sgo_plan_rows takes the measurements (row order of graphs whose poses contradict their closures); 0.1.5: the multifrontal path for mid-size graphs (sgo_mfront_plan; sgo_solver_description names it); 0.1.4: sgo_kernel_profile_samples, sgo_update_graph_se2 (incremental set-up); 0.1.3: row-owner multi-GPU mode (sgo_comm_host_allgather, sgo_debug_level0_bytes); 0.1.2: sgo_comm_init_host; 0.1.1: sgo_opts.direct_rows (took a reserved slot), sgo_solver_description */
#define SGO_MAX_ITERS 256        /* capacity of the per-iteration arrays in sgo_stats */

/* error codes (negative).  -1 mirrors g2o's optimize() "nothing to optimise". */
#define SGO_OK 0
#define SGO_ENOTHING (-1)
#define SGO_EINVAL (-2)
#define SGO_EHIP (-3)
#define SGO_ENOGRAPH (-4)
#define SGO_ECOMM (-5)
#define SGO_ENOMEM (-6)

/* linear solver behind BlockSolver::solve (replaces LinearSolverEigen, graphs.cpp:19) */
#define SGO_SOLVER_PCG_BJ 0      /* block-Jacobi preconditioned CG */
#define SGO_SOLVER_PCG_AMG 1     /* CG preconditioned by a rigid-body smoothed-aggregation multigrid V-cycle
                                    with block-Jacobi smoothing (K-cycle on levels that keep the
                                    tentative prolongator) */

typedef struct sgo_ctx sgo_ctx;

typedef struct sgo_opts {
  int32_t struct_size;     /* = sizeof(sgo_opts); lets the struct grow compatibly */
  int32_t solver;          /* SGO_SOLVER_*; env SGO_SOLVER={pcg,amg} overrides the default */
  double pcg_tol;          /* stop when ||r|| <= pcg_tol * ||b||   (env SGO_PCG_TOL); chain-like graphs
                              (< 4 Hessian blocks per free pose, i.e. ill-conditioned and cheap to
                              iterate on) use pcg_tol / 10.  Inside one sgo_optimize_gn call the later
                              Gauss-Newton iterations keep the ABSOLUTE accuracy of the first solve,
                              ||r|| <= pcg_tol * ||b_first||, once their own right-hand side has shrunk
                              below ||b_first|| -- see pcg_tol_cap */
  int32_t pcg_maxit;       /* cap on PCG iterations per GN iteration (env SGO_PCG_MAXIT) */
  int32_t pcg_chunk;       /* graph mode: pcg_chunk / 16 replays of the 2-iteration hipGraph are kept in
                              flight speculatively between checks of the device-side stop flag;
                              plain mode: iterations launched between two host checks */
  int32_t use_graph;       /* 1: replay PCG iterations (incl. the multigrid cycle) from a hipGraph;
                              0: plain stream launches */
  int32_t profile;         /* 1: every launch carries its own start/stop HIP events
                              (hipExtLaunchKernelGGL; forces use_graph=0); per-kernel totals through
                              sgo_kernel_profile() */
  int32_t verbose;         /* mirrors SparseOptimizer::setVerbose (graphs.cpp:21) */
  int32_t direct_rows;     /* small-graph path (solver PCG_AMG, one GPU): a graph with at most this many free poses
                              whose elimination analysis fits -- trajectory chain + closures covered by <= 60
                              separator poses -- runs sgo_optimize_gn as ONE kernel launch of a sparse block
                              LDL^T (nested dissection of the chain, separators dense in LDS); 0 = never
                              (env SGO_DIRECT_ROWS); the single-step entry points keep using the PCG path.
                              The path itself works (and wins) up to ~100k chain-like poses; the default stops
                              where two backward-stable solvers stop agreeing to 1e-6 in chi2 (kappa ~ n^2).
                              Graphs it refuses are offered to the MID-SIZE path next (same conditions: PCG_AMG, one
                              GPU, direct_rows > 0): a multifrontal sparse Cholesky factorisation in nested-dissection
                              order, one launch per level of the elimination tree -- up to 12 288 free poses (env
                              SGO_MFRONT_ROWS), at most 2.5 edges per pose, no front of more than 1 023 rows and
                              at most 80 Mflop on the tree's critical path (env SGO_MFRONT_CRIT_MFLOP); env
                              SGO_MFRONT=0 switches it off.  What it refuses takes the multigrid PCG */
  double pcg_tol_cap;      /* loosest RELATIVE tolerance that absolute criterion may reach (default 1e-6; 0: every
                              solve uses pcg_tol relative to its own ||b||; env SGO_PCG_TOL_CAP).  As Gauss-Newton
                              converges ||b|| falls by orders of magnitude; solving each step to 1e-8 of ITSELF
                              buys no accuracy of the iterates (chi2 is second order in the step's error) and
                              costs a quarter of the PCG iterations */
  int32_t pcg_warm_start;  /* 1 (default): from the second Gauss-Newton iteration of a call PCG starts from the previous
                              step scaled by the energy-optimal factor (b.x_prev)/(x_prev.H x_prev) instead of from zero:
                              same stopping test, about two iterations fewer per solve (env SGO_PCG_WARM) */
  int32_t reserved[4];
} sgo_opts;

/* Environment variables (the call sites are frozen, so knobs come from the environment).  Read when a
 * context is created or a graph is set, or at the start of sgo_optimize_gn / sgo_solve (sgo_ctx::CallKnobs, read_call_knobs) -- never
 * inside a solve.
 *   mirrors of sgo_opts fields (the environment wins): SGO_SOLVER={pcg,amg}, SGO_PCG_TOL, SGO_PCG_TOL_CAP, SGO_PCG_MAXIT,
 *     SGO_PCG_CHUNK, SGO_PCG_WARM, SGO_USE_GRAPH, SGO_PROFILE, SGO_VERBOSE, SGO_DIRECT_ROWS, SGO_DEVICE
 *   path selection: SGO_MFRONT=0 (no multifrontal path), SGO_MFRONT_ROWS / _CRIT_MFLOP / _DEGREE / _LEAF (its admission limits
 *     and leaf size), SGO_INCREMENTAL=0 (sgo_update_graph_se2 is always a full set-up; the g2o-compat header, which reads it too, then also
 *     takes the full set-up after a removeEdge instead of sgo_set_edge_information), SGO_SPMV0={tile,group} (level-0 product
 *     kernel), SGO_PRECOND_F32=0 (fp64 blocks in the preconditioner's level-0 passes)
 *   multigrid set-up: SGO_AMG_THETA (strength threshold), SGO_AMG_THETA_FILTER / SGO_AMG_FILTER=0 (filtered smoothing),
 *     SGO_AMG_SMOOTH=0 (tentative transfers only), SGO_AMG_OMEGA, SGO_AMG_OMEGA_P, SGO_AMG_NU, SGO_AMG_FOLD, SGO_AMG_FOLD0_ROWS,
 *     SGO_AMG_KDEPTH, SGO_AMG_FCG2_DEPTH (cycle shape), SGO_HOST_THREADS (worker pool of the host set-up),
 *     SGO_AMG_SETUP={device,rebuilds,host} (round 6; default device on one GPU: the hierarchy's patterns -- P, A P, P^T A P, the
 *     tentative map -- and lists are made on the device from the host's aggregation, bit-identical to the host set-up's; rebuilds:
 *     only for the rebuilds inside sgo_optimize_gn; host: never), SGO_AMG_AGG=device (opt-in: the aggregation on the device as well --
 *     a parallel independent-set aggregation, weaker hierarchies: DESIGN.md section 5)
 *   inside sgo_optimize_gn: SGO_AMG_LAG=0 (the hierarchy's coarse operators are refreshed before EVERY solve; default: a solve keeps
 *     those of the solve before while the level-0 diagonal blocks have barely moved, and a hierarchy whose aggregation the blocks
 *     have moved far away from is re-made once inside the next call: DESIGN.md section 5), SGO_AMG_LAG_TAU (the largest relative
 *     movement a solve may keep its coarse operators over, 0.006)
 *   multi-GPU: SGO_COMM_MODE={owner,allreduce}, SGO_COMM_GRAPH (see sgo_comm_init), SGO_OWNER_MIN_ROWS, SGO_RCCL_LIB (library path)
 *   test hooks and A/B switches of scripts/ (not for production): SGO_AMG_LISTS=host, SGO_SETUP_PIPELINE, SGO_TILE_LDS,
 *     SGO_FIRST_SOLVE_CAP, SGO_PCG_STALL_WINDOW, SGO_TEST_FAIL_TRIAL_BUILD, SGO_TEST_FAIL_DEVICE_SETUP, SGO_AMG_FORCE_REBUILD, SGO_AMG_KEEP_AGG, SGO_AMG_REBUILD_COST, SGO_MIRROR, SGO_LANCZOS (sgo_debug_lanczos), SGO_MFRONT_DEBUG, SGO_AMG_LAG_FORCE / SGO_AMG_LAG_SLOPE
 *     (scripts/lag_calib.py, tests/test_gpu_lagged_refresh.py)
 * Removed in round 5 (measured, not kept: NOTES.md sections 9-10): SGO_DEFLATE, SGO_OWNER_XS_EXCHANGE, SGO_MFRONT_FUSED_SOLVE.
 * Of the interface SURVEY.md section 8(b) sketched, three items do not exist, on purpose: SGO_NGPU (one process per GPU: the
 * launcher sets the world size, sgo_comm_init takes it), SGO_SOLVER=direct_cpu (the product has no CPU path; the CPU solver is
 * the oracle, test infrastructure), sgo_stats.bytes_moved (algorithmic bytes are per kernel: sgo_kernel_profile). */

/* Defaults (also applied when opts == NULL):
 * solver = PCG_AMG (graphs with <= 400 free poses are preconditioned by an explicit dense inverse,
 * i.e. solved directly; falls back to PCG_BJ only when a larger graph cannot be coarsened),
 * pcg_tol = 1e-8, pcg_maxit = 20000, pcg_chunk = 16, use_graph = 1, direct_rows = 8192, pcg_tol_cap = 1e-6, pcg_warm_start = 1. */
void sgo_default_opts(sgo_opts* o);

typedef struct sgo_stats {
  int32_t iters_requested;
  int32_t iters_done;                        /* GN updates actually applied (the return value is 0 whenever a
                                                linear solve failed, as g2o's optimize(); this still counts the
                                                updates applied before the failure) */
  double chi2[SGO_MAX_ITERS + 1];            /* activeChi2 at the START of iteration k; [iters_done] = final */
  double robust_chi2[SGO_MAX_ITERS + 1];     /* activeRobustChi2, same indexing */
  int32_t pcg_iters[SGO_MAX_ITERS];          /* PCG iterations of GN iteration k (0 on the direct small-graph path) */
  int32_t pcg_converged[SGO_MAX_ITERS];      /* 1 = reached pcg_tol; 2 (round 6) = stopped without reaching it with x at the floating-point
                                              * floor of its system -- backward error of the Jacobi-scaled system, |S r| / (|S^-1 x| + |S b|)
                                              * with r = b - H x and S = diag(H)^-1/2, <= 1e-12 (single GPU): the step WAS applied, as the
                                              * solution of a backward-stable direct solver (LinearSolverEigen) would be;
                                              * 0 = failed: the step was not applied, sgo_optimize_gn returned 0 */
  double pcg_relres[SGO_MAX_ITERS];          /* final ||r|| / ||b|| (recurrence residual) */
  double seconds[SGO_MAX_ITERS];             /* device time of GN iteration k (HIP events) */
  double seconds_linearize[SGO_MAX_ITERS];   /* ... of which error/Jacobian/assembly */
  double seconds_solve[SGO_MAX_ITERS];       /* ... of which the linear solve */
  double seconds_total;                      /* wall time of the whole call (host clock) */
  double seconds_setup;                      /* host structure build + upload of the last set_graph */
} sgo_stats;

int sgo_version(void);

/* Replaces: new g2o::SparseOptimizer + setup_pose_opt() (graphs.cpp:17-23, graphs.h:38).
 * device = HIP device ordinal (env SGO_DEVICE overrides when device < 0).  NULL on failure
 * (sgo_last_error(NULL) has the reason). */
sgo_ctx* sgo_create(int device, const sgo_opts* opts);
/* Replaces: ~SparseOptimizer.  Never frees caller memory (README.md:22-23). */
void sgo_destroy(sgo_ctx* ctx);

/* Replaces: SparseOptimizer::initializeOptimization() (slc.cpp:286, log_runner.cpp:203): takes
 * the active vertices/edges, builds the hessian index map (non-fixed vertices in ascending id),
 * the block-sparse structure (rows numbered internally along a Hilbert curve through the poses, every
 * off-diagonal block stored once inside a tile of rows) and the device-resident SoA edge arrays.  Edges
 * whose endpoints are both fixed stay active for chi2 only.  With a communicator attached
 * (sgo_comm_init) every rank passes the same full graph. */
int sgo_set_graph_se2(sgo_ctx* ctx, int32_t V, const double* poses, const uint8_t* fixed, int32_t E,
                      const int32_t* ei, const int32_t* ej, const double* meas, const double* info,
                      const double* phi);

/* Incremental form of the same call for the reference's flow: after every accepted loop closure it appends a chain of
 * new poses with their odometry edges (slc.cpp:205-226) and one closure edge (slc.cpp:272-285) to the graph it optimised
 * before, then calls initializeOptimization(); optimize(20) again (slc.cpp:286-287).  Arguments as sgo_set_graph_se2 -- the
 * WHOLE new graph -- plus n_resident_edges: the caller's statement that edges [0, n_resident_edges) and the vertices they
 * use are the graph this context already holds, unchanged (ids, measurement, information, kernel, fixed flags; estimates
 * may differ: `poses` is uploaded in full).  When that is the resident graph and the appended part has the shape above --
 * new free poses whose mutual edges form a chain in id order, any edges between new and resident poses or among resident
 * poses, within the capacities of sgo_overlay.h -- the appended part becomes an overlay beside the resident level-0
 * structure and multigrid hierarchy, which are kept (the Gauss-Newton systems are still solved exactly: the chain is
 * eliminated by a block-tridiagonal factorisation, the resident rows by PCG on the Schur complement).  Otherwise --
 * including n_resident_edges == 0, a multi-GPU context, a graph on the single-launch direct path, an overlay whose PCG
 * iteration counts have drifted -- the call IS sgo_set_graph_se2.  sgo_solver_description says which happened.  While an
 * overlay is resident the single-step entry points (sgo_linearize, sgo_hessian_apply, sgo_precondition, sgo_solve) return
 * SGO_EINVAL; sgo_optimize_gn, sgo_chi2, sgo_edge_chi2, sgo_get_poses, sgo_set_poses, sgo_num_free, sgo_free_ids cover the
 * whole graph. */
int sgo_update_graph_se2(sgo_ctx* ctx, int32_t V, const double* poses, const uint8_t* fixed, int32_t E,
                         const int32_t* ei, const int32_t* ej, const double* meas, const double* info,
                         const double* phi, int32_t n_resident_edges);

/* Replaces: VertexSE2::setEstimate on every vertex (slc.cpp:219) without a structure rebuild. */
int sgo_set_poses(sgo_ctx* ctx, const double* poses);
/* Replaces: reading VertexSE2::estimate() after optimize() (slc.cpp:144-148, log_runner.cpp:258-267). */
int sgo_get_poses(sgo_ctx* ctx, double* poses);

/* Replaces: SparseOptimizer::optimize(iters) with OptimizationAlgorithmGaussNewton (slc.cpp:287,
 * log_runner.cpp:204): iters x { computeActiveErrors; buildSystem; solve; update }, no damping, no
 * convergence test.  Returns iterations done; 0 when a linear solve failed -- PCG breakdown (H not
 * positive definite) or pcg_maxit reached without pcg_tol (on one GPU also: the residual has not reached a new minimum for
 * max(3000, 30 x the previous solve's count) iterations -- a solve that stagnates is not ground on to pcg_maxit): that step
 * is not applied, the estimates stay
 * at the last applied update (out->iters_done of them) and sgo_last_error has the reason, as
 * g2o::SparseOptimizer::optimize returns 0 on OptimizationAlgorithm::Fail; SGO_ENOTHING (-1) when
 * there is no free active vertex; or another negative code.
 * `out` may be NULL. */
int sgo_optimize_gn(sgo_ctx* ctx, int32_t iters, sgo_stats* out);

/* (later additions, version 107) Gauss-Newton that ends at convergence: g2o's SparseOptimizerTerminateAction as one call
 * (DESIGN.md section 5h).
 *
 * The gain rule, a pure function (no context, no GPU): with last_robust_chi2 and robust_chi2 the robust chi2 at the start of the
 * previous and of the current iteration,
 *     gain = (last_robust_chi2 - robust_chi2) / robust_chi2;   returns 1 iff gain >= 0 && gain < gain_tol, else 0.
 * A negative gain does not stop (DCS makes chi2 non-monotone), gain_tol <= 0 never stops, and robust_chi2 == 0 or a non-finite
 * argument gives NaN or inf, for which a comparison is false: 0. */
int sgo_gain_stop(double last_robust_chi2, double robust_chi2, double gain_tol);

/* sgo_optimize_gn(ctx, max_iters, out) that ends early: before iteration `it` with 2 <= it < max_iters the call stops iff
 * sgo_gain_stop(robust_chi2[it - 1], robust_chi2[it], gain_tol).  At least two updates always run (g2o's action stores chi2 only
 * after the first).  A stop before iteration `it` ends the call with `it` updates applied: out->iters_done = it, chi2[it] and
 * robust_chi2[it] are the final values, only the entries of applied iterations are filled, out->iters_requested = max_iters.
 * Every iteration before the stop is the one sgo_optimize_gn(max_iters) runs: the histories agree bit for bit up to the stop.  On
 * the factorisation paths the rule is applied on the device (no host round trip inside the call), and the poses and the factor are
 * bit for bit those of sgo_optimize_gn(it); on the PCG path, an active incremental overlay included, the host reads chi2 once per
 * iteration and starts no solve for the stopped iteration.
 * *stop_reason (may be NULL; written when the return value is >= 0) is one of SGO_STOP_*: max_iters updates applied, the gain rule,
 * or a failed linear solve (return value 0, the step not applied, as sgo_optimize_gn).
 * Return values and argument checks are sgo_optimize_gn's; SGO_EINVAL in addition, with the poses untouched, for a gain_tol that
 * is not finite and for a multi-GPU context (sgo_debug_set_shard's emulation included). */
#define SGO_STOP_MAX_ITERS 0
#define SGO_STOP_GAIN 1
#define SGO_STOP_FAILED 2
int sgo_optimize_gn_until(sgo_ctx* ctx, int32_t max_iters, double gain_tol, sgo_stats* out, int32_t* stop_reason);

/* (later additions, version 107) Levenberg-Marquardt on the multifrontal factor.
 * Replaces: SparseOptimizer::optimize(iters) with OptimizationAlgorithmLevenberg on a pose-only SE(2) graph, with g2o 2020.5.29's
 * schedule.  lambda_0 = lambda_init, or 1e-5 * max |diag(H)| at the starting poses when lambda_init <= 0, is set at iteration 0 of
 * every call, and nu = 2.  One trial solves (H + lambda I) x = b -- H and b the robustified system of every kernel kind at the
 * accepted poses -- and scores the poses (+) x by
 *     scale = x . (lambda x + b) + 1e-3,   rho = (robust chi2 at the accepted poses - robust chi2 at the trial poses) / scale.
 * It is accepted iff rho > 0, the trial chi2 is finite and the solve succeeded: lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)),
 * nu = 2, the trial poses become the accepted ones.  Otherwise lambda *= nu, nu *= 2; a pivot that is not positive definite or a
 * non-finite solution is such a rejection, not a failed call.  An iteration repeats trials while rho < 0 and fewer than ten have
 * run; the call terminates after ten trials of one iteration, at rho == 0 exactly, or when lambda is no longer finite (that last
 * trial is counted).
 *
 * sgo_lm_trial_rule is that rule for one trial as the library and its kernel compile it (no context, no GPU): `scale` includes the
 * 1e-3; *lambda and *nu are updated in place.  Returns 1: accepted; 0: rejected with rho < 0 (the iteration tries again); 2:
 * rejected with rho == 0; 3: rejected otherwise (rho is NaN, or positive with a non-finite trial chi2) -- the iteration ends.
 *
 * The solves go through the multifrontal factor: the resident plan on a multifrontal_cholesky context, otherwise a plan analysed once
 * per set-up (as sgo_marginals_selected does), whatever path sgo_optimize_gn takes.  The trials and their decisions run on the
 * device; the host reads the state once per round of queued trials (out->sync_rounds: 1 for a call without a rejection, at most
 * 1 + the rejected trials).  Two calls from the same state return the same bits.
 * Returns the iterations counted (out->iters_done; `out` may be NULL).  robust_chi2[k + 1], chi2[k + 1] and lambda[k] are the values
 * at the accepted poses after iteration k, trials[k] its trials; robust_chi2[] never increases, and the entries [iters_done] are
 * what sgo_chi2 returns after the call, bit for bit.  Afterwards the context is as after sgo_set_poses(the final poses):
 * sgo_optimize_gn keeps its path and its bits, and the joint tables stay the snapshots they are.
 * SGO_EINVAL, with nothing changed: max_iters outside [0, SGO_MAX_ITERS], a lambda_init that is not finite, an active incremental
 * overlay, a multi-GPU context (sgo_debug_set_shard's emulation included).  SGO_ENOTHING when there is no free active vertex, and,
 * with the analysis' reason in sgo_last_error, when the multifrontal analysis refuses the graph: use sgo_optimize_lm_pcg (below) or
 * sgo_optimize_gn then. */
#define SGO_LM_STOP_MAX_ITERS 0   /* max_iters iterations counted */
#define SGO_LM_STOP_TRIALS    1   /* ten trials of one iteration rejected (g2o: Terminate) */
#define SGO_LM_STOP_ZERO_GAIN 2   /* rho == 0 exactly */
#define SGO_LM_STOP_LAMBDA    3   /* lambda no longer finite */
typedef struct sgo_lm_stats {
  int32_t iters_requested, iters_done, trials_total, stop_reason, sync_rounds;
  double  lambda0;
  double  lambda[SGO_MAX_ITERS];          /* after iteration k */
  double  robust_chi2[SGO_MAX_ITERS + 1]; /* [0] at the start, [k+1] at the accepted poses after iteration k */
  double  chi2[SGO_MAX_ITERS + 1];        /* plain chi2, same indexing */
  int32_t trials[SGO_MAX_ITERS];
  double  seconds_total;
} sgo_lm_stats;
int sgo_optimize_lm(sgo_ctx* ctx, int32_t max_iters, double lambda_init /* <= 0: 1e-5 * max diag(H) */, sgo_lm_stats* out);
int sgo_lm_trial_rule(double cur, double trial, double scale, int solve_ok, double* lambda, double* nu); /* pure, no GPU */

/* (later additions, version 107) Levenberg-Marquardt on the PCG: sgo_optimize_lm's schedule -- lambda_0, nu,
 * the gain ratio over x . (lambda x + b) + 1e-3, ten trials, g2o's terminations, sgo_lm_stats filled the same way, the same return
 * values and the same SGO_EINVAL refusals with nothing changed -- with every trial's (H + lambda I) x = b solved by the
 * preconditioned conjugate gradients: cold from x = 0, at pcg_tol (times the chain-graph scale of sgo_optimize_gn) relative to the
 * trial's own |b|, behind a hierarchy refreshed for H + lambda I before every trial.  It differs in three ways:
 *   - It works on EVERY single-GPU context -- PCG with multigrid, PCG with block-Jacobi, single-launch direct, multifrontal; the last
 *     two build the row plan and the hierarchy on first use, as sgo_marginals and sgo_linearize do -- and is never refused for the
 *     graph's size or density.  SGO_ENOTHING only when there is no free active vertex.
 *   - out->sync_rounds equals the trials run: the PCG reads its scalars on the host anyway, so the state is read once per trial.
 *   - A trial whose solve breaks down (p . H p <= 0 or non-finite), or stops short of pcg_tol without standing at the
 *     floating-point floor of its system, is a REJECTED trial, not a failed call: lambda grows and the next trial's system is
 *     better conditioned.  sgo_optimize_gn's rebuild / re-aggregation recoveries are not used.
 * The decision of a trial is taken on the device by the rule sgo_lm_trial_rule states; two calls from the same state return the same
 * bits; robust_chi2[] never increases and its last entries are sgo_chi2's bits.  Afterwards the context is as after
 * sgo_set_poses(the final poses): the next sgo_optimize_gn refreshes its hierarchy and starts cold, keeps its path and its bits; what
 * the hierarchy has learned (its best count, the lag calibration) and the resident factor and joint tables are untouched.
 *
 * sgo_lm_pcg_trace: the trials of the context's last sgo_optimize_lm_pcg.  Returns their number and fills, for the first `cap` of
 * them (either array may be NULL), the trial's PCG iteration count and how its solve ended: SGO_LM_SOLVE_CONVERGED (pcg_tol reached),
 * SGO_LM_SOLVE_FLOOR (accepted at the floating-point floor), or, for a failed solve -- a rejected trial --, minus the PCG's stop
 * code: -2 out of iterations or stagnated, -3 breakdown.  SGO_EINVAL for a NULL context or a negative cap. */
#define SGO_LM_SOLVE_CONVERGED 1
#define SGO_LM_SOLVE_FLOOR 2
int sgo_optimize_lm_pcg(sgo_ctx* ctx, int32_t max_iters, double lambda_init /* <= 0: 1e-5 * max diag(H) */, sgo_lm_stats* out);
int sgo_lm_pcg_trace(sgo_ctx* ctx, int32_t cap, int32_t* pcg_iters, int32_t* solve_stop);

/* (later additions, version 107) Powell's dogleg.
 * Replaces: SparseOptimizer::optimize(iters) with OptimizationAlgorithmDogleg on a pose-only SE(2) graph, with g2o 2020.5.29's
 * schedule.  At iteration 0 of every call delta = delta_init (<= 0: 1e4), the damping lambda = 1e-7 and "H was positive definite in
 * every iteration" holds.  An iteration solves the UNDAMPED system H g = b once -- H and b the robustified system of every kernel
 * kind at the accepted poses -- and forms the Cauchy step alpha b, alpha = b.b / b.Hb.  Every trial of the iteration is a blend of
 * those two fixed vectors, chosen by delta:
 *     |g| < delta: h = g (GN);   else |alpha b| > delta: h = (delta / |alpha b|) alpha b (SD);   else the point of the segment
 *     from alpha b to g at distance delta (DL).
 * With the linear gain L = -h.Hh + 2 b.h (|L| < 1e-12: 1e-12) and rho = (robust chi2 at the accepted poses - at poses (+) h) / L the
 * trial is accepted iff rho > 0 and the trial chi2 is finite; rho > 0.75: delta = max(delta, 3 |h|); rho < 0.25: delta *= 0.5.  One
 * deviation from g2o: a trial chi2 or rho that is not finite counts as rho = -inf (rejected, delta halved).  An iteration repeats
 * trials until one is accepted or 100 have run; the latter ends the call (SGO_DL_STOP_TRIALS; that iteration is counted).
 * Damping applies only after a failed solve (a pivot that is not positive definite, a non-finite solution, on the PCG a solve that
 * neither converged nor stands at its floating-point floor): lambda *= 10, beyond 1e3 the call ends (SGO_DL_STOP_DAMPING, poses at
 * the accepted ones), otherwise the solve is repeated on H + lambda I, as is every later solve of the call, each success followed
 * by lambda = max(1e-12, lambda / 5).  While no solve has failed nothing is added and the GN step is sgo_optimize_gn's to the bit
 * on a multifrontal_cholesky context.
 *
 * sgo_dogleg_step_rule / sgo_dogleg_trial_rule are the two rules as the library and its kernels compile them (no context, no GPU).
 * forms = {b.b, b.g, g.g, b.Hb, b.Hg, g.Hg}; the step is h = a b + c g; returns its kind (SGO_DL_STEP_*), or SGO_EINVAL for a NULL
 * pointer.  The trial rule updates *delta in place and returns 1: accepted, 0: rejected.
 *
 * sgo_optimize_dogleg solves through the multifrontal factor (the route of sgo_optimize_lm: refusals, plan and what the call leaves
 * are that call's; a graph the analysis refuses: SGO_ENOTHING, use sgo_optimize_dogleg_pcg or sgo_optimize_gn); the host queues one
 * iteration per remaining iteration and reads the state once per round: sync_rounds is 1 for a call without a rejection and at
 * most 1 + the rejected trials while H stays positive definite.  A rejected trial costs one chi2 pass and three small launches: no
 * edge pass, no factorisation.  sgo_optimize_dogleg_pcg solves with the context's preconditioned conjugate gradients (the route
 * of sgo_optimize_lm_pcg: every single-GPU context, a refreshed hierarchy and a cold solve per ITERATION; the state is read once per
 * solve and once per group of re-trials).  `solves` counts factorisations or PCG solves: iters_done while H stayed positive
 * definite, whatever trials_total is.
 * Returns the iterations counted (`out` may be NULL).  robust_chi2[k + 1], chi2[k + 1], delta[k] are the values after iteration k,
 * trials[k] its trials, step_kind[k] the accepted trial's kind (-1: none); robust_chi2[] never increases and the entries
 * [iters_done] are what sgo_chi2 returns after the call, bit for bit.  Two calls from the same state return the same bits. */
#define SGO_DL_STOP_MAX_ITERS 0   /* max_iters iterations counted */
#define SGO_DL_STOP_TRIALS    1   /* 100 trials of one iteration rejected (g2o: Terminate) */
#define SGO_DL_STOP_DAMPING   2   /* the damping passed 1e3 without a successful solve (g2o: Fail) */
#define SGO_DL_STEP_GN 0
#define SGO_DL_STEP_SD 1
#define SGO_DL_STEP_DL 2
typedef struct sgo_dogleg_stats {
  int32_t iters_requested, iters_done, trials_total, solves, stop_reason, sync_rounds;
  double  delta0;
  double  delta[SGO_MAX_ITERS];           /* after iteration k */
  double  robust_chi2[SGO_MAX_ITERS + 1]; /* [0] at the start, [k+1] at the accepted poses after iteration k */
  double  chi2[SGO_MAX_ITERS + 1];        /* plain chi2, same indexing */
  int32_t trials[SGO_MAX_ITERS];
  int32_t step_kind[SGO_MAX_ITERS];       /* SGO_DL_STEP_* of the accepted trial; -1: none */
  double  lambda;                         /* the last damping a solve used; 0 while H was always positive definite */
  double  seconds_total;
} sgo_dogleg_stats;
int sgo_optimize_dogleg(sgo_ctx* ctx, int32_t max_iters, double delta_init /* <= 0: 1e4 */, sgo_dogleg_stats* out);
int sgo_optimize_dogleg_pcg(sgo_ctx* ctx, int32_t max_iters, double delta_init /* <= 0: 1e4 */, sgo_dogleg_stats* out);
int sgo_dogleg_step_rule(double delta, const double forms[6], double* a, double* c, double* step_norm, double* linear_gain); /* pure, no GPU */
int sgo_dogleg_trial_rule(double cur, double trial, double linear_gain, double step_norm, double* delta);                    /* pure, no GPU */

/* (later additions, version 107) Many closure hypotheses of the resident graph in one call: "is this set of
 * closures consistent", leave-one-out over a round's closures, cluster tests -- the same graph optimised once per hypothesis.
 *
 * Hypothesis b is the resident graph with every edge k with edge_off[b][k] != 0 deactivated, as sgo_set_edge_information does with
 * an all-zero row; an edge the context holds inactive already stays inactive in every hypothesis.  It starts from poses0[b] -- taken
 * as sgo_set_poses takes its argument: every entry as given, those of fixed vertices included, so pass the resident values there
 * -- or, with poses0 == NULL, from the resident poses, and runs sgo_optimize_gn_until(max_iters, gain_tol); gain_tol <= 0 never
 * stops, which is sgo_optimize_gn(max_iters).
 *   res[b]          updates applied, SGO_STOP_*, and (chi2, robust chi2) at the hypothesis' final poses
 *   hist[b]         (chi2, robust chi2) at the start of every applied iteration and at the end; the entries behind them are NaN
 *   poses_out[b]    the final poses (of a failed hypothesis: the last applied update)
 *   edge_chi2[b][k] e^T Omega e of edge k at those poses with the RESIDENT information: an edge the hypothesis switched off reports
 *                   what it would cost (the number a consistency test needs), an edge the context holds inactive reports 0
 * hist, poses_out and edge_chi2 may be NULL.  On the factorisation paths everything but edge_chi2 is, bit for bit, what the host
 * loop { sgo_set_edge_information(zero rows); sgo_set_poses; sgo_optimize_gn_until; read back; restore the rows } returns.
 * A linear solve that fails -- a pivot that is not positive definite, a non-finite update -- fails its hypothesis alone
 * (SGO_STOP_FAILED, iters_done the updates applied before); the call still returns >= 0.
 * The context is left as it was: resident poses, informations, kernel kinds, edge activity, sgo_stats.seconds_setup and
 * sgo_solver_description.
 * Returns the route taken: SGO_HYP_BATCHED on a direct_ldlt context -- ONE launch of B workgroups of the single-launch kernel,
 * each on its own copy of what the kernel writes (workspaces of the context's, grown on demand; SGO_ENOMEM with the context intact
 * when they do not fit), the resident factor untouched -- and SGO_HYP_SEQUENTIAL on every other single-GPU path: the host loop
 * above inside the call, the resident solver's own arrays serving every hypothesis and the hierarchy's coarse operators refreshed
 * by the next solve as after any sgo_set_edge_information (a multifrontal_cholesky context that has been granted memory batches
 * too: sgo_set_hypotheses_workspace below).  B == 0 returns SGO_HYP_BATCHED and does nothing.
 * SGO_EINVAL, with nothing changed and no output written: B < 0, max_iters outside [0, SGO_MAX_ITERS], a NULL edge_off or res
 * with B > 0, a non-finite gain_tol or poses0 entry, a multi-GPU context (sgo_debug_set_shard's emulation included), an active
 * incremental overlay, and a hypothesis that would leave a free pose without any incident edge of non-zero information
 * (sgo_set_edge_information's rule, decided on the host before anything is queued; sgo_last_error names hypothesis and vertex). */
typedef struct sgo_hypothesis_result {
  int32_t iters_done;      /* updates applied */
  int32_t stop_reason;     /* SGO_STOP_MAX_ITERS / SGO_STOP_GAIN / SGO_STOP_FAILED */
  double chi2, robust_chi2;/* at the hypothesis' final poses */
} sgo_hypothesis_result;
#define SGO_HYP_BATCHED 1     /* all hypotheses in one launch */
#define SGO_HYP_SEQUENTIAL 2  /* one after the other through the resident solver */
int sgo_optimize_gn_hypotheses(sgo_ctx* ctx, int32_t B, int32_t max_iters, double gain_tol,
                               const uint8_t* edge_off /*[B][E]*/, const double* poses0 /*[B][V][3] or NULL*/,
                               sgo_hypothesis_result* res /*[B]*/, double* hist /*[B][max_iters+1][2] or NULL*/,
                               double* poses_out /*[B][V][3] or NULL*/, double* edge_chi2 /*[B][E] or NULL*/);
/* That rule as a pure function (no context, no GPU): info[E][6] the resident rows, off[E] one hypothesis' mask.  Returns the lowest
 * free vertex that an edge the mask switches off (one whose resident row is not all zero) leaves without any incident edge of
 * non-zero information, -1 when there is none, SGO_EINVAL for a NULL buffer, a negative count or an endpoint outside [0, V). */
int32_t sgo_hypothesis_isolated_vertex(int32_t V, const uint8_t* fixed, int32_t E, const int32_t* ei, const int32_t* ej,
                                       const double* info, const uint8_t* off);

/* (later additions, version 107) The batched route of sgo_optimize_gn_hypotheses on a multifrontal_cholesky context (DESIGN.md
 * section 5i-2).  It is opt-in: every hypothesis of a launch chain owns a copy of everything the factorisation writes -- the frontal
 * arena above all, up to 1 GiB -- and the library does not take that memory unasked.
 *
 * sgo_set_hypotheses_workspace grants the context max_bytes of device memory for those copies; 0 (the default) is the behaviour
 * described above, exactly.  The grant is the context's: it survives sgo_set_graph_se2, the workspace is allocated by the first call
 * that uses it, grown on demand and freed by sgo_destroy.  A negative value is refused (SGO_EINVAL).  It has no effect on direct_ldlt
 * contexts (always SGO_HYP_BATCHED) or on PCG contexts (always SGO_HYP_SEQUENTIAL).
 *
 * With chunk = sgo_hypotheses_chunk(sgo_hypotheses_bytes(ctx, max_iters, edge_chi2 != NULL), max_bytes, B) >= 2,
 * sgo_optimize_gn_hypotheses on a multifrontal context runs its B hypotheses in ceil(B / chunk) launch chains -- the launches of one
 * sgo_optimize_gn_until, each shared by the chain's hypotheses, so that the upper levels of the elimination tree fill the chip -- and
 * returns SGO_HYP_BATCHED; otherwise it takes the sequential route.  Argument checks and refusals are the same on both routes and
 * come first.  Everything a hypothesis returns but edge_chi2 is bit for bit what the sequential route returns, whatever the chunk;
 * edge_chi2 is e^T Omega e with the resident rows in one pass behind the chain (an active edge: the very term of the hypothesis'
 * final chi2).  A hypothesis that fails or that the gain rule stops costs its chain nothing more and disturbs no neighbour.
 * UNLIKE the sequential route, the batched one writes nothing of the resident solver: the factor and its arrays (sgo_debug_mfront_array),
 * the poses and the informations are not those of the last hypothesis afterwards but what they were before the call.
 * SGO_ENOMEM, with the context intact, when the workspace cannot be allocated.
 * The grant is a hard bound: the workspace this route allocates is chunk * sgo_hypotheses_bytes(...) bytes exactly, with no head-room,
 * and so never more than max_bytes.  (A workspace the context already holds -- from a larger grant or from a direct_ldlt graph -- is
 * reused as it is and not shrunk.)  sgo_hypotheses_workspace_bytes: the bytes the context's hypotheses workspace holds now, 0 before
 * the first call that needed it, < 0 for a NULL context.
 *
 * sgo_hypotheses_bytes: the device memory one hypothesis takes on the resident graph for these arguments; 0 where there is no batched
 * multifrontal route (another solver path, an active incremental overlay, a multi-GPU context), < 0 for a bad context or max_iters.
 * sgo_hypotheses_chunk (pure: no context, no GPU): hypotheses per launch chain, min(B, budget / per, 65535); 0 -- the sequential
 * route -- when that is below 2 or per_hypothesis_bytes <= 0. */
int sgo_set_hypotheses_workspace(sgo_ctx* ctx, int64_t max_bytes);
int64_t sgo_hypotheses_bytes(sgo_ctx* ctx, int32_t max_iters, int32_t want_edge_chi2);
int64_t sgo_hypotheses_workspace_bytes(sgo_ctx* ctx);
int32_t sgo_hypotheses_chunk(int64_t per_hypothesis_bytes, int64_t budget_bytes, int32_t B);

/* (later additions, version 107) Many INDEPENDENT pose graphs in one call: a back-end that serves the graphs
 * of a swarm, several sessions or maps of one robot, or a sweep over many logs.
 * Replaces: a loop of SparseOptimizer::optimize(max_iters) over several SparseOptimizers -- for (i) sgo_optimize_gn_until(ctxs[i],
 * ...), one launch and one synchronisation per graph, each on one compute unit while the rest of the chip idles.
 *
 * Context i ends as after sgo_optimize_gn_until(ctxs[i], max_iters, gain_tol, out[i], &res[i].stop_reason) -- poses, chi2 history,
 * sgo_stats, sgo_last_error, bit for bit -- and res[i].rc is what that call would have returned; gain_tol <= 0 never stops, which
 * is sgo_optimize_gn(max_iters).  out, or any entry of it, may be NULL.  sgo_stats.seconds_total is the wall time of the whole call.
 * Every direct_ldlt context joins ONE launch of the single-launch kernel with a workgroup per graph, each working from its own
 * plan, edges and poses (res[i].in_launch = 1).  Graphs whose kernel differs at compile time -- edges with kernels other than DCS
 * (sgo_set_robust_kernels), a right-hand side too long for the LDS -- take a launch per kind, at most four, back to back; *launches
 * (may be NULL) is their number, 1 for the usual homogeneous call.  A context on another path -- multifrontal_cholesky, PCG, an
 * active incremental overlay, no free pose, SGO_DIRECT_DEBUG at its set-up -- runs its own sgo_optimize_gn_until inside the call,
 * after the shared launch has been queued (in_launch = 0).
 * A linear solve that fails fails its graph alone: rc 0, SGO_STOP_FAILED, the step not applied, the reason in that context's
 * sgo_last_error; an error of one context's own route is that context's rc.  No other context is touched by either.
 * Returns the number of contexts whose call ended without an error and without a failed solve; 0 for n == 0.
 * The first context owns the call's workspace (job table, histories, result records; device and pinned host memory, grown on
 * demand, reused by later calls, freed by its sgo_destroy) and its stream carries the launch, which starts after every
 * participant's pending work; the call returns after the launch has finished.  With sgo_opts.profile the first context's
 * "direct" slot records each shared launch once, with the summed bytes.  sgo_many_workspace_bytes: the bytes that workspace holds
 * now (device + pinned), 0 before the first call that needed it, < 0 for a NULL context.
 * SGO_EINVAL, with nothing queued and no pose or output written: n < 0, max_iters outside [0, SGO_MAX_ITERS], a non-finite
 * gain_tol, a NULL ctxs or res with n > 0, a NULL or duplicate context, contexts on different devices, a multi-GPU context
 * (sgo_debug_set_shard's emulation included).  SGO_ENOGRAPH, likewise, if any context has no graph.  At most 65535 graphs share
 * a launch; more take further launches.  The contexts must not be used from other threads during the call. */
typedef struct sgo_many_result {
  int32_t rc;           /* what sgo_optimize_gn_until would have returned */
  int32_t stop_reason;  /* SGO_STOP_*; written when rc >= 0 */
  int32_t in_launch;    /* 1: ran in the shared launch, 0: own route */
} sgo_many_result;
int sgo_optimize_gn_many(sgo_ctx* const* ctxs, int32_t n, int32_t max_iters, double gain_tol,
                         sgo_stats* const* out /*[n], entries or the array may be NULL*/, sgo_many_result* res /*[n]*/,
                         int32_t* launches /*may be NULL*/);
int64_t sgo_many_workspace_bytes(sgo_ctx* ctx);

/* Replaces: computeActiveErrors(); activeChi2(); activeRobustChi2() (slc.cpp:288, drone.cpp:162-165).
 * Called right after sgo_optimize_gn or sgo_optimize_gn_until it returns the final entries of that call's history bit for bit
 * (on a direct_ldlt context the sums come from the single-launch kernel's own closing pass). */
int sgo_chi2(sgo_ctx* ctx, double* plain, double* robust);
/* Replaces: EdgeSE2::computeError(); chi2() per edge (log_runner.cpp:183-184, the 11.345 gate).
 * e2[E] in the edge order given to sgo_set_graph_se2. */
int sgo_edge_chi2(sgo_ctx* ctx, double* e2);

/* Replaces: EdgeSE2::setInformation on resident edges, and SparseOptimizer::removeEdge + initializeOptimization
 * (log_runner.cpp:186,203) with an all-zero row.  edge_ids in [0, E) in the order given to sgo_set_graph_se2 /
 * sgo_update_graph_se2 (appended overlay edges included); info[n][6] upper triangles.  Keeps every resident structure.
 *
 * An edge whose information is all zero is DEACTIVATED: it adds nothing to chi2, to the right-hand side or to any Hessian
 * block, reports 0 in sgo_edge_chi2 and contributes 0 to sgo_chi2 -- the graph optimises as if the edge had been removed, while
 * the row plan, the tiles, the elimination trees, the overlay and the multigrid hierarchy's aggregation stay as they are (no
 * set-up; sgo_stats.seconds_setup does not change).  Its original row through the same call brings it back.  The first solve
 * of the next sgo_optimize_gn / sgo_solve refreshes the hierarchy's coarse operators from the new blocks; an earlier
 * sgo_linearize is void.  sgo_solver_description keeps naming the same path and ends in "; K edges inactive" while K > 0 edges
 * carry a zero information.
 * SGO_EINVAL, with nothing on the device changed: a multi-GPU context (sgo_debug_set_shard's emulation included), an id outside
 * [0, E), a non-finite entry, and a change that would leave a free pose without any incident edge of non-zero information
 * (sgo_last_error names the vertex; its diagonal block would be singular).  Disconnecting the graph in any other way is the
 * caller's responsibility, as it is in g2o.  Of an id listed twice the later row counts.
 * A later sgo_update_graph_se2 or sgo_set_graph_se2 takes its arrays at face value: pass zero rows there for the edges that
 * are to stay inactive (an incremental update's resident prefix is not re-read: those edges keep what they have). */
int sgo_set_edge_information(sgo_ctx* ctx, int32_t n, const int32_t* edge_ids, const double* info);

/* Replaces: the chi2 gate of log_runner.cpp:182-189, on the device.  For the listed edges (edge_ids == NULL: every edge with
 * phi >= 0, n then ignored) evaluates e^T Omega e at the current poses with the arithmetic of sgo_edge_chi2 and
 * deactivates (information := 0) those with chi2 > chi2_max.  gated[n] (or [E] with NULL ids; may be NULL) = 1 for the
 * edges it deactivated.  Returns how many (an id listed twice counts once; an edge that is inactive already is left alone), or a
 * negative code.  The decision is taken first and nothing is written when the call refuses: rules, refusals and what the next
 * solve does are sgo_set_edge_information's. */
int sgo_gate_edges(sgo_ctx* ctx, int32_t n, const int32_t* edge_ids, double chi2_max, uint8_t* gated);

/* The robust kernels of g2o's robust_kernel_impl.h, per edge.  With e = e^T Omega e, d = delta and s = sqrt(e), a kernel is the
 * pair rho0 (what the edge adds to the robust chi2) and rho1 (the weight: g2o's robust Gauss-Newton scales the edge's
 * information and Omega e by rho1 and uses nothing else):
 *   NONE           e                                                 1
 *   DCS            RobustKernelDCS, as phi >= 0 in sgo_set_graph_se2: with c = 2 d / (d + e), e and 1 if c >= 1, else c^2 e and c^2
 *   HUBER          e if e <= d^2, else 2 s d - d^2                    1, else d / s
 *   PSEUDO_HUBER   2 d^2 (a - 1), a = sqrt(1 + e / d^2)              1 / a
 *   CAUCHY         d^2 log a, a = 1 + e / d^2                        1 / a
 *   GEMAN_MCCLURE  e a, a = 1 / (1 + e)  (delta unused, as in g2o)   a^2
 *   WELSCH         d^2 (1 - a), a = exp(-e / d^2)                    a
 *   FAIR           2 d^2 (a - log1p a), a = s / d                    1 / (1 + a)
 *   TUKEY          d^2 (1 - u^3) / 3, u = 1 - e / d^2, if s <= d; else d^2 / 3      u^2, else 0
 *   SATURATED      e if e <= d^2, else d^2                           1, else 0 */
#define SGO_KERNEL_NONE 0
#define SGO_KERNEL_DCS 1
#define SGO_KERNEL_HUBER 2
#define SGO_KERNEL_PSEUDO_HUBER 3
#define SGO_KERNEL_CAUCHY 4
#define SGO_KERNEL_GEMAN_MCCLURE 5
#define SGO_KERNEL_WELSCH 6
#define SGO_KERNEL_FAIR 7
#define SGO_KERNEL_TUKEY 8
#define SGO_KERNEL_SATURATED 9

/* Replaces: OptimizableGraph::Edge::setRobustKernel(new RobustKernelHuber / ...Cauchy / ...) with setDelta(delta) on resident
 * edges.  edge_ids as for sgo_set_edge_information (NULL: edges 0 .. n-1; appended overlay edges included), kind[n] one of
 * SGO_KERNEL_*, delta[n] the kernel's parameter (ignored by NONE, unused by GEMAN_MCCLURE).  Every solver path evaluates the
 * kind where it evaluates phi; a graph that holds only NONE and DCS edges runs the kernels, and gives the bits, of one that never
 * made this call.  Keeps every resident structure: no set-up, sgo_stats.seconds_setup does not change, an earlier sgo_linearize
 * is void, and the first solve of the next sgo_optimize_gn / sgo_solve refreshes the hierarchy's coarse operators.  An edge whose
 * information is zero has e = 0, where every kind gives rho0 = 0 and weight 1 (DCS with delta = 0 excepted: 2 d / (d + e) is
 * 0 / 0 there, as in g2o): deactivating and gating compose with any kind
 * (sgo_gate_edges with NULL ids gates the edges with any kernel, all but NONE).
 * SGO_EINVAL, with nothing on the device changed: a multi-GPU context (sgo_debug_set_shard's emulation included), an id outside
 * [0, E), an unknown kind, a non-finite delta, delta < 0 for DCS, delta <= 0 for any other kind but NONE.  Of an id listed twice
 * the later entry counts.
 * sgo_set_graph_se2 resets every edge to what its phi says, NONE or DCS.  sgo_update_graph_se2 keeps the kinds of the edges
 * [0, n_resident_edges) whichever way it takes -- as an overlay the resident prefix is not re-read; on a full set-up the context
 * applies the kinds it remembers to those ids, with delta = the phi passed (an edge passed with phi < 0 has no kernel, an edge
 * remembered as NONE keeps none) --, and appended edges start as NONE or DCS. */
int sgo_set_robust_kernels(sgo_ctx* ctx, int32_t n, const int32_t* edge_ids, const int32_t* kind, const double* delta);

/* Replaces: RobustKernel::robustify on every edge after computeActiveErrors().  rho0[E], weight[E] (either may be NULL) in the
 * edge order of sgo_edge_chi2, at the current poses and with its arithmetic: the weight is DCS's switch value s^2, or any
 * kernel's outlier score of a closure (1 = inlier, towards 0 = discounted).  Covers overlay edges; works while an overlay
 * is resident. */
int sgo_edge_robust(sgo_ctx* ctx, double* rho0, double* weight);

/* Replaces: the covariance producer of a loop closure and its use as the edge information
 * (src/sparse_gslam/src/cartographer_bindings/fast_correlative_scan_matcher_2d.cc:537-561,
 * submap_loop_closer.cpp:276), batched: for match q the scores of the
 * (2 w + 1) x (2 w + 1) x (2 scan_window + 1) window around the best candidate, in the reference's
 * loop order (x offset i outermost, y offset j, scan index k fastest), give
 *     x(i,j,k) = (-j res, -i res, (k - num_angular_perturbations) angular_step)
 *                 (include/cartographer_bindings/correlative_scan_matcher_2d.h:78-82)
 *     K = sum score x x^T, u = sum score x, s = sum score,   cov = K / s - u u^T / s^2,
 * and information = cov^-1 (3x3 row-major, cofactors / determinant as Eigen's fixed-size inverse).
 * A window with s == 0 or a singular covariance yields non-finite entries, as the reference's
 * arithmetic does.  Needs no graph.  scores are addressed from win[q].score_offset. */
typedef struct sgo_match_window {
  int32_t x_index_offset;   /* best candidate (cells) */
  int32_t y_index_offset;
  int32_t scan_index;
  int32_t scan_window;      /* min(w, scan_index, n_scans - 1 - scan_index) at the call site */
  int32_t w_size;           /* 5 in the reference */
  int32_t num_angular_perturbations;
  double resolution;        /* SearchParameters::resolution */
  double angular_step;      /* SearchParameters::angular_perturbation_step_size */
  int64_t score_offset;     /* first score of this window in scores[] */
} sgo_match_window;
int sgo_closure_information(sgo_ctx* ctx, int32_t n, const sgo_match_window* win, const float* scores,
                            int64_t n_scores, double* cov /*[n][9]*/, double* info /*[n][9]*/);

/* ---- single-step entry points (what BlockSolver::buildSystem / solve expose inside g2o);
 *      used by the parity tests to check each kernel against the oracle. ---------------------- */
/* number of free (non-fixed, active) vertices n; hessian index h -> vertex id in free_ids[n] */
int sgo_num_free(sgo_ctx* ctx);
int sgo_free_ids(sgo_ctx* ctx, int32_t* free_ids);
/* buildSystem at the current poses: b[n][3], diag[n][9] (row-major 3x3), chi2 values. */
int sgo_linearize(sgo_ctx* ctx, double* b, double* diag, double* plain, double* robust);
/* y = H x with the Hessian of the last sgo_linearize (x, y: [n][3]). */
int sgo_hessian_apply(sgo_ctx* ctx, const double* x, double* y);
/* solve H x = b of the last sgo_linearize; returns PCG iterations (>= 0). */
int sgo_solve(sgo_ctx* ctx, double* x, double* relres);
/* z = M^-1 r with the configured preconditioner of the last sgo_linearize (r, z: [n][3]). */
int sgo_precondition(sgo_ctx* ctx, const double* r, double* z);
/* H x = b for the CALLER's right-hand side, with the Hessian of the last sgo_linearize. b, x: [n][3] in hessian order.
 * Same solver, tolerance (pcg_tol, relative to |b|), cold start and failure rules as sgo_solve; returns PCG iterations.
 * Refuses what sgo_solve refuses, and a null or non-finite b.  The linearisation's own right-hand side is untouched: a later
 * sgo_solve returns what it would have returned without this call. */
int sgo_solve_rhs(sgo_ctx* ctx, const double* b, double* x, double* relres);

/* Replaces: SparseOptimizer::computeMarginals(spinv, blockIndices).  For pair t the 3x3 block of H^-1 with the rows of
 * vertex vi[t] and the columns of vertex vj[t] (VERTEX ids, not hessian indices), row-major in cov[t][9].
 * H is the robustified Gauss-Newton Hessian at the CURRENT poses: the call linearises there itself (the weights of every kernel
 * kind; inactive edges add nothing).  g2o inverts the system of its last iteration, one update behind the estimates; this is the
 * system at the estimates the caller sees.
 * No factorisation: for every distinct FREE vertex among vj three unit right-hand sides are solved with the level-0 PCG machinery
 * of the single-step entry points, and the rows of the vi that were asked for are gathered on the device; the blocks cross to
 * the host once, at the end.  Cost: three solves per distinct column vertex -- the order of a pair is the caller's lever.  Each
 * solve is cold, at pcg_tol relative to its own right-hand side (no pcg_tol_cap, no soft cap), and the hierarchy's coarse
 * operators are refreshed once per call.  A graph on the single-launch direct path or the multifrontal path builds its row plan
 * and hierarchy on the first call, as sgo_linearize does, and stays on its path for sgo_optimize_gn.
 * A pair with a fixed vertex on either side yields the zero block (a fixed pose has no uncertainty; a fixed column vertex costs
 * no solve).  Blocks with vi == vj are symmetrised, (S + S^T) / 2; off-diagonal blocks come as solved.  A pair listed twice is
 * answered twice.
 * Returns the number of solves run, or a negative code.  A column that neither reached pcg_tol nor stands at the floating-point
 * floor of its system (sgo_stats.pcg_converged == 2's rule) fails the whole call: SGO_EINVAL, sgo_last_error names the vertex
 * and the relative residual, cov is left untouched.  Afterwards the context is linearised at the current poses, as after
 * sgo_linearize.
 * SGO_EINVAL, with nothing on the device changed: npairs < 0 or a null buffer, an id outside [0, V), a vertex that is not
 * active (it has no edge), an active overlay (as the single-step entry points), a multi-GPU context (sgo_debug_set_shard's
 * emulation included). */
int sgo_marginals(sgo_ctx* ctx, int32_t npairs, const int32_t* vi, const int32_t* vj, double* cov);

/* The covariance of EVERY pose, and of pairs of poses that share a front, by selected inversion of the multifrontal Cholesky
 * factor (Takahashi's recurrence: a top-down pass over the elimination tree, about the arithmetic of one factorisation whatever
 * the number of blocks asked for).  H is the robustified Gauss-Newton Hessian at the CURRENT poses, exactly
 * as in sgo_marginals: the call assembles and factorises there itself (the weights of every kernel kind; inactive edges add nothing).
 * diag (NULL: not wanted): [V][9], the 3x3 block Sigma_vv of every vertex id, row-major, exactly symmetric (one triangle is
 *   computed, the other is its mirror); a fixed vertex and a vertex without an edge yield the zero block.
 * pairs: cov[t][9] = the block with the rows of vi[t] and the columns of vj[t].  A pair is answered when one front of the
 *   factorisation holds both poses -- always for vi == vj and for two free poses joined by an edge the graph was set up with
 *   (active or deactivated).  A pair with a fixed vertex is the zero block; a pair listed twice is answered twice; the block
 *   (vi, vj) is the transpose of (vj, vi) bit for bit.  A pair outside the pattern refuses the whole call (SGO_EINVAL, nothing
 *   written; sgo_last_error names the pair): such blocks are sgo_marginals' to compute.
 * The plan is the resident multifrontal one when sgo_optimize_gn takes that path.  A graph on the single-launch direct path or the
 * PCG gets a multifrontal plan of its own, analysed once per set-up under the multifrontal path's admission limits (SGO_MFRONT_*
 * of the environment included; SGO_MFRONT=0 only keeps optimize() off that path); sgo_optimize_gn keeps its path, and a later
 * call has the chi2 history and the poses, bit for bit, of a context that never made this call.  SGO_ENOTHING with the analysis'
 * reason in sgo_last_error when the analysis refuses the graph: use sgo_marginals then.
 * SGO_EINVAL, with nothing on the device changed: npairs < 0 or a null buffer where one is needed, an id outside [0, V), a pair
 * naming a vertex that is not active, an active overlay, a multi-GPU context (sgo_debug_set_shard's emulation included).
 * SGO_EINVAL with the outputs untouched when the factorisation is not positive definite; the next sgo_optimize_gn is unaffected.
 * Returns the number of fronts of the plan, or a negative code.  Two calls at the same poses give the same bits. */
int sgo_marginals_selected(sgo_ctx* ctx, double* diag, int32_t npairs, const int32_t* vi, const int32_t* vj, double* cov);

/* (later additions, version 107) Panels of right-hand sides through the multifrontal factor, and the innovation gate for candidate
 * closures built on them.
 *
 * H X = B for nrhs right-hand sides through the multifrontal Cholesky factor.  H: the robustified Gauss-Newton Hessian at the
 * CURRENT poses, as in sgo_marginals_selected (the call assembles and factorises there itself).  B, X: [nrhs][n][3], every
 * right-hand side contiguous, hessian order (sgo_free_ids), as sgo_solve_rhs's b and x.  X may alias B.
 * Forward and backward substitution run for 16 right-hand sides at a time on the fp64 matrix cores; long requests are processed
 * in chunks of 256.  A right-hand side's solution does not depend on nrhs or on which other columns share its panel, and two calls
 * at the same poses give the same bits.  The plan is sgo_marginals_selected's (the resident multifrontal one, or one analysed once
 * per set-up); sgo_optimize_gn keeps its path and a later call has the chi2 history and the poses, bit for bit, of a context that
 * never made this call.  SGO_ENOTHING with the analysis' reason in sgo_last_error when the analysis refuses the graph: use
 * sgo_solve_rhs then.
 * SGO_EINVAL, with nothing on the device changed and X untouched: nrhs < 0 or a null buffer, a non-finite entry of B, an active
 * overlay, a multi-GPU context (sgo_debug_set_shard's emulation included).  SGO_EINVAL with X untouched when the factorisation is
 * not positive definite; the next sgo_optimize_gn is unaffected.
 * Returns the number of fronts of the plan (0 for nrhs == 0 or a graph without a free pose), or a negative code. */
int sgo_factor_solve(sgo_ctx* ctx, int32_t nrhs, const double* B, double* X);

/* The innovation gate: is a candidate closure compatible with the current estimate AND its uncertainty, before it is inserted?
 * For candidate t -- an EdgeSE2 between vertices ci[t] and cj[t] with measurement meas[t][3] and information info[t][6] (upper
 * triangle by rows, as sgo_set_graph_se2's) that is NOT part of the graph --: e = its error at the current poses, A, B = its
 * Jacobians (EdgeSE2::linearizeOplus),
 *   cov_pred[t][9] = P = 1/2 (Q + Q^T),  Q = [A B] Sigma_{(i,j),(i,j)} [A B]^T   (a fixed endpoint drops out; both fixed: 0)
 *   d2[t] = e^T (Omega^-1 + P)^-1 e,   pass[t] = d2[t] <= chi2_max
 * with Sigma = H^-1 of sgo_marginals_selected's H.  No block of Sigma is formed: Q = R^T H^-1 R with A^T and B^T at the rows of the
 * two poses, three right-hand sides per candidate through sgo_factor_solve's substitution (the pair need not share a front, which
 * sgo_marginals_selected requires).  When the multifrontal analysis refuses the graph the same right-hand sides go through the
 * PCG machinery of sgo_solve_rhs under sgo_marginals' rules (cold, pcg_tol relative to each right-hand side's own norm, the floor
 * rule, one refresh of the coarse operators per call; a column that neither converges nor stands at the floor fails the call:
 * SGO_EINVAL, candidate and residual named, outputs untouched): the call answers on every single-GPU graph.
 * Returns how many pass, or a negative code.  The graph, the poses and every resident structure stay as they are; a candidate
 * listed twice is answered twice; two calls at the same poses give the same bits.
 * SGO_EINVAL, with nothing on the device changed and no output written: n < 0 or a null ci, cj, meas or info, a non-finite entry of
 * meas or info, chi2_max not finite, a vertex id outside [0, V), a vertex without an edge, ci[t] == cj[t], an information matrix
 * that is not symmetric positive definite (leading minors), an active overlay, a multi-GPU context.  SGO_EINVAL with the outputs
 * untouched when the Hessian is not positive definite; the next sgo_optimize_gn is unaffected. */
int sgo_candidate_gate(sgo_ctx* ctx, int32_t n, const int32_t* ci, const int32_t* cj, const double* meas, const double* info,
                       double chi2_max, double* d2 /*[n], may be NULL*/, double* cov_pred /*[n][9], may be NULL*/,
                       uint8_t* pass /*[n], may be NULL*/);

/* (later additions, version 107) Joint compatibility of a SET of candidate closures: sgo_candidate_gate
 * judges every candidate alone, but the innovations of a burst of candidates that cross the same drift are correlated.  For the n
 * stacked candidates (arguments as sgo_candidate_gate's), with R = their Jacobians' columns and H as there,
 *   S = blockdiag(Omega_t^-1) + 1/2 (G + G^T),   G = R^T H^-1 R   (3 n x 3 n),   e = (e_1 ... e_n)
 *   d2(s) = e_s^T (S_ss)^-1 e_s   for a subset s of the candidates: 3 |s| degrees of freedom.
 * The diagonal blocks are sgo_candidate_gate's Omega^-1 + P; the cross blocks G_st = [A_s B_s] (H^-1 R_t)[rows of i_s, j_s] come from
 * the same three columns per candidate (through the factor, or through the PCG where the analysis refuses the graph, under
 * sgo_candidate_gate's rules: a failing column fails the call, candidate and residual named), so the table costs the gate plus one
 * small product.  One triangle is computed and mirrored: S is exactly symmetric.  A fixed endpoint drops out of R; a candidate
 * between two fixed vertices has S_tt = Omega_t^-1 and zero cross blocks; a candidate listed twice is two rows of the table.
 *
 * sgo_candidate_joint builds the table at the CURRENT poses, copies S and e out where asked and keeps the table in the context.
 * Returns n.  The table is a SNAPSHOT: later changes of the poses (sgo_set_poses, sgo_optimize_gn) do not touch or invalidate it; it
 * lasts until the next successful sgo_candidate_joint, sgo_set_graph_se2, sgo_update_graph_se2 or sgo_destroy.  n == 0 drops the
 * table and returns 0.  Refusals are sgo_candidate_gate's (SGO_EINVAL, nothing on the device changed, no output written, a resident
 * table kept: n < 0 or a null ci, cj, meas or info, a non-finite entry, an id outside [0, V), a vertex without an edge,
 * ci[t] == cj[t], an information matrix that is not symmetric positive definite, an active overlay, a multi-GPU context) and
 * n > SGO_JOINT_MAX_CANDIDATES.  SGO_EINVAL with the outputs untouched and the resident table kept when the Hessian is not positive
 * definite; the next sgo_optimize_gn is unaffected.  Like sgo_candidate_gate the call writes only what every Gauss-Newton iteration
 * recomputes, and scratch: a later sgo_optimize_gn has the bits of a context that never called.
 *
 * sgo_joint_subsets evaluates B subsets of the resident table, one workgroup each (Cholesky of S_ss in LDS): subset[b][t] != 0
 * selects candidate t, the selected ones are taken in ascending t; d2[b] as above, dof[b] = 3 |s|, pass[b] = d2[b] <= chi2_max[b]
 * (the chi2 quantile for dof[b] is the caller's to look up).  Returns how many pass, 0 with chi2_max == NULL (no decisions; pass
 * is not written).  The empty subset gives 0 exactly; an S_ss that is not positive definite gives NaN, which does not pass.  d2[b]
 * depends on the table and the subset alone -- not on B, its place in the batch or the other subsets --, and two calls give the
 * same bits.  It touches no graph structure.  SGO_EINVAL, nothing written: no resident table, n not the table's n, B < 0, a null
 * subset or d2 with B > 0, a non-finite chi2_max entry, a subset of more than SGO_JOINT_MAX_SUBSET candidates (the subset is
 * named in sgo_last_error).  B == 0 returns 0.
 *
 * sgo_joint_pairs: d2 of every pair {s, t} by the same kernel, the index pairs made on the device; d2[s][t] == d2[t][s] bit for bit
 * (evaluated once, stored twice), the diagonal holds the single candidates' d2.  Returns n.  SGO_EINVAL: no resident table, n not
 * the table's n, a null d2. */
#define SGO_JOINT_MAX_CANDIDATES 256   /* S is 768 x 768 doubles = 4.7 MB */
#define SGO_JOINT_MAX_SUBSET 40        /* 120 rows: 120 x 121 doubles = 116 KB of LDS, one workgroup (160 KiB per CU) */
int sgo_candidate_joint(sgo_ctx* ctx, int32_t n, const int32_t* ci, const int32_t* cj, const double* meas, const double* info,
                        double* S /*[3n][3n] row-major, may be NULL*/, double* e /*[n][3], may be NULL*/);
int sgo_joint_subsets(sgo_ctx* ctx, int32_t n, int32_t B, const uint8_t* subset /*[B][n]*/, const double* chi2_max /*[B] or NULL*/,
                      double* d2 /*[B]*/, int32_t* dof /*[B] or NULL*/, uint8_t* pass /*[B] or NULL*/);
int sgo_joint_pairs(sgo_ctx* ctx, int32_t n, double* d2 /*[n][n]*/);

/* (later additions, version 107) Leave-one-out test of the edges ALREADY in the graph, all from one selected inversion (DESIGN.md
 * section 5k).  sgo_gate_edges compares the raw e^T Omega e, which is under-dispersed after the fit (its covariance is
 * Omega^-1 - J Sigma J^T, not Omega^-1) and changes meaning once a robust kernel down-weights the edge.  For resident edge k with
 * error e, Jacobians A, B (a fixed endpoint drops out), resident information Omega and kernel weight w (sgo_edge_robust's),
 * H and Sigma = H^-1 exactly sgo_marginals_selected's (the call assembles, factorises and selectively inverts at the CURRENT poses):
 *   P  = 1/2 (Q + Q^T),  Q = [A B] Sigma_{(i,j),(i,j)} [A B]^T                   (both endpoints fixed: P = 0)
 *   Omega = G G^T (lower Cholesky),  N = G^T P G = V diag(nu) V^T,  c = V^T G^T e
 *   redundancy[t] = 1 - w nu_max                          (lambda_min of I - w N, in [0, 1] up to rounding)
 *   d2[t]         = sum_q c_q^2 / ((1 + (1 - w) nu_q) (1 - w nu_q))
 *   cov_loo[t]    = G^-T V diag(nu_q / (1 - w nu_q)) V^T G^-1                    (row-major, exactly symmetric)
 * d2 is e~^T (Omega^-1 + P_)^-1 e~ with P_ = J H_^-1 J^T the predicted covariance of the graph WITHOUT the edge (H_ = H - J^T (w Omega) J),
 * = cov_loo, and e~ the edge's error after the one linear step its removal causes: what sgo_candidate_gate would say about the edge
 * had it never been inserted.  w = 1 gives the normalised-residual test e^T (Omega^-1 - P)^-1 e, w = 0 the gate's own formula.
 * An edge with all-zero information (deactivated): d2 = 0, redundancy = 1, cov_loo = P, no fail.  An information that is not
 * positive definite: d2 = redundancy = NaN, no fail.  A BRIDGE edge (its removal disconnects the graph: the odometry tail, a chain
 * stretch inside no loop) has redundancy 0 up to rounding and the test is 0 / 0: whenever redundancy < min_redundancy or is not finite,
 * d2 and cov_loo are NaN, redundancy is reported as computed and the edge does not fail.
 * fail[t] = redundancy >= min_redundancy && d2 > chi2_max; returns how many fail, or a negative code.  edge_ids == NULL: edges
 * 0 .. n-1.  An edge's result does not depend on n or on its place in the list, an id listed twice is answered twice, two calls at
 * the same poses give the same bits.  Nothing of Sigma crosses to the host: one kernel reads the 21 doubles per edge in place.
 * The plan is sgo_marginals_selected's, whose factor and selected-inversion launches the call shares; like that call it writes only
 * what every Gauss-Newton iteration recomputes, and scratch: a later sgo_optimize_gn has the bits of a context that never called.
 * SGO_ENOTHING with the analysis' reason when the multifrontal analysis refuses the graph: use sgo_optimize_gn_hypotheses (one
 * hypothesis per edge) then.
 * SGO_EINVAL, with nothing on the device changed and no output written: n < 0 or a null d2 (n > E without ids), an id outside
 * [0, E), chi2_max not finite, min_redundancy outside (0, 1] (zero is refused so that a bridge's 0 / 0 can never decide), an active
 * overlay, a multi-GPU context (sgo_debug_set_shard's emulation included).  SGO_EINVAL with the outputs untouched when the
 * factorisation is not positive definite; the next sgo_optimize_gn is unaffected.
 * Groups of edges (several wrong closures that vouch for each other) are sgo_edge_joint / sgo_edge_groups' below.  Not covered:
 * deactivation inside the call (sgo_set_edge_information).
 *
 * sgo_edge_loo_rule: the per-edge arithmetic alone, as the kernel compiles it (sgo_rules.h; no context, no GPU, like sgo_gain_stop):
 * info6 = Omega's upper triangle by rows, P9 row-major, e3, w -> d2, redundancy, cov_loo (may be NULL); no min_redundancy is applied.
 * Returns 0, 1 for an all-zero information, 2 for an information that is not positive definite. */
int sgo_edge_leave_one_out(sgo_ctx* ctx, int32_t n, const int32_t* edge_ids /*NULL: edges 0..n-1*/, double chi2_max,
                           double min_redundancy, double* d2 /*[n]*/, double* redundancy /*[n], may be NULL*/,
                           double* cov_loo /*[n][9], may be NULL*/, uint8_t* fail /*[n], may be NULL*/);
int sgo_edge_loo_rule(const double* info6, const double* P9, const double* e3, double w, double* d2, double* redundancy,
                      double* cov_loo /*[9] or NULL*/);

/* (later additions, version 107) Leave-GROUP-out test of clusters of resident edges on a joint table.
 * Closures arrive in bursts: several matches against the same submap are wrong together and vouch for each other, which the
 * single-edge test above cannot see.  A group g of k resident edges at the current poses, stacked: e (3 k), J the Jacobian rows (a
 * fixed endpoint drops out), Omega = blockdiag(Omega_t) the resident information, w_t the kernel weights (sgo_edge_robust's),
 * D = blockdiag(w_t I3), H sgo_marginals_selected's robustified Hessian, N = 1/2 (Q + Q^T) with Q = J H^-1 J^T.  With
 * Omega_t = G_t G_t^T (lower Cholesky), G = blockdiag(G_t), Nt = G^T N G, c = G^T e, T = D^1/2:
 *   K     = I + Nt - D Nt - Nt D - Nt D (I - D) Nt        (symmetric)
 *   d2    = c^T K^-1 c,   dof = 3 k
 *   pivot = the smallest squared diagonal entry of the Cholesky factor of I - T Nt T
 * d2 is e~^T (Omega^-1 + P_)^-1 e~ with H_ = H - J^T (D Omega) J, P_ = J H_^-1 J^T and e~ = e + J H_^-1 J^T D Omega e:
 * sgo_edge_leave_one_out's definition with a group in the edge's place, what sgo_joint_subsets would say about the cluster had it
 * never been inserted.  k = 1 is that call's closed form, w = 1 gives K = I - Nt, w = 0 gives K = I + Nt (the joint test's S).  pivot
 * lies in [0, 1], bounds lambda_min(I - T Nt T) from above and is 0 up to rounding exactly when removing the group disconnects the graph.
 * A member with all-zero information is dropped from its group and adds nothing to dof; an information that is not positive
 * definite gives d2 = pivot = NaN, no fail; the empty group gives d2 = 0 exactly, dof = 0, pivot = 1.  Whenever pivot is not finite
 * or pivot < min_pivot, d2 is NaN, pivot is reported as computed and the group does not fail.  Otherwise fail = d2 > chi2_max[b].
 *
 * sgo_edge_joint builds the table of the n <= SGO_JOINT_MAX_CANDIDATES listed resident edges at the CURRENT poses -- N, e, w and the
 * resident Omega --, copies N, e and w out where asked and keeps the table in the context.  Returns n.  The columns H^-1 J^T are
 * sgo_candidate_joint's (through the factor, or through the PCG where the analysis refuses the graph, under its rules); the
 * per-edge records are filled on the device from the resident edge list, no edge data crosses to the host.  One triangle of N is
 * computed and mirrored: N is exactly symmetric.  The table is a SNAPSHOT with the lifetime of the candidates' table (until the
 * next successful sgo_edge_joint, sgo_set_graph_se2, sgo_update_graph_se2 or sgo_destroy; n == 0 drops it and returns 0), and it is
 * a SECOND table: neither sgo_edge_joint nor sgo_candidate_joint drops or changes the other's.  SGO_EINVAL with nothing on the
 * device changed, no output written and the resident tables kept: n < 0, null edge_ids with n > 0, n > SGO_JOINT_MAX_CANDIDATES, an
 * id outside [0, E), an id listed twice (removing an edge twice has no meaning), an active overlay, a multi-GPU context; with the
 * outputs untouched and the tables kept when the Hessian is not positive definite.
 *
 * sgo_edge_groups evaluates B groups of the resident table, one workgroup each: member[b][t] != 0 puts table row t into group b,
 * members are taken in ascending t, at most SGO_JOINT_MAX_SUBSET per group.  Returns how many fail, 0 with chi2_max == NULL (no
 * decisions; fail is not written).  A group's result depends on the table and its member row alone -- not on B or its place in
 * the batch --, and two calls give the same bits.  SGO_EINVAL, nothing written: no resident table, n not the table's n, B < 0, a
 * null member or d2 with B > 0, a non-finite chi2_max entry, min_pivot outside (0, 1], a group above the cap (named in
 * sgo_last_error).  B == 0 returns 0.
 * Both calls write only scratch and what every Gauss-Newton iteration recomputes: a later sgo_optimize_gn has the bits of a context
 * that never called, and sgo_joint_subsets returns the bits it returned before.
 *
 * sgo_edge_group_rule: one group's arithmetic alone, as the kernel compiles it (sgo_rules.h; no context, no GPU, like
 * sgo_edge_loo_rule): the k members' info6 (Omega's upper triangle by rows), N (3 k x 3 k row-major), e, w -> d2, pivot, dof; no
 * min_pivot is applied (d2 is NaN only where pivot is not above zero or K is not positive definite).  Returns 0, 1 when a member
 * with all-zero information was dropped, 2 when pivot is NaN (an information that is not positive definite), SGO_EINVAL for
 * k outside [0, SGO_JOINT_MAX_SUBSET] or a null argument. */
int sgo_edge_joint(sgo_ctx* ctx, int32_t n, const int32_t* edge_ids, double* N /*[3n][3n] or NULL*/, double* e /*[n][3] or NULL*/,
                   double* w /*[n] or NULL*/);
int sgo_edge_groups(sgo_ctx* ctx, int32_t n, int32_t B, const uint8_t* member /*[B][n]*/, const double* chi2_max /*[B] or NULL*/,
                    double min_pivot, double* d2 /*[B]*/, int32_t* dof /*[B] or NULL*/, double* pivot /*[B] or NULL*/,
                    uint8_t* fail /*[B] or NULL*/);
int sgo_edge_group_rule(int32_t k, const double* info6 /*[k][6]*/, const double* N /*[3k][3k]*/, const double* e /*[3k]*/,
                        const double* w /*[k]*/, double* d2, double* pivot, int32_t* dof);

/* (later additions, version 107) Covariance-aware closure search: all listed poses against each query pose, from one selected
 * inversion and one panel solve per 85 queries.  The step BEFORE a match exists: which poses are worth
 * matching against the query pose at all, and with what search window.  A fixed Euclidean threshold on the current estimates
 * misses true revisits after a long loop (drift) and a fixed matcher window is far wider than needed right after a closure.
 * Per query vertex c and listed vertex j at the CURRENT poses, with H and Sigma = H^-1 exactly sgo_marginals_selected's (the call
 * assembles, factorises and selectively inverts itself):
 *   rel      = (t, phi), t = R(theta_j)^T (p_c - p_j), phi = normalize(theta_c - theta_j): the pose of c in j's frame, EdgeSE2's
 *              prediction for an edge j -> c (the matcher searches in the submap's frame)
 *   A, B     = d rel / d x_j, d rel / d x_c: the Jacobians of an EdgeSE2 j -> c at the measurement whose rotation is the identity, so
 *              that P is the covariance of rel itself in j's frame (the edge whose measurement is rel has R(-phi) P R(-phi)^T:
 *              the same m2 and sigma)
 *   cov_rel  = P = 1/2 (Q + Q^T), Q = A Sigma_jj A^T + A Sigma_jc B^T + B Sigma_cj A^T + B Sigma_cc B^T   (row-major, exactly
 *              symmetric; a fixed endpoint drops out; both fixed: P = 0)
 *   m2       = max(0, |t| - radius)^2 / (u^T P_tt u), u = t / |t|: the squared Mahalanobis distance from the relative translation
 *              to the half-plane {y : u^T y <= radius}.  The half-plane contains the disc |y| <= radius (u^T y <= |y|), so m2 is a
 *              lower bound of the distance to the disc: a pose the exact disc test would keep is never dropped.  1 degree of
 *              freedom.  A zero excess gives m2 = 0 whatever the denominator, a positive excess over a zero denominator +inf.
 *   sigma    = (sqrt(lambda_max(P_tt)), sqrt(P_phiphi)): the 1-sigma linear and angular half-widths of the matcher's window in j's
 *              frame; the caller scales them
 *   near     = m2 <= chi2_max && j != c && |j - c| >= min_sep
 * j == c gives rel = 0, P = 0, m2 = 0, sigma = 0, near = 0.  ids == NULL: vertices 0 .. n-1, of which one without an edge gives NaN
 * everywhere and near = 0.  Returns the number of near pairs, or a negative code.  nq == 0 or n == 0 returns 0.
 * An answer does not depend on nq, n, the pair's place in either list or on which queries share a panel; an id or a query listed
 * twice is answered twice; two calls at the same poses give the same bits.  Nothing of Sigma crosses to the host: Sigma_jj and
 * Sigma_cc are read in place in the selected inverse, Sigma_jc for all j is the three columns H^-1 E_c of sgo_factor_solve's
 * substitution through the same factorisation.  A fixed query costs no solve.  The plan is sgo_marginals_selected's (a graph on the
 * direct path or the PCG gets one of its own); like that call this one writes only what every Gauss-Newton iteration recomputes,
 * and scratch: a later sgo_optimize_gn has the bits of a context that never called.
 * SGO_ENOTHING with the analysis' reason when the multifrontal analysis refuses the graph (there is no cheap Sigma_jj of every pose
 * without a factor): gate a Euclidean shortlist with sgo_candidate_gate then.
 * SGO_EINVAL, with nothing on the device changed and no output written: negative counts, a null query, a null m2 with nq n > 0,
 * n > V without ids, an id or a query outside [0, V), a listed id or a query without an edge, radius negative or not finite,
 * chi2_max not finite, min_sep < 0, an active overlay, a multi-GPU context (sgo_debug_set_shard's emulation included).
 * SGO_EINVAL with the outputs untouched when the factorisation is not positive definite; the next sgo_optimize_gn is unaffected.
 *
 * sgo_closure_search_rule: one pair's arithmetic alone, as the kernel compiles it (sgo_rules.h; no context, no GPU, like
 * sgo_edge_loo_rule): the poses xj, xc and the blocks Sjj, Sjc (the rows of j), Scc of Sigma, row-major; a NULL Sjj or Scc stands
 * for a FIXED pose, which drops out with the cross block (Sjc may be NULL then).  rel [3], cov_rel [9] and sigma [2] may be NULL.
 * No special case for j == c.  Returns 0, SGO_EINVAL for a null xj, xc or m2 or a null Sjc between two free poses. */
int sgo_closure_search(sgo_ctx* ctx, int32_t nq, const int32_t* query /*[nq] vertex ids*/,
                       int32_t n, const int32_t* ids /*NULL: vertices 0..n-1*/,
                       double radius, double chi2_max, int32_t min_sep,
                       double* m2 /*[nq][n]*/, double* rel /*[nq][n][3] or NULL*/, double* cov_rel /*[nq][n][9] or NULL*/,
                       double* sigma /*[nq][n][2] or NULL*/, uint8_t* near /*[nq][n] or NULL*/);
int sgo_closure_search_rule(const double xj[3], const double xc[3], const double Sjj[9], const double Sjc[9], const double Scc[9],
                            double radius, double* rel, double* cov_rel, double* m2, double* sigma);   /* pure, no GPU */

/* (later additions, version 107) Greedy search for a large jointly compatible set on the resident table of sgo_candidate_joint
 * (DESIGN.md section 5l): "which of these candidates form the largest consistent set?" without a from-scratch factorisation per
 * extension.  Growing a subset by one candidate is one step of a block-pivoted Cholesky of S.  After the ordered pivots t_1 .. t_k
 * (m = 3 k rows) every candidate c holds W_c (m x 3), C_c = S_cc - W_c^T W_c and q_c = e_c - W_c^T z; z (m) and d2 = z^T z are the set's.
 *   extension value  v_c = d2 + q_c^T C_c^-1 q_c by a 3 x 3 lower Cholesky of C_c: the d2 of the set with c added.  NaN where C_c is
 *                    not positive definite; d2 itself, bit for bit, for a c that is a pivot already.
 *   pivot step p     G = chol(C_p), z+ = G^-1 q_p; for every c that is not a pivot w = G^-1 (S_pc - W_p^T W_c), C_c -= w^T w,
 *                    q_c -= w^T z+, w appended to W_c; d2 += z+^T z+.  Every sum runs in ascending row order.
 *   greedy rule      at count k < max_len the candidates that are not pivots, have allow[c] != 0 and a finite v_c <= chi2_max[k + 1]
 *                    are eligible; the smallest v_c is chosen, ties go to the lowest c; none eligible: the search stops.
 * sgo_joint_greedy runs B searches in one call, one workgroup each.  seed[b]: the candidates forced in, in this order, -1 padded; they are
 * never tested against chi2_max.  Outputs: order[b] = the seed, then the chosen candidates, then -1; count[b]; stop[b] (SGO_JSTOP_*);
 * d2_path[b][k] = d2 after k pivots ([0] = 0, NaN behind count); d2_ext[b][c] = v_c at the final set (members: d2_path[b][count] bit for
 * bit).  A seed pivot whose block is not positive definite ends that seed alone: count = the pivots done before it, order holds those and
 * -1, SGO_JSTOP_NOT_PD, d2_ext and d2_path behind count NaN.  chi2_max == NULL: no growth (stop is SGO_JSTOP_MAX_LEN when the seed has
 * max_len candidates, else SGO_JSTOP_NONE).  Returns B.
 * sgo_joint_extend is sgo_joint_greedy without growth, the primitive of a caller's own branch-and-bound: d2[b] of list b (NaN where
 * a pivot block is not positive definite) and d2_ext[b][c], the d2 of the list with c added.
 * Bit for bit: a seed's results depend on the table, its seed, its allow row, chi2_max and max_len alone -- not on B, its place in the
 * batch or the slicing --; two calls agree; sgo_joint_extend on a returned order gives d2 == d2_path[count] and the same d2_ext.  The
 * calls read the table and write scratch of their own: a later sgo_optimize_gn has the bits of a context that never called, and
 * sgo_joint_subsets returns what it returned before.
 * SGO_EINVAL, nothing written, the table kept: no resident table or n not the table's; B < 0; a null seed, order or count (lists, d2,
 * d2_ext) with B > 0; a seed entry outside [0, n); a candidate listed twice in a seed; an entry after a -1; max_len outside [the longest
 * seed's length, SGO_JOINT_MAX_SUBSET]; a non-finite chi2_max[1 ..].  B == 0 returns 0.  SGO_ENOMEM when the scratch (at most 192 MiB:
 * B is cut into slices of at most 256 seeds) cannot be allocated; the context and the table stay intact.
 * sgo_joint_greedy_rule: one seed's search on the host through the same arithmetic text as the kernel (sgo_rules.h; no context, no GPU,
 * like sgo_edge_loo_rule): S (3 n x 3 n row-major), e (3 n), one seed row, one allow row.  Returns 1, or SGO_EINVAL as above. */
#define SGO_JSTOP_MAX_LEN 0   /* max_len candidates chosen */
#define SGO_JSTOP_NONE    1   /* no eligible candidate */
#define SGO_JSTOP_NOT_PD  2   /* a seed pivot's block was not positive definite */
int sgo_joint_greedy(sgo_ctx* ctx, int32_t n, int32_t B, const int32_t* seed /*[B][SGO_JOINT_MAX_SUBSET], -1 padded*/,
                     const uint8_t* allow /*[B][n] or NULL = all*/,
                     const double* chi2_max /*[SGO_JOINT_MAX_SUBSET+1] by count, [0] ignored; NULL = no growth*/, int32_t max_len,
                     int32_t* order /*[B][SGO_JOINT_MAX_SUBSET]*/, int32_t* count /*[B]*/, int32_t* stop /*[B] or NULL*/,
                     double* d2_path /*[B][SGO_JOINT_MAX_SUBSET+1] or NULL*/, double* d2_ext /*[B][n] or NULL*/);
int sgo_joint_extend(sgo_ctx* ctx, int32_t n, int32_t B, const int32_t* lists /*as seed*/, double* d2 /*[B]*/, double* d2_ext /*[B][n]*/);
int sgo_joint_greedy_rule(int32_t n, const double* S, const double* e, const int32_t* seed, const uint8_t* allow, const double* chi2_max,
                          int32_t max_len, int32_t* order, int32_t* count, int32_t* stop, double* d2_path, double* d2_ext);

/* ---- profiling (opts.profile = 1) ---------------------------------------------------------- */
/* Per-kernel totals accumulated since the last sgo_profile_reset: for kernel slot k,
 * name (static string), launches, total milliseconds (HIP events on the ctx stream), and the
 * algorithmic bytes those launches were specified to move.
 * Slots are named as rocprofv3 prints the kernel; the launches of the three block-stream kernels on the
 * finest multigrid level are kept in slots of their own, named "<kernel> @level0" (the same kernels'
 * coarse-level launches sit on the launch-latency floor and would blur the bandwidth figure).
 * Returns the number of slots; fills up to cap entries. */
typedef struct sgo_kernel_stat {
  const char* name;
  int64_t launches;
  double ms;
  double bytes;
} sgo_kernel_stat;
int sgo_kernel_profile(sgo_ctx* ctx, sgo_kernel_stat* out, int cap);
/* The single launches behind slot `slot` of sgo_kernel_profile (same order of slots): their durations in milliseconds, in
 * launch order, up to the first 16384 per slot since the last sgo_profile_reset -- for medians and percentiles (a mean hides
 * what a few outliers or early-exit launches do to it).  In profile mode the PCG loop checks the stop flag after every
 * iteration, so no launch past convergence is among them.  Returns the number of samples written (<= cap), < 0 on error. */
int sgo_kernel_profile_samples(sgo_ctx* ctx, int slot, float* out_ms, int cap);
int sgo_profile_reset(sgo_ctx* ctx);
/* Milliseconds an EMPTY event bracket measures on this context's stream: the upper bound of the
 * per-launch bias of sgo_kernel_profile's times relative to rocprofv3 kernel durations. */
double sgo_profile_overhead_ms(sgo_ctx* ctx);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ------------------------------------------
 * Every rank is given the SAME full graph (sgo_set_graph_se2 with identical arguments) and makes the same row plan: the
 * rows of the level-0 Hessian in Hilbert order of the poses, cut into 256 tiles per rank; rank r owns the contiguous range
 * of tiles sgo_shard_range(ntiles, nranks, r).  Two modes, chosen per graph (sgo_solver_description says which):
 *   row-owner mode  (at most a quarter of the rows have an edge into another rank's range -- spatially local closures): a rank
 *     holds the Hessian blocks and edge operands of ITS rows only and linearises, multiplies, smooths, restricts, prolongates and
 *     updates these rows; per PCG iteration it exchanges the boundary rows of two vectors and the partial sums of the dot
 *     products (fixed-size all-gather packets, reduced in rank order: bit-identical scalars on all ranks) and all-reduces the
 *     coarse right-hand side; per Gauss-Newton iteration the boundary rows of the smoothed prolongator and the step (for the
 *     replicated pose update) travel, and the level-1 Galerkin blocks are all-reduced.  The coarse multigrid levels run replicated.
 *   all-reduce mode (random long-range closures: most rows are boundary rows): every rank holds the whole graph, evaluates every
 *     level-0 Hessian product of the solve for the rows of its tiles only, zeros elsewhere, and the product vector is summed over
 *     ranks with ncclAllReduce (one non-zero contributor per row: the sum is exact) -- the per-PCG-step exchange BASELINE.json's
 *     north_star names.  Linearisation, coarse levels and vector recurrences run replicated on bit-identical data.
 * chi2 is summed over edge ranges in both.  Every rank takes the same decisions (stopping, hierarchy rebuilds) from
 * bit-identical scalars. */
/* 128-byte unique id for rendezvous (wraps ncclGetUniqueId); rank 0 creates it, the host layer
 * broadcasts it (torch.distributed / MPI / a file), every rank passes it to sgo_comm_init. */
#define SGO_UNIQUE_ID_BYTES 128
int sgo_comm_unique_id(void* id_out);
int sgo_comm_init(sgo_ctx* ctx, int nranks, int rank, const void* unique_id);
int sgo_comm_size(sgo_ctx* ctx);
/* The same multi-GPU mode over a transport the CALLER brings (MPI, gloo, a socket layer) instead of RCCL: every
 * collective copies its vector to pinned host memory, calls `fn` -- which must replace buf[0..count) by its sum
 * over all ranks, bit-identical on every rank, and return 0 -- and copies the result back.  For nodes without
 * xGMI / RCCL and for multi-process tests on one GPU; slower than sgo_comm_init.  `fn` is called on the thread
 * that called into the library.  Must precede sgo_set_graph_se2. */
typedef int (*sgo_host_allreduce_fn)(double* buf, size_t count, void* user);
int sgo_comm_init_host(sgo_ctx* ctx, int nranks, int rank, sgo_host_allreduce_fn fn, void* user);
/* Optional companion of sgo_comm_init_host for the row-owner mode's packets: recv[r * count .. (r + 1) * count) = rank r's
 * send[0 .. count) (host memory), return 0.  Without it libsgo performs an all-gather as an all-reduce of zero-padded slots
 * through `fn` (exact, nranks times the bytes).  Call after sgo_comm_init_host, before sgo_set_graph_se2. */
typedef int (*sgo_host_allgather_fn)(const double* send, size_t count, double* recv, void* user);
int sgo_comm_host_allgather(sgo_ctx* ctx, sgo_host_allgather_fn fn);
/* The contiguous range [begin, end) of `count` work units (tiles, edges) that rank `rank` of
 * `nranks` evaluates.  Pure function (no GPU needed); exposed so the host layer and the CPU tests
 * can reproduce the partition. */
void sgo_shard_range(int32_t count, int32_t nranks, int32_t rank, int32_t* begin, int32_t* end);
/* The row plan sgo_set_graph_se2 makes for a graph, computed on the host alone (no GPU, no context): the
 * number of free active vertices n, the vertex id of every internal row (row_vertex[n], Hilbert order), the
 * tiles (tile_row_begin[ntiles + 1], capacity tile_cap) and the first row of every rank's tile range
 * (rank_row_begin[nranks + 1]).  Output pointers may be NULL.  Lets multi-process callers and the CPU tests
 * see which rows of a level-0 product each rank contributes.  meas (as sgo_set_graph_se2's; may be NULL): with it the plan is
 * also the one sgo_set_graph_se2 makes for a graph whose initial poses contradict its closures -- a dead-reckoned start --,
 * whose rows are ordered by spanning-tree positions instead of the poses (0.1.6).  Exception: a graph sgo_set_graph_se2 puts
 * on a factorisation path (single-launch direct, multifrontal: <= 12 288 free poses) has no level-0 row plan at set-up; the first
 * single-step entry point (sgo_linearize, ...) makes one from the poses CURRENT at that moment in plain Hilbert order, which this
 * function reproduces when given those poses and meas = NULL.  (The trailing `meas` argument was ADDED in 0.1.6: a caller built
 * against an older header must be rebuilt -- SGO_VERSION / sgo_version() is the check.) */
int sgo_plan_rows(int32_t V, const double* poses, const uint8_t* fixed, int32_t E, const int32_t* ei, const int32_t* ej,
                  int32_t nranks, int32_t* n_free, int32_t* row_vertex, int32_t* ntiles, int32_t* tile_row_begin,
                  int32_t tile_cap, int32_t* rank_row_begin, const double* meas);
/* The elimination plan of the multifrontal path (mid-size graphs: DESIGN.md section 5c), computed on the host alone (no GPU,
 * no context).  stats[12] = { free poses, fronts, levels, largest front (scalar rows), its own poses, its boundary poses,
 * flops per factorisation, flops on the critical path (largest front of every level), 16-column panels on the critical path,
 * bytes of frontal matrices, row order (0 Hilbert, 1 id), assembly targets }; elim_vertex[n] (optional): vertex id at every
 * elimination position; front_of_elim[n] (optional): its front (fronts are numbered children-first).  leaf <= 0 and
 * max_crit_mflop <= 0 take the defaults of sgo_set_graph_se2.  SGO_ENOTHING: the graph does not qualify (sgo_last_error
 * says why; stats[0] is still set). */
int sgo_mfront_plan(int32_t V, const double* poses, const uint8_t* fixed, int32_t E, const int32_t* ei, const int32_t* ej,
                    int32_t leaf, double max_crit_mflop, int64_t* stats, int32_t* elim_vertex, int32_t* front_of_elim);

/* Test hook: make this context evaluate the tile range of rank `rank` of `nranks` WITHOUT a
 * communicator (collectives are skipped), so that the per-rank partial products can be inspected on
 * a single GPU: summing sgo_hessian_apply's result over rank = 0..nranks-1 must reproduce the
 * single-rank product exactly.  Must precede sgo_set_graph_se2. */
int sgo_debug_set_shard(sgo_ctx* ctx, int nranks, int rank);

/* Further test / measurement hooks (no g2o counterpart).
 * sgo_debug_coarse_rhs: the coarse right-hand side the first half of a multigrid cycle makes from r ([n][3], hessian
 *   order): first sweep from zero, level-0 residual pass, restriction; under sgo_debug_set_shard this rank's partial
 *   (the partials of all ranks sum to the single-rank vector: the cycle's small all-reduce).  Returns its length,
 *   0 without a multi-level hierarchy.  Requires sgo_linearize.
 * sgo_debug_spmv0_us: mean microseconds of `reps` back-to-back launches of the level-0 Hessian product kernel on the
 *   resident graph (mode 0 = H x, 1 = residual, 2 = Jacobi sweep); variant 16 selects the wave-group kernel,
 *   variant 32 prints per-phase cycle stamps of the tile kernel. */
int sgo_debug_coarse_rhs(sgo_ctx* ctx, const double* r, double* out, int cap);
/* Device bytes of the level-0 structure THIS rank holds for the resident graph (Hessian blocks, per-slot edge operands,
 * per-slot / per-block index arrays, level-0 transfer blocks and product lists): proportional to 1 / nranks in row-owner mode. */
int64_t sgo_debug_level0_bytes(sgo_ctx* ctx);
double sgo_debug_spmv0_us(sgo_ctx* ctx, int mode, int variant, int reps);
/* Test hook: a read-only copy of one array of the resident multigrid hierarchy, exactly as the next sgo_precondition (the
 * cycle) and the next refresh of the coarse operators read it -- device memory as stored, nothing recomputed; the one gather
 * is SGO_AMG_A_BLK, a level's logical 3x3 blocks [nslot][9] (level 0: through its references into the symmetric storage;
 * SGO_AMG_A_BLK_F32: the same with the off-diagonal blocks from the fp32 copy, where the cycle's level-0 passes read that).
 * Rows are in the internal order: SGO_AMG_ROW_ORDER (level 0) gives the internal row of every hessian-order row.
 * `what` is one of SGO_AMG_*; tests/amg_reference.py names every array's type and shape.  The streamed fp32 copies
 * (P_RBLK, P_TBLK, PS_RBLK, PS_TBLK) come as stored: components 0..3 [m][4], components 4..7 [m][4], component 8 [m].
 * SGO_AMG_INFO: SGO_AMG_INFO_COUNT doubles { n, nslot, nc, smoothed, filtered, folded, cycle form (0 unfolded, 1 folded,
 * 2 folded in two sweeps), sweeps per side, omega, omega_p, entries of P, of A P, products of P's values, of A P, of
 * P^T A P, levels, level-0 passes read fp32, N, Np of the coarsest inverse, long columns of P, of P~, K-cycle depth,
 * theta_filter, slots of the next level, fcg2_depth (levels <= it take two flexible-CG steps under the K-cycle) }.
 * SGO_AMG_W_*: the cycle's work vectors [n][3] as the last sgo_precondition left them -- XS, RS, TR (smoother state and its two
 * residual buffers; every level), and on the levels >= 1 BK, XK, Z1, Q, BK2, Z2, P2, Q2 (the flexible-CG steps of fcg(), sgo_amg.hip),
 * the partial-sum buffers PA = (z1.q | z1.bk), PB = (p2.q2 | p2.bk2), PC = (q.z2 | unused) as [2][2048] doubles, and GRIDS: three
 * int32 { gA, gB, gC }, how many entries of each half their consumers reduce (0: that step did not run on this level; entries
 * beyond are never read).  A level >= 2 is visited more than once per cycle: the arrays are those of its LAST visit, which is
 * self-consistent -- every level's last visit lies inside its parent's last visit, so the exported residual of level l (RS, or TR
 * after two pre-smoothing sweeps) is what BK of level l + 1 was restricted from, and the exported Z1 / P2 (or XK) of level l + 1
 * are what level l's last post-smoothing launch prolongated.
 * Returns the array's size in bytes (copied when cap_bytes suffices), 0 when the level has no such array, < 0 on error.
 * Requires sgo_linearize; refuses the row-owner mode and an active overlay, as sgo_debug_coarse_rhs does. */
#define SGO_AMG_INFO 0
#define SGO_AMG_A_ROWPTR 1
#define SGO_AMG_A_COL 2
#define SGO_AMG_A_BLK 3
#define SGO_AMG_A_BLK_F32 4
#define SGO_AMG_A_DINV 5
#define SGO_AMG_POS 6
#define SGO_AMG_D 7
#define SGO_AMG_AGG 8
#define SGO_AMG_MEM_PTR 9
#define SGO_AMG_MEM 10
#define SGO_AMG_P_ROWPTR 11
#define SGO_AMG_P_ROW 12
#define SGO_AMG_P_COL 13
#define SGO_AMG_P_BLK 14
#define SGO_AMG_P_RBLK 15
#define SGO_AMG_P_TBLK 16
#define SGO_AMG_P_TPOS 17
#define SGO_AMG_P_TROW 18
#define SGO_AMG_P_TCOL 19
#define SGO_AMG_STRONG 20
#define SGO_AMG_DF 21
#define SGO_AMG_DINVF 22
#define SGO_AMG_AP_A 23
#define SGO_AMG_AP_B 24
#define SGO_AMG_AP_TGT 25
#define SGO_AMG_AP_BLK 26
#define SGO_AMG_PS_ROW 27
#define SGO_AMG_PS_COL 28
#define SGO_AMG_PS_RBLK 29
#define SGO_AMG_PS_TBLK 30
#define SGO_AMG_PS_TROW 31
#define SGO_AMG_PS_TCOL 32
#define SGO_AMG_PS_STPOS 33
#define SGO_AMG_INV 34
#define SGO_AMG_ROW_ORDER 35
#define SGO_AMG_W_XS 36
#define SGO_AMG_W_RS 37
#define SGO_AMG_W_TR 38
#define SGO_AMG_W_BK 39
#define SGO_AMG_W_XK 40
#define SGO_AMG_W_Z1 41
#define SGO_AMG_W_Q 42
#define SGO_AMG_W_BK2 43
#define SGO_AMG_W_Z2 44
#define SGO_AMG_W_P2 45
#define SGO_AMG_W_Q2 46
#define SGO_AMG_W_PA 47
#define SGO_AMG_W_PB 48
#define SGO_AMG_W_PC 49
#define SGO_AMG_W_GRIDS 50
#define SGO_AMG_INFO_COUNT 25
int64_t sgo_debug_amg_array(sgo_ctx* ctx, int32_t level, int32_t what, void* out, int64_t cap_bytes);
/* Test hooks for the incremental overlay (sgo_update_graph_se2; tests/overlay_reference.py names every array's type and shape).
 * All three return SGO_EINVAL when no overlay is resident and in a multi-GPU context; the single-step entry points above keep
 * refusing an overlay.
 * sgo_debug_overlay_array: a read-only copy of one array of the resident overlay as of the last linearisation -- device memory
 *   as stored, nothing recomputed, sizes from the device's own header.  Same convention as sgo_debug_amg_array: returns the
 *   array's size in bytes (0: it has no entries) and copies it when cap_bytes holds it.  `what` is one of SGO_OV_*: HDR = int32
 *   { chain rows k, touched rows nt, right-hand-side columns ncol = 3 (nt + nx) + 1, nnz, hub rows nx }; RP [k + nt + nx + 1],
 *   ENT_EDGE / ENT_OTHER (int32) and ENT_SIDE (uint8) per entry; VTX [k + nx], TROW [nt] (internal rows), NZ [nnz] (int32);
 *   doubles: DN [k][6], UN [k][9], H0 and Y [3 k][ncol], SINV [k][6], M0 and S [3 nk][3 nk] (nk = nt + nx), BT and GK [3 nk],
 *   WX [3 nx][3 nt + 1], M [3 nt][3 nt].  XT is the one gather: the 3 nt entries of the last solve's step at the touched rows.
 * sgo_debug_overlay_linearize: linearises the resident graph WITH its overlay at the current poses, as every Gauss-Newton
 *   iteration of sgo_optimize_gn does, and returns the resident rows' right-hand side b[n][3] in the hessian order of the
 *   resident free poses (ascending vertex id: what sgo_free_ids gave before the update).
 * sgo_debug_overlay_apply: y = H_base x + U M U^T x for x[n][3] (same order) through the PCG iteration's own product with its
 *   dot product on; *dot = the sum of the partial sums the recurrence reads as p.q.  Needs sgo_debug_overlay_linearize first. */
#define SGO_OV_HDR 0
#define SGO_OV_RP 1
#define SGO_OV_ENT_EDGE 2
#define SGO_OV_ENT_OTHER 3
#define SGO_OV_ENT_SIDE 4
#define SGO_OV_VTX 5
#define SGO_OV_TROW 6
#define SGO_OV_NZ 7
#define SGO_OV_DN 8
#define SGO_OV_UN 9
#define SGO_OV_H0 10
#define SGO_OV_Y 11
#define SGO_OV_SINV 12
#define SGO_OV_M0 13
#define SGO_OV_BT 14
#define SGO_OV_S 15
#define SGO_OV_GK 16
#define SGO_OV_WX 17
#define SGO_OV_M 18
#define SGO_OV_XT 19
int64_t sgo_debug_overlay_array(sgo_ctx* ctx, int32_t what, void* out, int64_t cap_bytes);
int sgo_debug_overlay_linearize(sgo_ctx* ctx, double* b);
int sgo_debug_overlay_apply(sgo_ctx* ctx, const double* x, double* y, double* dot);

/* Test hooks for the multifrontal path (mid-size graphs: DESIGN.md section 5c; tests/mfront_reference.py checks every stage of
 * one Gauss-Newton iteration from these arrays).
 * sgo_debug_mfront_array: a read-only copy of one array of the resident multifrontal factorisation as the LAST Gauss-Newton
 *   iteration of the last sgo_optimize_gn left it -- device memory as stored, nothing recomputed (the closing chi2 pass of a call
 *   writes no array).  Same convention as sgo_debug_amg_array: returns the array's size in bytes (0: it has no entries) and
 *   copies it when cap_bytes holds it.  SGO_EINVAL with a message when the resident graph is not on the multifrontal path
 *   (sgo_solver_description does not start with multifrontal_cholesky) or no sgo_optimize_gn with iters > 0 has run on it.
 * sgo_mfront_plan_array: the same arrays SGO_MF_INFO .. SGO_MF_ELIM_VERTEX from the host's originals -- the plan sgo_set_graph_se2 makes for
 *   this graph (arguments as sgo_mfront_plan's; leaf <= 0 and max_crit_mflop <= 0: its defaults, SGO_MFRONT_LEAF / _CRIT_MFLOP /
 *   _DEGREE of the environment included), on the host alone.  SGO_ENOTHING: the graph does not qualify.
 * `what` is one of SGO_MF_*:
 *   INFO         int64[8] { free poses n, edges E, fronts, levels, doubles of the arena, entries of PINV, targets, contributions }
 *                (the host's sizes: the device holds no copy)
 *   FRONTS       int64[fronts][14], fronts numbered children first: e0 (first elimination position of the own poses), own3 (own
 *                scalar rows), m (own + boundary scalar rows; the right-hand side is row m), ld, off (the matrix' place in ARENA:
 *                column-major, lower triangle, own columns first), nb (boundary poses), bnd_off, kid[0], kid[1] (-1: none),
 *                pinv_off[0], pinv_off[1], tgt0, tgt1, parent (-1: a root)
 *   LEVEL_PTR    int32[levels + 1] (host), LEVEL_FRONT int32[fronts]: the fronts of height h are LEVEL_FRONT[LEVEL_PTR[h] .. LEVEL_PTR[h + 1])
 *   BND          int32: the boundary poses of front f, elimination positions ascending, at bnd_off .. + nb
 *   PINV         int32: child k of front f: PINV[pinv_off[k] + local pose of f] = that pose's index among the child's boundary
 *                poses, -1: the child does not hold it
 *   TARGETS      int32[targets][4] { li, lj (local poses, li >= lj), c0, c1 }: the 3x3 blocks of front f that edges add to are
 *                tgt0 .. tgt1; CONTRIB int32: edge << 2 | part (0: D_ii and b_i, 1: D_jj and b_j, 2: H_ij as stored, 3: its transpose)
 *   ELIM_VERTEX  int32[n]: the vertex at every elimination position
 *   ELEM         double[E][28]: D_ii (upper triangle by rows, 6), D_jj (6), H_ij (9, by rows), b_i (3), b_j (3), one pad
 *                (after an sgo_optimize_gn_until that stopped by the gain rule: the elements at the FINAL poses -- the stopped
 *                iteration's edge pass had run --, where sgo_optimize_gn leaves those of its last factorisation; every other array
 *                is the plain call's)
 *   ARENA        double: every front's matrix after its factorisation: columns < own3 hold L11, L21 and (row m) the
 *                forward-substituted right-hand side; columns >= own3 the assembled boundary block and its right-hand side
 *   X            double[3 n]: the step by elimination position;  INVD double[3 n]: 1 / L[c][c];  YINV double[3 n][16]: row i of the
 *                inverse of its 16 x 16 diagonal block's factor
 *   FLAGS        int32[8]: fail, iteration of the failure, non-finite substitution, updates applied
 *   SEL          double, ARENA's size: every front's selected inverse as the last sgo_marginals_selected stored it -- the front's
 *                own layout (same off and ld, lower triangle, row m unused); 0 bytes before the first such call.  After
 *                sgo_marginals_selected the other arrays describe the factor at the current poses (ELEM, ARENA, INVD, YINV, FLAGS
 *                are rewritten by its factor phase) and X is unchanged; on a graph that is not on the multifrontal path the hook
 *                then reads the plan that call analysed for itself.
 *   FS_Y, FS_X   double[columns][3 n] by elimination position: the last chunk of the last sgo_factor_solve / sgo_candidate_gate after
 *                the forward pass (L Y = B) and after the backward pass (L^T X = Y); 0 bytes before the first such call (and after
 *                a call that went through the PCG).  Those calls rewrite the factor's arrays as SEL's note says, X is unchanged. */
#define SGO_MF_INFO 0
#define SGO_MF_FRONTS 1
#define SGO_MF_LEVEL_PTR 2
#define SGO_MF_LEVEL_FRONT 3
#define SGO_MF_BND 4
#define SGO_MF_PINV 5
#define SGO_MF_TARGETS 6
#define SGO_MF_CONTRIB 7
#define SGO_MF_ELIM_VERTEX 8
#define SGO_MF_ELEM 9
#define SGO_MF_ARENA 10
#define SGO_MF_X 11
#define SGO_MF_INVD 12
#define SGO_MF_YINV 13
#define SGO_MF_FLAGS 14
#define SGO_MF_SEL 15
#define SGO_MF_FS_Y 16
#define SGO_MF_FS_X 17
int64_t sgo_debug_mfront_array(sgo_ctx* ctx, int32_t what, void* out, int64_t cap_bytes);
int64_t sgo_mfront_plan_array(int32_t V, const double* poses, const uint8_t* fixed, int32_t E, const int32_t* ei, const int32_t* ej,
                              int32_t leaf, double max_crit_mflop, int32_t what, void* out, int64_t cap_bytes);
/* Test hooks for the single-launch direct path (small graphs: DESIGN.md section 5a; tests/direct_reference.py checks every stage
 * of one Gauss-Newton iteration of k_direct from these arrays).
 * sgo_direct_plan_array: one table of the host analysis sgo_set_graph_se2 makes for this graph (max_rows: sgo_opts.direct_rows;
 *   <= 0: its default), on the host alone -- no GPU is touched.  Same convention as sgo_debug_amg_array: returns the table's size in
 *   bytes (0: it has no entries) and copies it when cap_bytes holds it.  SGO_ENOTHING when the graph does not qualify, with the
 *   reason sgo_solver_description gives after "direct path not used: " in sgo_last_error(NULL).  Tables: SGO_DR_INFO .. SGO_DR_DPAIR,
 *   each exactly the array that is uploaded.
 * sgo_debug_direct_array: the same tables read back from the device, and what the last sgo_optimize_gn left -- device memory as
 *   stored, nothing recomputed.  SGO_EINVAL with a message when the resident graph is not on the direct path
 *   (sgo_solver_description does not start with direct_ldlt) or no sgo_optimize_gn with iters > 0 has run on it.
 *   ESCR, ZSC, WD, WO are the kernel's own work arrays and are there after every call (the closing chi2 pass writes none of them;
 *   sgo_optimize_gn_until leaves its last iteration's, sgo_optimize_gn_hypotheses works on copies of its own).  The snapshots A_*,
 *   F_*, D_*, X exist only in a DEBUG RUN: the environment variable SGO_DIRECT_DEBUG set when the graph is set makes
 *   sgo_optimize_gn launch an instantiation of the same kernel that copies out, in every iteration, the state that otherwise lives
 *   and dies in the LDS, so that they hold the LAST iteration that ran; outside a debug run (and after an sgo_optimize_gn_until,
 *   which has no such instantiation) each returns 0 bytes.  A debug run leaves the poses, the history and ESCR / WD / WO bit for
 *   bit as the production kernel does.
 * `what` is one of SGO_DR_* (positions are ELIMINATION positions 0 .. n: the nI poses of the sparse levels, then the ns separators):
 *   INFO         int64[13] { free poses n, sparse columns nI, separators ns, levels NL, edges E, slots NB, doubles of the packed
 *                separator triangle tri = 3 ns (3 ns + 1) / 2, zero slots, multi-edge pairs, forward tasks, contributions, bytes of
 *                dynamic LDS, 1 when the vector lives in global memory (the XG instantiations) } (the host's sizes)
 *   POS_VERTEX   int32[n]: the vertex at every position
 *   VREC         int32[n][4]: the incident (edge << 1 | side) of a position, -1: none; [3] <= -2: more at VOVER[-2 - [3]]
 *   VOVER        int32: the overflow lists, each { count, entries }
 *   EDGE_TGT     uint32[max(E, 1)]: where an edge's H_ij goes: kind << 30 | transposed << 29 | index; kind 0 nowhere (a fixed
 *                endpoint), 1 slot `index`, 2 separator block (row << 12 | column), 3 a pair with several edges (see MULTI)
 *   ZERO_SLOTS   int32: the slots that are pure fill (cleared before every factorisation)
 *   MULTI        int32[pairs][2] { target as EDGE_TGT's (kind 1 / 2, no transposed bit), first edge << 1 | transposed }; ENEXT
 *                int32[max(E, 1)]: the next edge of the same pair in that encoding, -1: the last
 *   SLOT_RC      int32[NB][2] { row position (-1: the dummy slot of an empty column), column position (-1: padding) }
 *   LMETA        int32[2 (NL + 1)]: the slot range (multiples of 64) and then the task range of every level
 *   TK           int32[tasks][4] { kind << 28 | index, first contribution, end, 0 }: kind 0 slot, 1 diagonal block of a sparse
 *                column (with its right-hand side), 2 separator block (row << 12 | column; a diagonal one with its right-hand side)
 *   CTR          int32[contributions][4] { slot of W_ik, slot of W_jk, k, 0 }
 *   DPAIR        uint16[ns (ns + 1) / 2]: separator block pairs bi << 8 | bj, bi >= bj, by bj descending
 *   ESCR         double[27][E]: per edge Hii (6, upper triangle by rows), bi (3), Hjj (6), bj (3) and -- only for the edges of
 *                multi pairs, the rest is never written -- Hij (9, by rows)
 *   ZSC          double[2][E]: sin and cos of the inverse measurement's angle
 *   WD           double[nI][10], WO double[NB][10]: the diagonal and the stored blocks after the forward levels (9 by rows, one pad)
 *   A_WD A_WO    the same two after the assembly barrier;  A_SD double[tri] the packed lower triangle of the separator block,
 *                A_XB double[3 n] the right-hand side by position, at that point
 *   F_SD F_XB    after the last forward level
 *   D_SD         after the dense elimination: block column p below the diagonal holds W_ip (the panel stays); the diagonal blocks
 *                of pivots >= 1 are NOT the pivots (only their factor is kept);  D_PINV double[ns][6] { l10, l20, l21, 1 / p0,
 *                1 / p1, 1 / p2 } of every pivot block D = L diag(p) L^T;  D_BS double[3 ns] the separators' forward-substituted
 *                right-hand side
 *   X            double[3 n]: the step by position, after the backward levels */
#define SGO_DR_INFO 0
#define SGO_DR_POS_VERTEX 1
#define SGO_DR_VREC 2
#define SGO_DR_VOVER 3
#define SGO_DR_EDGE_TGT 4
#define SGO_DR_ZERO_SLOTS 5
#define SGO_DR_MULTI 6
#define SGO_DR_ENEXT 7
#define SGO_DR_SLOT_RC 8
#define SGO_DR_LMETA 9
#define SGO_DR_TK 10
#define SGO_DR_CTR 11
#define SGO_DR_DPAIR 12
#define SGO_DR_ESCR 13
#define SGO_DR_ZSC 14
#define SGO_DR_WD 15
#define SGO_DR_WO 16
#define SGO_DR_A_WD 17
#define SGO_DR_A_WO 18
#define SGO_DR_A_SD 19
#define SGO_DR_A_XB 20
#define SGO_DR_F_SD 21
#define SGO_DR_F_XB 22
#define SGO_DR_D_SD 23
#define SGO_DR_D_PINV 24
#define SGO_DR_D_BS 25
#define SGO_DR_X 26
int64_t sgo_direct_plan_array(int32_t V, const uint8_t* fixed, int32_t E, const int32_t* ei, const int32_t* ej, int32_t max_rows,
                              int32_t what, void* out, int64_t cap_bytes);
int64_t sgo_debug_direct_array(sgo_ctx* ctx, int32_t what, void* out, int64_t cap_bytes);
/* Test hooks for the PCG recurrence (tests/pcg_reference.py checks every stage of one iteration and of the start from them).
 * Both need sgo_linearize and refuse a multi-GPU context and an active overlay, as the sibling hooks do.
 * sgo_debug_pcg_array: a read-only copy of one array of the recurrence as the last start / solve left it -- device memory as
 *   stored, nothing recomputed.  Same convention as sgo_debug_amg_array: returns the array's size in bytes (0: no such array
 *   here) and copies it when cap_bytes holds it.  `what` is one of SGO_PCG_*:
 *   B X R Z P Q   double[n][3], rows in the internal order (ROW_ORDER int32[n]: the internal row of every hessian-order row)
 *   DINV          double[n][6], the block-diagonal inverse (upper triangle by rows);  XS0 double[n][3], the cycle's first sweep
 *                 from zero, omega Dinv r (0 bytes without a hierarchy)
 *   SCALARS       the device's PcgScalars, 104 bytes: doubles rz, pq, rr, bb, alpha, beta, tol2, rz_prev at 0, 8, .. 56; int32
 *                 iter, maxit, stop, iter_prev, probe_k, (pad) at 64 .. 84; doubles probe_rel, probe_max at 88, 96.
 *                 HOST_SCALARS: the host copy the last solve returned with;  MIRROR: the pinned copy k_update_p rewrites
 *                 (both undefined before the first solve on the context: sgo_linearize alone writes neither)
 *   PARTIALS      double[3][2048], the partial-sum rows as stored;  ZPARTS double[2][2048], the cycle's (0 bytes without a
 *                 hierarchy);  COUNTS int32[8] { start_bb, start_rz, n_pq, n_rz, n_rr, n_zq, n_xq, n_bx }: how many entries
 *                 of a row the latest launches wrote.  After a start: b.b = PARTIALS[1][0 .. start_bb); r.z = PARTIALS[0]
 *                 (block-Jacobi) or ZPARTS[0] (multigrid) [0 .. start_rz); a warm start's x_prev . H x_prev = PARTIALS[0]
 *                 [0 .. n_xq) and b . x_prev = PARTIALS[2][0 .. n_bx) (that product stores over PARTIALS[1] too: b.b was
 *                 reduced before it).  After an iteration: p.q = PARTIALS[0][0 .. n_pq);
 *                 r.r = PARTIALS[2][0 .. n_rr); r.z = PARTIALS[1] (block-Jacobi) or ZPARTS[0] (multigrid) [0 .. n_rz);
 *                 z.q = ZPARTS[1][0 .. n_zq) (n_zq = 0: block-Jacobi, plain beta).  The iteration's counts are those of the
 *                 latest launch or capture of an iteration (a replayed hipGraph keeps them).
 *   START_ARGS    double[4] { tol, tol_cap, bb_ref, maxit }: what the last start handed to k_init_scalars (host bookkeeping)
 *   LANCZOS       double[min(iter, 2048)][3] { alpha, beta, rz_prev } per iteration (0 bytes unless SGO_LANCZOS was set)
 * sgo_debug_pcg_run: sgo_solve with the per-call fields sgo_optimize_gn sets for the solves of a call: an iteration cap
 *   (maxit > 0; maxit == 0: the start state alone, no iteration runs), a warm start from x_prev[n][3] (hessian order; NULL:
 *   cold), the absolute-tolerance reference bb_ref = |b|^2 of a call's first solve (0: relative tolerance) with the cap
 *   derived from sgo_opts.pcg_tol_cap as sgo_optimize_gn derives it, and the progress probe (probe_k = 0: none; probe_max = 0:
 *   record only; probe_max > 0 keeps the coarse operators as a lagged solve does).  The warm start and the probe need a
 *   multigrid hierarchy.  The fields are restored afterwards.  Returns the iterations run; a breakdown (stop == 3) is read
 *   from the scalars, not from the return value. */
#define SGO_PCG_B 0
#define SGO_PCG_X 1
#define SGO_PCG_R 2
#define SGO_PCG_Z 3
#define SGO_PCG_P 4
#define SGO_PCG_Q 5
#define SGO_PCG_DINV 6
#define SGO_PCG_XS0 7
#define SGO_PCG_SCALARS 8
#define SGO_PCG_HOST_SCALARS 9
#define SGO_PCG_MIRROR 10
#define SGO_PCG_PARTIALS 11
#define SGO_PCG_ZPARTS 12
#define SGO_PCG_COUNTS 13
#define SGO_PCG_LANCZOS 14
#define SGO_PCG_ROW_ORDER 15
#define SGO_PCG_START_ARGS 16
int64_t sgo_debug_pcg_array(sgo_ctx* ctx, int32_t what, void* out, int64_t cap_bytes);
int sgo_debug_pcg_run(sgo_ctx* ctx, int32_t maxit, const double* x_prev, double bb_ref, int32_t probe_k, double probe_max);
/* Diagnostic (env SGO_LANCZOS=1 when the graph is set): alpha, beta of every PCG iteration of the last solve as pairs in
 * iteration order -- the Lanczos matrix of the preconditioned operator follows from them (scripts/ritz_probe.py).  Returns
 * the iterations written (<= cap pairs), < 0 on error. */
int sgo_debug_lanczos(sgo_ctx* ctx, double* out, int cap);

/* One line naming the solver the resident graph's sgo_optimize_gn runs ("direct_ldlt: ...", "multifrontal_cholesky: ...",
 * "pcg_amg: L0 n=... ", "pcg_block_jacobi ..."): which path a graph took, and for the refusals of the direct and the
 * multifrontal path the reason ("pcg_amg: ...; direct path not used: more separators than the dense block holds;
 * multifrontal path not used: 4.00 edges per free pose > 2.50").  Never NULL. */
const char* sgo_solver_description(sgo_ctx* ctx);

/* Text of the last error on this context (or, with ctx == NULL, of the last failed sgo_create /
 * context-free call on this thread).  Never NULL. */
const char* sgo_last_error(sgo_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* SGO_H_ */
