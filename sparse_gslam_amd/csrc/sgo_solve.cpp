// sgo_solve.cpp -- host side of the Gauss-Newton iteration.
//
// Mirrors the control flow of g2o's SparseOptimizer::optimize() with OptimizationAlgorithmGaussNewton as sparse-gslam
// configures it (src/sparse_gslam/src/graphs.cpp:17-23; called at submap_loop_closer.cpp:286-288 and
// log_runner.cpp:203-204):
//     for k in 0..iters:  computeActiveErrors; buildSystem; solve; update
// with the linear solve done by preconditioned CG on the device instead of LinearSolverEigen.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sgo_ctx.h"
#include "sgo_rules.h"

namespace sgo {

// ---- profiling: HIP events around each launch on the ctx stream ---------------------------
hipEvent_t get_event(sgo_ctx* c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}
// An event pair with nothing between them still measures a few us on the queue; it is measured
// once (median of 33 empty brackets) and REPORTED (sgo_profile_overhead_ms) as the bias bound of
// the per-kernel averages relative to rocprofv3's kernel durations -- it is not subtracted.
void prof_calibrate(sgo_ctx* c) {
  if (c->prof_null_ms >= 0.0) return;
  std::vector<float> v;
  for (int k = 0; k < 33; ++k) {
    hipEvent_t a = get_event(c), b = get_event(c);
    hipEventRecord(a, c->stream);
    hipEventRecord(b, c->stream);
    hipStreamSynchronize(c->stream);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) == hipSuccess) v.push_back(ms);
    c->ev_pool.push_back(a);
    c->ev_pool.push_back(b);
  }
  std::sort(v.begin(), v.end());
  c->prof_null_ms = v.empty() ? 0.0 : v[v.size() / 2];
}
void prof_flush(sgo_ctx* c) {
  if (c->pending.empty()) return;
  hipStreamSynchronize(c->stream);
  for (auto& r : c->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      c->prof_ms[r.kid] += ms;
      if (c->prof_samples[r.kid].size() < sgo_ctx::kProfSamples) c->prof_samples[r.kid].push_back(ms);
    }
    c->ev_pool.push_back(r.a);
    c->ev_pool.push_back(r.b);
  }
  c->pending.clear();
}

// ---- algorithmic bytes per launch ------------
// (the level-0 product: bytes_spmv0, sgo_internal.h)
// linearise + assemble: the row-parallel design reads each edge's operands once per endpoint row
// (2 x 128 B: indices, inverse measurement, information, two poses), writes the off-diagonal block once
// (72 B) and 72 B of (diagonal block, b) per row
double bytes_linearize(const sgo_ctx* c) { return 128.0 * c->S0.ncs + 72.0 * c->S0.nu + 72.0 * c->n; }
double bytes_chi2(const sgo_ctx* c) { return 96.0 * c->E + 24.0 * c->V; }

// ---- one GN building block each ------------------------------------------------------------
int do_chi2(sgo_ctx* c, double* d_out2, double* d_e2) {
  int grid = 0;
  {
    Scope sc(c, K_CHI2, bytes_chi2(c));
    int e0 = 0, e1 = c->el.E;   // (the resident edge list; c->E also counts the edges an incremental update appended: el2 below)
    if (c->comm.nranks > 1 && !c->replicated && !d_e2) sgo_shard_range(c->el.E, c->comm.nranks, c->comm.rank, &e0, &e1);
    launch_chi2(c->stream, c->el, e0, e1, c->d_poses, d_e2, c->d_partials, &grid, c->ov.active ? &c->ov.dev.el : nullptr);
  }
  {
    Scope sc(c, K_REDUCE2, 16.0 * grid);
    launch_reduce2(c->stream, c->d_partials, grid, d_out2);
  }
  if (c->comm.nranks > 1 && !c->replicated && !d_e2 && !c->comm.allreduce_f64(d_out2, 2, c->stream, &c->err)) return SGO_ECOMM;
  return SGO_OK;
}

// PCG start state after k_finalize (x = 0, r = b, z = Dinv b, p = z; partials rz / bb with `grid`
// entries).  With the AMG preconditioner: refresh the coarse operators, z = M^-1 b, p = z.
int do_spmv(sgo_ctx* c, const double* x, double* y, bool dot, const PcgScalars* S, int* grid_out);

// Row-owner mode (multi-GPU): every vector lives on this rank's rows [row0, row1); a product needs the neighbours'
// boundary rows of its operand (one exchange), a dot product the other ranks' partial sums (they ride on an exchange and
// are reduced in rank order by the consumer: bit-identical scalars, hence identical decisions, on every rank).
static bool xch(sgo_ctx* c, double* vec, const HaloScalars& sc) {
  return halo_exchange(c->halo, c->stream, vec, 3, c->halo.bnd, c->halo.bmax, sc, &c->err);
}
static HaloScalars scal(const double* p0, int n0, const double* p1 = nullptr, int n1 = 0, const double* p2 = nullptr, int n2 = 0) {
  HaloScalars sc;
  sc.parts[0] = p0; sc.n[0] = n0;
  sc.parts[1] = p1; sc.n[1] = n1;
  sc.parts[2] = p2; sc.n[2] = n2;
  return sc;
}

static void set_probe(sgo_ctx* c, int k, double max);
static int start_pcg_owner(sgo_ctx* c, int grid) {
  set_probe(c, 0, 0.0);   // (the progress probe belongs to the single-GPU lagged refresh: never armed here)
  const HaloDev& H = c->halo;
  const int G = H.G, nr = H.row1 - H.row0;
  const size_t o3 = 3 * (size_t)H.row0;
  const int maxit = c->call.pcg_softcap > 0 ? std::min(c->call.pcg_softcap, c->opts.pcg_maxit) : c->opts.pcg_maxit;
  const double tol = c->opts.pcg_tol * c->tol_scale;
  double* bb_parts = c->d_partials + kMaxPartials;   // k_finalize: [0] r.z (block-Jacobi), [1] b.b over the owned rows
  int rc;
  if (c->amg && !c->call.skip_update && (rc = amg_update(c->amg, c->stream, &c->err))) return rc;
  if (c->amg && amg_comm_failed(c->amg)) return SGO_ECOMM;
  // the block-diagonal inverse of the neighbours' boundary rows (the halo-row recurrences of the iterations apply it)
  if (c->amg && !halo_exchange(H, c->stream, c->S0.dinv, 6, H.bnd, H.bmax, HaloScalars(), &c->err)) return SGO_ECOMM;
  if (!c->amg) {   // block-Jacobi: k_finalize left z = Dinv b, p = z and the partials of r.z
    if (!xch(c, c->d_p, scal(c->d_partials, grid, bb_parts, grid))) return SGO_ECOMM;
    Scope sc(c, K_INIT_SCALARS, 16.0 * G);
    launch_init_scalars(c->stream, c->d_S, H.gparts, G, H.gparts + G, G, tol, maxit, c->call.bb_ref, c->tol_cap);
    return SGO_OK;
  }
  if (c->call.warm_valid && c->d_xprev) {
    // warm start (see start_pcg): x_prev is the previous step, gathered to every rank before the pose update
    int gq = 0, gd = 0;
    // (the product's kernel stores both of its dot-product rows: k_finalize's b.b partials move out of its way first)
    double* bb_keep = c->d_zparts + kMaxPartials;
    HIP_TRY(c, hipMemcpyAsync(bb_keep, bb_parts, sizeof(double) * (size_t)grid, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = do_spmv(c, c->d_xprev, c->d_q, true, nullptr, &gq))) return rc;
    {
      Scope sc(c, K_DOT, 48.0 * nr);
      launch_dot(c->stream, 3 * nr, c->d_b + o3, c->d_xprev + o3, c->d_partials + 2 * kMaxPartials, nullptr, &gd);
    }
    if (!xch(c, nullptr, scal(bb_keep, grid, c->d_partials, gq, c->d_partials + 2 * kMaxPartials, gd))) return SGO_ECOMM;
    {
      Scope sc(c, K_INIT_SCALARS, 16.0 * G);   // ||b||^2, tolerance, iteration count (r.z is replaced below)
      launch_init_scalars(c->stream, c->d_S, H.gparts, G, H.gparts, G, tol, maxit, c->call.bb_ref, c->tol_cap);
    }
    {
      Scope sc(c, K_UPDATE_XR, 120.0 * nr);
      launch_warm_start(c->stream, 3 * nr, c->d_xprev + o3, c->d_q + o3, c->d_b + o3, c->d_x + o3, c->d_r + o3, H.gparts + G, G,
                        H.gparts + 2 * G, G);
    }
    const int gz = amg_apply(c->amg, c->stream, c->d_r, c->d_z, c->d_r, c->d_zparts, nullptr, nullptr, AmgXs0::compute);
    if (amg_comm_failed(c->amg)) return SGO_ECOMM;
    HIP_TRY(c, hipMemcpyAsync(c->d_p + o3, c->d_z + o3, sizeof(double) * 3 * (size_t)nr, hipMemcpyDeviceToDevice, c->stream));
    if (!xch(c, c->d_p, scal(c->d_zparts, gz))) return SGO_ECOMM;
    {
      Scope sc(c, K_INIT_SCALARS, 8.0 * G);
      launch_restart_scalars(c->stream, c->d_S, H.gparts, G, maxit, 1);
    }
    if (!xch(c, c->d_r, HaloScalars())) return SGO_ECOMM;   // the halo rows' copies of r start here
    return SGO_OK;
  }
  const int gz = amg_apply(c->amg, c->stream, c->d_r, c->d_z, c->d_r, c->d_zparts, nullptr, nullptr, AmgXs0::ready);
  if (amg_comm_failed(c->amg)) return SGO_ECOMM;
  HIP_TRY(c, hipMemcpyAsync(c->d_p + o3, c->d_z + o3, sizeof(double) * 3 * (size_t)nr, hipMemcpyDeviceToDevice, c->stream));
  if (!xch(c, c->d_p, scal(c->d_zparts, gz, bb_parts, grid))) return SGO_ECOMM;
  {
    Scope sc(c, K_INIT_SCALARS, 16.0 * G);
    launch_init_scalars(c->stream, c->d_S, H.gparts, G, H.gparts + G, G, tol, maxit, c->call.bb_ref, c->tol_cap);
  }
  if (!xch(c, c->d_r, HaloScalars())) return SGO_ECOMM;   // the halo rows' copies of r start here
  return SGO_OK;
}

// what k_update_p records besides the recurrence: the pinned mirror of the scalars and (diagnostic, env SGO_LANCZOS=1) the
// recurrence's coefficients per iteration -- the Lanczos matrix of M^-1 H follows from them (scripts/ritz_probe.py)
static RecDev rec_dev(const sgo_ctx* c) {
  RecDev r;
  r.mirror = c->d_Sz;
  r.lanczos = c->d_lanczos;
  return r;
}

// k_diag_change's three sums over `grid` workgroups, from half `half` of h_dchg (after a synchronisation behind the launch)
static void sum_diag_change(const sgo_ctx* c, int half, int grid, double v[3]) {
  const volatile double* h = c->h_dchg + 3 * (size_t)half * kMaxPartials;
  for (int k = 0; k < 3; ++k) {
    v[k] = 0.0;
    for (int i = 0; i < grid; ++i) v[k] += h[(size_t)k * kMaxPartials + i];
  }
}
static void read_diag_change(sgo_ctx* c) {
  sum_diag_change(c, 0, c->dchg_grid, c->last_dchg);
  c->amg_dchg_pending = false;
}
static void set_probe(sgo_ctx* c, int k, double max) {
  if (k == c->probe_dev_k && max == c->probe_dev_max) return;
  launch_set_probe(c->stream, c->d_S, k, max);
  c->probe_dev_k = k;
  c->probe_dev_max = max;
}

int start_pcg(sgo_ctx* c, int grid) {
  if (c->owner) return start_pcg_owner(c, grid);
  const int maxit = c->call.pcg_softcap > 0 ? std::min(c->call.pcg_softcap, c->opts.pcg_maxit) : c->opts.pcg_maxit;
  const double tol = c->opts.pcg_tol * c->tol_scale;
  c->pcg_counts.start_bb = c->pcg_counts.start_rz = grid;
  c->pcg_counts.n_xq = c->pcg_counts.n_bx = 0;
  c->pcg_start.tol = tol;
  c->pcg_start.tol_cap = c->tol_cap;
  c->pcg_start.bb_ref = c->call.bb_ref;
  c->pcg_start.maxit = maxit;
  if (c->amg) {
    int rc = c->call.skip_update ? SGO_OK : amg_update(c->amg, c->stream, &c->err);
    if (rc) return rc;
    const bool warm = c->call.warm_valid && c->d_xprev;
    if (warm) {
      // Start from the previous Gauss-Newton step scaled by the energy-optimal factor: consecutive steps of a linearly
      // converging iteration are nearly parallel, ||b - gamma H x_prev|| is 0.2-0.45 ||b|| on C4 / C2 (scripts/
      // warm_probe.py), i.e. two PCG iterations for the price of one Hessian product.  Same stopping test, same
      // solution; only the path to it is shorter.
      {
        Scope sc(c, K_INIT_SCALARS, 16.0 * grid);   // ||b||^2, tolerance, iteration count (r.z is replaced below)
        launch_init_scalars(c->stream, c->d_S, c->d_partials, grid, c->d_partials + kMaxPartials, grid, tol, maxit, c->call.bb_ref, c->tol_cap);
      }
      int gq = 0, gd = 0;
      if ((rc = do_spmv(c, c->d_xprev, c->d_q, true, nullptr, &gq))) return rc;
      {
        Scope sc(c, K_DOT, 48.0 * c->n);
        launch_dot(c->stream, 3 * c->n, c->d_b, c->d_xprev, c->d_partials + 2 * kMaxPartials, nullptr, &gd);
      }
      {
        Scope sc(c, K_UPDATE_XR, 120.0 * c->n);
        launch_warm_start(c->stream, 3 * c->n, c->d_xprev, c->d_q, c->d_b, c->d_x, c->d_r, c->d_partials, gq,
                          c->d_partials + 2 * kMaxPartials, gd);
      }
      c->pcg_counts.n_xq = gq;
      c->pcg_counts.n_bx = gd;
    }
    // (cold: k_finalize left x = 0, r = b and xs = omega Dinv b, the cycle's first sweep from zero)
    const AmgXs0 xs_ready = warm ? AmgXs0::compute : AmgXs0::ready;
    const int gz = amg_apply(c->amg, c->stream, c->d_r, c->d_z, c->d_r, c->d_zparts, nullptr, nullptr, xs_ready);
    if (amg_comm_failed(c->amg)) return SGO_ECOMM;
    HIP_TRY(c, hipMemcpyAsync(c->d_p, c->d_z, sizeof(double) * 3 * (size_t)c->n, hipMemcpyDeviceToDevice, c->stream));
    c->pcg_counts.start_rz = gz;
    if (warm) {
      Scope sc(c, K_INIT_SCALARS, 8.0 * gz);
      launch_restart_scalars(c->stream, c->d_S, c->d_zparts, gz, maxit, 1);
    } else {
      Scope sc(c, K_INIT_SCALARS, 8.0 * (gz + grid));
      launch_init_scalars(c->stream, c->d_S, c->d_zparts, gz, c->d_partials + kMaxPartials, grid, tol, maxit, c->call.bb_ref, c->tol_cap);
    }
    // progress probe of the lagged refresh (PcgScalars): a fresh solve records, a solve behind kept operators is held to the record
    set_probe(c, c->call.lag_on ? c->hier.probe_k : 0, c->call.skip_update ? c->hier.probe_max : 0.0);
  } else {
    Scope sc(c, K_INIT_SCALARS, 16.0 * grid);
    launch_init_scalars(c->stream, c->d_S, c->d_partials, grid, c->d_partials + kMaxPartials, grid, tol, maxit, c->call.bb_ref, c->tol_cap);
    set_probe(c, 0, 0.0);   // (a probe left armed by an earlier solve behind a hierarchy this graph has since lost would raise stop = 4 here)
  }
  return SGO_OK;
}

// The movement of the level-0 diagonal blocks up to which a solve keeps its coarse operators: what costs this graph's solves four
// PCG iterations by the slope learned from its kept solves (HierarchyState), at most SGO_AMG_LAG_TAU.
static double lag_allowed(const sgo_ctx* c) { return rules::lag_allowed(c->knobs.lag_tau, c->hier.lag_slope); }
// ... and how far they have moved against the coarse operators' reference (k_diag_change's sums; `none`: no sums)
static double moved_rel(const sgo_ctx* c, double none) { return c->last_dchg[1] > 0.0 ? c->last_dchg[0] / c->last_dchg[1] : none; }

// A solve behind KEPT coarse operators was stopped (its progress probe, or its iteration cap): the operators are refreshed and the
// solve carries on from its current x and r -- z = M^-1 r with the new cycle, p = z, the recurrence restarts (what the kept
// iterations gained in the residual stays; the Krylov memory goes, about two iterations' worth).  Single GPU only.
static int refresh_and_continue(sgo_ctx* c, int maxit) {
  int rc = amg_update(c->amg, c->stream, &c->err);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_dref, c->S0.dblk, sizeof(double) * 6 * (size_t)c->n, hipMemcpyDeviceToDevice, c->stream));
  c->hier.ref_valid = true;
  c->call.skip_update = false;
  const int gz = amg_apply(c->amg, c->stream, c->d_r, c->d_z, c->d_r, c->d_zparts, nullptr, nullptr, AmgXs0::compute);
  HIP_TRY(c, hipMemcpyAsync(c->d_p, c->d_z, sizeof(double) * 3 * (size_t)c->n, hipMemcpyDeviceToDevice, c->stream));
  {
    Scope sc(c, K_INIT_SCALARS, 8.0 * gz);
    launch_restart_scalars(c->stream, c->d_S, c->d_zparts, gz, maxit, 0);
  }
  set_probe(c, 0, 0.0);
  return SGO_OK;
}

// buildSystem + preconditioner + PCG start state.  Multi-GPU: every rank linearises the whole graph (1.5 % of
// a GN iteration; sharding it would mean all-reducing the blocks, 72 B per edge, to save it).
int do_linearize(sgo_ctx* c) {
  const int g0 = c->owner ? c->halo.g0 : 0, g1 = c->owner ? c->halo.g1 : c->S0.ngrp;   // row-owner mode: this rank's rows
  const int row0 = c->owner ? c->halo.row0 : 0, row1 = c->owner ? c->halo.row1 : c->n;
  {
    Scope sc(c, K_LINEARIZE, bytes_linearize(c) * (g1 - g0) / std::max(1, c->S0.ngrp));
    launch_linearize(c->stream, c->S0, g0, g1, c->es, c->d_poses, c->d_dgb);
  }
  if (c->ov.active) {
    // incremental set-up (sgo_overlay.h): the appended edges' linearisation, the elimination of the appended chain; the
    // touched rows' right-hand sides in dgb receive g = b_T - H_TN H_NN^-1 b_N before k_finalize reads them
    launch_ov_lin(c->stream, c->ov.dev, c->d_poses);
    launch_ov_solve(c->stream, c->ov.dev, c->d_dgb);
  }
  int grid = 0;
  {
    Scope sc(c, K_FINALIZE, (72.0 + 48.0 + 48.0 + 6 * 24.0) * (row1 - row0));
    launch_finalize(c->stream, c->S0, row0, row1, c->d_dgb, c->d_b, c->d_x, c->d_r, c->d_z, c->d_p,
                    c->amg ? amg_xs0(c->amg) : nullptr, c->amg ? amg_omega(c->amg) : 0.0, c->d_partials, &grid);
  }
  if (c->amg && c->call.lag_on && !c->owner && c->d_dref) {   // (an incremental overlay changes nothing here: the hierarchy is the resident rows')
    // Lagged refresh: a solve keeps the coarse operators of the previous one while the level-0 diagonal blocks have moved little
    // (lag_allowed: relative, summed over the rows) since those operators were made.
    c->call.skip_update = false;
    c->amg_dchg_pending = false;
    // The host waits for the sums -- the one round trip of the scheme, with the launches of the refresh not yet queued behind it:
    // 40-50 us -- only when the movement of the PREVIOUS iteration says this one may keep (a converging call's steps shrink);
    // otherwise the solve refreshes, the sums are read behind the solve's own synchronisation, and the kernel that measures
    // stores the new reference on its way.
    const bool wait = c->hier.ref_valid && ((c->call.lag_expect && c->hier.probe_max > 0.0) || c->call.force_keep);
    c->dchg_grid = launch_diag_change(c->stream, 0, c->n, c->S0.dblk, c->d_dref, !wait, c->h_dchg_dev);
    c->amg_dchg_pending = c->hier.ref_valid;
    if (wait) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      read_diag_change(c);
      c->call.skip_update = moved_rel(c, 1.0) <= lag_allowed(c) && c->last_dchg[2] <= rules::kLagRowsMoved && c->hier.probe_max > 0.0;
      if (c->call.force_keep) {   // calibration (SGO_AMG_LAG_FORCE=N): every solve after iteration N keeps, whatever moved
        c->call.skip_update = true;
        c->call.lag_cap = 0;
        c->hier.probe_max = 0.0;
      }
      if (!c->call.skip_update)
        HIP_TRY(c, hipMemcpyAsync(c->d_dref, c->S0.dblk, sizeof(double) * 6 * (size_t)c->n, hipMemcpyDeviceToDevice, c->stream));
    }
    if (c->call.skip_update && c->call.lag_cap > 0) c->call.pcg_softcap = c->call.pcg_softcap > 0 ? std::min(c->call.pcg_softcap, c->call.lag_cap) : c->call.lag_cap;
    if (!c->call.skip_update) c->hier.ref_valid = true;
  } else {
    c->call.skip_update = false;
    c->hier.ref_valid = false;
  }
  int rc = start_pcg(c, grid);
  if (rc) return rc;
  c->linearized = true;
  return SGO_OK;
}

// y = H x  (+ optional x.y partials).  The solve is replicated on every rank (identical H after
// the all-reduce in do_linearize), so no collective is needed here.
int do_spmv(sgo_ctx* c, const double* x, double* y, bool dot, const PcgScalars* S, int* grid_out) {
  Spmv0Args a{};
  a.x = x;
  a.y = y;
  a.S = S;
  if (c->owner) {
    // row-owner mode: this rank's tiles; x must hold the neighbours' boundary rows (the callers exchange them); the
    // dot product rides on the kernel as partials over the owned rows
    a.u0 = c->halo.u0;
    a.u1 = c->halo.u1;
    Scope sc(c, K_SPMV0T_AX, bytes_spmv0(c->S0, S0_AX) / c->halo.G);
    if (dot) {
      a.dotA = x;
      a.partials = c->d_partials;
    }
    const int grid = launch_spmv0_any(c->stream, c->S0, c->T0, S0_AX, a);
    if (grid_out) *grid_out = grid;
    return SGO_OK;
  }
  if (multi_rank(c)) {
    // multi-GPU: this rank's range of tiles only, zeros elsewhere, all-reduce of the product vector (every row
    // has exactly one non-zero contributor: the sum is exact), then the dot product on the full vectors --
    // the same arithmetic on every rank, so the replicated PCG recurrences stay bit-identical across ranks
    a.u0 = c->shard_u0;
    a.u1 = c->shard_u1;
    // (with a communicator the ranks' slices are all-gathered -- one contributor per row: nothing to sum, no zero fill;
    // the rank-emulation hook has no communicator: zeros elsewhere, so that a test can add the ranks' partial results)
    if (!c->gather_slices) HIP_TRY(c, hipMemsetAsync(y, 0, sizeof(double) * 3 * (size_t)c->n, c->stream));
    if (a.u1 > a.u0) {
      Scope sc(c, c->T0.ntile > 0 ? K_SPMV0T_AX : K_SPMV0_AX, bytes_spmv0(c->S0, S0_AX) * (a.u1 - a.u0) / std::max(1, c->shard_units));
      launch_spmv0_any(c->stream, c->S0, c->T0, S0_AX, a);
    }
    if (c->gather_slices) {
      if (!halo_gather_slices(c->halo, c->stream, y, 3, &c->err)) return SGO_ECOMM;
    } else if (!c->comm.allreduce_f64(y, 3 * (size_t)c->n, c->stream, &c->err)) {
      return SGO_ECOMM;
    }
    if (dot) {
      int grid = 0;
      Scope sc(c, K_DOT, 48.0 * c->n);
      launch_dot(c->stream, 3 * c->n, x, y, c->d_partials, S, &grid);
      if (grid_out) *grid_out = grid;
    }
    return SGO_OK;
  }
  Scope sc(c, c->T0.ntile > 0 ? K_SPMV0T_AX : K_SPMV0_AX, bytes_spmv0(c->S0, S0_AX));
  if (dot) {
    a.dotA = x;
    a.partials = c->d_partials;
  }
  const int grid = launch_spmv0_any(c->stream, c->S0, c->T0, S0_AX, a);
  if (c->ov.active) launch_ov_ax(c->stream, c->ov.dev, x, y, dot ? c->d_partials : nullptr, S);   // + U M U^T x (sgo_overlay.h)
  if (grid_out) *grid_out = grid;
  return SGO_OK;
}

// One PCG iteration in row-owner mode: two exchanges -- q's boundary with the partial sums of p.q | z's boundary with the
// partial sums of r.z, r.r, z.q -- and the all-reduce of the coarse right-hand side; all vector work on the owned rows.  The
// copies of the neighbours' boundary rows ("halo rows") of r, xs and p are kept current by repeating the recurrences on them
// (k_update_*_rows: same inputs, same arithmetic as the owner's: bit-identical), and the cycle prolongates the replicated
// coarse solution on them itself (k_prolong_rows, sgo_amg.hip): no exchange of xs, p or the corrected xs.
static int pcg_iteration_owner(sgo_ctx* c) {
  const HaloDev& H = c->halo;
  const int G = H.G, nr = H.row1 - H.row0;
  const size_t o3 = 3 * (size_t)H.row0;
  int g1 = 0, g2 = 0, rc;
  if ((rc = do_spmv(c, c->d_p, c->d_q, true, c->d_S, &g1))) return rc;
  double* parts2 = c->d_partials + kMaxPartials;  // [0] = r.z (block-Jacobi only), [1] = r.r
  if (c->amg) {
    if (!xch(c, c->d_q, scal(c->d_partials, g1))) return SGO_ECOMM;
    {
      Scope sc(c, K_UPDATE_XR, (7 * 24.0 + 48.0) * nr);
      launch_update_xr(c->stream, nr, c->d_S, H.gparts, G, c->S0.dinv + 6 * (size_t)H.row0, c->d_p + o3, c->d_q + o3, c->d_x + o3,
                       c->d_r + o3, c->d_z + o3, amg_xs0(c->amg) + o3, amg_omega(c->amg), parts2, &g2);
    }
    launch_update_xr_rows(c->stream, H.nhalo, H.halo_rows, c->d_S, c->S0.dinv, c->d_p, c->d_q, c->d_r, amg_xs0(c->amg), amg_omega(c->amg));
    const int gz = amg_apply(c->amg, c->stream, c->d_r, c->d_z, c->d_r, c->d_zparts, c->d_S, c->d_q, AmgXs0::ready_with_halo);
    if (amg_comm_failed(c->amg)) {
      c->err = "collective failed inside the multigrid cycle";
      return SGO_ECOMM;
    }
    if (!xch(c, c->d_z, scal(c->d_zparts, gz, parts2 + kMaxPartials, g2, c->d_zparts + kMaxPartials, gz))) return SGO_ECOMM;
    {
      Scope sc(c, K_UPDATE_P, 3 * 24.0 * nr);
      launch_update_p(c->stream, nr, c->d_S, H.gparts, G, H.gparts + G, G, H.gparts + 2 * G, c->d_z + o3, c->d_p + o3);
    }
    launch_update_p_rows(c->stream, H.nhalo, H.halo_rows, c->d_S, c->d_z, c->d_p);
    return SGO_OK;
  }
  // block-Jacobi: p.q | r.z, r.r | p
  if (!xch(c, nullptr, scal(c->d_partials, g1))) return SGO_ECOMM;
  {
    Scope sc(c, K_UPDATE_XR, (7 * 24.0 + 48.0) * nr);
    launch_update_xr(c->stream, nr, c->d_S, H.gparts, G, c->S0.dinv + 6 * (size_t)H.row0, c->d_p + o3, c->d_q + o3, c->d_x + o3,
                     c->d_r + o3, c->d_z + o3, nullptr, 0.0, parts2, &g2);
  }
  if (!xch(c, nullptr, scal(parts2, g2, parts2 + kMaxPartials, g2))) return SGO_ECOMM;
  {
    Scope sc(c, K_UPDATE_P, 3 * 24.0 * nr);
    launch_update_p(c->stream, nr, c->d_S, H.gparts, G, H.gparts + G, G, nullptr, c->d_z + o3, c->d_p + o3);
  }
  if (!xch(c, c->d_p, HaloScalars())) return SGO_ECOMM;
  return SGO_OK;
}

int pcg_iteration(sgo_ctx* c) {
  if (c->owner) return pcg_iteration_owner(c);
  int g1 = 0, g2 = 0, rc;
  if ((rc = do_spmv(c, c->d_p, c->d_q, true, c->d_S, &g1))) return rc;
  double* parts2 = c->d_partials + kMaxPartials;  // [0] = r.z (block-Jacobi only), [1] = r.r
  {
    // block-Jacobi: z = Dinv r; multigrid: xs = omega Dinv r, the cycle's first level-0 sweep from zero
    Scope sc(c, K_UPDATE_XR, (7 * 24.0 + 48.0) * c->n);
    launch_update_xr(c->stream, c->n, c->d_S, c->d_partials, g1, c->S0.dinv, c->d_p, c->d_q, c->d_x, c->d_r, c->d_z,
                     c->amg ? amg_xs0(c->amg) : nullptr, c->amg ? amg_omega(c->amg) : 0.0, parts2, &g2);
  }
  if (c->amg) {
    // the K-cycle is a (mildly) variable preconditioner: flexible beta from z.q
    const int gz = amg_apply(c->amg, c->stream, c->d_r, c->d_z, c->d_r, c->d_zparts, c->d_S, c->d_q, AmgXs0::ready);
    if (amg_comm_failed(c->amg)) {
      c->err = "collective failed inside the multigrid cycle";
      return SGO_ECOMM;
    }
    c->pcg_counts.n_rz = c->pcg_counts.n_zq = gz;
    Scope sc(c, K_UPDATE_P, 3 * 24.0 * c->n);
    launch_update_p(c->stream, c->n, c->d_S, c->d_zparts, gz, parts2 + kMaxPartials, g2, c->d_zparts + kMaxPartials,
                    c->d_z, c->d_p, rec_dev(c));
  } else {
    c->pcg_counts.n_rz = g2;
    c->pcg_counts.n_zq = 0;
    Scope sc(c, K_UPDATE_P, 3 * 24.0 * c->n);
    launch_update_p(c->stream, c->n, c->d_S, parts2, g2, parts2 + kMaxPartials, g2, nullptr, c->d_z, c->d_p, rec_dev(c));
  }
  c->pcg_counts.n_pq = g1;
  c->pcg_counts.n_rr = g2;
  return SGO_OK;
}

int ensure_pcg_graph(sgo_ctx* c, int chunk, bool* captured) {
  const int key = c->ov.active ? 1 : 0;
  if (captured) *captured = false;
  if (c->pcg_exec && c->pcg_exec_chunk == chunk && c->pcg_exec_key == key) return SGO_OK;
  if (captured) *captured = true;   // (attempted: every rank of a multi-GPU run gets here at the same solve)
  if (c->pcg_exec) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    hipGraphExecDestroy(c->pcg_exec);
    c->pcg_exec = nullptr;
  }
  hipGraph_t graph = nullptr;
  HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  int rc = SGO_OK;
  for (int k = 0; k < chunk && rc == SGO_OK; ++k) rc = pcg_iteration(c);
  hipError_t e = hipStreamEndCapture(c->stream, &graph);
  if (rc != SGO_OK) {
    if (graph) hipGraphDestroy(graph);
    return rc;
  }
  if (e != hipSuccess) {
    c->err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e);
    return SGO_EHIP;
  }
  e = hipGraphInstantiate(&c->pcg_exec, graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);
  if (e != hipSuccess) {
    c->pcg_exec = nullptr;
    c->err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
    return SGO_EHIP;
  }
  c->pcg_exec_chunk = chunk;
  c->pcg_exec_key = key;
  return SGO_OK;
}

void read_call_knobs(sgo_ctx* c) {
  sgo_ctx::CallKnobs k;
  if (const char* e = std::getenv("SGO_COMM_GRAPH")) k.comm_graph = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("SGO_PCG_STALL_WINDOW")) k.stall_window = std::max(0, std::atoi(e));
  if (const char* e = std::getenv("SGO_FIRST_SOLVE_CAP")) k.first_solve_cap = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("SGO_TEST_FAIL_TRIAL_BUILD")) k.fail_trial_build = std::atoi(e) != 0;
  if (const char* e = std::getenv("SGO_TEST_FAIL_DEVICE_SETUP")) k.fail_device_setup = std::atoi(e) != 0;
  if (const char* e = std::getenv("SGO_AMG_KEEP_AGG")) k.keep_agg = std::atoi(e) != 0;
  if (const char* e = std::getenv("SGO_AMG_SETUP")) k.setup_mode = std::string(e) == "host" ? 0 : (std::string(e) == "rebuilds" ? 1 : 2);
  if (const char* e = std::getenv("SGO_AMG_LISTS"))   // (test hook: product lists made on the host -- they belong to the host set-up)
    if (std::string(e) == "host") k.setup_mode = 0;
  if (const char* e = std::getenv("SGO_AMG_FORCE_REBUILD")) k.force_rebuild = std::atoi(e) != 0;
  if (const char* e = std::getenv("SGO_AMG_AGG")) k.dev_aggregation = std::string(e) == "device";
  if (const char* e = std::getenv("SGO_AMG_REBUILD_COST")) k.rebuild_cost = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("SGO_AMG_LAG")) k.lag_on = std::atoi(e) != 0;
  if (const char* e = std::getenv("SGO_AMG_LAG_TAU")) k.lag_tau = std::atof(e);
  if (const char* e = std::getenv("SGO_AMG_LAG_SLOPE")) k.lag_slope = std::atof(e);
  if (const char* e = std::getenv("SGO_AMG_LAG_FORCE")) k.lag_force_from = std::atoi(e);
  c->knobs = k;
}

// Runs PCG from the state k_finalize / start_pcg left (x = 0, r = b, ...) until S.stop != 0.
// Graph mode: a 2-iteration hipGraph is replayed; the first 0.8 * predicted - 4 iterations -- predicted
// = the count of the previous solve -- go out without any host check, after that one replay is always
// in flight while the host waits for the stop flag copied out after the previous one (kernels of
// iterations past convergence exit on the flag), so the GPU never idles on a host round trip and at
// most two replays of early-exit launches are wasted.
int run_pcg(sgo_ctx* c) {
  // Multi-GPU with an RCCL communicator: the collectives are captured into the hipGraph with the kernels around them (every
  // rank replays the same graph the same number of times: the replay count follows snapshots of the device-resident stop flag
  // taken at fixed points of the stream, bit-identical on all ranks; the exchanges of the set-up and of the solve's start have
  // run eagerly before, so the communicator's channels exist when the capture begins).  Measured with a 1-rank communicator
  // on C4: 191 -> 203 M edge-Jacobians/s.  Not possible with the host transport (a host callback inside the loop).
  // DEFAULT: on for a 1-rank communicator (the measured case: no peer to wait for), OFF for nranks > 1 -- RCCL with more than
  // one rank has never executed on this code (no multi-GPU node: DESIGN.md section 6), and a hang there would cost the whole
  // run; SGO_COMM_GRAPH=1 opts in, =0 opts out.  Whether the capture worked is decided COLLECTIVELY (an eager all-reduce of
  // the ranks' failure flags right after the attempt): ranks that replay graphs and ranks that launch plainly would issue
  // different numbers of collectives per solve and hang each other, so either all ranks replay or all fall back.
  bool comm_graph = c->comm.handle != nullptr && !c->comm.host_fn && !c->comm_graph_failed && c->comm.nranks <= 1;
  if (c->knobs.comm_graph >= 0)
    comm_graph = c->comm.handle != nullptr && !c->comm.host_fn && !c->comm_graph_failed && c->knobs.comm_graph != 0;
  // Stagnation guard (single GPU: the decision reads a clock-free but rank-local snapshot): a solve whose r.r has not reached a new
  // minimum for max(3000, 30 x the previous solve's count) iterations is ended as one that ran out of iterations -- the systems
  // PCG cannot finish in double precision otherwise grind on to pcg_maxit, three times per call.
  c->pcg_stalled = false;
  c->pcg_stall_window = multi_rank(c) ? 0 : std::max(3000, 30 * std::max(1, c->pcg_pred));
  // (once a solve of this call has been accepted at the floating-point floor of its system -- optimize_gn, solve_backward_error --
  // the call is at the edge of double precision: its later solves wait a tenth as long before they are looked at)
  if (c->call.floor_seen && c->pcg_stall_window > 0) c->pcg_stall_window = std::max(300, 3 * std::max(1, c->pcg_pred));
  if (c->knobs.stall_window >= 0) c->pcg_stall_window = multi_rank(c) ? 0 : c->knobs.stall_window;   // (test hook; 0: no guard)
  double stall_rr = -1.0;
  int stall_it = 0;
  auto stalled = [&](const volatile PcgScalars* S) -> bool {
    if (c->pcg_stall_window <= 0 || c->pcg_stalled) return false;
    const double rr = S->rr;
    const int it = S->iter;
    if (stall_rr < 0.0 || rr < stall_rr) {
      stall_rr = rr;
      stall_it = it;
      return false;
    }
    return it - stall_it > c->pcg_stall_window;
  };
  bool graph = c->opts.use_graph && !c->opts.profile && (!multi_rank(c) || comm_graph);
  constexpr int kUnit = 2;   // iterations per graph replay (1: 44.6, 2: 41.2, 4: 42, 8: 47 us per PCG iteration on C2 -- a replay costs
                             // ~7 us, an iteration past convergence eight early-exit nodes)
  if (graph) {
    bool attempted = false;
    const int grc = ensure_pcg_graph(c, kUnit, &attempted);
    if (multi_rank(c)) {
      int failed = grc != SGO_OK ? 1 : 0;
      if (attempted && c->comm.nranks > 1) {   // the ranks agree on the outcome before anyone replays
        if (!c->d_comm_flag) HIP_TRY(c, hipMalloc((void**)&c->d_comm_flag, sizeof(int)));
        HIP_TRY(c, hipMemcpyAsync(c->d_comm_flag, &failed, sizeof(int), hipMemcpyHostToDevice, c->stream));
        std::string cerr;
        if (!c->comm.allreduce_i32(c->d_comm_flag, 1, c->stream, &cerr)) {
          c->err = "all-reduce of the capture flags: " + cerr;
          return SGO_ECOMM;
        }
        HIP_TRY(c, hipMemcpyAsync(&failed, c->d_comm_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
      }
      if (failed) {
        if (c->pcg_exec) {   // (this rank's capture worked, another rank's did not)
          hipGraphExecDestroy(c->pcg_exec);
          c->pcg_exec = nullptr;
        }
        c->comm_graph_failed = true;
        graph = false;
        if (c->opts.verbose)
          std::fprintf(stderr, "[sgo] capturing the collectives failed on %d rank(s)%s%s: plain stream launches on all ranks from here on\n", failed,
                       grc != SGO_OK ? "; here: " : "", grc != SGO_OK ? c->err.c_str() : "");
      }
    } else if (grc != SGO_OK) {
      return grc;
    }
  }
  if (!graph) {
    // (profile mode: the stop flag is read after EVERY iteration, so that no early-exit launch past convergence is among
    // the timed launches -- their 1.5-us dispatches would pull the per-kernel figures down)
    const int chunk = c->opts.profile ? 1 : std::max(1, c->opts.pcg_chunk);
    for (;;) {
      HIP_TRY(c, hipMemcpyAsync(c->h_S, c->d_S, sizeof(PcgScalars), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      if (c->h_S->stop) break;
      if (stalled(c->h_S)) {
        c->pcg_stalled = true;
        launch_force_stop(c->stream, c->d_S, nullptr);
        continue;
      }
      for (int k = 0; k < chunk; ++k) {
        int rc = pcg_iteration(c);
        if (rc) return rc;
      }
    }
    c->pcg_pred = c->h_S->iter;
    return SGO_OK;
  }
  // One replay (2 iterations, >= 100 us even on 1k-pose graphs) in flight hides the host's read of the
  // stop flag; more only adds early-exit launches past convergence (measured: 8 iterations in flight
  // cost 3.5 % on C4 and 10 % on C1).  pcg_chunk = 16 -> 1 replay; larger values scale it up.
  const int chunk_launches = std::max(1, c->opts.pcg_chunk / 16);
  // unchecked prefix: 80 % of the previous count minus a margin (a solve that converges earlier
  // than that only wastes ~1 us per early-exit launch; tighter margins measured no different)
  const int pred = c->pcg_pred;
  const int unchecked = std::max(0, (int)(0.8 * pred) - 4) / kUnit;
  for (int k = 0; k < unchecked; ++k) HIP_TRY(c, hipGraphLaunch(c->pcg_exec, c->stream));
  // The stop flag is read from the pinned mirror every k_update_p rewrites (RecDev::mirror) behind an event: no copy kernel
  // between replays (4.3 us each on the stream, measured).  The mirror may already show the state of the replay in flight --
  // a later iteration of the same solve, equally valid; once a stop flag is set nothing moves any more.
  static const bool mirror_env = !(std::getenv("SGO_MIRROR") && std::atoi(std::getenv("SGO_MIRROR")) == 0);
  const bool mirror = mirror_env && !multi_rank(c) && !c->owner;   // (the multi-rank iterations do not pass the mirror: they keep the copy)
  int slot = 0;
  auto snapshot = [&](int sl) -> hipError_t {
    if (!mirror) {
      hipError_t e = hipMemcpyAsync(&c->h_S2[sl], c->d_S, sizeof(PcgScalars), hipMemcpyDeviceToHost, c->stream);
      if (e != hipSuccess) return e;
    }
    return hipEventRecord(c->ev_S[sl], c->stream);
  };
  if (mirror) {   // the start kernels' state (a solve may be over before its first iteration): one copy per solve
    HIP_TRY(c, hipMemcpyAsync(c->h_Sz, c->d_S, sizeof(PcgScalars), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, snapshot(slot));
  for (;;) {
    for (int k = 0; k < chunk_launches; ++k) HIP_TRY(c, hipGraphLaunch(c->pcg_exec, c->stream));  // speculative
    HIP_TRY(c, snapshot(slot ^ 1));
    HIP_TRY(c, hipEventSynchronize(c->ev_S[slot]));
    if (mirror ? ((volatile PcgScalars*)c->h_Sz)->stop : c->h_S2[slot].stop) break;
    if (stalled(mirror ? (volatile PcgScalars*)c->h_Sz : (volatile PcgScalars*)&c->h_S2[slot])) {
      c->pcg_stalled = true;
      launch_force_stop(c->stream, c->d_S, mirror ? c->d_Sz : nullptr);
    }
    slot ^= 1;
  }
  if (mirror) {
    HIP_TRY(c, hipEventSynchronize(c->ev_S[slot ^ 1]));   // (the replay in flight rewrites the mirror: let it finish before the final read)
    *c->h_S = *c->h_Sz;
    c->pcg_pred = c->h_S->iter;
    return SGO_OK;
  }
  *c->h_S = c->h_S2[slot];
  c->pcg_pred = c->h_S->iter;
  return SGO_OK;
}

int solve_from_linearization(sgo_ctx* c, bool run) {
  int rc, grid = 0;
  launch_finalize(c->stream, c->S0, c->owner ? c->halo.row0 : 0, c->owner ? c->halo.row1 : c->n, c->d_dgb, c->d_b, c->d_x, c->d_r,
                  c->d_z, c->d_p, c->amg ? amg_xs0(c->amg) : nullptr, c->amg ? amg_omega(c->amg) : 0.0, c->d_partials, &grid);
  if ((rc = start_pcg(c, grid))) return rc;
  if (run) return run_pcg(c);
  HIP_TRY(c, hipMemcpyAsync(c->h_S, c->d_S, sizeof(PcgScalars), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SGO_OK;
}

std::string multi_gpu_description(const sgo_ctx* c) {
  if (c->owner)
    return "; multi-GPU row-owner mode: rank " + std::to_string(c->halo.me) + " of " + std::to_string(c->halo.G) + " owns rows [" +
           std::to_string(c->halo.row0) + ", " + std::to_string(c->halo.row1) + "), largest boundary " + std::to_string(c->halo.bmax) + " rows";
  if (multi_rank(c)) return "; multi-GPU all-reduce mode (" + std::to_string(c->comm.nranks) + " ranks)";
  if (c->replicated) return "; multi-GPU: replicated on all " + std::to_string(c->comm.nranks) + " ranks (fewer level-0 work units than ranks)";
  return "";
}

// ---- build_amg's steps, in its order
// The hierarchy in use goes away, or -- a trial rebuild (keep_old) -- stays intact in its arena while the new one goes into the
// other.  *reuse_agg: the new set-up keeps its aggregates (host copies in c->kept_agg).
static int retire_hierarchy(sgo_ctx* c, bool keep_old, bool keep_agg, bool* reuse_agg) {
  // speculative replays of the captured PCG iteration (and the launches queued behind them) may still be
  // in flight: drain the stream before the exec and the old hierarchy's buffers go away
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->hier.new_hierarchy();   // (the lagged refresh's reference blocks belong to the old hierarchy's coarse operators)
  if (c->pcg_exec) {  // the captured PCG iteration references the old hierarchy's buffers
    hipGraphExecDestroy(c->pcg_exec);
    c->pcg_exec = nullptr;
  }
  c->pcg_pred = 0;  // the iteration count of the old hierarchy predicts nothing about the new one
  if (c->amg_prev) {   // (whatever an earlier trial kept is gone now)
    amg_destroy(c->amg_prev);
    c->amg_prev = nullptr;
  }
  if (keep_old && c->amg) {   // trial rebuild: the old hierarchy stays intact in its arena, the new one goes into the other
    c->amg_prev = c->amg;
    c->amg = nullptr;
    c->amg_prev_desc = c->solver_desc;
    std::swap(c->amg_arena.chunks, c->amg_arena_prev.chunks);
    std::swap(c->amg_arena.next_chunk, c->amg_arena_prev.next_chunk);
  }
  *reuse_agg = keep_agg && !keep_old && c->amg && !c->owner;
  if (*reuse_agg) amg_kept_aggregates(c->amg, &c->kept_agg);
  if (c->amg) {
    amg_destroy(c->amg);
    c->amg = nullptr;
  }
  c->amg_arena.rewind();
  return SGO_OK;
}

// Row-owner mode: a rank holds current blocks for its own rows only; the strength weights w0 of ALL level-0 slots come from the
// (replicated) edge list at the current poses, as in the set-up pipeline -- made here unless the helper thread has a result -- and
// the partition for amg_create
static int owner_inputs(sgo_ctx* c, std::vector<double>& w0, AmgHalo& ah) {
  if (!(c->l0_pre && amg_host_l0_ready(c->l0_pre))) {
    double* d_w = (double*)c->amg_arena.take(sizeof(double) * (size_t)std::max(c->H0.nslot, 1));
    if (!d_w) {
      c->err = "out of device memory";
      return SGO_ENOMEM;
    }
    launch_early_strength(c->stream, c->el, c->d_poses, c->n, c->d_rowptr, c->d_eidx, c->es.flags, c->d_hrowptr, d_w);
    w0.resize((size_t)c->H0.nslot);
    HIP_TRY(c, hipMemcpyAsync(w0.data(), d_w, sizeof(double) * w0.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  ah.dev = &c->halo;
  ah.G = c->halo_host.G;
  ah.bmax = c->halo_host.bmax;
  ah.bnd_host = c->halo_host.bnd.data();
  ah.user = c;
  ah.reserve = [](void* u, size_t doubles) { return halo_reserve((sgo_ctx*)u, doubles) == SGO_OK; };
  ah.w0 = &w0;
  return SGO_OK;
}

// c->amg from the device set-up where it applies, otherwise -- or when that cannot be made -- from the host set-up; nullptr: neither
// (the reason in aerr)
static void create_amg(sgo_ctx* c, const AmgConfig& cfg, const AmgHalo* ah, std::string& aerr) {
  AmgProf prof;
  prof.user = c;
  prof.begin = [](void* u, int kid, double bytes) {
    sgo_ctx* cc = (sgo_ctx*)u;
    cc->amg_scope = new Scope(cc, kid, bytes, kid == K_DENSE_INVERT);
  };
  prof.end = [](void* u) {
    sgo_ctx* cc = (sgo_ctx*)u;
    delete (Scope*)cc->amg_scope;
    cc->amg_scope = nullptr;
  };
  auto create = [&](AmgPatterns patterns, const AmgHalo* halo) {
    return amg_create(c->stream, c->A, c->S0, c->T0, c->H0, c->d_poses, c->d_free_id, cfg, prof, &aerr, &c->amg_scratch, &c->amg_arena,
                      &c->amg_tmp_arena, patterns, c->l0_pre, halo);
  };
  const double t_create0 = wall_s();
  const bool pre0_ready = c->l0_pre && amg_host_l0_ready(c->l0_pre);
  const bool pre0_agg = pre0_ready && amg_host_l0_agg_only(c->l0_pre);
  // The set-up ON THE DEVICE (sgo_amg_dev.inc): the rebuilds inside sgo_optimize_gn on one GPU (SGO_AMG_SETUP=host: the host
  // set-up for them too; =device: every set-up, sgo_set_graph_se2's included, whose level 0 the helper thread has not made ahead).
  const bool dev_setup = !c->owner && !multi_rank(c) && (pre0_agg || (!pre0_ready && (c->knobs.setup_mode == 2 || (c->knobs.setup_mode == 1 && c->call.in_optimize))));
  if (dev_setup) c->amg = create(c->knobs.dev_aggregation ? AmgPatterns::device_aggregation : AmgPatterns::device, nullptr);
  if (dev_setup && c->amg && c->knobs.fail_device_setup) {   // test hook (SGO_TEST_FAIL_DEVICE_SETUP): the device set-up "fails"
    amg_destroy(c->amg);
    c->amg = nullptr;
    aerr = "test hook";
  }
  if (dev_setup && !c->amg) {
    // (the device set-up could not be made -- out of device memory for its sort buffers, say --: the host set-up, which needs
    // none, before the graph is left to block-Jacobi; a helper thread's aggregation-only result is of no use to it)
    if (c->opts.verbose) std::fprintf(stderr, "[sgo] device set-up failed (%s): host set-up\n", aerr.c_str());
    c->amg_arena.rewind();
    aerr.clear();
  }
  if (!c->amg) c->amg = create(AmgPatterns::host, ah);
  l0_discard(c);
  if (c->opts.verbose)
    std::fprintf(stderr, "[sgo] multigrid set-up (%s): %.2f ms\n", dev_setup ? (c->knobs.dev_aggregation ? "aggregation and patterns on the device" : "host aggregation, patterns on the device") : "host", 1e3 * (wall_s() - t_create0));
}

// What solver_description says of the set-up's outcome (aerr: why there is no hierarchy)
static void describe_amg(sgo_ctx* c, const std::string& aerr) {
  if (c->amg) {
    // (a graph on the single-launch direct or the multifrontal path gets here through a single-step entry point -- sgo_linearize,
    // sgo_solve --: sgo_optimize_gn keeps running the factorisation, and the description keeps saying so)
    std::string amg_desc;
    amg_describe(c->amg, &amg_desc);
    if (c->direct || c->mf) {
      const size_t cut = c->solver_desc.find("; single-step entry points: ");
      if (cut != std::string::npos) c->solver_desc.resize(cut);
      c->solver_desc += "; single-step entry points: pcg_amg: " + amg_desc;
    } else {
      c->solver_desc = "pcg_amg: " + amg_desc;
      c->solver_desc += multi_gpu_description(c);
    }
  } else {
    if (c->direct || c->mf) c->solver_desc += "; single-step entry points: pcg_block_jacobi (AMG unavailable: " + aerr + ")";
    else c->solver_desc = "pcg_block_jacobi (AMG unavailable: " + aerr + ")";
    if (c->opts.verbose) std::fprintf(stderr, "[sgo] %s\n", c->solver_desc.c_str());
  }
}

// (Re)build the multigrid hierarchy from the CURRENT level-0 values (requires do_linearize).
int build_amg(sgo_ctx* c, bool keep_old, bool keep_agg) {
  bool reuse_agg = false;
  int rc = retire_hierarchy(c, keep_old, keep_agg, &reuse_agg);
  if (rc != SGO_OK) return rc;
  if (keep_old && c->amg_prev && c->knobs.fail_trial_build) {   // test hook (SGO_TEST_FAIL_TRIAL_BUILD, read once per sgo_optimize_gn): the trial's set-up "fails"
    c->solver_desc = "pcg_block_jacobi (AMG unavailable: test hook)";
    return SGO_OK;
  }
  AmgConfig cfg;
  cfg.theta_scale = c->hier.theta_scale;
  cfg.filtered_smoothing = !c->hier.no_filter;
  cfg.keep_agg = reuse_agg ? &c->kept_agg : nullptr;
  l0_join(c, true);   // the helper thread's analysis of level 0, when set_graph started one (first build only)
  AmgHalo ah;
  std::vector<double> w0;
  if (c->owner && (rc = owner_inputs(c, w0, ah)) != SGO_OK) return rc;
  std::string aerr;
  create_amg(c, cfg, c->owner ? &ah : nullptr, aerr);
  if (c->amg && amg_comm_failed(c->amg)) {
    c->err = "collective failed during the multigrid set-up";
    return SGO_ECOMM;
  }
  if (c->amg && !c->owner && multi_rank(c))
    amg_set_shard(c->amg, &c->comm, c->shard_u0, c->shard_u1, c->shard_row0, c->shard_row1, c->gather_slices ? &c->halo : nullptr);
  describe_amg(c, aerr);
  if (c->d_dref_agg && c->S0.dblk && !c->owner) {   // the blocks this aggregation was made from (optimize_gn's movement rule)
    HIP_TRY(c, hipMemcpyAsync(c->d_dref_agg, c->S0.dblk, sizeof(double) * 6 * (size_t)c->n, hipMemcpyDeviceToDevice, c->stream));
    c->hier.agg_ref_valid = true;
  }
  return SGO_OK;
}

// The hierarchy a trial rebuild made is dropped for the one it replaced (build_amg(c, true) kept it): the old one's values are
// refreshed by the next solve's amg_update like any other iteration's.  What the hierarchy state forgets with it
// (HierarchyState::reverted) is the caller's: CallPolicy applies it in order with the trial's verdict.
int revert_amg(sgo_ctx* c) {
  if (!c->amg_prev) return SGO_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->pcg_exec) {   // (the captured PCG iteration references the dropped hierarchy's buffers)
    hipGraphExecDestroy(c->pcg_exec);
    c->pcg_exec = nullptr;
  }
  if (c->amg) amg_destroy(c->amg);
  c->amg = c->amg_prev;
  c->amg_prev = nullptr;
  std::swap(c->amg_arena.chunks, c->amg_arena_prev.chunks);
  std::swap(c->amg_arena.next_chunk, c->amg_arena_prev.next_chunk);
  c->amg_arena_prev.rewind();
  c->solver_desc = c->amg_prev_desc;
  c->pcg_pred = 0;
  return SGO_OK;
}

// build_structure + what follows from it (multi-GPU tile range, tolerance rule)
int build_rows(sgo_ctx* c, const double* poses, const uint8_t* fixed, const int32_t* ei, const int32_t* ej) {
  int rc = build_structure(c, c->V, poses, fixed, c->E, ei, ej);
  if (rc != SGO_OK) return rc;
  c->shard_units = c->T0.ntile > 0 ? c->T0.ntile : c->S0.ngrp;
  // A graph with fewer work units than ranks (a few hundred poses on 8 GPUs) would leave some rank an EMPTY range, which the
  // level-0 kernels and the transfers read as "all" (u1 == 0 / row1 == 0): such a graph is not sharded at all -- every rank
  // runs the single-GPU computation on its own copy (same arithmetic: bit-identical ranks, no collective).
  c->replicated = (c->comm.nranks > 1 || c->comm.active()) && !c->owner && !c->gather_slices && c->shard_units < c->comm.nranks;
  if (c->replicated) {
    c->shard_u0 = c->shard_u1 = 0;
    c->shard_row0 = 0;
    c->shard_row1 = c->n;
  } else {
    sgo_shard_range(c->shard_units, c->comm.nranks, c->comm.rank, &c->shard_u0, &c->shard_u1);
    c->shard_row0 = c->unit_row0.empty() ? 0 : c->unit_row0[c->shard_u0];
    c->shard_row1 = c->unit_row0.empty() ? c->n : c->unit_row0[c->shard_u1];
  }
  // Chain-like graphs (fewer than ~1.5 edges per free pose: under 4 Hessian blocks per row) are the
  // ill-conditioned ones -- kappa(H) grows with the square of the chain length -- and a relative
  // residual of 1e-8 then leaves errors that show in chi2 (3000 poses / 3150 edges: iterates 3e-6 and
  // poses 7e-5 m from the direct-solver oracle at 1e-8, 1.4e-8 at 1e-9).  Their PCG iterations are the
  // cheap ones, so they get a 10x tighter tolerance than opts.pcg_tol.
  c->tol_scale = (c->n > 0 && (long long)c->A.nslot < 4LL * c->n) ? 0.1 : 1.0;   // logical slots: 2 per edge + 1 per row
  return SGO_OK;
}

// Graphs that optimize() through the single-launch direct path have their PCG-path structures built by the first
// entry point that needs them (sgo_linearize, sgo_hessian_apply, ...): the row order then follows the CURRENT poses.
int ensure_rows(sgo_ctx* c) {
  if (!c->rows_pending) return SGO_OK;
  std::vector<double> poses(3 * (size_t)c->V);
  HIP_TRY(c, hipMemcpyAsync(poses.data(), c->d_poses, sizeof(double) * poses.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int rc = build_rows(c, poses.data(), c->lz_fixed.data(), c->lz_ei.data(), c->lz_ej.data());
  if (rc != SGO_OK) return rc;   // (still pending: a later call tries again instead of running on half-built structures)
  c->rows_pending = false;
  c->lz_fixed = std::vector<uint8_t>();
  c->lz_ei = std::vector<int32_t>();
  c->lz_ej = std::vector<int32_t>();
  return rc;
}

// Graphs that optimize() through the single-launch direct path build their multigrid hierarchy only when a
// single-step entry point (sgo_solve, sgo_precondition) or the PCG fallback asks for it.
int ensure_amg(sgo_ctx* c) {
  int rc = ensure_rows(c);
  if (rc != SGO_OK) return rc;
  if (!c->amg_pending) return SGO_OK;
  if ((rc = do_linearize(c)) != SGO_OK || (rc = build_amg(c)) != SGO_OK) return rc;
  c->amg_pending = false;
  c->linearized = false;
  return SGO_OK;
}

// Vectors over the free vertices cross the API in g2o's hessian order and live on the device in the
// internal (Hilbert) row order: permute on the way (test / single-step entry points only).
int vec_to_device(sgo_ctx* c, const double* host_asc, double* dev) {
  std::vector<double> tmp(3 * (size_t)c->n);
  for (int i = 0; i < c->n; ++i)
    for (int q = 0; q < 3; ++q) tmp[3 * (size_t)c->row_of_asc[i] + q] = host_asc[3 * (size_t)i + q];
  HIP_TRY(c, hipMemcpyAsync(dev, tmp.data(), sizeof(double) * tmp.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SGO_OK;
}
int vec_from_device(sgo_ctx* c, const double* dev, double* host_asc) {
  std::vector<double> tmp(3 * (size_t)c->n);
  HIP_TRY(c, hipMemcpyAsync(tmp.data(), dev, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < c->n; ++i)
    for (int q = 0; q < 3; ++q) host_asc[3 * (size_t)i + q] = tmp[3 * (size_t)c->row_of_asc[i] + q];
  return SGO_OK;
}

int check_graph(sgo_ctx* c) {
  if (!c) return SGO_EINVAL;
  if (!c->has_graph) {
    c->err = "no graph: call sgo_set_graph_se2 first";
    return SGO_ENOGRAPH;
  }
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) {
    c->err = std::string("hipSetDevice: ") + hipGetErrorString(e);
    return SGO_EHIP;
  }
  return SGO_OK;
}

// The floor rule's backward error of the solve's current x (rules::floor_backward_error, sgo_rules.h: Jacobi-scaled, so one stiff
// row does not let a cut-off solve through).  A solve that stops making progress with eta at a few thousand units of roundoff has the
// solution double precision can give for this system -- a backward-stable direct solver (LinearSolverEigen's LDL^T, graphs.cpp:19)
// returns one of the same quality and g2o applies it --, whatever |r| / |b| says: seen from BASELINE.md's dead-reckoned start on large
// graphs with full information matrices, where undamped Gauss-Newton + DCS blows up (relative residuals of 10^-5 .. 10^-6 with x at
// the floor: NOTES.md section 29).  The residual is the TRUE one, r = b - H x with the PCG's own operator (do_spmv: the incremental
// overlay's U M U^T included), not the recurrence's.  Rare path -- only a solve that stopped short of pcg_tol comes here: one level-0
// product into q (free between solves: every PCG iteration recomputes it) and r, x, b and the diagonal blocks read on the host.
static int solve_backward_error(sgo_ctx* c, double* eta) {
  int rc = do_spmv(c, c->d_x, c->d_q, false, nullptr, nullptr);
  if (rc) return rc;
  const size_t n3 = 3 * (size_t)c->n;
  std::vector<double> hx(n3), hr(n3), hb(n3), hd(6 * (size_t)c->n);
  HIP_TRY(c, hipMemcpyAsync(hx.data(), c->d_x, sizeof(double) * n3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(hr.data(), c->d_q, sizeof(double) * n3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(hb.data(), c->d_b, sizeof(double) * n3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(hd.data(), c->S0.dblk, sizeof(double) * hd.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < n3; ++k) hr[k] = hb[k] - hr[k];
  *eta = rules::floor_backward_error(c->n, hr.data(), hx.data(), hb.data(), hd.data());
  if (c->opts.verbose) {
    // (with round 6's normwise measure beside it, |r_rec| / (2 max_i |D_i|_F |x| + |b|), for comparison)
    double xx = 0.0, rr = 0.0, dmax = 0.0;
    for (size_t k = 0; k < n3; ++k) {
      xx += hx[k] * hx[k];
      rr += hr[k] * hr[k];
    }
    for (int i = 0; i < c->n; ++i) {
      const double* d = hd.data() + 6 * (size_t)i;
      dmax = std::max(dmax, std::sqrt(d[0] * d[0] + 2 * d[1] * d[1] + 2 * d[2] * d[2] + d[3] * d[3] + 2 * d[4] * d[4] + d[5] * d[5]));
    }
    const double old_eta = std::sqrt(c->h_S->rr) / (2.0 * dmax * std::sqrt(xx) + std::sqrt(c->h_S->bb));
    std::fprintf(stderr, "[sgo] solve stopped without reaching pcg_tol: |r_rec| %.3e |b - Hx| %.3e |b| %.3e |x| %.3e max|D| %.3e: "
                 "scaled backward error %.2e (normwise, recurrence residual: %.2e)\n", std::sqrt(c->h_S->rr), std::sqrt(rr),
                 std::sqrt(c->h_S->bb), std::sqrt(xx), dmax, *eta, old_eta);
  }
  return SGO_OK;
}

// The chi2 history of the call's `done` iterations into sgo_stats (both paths).
static void copy_history(const sgo_ctx* c, int done, sgo_stats* out) {
  out->iters_done = done;
  for (int k = 0; k <= done; ++k) {
    out->chi2[k] = c->h_hist[2 * k];
    out->robust_chi2[k] = c->h_hist[2 * k + 1];
  }
}

// What every optimize call writes of sgo_stats before it starts.
void stats_begin(const sgo_ctx* c, int32_t iters, sgo_stats* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->iters_requested = iters;
  out->seconds_setup = c->setup_seconds;
}

// Small-graph path: the whole call is one launch (sgo_direct.h); mid-size path: one launch per level of the elimination tree and
// Gauss-Newton iteration, no host round trip inside the call (sgo_mfront.h).
// until (sgo_optimize_gn_until): the gain rule is applied on the device, no host round trip inside the call either.
static int optimize_factored(sgo_ctx* c, int32_t iters, sgo_stats* out, double t0, UntilGain* until) {
  hipError_t he;
  const double* tol = until ? &until->gain_tol : nullptr;
  if (c->direct) {
    Scope sc(c, K_DIRECT, direct_bytes(c->direct, c->E, iters));
    he = direct_optimize(c->direct, c->stream, c->el, c->d_poses, iters, c->d_hist, c->d_dres, tol);
  } else {
    Scope sc(c, K_MFRONT, mfront_bytes(c->mf, c->E, iters), true);
    he = mfront_optimize(c->mf, c->stream, c->el, c->d_poses, iters, c->d_hist, c->d_dres, tol);
  }
  if (he != hipSuccess) {
    c->err = std::string(c->direct ? "k_direct launch: " : "multifrontal launch: ") + hipGetErrorString(he);
    return SGO_EHIP;
  }
  HIP_TRY(c, hipMemcpyAsync(c->h_hist, c->d_hist, sizeof(double) * 2 * (size_t)(iters + 1), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_dres, c->d_dres, sizeof(DirectResult), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_flush(c);
  return factored_epilogue(c, iters, out, t0, until);
}

// What a finished call of a factorisation path leaves in its context, from the history in c->h_hist and the result record in
// c->h_dres (optimize_factored above; sgo_optimize_gn_many's shared launch, which puts each graph's two there): the stop reason, the
// error text of a failure, sgo_stats, the return value.
int factored_epilogue(sgo_ctx* c, int32_t iters, sgo_stats* out, double t0, UntilGain* until) {
  c->linearized = false;
  const DirectResult& R = *c->h_dres;
  const int done = R.done;
  if (until) until->stop_reason = R.fail ? SGO_STOP_FAILED : (done < iters ? SGO_STOP_GAIN : SGO_STOP_MAX_ITERS);
  const int ran = R.fail ? iters : done;   // (the stamps of a call that stopped are those of the call of `done` iterations)
  if (R.fail) {
    c->err = std::string(c->direct ? "direct" : "multifrontal") + " factorisation failed in GN iteration " + std::to_string(done) +
             (R.fail == 1 ? " (a pivot block is not positive definite: Hessian not positive definite)"
                          : " (non-finite update)") + "; the step was not applied";
  }
  if (out) {
    copy_history(c, done, out);
    const int timed = std::min(ran, done + (R.fail ? 1 : 0));
    for (int k = 0; k < timed; ++k) {
      out->pcg_iters[k] = 0;
      out->pcg_converged[k] = (k < done) ? 1 : 0;
      out->seconds_linearize[k] = 1e-8 * (double)(R.stamp[2 * k + 1] - R.stamp[2 * k]);
      out->seconds[k] = 1e-8 * (double)(R.stamp[2 * k + 2] - R.stamp[2 * k]);
      out->seconds_solve[k] = out->seconds[k] - out->seconds_linearize[k];
    }
    out->seconds_total = wall_s() - t0;
  }
  if (c->opts.verbose && done > 0 && c->direct)
    std::fprintf(stderr, "[sgo] direct: %.0f MHz shader clock during the call\n",
                 (double)R.cycles / (1e-2 * (double)(R.stamp[R.fail ? 2 * done + 2 : 2 * ran + 1] - R.stamp[0])));
  if (c->opts.verbose && done > 0 && c->direct)
    std::fprintf(stderr, "[sgo] direct, last iteration [us]: edges %.1f, assembly %.1f, sparse forward %.1f, separators %.1f + %.1f, "
                 "sparse backward %.1f, update %.1f\n", 1e-2 * (double)(R.phase[1] - R.phase[0]), 1e-2 * (double)(R.phase[2] - R.phase[1]),
                 1e-2 * (double)(R.phase[3] - R.phase[2]), 1e-2 * (double)(R.phase[4] - R.phase[3]), 1e-2 * (double)(R.phase[5] - R.phase[4]),
                 1e-2 * (double)(R.phase[6] - R.phase[5]), 1e-2 * (double)(R.phase[7] - R.phase[6]));
  if (c->opts.verbose > 1)
    for (int k = 0; k <= done; ++k)
      std::fprintf(stderr, "[sgo] iteration= %d\t chi2= %.9e\t robust= %.9e\t (%s)\n", k, c->h_hist[2 * k], c->h_hist[2 * k + 1], c->direct ? "direct" : "multifrontal");
  return R.fail ? 0 : done;
}

// chi2, buildSystem and the PCG start state of iteration `it`, with the set-up the policy asked for: the movement since the
// aggregation is measured in the call's first iteration, and a pending rebuild -- a re-aggregation trial's included -- is done here.
// until (sgo_optimize_gn_until): the gain rule is asked between the two -- the host reads this iteration's chi2 and the one before
// behind one small synchronisation, and a stop (*stopped) returns BEFORE the linearisation: no solve is started whose count would
// reach the policy or the hierarchy's state, and d_hist[2 it] is the call's final value (the closing do_chi2 rewrites the same sums).
static int linearize_step(sgo_ctx* c, CallPolicy& pol, int it, int iters, const UntilGain* until, bool* stopped) {
  if (pol.trial == CallPolicy::kTrialJudging || pol.rebuild_next) c->hier.ref_valid = false;   // (the trial's solves are fresh ones)
  int rc;
  if ((rc = do_chi2(c, c->d_hist + 2 * it, nullptr))) return rc;
  if (until && rules::gain_stop_applies(it, iters)) {
    HIP_TRY(c, hipMemcpyAsync(c->h_hist + 2 * (it - 1), c->d_hist + 2 * (it - 1), sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((*stopped = rules::gain_stop(c->h_hist[2 * it - 1], c->h_hist[2 * it + 1], until->gain_tol))) return SGO_OK;
  }
  if ((rc = do_linearize(c))) return rc;
  c->agg_grid = 0;
  if (it == 0 && c->amg && c->call.lag_on && c->hier.agg_ref_valid && !c->owner && iters > 1)   // (read behind the first solve's synchronisation)
    c->agg_grid = launch_diag_change(c->stream, 0, c->n, c->S0.dblk, c->d_dref_agg, false, c->h_dchg_dev + 3 * (size_t)kMaxPartials);
  if (!pol.rebuild_next || !c->amg) return SGO_OK;
  // Robust-kernel re-weighting has changed the strength of connection since the aggregation (CallPolicy::record): redo the set-up.
  if (pol.last_rebuild()) c->hier.no_filter = true;   // (the call's last rebuild: CallPolicy::abandon)
  const bool trial = pol.trial == CallPolicy::kTrialPending;
  rc = build_amg(c, trial, c->knobs.keep_agg);
  if (trial && c->amg_prev && (rc != SGO_OK || !c->amg) && rc != SGO_ECOMM) {
    // A TRIAL whose set-up did not come about (out of device memory -- a trial holds two hierarchies --, or the graph cannot be
    // coarsened at its current values): the parked hierarchy is intact and comes back.
    const std::string why = c->err;
    if ((rc = revert_amg(c))) return rc;
    pol.trial_failed(c->hier, why);
    c->err.clear();
    if (c->opts.verbose) std::fprintf(stderr, "[sgo] iteration %d: the trial set-up failed; the previous hierarchy is back\n", it);
    return do_linearize(c);
  }
  if (rc || (rc = do_linearize(c))) return rc;
  pol.rebuilt();
  if (c->opts.verbose) std::fprintf(stderr, "[sgo] multigrid hierarchy rebuilt before iteration %d\n", it);
  return SGO_OK;
}

// A solve that STAGNATED (run_pcg's guard) or ran out of iterations with x at the floating-point floor of its system: accepted,
// like a backward-stable direct solver's solution (solve_backward_error above).  Single GPU (the guard's domain).
int solve_at_floor(sgo_ctx* c, bool* accept, double* eta) {
  *accept = false;
  *eta = 1.0;
  if (!(c->h_S->stop == 2 && (c->pcg_stalled || c->h_S->iter >= c->opts.pcg_maxit) && !c->owner && !multi_rank(c))) return SGO_OK;
  const int rc = solve_backward_error(c, eta);
  if (rc) return rc;
  *accept = *eta <= rules::kFloorEta;
  return SGO_OK;
}
static int check_floor(sgo_ctx* c, CallPolicy& pol, int it, bool* accept) {
  if (*accept) return SGO_OK;
  double eta = 1.0;
  const int rc = solve_at_floor(c, accept, &eta);
  if (rc) return rc;
  if (*accept) {
    ++pol.floor_solves;
    c->call.floor_seen = true;
    if (c->opts.verbose)
      std::fprintf(stderr, "[sgo] iteration %d: the solve's x is at the floating-point floor of its system (scaled backward error %.1e <= %.0e): step applied\n", it, eta, rules::kFloorEta);
  }
  return SGO_OK;
}

// The hierarchy is re-made from the current values, the system linearised again and the solve repeated from x = 0 (`what`: why).
static int rebuild_and_solve(sgo_ctx* c, CallPolicy& pol, int it, bool keep_agg, const std::string& what, bool* floor_accept) {
  c->call.pcg_softcap = 0;
  int rc;
  if ((rc = build_amg(c, false, keep_agg)) || (rc = do_linearize(c)) || (rc = run_pcg(c))) return rc;
  pol.rebuilt();
  if (c->opts.verbose) std::fprintf(stderr, "[sgo] iteration %d: %s\n", it, what.c_str());
  return check_floor(c, pol, it, floor_accept);
}

// The solve of iteration `it` and its recoveries.  *wasted: the iterations of an abandoned solve; *interrupted: a solve behind kept
// coarse operators carried on behind refreshed ones; *floor_accept: the solve stands at the floating-point floor.
static int solve_step(sgo_ctx* c, CallPolicy& pol, int it, int* wasted, bool* interrupted, bool* floor_accept) {
  int rc;
  if ((rc = run_pcg(c))) return rc;
  const PcgScalars& S = *c->h_S;   // (what the latest run_pcg left)
  if (c->call.skip_update && c->amg && (S.stop == 4 || (S.stop == 2 && S.iter < c->opts.pcg_maxit && c->call.pcg_softcap > 0))) {
    // A solve behind KEPT coarse operators (lagged refresh) that its progress probe stopped -- half a decade behind the last fresh
    // solve after a third of its count -- or its cap, the fresh count + 3: the operators are refreshed and the solve carries on.
    const int at = S.iter;
    c->call.pcg_softcap = pol.continue_cap(c->hier, at);
    const int maxit = c->call.pcg_softcap > 0 ? std::min(c->call.pcg_softcap, c->opts.pcg_maxit) : c->opts.pcg_maxit;
    c->pcg_pred = std::max(2, pol.fresh_pcg);
    if ((rc = refresh_and_continue(c, maxit)) || (rc = run_pcg(c))) return rc;
    *interrupted = true;
    pol.kept_interrupted(c->hier, moved_rel(c, 0.0));
    if (c->opts.verbose)
      std::fprintf(stderr, "[sgo] iteration %d: solve behind kept coarse operators interrupted after %d PCG iterations, operators refreshed\n", it, at);
  }
  if ((rc = check_floor(c, pol, it, floor_accept))) return rc;
  if (!*floor_accept && c->call.pcg_softcap > 0 && S.stop == 2 && S.iter < c->opts.pcg_maxit && c->amg) {
    // The solve ran into the bail-out cap (4x the best count of this hierarchy): the aggregation no longer fits the re-weighted
    // Hessian -- rebuild and solve again instead of grinding on (seen: 735 iterations where the rebuilt hierarchy needs 16).
    *wasted = S.iter;
    pol.abandon(c->hier, amg_has_filtered(c->amg));
    const std::string what = "solve abandoned after " + std::to_string(*wasted) + " PCG iterations, hierarchy rebuilt";
    if ((rc = rebuild_and_solve(c, pol, it, c->knobs.keep_agg && c->hier.best != 0, what, floor_accept))) return rc;
  }
  if (!*floor_accept && S.stop == 3 && c->amg && amg_has_filtered(c->amg) && pol.can_rebuild()) {
    // A breakdown (p.Hp <= 0 or non-finite) behind FILTERED transfers: the Gauss-Newton Hessian is positive semi-definite, so the
    // preconditioner is the first suspect -- redone with tentative transfers, solved once more; an indefinite H fails again.
    *wasted += S.iter;
    c->hier.no_filter = true;
    return rebuild_and_solve(c, pol, it, false, "PCG breakdown behind a filtered hierarchy, rebuilt with tentative transfers and solved again", floor_accept);
  }
  return SGO_OK;
}

// The finished solve (no breakdown) into the call's policy, and what it says to do now: a lost trial's hierarchy goes back.
static int record_solve(sgo_ctx* c, CallPolicy& pol, int it, bool interrupted, bool floor_accept) {
  const PcgScalars& S = *c->h_S;
  double v[3];   // movement since the aggregation (measured in the call's first iteration)
  if (c->agg_grid > 0) sum_diag_change(c, 1, c->agg_grid, v);
  const SolveRecord r{it, S.iter, c->opts.pcg_tol * c->tol_scale, std::sqrt(S.tol2), c->call.skip_update, interrupted, floor_accept,
                      moved_rel(c, 0.0), S.probe_k, S.probe_rel, c->amg_prev != nullptr, c->agg_grid > 0 ? v : nullptr, c->n};
  c->agg_grid = 0;
  if (pol.record(c->hier, r, c->opts.verbose ? stderr : nullptr) != CallPolicy::kRevertTrial) return SGO_OK;
  if (const int rc = revert_amg(c)) return rc;
  if (c->opts.verbose)
    std::fprintf(stderr, "[sgo] iteration %d: the re-aggregated hierarchy is no better (%d against %d): the old one is back\n", it, pol.trial_best, pol.trial_old);
  return SGO_OK;
}

// Solver failure, as LinearSolverEigen::solve returning false (OptimizationAlgorithm::Fail): stop == 3: p.Hp <= 0 or non-finite
// (H not positive definite); stop == 2: pcg_maxit iterations without reaching pcg_tol (an inexact step is never applied).
static std::string failure_message(sgo_ctx* c, const PcgScalars& S, int it) {
  if (S.stop == 3)
    return "PCG breakdown in GN iteration " + std::to_string(it) + " (Hessian not positive definite" +
           (c->amg && amg_coarsest_not_spd(c->amg, c->stream) ? "; its coarsest Galerkin operator has a non-positive pivot" : "") + ")";
  return (c->pcg_stalled ? "PCG stagnated (no new minimum of the residual in the last " + std::to_string(c->pcg_stall_window) + " of " +
                               std::to_string(S.iter) + " iterations; pcg_maxit = "
                         : "PCG did not reach pcg_tol within pcg_maxit = ") + std::to_string(c->opts.pcg_maxit) +
         (c->pcg_stalled ? ")" : " iterations") + " in GN iteration " + std::to_string(it) + " (relative residual " +
         std::to_string(S.bb > 0 ? std::sqrt(S.rr / S.bb) : 0.0) + "); the step was not applied";
}

// g2o's optimize(iters) on the PCG path: per iteration linearise (with any rebuild the policy asked for),
// solve, recover, check the floor, record the solve in the call's policy (sgo_policy.h), then fail or apply the step.
// until != nullptr: sgo_optimize_gn_until -- the call ends before the first iteration at which rules::gain_stop holds (the
// factorisation paths decide on the device, this loop in linearize_step); the policy is built for `iters` either way.
int optimize_gn(sgo_ctx* c, int32_t iters, sgo_stats* out, UntilGain* until) {
  int rc = check_graph(c);
  if (rc) return rc;
  if (iters < 0 || iters > SGO_MAX_ITERS) {
    c->err = "sgo_optimize_gn: iters must be in [0, SGO_MAX_ITERS]";
    return SGO_EINVAL;
  }
  stats_begin(c, iters, out);
  if (c->n == 0) return SGO_ENOTHING;
  const double t0 = wall_s();
  read_call_knobs(c);
  if (until) until->stop_reason = SGO_STOP_MAX_ITERS;
  if (c->direct || c->mf) return optimize_factored(c, iters, out, t0, until);
  if ((rc = ensure_amg(c))) return rc;
  // per-iteration time stamps: events are kept in the context and reused by later calls
  while (c->iter_events.size() < 3 * (size_t)iters + 1) {
    hipEvent_t e = nullptr;
    HIP_TRY(c, hipEventCreate(&e));
    c->iter_events.push_back(e);
  }
  std::vector<hipEvent_t>& ev = c->iter_events;
  // the call's caps, accuracy target, warm start and lagged refresh apply to solves inside this call only
  struct CallScope { sgo_ctx* c; ~CallScope() { c->call = sgo_ctx::CallState(); } } call_scope{c};
  c->call = sgo_ctx::CallState();
  c->call.in_optimize = true;
  // Lagged refresh of the coarse operators (do_linearize): on by default on one GPU (the sharded modes, not exercised on hardware,
  // refresh before every solve); SGO_AMG_LAG=0 refreshes always.  The call's first solve always refreshes (HierarchyState::begin_call).
  c->call.lag_on = c->knobs.lag_on && !multi_rank(c);   // (replicated ranks: the whole single-GPU computation each)
  c->hier.begin_call(c->n, c->knobs.lag_slope);
  c->lag_note.clear();
  c->tol_cap = c->opts.pcg_tol_cap > 0.0 ? std::max(c->opts.pcg_tol_cap, c->opts.pcg_tol * c->tol_scale) : 0.0;
  CallPolicy pol(iters, c->knobs.rebuild_cost, c->knobs.force_rebuild && c->amg != nullptr);   // (test hook: a rebuild first)
  int done = 0;
  bool failed = false, stopped = false;
  for (int it = 0; it < iters; ++it) {
    hipEventRecord(ev[3 * it], c->stream);
    c->call.pcg_softcap = pol.solve_cap(c->hier, c->amg != nullptr, c->knobs.first_solve_cap);
    c->call.lag_cap = pol.lag_cap();
    c->call.force_keep = c->knobs.lag_force_from >= 0 && it > c->knobs.lag_force_from;   // (calibration hook, scripts/lag_calib.py)
    if ((rc = linearize_step(c, pol, it, iters, until, &stopped))) return rc;
    if (stopped) break;
    hipEventRecord(ev[3 * it + 1], c->stream);
    int wasted = 0;
    bool interrupted = false, floor_accept = false;
    if ((rc = solve_step(c, pol, it, &wasted, &interrupted, &floor_accept))) return rc;
    if (c->amg_dchg_pending) read_diag_change(c);   // (written before the solve began; the solve's end was waited for)
    // what the blocks moved by in this iteration, against the operators' reference: when they were refreshed now, the NEXT
    // iteration's movement against them will be about this iteration's one-step movement or less
    if (c->call.lag_on)
      c->call.lag_expect = c->hier.ref_valid && moved_rel(c, 1.0) <= 2.0 * lag_allowed(c) && c->last_dchg[2] <= 4.0 * rules::kLagRowsMoved;
    const PcgScalars S = *c->h_S;
    if (it == 0 && c->tol_cap > 0.0 && S.stop == 1) c->call.bb_ref = S.bb;
    if (c->amg && S.stop != 3 && (rc = record_solve(c, pol, it, interrupted, floor_accept))) return rc;
    if (it == 0 && S.stop == 1) {   // the call's first solve: what the incremental set-up's staleness rule compares (sgo_ctx.h)
      c->its_last = S.iter;
      if (!c->ov.active && c->its_base == 0) c->its_base = S.iter;
    }
    if (out) {
      out->pcg_iters[it] = S.iter + wasted;   // an abandoned solve's iterations count too
      out->pcg_converged[it] = S.stop == 1 ? 1 : (floor_accept ? 2 : 0);
      out->pcg_relres[it] = S.bb > 0 ? std::sqrt(S.rr / S.bb) : 0.0;
    }
    if (S.stop != 1 && !floor_accept) {   // the step is NOT applied; g2o::SparseOptimizer::optimize returns 0
      c->err = failure_message(c, S, it);
      failed = true;
      hipEventRecord(ev[3 * it + 2], c->stream);
      break;
    }
    // (row-owner mode: every rank holds all poses; the ranks' slices of the step are gathered first)
    if (c->owner && !halo_gather_slices(c->halo, c->stream, c->d_x, 3, &c->err)) return SGO_ECOMM;
    if (c->ov.active) launch_ov_finish(c->stream, c->ov.dev, c->d_x, c->d_poses);   // x_N and the appended poses' update
    {
      Scope sc(c, K_POSE_UPDATE, 72.0 * c->n);
      launch_pose_update(c->stream, c->n, c->d_free_id, c->d_x, c->d_poses);
    }
    if (c->opts.pcg_warm_start && c->amg && c->d_xprev) {   // (multi-GPU: the same replicated arithmetic on every rank)
      HIP_TRY(c, hipMemcpyAsync(c->d_xprev, c->d_x, sizeof(double) * 3 * (size_t)c->n, hipMemcpyDeviceToDevice, c->stream));
      c->call.warm_valid = !pol.rebuild_next;   // a rebuilt hierarchy starts cold (its first solve sets the reference counts)
    }
    hipEventRecord(ev[3 * it + 2], c->stream);
    c->linearized = false;
    ++done;
    if (c->opts.verbose)
      std::fprintf(stderr, "[sgo] iteration= %d\t pcg= %d\t relres= %.3e\t |b|= %.3e\t diag moved %.3e (%.0f rows > 1/4; kept up to %.1e)%s\n", it, S.iter,
                   S.bb > 0 ? std::sqrt(S.rr / S.bb) : 0.0, std::sqrt(S.bb), moved_rel(c, 0.0), c->last_dchg[2], lag_allowed(c),
                   c->call.skip_update ? " coarse operators kept" : "");
  }
  c->lag_note = pol.note(done);
  if (until) until->stop_reason = failed ? SGO_STOP_FAILED : (stopped ? SGO_STOP_GAIN : SGO_STOP_MAX_ITERS);
  if ((rc = do_chi2(c, c->d_hist + 2 * done, nullptr))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->h_hist, c->d_hist, sizeof(double) * 2 * (size_t)(done + 1), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->amg_prev && pol.trial == CallPolicy::kNoTrial) {   // a trial that was accepted: the replaced hierarchy goes; its arena keeps
    amg_destroy(c->amg_prev);                                // its chunks for the next trial (released and re-grown every time, the
    c->amg_prev = nullptr;                                   // chunk size doubled until each trial took a gigabyte)
    c->amg_arena_prev.rewind();
  }
  prof_flush(c);
  if (out) {
    copy_history(c, done, out);
    const int timed = std::min(iters, done + (stopped ? 0 : 1));   // (a stopped iteration has no solve to time)
    for (int k = 0; k < timed; ++k) {
      float a = 0.f, b = 0.f;
      hipEventElapsedTime(&a, ev[3 * k], ev[3 * k + 1]);
      hipEventElapsedTime(&b, ev[3 * k + 1], ev[3 * k + 2]);
      out->seconds_linearize[k] = a * 1e-3;
      out->seconds_solve[k] = b * 1e-3;
      out->seconds[k] = (a + b) * 1e-3;
    }
    out->seconds_total = wall_s() - t0;
  }
  return failed ? 0 : done;   // g2o: optimize() returns 0 when the algorithm reported Fail
}

// Micro-benchmark of the level-0 product on the resident graph: `reps` back-to-back launches of
// k_spmv0<mode> (operand = the PCG direction buffer, whatever it holds), HIP events around them on the
// context's stream; returns the mean microseconds per launch (< 0 on error).  variant 16: the wave-group kernel even when the graph has a tile view; variant 32: per-phase s_memtime stamps of the tile kernel on stderr (diagnostic).
double debug_spmv0_us(sgo_ctx* c, int mode, int variant, int reps) {
  if (check_graph(c) != SGO_OK || reps < 1 || c->n == 0 || ensure_rows(c) != SGO_OK || c->owner || c->ov.active) return -1.0;
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1.0;
  Spmv0Args args{};
  args.x = c->d_p;
  args.y = c->d_s2;
  args.b = c->d_b;
  args.omega = 0.8;
  args.force_f64 = (variant & 64) != 0;   // variant 64: RESID / JACOBI on the fp64 blocks although an fp32 copy exists
  const bool tiled = c->T0.ntile > 0 && !(variant & 16);   // variant 16: the wave-group kernel
  long long* d_st = nullptr;
  if ((variant & 32) && tiled) {
    hipMalloc((void**)&d_st, sizeof(long long) * 8 * (size_t)c->T0.ntile);
    hipMemset(d_st, 0, sizeof(long long) * 8 * (size_t)c->T0.ntile);
    args.dbg_stamps = d_st;
  }
  if (tiled) launch_spmv0t(c->stream, c->S0, c->T0, mode, args);
  else launch_spmv0(c->stream, c->S0, mode, args);
  if (variant & 128) {   // variant 128: as nodes of a replayed hipGraph (16 launches per graph), the way the solve runs them
    hipGraph_t g = nullptr;
    hipGraphExec_t ex = nullptr;
    hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    for (int k = 0; k < 16; ++k) {
      if (tiled) launch_spmv0t(c->stream, c->S0, c->T0, mode, args);
      else launch_spmv0(c->stream, c->S0, mode, args);
    }
    hipStreamEndCapture(c->stream, &g);
    if (!g || hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) return -1.0;
    hipGraphLaunch(ex, c->stream);
    hipEventRecord(a, c->stream);
    for (int k = 0; k < (reps + 15) / 16; ++k) hipGraphLaunch(ex, c->stream);
    hipEventRecord(b, c->stream);
    hipStreamSynchronize(c->stream);
    hipGraphExecDestroy(ex);
    hipGraphDestroy(g);
    reps = (reps + 15) / 16 * 16;
  } else {
  hipEventRecord(a, c->stream);
  for (int k = 0; k < reps; ++k) {
    if (tiled) launch_spmv0t(c->stream, c->S0, c->T0, mode, args);
    else launch_spmv0(c->stream, c->S0, mode, args);
  }
  hipEventRecord(b, c->stream);
  }
  hipStreamSynchronize(c->stream);
  float ms = 0.f;
  hipEventElapsedTime(&ms, a, b);
  hipEventDestroy(a);
  hipEventDestroy(b);
  if (d_st) {
    std::vector<long long> st(8 * (size_t)c->T0.ntile);
    hipMemcpy(st.data(), d_st, sizeof(long long) * st.size(), hipMemcpyDeviceToHost);
    hipFree(d_st);
    double ph[6] = {0, 0, 0, 0, 0, 0};
    for (int t = 0; t < c->T0.ntile; ++t)
      for (int q = 0; q < 6; ++q) ph[q] += (double)(st[8 * t + q + 1] - st[8 * t + q]);
    std::fprintf(stderr, "[sgo] tile kernel phases, shader cycles of wave 0 (s_memtime), mean over %d tiles: phase 0 %.0f, barrier %.0f, "
                 "phase 1 %.0f, barrier %.0f, phase 2 %.0f, barrier %.0f\n", c->T0.ntile,
                 ph[0] / c->T0.ntile, ph[1] / c->T0.ntile, ph[2] / c->T0.ntile, ph[3] / c->T0.ntile, ph[4] / c->T0.ntile,
                 ph[5] / c->T0.ntile);
    long long s0 = st[0], s1 = st[0], e0 = st[6], e1 = st[6], dmin = st[6] - st[0], dmax = dmin;
    double dsum = 0.0;
    for (int t = 0; t < c->T0.ntile; ++t) {
      const long long a0 = st[8 * t], a6 = st[8 * t + 6], dd = a6 - a0;
      s0 = std::min(s0, a0); s1 = std::max(s1, a0); e0 = std::min(e0, a6); e1 = std::max(e1, a6);
      dmin = std::min(dmin, dd); dmax = std::max(dmax, dd); dsum += (double)dd;
    }
    std::fprintf(stderr, "[sgo] tile kernel, per tile (wave 0): cycles min %lld mean %.0f max %lld; first stamps spread over %lld cycles, "
                 "last stamps over %lld; first start to last end %lld cycles\n", dmin, dsum / c->T0.ntile, dmax, s1 - s0, e1 - e0, e1 - s0);
  }
  return 1e3 * ms / reps;
}

}  // namespace sgo
