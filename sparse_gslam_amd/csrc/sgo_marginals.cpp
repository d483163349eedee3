// sgo_marginals.cpp -- sgo_marginals and sgo_solve_rhs (include/sgo.h): blocks of H^-1, and H x = b for the caller's b, with the
// level-0 PCG machinery of the single-step entry points.  No factorisation of its own: a block column of H^-1 is three solves of
// unit right-hand sides (kernels in sgo_marginals.hip), the loop per column is
//   inject -> launch_finalize -> start_pcg -> run_pcg -> gather        (solve_from_linearization, sgo_solve.cpp)
// The Hessian does not change between the columns of a call: the linearisation refreshes the hierarchy's coarse operators once and
// every column runs behind them (call.skip_update), cold, at pcg_tol relative to its own right-hand side, without soft cap or probe.
#include <algorithm>
#include <cmath>

#include "sgo_ctx.h"

using namespace sgo;

namespace {

const char* const kOverlayRefusal =
    "single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";

void inject(sgo_ctx* c, double* save, const double* src, int unit_row, int unit_k) {
  Scope sc(c, K_RHS_INJECT, (src ? 48.0 : 24.0) * c->n + (save ? 48.0 : 0.0) * c->n);
  launch_rhs_inject(c->stream, c->n, c->d_dgb, save, src, unit_row, unit_k);
}
void restore(sgo_ctx* c, const double* save) {
  Scope sc(c, K_RHS_RESTORE, 48.0 * c->n);
  launch_rhs_restore(c->stream, c->n, c->d_dgb, save);
}

// The three unit columns of the free vertex `vertex` (internal row `row`), gathered for the pairs order[q0 .. q1).  The
// linearisation's own b sits in d_s2 after the first injection (*saved).  *failed: a column neither reached pcg_tol nor stands at
// the floating-point floor (c->err says which).
int solve_columns(sgo_ctx* c, int vertex, int row, int q0, int q1, const int* d_order, const int* d_pair_row, bool* saved, bool* failed) {
  for (int k = 0; k < 3; ++k) {
    inject(c, *saved ? nullptr : c->d_s2, nullptr, row, k);
    *saved = true;
    int rc = solve_from_linearization(c, true);
    if (rc) return rc;
    const PcgScalars& S = *c->h_S;
    bool ok = S.stop == 1;
    double eta = 1.0;
    if (!ok && (rc = solve_at_floor(c, &ok, &eta))) return rc;
    if (!ok) {
      const double rel = S.bb > 0 ? std::sqrt(S.rr / S.bb) : 0.0;
      char buf[64];
      std::snprintf(buf, sizeof buf, "%.3e", rel);
      c->err = "sgo_marginals: column " + std::to_string(k) + " of vertex " + std::to_string(vertex) +
               (S.stop == 3 ? " broke down (Hessian not positive definite)" : " did not reach pcg_tol") + " after " + std::to_string(S.iter) +
               " PCG iterations (relative residual " + buf + ")";
      *failed = true;
      return SGO_OK;
    }
    Scope sc(c, K_COV_GATHER, 40.0 * (q1 - q0));
    launch_cov_gather(c->stream, q0, q1, d_order, d_pair_row, row, k, c->n, c->d_x, c->marg.d_cov);
  }
  return SGO_OK;
}

}  // namespace

extern "C" {

int sgo_solve_rhs(sgo_ctx* c, const double* b, double* x, double* relres) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (c->ov.active) {
      c->err = kOverlayRefusal;
      return SGO_EINVAL;
    }
    if (!c->linearized) {
      c->err = "sgo_solve_rhs: call sgo_linearize first";
      return SGO_EINVAL;
    }
    if (!b) {
      c->err = "sgo_solve_rhs: null right-hand side";
      return SGO_EINVAL;
    }
    for (size_t k = 0; k < 3 * (size_t)c->n; ++k)
      if (!std::isfinite(b[k])) {
        c->err = "sgo_solve_rhs: non-finite entry in the right-hand side (hessian index " + std::to_string(k / 3) + ")";
        return SGO_EINVAL;
      }
    read_call_knobs(c);
    if ((rc = vec_to_device(c, b, c->d_s1))) return rc;
    inject(c, c->d_s2, c->d_s1, -1, 0);
    rc = solve_from_linearization(c, true);
    restore(c, c->d_s2);   // (the linearisation's own b is back whatever the solve did)
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    if (c->owner && !halo_gather_slices(c->halo, c->stream, c->d_x, 3, &c->err)) return SGO_ECOMM;
    if (x && (rc = vec_from_device(c, c->d_x, x))) return rc;
    if (relres) *relres = c->h_S->bb > 0 ? std::sqrt(c->h_S->rr / c->h_S->bb) : 0.0;
    if (c->h_S->stop == 3) {
      c->err = "PCG breakdown (p.Hp <= 0 or non-finite): Hessian not positive definite";
      return SGO_EINVAL;
    }
    return c->h_S->iter;
  } SGO_CATCH(c)
}

int sgo_marginals(sgo_ctx* c, int32_t npairs, const int32_t* vi, const int32_t* vj, double* cov) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (npairs < 0 || (npairs > 0 && (!vi || !vj || !cov))) {
      c->err = "sgo_marginals: null buffer or negative count";
      return SGO_EINVAL;
    }
    if (c->ov.active) {
      c->err = kOverlayRefusal;
      return SGO_EINVAL;
    }
    if (multi_gpu_context(c)) {
      c->err = "sgo_marginals: not available in a multi-GPU context";
      return SGO_EINVAL;
    }
    // hessian index of a free active vertex, -1 for a fixed active one; anything else is refused
    auto hessian_index = [&](int v, int* h) {
      const auto f = std::lower_bound(c->free_id.begin(), c->free_id.end(), v);
      if (f != c->free_id.end() && *f == v) {
        *h = (int)(f - c->free_id.begin());
        return true;
      }
      *h = -1;
      return std::binary_search(c->fixed_active.begin(), c->fixed_active.end(), v);
    };
    std::vector<int> hi((size_t)npairs), hj((size_t)npairs);
    for (int t = 0; t < npairs; ++t)
      for (int side = 0; side < 2; ++side) {
        const int v = side ? vj[t] : vi[t];
        if (v < 0 || v >= c->V) {
          c->err = "sgo_marginals: vertex id " + std::to_string(v) + " outside [0, " + std::to_string(c->V) + ")";
          return SGO_EINVAL;
        }
        if (!hessian_index(v, side ? &hj[t] : &hi[t])) {
          c->err = "sgo_marginals: vertex " + std::to_string(v) + " is not active (it has no edge)";
          return SGO_EINVAL;
        }
      }
    if (npairs == 0) return 0;
    if (c->n == 0) {   // every active vertex is fixed: zero blocks, nothing to linearise
      std::fill(cov, cov + 9 * (size_t)npairs, 0.0);
      return 0;
    }
    // the system at the current poses, as sgo_linearize makes it (a graph on a factorisation path builds its PCG structures now)
    if ((rc = ensure_amg(c))) return rc;
    read_call_knobs(c);
    RestoreCall restore_call(c);
    c->call = sgo_ctx::CallState();
    c->hier.probe_k = 0;
    c->hier.probe_max = 0.0;
    if ((rc = do_chi2(c, c->d_hist, nullptr)) || (rc = do_linearize(c))) return rc;   // (the call's one refresh of the coarse operators)
    c->call.skip_update = true;

    // pairs with two free vertices, ordered by column vertex (stable: the caller's order within a column)
    std::vector<int> pair_row((size_t)npairs, -1), order;
    for (int t = 0; t < npairs; ++t)
      if (hi[t] >= 0 && hj[t] >= 0) {
        pair_row[t] = c->row_of_asc[hi[t]];
        order.push_back(t);
      }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hj[a] < hj[b]; });
    sgo_ctx::Marginals& M = c->marg;
    if ((rc = grow_device(c, &M.d_cov, &M.cov_cap, 9 * (size_t)npairs)) || (rc = grow_device(c, &M.d_idx, &M.idx_cap, 2 * (size_t)npairs))) return rc;
    int* d_pair_row = M.d_idx;
    int* d_order = M.d_idx + npairs;
    HIP_TRY(c, hipMemsetAsync(M.d_cov, 0, sizeof(double) * 9 * (size_t)npairs, c->stream));   // (a pair with a fixed vertex: the zero block)
    HIP_TRY(c, hipMemcpyAsync(d_pair_row, pair_row.data(), sizeof(int) * (size_t)npairs, hipMemcpyHostToDevice, c->stream));
    if (!order.empty())
      HIP_TRY(c, hipMemcpyAsync(d_order, order.data(), sizeof(int) * order.size(), hipMemcpyHostToDevice, c->stream));

    int solves = 0;
    bool saved = false, failed = false;
    for (size_t q0 = 0; q0 < order.size() && rc == SGO_OK && !failed;) {
      const int h = hj[order[q0]];
      size_t q1 = q0;
      while (q1 < order.size() && hj[order[q1]] == h) ++q1;
      rc = solve_columns(c, c->free_id[h], c->row_of_asc[h], (int)q0, (int)q1, d_order, d_pair_row, &saved, &failed);
      solves += 3;
      q0 = q1;
    }
    // the linearisation's own right-hand side and its start state again: the context is as after sgo_linearize
    if (saved) {
      restore(c, c->d_s2);
      const int rc2 = solve_from_linearization(c, false);
      if (rc == SGO_OK) rc = rc2;
    }
    if (rc == SGO_OK && hipGetLastError() != hipSuccess) {
      c->err = "sgo_marginals: kernel launch failed";
      rc = SGO_EHIP;
    }
    if (rc) return rc;
    if (failed) return SGO_EINVAL;
    HIP_TRY(c, hipMemcpyAsync(cov, M.d_cov, sizeof(double) * 9 * (size_t)npairs, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return solves;
  } SGO_CATCH(c)
}

}  // extern "C"
