// sgo_fsolve.cpp -- sgo_factor_solve, sgo_candidate_gate and the joint table's calls (include/sgo.h; DESIGN.md sections 5g, 5j):
// H X = B for panels of 16 right-hand sides through the multifrontal factor (kernels in sgo_fsolve.hip), and on top of it the innovation gate for candidate
// edges -- d2 = e^T (Omega^-1 + J Sigma J^T)^-1 e from three right-hand sides per candidate and no block of Sigma at all.  One call is
//   factor phase at the current poses (mfront_factorize: the multifrontal path's own launches) ->
//   per chunk of kFsChunkPanels panels: right-hand sides -> forward pass per level, bottom-up -> backward pass per level, top-down
//   (-> the gate's 3 x 3 arithmetic per candidate) -> one copy to the host.
// The plan is the one sgo_marginals_selected works through (selinv_plan: the resident one, or one analysed once per set-up); like
// that call this one writes only what every Gauss-Newton iteration recomputes from the poses, and scratch.  On a graph the analysis
// refuses sgo_candidate_gate sends the same right-hand sides through the PCG machinery of sgo_solve_rhs under sgo_marginals' rules.
// sgo_candidate_joint is the gate's driver with another contraction: the same checks (check_candidates) and
// the same columns (cand_columns), every chunk contracted with ALL candidates' records into the stacked innovation covariance S,
// which stays in the context (sgo_ctx::Joint) for sgo_joint_subsets / sgo_joint_pairs.  sgo_edge_joint is
// that driver again for RESIDENT edges: the records' sources filled on the device (edge_columns), the same columns and Gram blocks,
// a table of its own (sgo_ctx::EdgeJoint) for sgo_edge_groups (sgo_egroup.cpp).
#include <algorithm>
#include <cmath>

#include "sgo_ctx.h"
#include "sgo_mfront_dev.h"

using namespace sgo;

namespace {

const char* const kOverlayRefusal =
    "single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";

// what both entry points refuse before they look at their arguments' contents
int refuse_context(sgo_ctx* c, const char* who) {
  if (c->ov.active) {
    c->err = kOverlayRefusal;
    return SGO_EINVAL;
  }
  if (multi_gpu_context(c)) {
    c->err = std::string(who) + ": not available in a multi-GPU context";
    return SGO_EINVAL;
  }
  return SGO_OK;
}

}  // namespace

// The substitution's own device arrays, once per plan: the extend-add maps, every front's place in a panel's update buffer and
// the hessian index of every elimination position.  (These three are sgo_closure_search's too: sgo_search.cpp.)
int sgo::fs_prepare(sgo_ctx* c, Mfront* m, const char* who) {
  if (m->fs_ready) return SGO_OK;
  if (!fs_prepare_device()) {
    c->err = std::string(who) + ": the device does not grant the kernels' dynamic LDS";
    return SGO_EHIP;
  }
  int rc;
  if ((rc = mfront_maps_prepare(c, m))) return rc;
  const MfPlan& P = m->plan;
  std::vector<int> uoff(std::max<size_t>(P.fronts.size(), 1), 0), pos_h((size_t)std::max(P.n, 1), 0);
  int U3 = 0;
  for (size_t f = 0; f < P.fronts.size(); ++f) {
    uoff[f] = U3;
    U3 += 3 * P.fronts[f].nb;
  }
  for (int p = 0; p < P.n; ++p)
    pos_h[p] = (int)(std::lower_bound(c->free_id.begin(), c->free_id.end(), P.elim_vertex[p]) - c->free_id.begin());
  int *d_uoff = nullptr, *d_ph = nullptr;
  if ((rc = upload(c, &d_uoff, uoff)) || (rc = upload(c, &d_ph, pos_h))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the host vectors above go out of scope)
  m->fs.uoff = d_uoff;
  m->fs.pos_h = d_ph;
  m->fs.U3 = U3;
  m->fs_ready = true;
  return SGO_OK;
}

// One chunk's scratch: the panel after the forward pass (it holds the right-hand sides before), after the backward pass, and the
// fronts' update buffers, all for `panels` panels.
int sgo::fs_scratch(sgo_ctx* c, int n3, int U3, int panels, FsScratch* S) {
  const size_t vec = (size_t)panels * kMfPanel * (size_t)n3, upd = (size_t)panels * kMfPanel * (size_t)U3;
  sgo_ctx::SelInv& Z = c->selinv;
  int rc;
  if ((rc = grow_device(c, &Z.d_fs, &Z.fs_cap, 2 * vec + upd + 1))) return rc;
  S->Y = Z.d_fs;
  S->X = Z.d_fs + vec;
  S->U = Z.d_fs + 2 * vec;
  return SGO_OK;
}

// Both passes over the factor for the `panels` panels whose right-hand sides sit in S.Y
void sgo::fs_passes(sgo_ctx* c, Mfront* m, const FsScratch& S, int panels, int ncols) {
  const MfPlan& P = m->plan;
  const int n3 = 3 * P.n;
  const double pass_bytes = 8.0 * (double)P.arena_doubles * panels + 16.0 * kMfPanel * (double)panels * ((double)n3 + m->fs.U3);
  for (int h = 0; h <= P.height; ++h) {
    Scope sc(c, K_FS_FORWARD, pass_bytes / (P.height + 1));
    launch_fs_forward(c->stream, m->dev, m->sel, m->fs, P.level_ptr[h], P.level_ptr[h + 1] - P.level_ptr[h], panels, (size_t)m->level_lds[h], S.Y,
                      S.U, n3);
  }
  for (int h = P.height; h >= 0; --h) {
    Scope sc(c, K_FS_BACKWARD, pass_bytes / (P.height + 1));
    launch_fs_backward(c->stream, m->dev, P.level_ptr[h], P.level_ptr[h + 1] - P.level_ptr[h], panels, (size_t)m->level_lds[h], S.Y, S.X, n3);
  }
  m->fs_Y = S.Y;
  m->fs_X = S.X;
  m->fs_cols = ncols;
}

namespace {

int factorize(sgo_ctx* c, Mfront* m) {
  Scope sc(c, K_MF_FACTOR, mfront_bytes(m, c->E, 1), true);
  HIP_TRY(c, mfront_factorize(m, c->stream, c->el, c->d_poses, c->d_hist, c->d_dres));
  return SGO_OK;
}

const char* const kNotPd = ": the factorisation failed (a pivot block is not positive definite: Hessian not positive definite)";

// The candidates on the device: endpoints, rows, inverse measurements and information (k_edge_prepare, as a graph's edges), records
// and results.  row[t][side]: the pose's place in a right-hand side, -1 for a fixed endpoint.
int cand_upload(sgo_ctx* c, int n, const int32_t* ci, const int32_t* cj, const std::vector<int>& row, const double* meas, const double* info,
                FsCandDev* C, double** d_out) {
  sgo_ctx::SelInv& Z = c->selinv;
  const size_t N = (size_t)n;
  int rc;
  if ((rc = grow_device(c, &Z.d_cand, &Z.cand_cap, (3 + 6 + 3 + 6 + kFsRec + kFsOut) * N + 1)) || (rc = grow_device(c, &Z.d_cidx, &Z.cidx_cap, 4 * N)))
    return rc;
  double* d_meas = Z.d_cand;
  double* d_info = d_meas + 3 * N;
  double* d_zinv = d_info + 6 * N;
  double* d_soa = d_zinv + 3 * N;
  double* d_rec = d_soa + 6 * N;
  *d_out = d_rec + kFsRec * N;
  int* d_vi = Z.d_cidx;
  int* d_vj = d_vi + N;
  int* d_row = d_vj + N;
  HIP_TRY(c, hipMemcpyAsync(d_vi, ci, sizeof(int) * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_vj, cj, sizeof(int) * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_row, row.data(), sizeof(int) * 2 * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_meas, meas, sizeof(double) * 3 * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_info, info, sizeof(double) * 6 * N, hipMemcpyHostToDevice, c->stream));
  launch_edge_prepare(c->stream, n, d_meas, d_info, d_zinv, d_soa, N, 0);
  C->n = n;
  C->vi = d_vi;
  C->vj = d_vj;
  C->row = d_row;
  C->zinv = d_zinv;
  C->info = d_soa;
  C->rec = d_rec;
  return SGO_OK;
}

constexpr int kChunkCands = kFsChunkPanels * kMfPanel / 3;   // candidates per chunk: three columns each, packed

// The analysis refuses the graph: the candidates' right-hand sides through the PCG, one solve per column under sgo_marginals' rules
// (cold, pcg_tol relative to the column's own norm, the floor rule, one refresh of the coarse operators per call).  The columns
// are made and contracted by the same kernels, with the poses' hessian indices as their rows.
template <class Use>
int gate_by_pcg(sgo_ctx* c, const char* name, int n, const FsCandDev& C, const std::vector<int>& row, const int32_t* ci, const int32_t* cj, Use&& use) {
  int rc;
  if ((rc = ensure_amg(c))) return rc;
  read_call_knobs(c);
  RestoreCall restore_call(c);
  c->call = sgo_ctx::CallState();
  c->hier.probe_k = 0;
  c->hier.probe_max = 0.0;
  if ((rc = do_chi2(c, c->d_hist, nullptr)) || (rc = do_linearize(c))) return rc;   // (the call's one refresh of the coarse operators)
  c->call.skip_update = true;
  const int n3 = 3 * c->n;
  // (whole vectors per column here, on graphs of any size: a chunk holds at most 2^25 doubles per buffer)
  const int chunk = (int)std::max<long long>(1, std::min<long long>(std::min(n, kChunkCands), ((long long)1 << 25) / (3LL * n3)));
  FsScratch S;
  if ((rc = fs_scratch(c, n3, 0, (3 * chunk + kMfPanel - 1) / kMfPanel, &S))) return rc;
  std::vector<double> cols, sols;
  bool saved = false, failed = false;
  for (int t0 = 0; t0 < n && rc == SGO_OK && !failed; t0 += chunk) {
    const int t1 = std::min(n, t0 + chunk), nc = 3 * (t1 - t0);
    const size_t bytes = sizeof(double) * (size_t)nc * n3;
    HIP_TRY(c, hipMemsetAsync(S.Y, 0, bytes, c->stream));
    {
      Scope sc(c, K_FS_RHS, 8.0 * (kFsRec + 18) * (t1 - t0));
      launch_fs_rhs_candidates(c->stream, C, t0, t1, c->d_poses, n3, S.Y);
    }
    cols.resize((size_t)nc * n3);
    sols.assign((size_t)nc * n3, 0.0);
    HIP_TRY(c, hipMemcpyAsync(cols.data(), S.Y, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < nc && !failed; ++k) {
      const int t = t0 + k / 3;
      if (row[2 * (size_t)t] < 0 && row[2 * (size_t)t + 1] < 0) continue;   // both endpoints fixed: the zero column
      if ((rc = vec_to_device(c, cols.data() + (size_t)k * n3, c->d_s1))) break;
      {
        Scope sc(c, K_RHS_INJECT, 48.0 * c->n + (saved ? 0.0 : 48.0) * c->n);
        launch_rhs_inject(c->stream, c->n, c->d_dgb, saved ? nullptr : c->d_s2, c->d_s1, -1, 0);
      }
      saved = true;
      if ((rc = solve_from_linearization(c, true))) break;
      const PcgScalars& R = *c->h_S;
      bool ok = R.stop == 1;
      double eta = 1.0;
      if (!ok && (rc = solve_at_floor(c, &ok, &eta))) break;
      if (!ok) {
        char buf[64];
        std::snprintf(buf, sizeof buf, "%.3e", R.bb > 0 ? std::sqrt(R.rr / R.bb) : 0.0);
        c->err = std::string(name) + ": column " + std::to_string(k % 3) + " of candidate " + std::to_string(t) + " (" + std::to_string(ci[t]) + ", " +
                 std::to_string(cj[t]) + ")" + (R.stop == 3 ? " broke down (Hessian not positive definite)" : " did not reach pcg_tol") + " after " +
                 std::to_string(R.iter) + " PCG iterations (relative residual " + buf + ")";
        failed = true;
        break;
      }
      if ((rc = vec_from_device(c, c->d_x, sols.data() + (size_t)k * n3))) break;
    }
    if (rc || failed) break;
    HIP_TRY(c, hipMemcpyAsync(S.X, sols.data(), bytes, hipMemcpyHostToDevice, c->stream));
    use(t0, t1, S.X, n3, nullptr);
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (sols is rewritten by the next chunk)
  }
  // the linearisation's own right-hand side and its start state again: the context is as after sgo_linearize
  if (saved) {
    {
      Scope sc(c, K_RHS_RESTORE, 48.0 * c->n);
      launch_rhs_restore(c->stream, c->n, c->d_dgb, c->d_s2);
    }
    const int rc2 = solve_from_linearization(c, false);
    if (rc == SGO_OK) rc = rc2;
  }
  if (rc) return rc;
  return failed ? SGO_EINVAL : SGO_OK;
}

bool spd3(const double* o) {   // leading minors of the symmetric matrix 00 01 02 11 12 22
  const double m1 = o[0], m2 = o[0] * o[3] - o[1] * o[1];
  const double m3 = o[0] * (o[3] * o[5] - o[4] * o[4]) - o[1] * (o[1] * o[5] - o[4] * o[2]) + o[2] * (o[1] * o[4] - o[3] * o[2]);
  return m1 > 0.0 && m2 > 0.0 && m3 > 0.0;
}

// What sgo_candidate_gate and sgo_candidate_joint refuse in their candidates.  row[t][side]: hessian index of a free active vertex,
// -1 for a fixed active one.
int check_candidates(sgo_ctx* c, const char* name, int n, const int32_t* ci, const int32_t* cj, const double* meas, const double* info,
                     std::vector<int>* rowp) {
  // (anything but a free or a fixed active vertex is refused)
  std::vector<int>& row = *rowp;
  row.assign(2 * (size_t)n, -1);
  for (int t = 0; t < n; ++t) {
    const std::string who = std::string(name) + ": candidate " + std::to_string(t);
    for (int side = 0; side < 2; ++side) {
      const int v = side ? cj[t] : ci[t];
      if (v < 0 || v >= c->V) {
        c->err = who + ": vertex id " + std::to_string(v) + " outside [0, " + std::to_string(c->V) + ")";
        return SGO_EINVAL;
      }
      const auto f = std::lower_bound(c->free_id.begin(), c->free_id.end(), v);
      if (f != c->free_id.end() && *f == v) row[2 * (size_t)t + side] = (int)(f - c->free_id.begin());
      else if (!std::binary_search(c->fixed_active.begin(), c->fixed_active.end(), v)) {
        c->err = who + ": vertex " + std::to_string(v) + " is not active (it has no edge)";
        return SGO_EINVAL;
      }
    }
    if (ci[t] == cj[t]) {
      c->err = who + " joins vertex " + std::to_string(ci[t]) + " to itself";
      return SGO_EINVAL;
    }
    for (int q = 0; q < 9; ++q)
      if (!std::isfinite(q < 3 ? meas[3 * (size_t)t + q] : info[6 * (size_t)t + q - 3])) {
        c->err = who + ": non-finite entry in its " + (q < 3 ? "measurement" : "information");
        return SGO_EINVAL;
      }
    if (!spd3(info + 6 * (size_t)t)) {
      c->err = who + ": its information matrix is not symmetric positive definite";
      return SGO_EINVAL;
    }
  }
  return SGO_OK;
}

// The candidates' columns X = H^-1 R at the current poses, a chunk at a time: through the factor of selinv_plan's plan, or through
// the PCG where the analysis refuses the graph.  use(t0, t1, X, n3, flags) queues what the caller makes of the chunk [t0, t1)
// (X: its 3 (t1 - t0) columns, rows as C.row says; flags: the factorisation's, nullptr without one).  fill(pos_of, by_pcg, C, &row,
// &ci, &cj) puts the candidates on the device before the first chunk (*Cp) -- pos_of: hessian index -> elimination position on the
// factor's route, nullptr where a right-hand side's rows are the hessian indices themselves -- and names the host's view of rows
// and endpoints, which the PCG route alone reads.  records_first: every candidate's record (C.rec) is made before the first chunk,
// not chunk by chunk.
template <class Fill, class Use>
int columns_of(sgo_ctx* c, const char* name, int n, Fill&& fill, bool records_first, FsCandDev* Cp, Use&& use) {
  int rc;
  Mfront* m = nullptr;
  bool by_pcg = false;
  if (c->n > 0) {
    rc = selinv_plan(c, &m, name, "the PCG route");
    if (rc == SGO_ENOTHING) by_pcg = true;   // (the analysis refuses the graph: the same columns through the PCG)
    else if (rc) return rc;
  }
  std::vector<int> pos_of;   // hessian index -> elimination position
  if (m) {
    if ((rc = fs_prepare(c, m, name))) return rc;
    const MfPlan& P = m->plan;
    pos_of.assign((size_t)c->n, -1);
    for (int p = 0; p < P.n; ++p)
      pos_of[(size_t)(std::lower_bound(c->free_id.begin(), c->free_id.end(), P.elim_vertex[p]) - c->free_id.begin())] = p;
  }
  const std::vector<int>* rowp = nullptr;
  const int32_t *ci = nullptr, *cj = nullptr;
  if ((rc = fill(m ? &pos_of : nullptr, by_pcg, Cp, &rowp, &ci, &cj))) return rc;
  const FsCandDev& C = *Cp;
  if (records_first) {   // (a chunk's columns are contracted with the records of ALL candidates, later chunks' included)
    Scope sc(c, K_FS_RHS, 8.0 * (kFsRec + 9) * n);
    launch_fs_records(c->stream, C, c->d_poses);
  }
  if (by_pcg) {
    if ((rc = gate_by_pcg(c, name, n, C, *rowp, ci, cj, use))) return rc;
  } else {
    const int n3 = 3 * c->n;
    FsScratch S;
    if (m) {
      if ((rc = fs_scratch(c, n3, m->fs.U3, std::min(kFsChunkPanels, (3 * n + kMfPanel - 1) / kMfPanel), &S))) return rc;
      if ((rc = factorize(c, m))) return rc;
    }
    for (int t0 = 0; t0 < n; t0 += kChunkCands) {
      const int t1 = std::min(n, t0 + kChunkCands), nc = 3 * (t1 - t0), panels = (nc + kMfPanel - 1) / kMfPanel;
      if (m) HIP_TRY(c, hipMemsetAsync(S.Y, 0, sizeof(double) * (size_t)panels * kMfPanel * n3, c->stream));
      {
        Scope sc(c, K_FS_RHS, 8.0 * (kFsRec + 18) * (t1 - t0));
        launch_fs_rhs_candidates(c->stream, C, t0, t1, c->d_poses, n3, S.Y);
      }
      if (m) fs_passes(c, m, S, panels, nc);
      use(t0, t1, S.X, n3, m ? m->dev.flags : nullptr);
    }
  }
  return SGO_OK;
}

// ... for candidates the caller describes: row is check_candidates' (rewritten to elimination positions on the factor's route);
// *d_out: the results' place
template <class Use>
int cand_columns(sgo_ctx* c, const char* name, int n, const int32_t* ci, const int32_t* cj, const double* meas, const double* info,
                 std::vector<int>& row, bool records_first, FsCandDev* Cp, double** d_out, Use&& use) {
  return columns_of(c, name, n, [&](const std::vector<int>* pos_of, bool, FsCandDev* C, const std::vector<int>** rowp, const int32_t** cip, const int32_t** cjp) {
    if (pos_of)
      for (int& r : row)
        if (r >= 0) r = (*pos_of)[(size_t)r];
    *rowp = &row;
    *cip = ci;
    *cjp = cj;
    return cand_upload(c, n, ci, cj, row, meas, info, C, d_out);
  }, records_first, Cp, use);
}

// ... for resident edges (sgo_edge_joint): the records' sources are copied out of the resident edge list ON THE DEVICE (k_edge_cands:
// endpoints, rows through a vertex -> row map made here from the plan, inverse measurement, information, kernel weight), so no edge
// data crosses to the host.  *d_w: the weights [n].  The PCG route reads the endpoints' ids and rows back (3 n integers) for its
// messages and to skip a column between two fixed poses.
struct EdgeCandHost {
  std::vector<int> row;
  std::vector<int32_t> vi, vj;
};
template <class Use>
int edge_columns(sgo_ctx* c, const char* name, int n, const int32_t* ids, EdgeCandHost* H, FsCandDev* Cp, double** d_w, Use&& use) {
  return columns_of(c, name, n, [&](const std::vector<int>* pos_of, bool by_pcg, FsCandDev* C, const std::vector<int>** rowp, const int32_t** cip, const int32_t** cjp) {
    sgo_ctx::SelInv& Z = c->selinv;
    const size_t N = (size_t)n, V = (size_t)c->V;
    int rc;
    if ((rc = grow_device(c, &Z.d_cand, &Z.cand_cap, (3 + 6 + kFsRec + 1) * N + 1)) || (rc = grow_device(c, &Z.d_cidx, &Z.cidx_cap, 5 * N + V))) return rc;
    double* d_zinv = Z.d_cand;
    double* d_soa = d_zinv + 3 * N;
    double* d_rec = d_soa + 6 * N;
    *d_w = d_rec + kFsRec * N;
    int* d_vi = Z.d_cidx;
    int* d_vj = d_vi + N;
    int* d_row = d_vj + N;
    int* d_ids = d_row + 2 * N;
    int* d_vrow = d_ids + N;
    std::vector<int> vrow(V, -1);   // vertex -> its place in a right-hand side; -1: fixed (or without an edge)
    for (size_t h = 0; h < c->free_id.size(); ++h) vrow[(size_t)c->free_id[h]] = pos_of ? (*pos_of)[h] : (int)h;
    HIP_TRY(c, hipMemcpyAsync(d_ids, ids, sizeof(int) * N, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_vrow, vrow.data(), sizeof(int) * V, hipMemcpyHostToDevice, c->stream));
    C->n = n;
    C->vi = d_vi;
    C->vj = d_vj;
    C->row = d_row;
    C->zinv = d_zinv;
    C->info = d_soa;
    C->rec = d_rec;
    {
      Scope sc(c, K_EDGE_TABLE, 8.0 * (9 + 9 + 1 + 6) * n + 4.0 * 7 * n);
      launch_edge_cands(c->stream, *C, c->el, d_ids, d_vrow, c->d_poses, d_vi, d_vj, d_row, d_zinv, d_soa, *d_w);
    }
    if (by_pcg) {
      H->row.resize(2 * N);
      H->vi.resize(N);
      H->vj.resize(N);
      HIP_TRY(c, hipMemcpyAsync(H->row.data(), d_row, sizeof(int) * 2 * N, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(H->vi.data(), d_vi, sizeof(int) * N, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(H->vj.data(), d_vj, sizeof(int) * N, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (vrow goes out of scope; the PCG route's host view is complete)
    *rowp = &H->row;
    *cip = H->vi.data();
    *cjp = H->vj.data();
    return SGO_OK;
  }, true, Cp, use);
}

constexpr int kJointLaunch = 1 << 20;   // subsets (workgroups) per launch

}  // namespace

// what sgo_joint_subsets, sgo_joint_pairs and the search's calls (sgo_jsearch.cpp) refuse alike
int sgo::joint_table_check(sgo_ctx* c, const char* name, int32_t n) {
  int rc = check_graph(c);
  if (rc) return rc;
  if (c->joint.n < 0) {
    c->err = std::string(name) + ": no resident table (call sgo_candidate_joint; a new or updated graph drops the table)";
    return SGO_EINVAL;
  }
  if (n != c->joint.n) {
    c->err = std::string(name) + ": n = " + std::to_string(n) + ", the resident table holds " + std::to_string(c->joint.n) + " candidates";
    return SGO_EINVAL;
  }
  return SGO_OK;
}

extern "C" {

int sgo_factor_solve(sgo_ctx* c, int32_t nrhs, const double* B, double* X) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (nrhs < 0 || (nrhs > 0 && (!B || !X))) {
      c->err = "sgo_factor_solve: null buffer or negative count";
      return SGO_EINVAL;
    }
    if ((rc = refuse_context(c, "sgo_factor_solve"))) return rc;
    const size_t n3 = 3 * (size_t)c->n;
    for (size_t k = 0; k < (size_t)nrhs * n3; ++k)
      if (!std::isfinite(B[k])) {
        c->err = "sgo_factor_solve: non-finite entry in right-hand side " + std::to_string(k / n3) + " (hessian index " + std::to_string(k % n3 / 3) + ")";
        return SGO_EINVAL;
      }
    if (nrhs == 0 || c->n == 0) return 0;
    Mfront* m = nullptr;
    if ((rc = selinv_plan(c, &m, "sgo_factor_solve", "sgo_solve_rhs"))) return rc;
    if ((rc = fs_prepare(c, m, "sgo_factor_solve"))) return rc;
    const int chunk = kFsChunkPanels * kMfPanel;
    FsScratch S;
    if ((rc = fs_scratch(c, (int)n3, m->fs.U3, std::min(kFsChunkPanels, (nrhs + kMfPanel - 1) / kMfPanel), &S))) return rc;
    if ((rc = factorize(c, m))) return rc;
    std::vector<double> res((size_t)nrhs * n3), stage;
    const MfPlan& P = m->plan;
    std::vector<int> pos_h((size_t)P.n);
    for (int p = 0; p < P.n; ++p)
      pos_h[p] = (int)(std::lower_bound(c->free_id.begin(), c->free_id.end(), P.elim_vertex[p]) - c->free_id.begin());
    for (int c0 = 0; c0 < nrhs; c0 += chunk) {
      const int nc = std::min(chunk, nrhs - c0), panels = (nc + kMfPanel - 1) / kMfPanel;
      // the chunk's columns arrive in X's place (hessian order) and are permuted into Y's; a tail panel's padding is zero
      HIP_TRY(c, hipMemcpyAsync(S.X, B + (size_t)c0 * n3, sizeof(double) * (size_t)nc * n3, hipMemcpyHostToDevice, c->stream));
      if (nc < panels * kMfPanel)
        HIP_TRY(c, hipMemsetAsync(S.Y + (size_t)nc * n3, 0, sizeof(double) * (size_t)(panels * kMfPanel - nc) * n3, c->stream));
      {
        Scope sc(c, K_FS_RHS, 16.0 * (double)nc * (double)n3);
        launch_fs_rhs_columns(c->stream, nc, (int)n3, S.X, m->fs.pos_h, S.Y);
      }
      fs_passes(c, m, S, panels, nc);
      HIP_TRY(c, hipGetLastError());
      stage.resize((size_t)nc * n3);
      HIP_TRY(c, hipMemcpyAsync(stage.data(), S.X, sizeof(double) * (size_t)nc * n3, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      for (int k = 0; k < nc; ++k) {
        const double* s = stage.data() + (size_t)k * n3;
        double* d = res.data() + (size_t)(c0 + k) * n3;
        for (int p = 0; p < P.n; ++p)
          for (int q = 0; q < 3; ++q) d[3 * (size_t)pos_h[p] + q] = s[3 * (size_t)p + q];
      }
    }
    int flags[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(flags, m->dev.flags, sizeof flags, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    if (flags[0]) {
      c->err = std::string("sgo_factor_solve") + kNotPd;
      return SGO_EINVAL;
    }
    std::copy(res.begin(), res.end(), X);
    return (int)P.fronts.size();
  } SGO_CATCH(c)
}

int sgo_candidate_gate(sgo_ctx* c, int32_t n, const int32_t* ci, const int32_t* cj, const double* meas, const double* info, double chi2_max,
                       double* d2, double* cov_pred, uint8_t* pass) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!ci || !cj || !meas || !info))) {
      c->err = "sgo_candidate_gate: null buffer or negative count";
      return SGO_EINVAL;
    }
    if (!std::isfinite(chi2_max)) {
      c->err = "sgo_candidate_gate: chi2_max is not finite";
      return SGO_EINVAL;
    }
    if ((rc = refuse_context(c, "sgo_candidate_gate"))) return rc;
    std::vector<int> row;
    if ((rc = check_candidates(c, "sgo_candidate_gate", n, ci, cj, meas, info, &row))) return rc;
    if (n == 0) return 0;
    FsCandDev C;
    double* d_out = nullptr;
    if ((rc = cand_columns(c, "sgo_candidate_gate", n, ci, cj, meas, info, row, false, &C, &d_out, [&](int t0, int t1, const double* X, int n3, const int* flags) {
          Scope sc(c, K_FS_GATE, 8.0 * (kFsRec + kFsOut + 24) * (t1 - t0));
          launch_fs_gate(c->stream, C, t0, t1, X, n3, chi2_max, flags, d_out);
        })))
      return rc;
    const size_t nout = (size_t)kFsOut * n + 1;
    HIP_TRY(c, hipGetLastError());
    std::vector<double> out(nout);
    HIP_TRY(c, hipMemcpyAsync(out.data(), d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    if (out[nout - 1] != 0.0) {
      c->err = std::string("sgo_candidate_gate") + kNotPd;
      return SGO_EINVAL;
    }
    int npass = 0;
    for (int t = 0; t < n; ++t) {
      const double* o = out.data() + (size_t)kFsOut * t;
      if (d2) d2[t] = o[0];
      if (cov_pred) std::copy(o + 1, o + 10, cov_pred + 9 * (size_t)t);
      if (pass) pass[t] = o[10] != 0.0;
      npass += o[10] != 0.0;
    }
    return npass;
  } SGO_CATCH(c)
}

int sgo_candidate_joint(sgo_ctx* c, int32_t n, const int32_t* ci, const int32_t* cj, const double* meas, const double* info, double* S, double* e) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!ci || !cj || !meas || !info))) {
      c->err = "sgo_candidate_joint: null buffer or negative count";
      return SGO_EINVAL;
    }
    if (n > SGO_JOINT_MAX_CANDIDATES) {
      c->err = "sgo_candidate_joint: " + std::to_string(n) + " candidates, more than SGO_JOINT_MAX_CANDIDATES = " + std::to_string(SGO_JOINT_MAX_CANDIDATES);
      return SGO_EINVAL;
    }
    if ((rc = refuse_context(c, "sgo_candidate_joint"))) return rc;
    std::vector<int> row;
    if ((rc = check_candidates(c, "sgo_candidate_joint", n, ci, cj, meas, info, &row))) return rc;
    sgo_ctx::Joint& J = c->joint;
    if (n == 0) {
      J.n = -1;
      return 0;
    }
    if (!J.lds_ready) {
      if (!joint_prepare_device()) {
        c->err = "sgo_candidate_joint: the device does not grant the subset kernel's dynamic LDS";
        return SGO_EHIP;
      }
      J.lds_ready = true;
    }
    // built beside the resident table, which stays until this call has succeeded
    const int other = J.n < 0 ? J.cur : 1 - J.cur;
    const size_t N3 = 3 * (size_t)n, ntab = joint_table_doubles(n);
    if ((rc = grow_device(c, &J.d_raw, &J.raw_cap, N3 * N3)) || (rc = grow_device(c, &J.d_tab[other], &J.tab_cap[other], ntab))) return rc;
    double* const tab = J.d_tab[other];
    FsCandDev C;
    double* d_out = nullptr;
    const int* fl = nullptr;
    if ((rc = cand_columns(c, "sgo_candidate_joint", n, ci, cj, meas, info, row, true, &C, &d_out, [&](int t0, int t1, const double* X, int n3, const int* flags) {
          Scope sc(c, K_FS_GRAM, 8.0 * (kFsRec + 18 + 9) * (double)n * (t1 - t0));
          launch_fs_gram(c->stream, C, t0, t1, X, n3, J.d_raw);
          fl = flags;
        })))
      return rc;
    {
      Scope sc(c, K_FS_JOINT_TABLE, 8.0 * 18 * (double)n * n);
      launch_fs_joint_table(c->stream, C, J.d_raw, fl, tab);
    }
    HIP_TRY(c, hipGetLastError());
    // the failure flag first: the outputs stay untouched when the Hessian is not positive definite; then S and e straight into the
    // caller's arrays (4.7 MB at 256 candidates: no staging copy)
    double failed = 0.0;
    HIP_TRY(c, hipMemcpyAsync(&failed, tab + ntab - 1, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    if (failed != 0.0) {
      c->err = std::string("sgo_candidate_joint") + kNotPd;
      return SGO_EINVAL;
    }
    if (S) HIP_TRY(c, hipMemcpyAsync(S, tab, sizeof(double) * N3 * N3, hipMemcpyDeviceToHost, c->stream));
    if (e) HIP_TRY(c, hipMemcpyAsync(e, tab + N3 * N3, sizeof(double) * N3, hipMemcpyDeviceToHost, c->stream));
    if (S || e) HIP_TRY(c, hipStreamSynchronize(c->stream));
    J.cur = other;
    J.n = n;
    return n;
  } SGO_CATCH(c)
}


int sgo_edge_joint(sgo_ctx* c, int32_t n, const int32_t* edge_ids, double* N, double* e, double* w) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !edge_ids)) {
      c->err = "sgo_edge_joint: null edge_ids or negative count";
      return SGO_EINVAL;
    }
    if (n > SGO_JOINT_MAX_CANDIDATES) {
      c->err = "sgo_edge_joint: " + std::to_string(n) + " edges, more than SGO_JOINT_MAX_CANDIDATES = " + std::to_string(SGO_JOINT_MAX_CANDIDATES);
      return SGO_EINVAL;
    }
    if ((rc = refuse_context(c, "sgo_edge_joint"))) return rc;
    {
      std::vector<int32_t> seen(edge_ids, edge_ids + n);
      std::sort(seen.begin(), seen.end());
      for (int t = 0; t < n; ++t) {
        if (seen[(size_t)t] < 0 || seen[(size_t)t] >= c->E) {
          c->err = "sgo_edge_joint: edge id " + std::to_string(seen[(size_t)t]) + " outside [0, " + std::to_string(c->E) + ")";
          return SGO_EINVAL;
        }
        if (t > 0 && seen[(size_t)t] == seen[(size_t)t - 1]) {
          c->err = "sgo_edge_joint: edge " + std::to_string(seen[(size_t)t]) + " is listed twice (removing an edge twice has no meaning)";
          return SGO_EINVAL;
        }
      }
    }
    sgo_ctx::EdgeJoint& J = c->ejoint;
    if (n == 0) {
      J.n = -1;
      return 0;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (!J.lds_ready) {
      if (!edge_groups_prepare_device()) {
        c->err = "sgo_edge_joint: the device does not grant the group kernel's dynamic LDS";
        return SGO_EHIP;
      }
      J.lds_ready = true;
    }
    // built beside the resident table, which stays until this call has succeeded; the Gram blocks go through the candidates'
    // table's scratch (joint.d_raw), which holds nothing between calls
    const int other = J.n < 0 ? J.cur : 1 - J.cur;
    const size_t N3 = 3 * (size_t)n, ntab = edge_table_doubles(n);
    if ((rc = grow_device(c, &c->joint.d_raw, &c->joint.raw_cap, N3 * N3)) || (rc = grow_device(c, &J.d_tab[other], &J.tab_cap[other], ntab))) return rc;
    double* const tab = J.d_tab[other];
    FsCandDev C;
    EdgeCandHost host;
    double* d_w = nullptr;
    const int* fl = nullptr;
    if ((rc = edge_columns(c, "sgo_edge_joint", n, edge_ids, &host, &C, &d_w, [&](int t0, int t1, const double* X, int n3, const int* flags) {
          Scope sc(c, K_FS_GRAM, 8.0 * (kFsRec + 18 + 9) * (double)n * (t1 - t0));
          launch_fs_gram(c->stream, C, t0, t1, X, n3, c->joint.d_raw);
          fl = flags;
        })))
      return rc;
    {
      Scope sc(c, K_EDGE_TABLE, 8.0 * 18 * (double)n * n);
      launch_edge_table(c->stream, C, d_w, c->joint.d_raw, fl, tab);
    }
    HIP_TRY(c, hipGetLastError());
    double failed = 0.0;   // the failure flag first: the outputs stay untouched when the Hessian is not positive definite
    HIP_TRY(c, hipMemcpyAsync(&failed, tab + ntab - 1, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    if (failed != 0.0) {
      c->err = std::string("sgo_edge_joint") + kNotPd;
      return SGO_EINVAL;
    }
    if (N) HIP_TRY(c, hipMemcpyAsync(N, tab, sizeof(double) * N3 * N3, hipMemcpyDeviceToHost, c->stream));
    if (e) HIP_TRY(c, hipMemcpyAsync(e, tab + N3 * N3, sizeof(double) * N3, hipMemcpyDeviceToHost, c->stream));
    if (w) HIP_TRY(c, hipMemcpyAsync(w, tab + N3 * N3 + N3, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (N || e || w) HIP_TRY(c, hipStreamSynchronize(c->stream));
    J.cur = other;
    J.n = n;
    return n;
  } SGO_CATCH(c)
}

int sgo_joint_subsets(sgo_ctx* c, int32_t n, int32_t B, const uint8_t* subset, const double* chi2_max, double* d2, int32_t* dof, uint8_t* pass) {
  try {
    int rc = joint_table_check(c, "sgo_joint_subsets", n);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!subset || !d2))) {
      c->err = "sgo_joint_subsets: null buffer or negative count";
      return SGO_EINVAL;
    }
    if (chi2_max)
      for (int b = 0; b < B; ++b)
        if (!std::isfinite(chi2_max[b])) {
          c->err = "sgo_joint_subsets: chi2_max of subset " + std::to_string(b) + " is not finite";
          return SGO_EINVAL;
        }
    std::vector<int> cnt((size_t)B);
    int largest = 0;
    for (int b = 0; b < B; ++b) {
      int k = 0;
      for (int t = 0; t < n; ++t) k += subset[(size_t)b * n + t] != 0;
      if (k > SGO_JOINT_MAX_SUBSET) {
        c->err = "sgo_joint_subsets: subset " + std::to_string(b) + " selects " + std::to_string(k) + " candidates, more than SGO_JOINT_MAX_SUBSET = " +
                 std::to_string(SGO_JOINT_MAX_SUBSET);
        return SGO_EINVAL;
      }
      cnt[(size_t)b] = k;
      largest = std::max(largest, k);
    }
    if (B == 0) return 0;
    sgo_ctx::Joint& J = c->joint;
    const size_t nm = (size_t)B * n;
    if ((rc = grow_device(c, &J.d_d2, &J.d2_cap, (size_t)B)) || (rc = grow_device(c, &J.d_mask, &J.mask_cap, nm))) return rc;
    HIP_TRY(c, hipMemcpyAsync(J.d_mask, subset, nm, hipMemcpyHostToDevice, c->stream));
    for (int b0 = 0; b0 < B; b0 += kJointLaunch) {
      const int nb = std::min(kJointLaunch, B - b0);
      Scope sc(c, K_JOINT_SUBSETS, (double)nb * (n + 8.0 + 4.0 * (3.0 * largest + 1) * (3.0 * largest + 2)));
      launch_joint_subsets(c->stream, J.d_tab[J.cur], n, J.d_mask, b0, nb, std::max(3 * largest, 3), J.d_d2);
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<double> res((size_t)B);
    HIP_TRY(c, hipMemcpyAsync(res.data(), J.d_d2, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    int npass = 0;
    for (int b = 0; b < B; ++b) {
      d2[b] = res[(size_t)b];
      if (dof) dof[b] = 3 * cnt[(size_t)b];
      if (chi2_max) {
        const bool ok = res[(size_t)b] <= chi2_max[b];
        if (pass) pass[b] = ok;
        npass += ok;
      }
    }
    return npass;
  } SGO_CATCH(c)
}

int sgo_joint_pairs(sgo_ctx* c, int32_t n, double* d2) {
  try {
    int rc = joint_table_check(c, "sgo_joint_pairs", n);
    if (rc) return rc;
    if (n > 0 && !d2) {
      c->err = "sgo_joint_pairs: null buffer";
      return SGO_EINVAL;
    }
    sgo_ctx::Joint& J = c->joint;
    const size_t nn = (size_t)n * n;
    const int B = n * (n + 1) / 2;
    if ((rc = grow_device(c, &J.d_d2, &J.d2_cap, nn))) return rc;
    {
      Scope sc(c, K_JOINT_SUBSETS, (double)B * (16.0 + 8.0 * 7 * 8));
      launch_joint_subsets(c->stream, J.d_tab[J.cur], n, nullptr, 0, B, 6, J.d_d2);
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<double> res(nn);
    HIP_TRY(c, hipMemcpyAsync(res.data(), J.d_d2, sizeof(double) * nn, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    std::copy(res.begin(), res.end(), d2);
    return n;
  } SGO_CATCH(c)
}

}  // extern "C"
