// sgo_loo.cpp -- sgo_edge_leave_one_out (include/sgo.h): the leave-one-out test of every listed resident
// edge from one selected inversion (kernel in sgo_loo.hip, the rule in sgo_rules.h).  One call is
//   sgo_marginals_selected's two phases (selinv_run, sgo_selinv.cpp: the factor phase at the current poses, then the selected
//   inversion top-down) -> k_loo_edges over the listed edges, reading Sigma's blocks in place -> one copy of [n][12] to the host.
// The per-edge descriptors (where the selected inverse holds an edge's three blocks) are made once per plan and kept with it.
#include <algorithm>
#include <cmath>

#include "sgo_ctx.h"
#include "sgo_mfront_dev.h"

using namespace sgo;

namespace {

// Every resident edge's descriptor in the plan's terms, once per plan (out of the per-graph arena, as the selected inversion's arrays).
int loo_prepare(sgo_ctx* c, Mfront* m) {
  if (m->loo && m->loo_E == c->E) return SGO_OK;
  const size_t E = (size_t)c->E;
  std::vector<int32_t> ei(E), ej(E);
  HIP_TRY(c, hipMemcpyAsync(ei.data(), c->el.vi, sizeof(int32_t) * E, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(ej.data(), c->el.vj, sizeof(int32_t) * E, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const std::vector<int> pos_of = selinv_positions(c, m);
  auto position = [&](int v) {   // elimination position of a free vertex, -1 for a fixed one
    const auto f = std::lower_bound(c->free_id.begin(), c->free_id.end(), v);
    return (f != c->free_id.end() && *f == v) ? pos_of[(size_t)(f - c->free_id.begin())] : -1;
  };
  std::vector<LooEdgeDev> desc(E);
  for (size_t k = 0; k < E; ++k) {
    LooEdgeDev& d = desc[k];
    d.pi = position(ei[k]);
    d.pj = position(ej[k]);
    d.pair = make_int4(-1, 0, 0, 0);
    if (d.pi >= 0 && d.pj >= 0 && !selinv_pair(m, d.pi, d.pj, &d.pair)) {
      c->err = "sgo_edge_leave_one_out: no front of the plan holds both poses of edge " + std::to_string(k) + " (internal error)";
      return SGO_EINVAL;
    }
  }
  LooEdgeDev* d_desc = nullptr;
  int rc;
  if ((rc = upload(c, &d_desc, desc))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the host vector goes out of scope)
  m->loo = d_desc;
  m->loo_E = c->E;
  return SGO_OK;
}

}  // namespace

extern "C" {

int sgo_edge_leave_one_out(sgo_ctx* c, int32_t n, const int32_t* edge_ids, double chi2_max, double min_redundancy, double* d2, double* redundancy,
                           double* cov_loo, uint8_t* fail) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (n < 0 || !d2) {
      c->err = "sgo_edge_leave_one_out: negative count or null d2";
      return SGO_EINVAL;
    }
    if (!std::isfinite(chi2_max)) {
      c->err = "sgo_edge_leave_one_out: chi2_max is not finite";
      return SGO_EINVAL;
    }
    if (!(min_redundancy > 0.0 && min_redundancy <= 1.0)) {
      c->err = "sgo_edge_leave_one_out: min_redundancy outside (0, 1] (zero would let a bridge edge's 0 / 0 decide)";
      return SGO_EINVAL;
    }
    if (c->ov.active) {
      c->err = "single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";
      return SGO_EINVAL;
    }
    if (multi_gpu_context(c)) {
      c->err = "sgo_edge_leave_one_out: not available in a multi-GPU context";
      return SGO_EINVAL;
    }
    if (!edge_ids && n > c->E) {
      c->err = "sgo_edge_leave_one_out: n = " + std::to_string(n) + " without ids, the graph has " + std::to_string(c->E) + " edges";
      return SGO_EINVAL;
    }
    for (int t = 0; edge_ids && t < n; ++t)
      if (edge_ids[t] < 0 || edge_ids[t] >= c->E) {
        c->err = "sgo_edge_leave_one_out: edge id " + std::to_string(edge_ids[t]) + " outside [0, " + std::to_string(c->E) + ")";
        return SGO_EINVAL;
      }
    if (n == 0) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    Mfront* m = nullptr;
    if (c->n > 0) {   // (no free pose: every P is zero, nothing to factorise)
      if ((rc = selinv_plan(c, &m, "sgo_edge_leave_one_out", "sgo_optimize_gn_hypotheses"))) return rc;
      if ((rc = selinv_prepare(c, m, "sgo_edge_leave_one_out")) || (rc = loo_prepare(c, m))) return rc;
    }
    sgo_ctx::SelInv& Z = c->selinv;
    const size_t nres = (size_t)kLooOut * n + 2, nout = nres + kMaxPartials;
    if ((rc = grow_device(c, &Z.d_loo, &Z.loo_cap, nout)) || (edge_ids && (rc = grow_device(c, &Z.d_loo_ids, &Z.loo_ids_cap, (size_t)n)))) return rc;
    if (edge_ids) HIP_TRY(c, hipMemcpyAsync(Z.d_loo_ids, edge_ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (m && (rc = selinv_run(c, m))) return rc;
    {
      Scope sc(c, K_LOO_EDGES, 8.0 * (21 + 15 + 6 + kLooOut) * n);
      launch_loo_edges(c->stream, m ? m->dev : MfDev(), m ? m->sel : MfSelDev(), m ? m->loo : nullptr, c->el, c->d_poses, n,
                       edge_ids ? Z.d_loo_ids : nullptr, chi2_max, min_redundancy, Z.d_loo, Z.d_loo + nres);
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<double> out(nres);
    HIP_TRY(c, hipMemcpyAsync(out.data(), Z.d_loo, sizeof(double) * nres, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    if (out[nres - 2] != 0.0) {
      c->err = "sgo_edge_leave_one_out: the factorisation failed (a pivot block is not positive definite: Hessian not positive definite)";
      return SGO_EINVAL;
    }
    for (int t = 0; t < n; ++t) {
      const double* o = out.data() + (size_t)kLooOut * t;
      d2[t] = o[0];
      if (redundancy) redundancy[t] = o[1];
      if (cov_loo) std::copy(o + 2, o + 11, cov_loo + 9 * (size_t)t);
      if (fail) fail[t] = o[11] != 0.0;
    }
    return (int)out[nres - 1];
  } SGO_CATCH(c)
}

}  // extern "C"
