// sgo_search.cpp -- sgo_closure_search (include/sgo.h): for every query pose c and every listed pose j, whether
// c can be excluded from lying within `radius` of j once the covariance of their relative pose is taken into account (kernels in
// sgo_search.hip, the pair rule in sgo_rules.h).  One call is
//   sgo_marginals_selected's two phases (selinv_run, sgo_selinv.cpp: the factor phase at the current poses, then the selected
//   inversion top-down: Sigma_jj of every pose, in place) ->
//   per chunk of at most kCsChunkQueries queries: unit right-hand sides at the free queries' elimination positions (a memset and
//   k_cs_unit) -> sgo_factor_solve's two passes over the SAME factor (fs_passes, sgo_fsolve.cpp: Sigma_jc of every j, the rows of the
//   queries' columns) -> k_closure_search -> the ordered count -> one copy per requested output.
// One factorisation serves both phases: k_si_panels reads the factor (the arena and YINV) and writes the selected inverse to an
// arena of its own, so k_fs_forward / k_fs_backward find the factor as k_mf_panels left it.
// A chunk whose queries are all fixed queues no substitution at all.
#include <algorithm>
#include <cmath>

#include "sgo_ctx.h"
#include "sgo_mfront_dev.h"

using namespace sgo;

namespace {

// one chunk's results may take this many doubles of scratch (256 MiB): a chunk holds fewer queries where n is large
constexpr size_t kCsScratchDoubles = (size_t)1 << 25;

}  // namespace

extern "C" {

int sgo_closure_search(sgo_ctx* c, int32_t nq, const int32_t* query, int32_t n, const int32_t* ids, double radius, double chi2_max, int32_t min_sep,
                       double* m2, double* rel, double* cov_rel, double* sigma, uint8_t* near) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    const size_t npairs = nq < 0 || n < 0 ? 0 : (size_t)nq * (size_t)n;
    if (nq < 0 || n < 0 || (nq > 0 && !query) || (npairs > 0 && !m2)) {
      c->err = "sgo_closure_search: negative count, null query or null m2";
      return SGO_EINVAL;
    }
    if (!std::isfinite(radius) || radius < 0.0) {
      c->err = "sgo_closure_search: radius is negative or not finite";
      return SGO_EINVAL;
    }
    if (!std::isfinite(chi2_max)) {
      c->err = "sgo_closure_search: chi2_max is not finite";
      return SGO_EINVAL;
    }
    if (min_sep < 0) {
      c->err = "sgo_closure_search: min_sep is negative";
      return SGO_EINVAL;
    }
    if (c->ov.active) {
      c->err = "sgo_closure_search: single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";
      return SGO_EINVAL;
    }
    if (multi_gpu_context(c)) {
      c->err = "sgo_closure_search: not available in a multi-GPU context";
      return SGO_EINVAL;
    }
    if (!ids && n > c->V) {
      c->err = "sgo_closure_search: n = " + std::to_string(n) + " without ids, the graph has " + std::to_string(c->V) + " vertices";
      return SGO_EINVAL;
    }
    // hessian index of a free active vertex, -1 for a fixed active one, -2 for one without an edge
    auto status = [&](int v) {
      const auto f = std::lower_bound(c->free_id.begin(), c->free_id.end(), v);
      if (f != c->free_id.end() && *f == v) return (int)(f - c->free_id.begin());
      return std::binary_search(c->fixed_active.begin(), c->fixed_active.end(), v) ? -1 : -2;
    };
    for (int k = 0; k < nq + (ids ? n : 0); ++k) {
      const int v = k < nq ? query[k] : ids[k - nq];
      const char* what = k < nq ? "query " : "listed id ";
      if (v < 0 || v >= c->V) {
        c->err = std::string("sgo_closure_search: ") + what + std::to_string(v) + " outside [0, " + std::to_string(c->V) + ")";
        return SGO_EINVAL;
      }
      if (status(v) == -2) {
        c->err = std::string("sgo_closure_search: ") + what + std::to_string(v) + " is not active (the vertex has no edge)";
        return SGO_EINVAL;
      }
    }
    if (npairs == 0) return 0;
    Mfront* m = nullptr;
    if (c->n > 0) {   // (no free pose: every P is zero, nothing to factorise)
      if ((rc = selinv_plan(c, &m, "sgo_closure_search",
                            "sgo_candidate_gate on a Euclidean shortlist (there is no cheap Sigma_jj of every pose without a factor)")))
        return rc;
      if ((rc = selinv_prepare(c, m, "sgo_closure_search")) || (rc = fs_prepare(c, m, "sgo_closure_search"))) return rc;
    }
    // every vertex's place in the plan's terms
    std::vector<int> vpos((size_t)c->V, -2);
    {
      const std::vector<int> pos_of = m ? selinv_positions(c, m) : std::vector<int>();
      for (size_t h = 0; h < c->free_id.size(); ++h) vpos[(size_t)c->free_id[h]] = pos_of[h];
      for (const int v : c->fixed_active) vpos[(size_t)v] = -1;
    }
    const size_t N = (size_t)n, V = (size_t)c->V;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)nq, (size_t)kCsChunkQueries), kCsScratchDoubles / ((size_t)kCsOut * N)));
    sgo_ctx::SelInv& Z = c->selinv;
    const size_t nout = (size_t)kCsOut * chunk * N + 2 + kMaxPartials;
    if ((rc = grow_device(c, &Z.d_search, &Z.search_cap, nout)) ||
        (rc = grow_device(c, &Z.d_search_idx, &Z.search_idx_cap, 4 * (size_t)kCsChunkQueries + V + (ids ? N : 0))))
      return rc;
    CsQueryDev* d_queries = reinterpret_cast<CsQueryDev*>(Z.d_search_idx);   // (first: 16-byte aligned)
    int* d_vpos = Z.d_search_idx + 4 * (size_t)kCsChunkQueries;
    int* d_ids = ids ? d_vpos + V : nullptr;
    HIP_TRY(c, hipMemcpyAsync(d_vpos, vpos.data(), sizeof(int) * V, hipMemcpyHostToDevice, c->stream));
    if (ids) HIP_TRY(c, hipMemcpyAsync(d_ids, ids, sizeof(int32_t) * N, hipMemcpyHostToDevice, c->stream));
    const int n3 = 3 * c->n;
    FsScratch S;
    if (m) {
      bool any_free = false;
      for (int k = 0; k < nq && !any_free; ++k) any_free = vpos[(size_t)query[k]] >= 0;
      if (any_free && (rc = fs_scratch(c, n3, m->fs.U3, (3 * chunk + kMfPanel - 1) / kMfPanel, &S))) return rc;
      if ((rc = selinv_run(c, m))) return rc;
    }
    // what the caller asked for, as ranges of fields of a chunk's results: m2 | rel | cov_rel | sigma | near
    const int f0[5] = {0, 1, 4, 10, 12}, f1[5] = {1, 4, 10, 12, 13};
    const bool want[5] = {true, rel != nullptr, cov_rel != nullptr, sigma != nullptr, near != nullptr};
    std::vector<double> st;
    std::vector<CsQueryDev> desc;
    long long count = 0;
    for (int q0 = 0; q0 < nq; q0 += chunk) {
      const int cq = std::min(chunk, nq - q0);
      desc.assign((size_t)cq, make_int4(0, -1, -1, 0));
      int ncols = 0;
      for (int q = 0; q < cq; ++q) {
        CsQueryDev& d = desc[(size_t)q];
        d.x = query[q0 + q];
        d.y = vpos[(size_t)d.x];
        if (d.y >= 0) {
          d.z = ncols;
          ncols += 3;
        }
      }
      HIP_TRY(c, hipMemcpyAsync(d_queries, desc.data(), sizeof(CsQueryDev) * (size_t)cq, hipMemcpyHostToDevice, c->stream));
      if (ncols > 0) {   // (a chunk of fixed queries costs no solve)
        const int panels = (ncols + kMfPanel - 1) / kMfPanel;
        HIP_TRY(c, hipMemsetAsync(S.Y, 0, sizeof(double) * (size_t)panels * kMfPanel * n3, c->stream));
        {
          Scope sc(c, K_FS_RHS, 8.0 * ncols);
          launch_cs_unit(c->stream, cq, d_queries, n3, S.Y);
        }
        fs_passes(c, m, S, panels, ncols);
      }
      const size_t plane = (size_t)cq * N, nres = (size_t)kCsOut * plane + 2;
      {
        Scope sc(c, K_CLOSURE_SEARCH, 8.0 * (9 + kCsOut) * (double)plane + (8.0 * 9 + 8.0) * (double)N);
        launch_closure_search(c->stream, m ? m->dev : MfDev(), m ? m->sel : MfSelDev(), m != nullptr, d_vpos, c->d_poses, n, d_ids, cq, d_queries, S.X, n3,
                              radius, chi2_max, min_sep, Z.d_search, Z.d_search + nres);
      }
      HIP_TRY(c, hipGetLastError());
      st.resize(nres);
      for (int g = 0; g < 5; ++g)
        if (want[g])
          HIP_TRY(c, hipMemcpyAsync(st.data() + f0[g] * plane, Z.d_search + f0[g] * plane, sizeof(double) * (f1[g] - f0[g]) * plane, hipMemcpyDeviceToHost,
                                    c->stream));
      HIP_TRY(c, hipMemcpyAsync(st.data() + nres - 2, Z.d_search + nres - 2, sizeof(double) * 2, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      if (st[nres - 2] != 0.0) {   // (the one factorisation of the call: the first chunk says so, before anything is written)
        prof_flush(c);
        c->err = "sgo_closure_search: the factorisation failed (a pivot block is not positive definite: Hessian not positive definite)";
        return SGO_EINVAL;
      }
      count += (long long)st[nres - 1];
      for (int q = 0; q < cq; ++q) {
        const size_t o = ((size_t)q0 + q) * N;
        const double* s = st.data() + (size_t)q * N;   // field f of pair (q, t): s[f * plane + t]
        std::copy(s, s + N, m2 + o);
        for (size_t t = 0; t < N; ++t) {
          if (rel)
            for (int a = 0; a < 3; ++a) rel[3 * (o + t) + a] = s[(1 + a) * plane + t];
          if (cov_rel) {
            double* P = cov_rel + 9 * (o + t);
            P[0] = s[4 * plane + t];
            P[1] = P[3] = s[5 * plane + t];
            P[2] = P[6] = s[6 * plane + t];
            P[4] = s[7 * plane + t];
            P[5] = P[7] = s[8 * plane + t];
            P[8] = s[9 * plane + t];
          }
          if (sigma) {
            sigma[2 * (o + t)] = s[10 * plane + t];
            sigma[2 * (o + t) + 1] = s[11 * plane + t];
          }
          if (near) near[o + t] = s[12 * plane + t] != 0.0;
        }
      }
    }
    prof_flush(c);
    return (int)std::min<long long>(count, 2147483647LL);
  } SGO_CATCH(c)
}

}  // extern "C"
