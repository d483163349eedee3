// sgo_selinv.cpp -- sgo_marginals_selected (include/sgo.h): the covariance blocks of every pose, and of every pair inside the
// multifrontal factor's pattern, by selected inversion of the factor (kernels in sgo_selinv.hip).  One call is
//   factor phase at the current poses (mfront_factorize: the multifrontal path's own launches) ->
//   top-down per level: gather Sigma_bb from the parent, then the own columns of every front of the level ->
//   result gather -> one copy to the host.
// The plan is the resident one when optimize() takes the multifrontal path; a graph on another path gets a plan of its own,
// analysed once per set-up under the multifrontal path's admission limits.  sgo_optimize_gn keeps its path either way: the call
// writes the factor's arrays (which every Gauss-Newton iteration recomputes from the poses) and the scratch d_hist / d_dres.
// The first two phases (selinv_prepare, selinv_run) and the pairs' descriptors (selinv_pair) are sgo_edge_leave_one_out's too
// (sgo_loo.cpp), which reads the selected inverse in place instead of gathering it.
#include <algorithm>
#include <cstdlib>

#include "sgo_ctx.h"
#include "sgo_mfront_dev.h"

using namespace sgo;

namespace sgo {

// The plan the factor's calls work through (sgo_marginals_selected, sgo_factor_solve, sgo_candidate_gate): the resident one, or one
// analysed for this purpose (once per set-up; a refusal is cached too).  who / instead: the entry point and what its caller is
// pointed to, for the refusal's text.
int selinv_plan(sgo_ctx* c, Mfront** out, const char* who, const char* instead) {
  if (c->mf) {
    *out = c->mf;
    return SGO_OK;
  }
  sgo_ctx::SelInv& Z = c->selinv;
  if (!Z.tried) {
    std::vector<int32_t> ei((size_t)c->E), ej((size_t)c->E);
    std::vector<double> poses(3 * (size_t)c->V);
    if (c->E > 0) {
      HIP_TRY(c, hipMemcpyAsync(ei.data(), c->el.vi, sizeof(int32_t) * ei.size(), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(ej.data(), c->el.vj, sizeof(int32_t) * ej.size(), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(poses.data(), c->d_poses, sizeof(double) * poses.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int mf_rows = 12288, hint = -1;
    if (const char* s = std::getenv("SGO_MFRONT_ROWS"))
      if (std::atoi(s) > 0) mf_rows = std::atoi(s);
    std::string merr;
    Z.why.clear();
    Z.mf = mfront_create(c->stream, &c->graph_arena, c->V, c->n, c->free_id.data(), poses.data(), c->E, ei.data(), ej.data(), mf_rows, &hint,
                         &Z.why, &merr);
    if (!Z.mf && !merr.empty()) {
      c->err = merr;
      return SGO_EHIP;
    }
    Z.tried = true;
  }
  if (!Z.mf) {
    c->err = std::string(who) + ": the multifrontal analysis refuses this graph (" + Z.why + "): use " + instead;
    return SGO_ENOTHING;
  }
  *out = Z.mf;
  return SGO_OK;
}

// The extend-add maps in the child -> parent direction on the device (sel.cmap, sel.cmap_off), once per plan: the selected
// inversion gathers through them, the multi-right-hand-side substitution adds the children's updates through them.
int mfront_maps_prepare(sgo_ctx* c, Mfront* m) {
  if (m->sel.cmap) return SGO_OK;
  const MfPlan& P = m->plan;
  const int nf = (int)P.fronts.size();
  std::vector<int> cmap_off((size_t)nf, 0);
  for (int f = 0; f < nf; ++f)
    for (int k = 0; k < 2; ++k)
      if (P.fronts[f].kid[k] >= 0) cmap_off[P.fronts[f].kid[k]] = P.fronts[f].map_off[k];
  std::vector<int> cmap = P.cmap;
  if (cmap.empty()) cmap.push_back(0);
  int *d_cmap = nullptr, *d_off = nullptr;
  int rc;
  if ((rc = upload(c, &d_cmap, cmap)) || (rc = upload(c, &d_off, cmap_off))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the host vectors above go out of scope)
  m->sel.cmap = d_cmap;
  m->sel.cmap_off = d_off;
  return SGO_OK;
}

// The selected inversion's own device arrays, once per plan: the second arena (zeroed once: the entries no kernel writes stay
// zero), the extend-add maps, the gather's tiles and the front of every elimination position.
int selinv_prepare(sgo_ctx* c, Mfront* m, const char* who) {
  if (m->sel_ready) return SGO_OK;
  if (!si_prepare_device()) {
    c->err = std::string(who) + ": the device does not grant the kernel's dynamic LDS";
    return SGO_EHIP;
  }
  int rc;
  if ((rc = mfront_maps_prepare(c, m))) return rc;
  const MfPlan& P = m->plan;
  const int nf = (int)P.fronts.size();
  std::vector<int> pos_front((size_t)std::max(P.n, 1), 0);
  for (int f = 0; f < nf; ++f) {
    const MfFront& F = P.fronts[f];
    for (int p = F.e0; p < F.e0 + F.own; ++p) pos_front[p] = f;
  }
  std::vector<int2> gtile;
  m->gtile_ptr.assign((size_t)P.height + 2, 0);
  for (int h = 0; h <= P.height; ++h) {
    m->gtile_ptr[h] = (int)gtile.size();
    for (int q = P.level_ptr[h]; q < P.level_ptr[h + 1]; ++q) {
      const int f = P.level_front[q];
      if (P.fronts[f].parent < 0) continue;
      const int nt = (3 * P.fronts[f].nb + 15) / 16;
      for (int tc = 0; tc < nt; ++tc)
        for (int tr = tc; tr < nt; ++tr) gtile.push_back(make_int2(f, tr | (tc << 16)));
    }
  }
  m->gtile_ptr[(size_t)P.height + 1] = (int)gtile.size();
  int* d_pf = nullptr;
  int2* d_gt = nullptr;
  double* d_S = nullptr;
  if (gtile.empty()) gtile.push_back(make_int2(0, 0));
  if ((rc = upload(c, &d_pf, pos_front)) || (rc = upload(c, &d_gt, gtile)) || (rc = dalloc(c, &d_S, (size_t)P.arena_doubles))) return rc;
  HIP_TRY(c, hipMemsetAsync(d_S, 0, sizeof(double) * (size_t)std::max<long long>(P.arena_doubles, 1), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the host vectors above go out of scope)
  m->sel.S = d_S;
  m->sel.gtile = d_gt;
  m->sel.pos_front = d_pf;
  m->pos_front = pos_front;
  m->sel_ready = true;
  return SGO_OK;
}

// hessian index -> elimination position
std::vector<int> selinv_positions(const sgo_ctx* c, const Mfront* m) {
  const MfPlan& P = m->plan;
  std::vector<int> pos_of((size_t)c->n, -1);
  for (int p = 0; p < P.n; ++p) {
    const auto f = std::lower_bound(c->free_id.begin(), c->free_id.end(), P.elim_vertex[p]);
    pos_of[(size_t)(f - c->free_id.begin())] = p;
  }
  return pos_of;
}

// The block with the rows of elimination position pi and the columns of pj in the plan's terms: the front of the endpoint
// eliminated first holds it, if any front does (m->pos_front: selinv_prepare's).
bool selinv_pair(const Mfront* m, int pi, int pj, int4* out) {
  const MfPlan& P = m->plan;
  const int plo = std::min(pi, pj), phi = std::max(pi, pj);
  const int f = m->pos_front[plo];
  const MfFront& F = P.fronts[f];
  int lrow = -1;
  if (phi < F.e0 + F.own) lrow = phi - F.e0;
  else {
    const int* b0 = P.bnd.data() + F.bnd_off;
    const int* b = std::lower_bound(b0, b0 + F.nb, phi);
    if (b != b0 + F.nb && *b == phi) lrow = F.own + (int)(b - b0);
  }
  if (lrow < 0) return false;
  // stored block: rows of the later-eliminated pose, columns of the earlier one; the caller's rows are pi's
  *out = make_int4(f, lrow, plo - F.e0, pi < pj ? 1 : 0);
  return true;
}

// The factor phase at the current poses (mfront_factorize: the multifrontal path's own launches), then the selected inversion top-down.
int selinv_run(sgo_ctx* c, Mfront* m) {
  const MfPlan& P = m->plan;
  const MfDev& D = m->dev;
  {
    Scope sc(c, K_MF_FACTOR, mfront_bytes(m, c->E, 1), true);
    HIP_TRY(c, mfront_factorize(m, c->stream, c->el, c->d_poses, c->d_hist, c->d_dres));
  }
  for (int h = P.height; h >= 0; --h) {
    const int cnt = P.level_ptr[h + 1] - P.level_ptr[h];
    const int t0 = m->gtile_ptr[h], t1 = m->gtile_ptr[h + 1];
    if (t1 > t0) {
      Scope sc(c, K_SI_GATHER, 16.0 * 256.0 * (t1 - t0));
      launch_si_gather(c->stream, D, m->sel, t0, t1);
    }
    Scope sc(c, K_SI_PANELS, 0.0);
    launch_si_panels(c->stream, D, m->sel, P.level_ptr[h], cnt, (size_t)m->level_lds[h]);
  }
  m->sel_ran = true;
  return SGO_OK;
}

}  // namespace sgo

extern "C" {

int sgo_marginals_selected(sgo_ctx* c, double* diag, int32_t npairs, const int32_t* vi, const int32_t* vj, double* cov) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (npairs < 0 || (npairs > 0 && (!vi || !vj || !cov))) {
      c->err = "sgo_marginals_selected: null buffer or negative count";
      return SGO_EINVAL;
    }
    if (c->ov.active) {
      c->err = "single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";
      return SGO_EINVAL;
    }
    if (multi_gpu_context(c)) {
      c->err = "sgo_marginals_selected: not available in a multi-GPU context";
      return SGO_EINVAL;
    }
    // hessian index of a free active vertex, -1 for a fixed active one; anything else is refused
    std::vector<int> hi((size_t)npairs), hj((size_t)npairs);
    for (int t = 0; t < npairs; ++t)
      for (int side = 0; side < 2; ++side) {
        const int v = side ? vj[t] : vi[t];
        if (v < 0 || v >= c->V) {
          c->err = "sgo_marginals_selected: vertex id " + std::to_string(v) + " outside [0, " + std::to_string(c->V) + ")";
          return SGO_EINVAL;
        }
        int& h = side ? hj[t] : hi[t];
        const auto f = std::lower_bound(c->free_id.begin(), c->free_id.end(), v);
        if (f != c->free_id.end() && *f == v) h = (int)(f - c->free_id.begin());
        else if (std::binary_search(c->fixed_active.begin(), c->fixed_active.end(), v)) h = -1;
        else {
          c->err = "sgo_marginals_selected: vertex " + std::to_string(v) + " is not active (it has no edge)";
          return SGO_EINVAL;
        }
      }
    if (c->n == 0) {   // every active vertex is fixed: zero blocks, nothing to factorise
      if (diag) std::fill(diag, diag + 9 * (size_t)c->V, 0.0);
      if (npairs > 0) std::fill(cov, cov + 9 * (size_t)npairs, 0.0);
      return 0;
    }
    Mfront* m = nullptr;
    if ((rc = selinv_plan(c, &m, "sgo_marginals_selected", "sgo_marginals"))) return rc;
    const MfPlan& P = m->plan;
    // the pairs in the plan's terms
    const std::vector<int> pos_of = selinv_positions(c, m);
    if ((rc = selinv_prepare(c, m, "sgo_marginals_selected"))) return rc;
    std::vector<int4> pairs((size_t)npairs);
    for (int t = 0; t < npairs; ++t) {
      if (hi[t] < 0 || hj[t] < 0) {
        pairs[t] = make_int4(-1, 0, 0, 0);
        continue;
      }
      if (!selinv_pair(m, pos_of[hi[t]], pos_of[hj[t]], &pairs[t])) {
        c->err = "sgo_marginals_selected: the pair (" + std::to_string(vi[t]) + ", " + std::to_string(vj[t]) +
                 ") lies outside the factor's pattern (no front holds both poses): use sgo_marginals for it";
        return SGO_EINVAL;
      }
    }
    sgo_ctx::SelInv& Z = c->selinv;
    const size_t nout = 9 * ((size_t)c->V + (size_t)npairs) + 1;
    if ((rc = grow_device(c, &Z.d_out, &Z.out_cap, nout)) || (rc = grow_device(c, &Z.d_pairs, &Z.pairs_cap, (size_t)std::max(npairs, 1)))) return rc;
    HIP_TRY(c, hipMemsetAsync(Z.d_out, 0, sizeof(double) * nout, c->stream));
    if (npairs > 0) HIP_TRY(c, hipMemcpyAsync(Z.d_pairs, pairs.data(), sizeof(int4) * (size_t)npairs, hipMemcpyHostToDevice, c->stream));

    if ((rc = selinv_run(c, m))) return rc;
    {
      Scope sc(c, K_SI_RESULT, 16.0 * 9.0 * ((double)c->n + npairs));
      launch_si_result(c->stream, m->dev, m->sel, c->V, npairs, Z.d_pairs, Z.d_out);
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<double> out(nout);
    HIP_TRY(c, hipMemcpyAsync(out.data(), Z.d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    if (out[nout - 1] != 0.0) {
      c->err = "sgo_marginals_selected: the factorisation failed (a pivot block is not positive definite: Hessian not positive definite)";
      return SGO_EINVAL;
    }
    if (diag) std::copy(out.begin(), out.begin() + 9 * (size_t)c->V, diag);
    if (npairs > 0) std::copy(out.begin() + 9 * (size_t)c->V, out.begin() + 9 * ((size_t)c->V + (size_t)npairs), cov);
    return (int)P.fronts.size();
  } SGO_CATCH(c)
}

}  // extern "C"
