// sgo_many.cpp -- sgo_optimize_gn_many (include/sgo.h): many independent pose graphs optimised by one call.
// Replaces: a loop of SparseOptimizer::optimize() over several SparseOptimizers -- one launch of ONE workgroup and one
// synchronisation per graph -- by one launch of k_direct's MANY instantiation with a workgroup per graph (sgo_direct.h); contexts
// that are not on the single-launch path run their own sgo_optimize_gn_until inside the call.
// Writes: every participating context's poses, factor scratch, h_hist / h_dres and error text, as its own call would; the first
// context's `many` workspace.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sgo_ctx.h"
#include "sgo_direct.h"

using namespace sgo;

namespace {

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// where the three pieces of the call's workspace lie, on the device and in the pinned copy alike
struct ManyLayout {
  size_t o_jobs = 0, o_hist = 0, o_res = 0, hist_stride = 0, bytes = 0;
  ManyLayout(int m, int iters) {
    hist_stride = 2 * ((size_t)iters + 1);
    o_jobs = 0;
    o_hist = align256((size_t)m * kDirectJobBytes);
    o_res = o_hist + align256(sizeof(double) * (size_t)m * hist_stride);
    bytes = o_res + align256(sizeof(DirectResult) * (size_t)m);
  }
};

// The first context's workspace, at least `bytes` on both sides.  (Whatever used it before has finished: every call ends behind a
// synchronisation of the stream that carried it.)
int many_reserve(sgo_ctx* owner, size_t bytes) {
  sgo_ctx::Many& W = owner->many;
  int rc = grow_device(owner, &W.d_ws, &W.d_cap, bytes);
  if (rc) {
    owner->err = "sgo_optimize_gn_many: out of device memory (" + std::to_string(bytes) + " bytes of job table and results)";
    return rc;
  }
  if (W.h_cap >= W.d_cap) return SGO_OK;
  if (W.h_ws) hipHostFree(W.h_ws);
  W.h_ws = nullptr;
  W.h_cap = 0;
  if (hipHostMalloc((void**)&W.h_ws, W.d_cap) != hipSuccess) {
    (void)hipGetLastError();
    owner->err = "sgo_optimize_gn_many: out of pinned host memory (" + std::to_string(W.d_cap) + " bytes)";
    return SGO_ENOMEM;
  }
  W.h_cap = W.d_cap;
  return SGO_OK;
}

bool joins_launch(const sgo_ctx* c) { return c->direct && !c->mf && !c->ov.active && c->n > 0 && direct_joins_many(c->direct); }

// The shared launch of the contexts J (all joins_launch) on owner's stream, and the read-back queued behind it.
int many_launch(sgo_ctx* owner, const std::vector<sgo_ctx*>& J, int max_iters, double gain_tol, const ManyLayout& L, int* launches) {
  const int m = (int)J.size();
  int rc = many_reserve(owner, L.bytes);
  if (rc) return rc;
  sgo_ctx::Many& W = owner->many;
  // The launch reads and writes every participant's arrays on the FIRST context's stream: whatever the others have pending on
  // their own streams is waited for on the host (a synchronisation per foreign stream, not an event: the entry points leave
  // their streams idle, and an idle stream costs a synchronisation nothing while an event costs it a packet).
  for (sgo_ctx* c : J)
    if (c != owner) HIP_TRY(owner, hipStreamSynchronize(c->stream));
  std::vector<DirectManyItem> items((size_t)m);
  double* d_hist = reinterpret_cast<double*>(W.d_ws + L.o_hist);
  DirectResult* d_res = reinterpret_cast<DirectResult*>(W.d_ws + L.o_res);
  for (int k = 0; k < m; ++k) items[k] = {J[k]->direct, &J[k]->el, J[k]->d_poses, d_hist + L.hist_stride * (size_t)k, d_res + k};
  DirectManyTable T;
  direct_many_table(m, items.data(), max_iters, gain_tol, W.h_ws + L.o_jobs, &T);
  HIP_TRY(owner, hipMemcpyAsync(W.d_ws + L.o_jobs, W.h_ws + L.o_jobs, (size_t)m * kDirectJobBytes, hipMemcpyHostToDevice, owner->stream));
  for (const DirectManyTable::Launch& l : T.launches) {
    Scope sc(owner, K_DIRECT, l.bytes);
    const hipError_t he = direct_optimize_many(owner->stream, l, W.d_ws + L.o_jobs);
    if (he != hipSuccess) {
      owner->err = std::string("k_direct (many graphs) launch: ") + hipGetErrorString(he);
      return SGO_EHIP;
    }
  }
  *launches = (int)T.launches.size();
  HIP_TRY(owner, hipMemcpyAsync(W.h_ws + L.o_hist, W.d_ws + L.o_hist, sizeof(double) * (size_t)m * L.hist_stride, hipMemcpyDeviceToHost, owner->stream));
  HIP_TRY(owner, hipMemcpyAsync(W.h_ws + L.o_res, W.d_ws + L.o_res, sizeof(DirectResult) * (size_t)m, hipMemcpyDeviceToHost, owner->stream));
  return SGO_OK;
}

int refuse(sgo_ctx* first, const std::string& why, int rc = SGO_EINVAL) {
  g_err = "sgo_optimize_gn_many: " + why;
  if (first) first->err = g_err;
  return rc;
}

}  // namespace

extern "C" {

int sgo_optimize_gn_many(sgo_ctx* const* ctxs, int32_t n, int32_t max_iters, double gain_tol, sgo_stats* const* out, sgo_many_result* res,
                         int32_t* launches) {
  sgo_ctx* const first = (ctxs && n > 0) ? ctxs[0] : nullptr;
  try {
    // ---- refusals: nothing queued, nothing written
    if (n < 0) return refuse(first, "negative number of contexts");
    if (max_iters < 0 || max_iters > SGO_MAX_ITERS) return refuse(first, "max_iters must be in [0, SGO_MAX_ITERS]");
    if (!std::isfinite(gain_tol)) return refuse(first, "gain_tol is not finite");
    if (n > 0 && (!ctxs || !res)) return refuse(first, "null ctxs or res");
    if (n == 0) {
      if (launches) *launches = 0;
      return 0;
    }
    for (int i = 0; i < n; ++i)
      if (!ctxs[i]) return refuse(first, "context " + std::to_string(i) + " is NULL");
    {
      std::vector<const sgo_ctx*> sorted(ctxs, ctxs + n);
      std::sort(sorted.begin(), sorted.end());
      if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return refuse(first, "a context is listed twice");
    }
    for (int i = 0; i < n; ++i) {
      if (ctxs[i]->device != first->device) return refuse(first, "context " + std::to_string(i) + " is on another device than context 0");
      if (multi_gpu_context(ctxs[i])) return refuse(first, "context " + std::to_string(i) + " is a multi-GPU context");
    }
    for (int i = 0; i < n; ++i)
      if (!ctxs[i]->has_graph) return refuse(first, "context " + std::to_string(i) + " has no graph: call sgo_set_graph_se2 first", SGO_ENOGRAPH);
    HIP_TRY(first, hipSetDevice(first->device));
    const double t0 = wall_s();
    // ---- the shared launch of the single-launch contexts, queued with its read-back on the first context's stream
    std::vector<sgo_ctx*> J;
    std::vector<int> at;   // J[k] = ctxs[at[k]]
    for (int i = 0; i < n; ++i)
      if (joins_launch(ctxs[i])) {
        J.push_back(ctxs[i]);
        at.push_back(i);
      }
    const ManyLayout L((int)J.size(), max_iters);
    int nl = 0;
    if (!J.empty()) {
      for (size_t k = 0; k < J.size(); ++k) {
        stats_begin(J[k], max_iters, out ? out[at[k]] : nullptr);
        read_call_knobs(J[k]);
      }
      const int rc = many_launch(first, J, max_iters, gain_tol, L, &nl);
      if (rc) {
        hipStreamSynchronize(first->stream);   // (whatever was queued before the error has finished when the call returns)
        for (sgo_ctx* c : J) c->linearized = false;
        return rc;
      }
    }
    if (launches) *launches = nl;
    // ---- every other context: its own call, while the launch runs
    int good = 0;
    for (int i = 0; i < n; ++i) {
      sgo_ctx* c = ctxs[i];
      if (joins_launch(c)) continue;
      res[i].in_launch = 0;
      res[i].stop_reason = SGO_STOP_MAX_ITERS;
      res[i].rc = sgo_optimize_gn_until(c, max_iters, gain_tol, out ? out[i] : nullptr, &res[i].stop_reason);
      if (res[i].rc >= 0 && res[i].stop_reason != SGO_STOP_FAILED) ++good;
    }
    if (J.empty()) return good;
    // ---- behind the launch (the contexts' later calls are ordered after it by this synchronisation: it has finished when the call
    //      returns): per context what optimize_factored does behind its own
    HIP_TRY(first, hipStreamSynchronize(first->stream));
    prof_flush(first);
    const sgo_ctx::Many& W = first->many;
    for (size_t k = 0; k < J.size(); ++k) {
      sgo_ctx* c = J[k];
      std::memcpy(c->h_hist, W.h_ws + L.o_hist + sizeof(double) * L.hist_stride * k, sizeof(double) * L.hist_stride);
      std::memcpy(c->h_dres, W.h_ws + L.o_res + sizeof(DirectResult) * k, sizeof(DirectResult));
      UntilGain until{gain_tol, SGO_STOP_MAX_ITERS};
      sgo_many_result& r = res[at[k]];
      r.in_launch = 1;
      r.rc = factored_epilogue(c, max_iters, out ? out[at[k]] : nullptr, t0, &until);
      r.stop_reason = until.stop_reason;
      if (r.rc >= 0 && r.stop_reason != SGO_STOP_FAILED) ++good;
    }
    return good;
  } SGO_CATCH(first)
}

int64_t sgo_many_workspace_bytes(sgo_ctx* c) { return c ? (int64_t)(c->many.d_cap + c->many.h_cap) : (int64_t)SGO_EINVAL; }

}  // extern "C"
