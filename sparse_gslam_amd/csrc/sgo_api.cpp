// sgo_api.cpp -- the C-ABI of include/sgo.h (argument checks, error convention, no exception across the boundary) over
// the host runtime of sgo_plan.cpp / sgo_structure.cpp / sgo_solve.cpp and the HIP kernels.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "sgo_ctx.h"
#include "sgo_rules.h"

using namespace sgo;

namespace sgo {
thread_local std::string g_err;  // for ctx == NULL
}

// ---- edge activity: sgo_set_edge_information / sgo_gate_edges (include/sgo.h; kernels in sgo_gate.hip) -----------------------
namespace {

template <class T>
int grow_scratch(sgo_ctx* c, T** p, size_t* cap, size_t count) {
  if (count <= *cap) return SGO_OK;
  if (*p) hipFree(*p);   // (every call that used it has synchronised the stream)
  *p = nullptr;
  *cap = 0;
  const size_t want = count + count / 4 + 64;
  if (hipMalloc((void**)p, want * sizeof(T)) != hipSuccess) {
    c->err = "out of device memory (" + std::to_string(want * sizeof(T)) + " bytes of edge scratch)";
    return SGO_ENOMEM;
  }
  *cap = want;
  return SGO_OK;
}

bool zero_row(const double* r) { return r[0] == 0.0 && r[1] == 0.0 && r[2] == 0.0 && r[3] == 0.0 && r[4] == 0.0 && r[5] == 0.0; }

// The host bookkeeping, made from what the device holds on the first call that needs it.
int edge_activity_ensure(sgo_ctx* c) {
  sgo_ctx::EdgeActivity& A = c->edges;
  if (A.ready) return SGO_OK;
  const int E0 = c->el.E, E1 = c->E - E0, V = c->V;
  if (E1 < 0 || E1 != (c->ov.active ? c->ov.dev.el.cnt : 0) || (size_t)E1 > c->ov.ei.size() || c->ov.fixed.size() != (size_t)V) {
    c->err = "internal error: the appended edges and the overlay's edge list disagree";
    return SGO_EINVAL;
  }
  const size_t E = (size_t)c->E;
  A.vi.resize(E);
  A.vj.resize(E);
  A.dead.resize(E);
  // the endpoints as the device holds them, and one byte per edge from a sweep over the information (not its 48 bytes per edge)
  int rc = grow_scratch(c, &A.d_flag, &A.flag_cap, E);
  if (rc) return rc;
  if (E > 0) {
    launch_edge_dead_flags(c->stream, c->el, E1 > 0 ? &c->ov.dev.el : nullptr, A.d_flag);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(A.dead.data(), A.d_flag, E, hipMemcpyDeviceToHost, c->stream));
  }
  if (E0 > 0) {
    HIP_TRY(c, hipMemcpyAsync(A.vi.data(), c->el.vi, sizeof(int32_t) * (size_t)E0, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(A.vj.data(), c->el.vj, sizeof(int32_t) * (size_t)E0, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t ov0 = c->ov.ei.size() - (size_t)E1;
  for (int k = 0; k < E1; ++k) {
    A.vi[E0 + k] = c->ov.ei[ov0 + k];
    A.vj[E0 + k] = c->ov.ej[ov0 + k];
  }
  A.live_deg.assign((size_t)V, 0);
  A.n_inactive = 0;
  for (size_t e = 0; e < E; ++e) {
    const int a = A.vi[e], b = A.vj[e];
    if (a < 0 || a >= V || b < 0 || b >= V) {
      c->err = "internal error: the device's edge list references a vertex outside [0, V)";
      return SGO_EINVAL;
    }
    if (A.dead[e]) {
      A.n_inactive++;
    } else {
      A.live_deg[a]++;
      A.live_deg[b]++;
    }
  }
  A.ready = true;
  return SGO_OK;
}

// An incremental update appended dE edges (rows info[dE][6]) and possibly vertices: the bookkeeping follows.
void edge_activity_append(sgo_ctx* c, int V, int dE, const int32_t* ei, const int32_t* ej, const double* info) {
  sgo_ctx::EdgeActivity& A = c->edges;
  if (!A.ready) return;
  A.live_deg.resize((size_t)V, 0);
  for (int k = 0; k < dE; ++k) {
    const bool zero = zero_row(info + 6 * (size_t)k);
    A.vi.push_back(ei[k]);
    A.vj.push_back(ej[k]);
    A.dead.push_back(zero ? 1 : 0);
    if (zero) {
      A.n_inactive++;
    } else {
      A.live_deg[ei[k]]++;
      A.live_deg[ej[k]]++;
    }
  }
}

// New information rows for the listed edges (every id once, all in [0, E), all entries finite).  The host decides first -- a change
// that would leave a free pose without any incident edge of non-zero information is refused with nothing written -- then the
// edge lists, and the per-slot copies where they exist, are rewritten and the next solve is told that the operator changed.
int edge_info_apply(sgo_ctx* c, const char* who, const std::vector<int32_t>& ids, const std::vector<double>& rows) {
  sgo_ctx::EdgeActivity& A = c->edges;
  const size_t m = ids.size();
  if (m == 0) return SGO_OK;
  std::vector<uint8_t> now_dead(m);
  // the live-edge counts with the change applied (sign +1) and as they were (sign -1)
  auto count = [&](int sign) {
    for (size_t t = 0; t < m; ++t) {
      const int e = ids[t];
      const int d = sign * ((int)A.dead[e] - (int)now_dead[t]);   // +1: comes back to life, -1: deactivated
      A.live_deg[A.vi[e]] += d;
      A.live_deg[A.vj[e]] += d;
    }
  };
  auto undo = [&]() { count(-1); };
  for (size_t t = 0; t < m; ++t) now_dead[t] = zero_row(&rows[6 * t]) ? 1 : 0;
  count(+1);
  int orphan = -1;
  for (size_t t = 0; t < m && orphan < 0; ++t) {
    const int e = ids[t];
    if (!now_dead[t] || A.dead[e]) continue;
    for (const int v : {A.vi[e], A.vj[e]})
      if (!c->ov.fixed[v] && A.live_deg[v] == 0 && orphan < 0) orphan = v;
  }
  if (orphan >= 0) {
    undo();
    c->err = std::string(who) + ": free vertex " + std::to_string(orphan) +
             " would be left without an incident edge of non-zero information (its Hessian block would be singular)";
    return SGO_EINVAL;
  }
  int rc;
  const bool slots = c->es.info != nullptr && !c->rows_pending && c->d_eidx != nullptr && c->el.E > 0;
  if ((rc = grow_scratch(c, &A.d_ids, &A.ids_cap, m)) || (rc = grow_scratch(c, &A.d_rows, &A.rows_cap, 6 * m))) {
    undo();
    return rc;
  }
  if (slots && (size_t)c->el.E > A.mark_cap) {
    if ((rc = grow_scratch(c, &A.d_mark, &A.mark_cap, (size_t)c->el.E))) {
      undo();
      return rc;
    }
    if (hipMemsetAsync(A.d_mark, 0, A.mark_cap, c->stream) != hipSuccess) {
      A.mark_cap = 0;
      undo();
      c->err = std::string(who) + ": device error";
      return SGO_EHIP;
    }
  }
  hipError_t e = hipMemcpyAsync(A.d_ids, ids.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(A.d_rows, rows.data(), sizeof(double) * 6 * m, hipMemcpyHostToDevice, c->stream);
  if (e != hipSuccess) {   // (nothing of the graph has been written yet)
    undo();
    c->err = std::string(who) + ": " + hipGetErrorString(e);
    return SGO_EHIP;
  }
  launch_edge_info_scatter(c->stream, (int)m, A.d_ids, A.d_rows, c->el, c->ov.active ? &c->ov.dev.el : nullptr, slots ? A.d_mark : nullptr);
  if (slots) {
    launch_slot_info_refresh(c->stream, c->S0.ncs, c->d_eidx, A.d_mark, c->el, c->es);
    e = hipMemsetAsync(A.d_mark, 0, (size_t)c->el.E, c->stream);
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (ids / rows are the caller's frame's)
  for (size_t t = 0; t < m; ++t) {
    const int ed = ids[t];
    A.n_inactive += (int)now_dead[t] - (int)A.dead[ed];
    A.dead[ed] = now_dead[t];
  }
  // The operator changed under the resident structures: whatever was linearised is stale, the next solve refreshes the multigrid
  // hierarchy's coarse operators from the new blocks (no kept operators across the change: the lagged refresh's reference goes),
  // and its iteration count sets a new reference for the count rules, as after an incremental update.
  c->linearized = false;
  c->hier.ref_valid = false;
  c->call.skip_update = false;
  c->hier.new_rhs();
  if (e != hipSuccess) {
    c->err = std::string(who) + ": " + hipGetErrorString(e);
    return SGO_EHIP;
  }
  return SGO_OK;
}

// ---- robust kernels per edge: sgo_set_robust_kernels (include/sgo.h; kernels in sgo_gate.hip) ------------------------------------
// What the device stores for an SGO_KERNEL_* number and its delta: the parameter beside a RobustKind byte (sgo_internal.h).
double robust_phi(int kind, double delta) { return kind == SGO_KERNEL_NONE ? -1.0 : delta; }
unsigned char robust_byte(int kind) { return kind >= SGO_KERNEL_HUBER ? (unsigned char)kind : (unsigned char)kRobustDcs; }

// (kind, delta) for the listed edges (every id once, all in [0, E), every pair valid): the edge lists, the per-slot copies where
// they exist, the host's record and the lists' `kinds` flag; the next solve is told that the operator changed.
int robust_apply(sgo_ctx* c, const char* who, const std::vector<int32_t>& ids, const std::vector<int32_t>& kinds, const std::vector<double>& delta) {
  sgo_ctx::EdgeActivity& A = c->edges;
  sgo_ctx::RobustKinds& R = c->robust;
  const size_t m = ids.size();
  if (m == 0) return SGO_OK;
  std::vector<double> phi(m);
  std::vector<unsigned char> bytes(m);
  for (size_t t = 0; t < m; ++t) {
    phi[t] = robust_phi(kinds[t], delta[t]);
    bytes[t] = robust_byte(kinds[t]);
  }
  int rc;
  const bool slots = c->es.phi != nullptr && !c->rows_pending && c->d_eidx != nullptr && c->el.E > 0;
  if ((rc = grow_scratch(c, &A.d_ids, &A.ids_cap, m)) || (rc = grow_scratch(c, &A.d_rows, &A.rows_cap, m)) ||
      (rc = grow_scratch(c, &R.d_kind, &R.kind_cap, m)))
    return rc;
  if (slots && (size_t)c->el.E > A.mark_cap) {
    if ((rc = grow_scratch(c, &A.d_mark, &A.mark_cap, (size_t)c->el.E))) return rc;
    if (hipMemsetAsync(A.d_mark, 0, A.mark_cap, c->stream) != hipSuccess) {
      A.mark_cap = 0;
      c->err = std::string(who) + ": device error";
      return SGO_EHIP;
    }
  }
  hipError_t e = hipMemcpyAsync(A.d_ids, ids.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(A.d_rows, phi.data(), sizeof(double) * m, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(R.d_kind, bytes.data(), m, hipMemcpyHostToDevice, c->stream);
  if (e != hipSuccess) {   // (nothing of the graph has been written yet)
    c->err = std::string(who) + ": " + hipGetErrorString(e);
    return SGO_EHIP;
  }
  launch_edge_kernel_scatter(c->stream, (int)m, A.d_ids, A.d_rows, R.d_kind, c->el, c->ov.active ? &c->ov.dev.el : nullptr, slots ? A.d_mark : nullptr);
  if (slots) {
    launch_slot_kernel_refresh(c->stream, c->S0.ncs, c->d_eidx, A.d_mark, c->el, c->es);
    e = hipMemsetAsync(A.d_mark, 0, (size_t)c->el.E, c->stream);
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the staging vectors are this frame's)
  // the host's record: made from what phi said (an edge never listed is NONE or DCS, and which of the two nobody asks)
  if (R.kind.size() != (size_t)c->E) R.kind.resize((size_t)c->E, (uint8_t)SGO_KERNEL_DCS);
  for (size_t t = 0; t < m; ++t) {
    uint8_t& k = R.kind[ids[t]];
    R.n_other += (int)(kinds[t] >= SGO_KERNEL_HUBER) - (int)(k >= SGO_KERNEL_HUBER);
    k = (uint8_t)kinds[t];
  }
  c->el.kinds = c->es.kinds = c->ov.dev.el.kinds = R.n_other > 0 ? 1 : 0;
  // as after sgo_set_edge_information: the operator changed under the resident structures
  c->linearized = false;
  c->hier.ref_valid = false;
  c->call.skip_update = false;
  c->hier.new_rhs();
  if (e != hipSuccess) {
    c->err = std::string(who) + ": " + hipGetErrorString(e);
    return SGO_EHIP;
  }
  return SGO_OK;
}

}  // namespace

// =============================================================================== C-ABI
extern "C" {

int sgo_version(void) { return SGO_VERSION; }

void sgo_default_opts(sgo_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = (int32_t)sizeof(sgo_opts);
  o->solver = SGO_SOLVER_PCG_AMG;
  o->pcg_tol = 1e-8;
  o->pcg_maxit = 20000;
  o->pcg_chunk = 16;
  o->use_graph = 1;
  o->profile = 0;
  o->verbose = 0;
  o->direct_rows = 8192;
  o->pcg_tol_cap = 1e-6;
  o->pcg_warm_start = 1;
  if (const char* s = std::getenv("SGO_PCG_WARM")) o->pcg_warm_start = std::atoi(s);
  if (const char* s = std::getenv("SGO_PCG_TOL_CAP")) o->pcg_tol_cap = std::atof(s);
  if (const char* s = std::getenv("SGO_DIRECT_ROWS")) o->direct_rows = std::atoi(s);
  if (const char* s = std::getenv("SGO_SOLVER")) {
    if (!std::strcmp(s, "pcg") || !std::strcmp(s, "bj")) o->solver = SGO_SOLVER_PCG_BJ;
    else if (!std::strcmp(s, "amg")) o->solver = SGO_SOLVER_PCG_AMG;
  }
  if (const char* s = std::getenv("SGO_PCG_TOL")) o->pcg_tol = std::atof(s);
  if (const char* s = std::getenv("SGO_PCG_MAXIT")) o->pcg_maxit = std::atoi(s);
  if (const char* s = std::getenv("SGO_PCG_CHUNK")) o->pcg_chunk = std::atoi(s);
  if (const char* s = std::getenv("SGO_USE_GRAPH")) o->use_graph = std::atoi(s);
  if (const char* s = std::getenv("SGO_PROFILE")) o->profile = std::atoi(s);
  if (const char* s = std::getenv("SGO_VERBOSE")) o->verbose = std::atoi(s);
}

sgo_ctx* sgo_create(int device, const sgo_opts* opts) {
  if (device < 0) {
    const char* s = std::getenv("SGO_DEVICE");
    device = s ? std::atoi(s) : 0;
  }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    g_err = std::string("no HIP device available: ") + hipGetErrorString(e);
    return nullptr;
  }
  if (device >= count) {
    g_err = "device ordinal " + std::to_string(device) + " out of range (" + std::to_string(count) + " devices)";
    return nullptr;
  }
  if ((e = hipSetDevice(device)) != hipSuccess) {
    g_err = std::string("hipSetDevice: ") + hipGetErrorString(e);
    return nullptr;
  }
  sgo_ctx* c = new (std::nothrow) sgo_ctx();
  if (!c) {
    g_err = "out of host memory";
    return nullptr;
  }
  c->device = device;
  sgo_default_opts(&c->opts);
  if (opts) {
    size_t sz = std::min<size_t>(sizeof(sgo_opts), opts->struct_size > 0 ? (size_t)opts->struct_size : sizeof(sgo_opts));
    std::memcpy(&c->opts, opts, sz);
    c->opts.struct_size = (int32_t)sizeof(sgo_opts);
  }
  if (c->opts.pcg_tol <= 0) c->opts.pcg_tol = 1e-8;
  if (c->opts.pcg_maxit <= 0) c->opts.pcg_maxit = 20000;
  if (c->opts.pcg_chunk <= 0) c->opts.pcg_chunk = 16;
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipHostMalloc((void**)&c->h_S, sizeof(PcgScalars))) != hipSuccess ||
      (e = hipHostMalloc((void**)&c->h_S2, 2 * sizeof(PcgScalars))) != hipSuccess ||
      (e = hipHostMalloc((void**)&c->h_Sz, sizeof(PcgScalars))) != hipSuccess ||
      (e = hipHostGetDevicePointer((void**)&c->d_Sz, c->h_Sz, 0)) != hipSuccess ||
      (e = hipHostMalloc((void**)&c->h_dchg, 6 * sizeof(double) * kMaxPartials)) != hipSuccess ||
      (e = hipHostGetDevicePointer((void**)&c->h_dchg_dev, c->h_dchg, 0)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_S[0], hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_S[1], hipEventDisableTiming)) != hipSuccess ||
      (e = hipHostMalloc((void**)&c->h_hist, sizeof(double) * 2 * (SGO_MAX_ITERS + 2))) != hipSuccess ||
      (e = hipHostMalloc((void**)&c->h_dres, sizeof(DirectResult))) != hipSuccess ||
      (e = hipMalloc((void**)&c->d_dres, sizeof(DirectResult))) != hipSuccess) {
    g_err = std::string("context setup: ") + hipGetErrorString(e);
    sgo_destroy(c);
    return nullptr;
  }
  return c;
}

void sgo_destroy(sgo_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  prof_flush(c);
  free_graph(c);
  c->graph_arena.release();
  c->amg_arena.release();
  c->amg_arena_prev.release();
  c->amg_tmp_arena.release();
  c->comm.destroy();
  overlay_release(c->ov);
  for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
  for (hipEvent_t e : c->iter_events) hipEventDestroy(e);
  if (c->h_S) hipHostFree(c->h_S);
  if (c->h_S2) hipHostFree(c->h_S2);
  if (c->h_Sz) hipHostFree(c->h_Sz);
  if (c->h_dchg) hipHostFree(c->h_dchg);
  if (c->h_pose_stage) hipHostFree(c->h_pose_stage);
  for (hipEvent_t ev : c->ev_S)
    if (ev) hipEventDestroy(ev);
  if (c->h_hist) hipHostFree(c->h_hist);
  if (c->halo_send) hipFree(c->halo_send);
  if (c->halo_recv) hipFree(c->halo_recv);
  if (c->h_dres) hipHostFree(c->h_dres);
  if (c->d_dres) hipFree(c->d_dres);
  if (c->d_comm_flag) hipFree(c->d_comm_flag);
  if (c->edges.d_ids) hipFree(c->edges.d_ids);
  if (c->edges.d_rows) hipFree(c->edges.d_rows);
  if (c->edges.d_flag) hipFree(c->edges.d_flag);
  if (c->edges.d_mark) hipFree(c->edges.d_mark);
  if (c->edges.d_parts) hipFree(c->edges.d_parts);
  if (c->robust.d_kind) hipFree(c->robust.d_kind);
  if (c->marg.d_cov) hipFree(c->marg.d_cov);
  if (c->marg.d_idx) hipFree(c->marg.d_idx);
  if (c->selinv.d_out) hipFree(c->selinv.d_out);
  if (c->selinv.d_pairs) hipFree(c->selinv.d_pairs);
  if (c->selinv.d_fs) hipFree(c->selinv.d_fs);
  if (c->selinv.d_cand) hipFree(c->selinv.d_cand);
  if (c->selinv.d_cidx) hipFree(c->selinv.d_cidx);
  if (c->selinv.d_loo) hipFree(c->selinv.d_loo);
  if (c->selinv.d_loo_ids) hipFree(c->selinv.d_loo_ids);
  if (c->selinv.d_search) hipFree(c->selinv.d_search);
  if (c->selinv.d_search_idx) hipFree(c->selinv.d_search_idx);
  if (c->lm.d_trial) hipFree(c->lm.d_trial);
  if (c->lm.d_scratch) hipFree(c->lm.d_scratch);
  if (c->lm.d_state) hipFree(c->lm.d_state);
  if (c->dl.d_vec) hipFree(c->dl.d_vec);
  if (c->dl.d_scratch) hipFree(c->dl.d_scratch);
  if (c->dl.d_state) hipFree(c->dl.d_state);
  for (void* p : {(void*)c->joint.d_tab[0], (void*)c->joint.d_tab[1], (void*)c->joint.d_raw, (void*)c->joint.d_d2, (void*)c->joint.d_mask,
                  (void*)c->joint.d_grow, (void*)c->joint.d_gout, (void*)c->joint.d_gint, (void*)c->ejoint.d_tab[0], (void*)c->ejoint.d_tab[1],
                  (void*)c->ejoint.d_out, (void*)c->ejoint.d_mask})
    if (p) hipFree(p);
  if (c->hyp.d_ws) hipFree(c->hyp.d_ws);
  if (c->many.d_ws) hipFree(c->many.d_ws);
  if (c->many.h_ws) hipHostFree(c->many.h_ws);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
}

const char* sgo_solver_description(sgo_ctx* c) {
  if (!c || !c->has_graph) return "";
  try {
    c->solver_text = c->solver_desc;
    if (!c->direct && !c->direct_why.empty()) c->solver_text += "; direct path not used: " + c->direct_why;
    if (!c->direct && !c->mf && !c->mf_why.empty()) c->solver_text += "; multifrontal path not used: " + c->mf_why;
    if (c->ov.active)
      c->solver_text += "; incremental overlay: " + std::to_string(c->ov.new_vertex.size()) + " appended rows (" + std::to_string(c->ov.dev.nx) +
                        " hubs), " + std::to_string(c->ov.dev.nt) + " touched rows, " + std::to_string(c->ov.dev.el.cnt) + " appended edges (" +
                        std::to_string(c->ov.updates) + " updates)";
    if (!c->update_note.empty()) c->solver_text += "; last update: " + c->update_note;
    if (!c->lag_note.empty()) c->solver_text += "; " + c->lag_note;
    if (c->edges.n_inactive > 0) c->solver_text += "; " + std::to_string(c->edges.n_inactive) + " edges inactive";
    return c->solver_text.c_str();
  } catch (...) {   // no C++ exception crosses the C boundary
    return "";
  }
}

const char* sgo_last_error(sgo_ctx* c) { return c ? c->err.c_str() : g_err.c_str(); }

int sgo_set_graph_se2(sgo_ctx* c, int32_t V, const double* poses, const uint8_t* fixed, int32_t E, const int32_t* ei,
                      const int32_t* ej, const double* meas, const double* info, const double* phi) {
  try {
    if (!c) return SGO_EINVAL;
    if (V <= 0 || E < 0 || !poses || !fixed || (E > 0 && (!ei || !ej || !meas || !info || !phi))) {
      c->err = "sgo_set_graph_se2: bad argument";
      return SGO_EINVAL;
    }
    if (2 * (int64_t)E + (int64_t)V > (int64_t)INT32_MAX / 2) {  // slot indices are 32-bit (2E + n slots)
      c->err = "sgo_set_graph_se2: graph too large for 32-bit slot indices";
      return SGO_EINVAL;
    }
    read_call_knobs(c);   // (which set-up the multigrid hierarchy takes is decided here: the helper thread of the pipeline depends on it)
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) {
      c->err = std::string("hipSetDevice: ") + hipGetErrorString(e);
      return SGO_EHIP;
    }
    const double t0 = wall_s();
    hipStreamSynchronize(c->stream);
    free_graph(c);
    if (c->opts.verbose) std::fprintf(stderr, "[sgo] set_graph: release of the previous graph %.1f ms\n", 1e3 * (wall_s() - t0));
    int rc = build_edges(c, V, poses, fixed, E, ei, ej, meas, info, phi);
    if (rc != SGO_OK) {
      free_graph(c);
      return rc;
    }
    c->has_graph = true;
    c->solver_desc = "pcg_block_jacobi";
    c->direct_why.clear();
    if (c->opts.solver == SGO_SOLVER_PCG_AMG && c->n > 0 && c->opts.direct_rows > 0 && c->comm.nranks <= 1 && !c->comm.active()) {
      // Small graphs (the reference's own sizes): optimize() as ONE launch of a sparse direct solver when the
      // elimination analysis fits (sgo_direct.h); the multigrid hierarchy is then built only if a single-step
      // entry point asks for it.
      std::string derr;
      const double td0 = wall_s();
      c->direct = direct_create(c->stream, &c->graph_arena, V, c->n, c->free_id.data(), E, ei, ej, c->opts.direct_rows,
                                &c->direct_why, &derr);
      if (!c->direct && !derr.empty()) {
        c->err = derr;
        free_graph(c);
        return SGO_EHIP;
      }
      if (c->opts.verbose) std::fprintf(stderr, "[sgo] set_graph: direct-path analysis %.2f ms\n", 1e3 * (wall_s() - td0));
      if (c->direct) {
        const DirectInfo& di = direct_info(c->direct);
        c->solver_desc = "direct_ldlt: " + std::to_string(di.n_chain) + " chain poses in " + std::to_string(di.levels) +
                         " levels + " + std::to_string(di.n_sep) + " separators (dense), " + std::to_string(di.slots) +
                         " stored blocks, " + std::to_string(di.contributions) + " block products per factorisation; pcg_amg on demand";
        c->amg_pending = true;
        // the row plan and the level-0 structures of the PCG path wait for the first entry point that needs them
        c->rows_pending = true;
        c->lz_fixed.assign(fixed, fixed + V);
        c->lz_ei.assign(ei, ei + E);
        c->lz_ej.assign(ej, ej + E);
      } else if (c->opts.verbose) {
        std::fprintf(stderr, "[sgo] direct path not used: %s\n", c->direct_why.c_str());
      }
      // Mid-size graphs (the reference's largest: a few thousand poses, a closure every few poses): a multifrontal sparse
      // Cholesky factorisation, one launch per level of the elimination tree (sgo_mfront.h), when the tree's critical path
      // is short enough.  SGO_MFRONT=0 keeps the multigrid PCG; SGO_MFRONT_ROWS bounds the graph size.
      bool mf_on = true;
      int mf_rows = 12288;
      if (const char* s = std::getenv("SGO_MFRONT")) mf_on = std::atoi(s) != 0;
      if (const char* s = std::getenv("SGO_MFRONT_ROWS")) mf_rows = std::atoi(s);
      c->mf_why.clear();
      if (!c->direct && mf_on && mf_rows > 0) {
        std::string merr;
        const double tm0 = wall_s();
        c->mf = mfront_create(c->stream, &c->graph_arena, V, c->n, c->free_id.data(), poses, E, ei, ej, mf_rows, &c->mf_order_hint, &c->mf_why, &merr);
        if (!c->mf && !merr.empty()) {
          c->err = merr;
          free_graph(c);
          return SGO_EHIP;
        }
        if (c->opts.verbose) std::fprintf(stderr, "[sgo] set_graph: multifrontal analysis %.2f ms\n", 1e3 * (wall_s() - tm0));
        if (c->mf) {
          const MfrontInfo& mi = mfront_info(c->mf);
          char buf[320];
          std::snprintf(buf, sizeof buf, "multifrontal_cholesky: %d fronts in %d levels (nested dissection in %s order), largest front %d rows "
                        "(%d own + %d boundary poses), %.0f Mflop per factorisation, %.1f on the critical path in %d panels, %.1f MB of fronts; "
                        "pcg_amg on demand", mi.fronts, mi.height + 1, mi.order_kind == 0 ? "Hilbert" : "id", mi.max_dim, mi.max_own, mi.max_bnd,
                        1e-6 * mi.flops, 1e-6 * mi.crit_flops, mi.crit_panels, 1e-6 * (double)mi.arena_bytes);
          c->solver_desc = buf;
          c->amg_pending = true;
          c->rows_pending = true;
          c->lz_fixed.assign(fixed, fixed + V);
          c->lz_ei.assign(ei, ei + E);
          c->lz_ej.assign(ej, ej + E);
        } else if (c->opts.verbose) {
          std::fprintf(stderr, "[sgo] multifrontal path not used: %s\n", c->mf_why.c_str());
        }
      }
    }
    if (!c->rows_pending) {
      // a graph whose initial poses contradict its closures gets its ROW ORDER from spanning-tree positions (sgo_plan.cpp)
      const double tp0 = wall_s();
      if (!plan_order_positions(V, poses, fixed, E, ei, ej, meas, c->order_xy)) c->order_xy.clear();
      else if (c->opts.verbose)
        std::fprintf(stderr, "[sgo] set_graph: the initial poses contradict the closures: row order from spanning-tree positions (%.1f ms)\n",
                     1e3 * (wall_s() - tp0));
    }
    if (!c->rows_pending && (rc = build_rows(c, poses, fixed, ei, ej)) != SGO_OK) {
      free_graph(c);
      return rc;
    }
    if (c->opts.solver != SGO_SOLVER_PCG_AMG) c->solver_desc += multi_gpu_description(c);
    if (c->opts.solver == SGO_SOLVER_PCG_AMG && c->n > 0 && !c->direct && !c->mf) {
      // the hierarchy is built from the Hessian at the initial poses (strength of connection)
      const double ta0 = wall_s();
      if ((rc = do_linearize(c)) != SGO_OK || (rc = build_amg(c)) != SGO_OK) {
        free_graph(c);
        return rc;
      }
      if (c->opts.verbose) std::fprintf(stderr, "[sgo] set_graph: multigrid set-up %.1f ms\n", 1e3 * (wall_s() - ta0));
      c->linearized = false;
    }
    // what an incremental update (sgo_update_graph_se2) appends to
    c->ov.base_V = V;
    c->ov.base_E = E;
    c->ov.base_n = c->n;
    c->ov.fixed.assign(fixed, fixed + V);
    c->setup_seconds = wall_s() - t0;
    if (c->opts.verbose)
      std::fprintf(stderr, "[sgo] solver: %s\n[sgo] set_graph: total %.1f ms\n", c->solver_desc.c_str(), 1e3 * c->setup_seconds);
    return SGO_OK;
  } SGO_CATCH(c)
}

// Incremental re-initialisation: see include/sgo.h and sgo_overlay.h.
int sgo_update_graph_se2(sgo_ctx* c, int32_t V, const double* poses, const uint8_t* fixed, int32_t E, const int32_t* ei,
                         const int32_t* ej, const double* meas, const double* info, const double* phi, int32_t n_resident_edges) {
  try {
    if (!c) return SGO_EINVAL;
    if (V <= 0 || E < 0 || !poses || !fixed || (E > 0 && (!ei || !ej || !meas || !info || !phi)) || n_resident_edges < 0 || n_resident_edges > E) {
      c->err = "sgo_update_graph_se2: bad argument";
      return SGO_EINVAL;
    }
    const double t0 = wall_s();
    Overlay& ov = c->ov;
    std::string why;
    const int res_E = c->has_graph ? ov.base_E + (int)ov.ei.size() : 0;
    bool env_on = true;
    if (const char* e = std::getenv("SGO_INCREMENTAL")) env_on = std::atoi(e) != 0;
    if (!c->has_graph) why = "no resident graph";
    else if (!env_on) why = "disabled (SGO_INCREMENTAL=0)";
    else if (n_resident_edges == 0) why = "the caller reports no common prefix";
    // (c->direct / c->mf themselves, not only the pending flags: a single-step entry point -- sgo_linearize, sgo_solve -- builds the
    // PCG structures of such a graph on demand and clears the flags, while sgo_optimize_gn keeps taking the factorisation path,
    // which knows nothing of an overlay)
    else if (c->mf) why = "the resident graph takes the multifrontal path (its set-up is cheap)";
    else if (c->direct) why = "the resident graph takes the single-launch direct path (its set-up is cheap)";
    else if (c->rows_pending || c->amg_pending) why = "the resident graph's PCG structures are not built";
    else if (!c->amg || c->opts.solver != SGO_SOLVER_PCG_AMG) why = "no multigrid hierarchy resident";
    else if (c->comm.nranks > 1 || c->comm.active()) why = "multi-GPU contexts re-partition";
    else if (n_resident_edges != res_E || V < c->V) why = "the resident graph is not a prefix of the new one";
    else if (V - ov.base_V > kOvMaxVerts || E - ov.base_E > kOvMaxEdges) why = "the appended part has outgrown the overlay";
    else if (std::memcmp(fixed, ov.fixed.data(), (size_t)c->V) != 0) why = "fixed flags of resident vertices changed";
    else if (ov.hpos.size() != (size_t)ov.base_V) why = "no row map of the resident structure";
    // an overlay that costs too many PCG iterations (counts only: the first solves of the optimize() calls, which run at the same
    // relative tolerance) is dropped for a fresh hierarchy that knows the closures
    else if (ov.active && c->its_base > 0 && 4 * c->its_last > 5 * c->its_base + 12) why = "the overlay costs too many PCG iterations";
    if (why.empty()) {
      for (int e = n_resident_edges; e < E; ++e) {
        const int a = ei[e], b = ej[e];
        if (a < 0 || a >= V || b < 0 || b >= V) {
          c->err = "edge " + std::to_string(e) + " references a vertex outside [0, V)";
          return SGO_EINVAL;
        }
        if (a == b) {
          c->err = "edge " + std::to_string(e) + " is a self edge";
          return SGO_EINVAL;
        }
      }
      hipError_t he = hipSetDevice(c->device);
      if (he != hipSuccess) {
        c->err = std::string("hipSetDevice: ") + hipGetErrorString(he);
        return SGO_EHIP;
      }
      // the update is tried on copies of the host state: a shape the overlay cannot take leaves the resident graph as it was
      const size_t old_ne = ov.ei.size();
      const int dE = E - n_resident_edges;
      ov.ei.insert(ov.ei.end(), ei + n_resident_edges, ei + E);
      ov.ej.insert(ov.ej.end(), ej + n_resident_edges, ej + E);
      const std::vector<unsigned char> old_fixed = ov.fixed;
      ov.fixed.assign(fixed, fixed + V);
      double tl = wall_s();
      auto lap = [&](const char* what) {
        if (c->opts.verbose > 2) hipStreamSynchronize(c->stream);   // (diagnostic: charge the device time to the phase that queued it)
        const double t = wall_s();
        if (c->opts.verbose > 1) std::fprintf(stderr, "[sgo]   update %-16s %.3f ms\n", what, 1e3 * (t - tl));
        tl = t;
      };
      hipStreamSynchronize(c->stream);   // (nothing of an earlier optimize() may still read the overlay's structure arrays)
      lap("stream drain");
      bool ok = overlay_upload_edges(ov, c->stream, (int)old_ne, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &c->err);   // (allocates on first use)
      const OverlayDev old_dev = ov.dev;   // (with the device pointers in place: restored when the new shape is refused)
      const std::vector<int> old_new = ov.new_vertex;
      if (ok) ok = overlay_upload_edges(ov, c->stream, (int)old_ne, dE, ei + n_resident_edges, ej + n_resident_edges,
                                     meas + 3 * (size_t)n_resident_edges, info + 6 * (size_t)n_resident_edges, phi + n_resident_edges, &c->err);
      lap("edge upload");
      if (ok) ok = overlay_build(ov, V, c->stream, &why, &c->err);
      lap("overlay build");
      if (ok && upload_poses(c, poses, V) != SGO_OK) {
        ok = false;
        why = "pose upload failed";
      }
      if (ok && hipStreamSynchronize(c->stream) != hipSuccess) {   // the caller's arrays may go away after the call
        ok = false;
        why = "device error";
      }
      lap("poses + sync");
      if (ok) {
        ov.active = ov.dev.k + ov.dev.nt + ov.dev.nx > 0;
        ov.updates++;
        c->V = V;
        c->E = E;
        c->linearized = false;
        c->joint.n = -1;   // (sgo_candidate_joint's table described the graph before the update)
        c->ejoint.n = -1;  // (... and sgo_edge_joint's)
        edge_activity_append(c, V, dE, ei + n_resident_edges, ej + n_resident_edges, info + 6 * (size_t)n_resident_edges);
        if (!c->robust.kind.empty()) c->robust.kind.resize((size_t)E, (uint8_t)SGO_KERNEL_DCS);   // (appended edges: what phi says)
        ov.dev.el.kinds = c->el.kinds;
        // the hierarchy's own staleness rule compares a solve with the best count seen so far (sgo_policy.h): the solves after
        // an update have another right-hand side (the appended poses' residual) -- their first one sets a new reference
        c->hier.new_rhs();
        c->setup_seconds = wall_s() - t0;
        c->update_note = "incremental (" + std::to_string(dE) + " edges appended in " + std::to_string(1e3 * c->setup_seconds).substr(0, 5) + " ms)";
        if (c->opts.verbose)
          std::fprintf(stderr, "[sgo] update_graph: %d edges / %d vertices appended as overlay (%d chain rows, %d hubs, %d touched) in %.2f ms\n", dE,
                       V - (int)old_fixed.size(), ov.dev.k, ov.dev.nx, ov.dev.nt, 1e3 * c->setup_seconds);
        return SGO_OK;
      }
      ov.ei.resize(old_ne);
      ov.ej.resize(old_ne);
      ov.fixed = old_fixed;
      ov.dev = old_dev;
      ov.new_vertex = old_new;
      if (why.empty()) why = "overlay set-up failed";
    }
    if (c->opts.verbose) std::fprintf(stderr, "[sgo] update_graph: full set-up (%s)\n", why.c_str());
    // the kinds sgo_set_robust_kernels gave the resident prefix outlive the set-up, with delta from the phi passed now
    std::vector<int32_t> kept_id, kept_kind;
    std::vector<double> kept_delta;
    if (c->has_graph && !multi_gpu_context(c))
      for (size_t e = 0; e < c->robust.kind.size() && e < (size_t)n_resident_edges; ++e) {
        const int k = c->robust.kind[e];
        if (k == SGO_KERNEL_DCS || (k != SGO_KERNEL_NONE && !(phi[e] > 0.0 && std::isfinite(phi[e])))) continue;   // (what phi says already)
        kept_id.push_back((int32_t)e);
        kept_kind.push_back(k);
        kept_delta.push_back(phi[e]);
      }
    int rc = sgo_set_graph_se2(c, V, poses, fixed, E, ei, ej, meas, info, phi);
    if (rc == SGO_OK && !kept_id.empty()) {
      const double ts = c->setup_seconds;
      rc = robust_apply(c, "sgo_update_graph_se2", kept_id, kept_kind, kept_delta);
      c->setup_seconds = ts;
    }
    if (rc == SGO_OK) c->update_note = "full set-up (" + why + ")";
    return rc;
  } SGO_CATCH(c)
}

int sgo_set_poses(sgo_ctx* c, const double* poses) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (!poses) return SGO_EINVAL;
    if ((rc = upload_poses(c, poses, c->V))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->linearized = false;
    return SGO_OK;
  } SGO_CATCH(c)
}

int sgo_get_poses(sgo_ctx* c, double* poses) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (!poses) return SGO_EINVAL;
    HIP_TRY(c, hipMemcpyAsync(poses, c->d_poses, sizeof(double) * 3 * (size_t)c->V, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SGO_OK;
  } SGO_CATCH(c)
}

int sgo_num_free(sgo_ctx* c) {
  int rc = check_graph(c);
  return rc ? rc : c->n + (c->ov.active ? (int)c->ov.new_vertex.size() : 0);
}

int sgo_free_ids(sgo_ctx* c, int32_t* out) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (!out) return SGO_EINVAL;
    if (c->ov.active && !c->ov.new_vertex.empty()) {   // g2o's hessian order over the resident and the appended free poses
      std::merge(c->free_id.begin(), c->free_id.end(), c->ov.new_vertex.begin(), c->ov.new_vertex.end(), out);
      return c->n + (int)c->ov.new_vertex.size();
    }
    std::copy(c->free_id.begin(), c->free_id.end(), out);
    return c->n;
  } SGO_CATCH(c)
}

int sgo_chi2(sgo_ctx* c, double* plain, double* robust) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (c->direct && !c->ov.active) {
      // Single-launch path: the sums are k_direct's own closing pass (a call of 0 iterations: it writes the two sums and its scratch
      // result record, nothing else), so that they equal the final entry of the history of the call before, sgo_optimize_gn's or
      // sgo_optimize_gn_until's, bit for bit -- as they do on the other paths, whose histories are do_chi2's.  k_chi2 forms the
      // edge error from another sincos and adds in another order: the same sums to rounding, not to the bit.
      Scope sc(c, K_DIRECT, direct_bytes(c->direct, c->E, 0));
      const hipError_t he = direct_optimize(c->direct, c->stream, c->el, c->d_poses, 0, c->d_hist, c->d_dres, nullptr);
      if (he != hipSuccess) {
        c->err = std::string("k_direct launch: ") + hipGetErrorString(he);
        return SGO_EHIP;
      }
    } else if ((rc = do_chi2(c, c->d_hist, nullptr))) {
      return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(c->h_hist, c->d_hist, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (plain) *plain = c->h_hist[0];
    if (robust) *robust = c->h_hist[1];
    return SGO_OK;
  } SGO_CATCH(c)
}

int sgo_edge_chi2(sgo_ctx* c, double* e2) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (!e2) return SGO_EINVAL;
    if ((rc = do_chi2(c, c->d_hist, c->d_e2))) return rc;
    HIP_TRY(c, hipMemcpyAsync(e2, c->d_e2, sizeof(double) * (size_t)c->E, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SGO_OK;
  } SGO_CATCH(c)
}

int sgo_set_edge_information(sgo_ctx* c, int32_t n, const int32_t* edge_ids, const double* info) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!edge_ids || !info))) {
      c->err = "sgo_set_edge_information: null buffer or negative count";
      return SGO_EINVAL;
    }
    if (multi_gpu_context(c)) {
      c->err = "sgo_set_edge_information: not available in a multi-GPU context (call sgo_set_graph_se2)";
      return SGO_EINVAL;
    }
    for (int t = 0; t < n; ++t) {
      if (edge_ids[t] < 0 || edge_ids[t] >= c->E) {
        c->err = "sgo_set_edge_information: edge id " + std::to_string(edge_ids[t]) + " outside [0, " + std::to_string(c->E) + ")";
        return SGO_EINVAL;
      }
      for (int q = 0; q < 6; ++q)
        if (!std::isfinite(info[6 * (size_t)t + q])) {
          c->err = "sgo_set_edge_information: non-finite information entry for edge " + std::to_string(edge_ids[t]);
          return SGO_EINVAL;
        }
    }
    if (n == 0) return SGO_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = edge_activity_ensure(c))) return rc;
    // every id once: of an id listed twice the later row counts
    std::vector<int32_t> order((size_t)n);
    for (int t = 0; t < n; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return edge_ids[a] < edge_ids[b]; });
    std::vector<int32_t> ids;
    std::vector<double> rows;
    for (int k = 0; k < n; ++k) {
      const int t = order[k];
      if (k + 1 < n && edge_ids[order[k + 1]] == edge_ids[t]) continue;
      ids.push_back(edge_ids[t]);
      rows.insert(rows.end(), info + 6 * (size_t)t, info + 6 * (size_t)t + 6);
    }
    return edge_info_apply(c, "sgo_set_edge_information", ids, rows);
  } SGO_CATCH(c)
}

int sgo_gate_edges(sgo_ctx* c, int32_t n, const int32_t* edge_ids, double chi2_max, uint8_t* gated) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (edge_ids && n < 0) {
      c->err = "sgo_gate_edges: negative count";
      return SGO_EINVAL;
    }
    if (multi_gpu_context(c)) {
      c->err = "sgo_gate_edges: not available in a multi-GPU context (gate on the host and call sgo_set_graph_se2)";
      return SGO_EINVAL;
    }
    const int items = edge_ids ? n : c->E;
    for (int t = 0; edge_ids && t < n; ++t)
      if (edge_ids[t] < 0 || edge_ids[t] >= c->E) {
        c->err = "sgo_gate_edges: edge id " + std::to_string(edge_ids[t]) + " outside [0, " + std::to_string(c->E) + ")";
        return SGO_EINVAL;
      }
    if (items == 0) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = edge_activity_ensure(c))) return rc;
    sgo_ctx::EdgeActivity& A = c->edges;
    if ((rc = grow_scratch(c, &A.d_flag, &A.flag_cap, (size_t)items)) || (rc = grow_scratch(c, &A.d_parts, &A.parts_cap, (size_t)kMaxPartials + 1)) ||
        (edge_ids && (rc = grow_scratch(c, &A.d_ids, &A.ids_cap, (size_t)items))))
      return rc;
    if (edge_ids) HIP_TRY(c, hipMemcpyAsync(A.d_ids, edge_ids, sizeof(int32_t) * (size_t)items, hipMemcpyHostToDevice, c->stream));
    // the decision first: flags and their count, the graph untouched
    int* d_count = reinterpret_cast<int*>(A.d_parts + kMaxPartials);
    launch_edge_gate(c->stream, c->el, c->ov.active ? &c->ov.dev.el : nullptr, items, edge_ids ? A.d_ids : nullptr, c->d_poses, chi2_max,
                     A.d_flag, A.d_parts, d_count);
    HIP_TRY(c, hipGetLastError());
    int count = 0;
    HIP_TRY(c, hipMemcpyAsync(&count, d_count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<uint8_t> flag((size_t)items, 0);
    if (count > 0) {
      HIP_TRY(c, hipMemcpyAsync(flag.data(), A.d_flag, (size_t)items, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    // then the host: the edges this call deactivates (an edge that is inactive already stays as it is; an id listed twice counts once)
    std::vector<int32_t> ids;
    for (int t = 0; t < items && count > 0; ++t) {
      if (!flag[t]) continue;
      const int e = edge_ids ? edge_ids[t] : t;
      if (A.dead[e]) flag[t] = 0;
      else ids.push_back(e);
    }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const std::vector<double> rows(6 * ids.size(), 0.0);
    if ((rc = edge_info_apply(c, "sgo_gate_edges", ids, rows))) return rc;
    if (gated) std::copy(flag.begin(), flag.end(), gated);
    return (int)ids.size();
  } SGO_CATCH(c)
}

int sgo_set_robust_kernels(sgo_ctx* c, int32_t n, const int32_t* edge_ids, const int32_t* kind, const double* delta) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!kind || !delta))) {
      c->err = "sgo_set_robust_kernels: null buffer or negative count";
      return SGO_EINVAL;
    }
    if (multi_gpu_context(c)) {
      c->err = "sgo_set_robust_kernels: not available in a multi-GPU context (only DCS through sgo_set_graph_se2's phi is)";
      return SGO_EINVAL;
    }
    for (int t = 0; t < n; ++t) {
      const int id = edge_ids ? edge_ids[t] : t;
      if (id < 0 || id >= c->E) {
        c->err = "sgo_set_robust_kernels: edge id " + std::to_string(id) + " outside [0, " + std::to_string(c->E) + ")";
        return SGO_EINVAL;
      }
      if (kind[t] < SGO_KERNEL_NONE || kind[t] > SGO_KERNEL_SATURATED) {
        c->err = "sgo_set_robust_kernels: unknown kind " + std::to_string(kind[t]) + " for edge " + std::to_string(id);
        return SGO_EINVAL;
      }
      const bool bad = !std::isfinite(delta[t]) || (kind[t] == SGO_KERNEL_DCS && delta[t] < 0.0) || (kind[t] >= SGO_KERNEL_HUBER && !(delta[t] > 0.0));
      if (bad) {
        c->err = "sgo_set_robust_kernels: delta " + std::to_string(delta[t]) + " of edge " + std::to_string(id) +
                 " is not finite or not in the kind's range (DCS: >= 0, the others: > 0)";
        return SGO_EINVAL;
      }
    }
    if (n == 0) return SGO_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // every id once: of an id listed twice the later entry counts
    std::vector<int32_t> order((size_t)n);
    for (int t = 0; t < n; ++t) order[t] = t;
    auto id_of = [&](int t) { return edge_ids ? edge_ids[t] : t; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return id_of(a) < id_of(b); });
    std::vector<int32_t> ids, kinds;
    std::vector<double> deltas;
    for (int k = 0; k < n; ++k) {
      const int t = order[k];
      if (k + 1 < n && id_of(order[k + 1]) == id_of(t)) continue;
      ids.push_back(id_of(t));
      kinds.push_back(kind[t]);
      deltas.push_back(delta[t]);
    }
    return robust_apply(c, "sgo_set_robust_kernels", ids, kinds, deltas);
  } SGO_CATCH(c)
}

int sgo_edge_robust(sgo_ctx* c, double* rho0, double* weight) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (c->E == 0 || (!rho0 && !weight)) return SGO_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    sgo_ctx::EdgeActivity& A = c->edges;
    const size_t E = (size_t)c->E;
    if ((rc = grow_scratch(c, &A.d_rows, &A.rows_cap, 2 * E))) return rc;
    launch_edge_robust(c->stream, c->el, c->ov.active ? &c->ov.dev.el : nullptr, c->d_poses, A.d_rows, A.d_rows + E);
    HIP_TRY(c, hipGetLastError());
    if (rho0) HIP_TRY(c, hipMemcpyAsync(rho0, A.d_rows, sizeof(double) * E, hipMemcpyDeviceToHost, c->stream));
    if (weight) HIP_TRY(c, hipMemcpyAsync(weight, A.d_rows + E, sizeof(double) * E, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SGO_OK;
  } SGO_CATCH(c)
}

int sgo_closure_information(sgo_ctx* c, int32_t n, const sgo_match_window* win, const float* scores, int64_t n_scores,
                            double* cov, double* info) {
  try {
    if (!c) return SGO_EINVAL;
    if (n < 0 || n_scores < 0 || (n > 0 && (!win || !scores || !cov || !info))) {
      c->err = "sgo_closure_information: null buffer or negative count";
      return SGO_EINVAL;
    }
    if (n == 0) return SGO_OK;
    // every window must lie inside scores[]: the kernel trusts these bounds
    for (int q = 0; q < n; ++q) {
      const sgo_match_window& W = win[q];
      if (W.w_size < 0 || W.w_size > 1024 || W.scan_window < 0 || W.scan_window > 1024 || W.score_offset < 0) {
        c->err = "sgo_closure_information: window " + std::to_string(q) + " has a negative or oversized extent";
        return SGO_EINVAL;
      }
      const int64_t nw = 2 * (int64_t)W.w_size + 1, total = nw * nw * (2 * (int64_t)W.scan_window + 1);
      if (total > INT32_MAX || W.score_offset + total > n_scores) {
        c->err = "sgo_closure_information: window " + std::to_string(q) + " reaches past scores[n_scores]";
        return SGO_EINVAL;
      }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    sgo_match_window* d_win = nullptr;
    float* d_sc = nullptr;
    double* d_out = nullptr;
    auto release = [&]() {
      if (d_win) hipFree(d_win);
      if (d_sc) hipFree(d_sc);
      if (d_out) hipFree(d_out);
    };
    if (hipMalloc(&d_win, sizeof(sgo_match_window) * (size_t)n) != hipSuccess ||
        hipMalloc(&d_sc, sizeof(float) * (size_t)std::max<int64_t>(n_scores, 1)) != hipSuccess ||
        hipMalloc(&d_out, sizeof(double) * 18 * (size_t)n) != hipSuccess) {
      release();
      c->err = "sgo_closure_information: out of device memory";
      return SGO_ENOMEM;
    }
    hipError_t e = hipMemcpyAsync(d_win, win, sizeof(sgo_match_window) * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(d_sc, scores, sizeof(float) * (size_t)n_scores, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
      launch_closure_cov(c->stream, n, d_win, d_sc, d_out, d_out + 9 * (size_t)n);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(cov, d_out, sizeof(double) * 9 * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(info, d_out + 9 * (size_t)n, sizeof(double) * 9 * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    release();
    if (e != hipSuccess) {
      c->err = std::string("sgo_closure_information: ") + hipGetErrorString(e);
      return SGO_EHIP;
    }
    return SGO_OK;
  } SGO_CATCH(c)
}

int sgo_linearize(sgo_ctx* c, double* b, double* diag, double* plain, double* robust) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (c->ov.active) {
      c->err = "single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";
      return SGO_EINVAL;
    }
    if (c->n == 0) return SGO_ENOTHING;
    if ((rc = ensure_amg(c))) return rc;
    if ((rc = do_chi2(c, c->d_hist, nullptr))) return rc;
    if ((rc = do_linearize(c))) return rc;
    if (c->owner && !halo_gather_slices(c->halo, c->stream, c->d_dgb, 9, &c->err)) return SGO_ECOMM;   // every rank reports all rows
    std::vector<double> dgb(9 * (size_t)c->n);
    HIP_TRY(c, hipMemcpyAsync(dgb.data(), c->d_dgb, sizeof(double) * dgb.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->h_hist, c->d_hist, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < c->n; ++i) {   // i: hessian index (g2o order); its values sit in internal row row_of_asc[i]
      const double* d = &dgb[9 * (size_t)c->row_of_asc[i]];
      if (diag) {
        double* D = diag + 9 * (size_t)i;
        D[0] = d[0]; D[1] = d[1]; D[2] = d[2];
        D[3] = d[1]; D[4] = d[3]; D[5] = d[4];
        D[6] = d[2]; D[7] = d[4]; D[8] = d[5];
      }
      if (b) {
        b[3 * (size_t)i] = d[6];
        b[3 * (size_t)i + 1] = d[7];
        b[3 * (size_t)i + 2] = d[8];
      }
    }
    if (plain) *plain = c->h_hist[0];
    if (robust) *robust = c->h_hist[1];
    return SGO_OK;
  } SGO_CATCH(c)
}

int sgo_hessian_apply(sgo_ctx* c, const double* x, double* y) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (c->ov.active) {
      c->err = "single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";
      return SGO_EINVAL;
    }
    if (!x || !y) return SGO_EINVAL;
    if (!c->linearized) {
      c->err = "sgo_hessian_apply: call sgo_linearize first";
      return SGO_EINVAL;
    }
    if ((rc = vec_to_device(c, x, c->d_s1))) return rc;
    if ((rc = do_spmv(c, c->d_s1, c->d_s2, false, nullptr, nullptr))) return rc;
    if (c->owner && !halo_gather_slices(c->halo, c->stream, c->d_s2, 3, &c->err)) return SGO_ECOMM;
    return vec_from_device(c, c->d_s2, y);
  } SGO_CATCH(c)
}

int sgo_precondition(sgo_ctx* c, const double* r, double* z) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (c->ov.active) {
      c->err = "single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";
      return SGO_EINVAL;
    }
    if (!r || !z) return SGO_EINVAL;
    if (!c->linearized) {
      c->err = "sgo_precondition: call sgo_linearize first";
      return SGO_EINVAL;
    }
    if ((rc = vec_to_device(c, r, c->d_s1))) return rc;
    if (c->amg) amg_apply(c->amg, c->stream, c->d_s1, c->d_s2, nullptr, nullptr, nullptr);
    else if (c->owner) launch_precond_bj(c->stream, c->halo.row1 - c->halo.row0, c->S0.dinv + 6 * (size_t)c->halo.row0, c->d_s1 + 3 * (size_t)c->halo.row0, c->d_s2 + 3 * (size_t)c->halo.row0, 1.0);
    else launch_precond_bj(c->stream, c->n, c->S0.dinv, c->d_s1, c->d_s2, 1.0);
    if (c->amg && amg_comm_failed(c->amg)) return SGO_ECOMM;
    if (c->owner && !halo_gather_slices(c->halo, c->stream, c->d_s2, 3, &c->err)) return SGO_ECOMM;
    return vec_from_device(c, c->d_s2, z);
  } SGO_CATCH(c)
}

int sgo_solve(sgo_ctx* c, double* x, double* relres) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (c->ov.active) {
      c->err = "single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";
      return SGO_EINVAL;
    }
    if (!c->linearized) {
      c->err = "sgo_solve: call sgo_linearize first";
      return SGO_EINVAL;
    }
    read_call_knobs(c);
    if ((rc = solve_from_linearization(c, true))) return rc;
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

// Test hooks for the PCG recurrence (include/sgo.h; tests/pcg_reference.py checks every stage of an iteration from these arrays).
static int pcg_hook_ready(sgo_ctx* c, const char* name) {
  int rc = check_graph(c);
  if (rc) return rc;
  if (c->ov.active) {
    c->err = "single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";
    return SGO_EINVAL;
  }
  if (c->owner || multi_rank(c)) {   // a rank holds its own rows; the multi-rank iterations keep other partial-sum rows
    c->err = std::string(name) + ": not available in a multi-GPU context";
    return SGO_EINVAL;
  }
  if (!c->linearized) {
    c->err = std::string(name) + ": call sgo_linearize first";
    return SGO_EINVAL;
  }
  return SGO_OK;
}

static_assert(sizeof(PcgScalars) == 104, "sgo_debug_pcg_array documents the layout of PcgScalars (include/sgo.h)");

int64_t sgo_debug_pcg_array(sgo_ctx* c, int32_t what, void* out, int64_t cap_bytes) {
  try {
    int rc = pcg_hook_ready(c, "sgo_debug_pcg_array");
    if (rc) return rc;
    if (cap_bytes < 0 || (cap_bytes > 0 && !out)) {
      c->err = "sgo_debug_pcg_array: negative capacity, or a capacity without a buffer";
      return SGO_EINVAL;
    }
    const size_t n = (size_t)c->n;
    const void* dev = nullptr;    // a device array ...
    const void* host = nullptr;   // ... or host memory
    size_t bytes = 0;
    int counts[8];
    double args[4];
    switch (what) {
      case SGO_PCG_B: dev = c->d_b; bytes = 24 * n; break;
      case SGO_PCG_X: dev = c->d_x; bytes = 24 * n; break;
      case SGO_PCG_R: dev = c->d_r; bytes = 24 * n; break;
      case SGO_PCG_Z: dev = c->d_z; bytes = 24 * n; break;
      case SGO_PCG_P: dev = c->d_p; bytes = 24 * n; break;
      case SGO_PCG_Q: dev = c->d_q; bytes = 24 * n; break;
      case SGO_PCG_DINV: dev = c->S0.dinv; bytes = 48 * n; break;
      case SGO_PCG_XS0: dev = c->amg ? amg_xs0(c->amg) : nullptr; bytes = dev ? 24 * n : 0; break;
      case SGO_PCG_SCALARS: dev = c->d_S; bytes = sizeof(PcgScalars); break;
      case SGO_PCG_HOST_SCALARS: host = c->h_S; bytes = sizeof(PcgScalars); break;
      case SGO_PCG_MIRROR: host = c->h_Sz; bytes = sizeof(PcgScalars); break;
      case SGO_PCG_PARTIALS: dev = c->d_partials; bytes = sizeof(double) * 3 * (size_t)kMaxPartials; break;
      case SGO_PCG_ZPARTS: dev = c->amg ? c->d_zparts : nullptr; bytes = dev ? sizeof(double) * 2 * (size_t)kMaxPartials : 0; break;
      case SGO_PCG_COUNTS: {
        const sgo_ctx::PcgCounts& k = c->pcg_counts;
        const int v[8] = {k.start_bb, k.start_rz, k.n_pq, k.n_rz, k.n_rr, k.n_zq, k.n_xq, k.n_bx};
        std::memcpy(counts, v, sizeof(v));
        host = counts;
        bytes = sizeof(counts);
        break;
      }
      case SGO_PCG_LANCZOS: {   // (sized from the device's own iteration count: the host copy is undefined before the first solve)
        dev = c->d_lanczos;
        PcgScalars S{};
        if (dev) {
          HIP_TRY(c, hipStreamSynchronize(c->stream));
          HIP_TRY(c, hipMemcpy(&S, c->d_S, sizeof(PcgScalars), hipMemcpyDeviceToHost));
        }
        bytes = dev ? sizeof(double) * 3 * (size_t)std::min(std::max(S.iter, 0), (int)kLanczosMax) : 0;
        break;
      }
      case SGO_PCG_START_ARGS:
        args[0] = c->pcg_start.tol; args[1] = c->pcg_start.tol_cap; args[2] = c->pcg_start.bb_ref; args[3] = c->pcg_start.maxit;
        host = args;
        bytes = sizeof(args);
        break;
      case SGO_PCG_ROW_ORDER: host = c->row_of_asc.data(); bytes = sizeof(int) * n; break;
      default: c->err = "sgo_debug_pcg_array: unknown array"; return SGO_EINVAL;
    }
    if (bytes == 0 || (int64_t)bytes > cap_bytes) return (int64_t)bytes;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the pinned copies are written by kernels: nothing may be in flight)
    if (dev) HIP_TRY(c, hipMemcpy(out, dev, bytes, hipMemcpyDeviceToHost));
    else std::memcpy(out, host, bytes);
    return (int64_t)bytes;
  } SGO_CATCH(c)
}

int sgo_debug_pcg_run(sgo_ctx* c, int32_t maxit, const double* x_prev, double bb_ref, int32_t probe_k, double probe_max) {
  try {
    int rc = pcg_hook_ready(c, "sgo_debug_pcg_run");
    if (rc) return rc;
    if (maxit < 0 || probe_k < 0 || !(probe_max >= 0.0) || !(bb_ref >= 0.0)) {
      c->err = "sgo_debug_pcg_run: maxit, probe_k, probe_max and bb_ref must be >= 0";
      return SGO_EINVAL;
    }
    if ((x_prev || probe_k > 0) && !c->amg) {   // (start_pcg: both belong to the solves behind a hierarchy)
      c->err = "sgo_debug_pcg_run: the warm start and the progress probe need a multigrid hierarchy";
      return SGO_EINVAL;
    }
    read_call_knobs(c);
    // the per-call fields optimize_gn would set, put back whatever happens
    struct Restore {
      sgo_ctx* c;
      sgo_ctx::CallState call;
      double tol_cap;
      int probe_k;
      double probe_max;
      ~Restore() {
        c->call = call;
        c->tol_cap = tol_cap;
        c->hier.probe_k = probe_k;
        c->hier.probe_max = probe_max;
      }
    } restore{c, c->call, c->tol_cap, c->hier.probe_k, c->hier.probe_max};
    c->call.pcg_softcap = maxit;
    c->tol_cap = c->opts.pcg_tol_cap > 0.0 ? std::max(c->opts.pcg_tol_cap, c->opts.pcg_tol * c->tol_scale) : 0.0;
    c->call.bb_ref = c->tol_cap > 0.0 ? bb_ref : 0.0;
    c->call.warm_valid = false;
    if (x_prev) {
      if ((rc = vec_to_device(c, x_prev, c->d_xprev))) return rc;
      c->call.warm_valid = true;
    }
    // the probe as a solve of the lagged refresh carries it (start_pcg): armed at hier.probe_k, held to hier.probe_max behind kept operators
    c->call.lag_on = probe_k > 0;
    c->call.skip_update = probe_k > 0 && probe_max > 0.0;
    c->hier.probe_k = probe_k;
    c->hier.probe_max = probe_max;
    if ((rc = solve_from_linearization(c, maxit > 0))) return rc;
    return c->h_S->iter;
  } SGO_CATCH(c)
}

int sgo_optimize_gn(sgo_ctx* c, int32_t iters, sgo_stats* out) {
  try {
    return optimize_gn(c, iters, out);
  } SGO_CATCH(c)
}

int sgo_gain_stop(double last_robust_chi2, double robust_chi2, double gain_tol) {
  return rules::gain_stop(last_robust_chi2, robust_chi2, gain_tol) ? 1 : 0;
}

int sgo_edge_loo_rule(const double* info6, const double* P9, const double* e3, double w, double* d2, double* redundancy, double* cov_loo) {
  return rules::edge_loo(info6, P9, e3, w, d2, redundancy, cov_loo);
}

int sgo_closure_search_rule(const double xj[3], const double xc[3], const double Sjj[9], const double Sjc[9], const double Scc[9], double radius,
                            double* rel, double* cov_rel, double* m2, double* sigma) {
  if (!xj || !xc || !m2 || (Sjj && Scc && !Sjc)) return SGO_EINVAL;
  return rules::closure_search(xj, xc, Sjj != nullptr, Scc != nullptr, Sjj, Sjc, Scc, radius, rel, cov_rel, m2, sigma);
}

int sgo_optimize_gn_until(sgo_ctx* c, int32_t max_iters, double gain_tol, sgo_stats* out, int32_t* stop_reason) {
  try {
    const int rc = check_graph(c);
    if (rc) return rc;
    if (!std::isfinite(gain_tol)) {
      c->err = "sgo_optimize_gn_until: gain_tol is not finite";
      return SGO_EINVAL;
    }
    if (multi_gpu_context(c)) {
      c->err = "sgo_optimize_gn_until: not available in a multi-GPU context (call sgo_optimize_gn)";
      return SGO_EINVAL;
    }
    UntilGain until{gain_tol, SGO_STOP_MAX_ITERS};
    const int done = optimize_gn(c, max_iters, out, &until);
    if (stop_reason && done >= 0) *stop_reason = until.stop_reason;
    return done;
  } SGO_CATCH(c)
}

int32_t sgo_hypothesis_isolated_vertex(int32_t V, const uint8_t* fixed, int32_t E, const int32_t* ei, const int32_t* ej, const double* info,
                                       const uint8_t* off) {
  try {
    if (V < 0 || E < 0 || (V > 0 && !fixed) || (E > 0 && (!ei || !ej || !info || !off))) {
      g_err = "sgo_hypothesis_isolated_vertex: null buffer or negative count";
      return SGO_EINVAL;
    }
    for (int e = 0; e < E; ++e)
      if (ei[e] < 0 || ei[e] >= V || ej[e] < 0 || ej[e] >= V) {
        g_err = "sgo_hypothesis_isolated_vertex: edge " + std::to_string(e) + " references a vertex outside [0, V)";
        return SGO_EINVAL;
      }
    auto dead = [&](int e) { return zero_row(info + 6 * (size_t)e); };
    std::vector<int> deg((size_t)V, 0);
    for (int e = 0; e < E; ++e)
      if (!dead(e)) {
        deg[ei[e]]++;
        deg[ej[e]]++;
      }
    return rules::hypothesis_isolated_vertex(fixed, E, ei, ej, dead, off, deg.data());
  } SGO_CATCH((sgo_ctx*)nullptr)
}

namespace {

// What the two routes of sgo_optimize_gn_hypotheses share of their outputs: hypothesis b's record and the history's NaN tail.
void hypothesis_record(int b, int max_iters, int done, int fail, const double* hist_b, sgo_hypothesis_result* res, double* hist) {
  res[b].iters_done = done;
  res[b].stop_reason = fail ? SGO_STOP_FAILED : (done < max_iters ? SGO_STOP_GAIN : SGO_STOP_MAX_ITERS);
  res[b].chi2 = hist_b[2 * done];
  res[b].robust_chi2 = hist_b[2 * done + 1];
  if (!hist) return;
  double* h = hist + 2 * ((size_t)max_iters + 1) * (size_t)b;
  for (int k = 0; k <= max_iters; ++k) {
    h[2 * k] = k <= done ? hist_b[2 * k] : std::nan("");
    h[2 * k + 1] = k <= done ? hist_b[2 * k + 1] : std::nan("");
  }
}

// The single-launch path: one launch of B workgroups (sgo_direct.h), every result read once behind it.
int hypotheses_batched(sgo_ctx* c, int B, int max_iters, double gain_tol, const uint8_t* edge_off, const double* poses0,
                       sgo_hypothesis_result* res, double* hist, double* poses_out, double* edge_chi2) {
  const size_t E = (size_t)c->E, V3 = 3 * (size_t)c->V, H = 2 * ((size_t)max_iters + 1);
  const DirectBatchLayout L = direct_batch_layout(c->direct, c->V, B, max_iters);
  int rc;
  if (L.bytes > c->hyp.ws_cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = grow_device(c, &c->hyp.d_ws, &c->hyp.ws_cap, L.bytes))) {
      c->err = "sgo_optimize_gn_hypotheses: out of device memory (" + std::to_string(L.bytes) + " bytes for " + std::to_string(B) + " hypotheses)";
      return rc;
    }
  }
  char* ws = c->hyp.d_ws;
  HIP_TRY(c, hipMemcpyAsync(ws + L.o_off, edge_off, (size_t)B * E, hipMemcpyHostToDevice, c->stream));
  if (poses0) HIP_TRY(c, hipMemcpyAsync(ws + L.o_poses, poses0, sizeof(double) * (size_t)B * V3, hipMemcpyHostToDevice, c->stream));
  {
    Scope sc(c, K_DIRECT, (double)B * direct_bytes(c->direct, c->E, max_iters), true);
    const hipError_t he = direct_optimize_batch(c->direct, c->stream, c->el, c->d_poses, poses0 != nullptr, L, ws, max_iters, gain_tol,
                                                edge_chi2 != nullptr);
    if (he != hipSuccess) {
      c->err = std::string("k_direct (batched) launch: ") + hipGetErrorString(he);
      return SGO_EHIP;
    }
  }
  std::vector<double> h_hist((size_t)B * H);
  std::vector<int> h_brief(2 * (size_t)B);
  HIP_TRY(c, hipMemcpyAsync(h_hist.data(), ws + L.o_hist, sizeof(double) * h_hist.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h_brief.data(), ws + L.o_brief, sizeof(int) * h_brief.size(), hipMemcpyDeviceToHost, c->stream));
  if (poses_out) HIP_TRY(c, hipMemcpyAsync(poses_out, ws + L.o_poses, sizeof(double) * (size_t)B * V3, hipMemcpyDeviceToHost, c->stream));
  if (edge_chi2) HIP_TRY(c, hipMemcpyAsync(edge_chi2, ws + L.o_echi2, sizeof(double) * (size_t)B * E, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_flush(c);
  for (int b = 0; b < B; ++b) {
    const int done = std::min(std::max(h_brief[2 * (size_t)b], 0), max_iters);
    hypothesis_record(b, max_iters, done, h_brief[2 * (size_t)b + 1], h_hist.data() + H * (size_t)b, res, hist);
  }
  return SGO_HYP_BATCHED;
}

// The multifrontal path with a granted workspace (sgo_set_hypotheses_workspace): chains of `chunk` hypotheses, each one pass through
// mfront_optimize's launches with every grid x chunk (sgo_mfront.h), every result of a chain read once behind it.
int hypotheses_mfront_batched(sgo_ctx* c, int chunk, int B, int max_iters, double gain_tol, const uint8_t* edge_off, const double* poses0,
                              sgo_hypothesis_result* res, double* hist, double* poses_out, double* edge_chi2) {
  const size_t E = (size_t)c->E, V3 = 3 * (size_t)c->V, H = 2 * ((size_t)max_iters + 1);
  const size_t need = mfront_batch_layout(c->mf, c->V, chunk, max_iters, edge_chi2 != nullptr).bytes;
  int rc;
  if (need > c->hyp.ws_cap) {   // need = chunk x per-hypothesis bytes <= the grant, and exactly that is allocated: no head-room
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = grow_device(c, &c->hyp.d_ws, &c->hyp.ws_cap, need, false))) {
      c->err = "sgo_optimize_gn_hypotheses: out of device memory (" + std::to_string(need) + " bytes for chains of " + std::to_string(chunk) + " hypotheses)";
      return rc;
    }
  }
  char* ws = c->hyp.d_ws;
  std::vector<double> h_hist((size_t)chunk * H);
  std::vector<int> h_brief(2 * (size_t)chunk);
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nb = std::min(chunk, B - b0);
    const MfBatchLayout L = mfront_batch_layout(c->mf, c->V, nb, max_iters, edge_chi2 != nullptr);
    HIP_TRY(c, hipMemcpyAsync(ws + L.o_off, edge_off + (size_t)b0 * E, (size_t)nb * E, hipMemcpyHostToDevice, c->stream));
    if (poses0) HIP_TRY(c, hipMemcpyAsync(ws + L.o_poses, poses0 + V3 * (size_t)b0, sizeof(double) * (size_t)nb * V3, hipMemcpyHostToDevice, c->stream));
    {
      Scope sc(c, K_MFRONT_BATCH, (double)nb * mfront_bytes(c->mf, c->E, max_iters), true);
      const hipError_t he = mfront_optimize_batch(c->mf, c->stream, c->el, c->d_poses, poses0 != nullptr, L, ws, max_iters, gain_tol, edge_chi2 != nullptr);
      if (he != hipSuccess) {
        c->err = std::string("multifrontal (batched) launch: ") + hipGetErrorString(he);
        return SGO_EHIP;
      }
    }
    HIP_TRY(c, hipMemcpyAsync(h_hist.data(), ws + L.o_hist, sizeof(double) * (size_t)nb * H, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_brief.data(), ws + L.o_brief, sizeof(int) * 2 * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    if (poses_out) HIP_TRY(c, hipMemcpyAsync(poses_out + V3 * (size_t)b0, ws + L.o_poses, sizeof(double) * (size_t)nb * V3, hipMemcpyDeviceToHost, c->stream));
    if (edge_chi2) HIP_TRY(c, hipMemcpyAsync(edge_chi2 + E * (size_t)b0, ws + L.o_echi2, sizeof(double) * (size_t)nb * E, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int b = 0; b < nb; ++b) {
      const int done = std::min(std::max(h_brief[2 * (size_t)b], 0), max_iters);
      hypothesis_record(b0 + b, max_iters, done, h_brief[2 * (size_t)b + 1], h_hist.data() + H * (size_t)b, res, hist);
    }
  }
  prof_flush(c);
  return SGO_HYP_BATCHED;
}

// Every other single-GPU path: the host loop itself -- zero rows, the start, optimise, read back, the rows again -- and the
// resident poses at the end.
int hypotheses_sequential(sgo_ctx* c, int B, int max_iters, double gain_tol, const uint8_t* edge_off, const double* poses0,
                          sgo_hypothesis_result* res, double* hist, double* poses_out, double* edge_chi2) {
  const size_t E = (size_t)c->E, V3 = 3 * (size_t)c->V, E0 = (size_t)c->el.E;
  sgo_ctx::EdgeActivity& A = c->edges;
  std::vector<double> resident(V3), info(6 * E0);
  HIP_TRY(c, hipMemcpyAsync(resident.data(), c->d_poses, sizeof(double) * V3, hipMemcpyDeviceToHost, c->stream));
  if (E0) HIP_TRY(c, hipMemcpyAsync(info.data(), c->el.info, sizeof(double) * 6 * E0, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const std::string lag_note = c->lag_note;
  std::unique_ptr<sgo_stats> st(new sgo_stats);
  std::vector<int32_t> ids;
  std::vector<double> zero, rows, e2(edge_chi2 ? E : 0);
  int rc = SGO_OK;
  for (int b = 0; b < B && rc == SGO_OK; ++b) {
    const uint8_t* off = edge_off + (size_t)b * E;
    ids.clear();
    rows.clear();
    for (size_t k = 0; k < E; ++k)
      if (off[k] && !A.dead[k]) {
        ids.push_back((int32_t)k);
        for (int q = 0; q < 6; ++q) rows.push_back(info[(size_t)q * E0 + k]);
      }
    zero.assign(rows.size(), 0.0);
    if ((rc = edge_info_apply(c, "sgo_optimize_gn_hypotheses", ids, zero))) break;
    UntilGain until{gain_tol, SGO_STOP_MAX_ITERS};
    int done = 0;
    rc = upload_poses(c, poses0 ? poses0 + V3 * (size_t)b : resident.data(), c->V);
    if (rc == SGO_OK) {
      c->linearized = false;
      done = optimize_gn(c, max_iters, st.get(), &until);
      if (done < 0 && done != SGO_ENOTHING) rc = done;
    }
    if (rc == SGO_OK) {
      std::vector<double> hb(2 * ((size_t)max_iters + 1), 0.0);
      const int applied = std::min(std::max(st->iters_done, 0), max_iters);
      for (int k = 0; k <= applied; ++k) {
        hb[2 * k] = st->chi2[k];
        hb[2 * k + 1] = st->robust_chi2[k];
      }
      hypothesis_record(b, max_iters, applied, until.stop_reason == SGO_STOP_FAILED, hb.data(), res, hist);
      res[b].stop_reason = until.stop_reason;
      if (poses_out) {
        HIP_TRY(c, hipMemcpyAsync(poses_out + V3 * (size_t)b, c->d_poses, sizeof(double) * V3, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
      }
    }
    // the rows come back whatever happened, and the per-edge values are formed behind them: with the resident information
    const int rb = edge_info_apply(c, "sgo_optimize_gn_hypotheses", ids, rows);
    if (rc == SGO_OK) rc = rb;
    if (rc == SGO_OK && edge_chi2) {
      if ((rc = do_chi2(c, c->d_hist, c->d_e2))) break;
      HIP_TRY(c, hipMemcpyAsync(edge_chi2 + E * (size_t)b, c->d_e2, sizeof(double) * E, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
  }
  const int rp = upload_poses(c, resident.data(), c->V);
  if (rp == SGO_OK) HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->linearized = false;
  c->lag_note = lag_note;
  if (rc == SGO_OK) rc = rp;
  return rc ? rc : SGO_HYP_SEQUENTIAL;
}

}  // namespace

int sgo_optimize_gn_hypotheses(sgo_ctx* c, int32_t B, int32_t max_iters, double gain_tol, const uint8_t* edge_off, const double* poses0,
                               sgo_hypothesis_result* res, double* hist, double* poses_out, double* edge_chi2) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    auto refuse = [&](const std::string& why) {
      c->err = "sgo_optimize_gn_hypotheses: " + why;
      return SGO_EINVAL;
    };
    if (B < 0) return refuse("negative number of hypotheses");
    if (max_iters < 0 || max_iters > SGO_MAX_ITERS) return refuse("max_iters must be in [0, SGO_MAX_ITERS]");
    if (!std::isfinite(gain_tol)) return refuse("gain_tol is not finite");
    if (B > 0 && (!edge_off || !res)) return refuse("null edge_off or res");
    if (multi_gpu_context(c)) return refuse("not available in a multi-GPU context");
    if (c->ov.active) return refuse("not available while an incremental overlay is active (call sgo_set_graph_se2)");
    if (B == 0) return SGO_HYP_BATCHED;
    if (c->n == 0) return refuse("the graph has no free pose");
    const size_t E = (size_t)c->E, V3 = 3 * (size_t)c->V;
    if (poses0)
      for (size_t k = 0; k < (size_t)B * V3; ++k)
        if (!std::isfinite(poses0[k]))
          return refuse("non-finite starting pose of hypothesis " + std::to_string(k / V3) + " (vertex " + std::to_string((k % V3) / 3) + ")");
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = edge_activity_ensure(c))) return rc;
    sgo_ctx::EdgeActivity& A = c->edges;
    for (int b = 0; b < B; ++b) {
      const int v = rules::hypothesis_isolated_vertex(c->ov.fixed.data(), c->E, A.vi.data(), A.vj.data(), [&](int e) { return A.dead[e] != 0; },
                                                      edge_off + (size_t)b * E, A.live_deg.data());
      if (v >= 0)
        return refuse("hypothesis " + std::to_string(b) + " leaves free vertex " + std::to_string(v) +
                      " without an incident edge of non-zero information (its Hessian block would be singular)");
    }
    read_call_knobs(c);
    if (c->direct) return hypotheses_batched(c, B, max_iters, gain_tol, edge_off, poses0, res, hist, poses_out, edge_chi2);
    if (c->mf && c->hyp.mf_budget > 0) {
      const long long per = (long long)mfront_batch_layout(c->mf, c->V, 1, max_iters, edge_chi2 != nullptr).per_hypothesis;
      const int chunk = rules::hypotheses_chunk(per, c->hyp.mf_budget, B);
      if (chunk >= 2) return hypotheses_mfront_batched(c, chunk, B, max_iters, gain_tol, edge_off, poses0, res, hist, poses_out, edge_chi2);
    }
    return hypotheses_sequential(c, B, max_iters, gain_tol, edge_off, poses0, res, hist, poses_out, edge_chi2);
  } SGO_CATCH(c)
}

int sgo_set_hypotheses_workspace(sgo_ctx* c, int64_t max_bytes) {
  try {
    if (!c) return SGO_EINVAL;
    if (max_bytes < 0) {
      c->err = "sgo_set_hypotheses_workspace: negative number of bytes";
      return SGO_EINVAL;
    }
    c->hyp.mf_budget = max_bytes;
    return SGO_OK;
  } SGO_CATCH(c)
}

int64_t sgo_hypotheses_bytes(sgo_ctx* c, int32_t max_iters, int32_t want_edge_chi2) {
  try {
    const int rc = check_graph(c);
    if (rc) return rc;
    if (max_iters < 0 || max_iters > SGO_MAX_ITERS) {
      c->err = "sgo_hypotheses_bytes: max_iters must be in [0, SGO_MAX_ITERS]";
      return SGO_EINVAL;
    }
    if (!c->mf || c->direct || c->ov.active || multi_gpu_context(c)) return 0;
    return (int64_t)mfront_batch_layout(c->mf, c->V, 1, max_iters, want_edge_chi2 != 0).per_hypothesis;
  } SGO_CATCH(c)
}

int64_t sgo_hypotheses_workspace_bytes(sgo_ctx* c) { return c ? (int64_t)c->hyp.ws_cap : (int64_t)SGO_EINVAL; }

int32_t sgo_hypotheses_chunk(int64_t per_hypothesis_bytes, int64_t budget_bytes, int32_t B) {
  return rules::hypotheses_chunk(per_hypothesis_bytes, budget_bytes, B);
}

double sgo_debug_spmv0_us(sgo_ctx* c, int mode, int variant, int reps) { return debug_spmv0_us(c, mode, variant, reps); }

// Test hook for the multi-GPU scheme: the coarse right-hand side the first half of a multigrid cycle makes from r
// (hessian order, [n][3]): first sweep from zero, level-0 residual pass, restriction.  Under sgo_debug_set_shard it
// is this rank's partial; the partials of all ranks sum to the single-rank vector.  Returns its length (3 x coarse
// nodes), 0 without a multi-level hierarchy, < 0 on error.  Requires sgo_linearize.
int sgo_debug_coarse_rhs(sgo_ctx* c, const double* r, double* out, int cap) {
  int rc = check_graph(c);
  if (rc) return rc;
  if (!r || !out || !c->linearized || c->ov.active) return SGO_EINVAL;
  if (c->owner) {   // this rank holds its own rows' blocks and transfer entries only: the hook walks whole-graph arrays
    c->err = "sgo_debug_coarse_rhs: not available in multi-GPU row-owner mode";
    return SGO_EINVAL;
  }
  if (ensure_amg(c)) return 0;
  if (!c->amg) return 0;
  if ((rc = vec_to_device(c, r, c->d_s1))) return rc;
  const int n3 = amg_debug_coarse_rhs(c->amg, c->stream, c->d_s1, c->d_s2, 3 * c->n);
  if (n3 <= 0) return n3;
  if (cap < n3) return SGO_EINVAL;
  HIP_TRY(c, hipMemcpyAsync(out, c->d_s2, sizeof(double) * (size_t)n3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return n3;
}

// Test hook: one array of the resident multigrid hierarchy as the next cycle / refresh reads it (amg_debug_array, sgo_amg.hip).
int64_t sgo_debug_amg_array(sgo_ctx* c, int32_t level, int32_t what, void* out, int64_t cap_bytes) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (c->ov.active) {
      c->err = "single-step entry points need a full set-up: the resident graph carries an incremental overlay (call sgo_set_graph_se2)";
      return SGO_EINVAL;
    }
    if (!c->linearized) {
      c->err = "sgo_debug_amg_array: call sgo_linearize first";
      return SGO_EINVAL;
    }
    if (c->owner) {   // a rank holds its own rows' blocks and transfer entries only
      c->err = "sgo_debug_amg_array: not available in multi-GPU row-owner mode";
      return SGO_EINVAL;
    }
    if (cap_bytes < 0 || (cap_bytes > 0 && !out)) return SGO_EINVAL;
    if (!c->amg) return 0;
    if (what == SGO_AMG_ROW_ORDER) {
      if (level != 0) return 0;
      const int64_t bytes = (int64_t)sizeof(int) * c->n;
      if (cap_bytes >= bytes)
        for (int i = 0; i < c->n; ++i) static_cast<int*>(out)[i] = c->row_of_asc[i];
      return bytes;
    }
    const long long r = amg_debug_array(c->amg, c->stream, level, what, out, cap_bytes);
    if (r == SGO_EINVAL) c->err = "sgo_debug_amg_array: unknown array, or the level-0 passes are sharded";
    if (r == SGO_EHIP) c->err = "sgo_debug_amg_array: device copy failed";
    return r;
  } SGO_CATCH(c)
}

// Test hooks for the incremental overlay (include/sgo.h): the arrays of sgo_overlay.h as stored, the linearisation and the
// operator of a Gauss-Newton iteration under an overlay.
static int overlay_hook_ready(sgo_ctx* c, const char* name) {
  int rc = check_graph(c);
  if (rc) return rc;
  if (!c->ov.active) {
    c->err = std::string(name) + ": the resident graph carries no incremental overlay";
    return SGO_EINVAL;
  }
  if (c->owner || multi_rank(c) || c->comm.nranks > 1) {
    c->err = std::string(name) + ": not available in a multi-GPU context";
    return SGO_EINVAL;
  }
  if (c->rows_pending || c->amg_pending || c->n == 0) {
    c->err = std::string(name) + ": the resident structures are not built";
    return SGO_EINVAL;
  }
  return SGO_OK;
}

int64_t sgo_debug_overlay_array(sgo_ctx* c, int32_t what, void* out, int64_t cap_bytes) {
  try {
    int rc = overlay_hook_ready(c, "sgo_debug_overlay_array");
    if (rc) return rc;
    if (cap_bytes < 0 || (cap_bytes > 0 && !out)) return SGO_EINVAL;
    const long long r = overlay_debug_array(c->ov, c->stream, what, c->d_x, out, cap_bytes);
    if (r == SGO_EINVAL) c->err = "sgo_debug_overlay_array: unknown array";
    if (r == SGO_EHIP) c->err = "sgo_debug_overlay_array: device copy failed";
    return r;
  } SGO_CATCH(c)
}

int sgo_debug_overlay_linearize(sgo_ctx* c, double* b) {
  try {
    int rc = overlay_hook_ready(c, "sgo_debug_overlay_linearize");
    if (rc) return rc;
    if (!b) return SGO_EINVAL;
    if ((rc = do_linearize(c))) return rc;
    std::vector<double> dgb(9 * (size_t)c->n);
    HIP_TRY(c, hipMemcpyAsync(dgb.data(), c->d_dgb, sizeof(double) * dgb.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < c->n; ++i)
      for (int q = 0; q < 3; ++q) b[3 * (size_t)i + q] = dgb[9 * (size_t)c->row_of_asc[i] + 6 + q];
    return SGO_OK;
  } SGO_CATCH(c)
}

int sgo_debug_overlay_apply(sgo_ctx* c, const double* x, double* y, double* dot) {
  try {
    int rc = overlay_hook_ready(c, "sgo_debug_overlay_apply");
    if (rc) return rc;
    if (!x || !y || !dot) return SGO_EINVAL;
    if (!c->linearized) {
      c->err = "sgo_debug_overlay_apply: call sgo_debug_overlay_linearize first";
      return SGO_EINVAL;
    }
    if ((rc = vec_to_device(c, x, c->d_s1))) return rc;
    int grid = 0;
    if ((rc = do_spmv(c, c->d_s1, c->d_s2, true, nullptr, &grid))) return rc;
    if (grid < 0 || grid > (int)kMaxPartials) return SGO_EHIP;
    std::vector<double> parts((size_t)grid);
    if (grid > 0) HIP_TRY(c, hipMemcpyAsync(parts.data(), c->d_partials, sizeof(double) * (size_t)grid, hipMemcpyDeviceToHost, c->stream));
    if ((rc = vec_from_device(c, c->d_s2, y))) return rc;
    long double s = 0.0L;
    for (double p : parts) s += p;
    *dot = (double)s;
    return SGO_OK;
  } SGO_CATCH(c)
}

// Test hook for the multifrontal path (include/sgo.h): the resident factorisation's arrays as stored (mfront_debug_array).
int64_t sgo_debug_mfront_array(sgo_ctx* c, int32_t what, void* out, int64_t cap_bytes) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    Mfront* mf = c->mf ? c->mf : c->selinv.mf;   // (a graph on another path: the plan the factor's calls made for themselves, if any)
    if (!mf) {
      c->err = "sgo_debug_mfront_array: the resident graph is not on the multifrontal path (" + c->solver_desc.substr(0, c->solver_desc.find(':')) + ")";
      return SGO_EINVAL;
    }
    if (cap_bytes < 0 || (cap_bytes > 0 && !out)) return SGO_EINVAL;
    const long long r = mfront_debug_array(mf, c->stream, what, out, cap_bytes);
    if (r == SGO_ENOTHING) {
      c->err = "sgo_debug_mfront_array: no sgo_optimize_gn has run on the resident graph";
      return SGO_EINVAL;
    }
    if (r == SGO_EINVAL) c->err = "sgo_debug_mfront_array: unknown array";
    if (r == SGO_EHIP) c->err = "sgo_debug_mfront_array: device copy failed";
    return r;
  } SGO_CATCH(c)
}

// Test hook for the single-launch direct path (include/sgo.h): the plan tables and k_direct's arrays as stored (direct_debug_array).
int64_t sgo_debug_direct_array(sgo_ctx* c, int32_t what, void* out, int64_t cap_bytes) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (!c->direct) {
      c->err = "sgo_debug_direct_array: the resident graph is not on the direct path (" + c->solver_desc.substr(0, c->solver_desc.find(':')) + ")";
      return SGO_EINVAL;
    }
    if (cap_bytes < 0 || (cap_bytes > 0 && !out)) return SGO_EINVAL;
    const long long r = direct_debug_array(c->direct, c->stream, what, out, cap_bytes);
    if (r == SGO_ENOTHING) {
      c->err = "sgo_debug_direct_array: no sgo_optimize_gn has run on the resident graph";
      return SGO_EINVAL;
    }
    if (r == SGO_EINVAL) c->err = "sgo_debug_direct_array: unknown array";
    if (r == SGO_EHIP) c->err = "sgo_debug_direct_array: device copy failed";
    return r;
  } SGO_CATCH(c)
}

// Diagnostic (env SGO_LANCZOS=1 at sgo_set_graph_se2): alpha / beta of every PCG iteration of the last solve, pairs in
// iteration order; returns the number of iterations written (the Lanczos matrix of the preconditioned operator follows
// from them: scripts/ritz_probe.py), < 0 on error.
int sgo_debug_lanczos(sgo_ctx* c, double* out, int cap) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    if (!c->d_lanczos || !out || !c->h_S) return SGO_EINVAL;
    const int n = std::min(std::min(c->h_S->iter, (int)kLanczosMax), cap);
    if (n > 0) {
      std::vector<double> t(3 * (size_t)n);
      HIP_TRY(c, hipMemcpyAsync(t.data(), c->d_lanczos, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      for (int j = 0; j < n; ++j) {
        out[2 * j] = t[3 * (size_t)j];
        out[2 * j + 1] = t[3 * (size_t)j + 1];
      }
    }
    return n;
  } SGO_CATCH(c)
}

int sgo_kernel_profile(sgo_ctx* c, sgo_kernel_stat* out, int cap) {
  try {
    if (!c || (cap > 0 && !out)) return SGO_EINVAL;
    prof_flush(c);
    for (int k = 0; k < K_COUNT && k < cap; ++k) {
      out[k].name = kKernelNames[k];
      out[k].launches = c->prof_launches[k];
      out[k].ms = c->prof_ms[k];
      out[k].bytes = c->prof_bytes[k];
    }
    return K_COUNT;
  } SGO_CATCH(c)
}

int sgo_kernel_profile_samples(sgo_ctx* c, int slot, float* out_ms, int cap) {
  try {
    if (!c || slot < 0 || slot >= K_COUNT || cap < 0 || (cap > 0 && !out_ms)) return SGO_EINVAL;
    prof_flush(c);
    const std::vector<float>& v = c->prof_samples[slot];
    const int n = (int)std::min<size_t>(v.size(), (size_t)cap);
    std::copy(v.begin(), v.begin() + n, out_ms);
    return n;
  } SGO_CATCH(c)
}

double sgo_profile_overhead_ms(sgo_ctx* c) {
  if (!c) return -1.0;
  if (c->prof_null_ms < 0.0) prof_calibrate(c);
  return c->prof_null_ms;
}

int sgo_profile_reset(sgo_ctx* c) {
  try {
    if (!c) return SGO_EINVAL;
    prof_flush(c);
    for (int k = 0; k < K_COUNT; ++k) {
      c->prof_ms[k] = 0;
      c->prof_launches[k] = 0;
      c->prof_bytes[k] = 0;
      c->prof_samples[k].clear();
    }
    return SGO_OK;
  } SGO_CATCH(c)
}

int sgo_comm_unique_id(void* id_out) {
  if (!id_out) return SGO_EINVAL;
  return comm_unique_id(id_out, &g_err) ? SGO_OK : SGO_ECOMM;
}

int sgo_comm_init(sgo_ctx* c, int nranks, int rank, const void* unique_id) {
  try {
    if (!c || nranks < 1 || rank < 0 || rank >= nranks || !unique_id) return SGO_EINVAL;
    hipSetDevice(c->device);
    if (c->has_graph) {
      c->err = "sgo_comm_init must precede sgo_set_graph_se2";
      return SGO_EINVAL;
    }
    return c->comm.init(nranks, rank, unique_id, &c->err) ? SGO_OK : SGO_ECOMM;
  } SGO_CATCH(c)
}

int sgo_comm_init_host(sgo_ctx* c, int nranks, int rank, sgo_host_allreduce_fn fn, void* user) {
  try {
    if (!c || nranks < 1 || rank < 0 || rank >= nranks || !fn) return SGO_EINVAL;
    hipSetDevice(c->device);
    if (c->has_graph) {
      c->err = "sgo_comm_init_host must precede sgo_set_graph_se2";
      return SGO_EINVAL;
    }
    return c->comm.init_host(nranks, rank, fn, user) ? SGO_OK : SGO_ECOMM;
  } SGO_CATCH(c)
}

int sgo_comm_host_allgather(sgo_ctx* c, sgo_host_allgather_fn fn) {
  if (!c || !c->comm.host_fn) return SGO_EINVAL;
  if (c->has_graph) {
    c->err = "sgo_comm_host_allgather must precede sgo_set_graph_se2";
    return SGO_EINVAL;
  }
  c->comm.host_gather_fn = fn;
  return SGO_OK;
}

int64_t sgo_debug_level0_bytes(sgo_ctx* c) {
  if (check_graph(c) != SGO_OK) return -1;
  return (int64_t)c->level0_bytes + (c->amg ? (int64_t)amg_level0_bytes(c->amg) : 0);
}

int sgo_comm_size(sgo_ctx* c) { return c ? c->comm.nranks : SGO_EINVAL; }

int sgo_debug_set_shard(sgo_ctx* c, int nranks, int rank) {
  if (!c || nranks < 1 || rank < 0 || rank >= nranks) return SGO_EINVAL;
  if (c->has_graph) {
    c->err = "sgo_debug_set_shard must precede sgo_set_graph_se2";
    return SGO_EINVAL;
  }
  c->comm.destroy();
  c->comm.nranks = nranks;  // no handle: Comm::allreduce_* are no-ops
  c->comm.rank = rank;
  return SGO_OK;
}


}  // extern "C"
