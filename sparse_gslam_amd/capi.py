"""ctypes binding of libsgo.so (include/sgo.h) -- the only way Python reaches the optimiser.

There is no CPU fallback: if the HIP library is missing or no GPU is present, calls fail
loudly (``SgoError``).  The oracle under ``oracle/`` is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libsgo.so")

SGO_MAX_ITERS = 256
SOLVER_PCG_BJ = 0
SOLVER_PCG_AMG = 1
UNIQUE_ID_BYTES = 128

# every symbol include/sgo.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "sgo_version", "sgo_default_opts", "sgo_create", "sgo_destroy", "sgo_set_graph_se2",
    "sgo_set_poses", "sgo_get_poses", "sgo_optimize_gn", "sgo_chi2", "sgo_edge_chi2",
    "sgo_num_free", "sgo_free_ids", "sgo_linearize", "sgo_hessian_apply", "sgo_solve",
    "sgo_precondition", "sgo_kernel_profile", "sgo_profile_reset", "sgo_profile_overhead_ms", "sgo_comm_unique_id",
    "sgo_comm_init", "sgo_comm_size", "sgo_shard_range", "sgo_debug_set_shard", "sgo_last_error",
    "sgo_closure_information", "sgo_plan_rows", "sgo_mfront_plan", "sgo_debug_coarse_rhs", "sgo_debug_spmv0_us",
    "sgo_solver_description", "sgo_comm_init_host", "sgo_comm_host_allgather", "sgo_debug_level0_bytes",
    "sgo_kernel_profile_samples", "sgo_update_graph_se2", "sgo_debug_lanczos", "sgo_debug_amg_array",
    "sgo_debug_overlay_array", "sgo_debug_overlay_linearize", "sgo_debug_overlay_apply",
    "sgo_debug_mfront_array", "sgo_mfront_plan_array", "sgo_debug_pcg_array", "sgo_debug_pcg_run",
    "sgo_direct_plan_array", "sgo_debug_direct_array",
    "sgo_set_edge_information", "sgo_gate_edges", "sgo_set_robust_kernels", "sgo_edge_robust",
    "sgo_solve_rhs", "sgo_marginals", "sgo_marginals_selected", "sgo_factor_solve", "sgo_candidate_gate",
    "sgo_gain_stop", "sgo_optimize_gn_until", "sgo_optimize_gn_hypotheses", "sgo_hypothesis_isolated_vertex",
    "sgo_candidate_joint", "sgo_joint_subsets", "sgo_joint_pairs", "sgo_edge_leave_one_out", "sgo_edge_loo_rule",
    "sgo_joint_greedy", "sgo_joint_extend", "sgo_joint_greedy_rule",
    "sgo_edge_joint", "sgo_edge_groups", "sgo_edge_group_rule", "sgo_closure_search", "sgo_closure_search_rule",
    "sgo_set_hypotheses_workspace", "sgo_hypotheses_bytes", "sgo_hypotheses_chunk", "sgo_hypotheses_workspace_bytes",
    "sgo_optimize_lm", "sgo_lm_trial_rule", "sgo_optimize_lm_pcg", "sgo_lm_pcg_trace",
    "sgo_optimize_dogleg", "sgo_optimize_dogleg_pcg", "sgo_dogleg_step_rule", "sgo_dogleg_trial_rule",
    "sgo_optimize_gn_many", "sgo_many_workspace_bytes",
]

# SGO_JOINT_MAX_*: the limits of sgo_candidate_joint's table and of a subset of it
JOINT_MAX_CANDIDATES, JOINT_MAX_SUBSET = 256, 40

# SGO_STOP_*: why sgo_optimize_gn_until ended
STOP_MAX_ITERS, STOP_GAIN, STOP_FAILED = 0, 1, 2

# SGO_LM_STOP_*: why sgo_optimize_lm ended
LM_STOP_MAX_ITERS, LM_STOP_TRIALS, LM_STOP_ZERO_GAIN, LM_STOP_LAMBDA = 0, 1, 2, 3
# what sgo_lm_trial_rule returns
LM_RETRY, LM_ACCEPT, LM_ZERO_GAIN, LM_END = 0, 1, 2, 3
# SGO_LM_SOLVE_*: how a trial's solve of sgo_optimize_lm_pcg ended (sgo_lm_pcg_trace; a failed solve: minus the PCG stop code)
LM_SOLVE_CONVERGED, LM_SOLVE_FLOOR = 1, 2

# SGO_DL_STOP_*: why sgo_optimize_dogleg ended; SGO_DL_STEP_*: the kind of a trial's step
DL_STOP_MAX_ITERS, DL_STOP_TRIALS, DL_STOP_DAMPING = 0, 1, 2
DL_STEP_GN, DL_STEP_SD, DL_STEP_DL = 0, 1, 2

# SGO_HYP_*: the route sgo_optimize_gn_hypotheses took
HYP_BATCHED, HYP_SEQUENTIAL = 1, 2

# SGO_KERNEL_*: the robust kernels sgo_set_robust_kernels takes, in include/sgo.h's numbering
KERNEL_NONE, KERNEL_DCS, KERNEL_HUBER, KERNEL_PSEUDO_HUBER, KERNEL_CAUCHY = 0, 1, 2, 3, 4
KERNEL_GEMAN_MCCLURE, KERNEL_WELSCH, KERNEL_FAIR, KERNEL_TUKEY, KERNEL_SATURATED = 5, 6, 7, 8, 9


class SgoError(RuntimeError):
    pass


def gain_stop(last_robust_chi2: float, robust_chi2: float, gain_tol: float) -> bool:
    """sgo_gain_stop: the rule sgo_optimize_gn_until stops by, as the library computes it (no context, no GPU)."""
    return bool(lib().sgo_gain_stop(last_robust_chi2, robust_chi2, gain_tol))


def lm_trial_rule(cur: float, trial: float, scale: float, solve_ok: bool, lam: float, nu: float):
    """sgo_lm_trial_rule: one trial of sgo_optimize_lm as the library (and its kernel) computes it, no context and no GPU: the robust
    chi2 at the accepted and at the trial poses, scale = x . (lambda x + b) + 1e-3 -> (one of LM_*, lambda, nu after the trial)."""
    a, b = C.c_double(lam), C.c_double(nu)
    code = lib().sgo_lm_trial_rule(cur, trial, scale, int(bool(solve_ok)), C.byref(a), C.byref(b))
    return code, a.value, b.value


def dogleg_step_rule(delta: float, forms):
    """sgo_dogleg_step_rule: the step of one dogleg trial as the library (and its kernel) computes it, no context and no GPU:
    forms = (b.b, b.g, g.g, b.Hb, b.Hg, g.Hg) of the right-hand side b and the Gauss-Newton step g -> (kind: one of DL_STEP_*,
    a, c of the step a b + c g, its norm, the linear gain)."""
    f = (C.c_double * 6)(*[float(x) for x in forms])
    a, c, n, g = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    kind = lib().sgo_dogleg_step_rule(delta, f, C.byref(a), C.byref(c), C.byref(n), C.byref(g))
    return kind, a.value, c.value, n.value, g.value


def dogleg_trial_rule(cur: float, trial: float, linear_gain: float, step_norm: float, delta: float):
    """sgo_dogleg_trial_rule: the decision of one dogleg trial as the library (and its kernel) computes it -> (accepted, delta
    after the trial)."""
    d = C.c_double(delta)
    acc = lib().sgo_dogleg_trial_rule(cur, trial, linear_gain, step_norm, C.byref(d))
    return bool(acc), d.value


def edge_loo_rule(info6, P, e, w: float):
    """sgo_edge_loo_rule: the per-edge arithmetic of sgo_edge_leave_one_out as the library (and its kernel) computes it, no context
    and no GPU: info6 = Omega's upper triangle by rows, P (3, 3), e (3,), the kernel weight w -> (rc, d2, redundancy, cov_loo (3, 3));
    rc 0, 1 for an all-zero information, 2 for one that is not positive definite.  No min_redundancy is applied."""
    o = np.ascontiguousarray(info6, dtype=np.float64).reshape(6)
    Pm = np.ascontiguousarray(P, dtype=np.float64).reshape(9)
    ev = np.ascontiguousarray(e, dtype=np.float64).reshape(3)
    d2, red, cov = C.c_double(), C.c_double(), np.empty((3, 3))
    rc = lib().sgo_edge_loo_rule(_dp(o), _dp(Pm), _dp(ev), float(w), C.byref(d2), C.byref(red), _dp(cov))
    return rc, d2.value, red.value, cov


def edge_group_rule(info6, N, e, w):
    """sgo_edge_group_rule: one group's arithmetic of sgo_edge_groups as the library (and its kernel) computes it, no context and no
    GPU: info6 (k, 6) = the members' Omega, upper triangle by rows, N (3 k, 3 k), e (k, 3), w (k,) -> (rc, d2, pivot, dof); rc 0, 1 when
    a member with all-zero information was dropped, 2 when an information is not positive definite, SGO_EINVAL (-2) for k above
    SGO_JOINT_MAX_SUBSET.  No min_pivot is applied."""
    o = np.ascontiguousarray(info6, dtype=np.float64).reshape(-1, 6)
    k = o.shape[0]
    Nm = np.ascontiguousarray(N, dtype=np.float64).reshape(3 * k, 3 * k)
    ev = np.ascontiguousarray(e, dtype=np.float64).reshape(3 * k)
    wv = np.ascontiguousarray(w, dtype=np.float64).reshape(k)
    d2, piv, dof = C.c_double(), C.c_double(), C.c_int32(-1)
    rc = lib().sgo_edge_group_rule(k, _dp(o), _dp(Nm), _dp(ev), _dp(wv), C.byref(d2), C.byref(piv), C.byref(dof))
    return rc, d2.value, piv.value, dof.value


def closure_search_rule(xj, xc, Sjj, Sjc, Scc, radius: float):
    """sgo_closure_search_rule: one pair's arithmetic of sgo_closure_search as the library (and its kernel) computes it, no context
    and no GPU: the poses xj, xc (3,) and the blocks Sjj, Sjc (the rows of j), Scc (3, 3) of Sigma -> (rel (3,), cov_rel (3, 3), m2,
    sigma (2,)).  Sjj or Scc None: that pose is fixed and drops out with the cross block."""
    def blk(S):
        return None if S is None else np.ascontiguousarray(S, dtype=np.float64).reshape(9)
    a, b = np.ascontiguousarray(xj, dtype=np.float64).reshape(3), np.ascontiguousarray(xc, dtype=np.float64).reshape(3)
    jj, jc, cc = blk(Sjj), blk(Sjc), blk(Scc)
    rel, P, m2, sg = np.empty(3), np.empty((3, 3)), C.c_double(), np.empty(2)
    rc = lib().sgo_closure_search_rule(_dp(a), _dp(b), None if jj is None else _dp(jj), None if jc is None else _dp(jc),
                                       None if cc is None else _dp(cc), float(radius), _dp(rel), _dp(P), C.byref(m2), _dp(sg))
    if rc < 0:
        raise SgoError(f"sgo_closure_search_rule: rc={rc}")
    return rel, P, m2.value, sg


# SGO_JSTOP_*: why a search of sgo_joint_greedy ended
JSTOP_MAX_LEN, JSTOP_NONE, JSTOP_NOT_PD = 0, 1, 2


def joint_lists(lists):
    """index lists (or a (B, 40) array, -1 padded) -> the [B][SGO_JOINT_MAX_SUBSET] int32 rows sgo_joint_greedy / sgo_joint_extend take"""
    if isinstance(lists, np.ndarray) and lists.ndim == 2 and lists.shape[1] == JOINT_MAX_SUBSET:
        return np.ascontiguousarray(lists, dtype=np.int32)
    out = np.full((len(lists), JOINT_MAX_SUBSET), -1, dtype=np.int32)
    for b, idx in enumerate(lists):
        idx = np.asarray(idx, dtype=np.int32).reshape(-1)
        if idx.size > JOINT_MAX_SUBSET:
            raise ValueError(f"list {b} has {idx.size} entries, more than SGO_JOINT_MAX_SUBSET = {JOINT_MAX_SUBSET}")
        out[b, :idx.size] = idx
    return out


def _chi2_ladder(chi2_max):
    if chi2_max is None:
        return None
    chi = np.ascontiguousarray(chi2_max, dtype=np.float64).reshape(-1)
    if chi.size != JOINT_MAX_SUBSET + 1:
        raise ValueError(f"chi2_max needs {JOINT_MAX_SUBSET + 1} entries by count ([0] is ignored)")
    return chi


def joint_greedy_rule(S, e, seed, chi2_max, max_len: int = JOINT_MAX_SUBSET, allow=None):
    """sgo_joint_greedy_rule: one seed's greedy search as the library (and its kernel) computes it, no context and no GPU: S (3 n, 3 n),
    e (n, 3), seed an index list, chi2_max (41,) by count or None -> (rc, order (40,), count, stop, d2_path (41,), d2_ext (n,));
    rc 1, or SGO_EINVAL (-2) for what sgo_joint_greedy refuses in its lists and thresholds."""
    Sm = np.ascontiguousarray(S, dtype=np.float64)
    ev = np.ascontiguousarray(e, dtype=np.float64).reshape(-1)
    n = ev.size // 3
    if Sm.shape != (3 * n, 3 * n):
        raise ValueError("inconsistent array sizes")
    sd, chi = joint_lists([seed]), _chi2_ladder(chi2_max)
    al = None if allow is None else np.ascontiguousarray(np.asarray(allow) != 0, dtype=np.uint8).reshape(n)
    order, cnt, stop = np.full(JOINT_MAX_SUBSET, -2, dtype=np.int32), C.c_int32(-1), C.c_int32(-1)
    path, ext = np.empty(JOINT_MAX_SUBSET + 1), np.empty(n)
    u8p = C.POINTER(C.c_uint8)
    rc = lib().sgo_joint_greedy_rule(n, _dp(Sm), _dp(ev), _ip(sd), None if al is None else al.ctypes.data_as(u8p), None if chi is None else _dp(chi),
                                     int(max_len), _ip(order), C.byref(cnt), C.byref(stop),
                                     _dp(path), _dp(ext))
    return rc, order, cnt.value, stop.value, path, ext


class Opts(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("solver", C.c_int32), ("pcg_tol", C.c_double),
                ("pcg_maxit", C.c_int32), ("pcg_chunk", C.c_int32), ("use_graph", C.c_int32),
                ("profile", C.c_int32), ("verbose", C.c_int32), ("direct_rows", C.c_int32),
                ("pcg_tol_cap", C.c_double), ("pcg_warm_start", C.c_int32), ("reserved", C.c_int32 * 4)]


class Stats(C.Structure):
    _fields_ = [("iters_requested", C.c_int32), ("iters_done", C.c_int32),
                ("chi2", C.c_double * (SGO_MAX_ITERS + 1)),
                ("robust_chi2", C.c_double * (SGO_MAX_ITERS + 1)),
                ("pcg_iters", C.c_int32 * SGO_MAX_ITERS),
                ("pcg_converged", C.c_int32 * SGO_MAX_ITERS),
                ("pcg_relres", C.c_double * SGO_MAX_ITERS),
                ("seconds", C.c_double * SGO_MAX_ITERS),
                ("seconds_linearize", C.c_double * SGO_MAX_ITERS),
                ("seconds_solve", C.c_double * SGO_MAX_ITERS),
                ("seconds_total", C.c_double), ("seconds_setup", C.c_double)]


class LmStats(C.Structure):
    """sgo_lm_stats (include/sgo.h)."""
    _fields_ = [("iters_requested", C.c_int32), ("iters_done", C.c_int32), ("trials_total", C.c_int32), ("stop_reason", C.c_int32),
                ("sync_rounds", C.c_int32), ("lambda0", C.c_double),
                ("lam", C.c_double * SGO_MAX_ITERS),
                ("robust_chi2", C.c_double * (SGO_MAX_ITERS + 1)),
                ("chi2", C.c_double * (SGO_MAX_ITERS + 1)),
                ("trials", C.c_int32 * SGO_MAX_ITERS),
                ("seconds_total", C.c_double)]


class DoglegStats(C.Structure):
    """sgo_dogleg_stats (include/sgo.h)."""
    _fields_ = [("iters_requested", C.c_int32), ("iters_done", C.c_int32), ("trials_total", C.c_int32), ("solves", C.c_int32),
                ("stop_reason", C.c_int32), ("sync_rounds", C.c_int32), ("delta0", C.c_double),
                ("delta", C.c_double * SGO_MAX_ITERS),
                ("robust_chi2", C.c_double * (SGO_MAX_ITERS + 1)),
                ("chi2", C.c_double * (SGO_MAX_ITERS + 1)),
                ("trials", C.c_int32 * SGO_MAX_ITERS),
                ("step_kind", C.c_int32 * SGO_MAX_ITERS),
                ("lam", C.c_double),
                ("seconds_total", C.c_double)]


class HypothesisResult(C.Structure):
    """sgo_hypothesis_result (include/sgo.h)."""
    _fields_ = [("iters_done", C.c_int32), ("stop_reason", C.c_int32), ("chi2", C.c_double), ("robust_chi2", C.c_double)]


class ManyResult(C.Structure):
    """sgo_many_result: one context's part of sgo_optimize_gn_many."""
    _fields_ = [("rc", C.c_int32), ("stop_reason", C.c_int32), ("in_launch", C.c_int32)]


def hypothesis_isolated_vertex(fixed, ei, ej, info, off) -> int:
    """sgo_hypothesis_isolated_vertex: the lowest free vertex the mask `off` (E,) leaves without an incident edge of non-zero
    information, or -1 (no context, no GPU)."""
    f = np.ascontiguousarray(fixed, dtype=np.uint8)
    a = np.ascontiguousarray(ei, dtype=np.int32)
    b = np.ascontiguousarray(ej, dtype=np.int32)
    o = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 6)
    m = np.ascontiguousarray(off, dtype=np.uint8).reshape(-1)
    if not (a.size == b.size == o.shape[0] == m.size):
        raise ValueError("inconsistent array sizes")
    u8 = C.POINTER(C.c_uint8)
    rc = lib().sgo_hypothesis_isolated_vertex(f.size, f.ctypes.data_as(u8), a.size, _ip(a), _ip(b), _dp(o), m.ctypes.data_as(u8))
    if rc < -1:
        raise SgoError(f"sgo_hypothesis_isolated_vertex: rc={rc}: " + lib().sgo_last_error(None).decode())
    return rc


def hypotheses_chunk(per_hypothesis_bytes: int, budget_bytes: int, B: int) -> int:
    """sgo_hypotheses_chunk: hypotheses per launch chain of the batched multifrontal route, 0 = the sequential route (no context,
    no GPU)."""
    return int(lib().sgo_hypotheses_chunk(int(per_hypothesis_bytes), int(budget_bytes), int(B)))


class MatchWindow(C.Structure):
    """sgo_match_window (include/sgo.h): one scan-match score window."""
    _fields_ = [("x_index_offset", C.c_int32), ("y_index_offset", C.c_int32), ("scan_index", C.c_int32),
                ("scan_window", C.c_int32), ("w_size", C.c_int32), ("num_angular_perturbations", C.c_int32),
                ("resolution", C.c_double), ("angular_step", C.c_double), ("score_offset", C.c_int64)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char_p), ("launches", C.c_int64), ("ms", C.c_double),
                ("bytes", C.c_double)]


# sgo_host_allreduce_fn: int fn(double* buf, size_t count, void* user)
HOST_ALLREDUCE = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_size_t, C.c_void_p)
HOST_ALLGATHER = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_double), C.c_void_p)

_LIB = None


def build(force: bool = False) -> str:
    """Compile libsgo.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)
            if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(_HERE, "..", "include", "sgo.h")]
    stale = (not os.path.exists(LIB_PATH) or
             any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs))
    if force or stale:
        subprocess.check_call(["make", "-s", "-C", CSRC, "libsgo.so"])
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise SgoError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; "
                       "g.build()'` (there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    d = C.POINTER(C.c_double)
    i32 = C.POINTER(C.c_int32)
    u8 = C.POINTER(C.c_uint8)
    vp = C.c_void_p
    L.sgo_version.restype = C.c_int
    L.sgo_default_opts.argtypes = [C.POINTER(Opts)]
    L.sgo_create.restype = vp
    L.sgo_create.argtypes = [C.c_int, C.POINTER(Opts)]
    L.sgo_destroy.argtypes = [vp]
    L.sgo_set_graph_se2.argtypes = [vp, C.c_int32, d, u8, C.c_int32, i32, i32, d, d, d]
    L.sgo_update_graph_se2.argtypes = [vp, C.c_int32, d, u8, C.c_int32, i32, i32, d, d, d, C.c_int32]
    L.sgo_debug_lanczos.argtypes = [vp, d, C.c_int]
    L.sgo_set_poses.argtypes = [vp, d]
    L.sgo_get_poses.argtypes = [vp, d]
    L.sgo_optimize_gn.argtypes = [vp, C.c_int32, C.POINTER(Stats)]
    L.sgo_optimize_gn_until.argtypes = [vp, C.c_int32, C.c_double, C.POINTER(Stats), i32]
    L.sgo_gain_stop.argtypes = [C.c_double, C.c_double, C.c_double]
    L.sgo_optimize_lm.argtypes = [vp, C.c_int32, C.c_double, C.POINTER(LmStats)]
    L.sgo_optimize_lm_pcg.argtypes = [vp, C.c_int32, C.c_double, C.POINTER(LmStats)]
    L.sgo_lm_pcg_trace.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sgo_optimize_dogleg.argtypes = [vp, C.c_int32, C.c_double, C.POINTER(DoglegStats)]
    L.sgo_optimize_dogleg_pcg.argtypes = [vp, C.c_int32, C.c_double, C.POINTER(DoglegStats)]
    L.sgo_dogleg_step_rule.argtypes = [C.c_double, C.POINTER(C.c_double), d, d, d, d]
    L.sgo_dogleg_trial_rule.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, d]
    L.sgo_lm_trial_rule.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sgo_optimize_gn_hypotheses.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, u8, d, C.POINTER(HypothesisResult), d, d, d]
    L.sgo_optimize_gn_many.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, C.c_double, C.POINTER(C.POINTER(Stats)), C.POINTER(ManyResult), i32]
    L.sgo_many_workspace_bytes.restype = C.c_int64
    L.sgo_many_workspace_bytes.argtypes = [vp]
    L.sgo_hypothesis_isolated_vertex.restype = C.c_int32
    L.sgo_set_hypotheses_workspace.argtypes = [vp, C.c_int64]
    L.sgo_hypotheses_bytes.restype = C.c_int64
    L.sgo_hypotheses_bytes.argtypes = [vp, C.c_int32, C.c_int32]
    L.sgo_hypotheses_workspace_bytes.restype = C.c_int64
    L.sgo_hypotheses_workspace_bytes.argtypes = [vp]
    L.sgo_hypotheses_chunk.restype = C.c_int32
    L.sgo_hypotheses_chunk.argtypes = [C.c_int64, C.c_int64, C.c_int32]
    L.sgo_hypothesis_isolated_vertex.argtypes = [C.c_int32, u8, C.c_int32, i32, i32, d, u8]
    L.sgo_chi2.argtypes = [vp, d, d]
    L.sgo_edge_chi2.argtypes = [vp, d]
    L.sgo_set_edge_information.argtypes = [vp, C.c_int32, i32, d]
    L.sgo_gate_edges.argtypes = [vp, C.c_int32, i32, C.c_double, u8]
    L.sgo_set_robust_kernels.argtypes = [vp, C.c_int32, i32, i32, d]
    L.sgo_edge_robust.argtypes = [vp, d, d]
    L.sgo_num_free.argtypes = [vp]
    L.sgo_free_ids.argtypes = [vp, i32]
    L.sgo_linearize.argtypes = [vp, d, d, d, d]
    L.sgo_hessian_apply.argtypes = [vp, d, d]
    L.sgo_solve.argtypes = [vp, d, d]
    L.sgo_precondition.argtypes = [vp, d, d]
    L.sgo_solve_rhs.argtypes = [vp, d, d, d]
    L.sgo_marginals.argtypes = [vp, C.c_int32, i32, i32, d]
    L.sgo_marginals_selected.argtypes = [vp, d, C.c_int32, i32, i32, d]
    L.sgo_factor_solve.argtypes = [vp, C.c_int32, d, d]
    L.sgo_candidate_gate.argtypes = [vp, C.c_int32, i32, i32, d, d, C.c_double, d, d, u8]
    L.sgo_candidate_joint.argtypes = [vp, C.c_int32, i32, i32, d, d, d, d]
    L.sgo_joint_subsets.argtypes = [vp, C.c_int32, C.c_int32, u8, d, d, i32, u8]
    L.sgo_joint_pairs.argtypes = [vp, C.c_int32, d]
    L.sgo_edge_leave_one_out.argtypes = [vp, C.c_int32, i32, C.c_double, C.c_double, d, d, d, u8]
    L.sgo_edge_loo_rule.argtypes = [d, d, d, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), d]
    L.sgo_joint_greedy.argtypes = [vp, C.c_int32, C.c_int32, i32, u8, d, C.c_int32, i32, i32, i32, d, d]
    L.sgo_joint_extend.argtypes = [vp, C.c_int32, C.c_int32, i32, d, d]
    L.sgo_edge_joint.argtypes = [vp, C.c_int32, i32, d, d, d]
    L.sgo_edge_groups.argtypes = [vp, C.c_int32, C.c_int32, u8, d, C.c_double, d, i32, d, u8]
    L.sgo_edge_group_rule.argtypes = [C.c_int32, d, d, d, d, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.sgo_closure_search.argtypes = [vp, C.c_int32, i32, C.c_int32, i32, C.c_double, C.c_double, C.c_int32, d, d, d, d, u8]
    L.sgo_closure_search_rule.argtypes = [d, d, d, d, d, C.c_double, d, d, C.POINTER(C.c_double), d]
    L.sgo_joint_greedy_rule.argtypes = [C.c_int32, d, d, i32, u8, d, C.c_int32, i32, i32, i32, d, d]
    L.sgo_kernel_profile.argtypes = [vp, C.POINTER(KernelStat), C.c_int]
    L.sgo_kernel_profile_samples.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int]
    L.sgo_solver_description.restype = C.c_char_p
    L.sgo_solver_description.argtypes = [vp]
    L.sgo_profile_reset.argtypes = [vp]
    L.sgo_profile_overhead_ms.restype = C.c_double
    L.sgo_profile_overhead_ms.argtypes = [vp]
    L.sgo_comm_unique_id.argtypes = [vp]
    L.sgo_comm_init.argtypes = [vp, C.c_int, C.c_int, vp]
    L.sgo_comm_size.argtypes = [vp]
    L.sgo_comm_init_host.argtypes = [vp, C.c_int, C.c_int, HOST_ALLREDUCE, vp]
    L.sgo_comm_host_allgather.argtypes = [vp, HOST_ALLGATHER]
    L.sgo_debug_amg_array.restype = C.c_int64
    L.sgo_debug_amg_array.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int64]
    L.sgo_debug_overlay_array.restype = C.c_int64
    L.sgo_debug_overlay_array.argtypes = [vp, C.c_int32, vp, C.c_int64]
    L.sgo_debug_overlay_linearize.argtypes = [vp, d]
    L.sgo_debug_overlay_apply.argtypes = [vp, d, d, d]
    L.sgo_debug_mfront_array.restype = C.c_int64
    L.sgo_debug_mfront_array.argtypes = [vp, C.c_int32, vp, C.c_int64]
    L.sgo_debug_pcg_array.restype = C.c_int64
    L.sgo_debug_pcg_array.argtypes = [vp, C.c_int32, vp, C.c_int64]
    L.sgo_debug_pcg_run.argtypes = [vp, C.c_int32, d, C.c_double, C.c_int32, C.c_double]
    L.sgo_debug_direct_array.restype = C.c_int64
    L.sgo_debug_direct_array.argtypes = [vp, C.c_int32, vp, C.c_int64]
    L.sgo_direct_plan_array.restype = C.c_int64
    L.sgo_direct_plan_array.argtypes = [C.c_int32, u8, C.c_int32, i32, i32, C.c_int32, C.c_int32, vp, C.c_int64]
    L.sgo_mfront_plan_array.restype = C.c_int64
    L.sgo_mfront_plan_array.argtypes = [C.c_int32, d, u8, C.c_int32, i32, i32, C.c_int32, C.c_double, C.c_int32, vp, C.c_int64]
    L.sgo_debug_level0_bytes.restype = C.c_int64
    L.sgo_debug_level0_bytes.argtypes = [vp]
    L.sgo_shard_range.restype = None
    L.sgo_shard_range.argtypes = [C.c_int32, C.c_int32, C.c_int32, i32, i32]
    L.sgo_debug_set_shard.argtypes = [vp, C.c_int, C.c_int]
    L.sgo_closure_information.argtypes = [vp, C.c_int32, C.POINTER(MatchWindow), C.POINTER(C.c_float), C.c_int64, d, d]
    L.sgo_plan_rows.argtypes = [C.c_int32, d, u8, C.c_int32, i32, i32, C.c_int32, i32, i32, i32, i32, C.c_int32, i32, d]
    L.sgo_last_error.restype = C.c_char_p
    L.sgo_last_error.argtypes = [vp]
    _LIB = L
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def default_opts() -> Opts:
    o = Opts()
    lib().sgo_default_opts(C.byref(o))
    return o


def shard_range(count: int, nranks: int, rank: int):
    """[begin, end) of the work units rank `rank` evaluates (sgo_shard_range; needs no GPU)."""
    a = C.c_int32()
    b = C.c_int32()
    lib().sgo_shard_range(count, nranks, rank, C.byref(a), C.byref(b))
    return a.value, b.value


def plan_rows(poses, fixed, ei, ej, nranks: int = 1, meas=None):
    """Host-only row plan of a graph (sgo_plan_rows; needs no GPU): dict with n, row_vertex (n,),
    tile_row_begin (ntiles + 1,), rank_row_begin (nranks + 1,).  meas: the measurements (as set_graph's) -- with them the plan is
    also right for a graph whose initial poses contradict its closures (rows ordered by spanning-tree positions)."""
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(fixed, dtype=np.uint8)
    a = np.ascontiguousarray(ei, dtype=np.int32)
    b = np.ascontiguousarray(ej, dtype=np.int32)
    V = p.shape[0]
    n = C.c_int32()
    nt = C.c_int32()
    rv = np.empty(V, dtype=np.int32)
    tb = np.empty(V + 2, dtype=np.int32)
    rb = np.empty(nranks + 1, dtype=np.int32)
    rc = lib().sgo_plan_rows(V, _dp(p), f.ctypes.data_as(C.POINTER(C.c_uint8)), a.size, _ip(a), _ip(b), nranks,
                             C.byref(n), _ip(rv), C.byref(nt), _ip(tb), tb.size, _ip(rb),
                             _dp(np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 3)) if meas is not None else None)
    if rc != 0:
        raise SgoError(f"sgo_plan_rows: rc={rc}: " + lib().sgo_last_error(None).decode())
    return dict(n=n.value, row_vertex=rv[: n.value].copy(), tile_row_begin=tb[: nt.value + 1].copy(),
                rank_row_begin=rb.copy())


MFRONT_STATS = ("n", "fronts", "levels", "max_dim", "max_own", "max_bnd", "flops", "crit_flops", "crit_panels",
                "arena_bytes", "order_kind", "targets")


def mfront_plan(poses, fixed, ei, ej, leaf: int = 0, max_crit_mflop: float = 0.0):
    """Host-only elimination plan of the multifrontal path (sgo_mfront_plan; needs no GPU): dict of MFRONT_STATS plus
    ``qualifies``, ``why``, ``elim_vertex`` (n,), ``front_of_elim`` (n,)."""
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(fixed, dtype=np.uint8)
    a = np.ascontiguousarray(ei, dtype=np.int32)
    b = np.ascontiguousarray(ej, dtype=np.int32)
    V = p.shape[0]
    st = np.zeros(12, dtype=np.int64)
    ev = np.full(V, -1, dtype=np.int32)
    fe = np.full(V, -1, dtype=np.int32)
    L = lib()
    L.sgo_mfront_plan.argtypes = [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_int32, C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32), C.c_int32, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32)]
    rc = L.sgo_mfront_plan(V, _dp(p), f.ctypes.data_as(C.POINTER(C.c_uint8)), a.size, _ip(a), _ip(b), leaf, max_crit_mflop,
                           st.ctypes.data_as(C.POINTER(C.c_int64)), _ip(ev), _ip(fe))
    if rc not in (0, -1):
        raise SgoError(f"sgo_mfront_plan: rc={rc}: " + L.sgo_last_error(None).decode())
    out = {k: int(v) for k, v in zip(MFRONT_STATS, st)}
    out["qualifies"] = rc == 0
    out["why"] = "" if rc == 0 else L.sgo_last_error(None).decode()
    n = out["n"]
    out["elim_vertex"] = ev[:n].copy()
    out["front_of_elim"] = fe[:n].copy()
    return out


# SGO_MF_* of include/sgo.h: name -> (number, dtype, columns); the first nine are the host plan's as well
MFRONT_ARRAYS = {"INFO": (0, np.int64, 0), "FRONTS": (1, np.int64, 14), "LEVEL_PTR": (2, np.int32, 0), "LEVEL_FRONT": (3, np.int32, 0),
                 "BND": (4, np.int32, 0), "PINV": (5, np.int32, 0), "TARGETS": (6, np.int32, 4), "CONTRIB": (7, np.int32, 0),
                 "ELIM_VERTEX": (8, np.int32, 0), "ELEM": (9, np.float64, 28), "ARENA": (10, np.float64, 0), "X": (11, np.float64, 0),
                 "INVD": (12, np.float64, 0), "YINV": (13, np.float64, 16), "FLAGS": (14, np.int32, 0),
                 "SEL": (15, np.float64, 0), "FS_Y": (16, np.float64, 0), "FS_X": (17, np.float64, 0)}
MFRONT_PLAN_ARRAYS = ("INFO", "FRONTS", "LEVEL_PTR", "LEVEL_FRONT", "BND", "PINV", "TARGETS", "CONTRIB", "ELIM_VERTEX")


def _mfront_fetch(name, call, err):
    what, dtype, cols = MFRONT_ARRAYS[name]
    size = call(what, None, 0)
    if size < 0:
        raise SgoError(f"{name}: rc={size}: " + err())
    out = np.empty(size // np.dtype(dtype).itemsize, dtype=dtype)
    if size:
        got = call(what, out.ctypes.data_as(C.c_void_p), out.nbytes)
        if got != size:
            raise SgoError(f"{name}: {got} bytes after {size}: " + err())
    return out.reshape(-1, cols) if cols else out


def mfront_plan_arrays(poses, fixed, ei, ej, leaf: int = 0, max_crit_mflop: float = 0.0):
    """The host plan's arrays (sgo_mfront_plan_array; needs no GPU): {name: array} for MFRONT_PLAN_ARRAYS, the very tables
    sgo_set_graph_se2 uploads for this graph under the same environment.  SgoError when the graph does not qualify."""
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(fixed, dtype=np.uint8)
    a = np.ascontiguousarray(ei, dtype=np.int32)
    b = np.ascontiguousarray(ej, dtype=np.int32)
    L = lib()

    def call(what, out, cap):
        return L.sgo_mfront_plan_array(p.shape[0], _dp(p), f.ctypes.data_as(C.POINTER(C.c_uint8)), a.size, _ip(a), _ip(b), leaf,
                                       max_crit_mflop, what, out, cap)
    return {k: _mfront_fetch(k, call, lambda: L.sgo_last_error(None).decode()) for k in MFRONT_PLAN_ARRAYS}


# SGO_DR_* of include/sgo.h: name -> (number, dtype, columns); the first thirteen are the host plan's as well
DIRECT_ARRAYS = {"INFO": (0, np.int64, 0), "POS_VERTEX": (1, np.int32, 0), "VREC": (2, np.int32, 4), "VOVER": (3, np.int32, 0),
                 "EDGE_TGT": (4, np.uint32, 0), "ZERO_SLOTS": (5, np.int32, 0), "MULTI": (6, np.int32, 2), "ENEXT": (7, np.int32, 0),
                 "SLOT_RC": (8, np.int32, 2), "LMETA": (9, np.int32, 0), "TK": (10, np.int32, 4), "CTR": (11, np.int32, 4),
                 "DPAIR": (12, np.uint16, 0), "ESCR": (13, np.float64, 0), "ZSC": (14, np.float64, 0), "WD": (15, np.float64, 10),
                 "WO": (16, np.float64, 10), "A_WD": (17, np.float64, 10), "A_WO": (18, np.float64, 10), "A_SD": (19, np.float64, 0),
                 "A_XB": (20, np.float64, 0), "F_SD": (21, np.float64, 0), "F_XB": (22, np.float64, 0), "D_SD": (23, np.float64, 0),
                 "D_PINV": (24, np.float64, 6), "D_BS": (25, np.float64, 0), "X": (26, np.float64, 0)}
DIRECT_PLAN_ARRAYS = tuple(DIRECT_ARRAYS)[:13]
DIRECT_INFO = ("n", "nI", "ns", "NL", "E", "NB", "tri", "nzero", "nmulti", "tasks", "contributions", "lds_bytes", "xb_global")


def _direct_fetch(name, call, err):
    what, dtype, cols = DIRECT_ARRAYS[name]
    size = call(what, None, 0)
    if size < 0:
        raise SgoError(f"{name}: rc={size}: " + err())
    out = np.empty(size // np.dtype(dtype).itemsize, dtype=dtype)
    if size:
        got = call(what, out.ctypes.data_as(C.c_void_p), out.nbytes)
        if got != size:
            raise SgoError(f"{name}: {got} bytes after {size}: " + err())
    return out.reshape(-1, cols) if cols else out


def direct_plan_arrays(fixed, ei, ej, max_rows: int = 0, names=DIRECT_PLAN_ARRAYS):
    """The host analysis of the single-launch direct path (sgo_direct_plan_array; needs no GPU): {name: array} for
    DIRECT_PLAN_ARRAYS, the very tables sgo_set_graph_se2 uploads for this graph.  SgoError when the graph does not qualify: its
    text ends with the reason sgo_solver_description gives."""
    f = np.ascontiguousarray(fixed, dtype=np.uint8)
    a = np.ascontiguousarray(ei, dtype=np.int32)
    b = np.ascontiguousarray(ej, dtype=np.int32)
    L = lib()

    def call(what, out, cap):
        return L.sgo_direct_plan_array(f.size, f.ctypes.data_as(C.POINTER(C.c_uint8)), a.size, _ip(a), _ip(b), max_rows, what, out, cap)
    return {k: _direct_fetch(k, call, lambda: L.sgo_last_error(None).decode()) for k in names}


# SGO_PCG_* of include/sgo.h: name -> (number, dtype, columns); SCALARS / HOST_SCALARS / MIRROR are PcgScalars records
PCG_SCALARS = np.dtype([("rz", "f8"), ("pq", "f8"), ("rr", "f8"), ("bb", "f8"), ("alpha", "f8"), ("beta", "f8"), ("tol2", "f8"),
                        ("rz_prev", "f8"), ("iter", "i4"), ("maxit", "i4"), ("stop", "i4"), ("iter_prev", "i4"), ("probe_k", "i4"),
                        ("pad", "i4"), ("probe_rel", "f8"), ("probe_max", "f8")])
PCG_ARRAYS = {"B": (0, np.float64, 3), "X": (1, np.float64, 3), "R": (2, np.float64, 3), "Z": (3, np.float64, 3), "P": (4, np.float64, 3),
              "Q": (5, np.float64, 3), "DINV": (6, np.float64, 6), "XS0": (7, np.float64, 3), "SCALARS": (8, PCG_SCALARS, 0),
              "HOST_SCALARS": (9, PCG_SCALARS, 0), "MIRROR": (10, PCG_SCALARS, 0), "PARTIALS": (11, np.float64, 2048),
              "ZPARTS": (12, np.float64, 2048), "COUNTS": (13, np.int32, 0), "LANCZOS": (14, np.float64, 3), "ROW_ORDER": (15, np.int32, 0),
              "START_ARGS": (16, np.float64, 0)}


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    rc = lib().sgo_comm_unique_id(C.cast(buf, C.c_void_p))
    if rc != 0:
        raise SgoError("sgo_comm_unique_id: " + lib().sgo_last_error(None).decode())
    return buf.raw


def optimize_many(opts, max_iters: int = 20, gain_tol: float = 0.0):
    """sgo_optimize_gn_many: every Optimizer of `opts` as its own optimize_until(max_iters, gain_tol), the direct_ldlt ones in one
    shared launch with a workgroup per graph -> (list with, per context, the stats dict optimize_until returns plus stop_reason
    and in_launch; launches: the shared launches the call made).  A context whose own call would have raised carries its error
    code in rc; SgoError for a refusal of the whole call."""
    opts = list(opts)
    n = len(opts)
    handles = (C.c_void_p * max(n, 1))(*[o._h for o in opts])
    stats = [Stats() for _ in opts]
    sp = (C.POINTER(Stats) * max(n, 1))(*[C.pointer(st) for st in stats])
    res = (ManyResult * max(n, 1))()
    launches = C.c_int32(-1)
    rc = lib().sgo_optimize_gn_many(handles, n, max_iters, float(gain_tol), sp, res, C.byref(launches))
    if rc < 0:
        raise SgoError(f"sgo_optimize_gn_many: rc={rc}: " + lib().sgo_last_error(opts[0]._h if n else None).decode())
    out = []
    for o, st, r in zip(opts, stats, res):
        d = o._stats_dict(r.rc, st, max_iters)
        d.update(stop_reason=r.stop_reason, in_launch=r.in_launch)
        out.append(d)
    return out, launches.value


class Optimizer:
    """One ``sgo_ctx``: the device-side stand-in for the reference's pose-graph
    ``g2o::SparseOptimizer`` (src/sparse_gslam/include/graphs.h:31-40)."""

    def __init__(self, device: int = 0, **opts):
        L = lib()
        o = default_opts()
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown option {k}")
            setattr(o, k, v)
        self._h = L.sgo_create(device, C.byref(o))
        if not self._h:
            raise SgoError("sgo_create: " + L.sgo_last_error(None).decode())
        self.V = self.E = 0
        self.last_stats = None

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            lib().sgo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc < 0 and rc != -1:
            raise SgoError(f"{what}: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        return rc

    # -- multi-GPU
    def comm_init(self, nranks: int, rank: int, unique_id: bytes):
        buf = C.create_string_buffer(unique_id, UNIQUE_ID_BYTES)
        self._check(lib().sgo_comm_init(self._h, nranks, rank, C.cast(buf, C.c_void_p)), "sgo_comm_init")

    def comm_init_host(self, nranks: int, rank: int, allreduce, allgather=None):
        """Multi-GPU mode over the caller's transport (sgo_comm_init_host): `allreduce(a)` must replace the
        float64 numpy array `a` in place by its sum over all ranks (e.g. a gloo all_reduce); the optional
        `allgather(send, recv)` fills recv (nranks * len(send)) with every rank's send (sgo_comm_host_allgather)."""
        def _cb(buf, count, _user):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(count,)))
                return 0
            except Exception:   # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        self._host_cb = HOST_ALLREDUCE(_cb)   # keep the trampoline alive as long as the context
        self._check(lib().sgo_comm_init_host(self._h, nranks, rank, self._host_cb, None), "sgo_comm_init_host")
        if allgather is not None:
            def _gcb(send, count, recv, _user):
                try:
                    allgather(np.ctypeslib.as_array(send, shape=(count,)), np.ctypeslib.as_array(recv, shape=(count * nranks,)))
                    return 0
                except Exception:
                    import traceback
                    traceback.print_exc()
                    return 1
            self._host_gcb = HOST_ALLGATHER(_gcb)
            self._check(lib().sgo_comm_host_allgather(self._h, self._host_gcb), "sgo_comm_host_allgather")

    def level0_bytes(self) -> int:
        """Device bytes of the level-0 structure this rank holds (sgo_debug_level0_bytes)."""
        return int(lib().sgo_debug_level0_bytes(self._h))

    def debug_set_shard(self, nranks: int, rank: int):
        self._check(lib().sgo_debug_set_shard(self._h, nranks, rank), "sgo_debug_set_shard")

    # -- graph
    def set_graph(self, poses, fixed, ei, ej, meas, info, phi):
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        f = np.ascontiguousarray(fixed, dtype=np.uint8)
        a = np.ascontiguousarray(ei, dtype=np.int32)
        b = np.ascontiguousarray(ej, dtype=np.int32)
        m = np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 3)
        o = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 6)
        ph = np.ascontiguousarray(phi, dtype=np.float64)
        if not (f.shape[0] == p.shape[0] and a.size == b.size == m.shape[0] == o.shape[0] == ph.size):
            raise ValueError("inconsistent array sizes")
        self._check(lib().sgo_set_graph_se2(self._h, p.shape[0], _dp(p), f.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            a.size, _ip(a), _ip(b), _dp(m), _dp(o), _dp(ph)),
                    "sgo_set_graph_se2")
        self.V, self.E = p.shape[0], a.size

    def update_graph(self, poses, fixed, ei, ej, meas, info, phi, n_resident_edges: int):
        """sgo_update_graph_se2: the whole new graph + how many leading edges are the resident graph's (incremental set-up)."""
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        f = np.ascontiguousarray(fixed, dtype=np.uint8)
        a = np.ascontiguousarray(ei, dtype=np.int32)
        b = np.ascontiguousarray(ej, dtype=np.int32)
        m = np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 3)
        o = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 6)
        ph = np.ascontiguousarray(phi, dtype=np.float64)
        if not (f.shape[0] == p.shape[0] and a.size == b.size == m.shape[0] == o.shape[0] == ph.size):
            raise ValueError("inconsistent array sizes")
        self._check(lib().sgo_update_graph_se2(self._h, p.shape[0], _dp(p), f.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               a.size, _ip(a), _ip(b), _dp(m), _dp(o), _dp(ph), int(n_resident_edges)),
                    "sgo_update_graph_se2")
        self.V, self.E = p.shape[0], a.size

    def set_poses(self, poses):
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(self.V, 3)
        self._check(lib().sgo_set_poses(self._h, _dp(p)), "sgo_set_poses")

    def get_poses(self):
        p = np.empty((self.V, 3))
        self._check(lib().sgo_get_poses(self._h, _dp(p)), "sgo_get_poses")
        return p

    @property
    def n_free(self):
        return self._check(lib().sgo_num_free(self._h), "sgo_num_free")

    def free_ids(self):
        out = np.empty(self.n_free, dtype=np.int32)
        self._check(lib().sgo_free_ids(self._h, _ip(out)), "sgo_free_ids")
        return out

    # -- optimisation
    def optimize(self, iters: int = 20):
        """optimize(iters) -> (iterations done, stats dict)."""
        st = Stats()
        rc = self._check(lib().sgo_optimize_gn(self._h, iters, C.byref(st)), "sgo_optimize_gn")
        return rc, self._stats_dict(rc, st, iters)

    def optimize_until(self, max_iters: int = 20, gain_tol: float = 1e-6):
        """sgo_optimize_gn_until: optimize(max_iters) that ends before the first iteration (from the third on) at which the relative
        gain of the robust chi2 is in [0, gain_tol) -> (iterations done, stats dict, stop reason: one of STOP_*)."""
        st = Stats()
        why = C.c_int32(-1)
        rc = self._check(lib().sgo_optimize_gn_until(self._h, max_iters, gain_tol, C.byref(st), C.byref(why)), "sgo_optimize_gn_until")
        return rc, self._stats_dict(rc, st, max_iters), why.value

    def optimize_lm(self, max_iters: int = 20, lambda_init: float = 0.0):
        """sgo_optimize_lm: Levenberg-Marquardt with g2o's schedule on the multifrontal factor -> (iterations counted, or -1 when the
        analysis refuses the graph (last_error() has the reason); stats dict: lambda0, lambda / trials per iteration, robust_chi2 /
        chi2 at the start and after every iteration, trials_total, stop_reason (one of LM_STOP_*), sync_rounds)."""
        st = LmStats()
        rc = self._check(lib().sgo_optimize_lm(self._h, max_iters, lambda_init, C.byref(st)), "sgo_optimize_lm")
        return rc, self._lm_dict(rc, st)

    @staticmethod
    def _lm_dict(rc, st):
        d = max(st.iters_done, 0)
        return dict(rc=rc, iters_done=st.iters_done, trials_total=st.trials_total, stop_reason=st.stop_reason,
                    sync_rounds=st.sync_rounds, lambda0=st.lambda0, lam=list(st.lam[:d]), trials=list(st.trials[:d]),
                    robust_chi2=list(st.robust_chi2[: d + 1]), chi2=list(st.chi2[: d + 1]), seconds_total=st.seconds_total)

    def optimize_lm_pcg(self, max_iters: int = 20, lambda_init: float = 0.0):
        """sgo_optimize_lm_pcg: optimize_lm's schedule with every trial solved by the context's PCG, on every single-GPU context and
        never refused for the graph's size -> (iterations counted, optimize_lm's stats dict; sync_rounds = the trials run)."""
        st = LmStats()
        rc = self._check(lib().sgo_optimize_lm_pcg(self._h, max_iters, lambda_init, C.byref(st)), "sgo_optimize_lm_pcg")
        return rc, self._lm_dict(rc, st)

    def lm_pcg_trace(self):
        """sgo_lm_pcg_trace: the trials of the last optimize_lm_pcg -> (pcg_iters, solve_stop), int32 arrays with one entry per trial;
        solve_stop is LM_SOLVE_CONVERGED, LM_SOLVE_FLOOR, or minus the PCG stop code of a failed solve (a rejected trial)."""
        n = self._check(lib().sgo_lm_pcg_trace(self._h, 0, None, None), "sgo_lm_pcg_trace")
        its, how = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        if n:
            self._check(lib().sgo_lm_pcg_trace(self._h, n, its.ctypes.data_as(C.POINTER(C.c_int32)), how.ctypes.data_as(C.POINTER(C.c_int32))),
                        "sgo_lm_pcg_trace")
        return its, how

    def optimize_dogleg(self, max_iters: int = 20, delta_init: float = 0.0):
        """sgo_optimize_dogleg: Powell's dogleg with g2o's schedule, one factorisation per iteration on the multifrontal factor ->
        (iterations counted, or -1 when the analysis refuses the graph (last_error() has the reason); stats dict: delta0, delta /
        trials / step_kind per iteration, robust_chi2 / chi2 at the start and after every iteration, trials_total, solves,
        stop_reason (one of DL_STOP_*), sync_rounds, lam: the last damping used)."""
        st = DoglegStats()
        rc = self._check(lib().sgo_optimize_dogleg(self._h, max_iters, delta_init, C.byref(st)), "sgo_optimize_dogleg")
        return rc, self._dogleg_dict(rc, st)

    def optimize_dogleg_pcg(self, max_iters: int = 20, delta_init: float = 0.0):
        """sgo_optimize_dogleg_pcg: optimize_dogleg's schedule with the iteration's one solve done by the context's PCG, on every
        single-GPU context and never refused for the graph's size -> (iterations counted, optimize_dogleg's stats dict)."""
        st = DoglegStats()
        rc = self._check(lib().sgo_optimize_dogleg_pcg(self._h, max_iters, delta_init, C.byref(st)), "sgo_optimize_dogleg_pcg")
        return rc, self._dogleg_dict(rc, st)

    @staticmethod
    def _dogleg_dict(rc, st):
        d = max(st.iters_done, 0)
        return dict(rc=rc, iters_done=st.iters_done, trials_total=st.trials_total, solves=st.solves, stop_reason=st.stop_reason,
                    sync_rounds=st.sync_rounds, delta0=st.delta0, delta=list(st.delta[:d]), trials=list(st.trials[:d]),
                    step_kind=list(st.step_kind[:d]), robust_chi2=list(st.robust_chi2[: d + 1]), chi2=list(st.chi2[: d + 1]),
                    lam=st.lam, seconds_total=st.seconds_total)

    def set_hypotheses_workspace(self, max_bytes: int) -> None:
        """sgo_set_hypotheses_workspace: the device memory optimize_hypotheses may take for per-hypothesis copies on a
        multifrontal_cholesky context (0, the default: the sequential route)."""
        self._check(lib().sgo_set_hypotheses_workspace(self._h, int(max_bytes)), "sgo_set_hypotheses_workspace")

    def hypotheses_bytes(self, max_iters: int = 20, want_edge_chi2: bool = True) -> int:
        """sgo_hypotheses_bytes: bytes one hypothesis takes on the resident graph; 0 where there is no batched multifrontal route."""
        return int(self._check(lib().sgo_hypotheses_bytes(self._h, max_iters, 1 if want_edge_chi2 else 0), "sgo_hypotheses_bytes"))

    def hypotheses_workspace_bytes(self) -> int:
        """sgo_hypotheses_workspace_bytes: the device bytes the context's hypotheses workspace holds now."""
        return int(self._check(lib().sgo_hypotheses_workspace_bytes(self._h), "sgo_hypotheses_workspace_bytes"))

    def many_workspace_bytes(self) -> int:
        """sgo_many_workspace_bytes: the bytes (device + pinned host) of the optimize_many workspace this context holds now."""
        return int(self._check(lib().sgo_many_workspace_bytes(self._h), "sgo_many_workspace_bytes"))

    def optimize_hypotheses(self, edge_off, max_iters: int = 20, gain_tol: float = 0.0, poses0=None,
                            want=("hist", "poses", "edge_chi2"), out=None):
        """sgo_optimize_gn_hypotheses: the resident graph optimised once per row of edge_off (B, E) -- non-zero: that edge is
        switched off in that hypothesis -- from poses0 (B, V, 3) or the resident poses, each as optimize_until(max_iters, gain_tol).
        -> dict: route (HYP_*), iters_done (B,), stop_reason (B,), chi2 (B,), robust_chi2 (B,) and, as `want` names them,
        hist (B, max_iters + 1, 2; NaN behind the applied iterations), poses (B, V, 3), edge_chi2 (B, E; with the resident
        information).  The context is left as it was.  out: arrays to write into instead of fresh ones, by those names and
        "res" (a HypothesisResult array)."""
        m = np.ascontiguousarray(edge_off, dtype=np.uint8)
        if m.ndim != 2 or m.shape[1] != self.E:
            raise ValueError("edge_off must be (B, E)")
        B = m.shape[0]
        p0 = None
        if poses0 is not None:
            p0 = np.ascontiguousarray(poses0, dtype=np.float64)
            if p0.shape != (B, self.V, 3):
                raise ValueError("poses0 must be (B, V, 3)")
        out = dict(out or {})
        res = out.get("res")
        if res is None:
            res = (HypothesisResult * max(B, 1))()
        shapes = dict(hist=(B, max_iters + 1, 2), poses=(B, self.V, 3), edge_chi2=(B, self.E))
        arr = {}
        for k in ("hist", "poses", "edge_chi2"):
            if k in want:
                a = out.get(k)
                arr[k] = np.empty(shapes[k]) if a is None else a
                if arr[k].shape != shapes[k] or arr[k].dtype != np.float64 or not arr[k].flags.c_contiguous:
                    raise ValueError(f"out[{k!r}] must be a contiguous float64 array of shape {shapes[k]}")
        ptr = {k: (_dp(arr[k]) if k in arr else None) for k in shapes}
        route = self._check(lib().sgo_optimize_gn_hypotheses(
            self._h, B, max_iters, float(gain_tol), m.ctypes.data_as(C.POINTER(C.c_uint8)), None if p0 is None else _dp(p0),
            res, ptr["hist"], ptr["poses"], ptr["edge_chi2"]), "sgo_optimize_gn_hypotheses")
        r = dict(route=route,
                 iters_done=np.array([res[b].iters_done for b in range(B)], dtype=np.int32),
                 stop_reason=np.array([res[b].stop_reason for b in range(B)], dtype=np.int32),
                 chi2=np.array([res[b].chi2 for b in range(B)], dtype=np.float64),
                 robust_chi2=np.array([res[b].robust_chi2 for b in range(B)], dtype=np.float64))
        r.update(arr)
        return r

    def _stats_dict(self, rc, st, iters):
        d = max(st.iters_done, 0)
        stats = dict(
            rc=rc, iters_done=st.iters_done, chi2=list(st.chi2[: d + 1]),
            robust_chi2=list(st.robust_chi2[: d + 1]), pcg_iters=list(st.pcg_iters[:iters]),
            pcg_converged=list(st.pcg_converged[:iters]), pcg_relres=list(st.pcg_relres[:iters]),
            seconds=list(st.seconds[:iters]), seconds_linearize=list(st.seconds_linearize[:iters]),
            seconds_solve=list(st.seconds_solve[:iters]), seconds_total=st.seconds_total,
            seconds_setup=st.seconds_setup)
        self.last_stats = stats
        return stats

    def chi2(self):
        a = C.c_double()
        b = C.c_double()
        self._check(lib().sgo_chi2(self._h, C.byref(a), C.byref(b)), "sgo_chi2")
        return a.value, b.value

    def edge_chi2(self):
        out = np.empty(self.E)
        self._check(lib().sgo_edge_chi2(self._h, _dp(out)), "sgo_edge_chi2")
        return out

    def set_edge_information(self, edge_ids, info):
        """sgo_set_edge_information: new information rows (n, 6) for resident edges; an all-zero row deactivates the edge.
        No set-up runs; SgoError (rc=-2) with the device untouched when the call refuses."""
        ids = np.ascontiguousarray(edge_ids, dtype=np.int32).reshape(-1)
        o = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 6)
        if o.shape[0] != ids.size:
            raise ValueError("inconsistent array sizes")
        self._check(lib().sgo_set_edge_information(self._h, ids.size, _ip(ids), _dp(o)), "sgo_set_edge_information")

    def gate_edges(self, edge_ids, chi2_max: float):
        """sgo_gate_edges: deactivates the listed edges (None: every edge with a robust kernel) whose chi2 at the current poses
        exceeds chi2_max -> (how many, bool array over the listed edges / over all edges)."""
        ids = None if edge_ids is None else np.ascontiguousarray(edge_ids, dtype=np.int32).reshape(-1)
        gated = np.zeros(self.E if ids is None else ids.size, dtype=np.uint8)
        k = self._check(lib().sgo_gate_edges(self._h, 0 if ids is None else ids.size, None if ids is None else _ip(ids),
                                             float(chi2_max), gated.ctypes.data_as(C.POINTER(C.c_uint8))), "sgo_gate_edges")
        return k, gated.astype(bool)

    def set_robust_kernels(self, edge_ids, kind, delta):
        """sgo_set_robust_kernels: the robust kernel (KERNEL_*) and its parameter for resident edges (edge_ids None: edges
        0 .. n-1); kind and delta broadcast over the edges.  No set-up runs; SgoError (rc=-2) with the device untouched when the
        call refuses."""
        ids = None if edge_ids is None else np.ascontiguousarray(edge_ids, dtype=np.int32).reshape(-1)
        n = np.broadcast(np.asarray(kind), np.asarray(delta)).size if ids is None else ids.size
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(kind, dtype=np.int32).reshape(-1), (n,)))
        dl = np.ascontiguousarray(np.broadcast_to(np.asarray(delta, dtype=np.float64).reshape(-1), (n,)))
        self._check(lib().sgo_set_robust_kernels(self._h, n, None if ids is None else _ip(ids), _ip(k), _dp(dl)),
                    "sgo_set_robust_kernels")

    def edge_robust(self):
        """sgo_edge_robust: (rho0, weight) of every edge at the current poses, in set-graph order."""
        rho0, w = np.empty(self.E), np.empty(self.E)
        self._check(lib().sgo_edge_robust(self._h, _dp(rho0), _dp(w)), "sgo_edge_robust")
        return rho0, w

    def closure_information(self, windows, scores):
        """Covariance and information of a batch of scan-match windows (sgo_closure_information).

        windows: sequence of dicts with the sgo_match_window fields except score_offset, which is
        assigned here (the windows' scores are laid out back to back in `scores`) unless given."""
        n = len(windows)
        arr = (MatchWindow * max(n, 1))()
        off = 0
        for q, w in enumerate(windows):
            for k in ("x_index_offset", "y_index_offset", "scan_index", "scan_window", "w_size",
                      "num_angular_perturbations", "resolution", "angular_step"):
                setattr(arr[q], k, w[k])
            arr[q].score_offset = w.get("score_offset", off)
            off += (2 * w["w_size"] + 1) ** 2 * (2 * w["scan_window"] + 1)
        sc = np.ascontiguousarray(scores, dtype=np.float32)
        cov = np.empty((n, 3, 3))
        info = np.empty((n, 3, 3))
        self._check(lib().sgo_closure_information(self._h, n, arr, sc.ctypes.data_as(C.POINTER(C.c_float)),
                                                  sc.size, _dp(cov), _dp(info)), "sgo_closure_information")
        return cov, info

    # -- single steps (parity tests)
    def linearize(self):
        n = self.n_free
        b = np.empty((n, 3))
        diag = np.empty((n, 3, 3))
        c = C.c_double()
        r = C.c_double()
        self._check(lib().sgo_linearize(self._h, _dp(b), _dp(diag), C.byref(c), C.byref(r)), "sgo_linearize")
        return b, diag, c.value, r.value

    def hessian_apply(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.n_free, 3)
        y = np.empty_like(x)
        self._check(lib().sgo_hessian_apply(self._h, _dp(x), _dp(y)), "sgo_hessian_apply")
        return y

    def precondition(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(self.n_free, 3)
        z = np.empty_like(r)
        self._check(lib().sgo_precondition(self._h, _dp(r), _dp(z)), "sgo_precondition")
        return z

    def solve(self):
        x = np.empty((self.n_free, 3))
        rr = C.c_double()
        it = self._check(lib().sgo_solve(self._h, _dp(x), C.byref(rr)), "sgo_solve")
        return x, it, rr.value

    def solve_rhs(self, b):
        """sgo_solve_rhs: H x = b for the caller's b (n_free, 3) with the Hessian of the last linearize() -> (x, iters, relres)."""
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(self.n_free, 3)
        x = np.empty_like(b)
        rr = C.c_double()
        it = self._check(lib().sgo_solve_rhs(self._h, _dp(b), _dp(x), C.byref(rr)), "sgo_solve_rhs")
        return x, it, rr.value

    def marginals_selected(self, vi=None, vj=None, diag=True):
        """sgo_marginals_selected: the 3x3 covariance block of every vertex (diag=True -> (V, 3, 3), zero blocks for fixed vertices
        and vertices without an edge) and the blocks (rows of vi[t], columns of vj[t]) of pairs that share a front of the
        multifrontal factorisation -> (diag or None, cov (npairs, 3, 3)).  One factorisation and one top-down pass whatever the
        counts; the number of fronts is kept in ``last_selected_fronts``.  SgoError with rc=-1 when the multifrontal analysis
        refuses the graph (use marginals then)."""
        a = np.ascontiguousarray([] if vi is None else vi, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray([] if vj is None else vj, dtype=np.int32).reshape(-1)
        if a.size != b.size:
            raise ValueError("inconsistent array sizes")
        D = np.empty((self.V, 3, 3)) if diag else None
        cov = np.empty((a.size, 3, 3))
        rc = lib().sgo_marginals_selected(self._h, _dp(D) if diag else None, a.size, _ip(a), _ip(b), _dp(cov))
        if rc < 0:
            raise SgoError(f"sgo_marginals_selected: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        self.last_selected_fronts = rc
        return D, cov

    def factor_solve(self, B):
        """sgo_factor_solve: H X = B for the right-hand sides B (nrhs, n_free, 3) (or one, (n_free, 3)) through the multifrontal
        factor at the current poses -> X of B's shape.  The number of fronts is kept in ``last_selected_fronts``; SgoError with rc=-1
        when the multifrontal analysis refuses the graph (use solve_rhs then)."""
        B = np.ascontiguousarray(B, dtype=np.float64)
        nrhs = B.size // max(3 * self.n_free, 1) if self.n_free else 0
        if nrhs * 3 * self.n_free != B.size:
            raise ValueError("B is not a whole number of right-hand sides")
        X = np.empty_like(B)
        rc = lib().sgo_factor_solve(self._h, nrhs, _dp(B), _dp(X))
        if rc < 0:
            raise SgoError(f"sgo_factor_solve: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        self.last_selected_fronts = rc
        return X

    def candidate_gate(self, ci, cj, meas, info, chi2_max):
        """sgo_candidate_gate: the innovation gate for candidate edges (ci[t], cj[t]) with measurements meas (n, 3) and information
        info (n, 6) that are not part of the graph -> (npass, d2 (n,), cov_pred (n, 3, 3), passed (n,) bool):
        d2 = e^T (Omega^-1 + J Sigma J^T)^-1 e at the current poses, passed = d2 <= chi2_max."""
        a = np.ascontiguousarray(ci, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(cj, dtype=np.int32).reshape(-1)
        z = np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 3)
        w = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 6)
        if not (a.size == b.size == z.shape[0] == w.shape[0]):
            raise ValueError("inconsistent array sizes")
        d2, P, ok = np.empty(a.size), np.empty((a.size, 3, 3)), np.zeros(a.size, dtype=np.uint8)
        rc = lib().sgo_candidate_gate(self._h, a.size, _ip(a), _ip(b), _dp(z), _dp(w), float(chi2_max), _dp(d2), _dp(P),
                                      ok.ctypes.data_as(C.POINTER(C.c_uint8)))
        if rc < 0:
            raise SgoError(f"sgo_candidate_gate: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        return rc, d2, P, ok.astype(bool)

    def edge_leave_one_out(self, edge_ids, chi2_max: float, min_redundancy: float = 1e-3):
        """sgo_edge_leave_one_out: the leave-one-out test of the listed resident edges (None: every edge) from one selected
        inversion -> (nfail, d2 (n,), redundancy (n,), cov_loo (n, 3, 3), fail (n,) bool): d2 is what candidate_gate would say about
        the edge had it never been inserted, fail = redundancy >= min_redundancy and d2 > chi2_max; a bridge edge (redundancy below
        min_redundancy) has d2 = cov_loo = NaN and does not fail.  SgoError with rc=-1 when the multifrontal analysis refuses the
        graph (use optimize_hypotheses then)."""
        ids = None if edge_ids is None else np.ascontiguousarray(edge_ids, dtype=np.int32).reshape(-1)
        n = self.E if ids is None else ids.size
        d2, red, cov, fl = np.empty(n), np.empty(n), np.empty((n, 3, 3)), np.zeros(n, dtype=np.uint8)
        rc = lib().sgo_edge_leave_one_out(self._h, n, None if ids is None else _ip(ids), float(chi2_max), float(min_redundancy),
                                          _dp(d2), _dp(red), _dp(cov), fl.ctypes.data_as(C.POINTER(C.c_uint8)))
        if rc < 0:
            raise SgoError(f"sgo_edge_leave_one_out: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        return rc, d2, red, cov, fl.astype(bool)

    def closure_search(self, query, ids, radius: float, chi2_max: float, min_sep: int = 0):
        """sgo_closure_search: every listed pose j (None: every vertex) against every query pose c from one selected inversion and
        one panel solve -> (count, m2 (nq, n), rel (nq, n, 3), cov_rel (nq, n, 3, 3), sigma (nq, n, 2), near (nq, n) bool): rel is
        c in j's frame, cov_rel its covariance, m2 the squared Mahalanobis distance (1 degree of freedom) from rel's translation
        to the half-plane that contains the disc of `radius`, sigma the 1-sigma linear and angular half-widths of a matcher's
        window, near = m2 <= chi2_max and j != c and |j - c| >= min_sep; count = near.sum().  SgoError with rc=-1 when the
        multifrontal analysis refuses the graph (gate a Euclidean shortlist with candidate_gate then)."""
        q = np.ascontiguousarray(query, dtype=np.int32).reshape(-1)
        j = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        nq, n = q.size, (self.V if j is None else j.size)
        m2, rel, P, sg = np.empty((nq, n)), np.empty((nq, n, 3)), np.empty((nq, n, 3, 3)), np.empty((nq, n, 2))
        nr = np.zeros((nq, n), dtype=np.uint8)
        rc = lib().sgo_closure_search(self._h, nq, _ip(q), n, None if j is None else _ip(j), float(radius), float(chi2_max), int(min_sep),
                                      _dp(m2), _dp(rel), _dp(P), _dp(sg), nr.ctypes.data_as(C.POINTER(C.c_uint8)))
        if rc < 0:
            raise SgoError(f"sgo_closure_search: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        return rc, m2, rel, P, sg, nr.astype(bool)

    def edge_joint(self, edge_ids):
        """sgo_edge_joint: the table of the listed resident edges at the current poses -> (N (3 n, 3 n), e (n, 3), w (n,)):
        N = 1/2 (Q + Q^T), Q = J H^-1 J^T, e the errors, w the kernel weights.  The table (with the edges' resident information) stays
        in the context, a snapshot beside candidate_joint's table, for edge_groups; no edges drop it."""
        ids = np.ascontiguousarray(edge_ids, dtype=np.int32).reshape(-1)
        n = ids.size
        N, e, w = np.empty((3 * n, 3 * n)), np.empty((n, 3)), np.empty(n)
        rc = lib().sgo_edge_joint(self._h, n, _ip(ids), _dp(N), _dp(e), _dp(w))
        if rc < 0:
            raise SgoError(f"sgo_edge_joint: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        self.edge_joint_n = rc
        return N, e, w

    def edge_groups(self, member, chi2_max=None, min_pivot: float = 1e-3):
        """sgo_edge_groups: the leave-group-out test of the groups member (B, n) (non-zero: table row t belongs to the group) of the
        resident edge table -> (nfail, d2 (B,), dof (B,), pivot (B,), fail (B,) bool): d2 is what joint_subsets would say about the
        cluster had it never been inserted, fail = pivot >= min_pivot and d2 > chi2_max[b] (chi2_max None: no decisions, nfail 0); a
        cluster whose removal disconnects the graph (pivot below min_pivot) has d2 = NaN and does not fail."""
        m = np.ascontiguousarray(np.asarray(member) != 0, dtype=np.uint8)
        m = m.reshape(-1, m.shape[-1]) if m.ndim else m.reshape(0, 0)
        B, n = m.shape
        chi = None if chi2_max is None else np.ascontiguousarray(np.broadcast_to(np.asarray(chi2_max, dtype=np.float64), (B,)))
        d2, dof, piv, fl = np.empty(B), np.zeros(B, dtype=np.int32), np.empty(B), np.zeros(B, dtype=np.uint8)
        u8p = C.POINTER(C.c_uint8)
        rc = lib().sgo_edge_groups(self._h, n, B, m.ctypes.data_as(u8p), None if chi is None else _dp(chi), float(min_pivot), _dp(d2), _ip(dof),
                                   _dp(piv), fl.ctypes.data_as(u8p))
        if rc < 0:
            raise SgoError(f"sgo_edge_groups: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        return rc, d2, dof, piv, fl.astype(bool)

    def candidate_joint(self, ci, cj, meas, info):
        """sgo_candidate_joint: the joint table of the candidate edges (arguments as candidate_gate's) at the current poses ->
        (S (3 n, 3 n), e (n, 3)): S = blockdiag(Omega^-1) + 1/2 (G + G^T), G = R^T H^-1 R.  The table stays resident in the context
        (a snapshot: later pose changes do not touch it) for joint_subsets / joint_pairs; no candidates drop it."""
        a = np.ascontiguousarray(ci, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(cj, dtype=np.int32).reshape(-1)
        z = np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 3)
        w = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 6)
        if not (a.size == b.size == z.shape[0] == w.shape[0]):
            raise ValueError("inconsistent array sizes")
        S, e = np.empty((3 * a.size, 3 * a.size)), np.empty((a.size, 3))
        rc = lib().sgo_candidate_joint(self._h, a.size, _ip(a), _ip(b), _dp(z), _dp(w), _dp(S), _dp(e))
        if rc < 0:
            raise SgoError(f"sgo_candidate_joint: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        self.joint_n = rc
        return S, e

    def joint_subsets(self, subset, chi2_max=None):
        """sgo_joint_subsets: d2 = e_s^T (S_ss)^-1 e_s of the subsets subset (B, n) (non-zero: selected) of the resident table ->
        (npass, d2 (B,), dof (B,), passed (B,) bool); passed = d2 <= chi2_max[b] (chi2_max None: no decisions, npass 0)."""
        m = np.ascontiguousarray(np.asarray(subset) != 0, dtype=np.uint8)
        m = m.reshape(-1, m.shape[-1]) if m.ndim else m.reshape(0, 0)
        B, n = m.shape
        chi = None if chi2_max is None else np.ascontiguousarray(np.broadcast_to(np.asarray(chi2_max, dtype=np.float64), (B,)))
        d2, dof, ok = np.empty(B), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8)
        u8p = C.POINTER(C.c_uint8)
        rc = lib().sgo_joint_subsets(self._h, n, B, m.ctypes.data_as(u8p), None if chi is None else _dp(chi), _dp(d2), _ip(dof), ok.ctypes.data_as(u8p))
        if rc < 0:
            raise SgoError(f"sgo_joint_subsets: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        return rc, d2, dof, ok.astype(bool)

    def joint_pairs(self):
        """sgo_joint_pairs: d2 of every pair {s, t} of the resident table -> (n, n), bitwise symmetric; the diagonal holds the single
        candidates' d2."""
        n = int(getattr(self, "joint_n", 0))
        d2 = np.empty((n, n))
        rc = lib().sgo_joint_pairs(self._h, n, _dp(d2))
        if rc < 0:
            raise SgoError(f"sgo_joint_pairs: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        return d2

    def joint_greedy(self, seeds, chi2_max, max_len: int = JOINT_MAX_SUBSET, allow=None):
        """sgo_joint_greedy: one greedy search per seed (index lists, or a (B, 40) array, -1 padded) on the resident table: from the
        forced seed the candidate with the smallest extension value v_c <= chi2_max[count + 1] is added (ties to the lowest index)
        until none is eligible or max_len are chosen -> (order (B, 40), count (B,), stop (B,), d2_path (B, 41), d2_ext (B, n)).
        allow (B, n): zero excludes a candidate from a seed's growth; chi2_max None: no growth."""
        sd, chi = joint_lists(seeds), _chi2_ladder(chi2_max)
        B, n = sd.shape[0], int(getattr(self, "joint_n", 0))
        al = None if allow is None else np.ascontiguousarray(np.asarray(allow) != 0, dtype=np.uint8).reshape(B, n)
        order, cnt, stop = np.empty((B, JOINT_MAX_SUBSET), dtype=np.int32), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
        path, ext = np.empty((B, JOINT_MAX_SUBSET + 1)), np.empty((B, n))
        rc = lib().sgo_joint_greedy(self._h, n, B, _ip(sd), None if al is None else al.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    None if chi is None else _dp(chi), int(max_len), _ip(order), _ip(cnt), _ip(stop), _dp(path), _dp(ext))
        if rc < 0:
            raise SgoError(f"sgo_joint_greedy: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        return order, cnt, stop, path, ext

    def joint_extend(self, lists):
        """sgo_joint_extend: for every ordered list of candidates of the resident table, d2 of the list and d2 of the list with each
        candidate added -> (d2 (B,), d2_ext (B, n)); members of a list hold its d2 bit for bit."""
        sd = joint_lists(lists)
        B, n = sd.shape[0], int(getattr(self, "joint_n", 0))
        d2, ext = np.empty(B), np.empty((B, n))
        rc = lib().sgo_joint_extend(self._h, n, B, _ip(sd), _dp(d2), _dp(ext))
        if rc < 0:
            raise SgoError(f"sgo_joint_extend: rc={rc}: " + lib().sgo_last_error(self._h).decode())
        return d2, ext

    def marginals(self, vi, vj):
        """sgo_marginals: the 3x3 blocks of H^-1 (rows of vertex vi[t], columns of vertex vj[t]; vertex ids) at the current poses
        -> cov (npairs, 3, 3).  Three solves per distinct free vertex among vj; their number is kept in ``last_marginal_solves``."""
        a = np.ascontiguousarray(vi, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(vj, dtype=np.int32).reshape(-1)
        if a.size != b.size:
            raise ValueError("inconsistent array sizes")
        cov = np.empty((a.size, 3, 3))
        self.last_marginal_solves = self._check(lib().sgo_marginals(self._h, a.size, _ip(a), _ip(b), _dp(cov)), "sgo_marginals")
        return cov

    def pcg_run(self, maxit: int, x_prev=None, bb_ref: float = 0.0, probe_k: int = 0, probe_max: float = 0.0) -> int:
        """sgo_debug_pcg_run: sgo_solve under the per-call fields of an optimize() call; returns the iterations run."""
        xp = None if x_prev is None else np.ascontiguousarray(x_prev, dtype=np.float64).reshape(self.n_free, 3)
        return self._check(lib().sgo_debug_pcg_run(self._h, maxit, None if xp is None else _dp(xp), bb_ref, probe_k, probe_max),
                           "sgo_debug_pcg_run")

    def pcg_array(self, name):
        """One array of the PCG recurrence as stored (sgo_debug_pcg_array; PCG_ARRAYS); None where there is no such array."""
        what, dtype, cols = PCG_ARRAYS[name]
        size = lib().sgo_debug_pcg_array(self._h, what, None, 0)
        if size < 0:
            raise SgoError(f"sgo_debug_pcg_array({name}): rc={size}: " + self.last_error())
        if size == 0:
            return None
        out = np.empty(size // np.dtype(dtype).itemsize, dtype=dtype)
        got = lib().sgo_debug_pcg_array(self._h, what, out.ctypes.data_as(C.c_void_p), out.nbytes)
        if got != size:
            raise SgoError(f"sgo_debug_pcg_array({name}): {got} bytes after {size}: " + self.last_error())
        return out.reshape(-1, cols) if cols else out

    def lanczos(self):
        """(alpha, beta) of every PCG iteration of the last solve (needs env SGO_LANCZOS=1 at set_graph)."""
        buf = np.empty((2048, 2))
        n = self._check(lib().sgo_debug_lanczos(self._h, _dp(buf), 2048), "sgo_debug_lanczos")
        return buf[:n, 0].copy(), buf[:n, 1].copy()

    def last_error(self) -> str:
        """Text of the last error on this context (sgo_last_error)."""
        return lib().sgo_last_error(self._h).decode()

    def mfront_arrays(self, names=tuple(k for k in MFRONT_ARRAYS if k not in ("SEL", "FS_Y", "FS_X"))):
        """The resident multifrontal factorisation's arrays as the last optimize() left them (sgo_debug_mfront_array).  "SEL", the
        selected inverse of the last marginals_selected, and "FS_Y" / "FS_X", the last chunk of the last factor_solve or
        candidate_gate after the forward / backward pass as flat [columns * 3 n] (all empty before the first such call), come
        only when named."""
        return {k: _mfront_fetch(k, lambda what, out, cap: lib().sgo_debug_mfront_array(self._h, what, out, cap), self.last_error)
                for k in names}

    def direct_arrays(self, names=None):
        """The single-launch direct path's tables as the device holds them and what the last optimize() left
        (sgo_debug_direct_array); the snapshots A_*, F_*, D_*, X are empty outside a debug run (SGO_DIRECT_DEBUG set when the graph
        was set).  names=None: all of DIRECT_ARRAYS."""
        names = tuple(DIRECT_ARRAYS) if names is None else names
        return {k: _direct_fetch(k, lambda what, out, cap: lib().sgo_debug_direct_array(self._h, what, out, cap), self.last_error)
                for k in names}

    def solver_description(self) -> str:
        """Which solver sgo_optimize_gn runs for the resident graph (sgo_solver_description)."""
        return lib().sgo_solver_description(self._h).decode()

    # -- profiling
    def kernel_profile(self, quantiles: bool = False):
        """Per-kernel launches / summed ms / algorithmic bytes (sgo_kernel_profile); quantiles=True adds the median, 10th and
        90th percentile of the single-launch durations in microseconds (sgo_kernel_profile_samples)."""
        arr = (KernelStat * 128)()
        n = self._check(lib().sgo_kernel_profile(self._h, arr, 128), "sgo_kernel_profile")
        out = {}
        buf = np.empty(16384, dtype=np.float32) if quantiles else None
        for k in range(min(n, 128)):
            if arr[k].launches:
                d = dict(launches=int(arr[k].launches), ms=arr[k].ms, bytes=arr[k].bytes)
                if quantiles:
                    m = lib().sgo_kernel_profile_samples(self._h, k, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size)
                    if m > 0:
                        q = np.percentile(1e3 * buf[:m].astype(np.float64), [10, 50, 90])
                        d.update(samples=int(m), p10_us=float(q[0]), median_us=float(q[1]), p90_us=float(q[2]))
                out[arr[k].name.decode()] = d
        return out

    def profile_overhead_ms(self):
        return lib().sgo_profile_overhead_ms(self._h)

    def profile_reset(self):
        self._check(lib().sgo_profile_reset(self._h), "sgo_profile_reset")
