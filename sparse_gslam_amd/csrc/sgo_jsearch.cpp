// sgo_jsearch.cpp -- sgo_joint_greedy, sgo_joint_extend and sgo_joint_greedy_rule (include/sgo.h): the greedy
// search for a large jointly compatible candidate set on the resident table of sgo_candidate_joint (kernel in sgo_jsearch.hip, the
// 3 x 3 pieces in sgo_rules.h).  One call is
//   the seeds, the allow rows and the thresholds to the device -> k_joint_grow, one launch per slice of at most kJointGrowSlabs
//   seeds (every workgroup of a slice has its own slab of W in the context's grow-on-demand scratch) -> one copy back of order,
//   count, stop, d2_path and d2_ext.
// The calls read the table and write scratch of their own: no graph structure, no pose, no plan.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sgo_ctx.h"
#include "sgo_mfront_dev.h"

using namespace sgo;

namespace {

// What the search refuses in its lists and thresholds, the device's entry points and the host rule alike.  len[b]: seed b's length.
// max_len < 0: the longest list (sgo_joint_extend).
bool search_check(const char* name, int n, int B, const int32_t* seed, const double* chi2, int32_t* max_len, std::vector<int>* len, std::string* err) {
  len->assign((size_t)B, 0);
  int longest = 0;
  std::vector<uint8_t> seen((size_t)n);
  for (int b = 0; b < B; ++b) {
    const int32_t* s = seed + (size_t)b * SGO_JOINT_MAX_SUBSET;
    std::fill(seen.begin(), seen.end(), 0);
    int k = 0;
    while (k < SGO_JOINT_MAX_SUBSET && s[k] != -1) ++k;
    for (int t = 0; t < SGO_JOINT_MAX_SUBSET; ++t) {
      if (t >= k) {
        if (s[t] != -1) {
          *err = std::string(name) + ": list " + std::to_string(b) + " has an entry after a -1";
          return false;
        }
        continue;
      }
      if (s[t] < 0 || s[t] >= n) {
        *err = std::string(name) + ": list " + std::to_string(b) + " names candidate " + std::to_string(s[t]) + " outside [0, " + std::to_string(n) + ")";
        return false;
      }
      if (seen[(size_t)s[t]]) {
        *err = std::string(name) + ": list " + std::to_string(b) + " names candidate " + std::to_string(s[t]) + " twice";
        return false;
      }
      seen[(size_t)s[t]] = 1;
    }
    (*len)[(size_t)b] = k;
    longest = std::max(longest, k);
  }
  if (*max_len < 0) *max_len = longest;
  if (*max_len < longest || *max_len > SGO_JOINT_MAX_SUBSET) {
    *err = std::string(name) + ": max_len = " + std::to_string(*max_len) + " outside [" + std::to_string(longest) + " (the longest seed), SGO_JOINT_MAX_SUBSET = " +
           std::to_string(SGO_JOINT_MAX_SUBSET) + "]";
    return false;
  }
  for (int k = 1; chi2 && k <= SGO_JOINT_MAX_SUBSET; ++k)
    if (!std::isfinite(chi2[k])) {
      *err = std::string(name) + ": chi2_max[" + std::to_string(k) + "] is not finite";
      return false;
    }
  return true;
}

// Both entry points behind their own argument checks.  Outputs may be null.
int search_run(sgo_ctx* c, const char* name, int n, int B, const int32_t* seed, const uint8_t* allow, const double* chi2, int32_t max_len, int32_t* order,
               int32_t* count, int32_t* stop, double* d2_path, double* d2_ext, double* d2_last) {
  std::vector<int> len;
  if (!search_check(name, n, B, seed, chi2, &max_len, &len, &c->err)) return SGO_EINVAL;
  if (B == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  sgo_ctx::Joint& J = c->joint;
  constexpr size_t kS = SGO_JOINT_MAX_SUBSET, kP = SGO_JOINT_MAX_SUBSET + 1;
  const size_t nB = (size_t)B, slab = joint_grow_slab_doubles(n, max_len);
  const int slice = joint_grow_slice(n, max_len, B);
  const size_t ndbl = kP + nB * kP + nB * n, nint = nB * kS * 2 + 2 * nB;
  int rc;
  if ((rc = grow_device(c, &J.d_grow, &J.grow_cap, slab * (size_t)slice, false)) || (rc = grow_device(c, &J.d_gout, &J.gout_cap, ndbl)) ||
      (rc = grow_device(c, &J.d_gint, &J.gint_cap, nint)) || (allow && (rc = grow_device(c, &J.d_mask, &J.mask_cap, nB * n))))
    return rc;
  JointGrowDev A;
  A.table = J.d_tab[J.cur];
  A.n = n;
  A.max_len = max_len;
  A.seed = J.d_gint;
  A.allow = allow ? J.d_mask : nullptr;
  A.chi2 = chi2 ? J.d_gout : nullptr;
  A.slabs = J.d_grow;
  A.slab = slab;
  A.order = J.d_gint + nB * kS;
  A.count = A.order + nB * kS;
  A.stop = A.count + nB;
  A.d2_path = J.d_gout + kP;
  A.d2_ext = A.d2_path + nB * kP;
  HIP_TRY(c, hipMemcpyAsync(J.d_gint, seed, sizeof(int32_t) * nB * kS, hipMemcpyHostToDevice, c->stream));
  if (allow) HIP_TRY(c, hipMemcpyAsync(J.d_mask, allow, nB * n, hipMemcpyHostToDevice, c->stream));
  if (chi2) HIP_TRY(c, hipMemcpyAsync(J.d_gout, chi2, sizeof(double) * kP, hipMemcpyHostToDevice, c->stream));
  for (int b0 = 0; b0 < B; b0 += slice) {
    const int nb = std::min(slice, B - b0);
    A.b0 = b0;
    Scope sc(c, K_JOINT_GROW, (double)nb * (8.0 * 12 * n + 8.0 * 4.5 * (double)max_len * max_len * 3 * n));
    launch_joint_grow(c->stream, A, nb);
  }
  HIP_TRY(c, hipGetLastError());
  std::vector<int32_t> ri(nB * kS + 2 * nB);
  std::vector<double> rd(nB * kP + nB * n);
  HIP_TRY(c, hipMemcpyAsync(ri.data(), A.order, sizeof(int32_t) * ri.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(rd.data(), A.d2_path, sizeof(double) * rd.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_flush(c);
  const int32_t* cnt = ri.data() + nB * kS;
  if (order) std::copy(ri.begin(), ri.begin() + (ptrdiff_t)(nB * kS), order);
  if (count) std::copy(cnt, cnt + nB, count);
  if (stop) std::copy(cnt + nB, cnt + 2 * nB, stop);
  if (d2_path) std::copy(rd.begin(), rd.begin() + (ptrdiff_t)(nB * kP), d2_path);
  if (d2_ext) std::copy(rd.begin() + (ptrdiff_t)(nB * kP), rd.end(), d2_ext);
  // (sgo_joint_extend) d2 of the whole list; NaN for a list whose pivot block was not positive definite
  for (size_t b = 0; d2_last && b < nB; ++b) d2_last[b] = cnt[b] == len[b] ? rd[b * kP + (size_t)cnt[b]] : std::nan("");
  return B;
}

}  // namespace

extern "C" {

int sgo_joint_greedy(sgo_ctx* c, int32_t n, int32_t B, const int32_t* seed, const uint8_t* allow, const double* chi2_max, int32_t max_len, int32_t* order,
                     int32_t* count, int32_t* stop, double* d2_path, double* d2_ext) {
  try {
    const int rc = joint_table_check(c, "sgo_joint_greedy", n);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!seed || !order || !count))) {
      c->err = "sgo_joint_greedy: null buffer or negative count";
      return SGO_EINVAL;
    }
    if (max_len < 0) {
      c->err = "sgo_joint_greedy: max_len = " + std::to_string(max_len) + " is negative";
      return SGO_EINVAL;
    }
    return search_run(c, "sgo_joint_greedy", n, B, seed, allow, chi2_max, max_len, order, count, stop, d2_path, d2_ext, nullptr);
  } SGO_CATCH(c)
}

int sgo_joint_extend(sgo_ctx* c, int32_t n, int32_t B, const int32_t* lists, double* d2, double* d2_ext) {
  try {
    const int rc = joint_table_check(c, "sgo_joint_extend", n);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!lists || !d2 || !d2_ext))) {
      c->err = "sgo_joint_extend: null buffer or negative count";
      return SGO_EINVAL;
    }
    return search_run(c, "sgo_joint_extend", n, B, lists, nullptr, nullptr, -1, nullptr, nullptr, nullptr, nullptr, d2_ext, d2);
  } SGO_CATCH(c)
}

// The search of ONE seed on the host, step for step what a workgroup of k_joint_grow does, through the same rules.
int sgo_joint_greedy_rule(int32_t n, const double* S, const double* e, const int32_t* seed, const uint8_t* allow, const double* chi2_max, int32_t max_len,
                          int32_t* order, int32_t* count, int32_t* stop, double* d2_path, double* d2_ext) {
  try {
    if (n < 1 || n > SGO_JOINT_MAX_CANDIDATES || !S || !e || !seed || !order || !count || max_len < 0) return SGO_EINVAL;
    std::vector<int> len;
    std::string err;
    if (!search_check("sgo_joint_greedy_rule", n, 1, seed, chi2_max, &max_len, &len, &err)) return SGO_EINVAL;
    const size_t ld = 3 * (size_t)n;
    std::vector<double> W(joint_grow_slab_doubles(n, max_len)), C6(6 * (size_t)n), q(3 * (size_t)n), Wp(9 * (size_t)SGO_JOINT_MAX_SUBSET);
    std::vector<uint8_t> pivot((size_t)n, 0);
    for (int c = 0; c < n; ++c) {
      const double* r = S + 3 * (size_t)c * ld + 3 * (size_t)c;
      const double blk[6] = {r[0], r[ld], r[ld + 1], r[2 * ld], r[2 * ld + 1], r[2 * ld + 2]};
      std::copy(blk, blk + 6, &C6[6 * (size_t)c]);
      std::copy(e + 3 * c, e + 3 * c + 3, &q[3 * (size_t)c]);
    }
    const double nan = std::nan("");
    double d2 = 0.0;
    int k = 0, why = SGO_JSTOP_MAX_LEN;
    std::vector<double> path((size_t)SGO_JOINT_MAX_SUBSET + 1, nan);
    std::fill(order, order + SGO_JOINT_MAX_SUBSET, -1);
    path[0] = 0.0;
    for (; k < max_len; ++k) {
      const int m = 3 * k;
      int p = seed[k];
      if (p < 0) {
        double v = 0.0;
        for (int c = 0; c < n && chi2_max; ++c) {
          if (pivot[(size_t)c] || (allow && !allow[c])) continue;
          const double t = rules::jgrow_value(d2, &C6[6 * (size_t)c], &q[3 * (size_t)c]);
          if (t - t == 0.0 && t <= chi2_max[k + 1] && (p < 0 || rules::jgrow_better(t, c, v, p))) {
            v = t;
            p = c;
          }
        }
        if (p < 0) {
          why = SGO_JSTOP_NONE;
          break;
        }
      }
      double G6[6], zp[3];
      if (!rules::jgrow_chol3(&C6[6 * (size_t)p], G6)) {
        why = SGO_JSTOP_NOT_PD;
        break;
      }
      rules::jgrow_solve3(G6, q[3 * (size_t)p], q[3 * (size_t)p + 1], q[3 * (size_t)p + 2], zp);
      for (int r = 0; r < m; ++r)
        for (int a = 0; a < 3; ++a) Wp[3 * (size_t)r + a] = W[(size_t)r * ld + 3 * (size_t)p + a];
      pivot[(size_t)p] = 1;
      for (int c = 0; c < n; ++c)
        if (!pivot[(size_t)c])
          rules::jgrow_update(G6, zp, S + 3 * (size_t)p * ld + 3 * (size_t)c, ld, Wp.data(), 3, W.data() + 3 * (size_t)c, ld, m, &C6[6 * (size_t)c], &q[3 * (size_t)c]);
      d2 += (zp[0] * zp[0] + zp[1] * zp[1]) + zp[2] * zp[2];
      order[k] = p;
      path[(size_t)k + 1] = d2;
    }
    *count = k;
    if (stop) *stop = why;
    if (d2_path) std::copy(path.begin(), path.end(), d2_path);
    for (int c = 0; d2_ext && c < n; ++c)
      d2_ext[c] = why == SGO_JSTOP_NOT_PD ? nan : pivot[(size_t)c] ? d2 : rules::jgrow_value(d2, &C6[6 * (size_t)c], &q[3 * (size_t)c]);
    return 1;
  } catch (...) {
    return SGO_ENOMEM;
  }
}

}  // extern "C"
