// sgo_egroup.cpp -- sgo_edge_groups and sgo_edge_group_rule (include/sgo.h): the leave-group-out test of
// clusters of resident edges on the table sgo_edge_joint keeps in the context (its driver sits with sgo_candidate_joint's in
// sgo_fsolve.cpp, whose columns it shares; kernels in sgo_egroup.hip, the rule in sgo_rules.h).  One call is
//   the member rows to the device -> k_edge_groups, one workgroup per group -> one copy of [B][kEgOut] to the host.
#include <algorithm>
#include <cmath>

#include "sgo_ctx.h"
#include "sgo_mfront_dev.h"
#include "sgo_rules.h"

using namespace sgo;

extern "C" {

int sgo_edge_groups(sgo_ctx* c, int32_t n, int32_t B, const uint8_t* member, const double* chi2_max, double min_pivot, double* d2, int32_t* dof,
                    double* pivot, uint8_t* fail) {
  try {
    int rc = check_graph(c);
    if (rc) return rc;
    sgo_ctx::EdgeJoint& J = c->ejoint;
    if (J.n < 0) {
      c->err = "sgo_edge_groups: no resident table (call sgo_edge_joint; a new or updated graph drops the table)";
      return SGO_EINVAL;
    }
    if (n != J.n) {
      c->err = "sgo_edge_groups: n = " + std::to_string(n) + ", the resident table holds " + std::to_string(J.n) + " edges";
      return SGO_EINVAL;
    }
    if (B < 0 || (B > 0 && (!member || !d2))) {
      c->err = "sgo_edge_groups: null buffer or negative count";
      return SGO_EINVAL;
    }
    if (!(min_pivot > 0.0 && min_pivot <= 1.0)) {
      c->err = "sgo_edge_groups: min_pivot outside (0, 1] (zero would let a cluster whose removal disconnects the graph decide by 0 / 0)";
      return SGO_EINVAL;
    }
    if (chi2_max)
      for (int b = 0; b < B; ++b)
        if (!std::isfinite(chi2_max[b])) {
          c->err = "sgo_edge_groups: chi2_max of group " + std::to_string(b) + " is not finite";
          return SGO_EINVAL;
        }
    int largest = 0;
    for (int b = 0; b < B; ++b) {
      int k = 0;
      for (int t = 0; t < n; ++t) k += member[(size_t)b * n + t] != 0;
      if (k > SGO_JOINT_MAX_SUBSET) {
        c->err = "sgo_edge_groups: group " + std::to_string(b) + " holds " + std::to_string(k) + " edges, more than SGO_JOINT_MAX_SUBSET = " +
                 std::to_string(SGO_JOINT_MAX_SUBSET);
        return SGO_EINVAL;
      }
      largest = std::max(largest, k);
    }
    if (B == 0) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nm = (size_t)B * n, nout = (size_t)kEgOut * B;
    if ((rc = grow_device(c, &J.d_out, &J.out_cap, nout + (size_t)B)) || (rc = grow_device(c, &J.d_mask, &J.mask_cap, nm))) return rc;
    double* d_chi = J.d_out + nout;
    HIP_TRY(c, hipMemcpyAsync(J.d_mask, member, nm, hipMemcpyHostToDevice, c->stream));
    if (chi2_max) HIP_TRY(c, hipMemcpyAsync(d_chi, chi2_max, sizeof(double) * (size_t)B, hipMemcpyHostToDevice, c->stream));
    {
      const double m = 3.0 * largest;
      Scope sc(c, K_EDGE_GROUPS, (double)B * (n + 8.0 * kEgOut + 8.0 * (m * (m + 1) / 2 + 10.0 * largest)));
      launch_edge_groups(c->stream, J.d_tab[J.cur], n, J.d_mask, chi2_max ? d_chi : nullptr, min_pivot, B, std::max(largest, 1), J.d_out);
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<double> res(nout);
    HIP_TRY(c, hipMemcpyAsync(res.data(), J.d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_flush(c);
    int nfail = 0;
    for (int b = 0; b < B; ++b) {
      const double* o = res.data() + (size_t)kEgOut * b;
      d2[b] = o[0];
      if (pivot) pivot[b] = o[1];
      if (dof) dof[b] = (int32_t)o[2];
      if (chi2_max) {
        if (fail) fail[b] = o[3] != 0.0;
        nfail += o[3] != 0.0;
      }
    }
    return nfail;
  } SGO_CATCH(c)
}

int sgo_edge_group_rule(int32_t k, const double* info6, const double* N, const double* e, const double* w, double* d2, double* pivot, int32_t* dof) {
  if (k < 0 || k > SGO_JOINT_MAX_SUBSET || !d2 || !pivot || (k > 0 && (!info6 || !N || !e || !w))) return SGO_EINVAL;
  try {
    std::vector<int> idx;
    int rc = 0;
    for (int t = 0; t < k; ++t) {
      const double* o = info6 + 6 * (size_t)t;
      if (o[0] == 0.0 && o[1] == 0.0 && o[2] == 0.0 && o[3] == 0.0 && o[4] == 0.0 && o[5] == 0.0) {
        rc = 1;   // (a member with all-zero information is left out)
        continue;
      }
      idx.push_back(t);
    }
    const int kk = (int)idx.size();
    std::vector<double> ws(rules::edge_group_ws_doubles(kk) + 1);
    rules::edge_group(kk, idx.data(), N, 3 * (size_t)k, e, w, info6, ws.data(), 0, 0, 1, rules::EdgeGroupNoSync(), d2, pivot);
    if (dof) *dof = 3 * kk;
    if (*pivot != *pivot) rc = 2;   // (an information that is not positive definite, or a non-finite entry)
    return rc;
  } catch (...) {
    return SGO_ENOMEM;
  }
}

}  // extern "C"
