// sgo_selinv.hip -- selected inversion of the multifrontal factor (sgo_marginals_selected, include/sgo.h): every entry of H^-1
// inside the factor's pattern by Takahashi's recurrence, the mirror image of the factorisation of sgo_mfront.hip -- top-down over
// the elimination tree, one launch sequence per level:
//   k_si_gather   Sigma_bb of every front of the level from its parent's selected inverse (every boundary pose of a child is a
//                 local pose of its parent), per 16 x 16 tile by many workgroups, as k_mf_merge in the opposite direction
//   k_si_panels   one workgroup per front: the own columns in panels of 16 from the last to the first.  For panel J and
//                 R = every row of the front after J (the later own rows, then the boundary):
//                     T = L_RJ L_JJ^-1            (YINV holds the rows of L_JJ^-1 of every 16 x 16 diagonal block)
//                     Sigma_RJ = -Sigma_RR T      (Sigma_RR: stored as a lower triangle, read as a full symmetric matrix)
//                     Sigma_JJ = L_JJ^-T L_JJ^-1 - T^T Sigma_RJ
//   k_si_result   the diagonal blocks by vertex id and the blocks of the listed pairs, to one output buffer
// A front's selected inverse has the front's own layout (column-major, leading dimension ld, lower triangle, row m unused) at the
// front's offset in a second arena.  All products run on the fp64 matrix cores (v_mfma_f64_16x16x4_f64: lane (lr, lk) = (lane & 15,
// lane >> 4) holds A[lr][lk] and B[lk][lr] of a step and the results D[lk + 4 q][lr]); operands beyond a tail are MASKED to zero
// on both sides (own3 is a multiple of 3, not of 16), rows beyond a front are clamped and not stored.  No atomics; every sum has
// a fixed order (Sigma_JJ's K range is split over the eight waves in fixed chunks and the partial tiles are added in wave order).
// Bounds: k_si_panels is a chain of barrier-separated steps per panel like k_mf_panels; the product Sigma_RR T dominates
// (nR^2 x 16 multiply-adds per panel, Sigma_RR from L2).  Measurements: NOTES.md section 35.
#include <algorithm>

#include "sgo_device.h"
#include "sgo_internal.h"
#include "sgo_mfront_dev.h"

namespace sgo {
namespace {

__global__ __launch_bounds__(kBlock) void k_si_gather(MfDev M, MfSelDev Z, int t0, int t1) {
  if (M.flags[0]) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  for (int t = t0 + (int)blockIdx.x * kWavesPerBlock + wave; t < t1; t += (int)gridDim.x * kWavesPerBlock) {
    const int2 te = Z.gtile[t];
    const MfFrontDev F = M.fronts[te.x];
    const MfFrontDev Pf = M.fronts[F.parent];
    const int* __restrict__ cm = Z.cmap + Z.cmap_off[te.x];
    const int nb3 = F.m - F.own3;
    const int R0 = 16 * (te.y & 0xffff), col = 16 * (te.y >> 16) + lr;
    if (col >= nb3) continue;
    const double* __restrict__ Sp = Z.S + Pf.off;
    double* __restrict__ Sf = Z.S + F.off;
    const int pc = 3 * cm[col / 3] + col % 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = R0 + lk + 4 * q;
      if (row < nb3 && row >= col) {
        const int pr = 3 * cm[row / 3] + row % 3;
        const int hi = max(pr, pc), lo = min(pr, pc);
        Sf[(size_t)(F.own3 + col) * F.ld + F.own3 + row] = Sp[(size_t)lo * Pf.ld + hi];
      }
    }
  }
}

__global__ __launch_bounds__(kMfThreads) void k_si_panels(MfDev M, MfSelDev Z, int lvl0) {
  extern __shared__ double Tn[];                        // T: column c at Tn + c * ldp, rows relative to the first row after the panel
  __shared__ double part[kMfNW][kMfPanel * kMfPanel];   // the waves' shares of T^T Sigma_RJ
  if (M.flags[0]) return;
  const MfFrontDev F = M.fronts[M.level_front[lvl0 + blockIdx.x]];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int m = F.m, s3 = F.own3, ld = F.ld;
  if (s3 == 0) return;   // a front without own columns only passes its gathered block on
  const double* __restrict__ A = M.arena + F.off;
  double* S = Z.S + F.off;
  const double* __restrict__ Y = M.yinv + 3 * (size_t)F.e0 * kMfPanel;
  const int ldp = (m + 2) | 1;
  for (int k0 = ((s3 - 1) / kMfPanel) * kMfPanel; k0 >= 0; k0 -= kMfPanel) {
    const int wp = min(kMfPanel, s3 - k0), rb = k0 + wp, nR = m - rb;
    const int nrt = (nR + 15) >> 4;
    // 1. T = L_RJ L_JJ^-1 to LDS (columns >= wp come out as zeros: YINV holds zeros right of the diagonal)
    for (int rt = wave; rt < nrt; rt += kMfNW) {
      const int r = rb + 16 * rt + lr;
      const bool rv = r < m;
      mf_d4 acc = {0.0, 0.0, 0.0, 0.0};
      double av[4], bv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = lk + 4 * s;
        const bool kv = k < wp;
        av[s] = (kv && rv) ? A[(size_t)(k0 + k) * ld + r] : 0.0;
        bv[s] = kv ? Y[(size_t)(k0 + k) * kMfPanel + lr] : 0.0;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * rt + lk + 4 * q;
        if (row < nR) Tn[lr * ldp + row] = acc[q];
      }
    }
    __syncthreads();
    // 2. Sigma_RJ = -Sigma_RR T, straight to the front's selected inverse (columns J: nothing this step reads)
    for (int rt = wave; rt < nrt; rt += kMfNW) {
      const int r = rb + min(16 * rt + lr, nR - 1);
      mf_d4 acc = {0.0, 0.0, 0.0, 0.0};
      for (int kk = 0; kk < nR; kk += 16) {
        double av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = kk + 4 * u + lk;
          const bool kv = k < nR;
          const int kc = min(k, nR - 1), c = rb + kc;
          const int hi = max(r, c), lo = min(r, c);
          av[u] = kv ? S[(size_t)lo * ld + hi] : 0.0;
          bv[u] = kv ? Tn[lr * ldp + kc] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * rt + lk + 4 * q;
        if (row < nR && lr < wp) S[(size_t)(k0 + lr) * ld + rb + row] = -acc[q];
      }
    }
    __syncthreads();
    // 3. Sigma_JJ = Y^T Y - T^T Sigma_RJ: the K range in eight fixed shares, one per wave, added in wave order
    {
      const int steps = (nR + 3) >> 2, per = (steps + kMfNW - 1) / kMfNW;
      const int st1 = min(steps, (wave + 1) * per);
      mf_d4 acc = {0.0, 0.0, 0.0, 0.0};
      const int cj = k0 + min(lr, wp - 1);
      for (int st = wave * per; st < st1; ++st) {
        const int k = 4 * st + lk;
        const bool kv = k < nR;
        const int kc = min(k, nR - 1);
        const double a = kv ? Tn[lr * ldp + kc] : 0.0;
        const double b = (kv && lr < wp) ? S[(size_t)cj * ld + rb + kc] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) part[wave][(lk + 4 * q) * kMfPanel + lr] = acc[q];
    }
    __syncthreads();
    if (wave == 0) {
      mf_d4 yy = {0.0, 0.0, 0.0, 0.0};
      double yv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = lk + 4 * s;
        yv[s] = k < wp ? Y[(size_t)(k0 + k) * kMfPanel + lr] : 0.0;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) yy = __builtin_amdgcn_mfma_f64_16x16x4f64(yv[s], yv[s], yy, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = lk + 4 * q;
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < kMfNW; ++w) sum += part[w][i * kMfPanel + lr];
        if (i < wp && lr <= i) S[(size_t)(k0 + lr) * ld + k0 + i] = yy[q] - sum;
      }
    }
    __syncthreads();   // (the next panel overwrites T and reads this one's columns as part of its Sigma_RR)
  }
}

__global__ __launch_bounds__(kBlock) void k_si_result(MfDev M, MfSelDev Z, int V, int npairs, const int4* __restrict__ pairs,
                                                      double* __restrict__ out) {
  const long long nd = 9LL * M.n, tot = nd + 9LL * npairs;
  if (blockIdx.x == 0 && threadIdx.x == 0) out[9 * ((size_t)V + (size_t)npairs)] = (double)M.flags[0];
  if (M.flags[0]) return;
  for (long long idx = (long long)blockIdx.x * kBlock + threadIdx.x; idx < tot; idx += (long long)gridDim.x * kBlock) {
    if (idx < nd) {
      const int p = (int)(idx / 9), e = (int)(idx % 9), a = e / 3, b = e % 3;
      const MfFrontDev F = M.fronts[Z.pos_front[p]];
      const int l = 3 * (p - F.e0), hi = max(a, b), lo = min(a, b);
      out[9 * (size_t)M.elim_vertex[p] + e] = Z.S[F.off + (size_t)(l + lo) * F.ld + l + hi];
    } else {
      const long long t = (idx - nd) / 9;
      const int e = (int)((idx - nd) % 9);
      const int4 pr = pairs[t];
      if (pr.x < 0) continue;
      const MfFrontDev F = M.fronts[pr.x];
      int a = e / 3, b = e % 3;   // the stored block B[a][b] = S[3 lc + b][3 lr + a] (row pose lr >= column pose lc)
      if (pr.w) {
        const int s = a;
        a = b;
        b = s;
      }
      int row = 3 * pr.y + a, col = 3 * pr.z + b;
      if (row < col) {   // (a diagonal block: the other triangle is the mirror)
        const int s = row;
        row = col;
        col = s;
      }
      out[9 * (size_t)V + (size_t)(idx - nd)] = Z.S[F.off + (size_t)col * F.ld + row];
    }
  }
}

}  // namespace

void launch_si_gather(hipStream_t s, const MfDev& M, const MfSelDev& Z, int t0, int t1) {
  const int grid = std::max(1, std::min((t1 - t0 + kWavesPerBlock - 1) / kWavesPerBlock, 8192));
  SGO_LAUNCH(k_si_gather, dim3(grid), dim3(kBlock), 0, s, M, Z, t0, t1);
}
void launch_si_panels(hipStream_t s, const MfDev& M, const MfSelDev& Z, int lvl0, int count, size_t lds) {
  SGO_LAUNCH(k_si_panels, dim3(count), dim3(kMfThreads), lds, s, M, Z, lvl0);
}
void launch_si_result(hipStream_t s, const MfDev& M, const MfSelDev& Z, int V, int npairs, const int4* pairs, double* out) {
  const long long tot = 9LL * M.n + 9LL * npairs;
  const int grid = (int)std::max<long long>(1, std::min<long long>((tot + kBlock - 1) / kBlock, 4096));
  SGO_LAUNCH(k_si_result, dim3(grid), dim3(kBlock), 0, s, M, Z, V, npairs, pairs, out);
}
bool si_prepare_device() {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_si_panels), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)sizeof(double) * kMfPanel * ((kMfMaxDim + 2) | 1)) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

}  // namespace sgo
