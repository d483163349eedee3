// sgo_rules.h -- the decisions sgo_optimize_gn takes about its multigrid hierarchy, as PURE functions of iteration counts and of
// sums every rank holds bit-identically: no clocks, no device state, no environment.  Every rank of a multi-GPU run must take the
// same decision from the same numbers, so the rules live here, apart from the driver that feeds them (CallPolicy, sgo_policy.h,
// driven by optimize_gn, sgo_solve.cpp), and are unit-tested with that policy on recorded count sequences without a GPU
// (tests/cpp/rules_unit.cpp, tests/test_rules.py).  The floor rule at
// the end (single GPU: whether a solve that stopped short of pcg_tol is accepted) is tested against numpy the same way
// (tests/cpp/floor_shim.cpp, tests/test_floor_rule.py).
// DESIGN.md section 5 says what each rule is for and where its constants were measured.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <initializer_list>

// A rule the kernels compile too carries SGO_RULE_HD: the compiler's own attributes under a HIP compilation, nothing for a host
// compiler -- no HIP header either way.
#if defined(__HIP__)
#define SGO_RULE_HD __attribute__((host)) __attribute__((device))
#else
#define SGO_RULE_HD
#endif

namespace sgo {
namespace rules {

// The gain rule of sgo_optimize_gn_until (g2o's SparseOptimizerTerminateAction): with `last` and `cur` the
// robust chi2 at the start of the previous and of this iteration, the call stops before this iteration iff the relative gain
// (last - cur) / cur is in [0, gain_tol).  A negative gain does not stop (DCS makes chi2 non-monotone), gain_tol <= 0 never does,
// and cur == 0 or a non-finite argument gives NaN or inf, for which both comparisons are false.  The caller applies it from the
// third iteration on (gain_stop_applies).  `double` and comparisons only: the host, k_direct and k_mf_gain_stop compile this text.
SGO_RULE_HD inline bool gain_stop(double last, double cur, double gain_tol) {
  const double gain = (last - cur) / cur;
  return gain >= 0.0 && gain < gain_tol;
}
// ... and the iterations before which it is asked: at least two updates always run, and the closing pass decides nothing.
SGO_RULE_HD inline bool gain_stop_applies(int it, int max_iters) { return it >= 2 && it < max_iters; }

// One trial of sgo_optimize_lm (g2o 2020.5.29's OptimizationAlgorithmLevenberg::solve).  cur: the robust chi2
// at the accepted poses; trial: at the trial poses; scale = x . (lambda x + b) + 1e-3; solve_ok == 0: the factorisation or the
// substitution failed, which g2o scores as trial = DBL_MAX over scale = 1e-3.  With rho = (cur - trial) / scale the trial is accepted
// iff rho > 0, the trial chi2 is finite and the solve succeeded: lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), nu = 2.  Otherwise
// lambda *= nu, nu *= 2.  Returns kLmAccept, or what the rejection means for the iteration: kLmRetry (rho < 0: another trial while
// fewer than kLmMaxTrials have run), kLmZeroGain (rho == 0: the iteration ends and the call terminates) or kLmEnd (rho is NaN, or
// positive with a non-finite trial: the iteration ends).  `double` and comparisons only: the host and k_lm_decide compile this text.
constexpr int kLmMaxTrials = 10;
constexpr int kLmRetry = 0, kLmAccept = 1, kLmZeroGain = 2, kLmEnd = 3;
SGO_RULE_HD inline int lm_trial(double cur, double trial, double scale, int solve_ok, double* lambda, double* nu) {
  if (!solve_ok) {
    trial = 1.7976931348623157e308;
    scale = 1e-3;
  }
  const double rho = (cur - trial) / scale;
  if (rho > 0.0 && trial - trial == 0.0 && solve_ok) {   // (x - x == 0: x is finite)
    const double t = 2.0 * rho - 1.0;
    double alpha = 1.0 - t * t * t;
    if (!(alpha < 2.0 / 3.0)) alpha = 2.0 / 3.0;
    *lambda *= alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0;
    *nu = 2.0;
    return kLmAccept;
  }
  *lambda *= *nu;
  *nu *= 2.0;
  return rho < 0.0 ? kLmRetry : (rho == 0.0 ? kLmZeroGain : kLmEnd);
}

// The step of one trial of sgo_optimize_dogleg (g2o 2020.5.29's OptimizationAlgorithmDogleg::solve).  With b
// the right-hand side and g the Gauss-Newton step of H g = b, forms = {b.b, b.g, g.g, b.Hb, b.Hg, g.Hg}; the Cauchy step is
// alpha b with alpha = b.b / b.Hb.  Every step is h = a b + c g:
//   kDlGn  |g| < delta:            h = g                                  (a = 0, c = 1: the caller copies g)
//   kDlSd  else |alpha b| > delta: h = (delta / |alpha b|) alpha b
//   kDlDl  else:                   h = alpha b + beta (g - alpha b), with d = g - alpha b, k = alpha b . d, s2 = |alpha b|^2,
//                                  D = sqrt(k^2 + |d|^2 (delta^2 - s2)), beta = (-k + D) / |d|^2 if k <= 0, else (delta^2 - s2) / (k + D)
// step_norm = |h| and the linear gain L = -h.Hh + 2 b.h follow from the six forms; |L| < 1e-12 gives L = 1e-12.  `double`,
// comparisons and sqrt only: the host (sgo_dogleg_step_rule) and k_dl_trial compile this text.
constexpr int kDlMaxTrials = 100;
constexpr int kDlGn = 0, kDlSd = 1, kDlDl = 2;
constexpr double kDlDeltaInit = 1e4, kDlLambdaInit = 1e-7, kDlLambdaFactor = 10.0, kDlLambdaMin = 1e-12, kDlLambdaMax = 1e3;
SGO_RULE_HD inline int dogleg_step(double delta, const double* forms, double* a, double* c, double* step_norm, double* linear_gain) {
  const double bb = forms[0], bg = forms[1], gg = forms[2], bHb = forms[3], bHg = forms[4], gHg = forms[5];
  const double alpha = bb / bHb;
  const double gn_norm = std::sqrt(gg), s2 = alpha * alpha * bb, sd_norm = std::sqrt(s2);
  int kind;
  double ca, cc;
  if (gn_norm < delta) {
    kind = kDlGn;
    ca = 0.0;
    cc = 1.0;
  } else if (sd_norm > delta) {
    kind = kDlSd;
    ca = (delta / sd_norm) * alpha;
    cc = 0.0;
  } else {
    kind = kDlDl;
    const double k = alpha * bg - s2;                         // alpha b . (g - alpha b)
    const double d2 = (gg - 2.0 * alpha * bg) + s2;           // |g - alpha b|^2
    const double gap = delta * delta - s2;
    const double D = std::sqrt(k * k + d2 * gap);
    const double beta = k <= 0.0 ? (-k + D) / d2 : gap / (k + D);
    ca = alpha * (1.0 - beta);
    cc = beta;
  }
  *a = ca;
  *c = cc;
  *step_norm = std::sqrt((ca * ca * bb + 2.0 * ca * cc * bg) + cc * cc * gg);
  double L = -((ca * ca * bHb + 2.0 * ca * cc * bHg) + cc * cc * gHg) + 2.0 * (ca * bb + cc * bg);
  if (L < 1e-12 && L > -1e-12) L = 1e-12;
  *linear_gain = L;
  return kind;
}

// ... and its decision.  cur: the robust chi2 at the accepted poses; trial: at the trial poses.  rho = (cur - trial) / L; the trial
// is accepted iff rho > 0 and the trial chi2 is finite; rho > 0.75: delta = max(delta, 3 |h|); rho < 0.25: delta *= 0.5.  A trial
// chi2 or a rho that is not finite counts as rho = -inf -- rejected, delta halved -- where g2o would repeat the identical trial.
// Returns 1: accepted, 0: rejected.  The host (sgo_dogleg_trial_rule) and k_dl_decide compile this text.
SGO_RULE_HD inline int dogleg_trial(double cur, double trial, double linear_gain, double step_norm, double* delta) {
  if (linear_gain < 1e-12 && linear_gain > -1e-12) linear_gain = 1e-12;
  const double rho = (cur - trial) / linear_gain;
  if (!(trial - trial == 0.0) || !(rho - rho == 0.0)) {   // (x - x == 0: x is finite)
    *delta *= 0.5;
    return 0;
  }
  if (rho > 0.75) {
    const double wide = 3.0 * step_norm;
    if (wide > *delta) *delta = wide;
  } else if (rho < 0.25) {
    *delta *= 0.5;
  }
  return rho > 0.0 ? 1 : 0;
}

// The leave-one-out rule of sgo_edge_leave_one_out: what sgo_candidate_gate would say about a resident edge
// had it never been inserted, from the edge's own quantities alone.  info: Omega's upper triangle by rows; P = J Sigma J^T at the
// current poses WITH the edge in H (row-major, symmetric); e its error; w its kernel weight.  With Omega = G G^T (lower Cholesky),
// N = G^T P G = V diag(nu) V^T, c = V^T G^T e:
//   redundancy = 1 - w nu_max                       (lambda_min of I - w N: 0 for a bridge, whose test is 0 / 0)
//   d2         = sum_q c_q^2 / ((1 + (1 - w) nu_q) (1 - w nu_q))
//   cov_loo    = G^-T V diag(nu_q / (1 - w nu_q)) V^T G^-1    (exactly symmetric: one triangle is computed and mirrored)
// Everything goes through G and N, never through a factor of w Omega: w reaches 4e-9 under DCS.  Returns 0; 1 for an all-zero Omega
// (a deactivated edge: d2 = 0, redundancy = 1, cov_loo = P); 2 for an Omega that is not positive definite (NaN everywhere).  The
// caller decides what a small redundancy means.  cov_loo may be null.  `double` and comparisons only: the host and k_loo_edges
// compile this text.
// jacobi3: a symmetric 3 x 3 matrix (a: overwritten by the rotated matrix; its diagonal ends as the eigenvalues) by kJacobiSweeps
// cyclic sweeps; V's COLUMNS are the eigenvectors.  A fixed count, not a convergence test: after five sweeps a 3 x 3 matrix is
// diagonal to rounding (the convergence is quadratic), and an exactly zero entry is not rotated.
constexpr int kJacobiSweeps = 8;
template <int p, int q>
SGO_RULE_HD inline void jacobi3_rotate(double (&a)[3][3], double (&V)[3][3]) {
  const double apq = a[p][q];
  if (apq == 0.0) return;
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  const double at = theta < 0.0 ? -theta : theta;
  double t = 1.0 / (at + sqrt(theta * theta + 1.0));   // (a huge theta: t = 0, the entry is negligible already)
  if (theta < 0.0) t = -t;
  const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
  a[p][p] -= t * apq;
  a[q][q] += t * apq;
  a[p][q] = a[q][p] = 0.0;
  constexpr int r = 3 - p - q;   // the third index
  const double arp = a[r][p], arq = a[r][q];
  a[r][p] = a[p][r] = cs * arp - sn * arq;
  a[r][q] = a[q][r] = sn * arp + cs * arq;
  for (int k = 0; k < 3; ++k) {
    const double vkp = V[k][p], vkq = V[k][q];
    V[k][p] = cs * vkp - sn * vkq;
    V[k][q] = sn * vkp + cs * vkq;
  }
}
SGO_RULE_HD inline void jacobi3(double (&a)[3][3], double (&V)[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi3_rotate<0, 1>(a, V);
    jacobi3_rotate<0, 2>(a, V);
    jacobi3_rotate<1, 2>(a, V);
  }
}
SGO_RULE_HD inline int edge_loo(const double* info, const double* P, const double* e, double w, double* d2, double* redundancy, double* cov_loo) {
  const double o00 = info[0], o01 = info[1], o02 = info[2], o11 = info[3], o12 = info[4], o22 = info[5];
  if (o00 == 0.0 && o01 == 0.0 && o02 == 0.0 && o11 == 0.0 && o12 == 0.0 && o22 == 0.0) {
    *d2 = 0.0;
    *redundancy = 1.0;
    if (cov_loo)
      for (int q = 0; q < 9; ++q) cov_loo[q] = P[q];
    return 1;
  }
  // Omega = G G^T
  const double g00 = sqrt(o00), g10 = o01 / g00, g20 = o02 / g00;
  const double t11 = o11 - g10 * g10, g11 = sqrt(t11), g21 = (o12 - g20 * g10) / g11;
  const double t22 = o22 - g20 * g20 - g21 * g21, g22 = sqrt(t22);
  if (!(o00 > 0.0) || !(t11 > 0.0) || !(t22 > 0.0) || !(g22 - g22 == 0.0)) {   // (the last: a non-finite entry)
    const double nan = sqrt(-1.0);
    *d2 = nan;
    *redundancy = nan;
    if (cov_loo)
      for (int q = 0; q < 9; ++q) cov_loo[q] = nan;
    return 2;
  }
  const double G[3][3] = {{g00, 0.0, 0.0}, {g10, g11, 0.0}, {g20, g21, g22}};
  // N = G^T Ps G with Ps = (P + P^T) / 2
  double Ps[3][3], PG[3][3], N[3][3], V[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) Ps[a][b] = 0.5 * (P[3 * a + b] + P[3 * b + a]);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) PG[a][b] = Ps[a][0] * G[0][b] + Ps[a][1] * G[1][b] + Ps[a][2] * G[2][b];
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) N[a][b] = N[b][a] = G[0][a] * PG[0][b] + G[1][a] * PG[1][b] + G[2][a] * PG[2][b];
  jacobi3(N, V);
  const double nu[3] = {N[0][0], N[1][1], N[2][2]};
  const double u[3] = {g00 * e[0] + g10 * e[1] + g20 * e[2], g11 * e[1] + g21 * e[2], g22 * e[2]};
  double numax = nu[0] > nu[1] ? nu[0] : nu[1];
  if (nu[2] > numax) numax = nu[2];
  *redundancy = 1.0 - w * numax;
  double sum = 0.0, s[3];
  for (int q = 0; q < 3; ++q) {
    const double c = V[0][q] * u[0] + V[1][q] * u[1] + V[2][q] * u[2];
    const double r = 1.0 - w * nu[q];
    sum += c * c / ((1.0 + (1.0 - w) * nu[q]) * r);
    s[q] = nu[q] / r;
  }
  *d2 = sum;
  if (cov_loo) {
    // Y = G^-T V (column q: back substitution with G^T), cov_loo = Y diag(s) Y^T
    double Y[3][3];
    for (int q = 0; q < 3; ++q) {
      Y[2][q] = V[2][q] / g22;
      Y[1][q] = (V[1][q] - g21 * Y[2][q]) / g11;
      Y[0][q] = (V[0][q] - g10 * Y[1][q] - g20 * Y[2][q]) / g00;
    }
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) {
        const double v = Y[a][0] * s[0] * Y[b][0] + Y[a][1] * s[1] * Y[b][1] + Y[a][2] * s[2] * Y[b][2];
        cov_loo[3 * a + b] = cov_loo[3 * b + a] = v;
      }
  }
  return 0;
}

// The pair rule of sgo_closure_search: how far, in the metric of the graph's own uncertainty, the query pose c
// is from lying within `radius` of the listed pose j, and how wide a matcher's window must be.  xj, xc: the poses (x, y, theta); Sjj,
// Sjc, Scc: the blocks of Sigma = H^-1 (row-major; Sjc has the rows of j); free_j / free_c == false: that pose is FIXED and drops
// out with its cross block (its blocks are not read).
//   rel     = (t, phi), t = R(theta_j)^T (p_c - p_j), phi = normalize(theta_c - theta_j): c in j's frame, EdgeSE2's prediction j -> c
//   A, B    = d rel / d x_j, d rel / d x_c: the Jacobians of an EdgeSE2 j -> c as edge_jacobians (sgo_device.h) forms them with
//             sz = 0, cz = 1 (P is the covariance of rel in j's frame; an edge whose measurement is rel has R(-phi) P R(-phi)^T, the
//             same m2 and sigma).  The products with 1 and 0 are exact, so the entries are written out:
//             A = [-R^T | (t_y, -t_x)^T; 0 0 -1], B = [R^T 0; 0 0 1]
//   cov_rel = P = 1/2 (Q + Q^T), Q = A Sjj A^T + A Sjc B^T + B Sjc^T A^T + B Scc B^T   (one triangle computed and mirrored)
//   m2      = max(0, |t| - radius)^2 / (u^T P_tt u), u = t / |t|: the squared Mahalanobis distance from t to the half-plane
//             {y : u^T y <= radius}, which contains the disc |y| <= radius (u^T y <= |y|), so m2 never exceeds the distance to the
//             disc; 1 degree of freedom.  A zero excess gives 0 whatever the denominator; a positive excess over a denominator that
//             is not above zero gives +inf (a NaN denominator gives NaN)
//   sigma   = (sqrt(lambda_max(P_tt)), sqrt(P_phiphi)): the 1-sigma half-widths of the matcher's window in j's frame
// Returns 0.  `double`, comparisons, sqrt, floor, sin and cos only: the host (sgo_closure_search_rule) and k_closure_search compile this text.
// closure_norm_theta: g2o::normalize_theta, as norm_theta of sgo_device.h.  One text is not yet one result: a compiler that contracts
// t - m 2 pi into an FMA (hipcc does for the device) rounds once where the host rounds twice, and the two part wherever m 2 pi
// is inexact (from |m| = 11 on).  So contraction is off in this body under clang, which compiles every device pass and the library's host pass;
// the host builds of the tests (g++, x86-64 baseline: no FMA to contract into) round twice as written, and a host build for an
// FMA target with another compiler needs -ffp-contract=off to keep that.  tests/test_wrap_cases.py holds the host statements to
// each other's bits and tests/test_gpu_wrap_points.py the device to the host's.
SGO_RULE_HD inline double closure_norm_theta(double t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double pi = 3.14159265358979323846;
  if (t >= -pi && t < pi) return t;
  const double m = floor(t / (2 * pi));
  t = t - m * 2 * pi;
  if (t >= pi) t -= 2 * pi;
  if (t < -pi) t += 2 * pi;
  return t;
}
// Q += X S Y^T for 3 x 3 matrices (S row-major)
SGO_RULE_HD inline void closure_xsyt(const double (&X)[3][3], const double* S, const double (&Y)[3][3], double (&Q)[3][3]) {
  double XS[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) XS[a][b] = X[a][0] * S[b] + X[a][1] * S[3 + b] + X[a][2] * S[6 + b];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) Q[a][b] += XS[a][0] * Y[b][0] + XS[a][1] * Y[b][1] + XS[a][2] * Y[b][2];
}
SGO_RULE_HD inline int closure_search(const double* xj, const double* xc, bool free_j, bool free_c, const double* Sjj, const double* Sjc,
                                      const double* Scc, double radius, double* rel, double* cov_rel, double* m2, double* sigma) {
  const double si = sin(xj[2]), ci = cos(xj[2]);
  const double ddx = xc[0] - xj[0], ddy = xc[1] - xj[1];
  const double tx = ci * ddx + si * ddy, ty = -si * ddx + ci * ddy;
  if (rel) {
    rel[0] = tx;
    rel[1] = ty;
    rel[2] = closure_norm_theta(xc[2] - xj[2]);
  }
  const double A[3][3] = {{-ci, -si, ty}, {si, -ci, -tx}, {0.0, 0.0, -1.0}};
  const double B[3][3] = {{ci, si, 0.0}, {-si, ci, 0.0}, {0.0, 0.0, 1.0}};
  double Q[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (free_j) closure_xsyt(A, Sjj, A, Q);
  if (free_j && free_c) {
    double St[9];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) St[3 * a + b] = Sjc[3 * b + a];
    closure_xsyt(A, Sjc, B, Q);
    closure_xsyt(B, St, A, Q);
  }
  if (free_c) closure_xsyt(B, Scc, B, Q);
  double P[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) P[a][b] = P[b][a] = 0.5 * (Q[a][b] + Q[b][a]);
  if (cov_rel)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) cov_rel[3 * a + b] = P[a][b];
  const double d = sqrt(tx * tx + ty * ty);
  const double excess = d - radius;
  if (excess > 0.0) {
    const double ux = tx / d, uy = ty / d;
    const double den = ux * (P[0][0] * ux + P[0][1] * uy) + uy * (P[1][0] * ux + P[1][1] * uy);
    *m2 = den > 0.0 ? excess * excess / den : (den <= 0.0 ? HUGE_VAL : den);
  } else {
    *m2 = excess <= 0.0 ? 0.0 : excess;   // (a NaN pose stays NaN)
  }
  if (sigma) {
    const double h = 0.5 * (P[0][0] - P[1][1]);
    const double lam = 0.5 * (P[0][0] + P[1][1]) + sqrt(h * h + P[0][1] * P[0][1]);
    sigma[0] = sqrt(lam < 0.0 ? 0.0 : lam);
    sigma[1] = sqrt(P[2][2] < 0.0 ? 0.0 : P[2][2]);
  }
  return 0;
}

// The leave-group-out rule of sgo_edge_groups: sgo_edge_leave_one_out's question about k resident edges
// removed together, from the rows idx[0 .. k) of a resident-edge table: N (symmetric, leading dimension ld; block (s, t) at
// N[(3 idx[s] + a) ld + 3 idx[t] + b]) = 1/2 (Q + Q^T) with Q = J H^-1 J^T, e (3 per row), w (the kernel weights) and info6 (Omega's
// upper triangle by rows, 6 per row).  With Omega_t = G_t G_t^T (lower Cholesky), G = blockdiag(G_t), Nt = G^T N G, c = G^T e,
// D = blockdiag(w_t I3), T = D^1/2:
//   pivot = the smallest pivot of the Cholesky factorisation of I - T Nt T (the smallest squared diagonal entry of its factor; the
//           factorisation stops at the first pivot that is not above zero, which is then the answer)
//   K     = I + Nt - D Nt - Nt D - Nt D (I - D) Nt,   d2 = c^T K^-1 c by a Cholesky of K that carries c along as its last row
// d2 is NaN where pivot is not above zero, where K is not positive definite and where an Omega_t is not (pivot NaN too).  k = 0:
// d2 = 0, pivot = 1.  The caller leaves all-zero informations out of idx and decides what a small pivot means.
// The text is written for a square of ns x ns workers (ty, tx) that meet at sync(): the host runs it as one worker (ns = 1, a sync
// that does nothing), k_edge_groups as 16 x 16 threads of a workgroup with ws in LDS.  Every element of every stage is computed by
// ONE worker with its sums in ascending order, so the result does not depend on ns.  ns: a power of two.  ws: edge_group_ws_doubles(k)
// doubles -- two packed lower triangles (Nt: 3 k rows; the factorised matrix: 3 k + 1 rows, c the last), the G_t, w, sqrt(w) and
// the squares whose sum is d2.  d2 and pivot are written by worker (0, 0) alone.  `double`, comparisons and sqrt only.
struct EdgeGroupNoSync {
  void operator()() const {}
};
SGO_RULE_HD inline std::size_t edge_group_tri(int i, int j) { return (std::size_t)i * (std::size_t)(i + 1) / 2 + (std::size_t)j; }   // j <= i
SGO_RULE_HD inline std::size_t edge_group_ws_doubles(int k) {
  const int m = 3 * k;
  return edge_group_tri(m, 0) + edge_group_tri(m + 1, 0) + 8 * (std::size_t)k + (std::size_t)m;
}
template <class Sync>
SGO_RULE_HD inline void edge_group(int k, const int* idx, const double* N, std::size_t ld, const double* e, const double* w, const double* info6,
                                   double* ws, int ty, int tx, int ns, Sync&& sync, double* d2, double* pivot) {
  const int m = 3 * k, lin = ty * ns + tx, nt = ns * ns;
  if (k == 0) {
    if (lin == 0) {
      *d2 = 0.0;
      *pivot = 1.0;
    }
    return;
  }
  double* A = ws;                            // Nt, packed lower
  double* Bm = A + edge_group_tri(m, 0);     // I - T Nt T, then K; row m: c
  double* g = Bm + edge_group_tri(m + 1, 0); // [k][6] g00 g10 g11 g20 g21 g22
  double* wv = g + 6 * (std::size_t)k;
  double* sw = wv + k;
  double* zz = sw + k;
  for (int t = lin; t < k; t += nt) {
    const double* o = info6 + 6 * (std::size_t)idx[t];
    const double o00 = o[0], o01 = o[1], o02 = o[2], o11 = o[3], o12 = o[4], o22 = o[5];
    double g00 = sqrt(o00), g10 = o01 / g00, g20 = o02 / g00;
    const double t11 = o11 - g10 * g10;
    double g11 = sqrt(t11), g21 = (o12 - g20 * g10) / g11;
    const double t22 = o22 - g20 * g20 - g21 * g21;
    double g22 = sqrt(t22);
    if (!(o00 > 0.0) || !(t11 > 0.0) || !(t22 > 0.0) || !(g22 - g22 == 0.0)) g00 = g10 = g20 = g11 = g21 = g22 = sqrt(-1.0);
    double* gt = g + 6 * (std::size_t)t;
    gt[0] = g00, gt[1] = g10, gt[2] = g11, gt[3] = g20, gt[4] = g21, gt[5] = g22;
    wv[t] = w[idx[t]];
    sw[t] = sqrt(wv[t]);
  }
  sync();
  // Nt's blocks (s, t), t <= s: G_s^T N_st G_t; the diagonal block's worker adds c_s = G_s^T e_s
  for (int s = ty; s < k; s += ns)
    for (int t = tx; t <= s; t += ns) {
      const double* gs = g + 6 * (std::size_t)s;
      const double* gt = g + 6 * (std::size_t)t;
      const double Gs[3][3] = {{gs[0], 0.0, 0.0}, {gs[1], gs[2], 0.0}, {gs[3], gs[4], gs[5]}};
      const double Gt[3][3] = {{gt[0], 0.0, 0.0}, {gt[1], gt[2], 0.0}, {gt[3], gt[4], gt[5]}};
      const double* Nb = N + 3 * (std::size_t)idx[s] * ld + 3 * (std::size_t)idx[t];
      double X[3][3];
      for (int a = 0; a < 3; ++a) {
        const double n0 = Nb[a * ld], n1 = Nb[a * ld + 1], n2 = Nb[a * ld + 2];
        X[a][0] = n0 * Gt[0][0] + n1 * Gt[1][0] + n2 * Gt[2][0];
        X[a][1] = n1 * Gt[1][1] + n2 * Gt[2][1];
        X[a][2] = n2 * Gt[2][2];
      }
      for (int b = 0; b < 3; ++b) {
        const double y0 = Gs[0][0] * X[0][b] + Gs[1][0] * X[1][b] + Gs[2][0] * X[2][b];
        const double y1 = Gs[1][1] * X[1][b] + Gs[2][1] * X[2][b];
        const double y2 = Gs[2][2] * X[2][b];
        if (s > t || b <= 0) A[edge_group_tri(3 * s, 3 * t + b)] = y0;
        if (s > t || b <= 1) A[edge_group_tri(3 * s + 1, 3 * t + b)] = y1;
        A[edge_group_tri(3 * s + 2, 3 * t + b)] = y2;
      }
      if (s == t) {
        const double* es = e + 3 * (std::size_t)idx[s];
        Bm[edge_group_tri(m, 3 * s)] = Gs[0][0] * es[0] + Gs[1][0] * es[1] + Gs[2][0] * es[2];
        Bm[edge_group_tri(m, 3 * s + 1)] = Gs[1][1] * es[1] + Gs[2][1] * es[2];
        Bm[edge_group_tri(m, 3 * s + 2)] = Gs[2][2] * es[2];
      }
    }
  sync();
  for (int i = ty; i < m; i += ns)
    for (int j = tx; j <= i; j += ns) Bm[edge_group_tri(i, j)] = (i == j ? 1.0 : 0.0) - sw[i / 3] * A[edge_group_tri(i, j)] * sw[j / 3];
  sync();
  // the pivots of I - T Nt T: a right-looking Cholesky whose column kk stays unscaled (every worker takes 1 / sqrt(a_kk) itself);
  // element (i, j) is its own worker's, updated in ascending kk
  double piv = 1.0;
  for (int kk = 0; kk < m; ++kk) {
    const double akk = Bm[edge_group_tri(kk, kk)];
    if (!(akk >= piv)) piv = akk;
    if (!(akk > 0.0)) break;   // (every worker reads the same a_kk: they leave together)
    const double r = 1.0 / sqrt(akk);
    const int i0 = kk + 1 + ((ty - (kk + 1)) & (ns - 1)), j0 = kk + 1 + ((tx - (kk + 1)) & (ns - 1));
    for (int i = i0; i < m; i += ns) {
      const double li = Bm[edge_group_tri(i, kk)] * r;
      for (int j = j0; j <= i; j += ns) Bm[edge_group_tri(i, j)] -= li * (Bm[edge_group_tri(j, kk)] * r);
    }
    sync();
  }
  sync();
  if (!(piv > 0.0)) {
    if (lin == 0) {
      *d2 = sqrt(-1.0);
      *pivot = piv;
    }
    return;
  }
  // K; the product Nt D (I - D) Nt is skipped where every w (1 - w) is zero (it would add zeros)
  bool frac = false;
  for (int t = 0; t < k; ++t) frac = frac || wv[t] * (1.0 - wv[t]) != 0.0;
  for (int i = ty; i < m; i += ns)
    for (int j = tx; j <= i; j += ns) {
      double sum = 0.0;
      if (frac)
        for (int l = 0; l < m; ++l) {
          const double ail = l <= i ? A[edge_group_tri(i, l)] : A[edge_group_tri(l, i)];
          const double alj = j <= l ? A[edge_group_tri(l, j)] : A[edge_group_tri(j, l)];
          sum += ail * (wv[l / 3] * (1.0 - wv[l / 3])) * alj;
        }
      Bm[edge_group_tri(i, j)] = ((i == j ? 1.0 : 0.0) + A[edge_group_tri(i, j)] * ((1.0 - wv[i / 3]) - wv[j / 3])) - sum;
    }
  sync();
  // K = L L^T with c carried along as row m: after step kk row m holds c - L[:, :kk] z[:kk]
  for (int kk = 0; kk < m; ++kk) {
    const double akk = Bm[edge_group_tri(kk, kk)];
    const double r = akk > 0.0 ? 1.0 / sqrt(akk) : sqrt(-1.0);
    const int i0 = kk + 1 + ((ty - (kk + 1)) & (ns - 1)), j0 = kk + 1 + ((tx - (kk + 1)) & (ns - 1));
    for (int i = i0; i <= m; i += ns) {
      const double li = Bm[edge_group_tri(i, kk)] * r;
      for (int j = j0; j <= i && j < m; j += ns) Bm[edge_group_tri(i, j)] -= li * (Bm[edge_group_tri(j, kk)] * r);
    }
    sync();
  }
  for (int t = lin; t < m; t += nt) {
    const double akk = Bm[edge_group_tri(t, t)];
    const double z = Bm[edge_group_tri(m, t)] * (akk > 0.0 ? 1.0 / sqrt(akk) : sqrt(-1.0));
    zz[t] = z * z;
  }
  sync();
  if (lin == 0) {
    double sum = 0.0;
    for (int t = 0; t < m; ++t) sum += zz[t];
    *d2 = sum;
    *pivot = piv;
  }
}

// The 3 x 3 pieces of sgo_joint_greedy's block-pivoted Cholesky.  A candidate c keeps C_c = S_cc - W_c^T W_c
// as its lower triangle C6 = [c00 c10 c11 c20 c21 c22] and q_c = e_c - W_c^T z.  `double`, comparisons and sqrt only: the host
// (sgo_joint_greedy_rule) and k_joint_grow compile this text.
// jgrow_chol3: C = G G^T, G6 packed as C6; false (G6 not to be used) when C is not positive definite or not finite.
SGO_RULE_HD inline bool jgrow_chol3(const double* C6, double* G6) {
  const double g00 = sqrt(C6[0]), g10 = C6[1] / g00, g20 = C6[3] / g00;
  const double t11 = C6[2] - g10 * g10, g11 = sqrt(t11), g21 = (C6[4] - g20 * g10) / g11;
  const double t22 = C6[5] - g20 * g20 - g21 * g21, g22 = sqrt(t22);
  G6[0] = g00, G6[1] = g10, G6[2] = g11, G6[3] = g20, G6[4] = g21, G6[5] = g22;
  return C6[0] > 0.0 && t11 > 0.0 && t22 > 0.0 && g22 - g22 == 0.0;   // (the last: a non-finite entry)
}
// x = G^-1 b (forward substitution)
SGO_RULE_HD inline void jgrow_solve3(const double* G6, double b0, double b1, double b2, double* x) {
  x[0] = b0 / G6[0];
  x[1] = (b1 - G6[1] * x[0]) / G6[2];
  x[2] = (b2 - G6[3] * x[0] - G6[4] * x[1]) / G6[5];
}
// The extension value v_c = d2 + q_c^T C_c^-1 q_c; NaN where C_c is not positive definite.
SGO_RULE_HD inline double jgrow_value(double d2, const double* C6, const double* q) {
  double G6[6], x[3];
  if (!jgrow_chol3(C6, G6)) return sqrt(-1.0);
  jgrow_solve3(G6, q[0], q[1], q[2], x);
  return d2 + ((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
}
// The update of candidate c by the pivot p whose factor is G6 and whose z+ = G^-1 q_p is zp.  Sp: S's block (rows of p, columns of
// c), element (a, b) at Sp[a ld + b].  Wp, Wc: the m rows so far of W_p and W_c, row r's three entries at Wp[r wps], Wc[r wcs].
// R = S_pc - W_p^T W_c (every sum in ascending row order), w = G^-1 R, C_c -= w^T w, q_c -= w^T z+; w becomes rows m .. m + 2 of W_c.
constexpr int kJgrowRows = 6;   // (m is a multiple of 3: the tail is none or three rows)
SGO_RULE_HD inline void jgrow_update(const double* G6, const double* zp, const double* Sp, std::size_t ld, const double* Wp, std::size_t wps,
                                     double* Wc, std::size_t wcs, int m, double* C6, double* q) {
  double R[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) R[a][b] = Sp[a * ld + b];
  // (full batches of kJgrowRows rows of W_c are read before the first is used, so that their loads are in flight together; the
  // subtractions keep their ascending row order)
  int r = 0;
  for (; r + kJgrowRows <= m; r += kJgrowRows) {
    double wc[kJgrowRows][3];
    for (int u = 0; u < kJgrowRows; ++u) {
      const double* src = Wc + (std::size_t)(r + u) * wcs;
      wc[u][0] = src[0], wc[u][1] = src[1], wc[u][2] = src[2];
    }
    for (int u = 0; u < kJgrowRows; ++u) {
      const double* wp = Wp + (std::size_t)(r + u) * wps;
      for (int a = 0; a < 3; ++a) {
        R[a][0] -= wp[a] * wc[u][0];
        R[a][1] -= wp[a] * wc[u][1];
        R[a][2] -= wp[a] * wc[u][2];
      }
    }
  }
  for (; r < m; ++r) {
    const double* wp = Wp + (std::size_t)r * wps;
    const double* wc = Wc + (std::size_t)r * wcs;
    const double c0 = wc[0], c1 = wc[1], c2 = wc[2];
    for (int a = 0; a < 3; ++a) {
      R[a][0] -= wp[a] * c0;
      R[a][1] -= wp[a] * c1;
      R[a][2] -= wp[a] * c2;
    }
  }
  double w[3][3];   // w[a][b]: row a of the pivot's block, column b of the candidate
  for (int b = 0; b < 3; ++b) {
    double x[3];
    jgrow_solve3(G6, R[0][b], R[1][b], R[2][b], x);
    w[0][b] = x[0], w[1][b] = x[1], w[2][b] = x[2];
  }
  C6[0] -= (w[0][0] * w[0][0] + w[1][0] * w[1][0]) + w[2][0] * w[2][0];
  C6[1] -= (w[0][1] * w[0][0] + w[1][1] * w[1][0]) + w[2][1] * w[2][0];
  C6[2] -= (w[0][1] * w[0][1] + w[1][1] * w[1][1]) + w[2][1] * w[2][1];
  C6[3] -= (w[0][2] * w[0][0] + w[1][2] * w[1][0]) + w[2][2] * w[2][0];
  C6[4] -= (w[0][2] * w[0][1] + w[1][2] * w[1][1]) + w[2][2] * w[2][1];
  C6[5] -= (w[0][2] * w[0][2] + w[1][2] * w[1][2]) + w[2][2] * w[2][2];
  for (int b = 0; b < 3; ++b) q[b] -= (w[0][b] * zp[0] + w[1][b] * zp[1]) + w[2][b] * zp[2];
  for (int a = 0; a < 3; ++a) {
    double* o = Wc + (std::size_t)(m + a) * wcs;
    o[0] = w[a][0], o[1] = w[a][1], o[2] = w[a][2];
  }
}
// The greedy rule's order on (v, c): the smaller v, ties to the lower c.  NaN never reaches it (an ineligible candidate is left out).
SGO_RULE_HD inline bool jgrow_better(double v, int c, double vbest, int cbest) { return v < vbest || (v == vbest && c < cbest); }

// The mask rule of sgo_optimize_gn_hypotheses, which is sgo_set_edge_information's: a hypothesis may not leave a free pose without any
// incident edge of non-zero information.  live_deg[V] holds every vertex' count of such edges in the resident graph, dead(e) says
// whether edge e carries an all-zero information already, off[E] is the hypothesis' mask.  Returns the lowest free vertex that an
// edge the mask switches off leaves without a live edge, or -1; live_deg is used as scratch and put back.
template <class Dead>
inline int hypothesis_isolated_vertex(const unsigned char* fixed, int E, const int* ei, const int* ej, Dead dead, const unsigned char* off,
                                      int* live_deg) {
  for (int e = 0; e < E; ++e)
    if (off[e] && !dead(e)) {
      --live_deg[ei[e]];
      --live_deg[ej[e]];
    }
  int lowest = -1;
  for (int e = 0; e < E; ++e)
    if (off[e] && !dead(e))
      for (const int v : {ei[e], ej[e]})
        if (!fixed[v] && live_deg[v] <= 0 && (lowest < 0 || v < lowest)) lowest = v;
  for (int e = 0; e < E; ++e)
    if (off[e] && !dead(e)) {
      ++live_deg[ei[e]];
      ++live_deg[ej[e]];
    }
  return lowest;
}

// How many hypotheses of sgo_optimize_gn_hypotheses share one chain of launches on a multifrontal context (sgo_hypotheses_chunk):
// as many as the caller's budget holds copies for, at most B and at most the 65535 a grid's y dimension takes.  0: the sequential
// route -- a chain of fewer than two shares nothing, and per <= 0 says there is no batched route.
inline int hypotheses_chunk(long long per_hypothesis_bytes, long long budget_bytes, int B) {
  if (per_hypothesis_bytes <= 0 || budget_bytes <= 0 || B <= 0) return 0;
  const long long k = std::min<long long>(std::min<long long>(B, budget_bytes / per_hypothesis_bytes), 65535);
  return k < 2 ? 0 : (int)k;
}

// Iteration counts are compared at EQUAL tolerance: a solve that stopped at the absolute criterion (a looser relative tolerance
// tolk > tol0, pcg_tol_cap) is scaled to what tol0 would have cost -- PCG converges linearly, iterations ~ log(1 / tolerance).
inline int equal_tolerance_count(int iter, double tol0, double tolk) {
  return (tolk > tol0 && tolk < 1.0 && tol0 > 0.0) ? (int)std::lround(iter * std::log(tol0) / std::log(tolk)) : iter;
}

// How many set-ups one call may redo: three for a short call, one per three Gauss-Newton iterations for a long one.
inline int max_rebuilds(int iters) { return std::max(3, (iters + 2) / 3); }

// The bail-out cap of a solve behind a hierarchy whose best count is `best` (0: the hierarchy has not solved anything yet).
inline int bail_out_cap(int best) { return 4 * best + 40; }

// Staleness of the hierarchy by counts (fresh solves only, against the best count of the CURRENT call): rebuild when the count has
// more than doubled, or is > 25 % above the best while the iterations saved over the rest of the call exceed a set-up's worth
// (~150 PCG iterations).
struct Staleness {
  bool doubled, pays;
  bool rebuild() const { return doubled || pays; }
};
constexpr int kRebuildCostIters = 150;   // what a set-up is worth in PCG iterations (swept: NOTES.md sections 27, 30)
inline Staleness staleness(int eq_iter, int call_best, int iterations_left, int cost_iters = kRebuildCostIters) {
  Staleness s;
  s.doubled = eq_iter > 2 * call_best + 10;
  s.pays = 4 * eq_iter > 5 * call_best && (long long)(eq_iter - call_best) * iterations_left > cost_iters;
  return s;
}

// Lagged refresh: the movement of the level-0 diagonal blocks (relative, summed over the rows) up to which a solve keeps the coarse
// operators of the solve before -- what costs this graph's solves four PCG iterations by the learned slope, at most tau.
inline double lag_allowed(double tau, double slope) { return std::min(tau, 4.0 / std::max(slope, 1.0)); }
constexpr double kLagRowsMoved = 32.0;       // ... and the rows that may have moved by more than a quarter (k_diag_change's third sum)
constexpr double kLagSlopeStart = 2700.0;    // 0.15 % of movement: the cautious start on a graph not seen before
constexpr double kLagSlopeMax = 40000.0;     // no solve is locked out over more than 0.01 % of movement
// ... the slope after a KEPT solve that took `excess` iterations more than the last fresh one over a movement of `moved`:
// the first observation replaces the start value, later ones raise the slope at once and lower it by 20 % per solve.
inline double lag_slope_after_kept(double slope, bool seen, int excess, double moved) {
  const double obs = std::min(kLagSlopeMax, std::max(0.5, (double)excess) / std::max(moved, 1e-5));
  return seen ? std::max(obs, 0.8 * slope) : obs;
}
// ... after a kept solve that had to be INTERRUPTED (progress probe or cap): counted as sixteen iterations over.
inline double lag_slope_after_interrupt(double slope, double moved) {
  return std::min(std::max(slope, 16.0 / std::max(moved, 1e-6)), kLagSlopeMax);
}
// ... after a FRESH solve: a high slope decays by 5 % towards the start value (it is re-examined in time).
inline double lag_slope_after_fresh(double slope) { return slope > kLagSlopeStart ? std::max(kLagSlopeStart, 0.95 * slope) : slope; }
// A kept solve that cost more than a refresh is worth makes the next solve refresh whatever the movement says.
inline bool kept_solve_too_slow(int eq_iter, int fresh_pcg) { return eq_iter > fresh_pcg + 8 + fresh_pcg / 4; }
// The iteration cap of a solve behind kept operators (0: none).
inline int lag_cap(int fresh_pcg) { return fresh_pcg > 0 ? fresh_pcg + 3 : 0; }
// The iteration at which the progress probe of the solves that keep these operators looks.
inline int probe_iteration(int fresh_iter) { return std::max(4, fresh_iter / 3); }

// The aggregation's own staleness, across calls: blocks moved far since the hierarchy was AGGREGATED (sum of ||D - D_ref||_F against
// sum ||D||_F over the rows; rows that moved by a quarter) AND the call's first solve visibly above that aggregation's best count.
inline bool moved_far(double sum_diff, double sum_norm, double rows_quarter, int n) {
  return sum_norm > 0.0 && (sum_diff > 0.05 * sum_norm || rows_quarter > 0.01 * (double)n);
}
inline bool reaggregate(bool far, bool rule_off, int iterations_left_incl, int agg_best, int eq_iter, int rebuilds, int max_rb, bool rebuild_pending) {
  return far && !rule_off && iterations_left_incl >= 5 && agg_best > 0 && 10 * eq_iter > 11 * agg_best && rebuilds < max_rb && !rebuild_pending;
}
// The trial's verdict: the re-made hierarchy's better count of its first two solves against the old one's first solve of the call;
// true = the old hierarchy comes back.
inline bool trial_reverts(int trial_best, int trial_old) { return 100 * trial_best > 85 * trial_old; }

// The floor rule: a solve that stops without reaching pcg_tol (stagnation guard, pcg_maxit) is accepted -- its step applied, as a
// backward-stable direct solver's would be -- when the backward error of its x is at most kFloorEta, measured on the Jacobi-scaled
// system (S H S) y = S b, y = S^-1 x, S = diag(H)^-1/2:
//     eta = |S r| / (|S H S| |S^-1 x| + |S b|),   r = b - H x (the TRUE residual, not the recurrence's).
// The scaled measure does not change when one row is made stiffer (a prior, a closure from a sharp score peak): a normwise one with
// |H| ~ max_i |D_i| lets a cut-off solve through as soon as one diagonal block is large.  S H S has a unit diagonal (>= 1 with the
// incremental overlay's positive semi-definite U M U^T added to H), so |S H S|_2 >= 1: taking it as 1 UNDER-estimates the norm and
// eta errs on the strict side.  S_kk comes from the diagonal entries of each row's diagonal block, dblk6[6 i + {0, 3, 5}] (the
// symmetric packing [00 01 02 11 12 22] of S0.dblk).  A diagonal entry that is not finite or not positive, or a result that is not
// finite, gives eta = 1: not accepted.  r, x, b: 3 n doubles in the rows' order.
constexpr double kFloorEta = 1e-12;   // ~ 4 500 units of roundoff
inline double floor_backward_error(int n, const double* r, const double* x, const double* b, const double* dblk6) {
  double sr = 0.0, sx = 0.0, sb = 0.0;
  for (int i = 0; i < n; ++i)
    for (int q = 0; q < 3; ++q) {
      const double h = dblk6[6 * (std::size_t)i + (q == 0 ? 0 : q == 1 ? 3 : 5)];
      if (!(h > 0.0) || !std::isfinite(h)) return 1.0;
      const std::size_t k = 3 * (std::size_t)i + q;
      sr += r[k] * r[k] / h;
      sx += x[k] * x[k] * h;
      sb += b[k] * b[k] / h;
    }
  const double den = std::sqrt(sx) + std::sqrt(sb);
  const double eta = std::sqrt(sr) / den;
  return (den > 0.0 && std::isfinite(eta)) ? eta : 1.0;
}

}  // namespace rules
}  // namespace sgo
