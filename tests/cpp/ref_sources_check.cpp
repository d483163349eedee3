// ref_sources_check.cpp -- EdgeSE2RhoTheta::computeError on 2000 pose / line pairs that cover the wraps and the sign flip of
// rho, one pair per line ("e0 e1", 17 significant digits).  With -DSGO_REF_SOURCES the error is the REFERENCE's own
// computeError (src/sparse_gslam/src/g2o_bindings/edge_se2_rhotheta.cpp:9-16, through ls_extractor/utils.h:22-45), compiled
// verbatim from a reference checkout and linked in: scripts/make_golden_ref_rhotheta.py records that output in
// tests/golden/ref_rhotheta.npz.  Without it, the error is this repo's restatement (tests/cpp/landmark_rhotheta.cpp,
// oracle/np_lm_oracle.py), which tests/test_landmark_lm.py compares with the recorded values: the two must agree to rounding.
#include <iostream>
#include <iomanip>
#include "g2o/core/base_binary_edge.h"
#include "g2o/core/base_vertex.h"
#include "g2o/types/slam2d/vertex_se2.h"
#include "g2o/stuff/misc.h"
#ifdef SGO_REF_SOURCES
#include "g2o_bindings/edge_se2_rhotheta.h"
#include "g2o_bindings/vertex_rhotheta.h"
#endif
using namespace g2o;
inline Eigen::Vector2d move_line(const Eigen::Vector2d& rt, const Eigen::Vector2d& trans, double angle) {
  double th = rt[1] + angle;
  if (th > const_pi()) th -= 2 * const_pi();
  if (th < -const_pi()) th += 2 * const_pi();
  double rho = rt[0] + trans[0] * std::cos(th) + trans[1] * std::sin(th);
  if (rho < 0.0) { rho = -rho; th += const_pi(); if (th > const_pi()) th -= 2 * const_pi(); }
  return Eigen::Vector2d(rho, th);
}
int main() {
  std::cout << std::setprecision(17);
  for (int k = 0; k < 2000; ++k) {
    double x = std::sin(k * 1.3) * 5, y = std::cos(k * 0.7) * 5, t = std::sin(k * 2.1) * 3.1;
    double r = 1 + std::fabs(std::sin(k * 0.37)) * 6, th = std::sin(k * 0.91) * 3.1;
#ifdef SGO_REF_SOURCES
    VertexSE2 p; VertexRhoTheta l; EdgeSE2RhoTheta e;
    p.setEstimate(SE2(x, y, t)); l.setEstimate(Eigen::Vector2d(r, th));
    e.vertices()[0] = &p; e.vertices()[1] = &l; e.setMeasurement(Eigen::Vector2d(2.0, 0.3));
    e.computeError();
    double e0 = e.error()[0], e1 = e.error()[1];
#else
    const SE2 pinv = SE2(x, y, t).inverse();
    Eigen::Vector2d pred = move_line(Eigen::Vector2d(r, th), pinv.translation(), pinv.rotation().angle());
    double e0 = 2.0 - pred[0], e1 = normalize_theta(0.3 - pred[1]);
#endif
    std::cout << e0 << " " << e1 << "\n";
  }
  return 0;
}
