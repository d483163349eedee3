// terminate_action_host.cpp -- SparseOptimizerTerminateAction on the host solver of include/g2o/sgo_g2o_compat.h (no GPU needed): a
// small pose graph whose closures are of a user-defined edge class, so that optimize() takes the host's Gauss-Newton.  The same
// graph is built twice: optimize(50) with the action stops after k < 50 iterations; optimize(k) without it must leave the same
// estimates, bit for bit.  An action of another class is refused.  Prints
//   k  iterations_without_action  max_abs_estimate_difference  foreign_refused  same_action_twice  removed  iterations_max1
// for tests/test_stop_rule.py.  Public API only.
#include <cmath>
#include <deque>
#include <iomanip>
#include <iostream>

#include "g2o/core/block_solver.h"
#include "g2o/core/hyper_graph_action.h"
#include "g2o/core/optimization_algorithm_gauss_newton.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/core/sparse_optimizer_terminate_action.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam2d/edge_se2.h"
#include "g2o/types/slam2d/vertex_se2.h"

namespace {

class ClosureEdge : public g2o::EdgeSE2 {};             // not EdgeSE2 itself: the device path does not take the graph
class ForeignAction : public g2o::HyperGraphAction {};  // any post-iteration action that is not the terminate action

constexpr int NP = 24;

struct Graph {
  g2o::SparseOptimizer opt;
  std::deque<g2o::VertexSE2> poses;
  std::deque<g2o::EdgeSE2> odom;
  std::deque<ClosureEdge> closures;
  Graph() : poses(NP), odom(NP - 1) {
    using SlamBlockSolver = g2o::BlockSolver<g2o::BlockSolverTraits<3, 3>>;
    using SlamLinearSolver = g2o::LinearSolverEigen<SlamBlockSolver::PoseMatrixType>;
    opt.setAlgorithm(new g2o::OptimizationAlgorithmGaussNewton(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));
    g2o::SE2 truth[NP];
    for (int k = 0; k < NP; ++k) truth[k] = g2o::SE2(3.0 * std::cos(0.26 * k), 3.0 * std::sin(0.26 * k), 0.26 * k + 1.57);
    Eigen::Matrix3d cov;
    cov << 0.01, 0.001, 0, 0.001, 0.02, 0, 0, 0, 0.005;
    const Eigen::Matrix3d info = cov.inverse();
    for (int k = 0; k < NP; ++k) {
      poses[k].setId(k);
      poses[k].setEstimate(k == 0 ? truth[k]
                                  : g2o::SE2(truth[k][0] + 0.3 * std::cos(3.0 * k), truth[k][1] - 0.25 * std::sin(2.0 * k), truth[k][2] + 0.2 * std::cos(5.0 * k)));
      poses[k].setFixed(k == 0);
      opt.addVertex(&poses[k]);
    }
    for (int k = 0; k + 1 < NP; ++k) {
      odom[k].vertices()[0] = &poses[k];
      odom[k].vertices()[1] = &poses[k + 1];
      const g2o::SE2 z = truth[k].inverse() * truth[k + 1];
      odom[k].setMeasurement(g2o::SE2(z[0] + 0.02 * std::sin(1.3 * k), z[1] + 0.02 * std::cos(0.7 * k), z[2] + 0.01 * std::sin(2.1 * k)));
      odom[k].information() = info;
      opt.addEdge(&odom[k]);
    }
    for (int k = 0; k + 9 < NP; k += 5) {
      closures.emplace_back();
      ClosureEdge& c = closures.back();
      c.vertices()[0] = &poses[k];
      c.vertices()[1] = &poses[k + 9];
      c.setMeasurement(truth[k].inverse() * truth[k + 9]);
      c.information() = info;
      opt.addEdge(&c);
    }
    opt.initializeOptimization();
  }
  ~Graph() { delete opt.algorithm(); }
};

}  // namespace

int main() {
  Graph a, b, c;
  g2o::SparseOptimizerTerminateAction stop;   // gainThreshold 1e-6, maxIterations INT_MAX: the defaults
  ForeignAction foreign;
  const bool foreign_refused = !a.opt.addPostIterationAction(&foreign);
  const bool added = a.opt.addPostIterationAction(&stop);
  const bool twice = a.opt.addPostIterationAction(&stop);
  const int k = a.opt.optimize(50);
  const int kb = b.opt.optimize(k);
  double diff = 0.0;
  for (int v = 0; v < NP; ++v)
    for (int q = 0; q < 3; ++q) diff = std::max(diff, std::fabs(a.poses[v].estimate()[q] - b.poses[v].estimate()[q]));
  // maxIterations: the call stops after the iteration with that index
  g2o::SparseOptimizerTerminateAction cap;
  cap.setGainThreshold(0.0);
  cap.setMaxIterations(1);
  c.opt.addPostIterationAction(&cap);
  const int kc = c.opt.optimize(50);
  const bool removed = c.opt.removePostIterationAction(&cap) && !c.opt.removePostIterationAction(&cap);
  std::cout << std::setprecision(17) << k << " " << kb << " " << diff << " " << (foreign_refused ? 1 : 0) << " " << ((added && !twice) ? 1 : 0)
            << " " << (removed ? 1 : 0) << " " << kc << std::endl;
  return 0;
}
