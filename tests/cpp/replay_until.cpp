// replay_until.cpp -- the two lines a sparse-gslam maintainer adds after setup_pose_opt: a
// SparseOptimizerTerminateAction registered with addPostIterationAction, then the reference's optimize(20) on a VertexSE2 / EdgeSE2
// graph under Gauss-Newton.  On the device path the shim turns that into one sgo_optimize_gn_until.  Writes the iterations optimize()
// returned, the backend's description and the estimates for tests/test_gpu_optimize_until.py.  Public API only.
//
// usage: replay_until graph.txt out.txt gain_threshold          (graph.txt as tests/test_shim_replay.py writes it)
#include <cstdlib>
#include <deque>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "g2o/core/block_solver.h"
#include "g2o/core/optimization_algorithm_gauss_newton.h"
#include "g2o/core/robust_kernel_impl.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/core/sparse_optimizer_terminate_action.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam2d/edge_se2.h"
#include "g2o/types/slam2d/vertex_se2.h"

namespace {

g2o::RobustKernelDCS dcs_kernel;

Eigen::Matrix3d info_from(const double* u) {
  Eigen::Matrix3d O;
  O << u[0], u[1], u[2], u[1], u[3], u[4], u[2], u[4], u[5];
  return O;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  std::ifstream in(argv[1]);
  int V, E;
  double phi;
  in >> V >> E >> phi;
  std::vector<double> poses(3 * (size_t)V);
  for (auto& v : poses) in >> v;
  struct Ed { int i, j; double z[3], o[6]; int closure; };
  std::vector<Ed> edges(E);
  for (auto& e : edges) {
    in >> e.i >> e.j >> e.closure;
    for (double& v : e.z) in >> v;
    for (double& v : e.o) in >> v;
  }
  if (!in) return 3;
  dcs_kernel.setDelta(phi);

  std::deque<g2o::VertexSE2, Eigen::aligned_allocator<g2o::VertexSE2>> vs(V);
  std::deque<g2o::EdgeSE2, Eigen::aligned_allocator<g2o::EdgeSE2>> es(E);
  g2o::SparseOptimizer opt;
  using SlamBlockSolver = g2o::BlockSolver<g2o::BlockSolverTraits<3, 3>>;
  using SlamLinearSolver = g2o::LinearSolverEigen<SlamBlockSolver::PoseMatrixType>;
  opt.setAlgorithm(new g2o::OptimizationAlgorithmGaussNewton(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));
  g2o::SparseOptimizerTerminateAction stop;
  stop.setGainThreshold(std::atof(argv[3]));
  if (!opt.addPostIterationAction(&stop)) return 5;

  for (int k = 0; k < V; ++k) {
    vs[k].setId(k);
    vs[k].setEstimate(g2o::SE2(poses[3 * k], poses[3 * k + 1], poses[3 * k + 2]));
    vs[k].setFixed(k == 0);
    opt.addVertex(&vs[k]);
  }
  for (int k = 0; k < E; ++k) {
    const Ed& d = edges[k];
    es[k].vertices()[0] = &vs[d.i];
    es[k].vertices()[1] = &vs[d.j];
    es[k].setMeasurement(g2o::SE2(d.z[0], d.z[1], d.z[2]));
    es[k].information() = info_from(d.o);
    if (d.closure) es[k].setRobustKernel(&dcs_kernel);
    opt.addEdge(&es[k]);
  }
  opt.initializeOptimization();
  const int its = opt.optimize(20);
  const std::string desc = opt.backendDescription();

  std::ofstream out(argv[2]);
  out << std::setprecision(17);
  out << its << "\n" << desc << "\n";
  for (auto& v : vs) out << v.estimate()[0] << " " << v.estimate()[1] << " " << v.estimate()[2] << "\n";
  delete opt.algorithm();
  return out.good() ? 0 : 4;
}
