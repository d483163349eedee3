// replay_robust.cpp -- a pose graph whose closures carry RobustKernelHuber and RobustKernelCauchy (alternating), through the
// g2o-compat shim: build, initializeOptimization, optimize(iters).  Records what the backend says about the graph it holds, for
// tests/test_gpu_robust_kernels.py.  Public API only.
//
// usage: replay_robust graph.txt out.txt iters      (graph.txt as tests/test_shim_replay.py writes it; its phi is the kernels' delta)
#include <cstdlib>
#include <deque>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "g2o/core/block_solver.h"
#include "g2o/core/optimization_algorithm_gauss_newton.h"
#include "g2o/core/robust_kernel_impl.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam2d/edge_se2.h"
#include "g2o/types/slam2d/vertex_se2.h"

namespace {

struct PoseChain {
  g2o::VertexSE2 pose;
  g2o::EdgeSE2 edge;
};

g2o::RobustKernelHuber huber_kernel;
g2o::RobustKernelCauchy cauchy_kernel;

Eigen::Matrix3d info_from(const double* u) {
  Eigen::Matrix3d O;
  O << u[0], u[1], u[2], u[1], u[3], u[4], u[2], u[4], u[5];
  return O;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  std::ifstream in(argv[1]);
  const int iters = std::atoi(argv[3]);
  int V, E;
  double delta;
  in >> V >> E >> delta;
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
  huber_kernel.setDelta(delta);
  cauchy_kernel.setDelta(delta);

  std::deque<PoseChain, Eigen::aligned_allocator<PoseChain>> chain;
  std::deque<g2o::EdgeSE2, Eigen::aligned_allocator<g2o::EdgeSE2>> closures;
  g2o::SparseOptimizer opt;
  using SlamBlockSolver = g2o::BlockSolver<g2o::BlockSolverTraits<3, 3>>;
  using SlamLinearSolver = g2o::LinearSolverEigen<SlamBlockSolver::PoseMatrixType>;
  opt.setAlgorithm(new g2o::OptimizationAlgorithmGaussNewton(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));

  chain.emplace_back();
  chain.back().pose.setId(0);
  chain.back().pose.setEstimate(g2o::SE2(poses[0], poses[1], poses[2]));
  chain.back().pose.setFixed(true);
  opt.addVertex(&chain.back().pose);
  g2o::VertexSE2* prev = &chain.back().pose;
  for (int k = 1; k < V; ++k) {   // (the file lists the V - 1 odometry edges first)
    const Ed& od = edges[k - 1];
    chain.emplace_back();
    g2o::VertexSE2* pose = &chain.back().pose;
    g2o::EdgeSE2* edge = &chain.back().edge;
    pose->setId(k);
    pose->setEstimate(g2o::SE2(poses[3 * k], poses[3 * k + 1], poses[3 * k + 2]));
    edge->vertices()[0] = prev;
    edge->vertices()[1] = pose;
    edge->information() = info_from(od.o);
    edge->setMeasurement(g2o::SE2(od.z[0], od.z[1], od.z[2]));
    opt.addVertex(pose);
    opt.addEdge(edge);
    prev = pose;
  }
  for (int k = V - 1; k < E; ++k) {
    const Ed& c = edges[k];
    closures.emplace_back();
    g2o::EdgeSE2* ce = &closures.back();
    ce->setMeasurement(g2o::SE2(c.z[0], c.z[1], c.z[2]));
    ce->information() = info_from(c.o);
    ce->vertices()[0] = &chain[c.i].pose;
    ce->vertices()[1] = &chain[c.j].pose;
    if ((k - (V - 1)) % 2 == 0) ce->setRobustKernel(&huber_kernel);
    else ce->setRobustKernel(&cauchy_kernel);
    opt.addEdge(ce);
  }

  opt.initializeOptimization();
  const int done = opt.optimize(iters);
  const std::string desc = opt.backendDescription();
  opt.computeActiveErrors();
  const double chi2 = opt.activeChi2(), rchi2 = opt.activeRobustChi2();

  std::ofstream out(argv[2]);
  out << std::setprecision(17);
  out << done << " " << chi2 << " " << rchi2 << "\n" << desc << "\n";
  for (auto& pc : chain) out << pc.pose.estimate()[0] << " " << pc.pose.estimate()[1] << " " << pc.pose.estimate()[2] << "\n";
  delete opt.algorithm();
  return out.good() ? 0 : 4;
}
