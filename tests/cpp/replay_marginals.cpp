// replay_marginals.cpp -- SparseOptimizer::computeMarginals through the g2o-compat shim: a pose graph whose closures carry the
// shared RobustKernelDCS is built, optimised, and asked for the marginal covariance of its last vertex (the Vertex* overload), of
// a list of hessian block pairs and of a vertex container; a Levenberg-configured optimiser must refuse.  Records the estimates
// and the blocks for tests/test_gpu_marginals.py.  Public API only.
//
// build (from tests/cpp, the line of its Makefile's replays; tests/test_gpu_marginals.py builds it itself):
//   g++ -O2 -std=c++14 -Wall -Wextra -I../../include -o replay_marginals replay_marginals.cpp -L../../sparse_gslam_amd/csrc -lsgo
//       -Wl,-rpath,$PWD/../../sparse_gslam_amd/csrc -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib
// usage: replay_marginals graph.txt out.txt iters      (graph.txt as tests/test_shim_replay.py writes it; its phi is the kernel's delta)
//
// out.txt: "done" and the backend's description (two lines), the V estimates, then one line per block:
//   tag r c s00 s01 .. s22        tag: vertex | pairs | container; r, c hessian block indices
// and a last line "rows cols absent levenberg": spinv's size, whether a block never asked for is absent, what the
// Levenberg-configured optimiser returned.
#include <cstdlib>
#include <deque>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "g2o/core/block_solver.h"
#include "g2o/core/optimization_algorithm_gauss_newton.h"
#include "g2o/core/optimization_algorithm_levenberg.h"
#include "g2o/core/robust_kernel_impl.h"
#include "g2o/core/sparse_block_matrix.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam2d/edge_se2.h"
#include "g2o/types/slam2d/vertex_se2.h"

namespace {

struct PoseChain {
  g2o::VertexSE2 pose;
  g2o::EdgeSE2 edge;
};

g2o::RobustKernelDCS dcs_kernel;

Eigen::Matrix3d info_from(const double* u) {
  Eigen::Matrix3d O;
  O << u[0], u[1], u[2], u[1], u[3], u[4], u[2], u[4], u[5];
  return O;
}

void print_block(std::ostream& out, const char* tag, int r, int c, const g2o::MatrixX* B) {
  out << tag << " " << r << " " << c;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) out << " " << (*B)(a, b);
  out << "\n";
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
  dcs_kernel.setDelta(delta);

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
    ce->setRobustKernel(&dcs_kernel);
    opt.addEdge(ce);
  }

  opt.initializeOptimization();
  const int done = opt.optimize(iters);
  const std::string desc = opt.backendDescription();

  std::ofstream out(argv[2]);
  out << std::setprecision(17);
  out << done << "\n" << desc << "\n";
  for (auto& pc : chain) out << pc.pose.estimate()[0] << " " << pc.pose.estimate()[1] << " " << pc.pose.estimate()[2] << "\n";

  // the last vertex
  g2o::SparseBlockMatrix<g2o::MatrixX> spinv;
  const g2o::VertexSE2* last = &chain.back().pose;
  const int hl = last->hessianIndex();
  if (!opt.computeMarginals(spinv, last) || !spinv.block(hl, hl)) return 5;
  if (spinv.block(hl, hl)->rows() != 3 || spinv.block(hl, hl)->cols() != 3) return 5;
  print_block(out, "vertex", hl, hl, spinv.block(hl, hl));
  const int rows = spinv.rows(), cols = spinv.cols();
  const bool absent = spinv.block(0, 0) == nullptr && spinv.block(hl, 0) == nullptr;
  // a pair list: two diagonal blocks, an off-diagonal block and its mirror, one pair twice
  const int hm = hl / 2;
  const std::vector<std::pair<int, int>> pairs = {{0, 0}, {hm, hm}, {hl, hm}, {hm, hl}, {hl, hm}};
  if (!opt.computeMarginals(spinv, pairs)) return 6;
  for (const auto& rc : pairs) {
    if (!spinv.block(rc.first, rc.second)) return 6;
    print_block(out, "pairs", rc.first, rc.second, spinv.block(rc.first, rc.second));
  }
  if (spinv.block(hl, hl)) return 6;   // (spinv holds what the LAST call was asked for)
  // a container with the fixed vertex in it: skipped
  g2o::HyperGraph::VertexContainer some = {&chain[0].pose, &chain[1].pose, &chain[(size_t)V - 1].pose};
  if (!opt.computeMarginals(spinv, some) || spinv.block(0, 0) == nullptr || spinv.block(hl, hl) == nullptr) return 7;
  print_block(out, "container", 0, 0, spinv.block(0, 0));
  print_block(out, "container", hl, hl, spinv.block(hl, hl));
  if (opt.computeMarginals(spinv, &chain[0].pose)) return 7;   // (a fixed vertex has no hessian index: false, as upstream)

  // the same graph under Levenberg takes the host solver, which has no marginals: false
  delete opt.algorithm();
  opt.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));
  const bool lm = opt.computeMarginals(spinv, pairs);
  out << rows << " " << cols << " " << (absent ? 1 : 0) << " " << (lm ? 1 : 0) << "\n";
  delete opt.algorithm();
  return out.good() ? 0 : 4;
}
