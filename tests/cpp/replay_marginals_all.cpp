// replay_marginals_all.cpp -- SparseOptimizer::computeMarginals through the g2o-compat shim for EVERY vertex of a pose graph: the
// VertexContainer overload with all vertices (the fixed one is skipped), which is more than 8 distinct column vertices and so
// goes through sgo_marginals_selected.  Records the estimates and the diagonal blocks for tests/test_gpu_selinv.py.  Public API only.
//
// build: the line of replay_marginals.cpp with this file's name (tests/test_gpu_selinv.py builds it itself).
// usage: replay_marginals_all graph.txt out.txt iters      (graph.txt as tests/test_shim_replay.py writes it; its phi is the kernel's delta)
//
// out.txt: "done", the backend's description after optimize() and again after computeMarginals (three lines), the V estimates,
// then one line per free vertex in hessian order:  block h s00 s01 .. s22
#include <cstdlib>
#include <deque>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "g2o/core/block_solver.h"
#include "g2o/core/optimization_algorithm_gauss_newton.h"
#include "g2o/core/robust_kernel_impl.h"
#include "g2o/core/sparse_block_matrix.h"
#include "g2o/core/sparse_optimizer.h"
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

  std::deque<g2o::VertexSE2, Eigen::aligned_allocator<g2o::VertexSE2>> verts;
  std::deque<g2o::EdgeSE2, Eigen::aligned_allocator<g2o::EdgeSE2>> es;
  g2o::SparseOptimizer opt;
  using SlamBlockSolver = g2o::BlockSolver<g2o::BlockSolverTraits<3, 3>>;
  using SlamLinearSolver = g2o::LinearSolverEigen<SlamBlockSolver::PoseMatrixType>;
  opt.setAlgorithm(new g2o::OptimizationAlgorithmGaussNewton(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));
  for (int k = 0; k < V; ++k) {
    verts.emplace_back();
    g2o::VertexSE2* v = &verts.back();
    v->setId(k);
    v->setEstimate(g2o::SE2(poses[3 * k], poses[3 * k + 1], poses[3 * k + 2]));
    v->setFixed(k == 0);
    opt.addVertex(v);
  }
  for (const Ed& e : edges) {
    es.emplace_back();
    g2o::EdgeSE2* ed = &es.back();
    ed->vertices()[0] = &verts[(size_t)e.i];
    ed->vertices()[1] = &verts[(size_t)e.j];
    ed->setMeasurement(g2o::SE2(e.z[0], e.z[1], e.z[2]));
    ed->information() = info_from(e.o);
    if (e.closure) ed->setRobustKernel(&dcs_kernel);
    opt.addEdge(ed);
  }
  opt.initializeOptimization();
  const int done = opt.optimize(iters);
  const std::string desc = opt.backendDescription();

  g2o::HyperGraph::VertexContainer all;
  for (auto& v : verts) all.push_back(&v);
  g2o::SparseBlockMatrix<g2o::MatrixX> spinv;
  if (!opt.computeMarginals(spinv, all)) return 5;

  std::ofstream out(argv[2]);
  out << std::setprecision(17);
  out << done << "\n" << desc << "\n" << opt.backendDescription() << "\n";
  for (auto& v : verts) out << v.estimate()[0] << " " << v.estimate()[1] << " " << v.estimate()[2] << "\n";
  if (spinv.rows() != 3 * (V - 1) || spinv.cols() != 3 * (V - 1)) return 6;
  for (auto& v : verts) {
    const int h = v.hessianIndex();
    if (h < 0) continue;
    const g2o::MatrixX* B = spinv.block(h, h);
    if (!B || B->rows() != 3 || B->cols() != 3) return 6;
    out << "block " << h;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) out << " " << (*B)(a, b);
    out << "\n";
  }
  delete opt.algorithm();
  return out.good() ? 0 : 4;
}
