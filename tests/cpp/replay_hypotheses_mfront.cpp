// replay_hypotheses_mfront.cpp -- leave-one-out over the first closures of a graph of the multifrontal path through the
// g2o-compatible header, with a workspace granted: a VertexSE2 / EdgeSE2 graph under Gauss-Newton, sgoSetHypothesesWorkspace(bytes),
// initializeOptimization(), then SparseOptimizer::sgoOptimizeHypotheses with one hypothesis per closure (that closure switched off).
// Writes the backend's description, the number of hypotheses, how many vertex estimates moved (none may), and per hypothesis
// "iterations stopReason chi2 robustChi2", every edge's chi2 in edge order and the poses in vertex order -- doubles as the 16
// hexadecimal digits of their bits -- for tests/test_gpu_hypotheses_mfront.py.  Public API only.
//
// usage: replay_hypotheses_mfront graph.txt out.txt iters gain_threshold workspace_bytes hypotheses
//        (graph.txt as tests/test_shim_replay.py writes it)
#include <cstdint>
#include <cstdlib>
#include <cstring>
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

g2o::RobustKernelDCS dcs_kernel;

Eigen::Matrix3d info_from(const double* u) {
  Eigen::Matrix3d O;
  O << u[0], u[1], u[2], u[1], u[3], u[4], u[2], u[4], u[5];
  return O;
}

struct Hex {
  double v;
};
std::ostream& operator<<(std::ostream& os, Hex h) {
  std::uint64_t u;
  std::memcpy(&u, &h.v, sizeof u);
  return os << std::hex << std::setw(16) << std::setfill('0') << u << std::dec;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  const long long workspace = std::atoll(argv[5]);
  const size_t want = (size_t)std::atoll(argv[6]);
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
  for (int k = 0; k < V; ++k) {
    vs[k].setId(k);
    vs[k].setEstimate(g2o::SE2(poses[3 * k], poses[3 * k + 1], poses[3 * k + 2]));
    vs[k].setFixed(k == 0);
    opt.addVertex(&vs[k]);
  }
  std::vector<std::vector<g2o::OptimizableGraph::Edge*>> off;
  for (int k = 0; k < E; ++k) {
    const Ed& d = edges[k];
    es[k].vertices()[0] = &vs[d.i];
    es[k].vertices()[1] = &vs[d.j];
    es[k].setMeasurement(g2o::SE2(d.z[0], d.z[1], d.z[2]));
    es[k].information() = info_from(d.o);
    if (d.closure) {
      es[k].setRobustKernel(&dcs_kernel);
      if (off.size() < want) off.push_back(std::vector<g2o::OptimizableGraph::Edge*>(1, &es[k]));   // leave this closure out
    }
    opt.addEdge(&es[k]);
  }
  if (opt.sgoSetHypothesesWorkspace(-1) || !opt.sgoSetHypothesesWorkspace(workspace)) return 6;
  opt.initializeOptimization();
  std::vector<g2o::SgoHypothesis> hyp;
  if (!opt.sgoOptimizeHypotheses(off, std::atoi(argv[3]), std::atof(argv[4]), hyp)) return 5;
  const std::string desc = opt.backendDescription();
  int moved = 0;
  for (int k = 0; k < V; ++k)
    for (int q = 0; q < 3; ++q) {
      const double now = vs[k].estimate()[q];
      moved += std::memcmp(&now, &poses[3 * k + q], sizeof(double)) != 0;
    }

  std::ofstream out(argv[2]);
  out << desc << "\n" << hyp.size() << "\n" << moved << "\n";
  for (const g2o::SgoHypothesis& h : hyp) {
    out << h.iterations << " " << h.stopReason << " " << Hex{h.chi2} << " " << Hex{h.robustChi2} << "\n";
    for (int k = 0; k < E; ++k) out << Hex{h.edgeChi2.at(&es[k])} << (k + 1 < E ? " " : "\n");
    for (int k = 0; k < V; ++k) {
      const g2o::SE2& p = h.poses.at(k);
      out << Hex{p[0]} << " " << Hex{p[1]} << " " << Hex{p[2]} << "\n";
    }
  }
  delete opt.algorithm();
  return out.good() ? 0 : 4;
}
