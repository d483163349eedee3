// replay_edge_groups.cpp -- SparseOptimizer::sgoEdgeJoint / sgoEdgeGroups through the g2o-compat shim: a pose graph is optimised,
// a table of its closures is built and groups of them are put to the leave-group-out test.  Records the estimates, d2, pivot and
// the decision of every group, and what the calls return when they must refuse, for tests/test_gpu_edge_groups.py.  Public API only.
//
// build: the line of replay_candidate_gate.cpp with this file's name (tests/test_gpu_edge_groups.py builds it itself).
// usage: replay_edge_groups graph.txt out.txt iters chi2_max min_pivot group_size
//   graph.txt as tests/test_shim_replay.py writes it (its phi is the kernel's delta)
// The table holds the first 64 closures (all, if fewer); group b holds rows b, b + 1, ... b + group_size - 1 (mod the table), b = 0 .. 15.
//
// out.txt: "done", the backend's description after optimize() and again after the test (three lines), the V estimates, the table's
// edges as  row t k  (k: the edge's place in the graph's list), one line per group:  group b d2 pivot fail,  then  nfail N,
// not_active R,  stale R,  levenberg R,  refused R,  bad_row R  (R: what a call returned for an edge that was never added, after an
// addVertex without initializeOptimization, under Levenberg, for min_pivot = 0 and for a row outside the table)
#include <cstdlib>
#include <deque>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "g2o/core/block_solver.h"
#include "g2o/core/optimization_algorithm_gauss_newton.h"
#include "g2o/core/optimization_algorithm_levenberg.h"
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

}  // namespace

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  std::ifstream in(argv[1]);
  const int iters = std::atoi(argv[3]);
  const double chi2_max = std::atof(argv[4]), min_pivot = std::atof(argv[5]);
  const int gsize = std::atoi(argv[6]);
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
  auto fill = [&](g2o::EdgeSE2* ed, const Ed& e) {
    ed->vertices()[0] = &verts[(size_t)e.i];
    ed->vertices()[1] = &verts[(size_t)e.j];
    ed->setMeasurement(g2o::SE2(e.z[0], e.z[1], e.z[2]));
    ed->information() = info_from(e.o);
  };
  std::vector<g2o::OptimizableGraph::Edge*> list;
  std::vector<int> place;
  for (const Ed& e : edges) {
    es.emplace_back();
    fill(&es.back(), e);
    if (e.closure) es.back().setRobustKernel(&dcs_kernel);
    opt.addEdge(&es.back());
    if (e.closure && list.size() < 64) {
      list.push_back(&es.back());
      place.push_back((int)es.size() - 1);
    }
  }
  opt.initializeOptimization();
  const int done = opt.optimize(iters);
  const std::string desc = opt.backendDescription();

  const int n = opt.sgoEdgeJoint(list);
  if (n != (int)list.size() || n < gsize) return 5;
  std::vector<std::vector<int>> groups(16);
  for (int b = 0; b < 16; ++b)
    for (int q = 0; q < gsize; ++q) groups[(size_t)b].push_back((b + q) % n);
  const std::vector<double> chi(groups.size(), chi2_max);
  std::vector<double> d2, piv;
  std::vector<bool> fail;
  const int nfail = opt.sgoEdgeGroups(groups, chi, min_pivot, &d2, &piv, &fail);
  if (nfail < 0 || d2.size() != groups.size() || piv.size() != groups.size() || fail.size() != groups.size()) return 5;
  const std::string desc2 = opt.backendDescription();

  // the refusals: none may touch the outputs
  std::vector<double> d2r(1, 7.0), pivr(1, 7.0);
  std::vector<bool> failr(1, true);
  const int refused = opt.sgoEdgeGroups(groups, chi, 0.0, &d2r, &pivr, &failr);
  const int bad_row = opt.sgoEdgeGroups(std::vector<std::vector<int>>(1, std::vector<int>(1, n)), std::vector<double>(1, chi2_max), min_pivot, &d2r, &pivr, &failr);
  g2o::EdgeSE2 odd;   // an edge that was never added
  fill(&odd, edges[0]);
  const int not_active = opt.sgoEdgeJoint(std::vector<g2o::OptimizableGraph::Edge*>(1, &odd));
  g2o::VertexSE2 stranger;
  stranger.setId(V);
  stranger.setEstimate(g2o::SE2(0.0, 0.0, 0.0));
  opt.addVertex(&stranger);
  const int stale = opt.sgoEdgeJoint(list) < 0 && opt.sgoEdgeGroups(groups, chi, min_pivot, &d2r, &pivr, &failr) < 0 ? -1 : 0;
  opt.removeVertex(&stranger);
  opt.initializeOptimization();
  g2o::OptimizationAlgorithm* gn = opt.algorithm();
  opt.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));
  const int lm = opt.sgoEdgeJoint(list) < 0 && opt.sgoEdgeGroups(groups, chi, min_pivot, &d2r, &pivr, &failr) < 0 ? -1 : 0;
  delete opt.algorithm();
  opt.setAlgorithm(gn);
  if (d2r.size() != 1 || d2r[0] != 7.0 || pivr.size() != 1 || pivr[0] != 7.0 || failr.size() != 1 || !failr[0]) return 6;

  std::ofstream out(argv[2]);
  out << std::setprecision(17);
  out << done << "\n" << desc << "\n" << desc2 << "\n";
  for (auto& v : verts) out << v.estimate()[0] << " " << v.estimate()[1] << " " << v.estimate()[2] << "\n";
  for (size_t t = 0; t < place.size(); ++t) out << "row " << t << " " << place[t] << "\n";
  for (size_t b = 0; b < groups.size(); ++b) out << "group " << b << " " << d2[b] << " " << piv[b] << " " << (fail[b] ? 1 : 0) << "\n";
  out << "nfail " << nfail << "\nnot_active " << not_active << "\nstale " << stale << "\nlevenberg " << lm << "\nrefused " << refused
      << "\nbad_row " << bad_row << "\n";
  delete opt.algorithm();
  return out.good() ? 0 : 4;
}
