// replay_joint_search.cpp -- SparseOptimizer::sgoJointGreedy and sgoJointExtend through the g2o-compat shim: a pose graph is optimised,
// then a list of candidate closures -- EdgeSE2 objects as replay_candidate_joint.cpp builds them, never added to the graph -- is
// searched greedily from a list of seeds, and the returned orders are put to sgoJointExtend.  Records the estimates, every search's
// result, and what the calls return when they must refuse, for tests/test_gpu_jsearch.py.  Public API only.
//
// build: the line of replay_marginals.cpp with this file's name (tests/test_gpu_jsearch.py builds it itself).
// usage: replay_joint_search graph.txt candidates.txt out.txt iters seeds.txt
//   graph.txt and candidates.txt as replay_candidate_gate.cpp reads them; seeds.txt: first line max_len and the 41 thresholds by
//   count, then one line per seed: count t_0 ... t_{count-1}
//
// out.txt: "done", the backend's description after optimize() and again after the calls (three lines), the V estimates, per seed b:
//   path b stop count order... | d2_path (count + 1 values) | d2_ext (n values)      ext b d2 | d2_ext (n values)
// (ext: sgoJointExtend on the returned order), then  searches N,  nogrowth R (the seeds without thresholds),  unknown_vertex R,
// bad_index R,  twice R,  short_max_len R,  stale R,  levenberg R  (R: what sgoJointGreedy returned for a candidate whose vertex is not
// in the graph, a seed naming candidate n, a seed naming a candidate twice, max_len below a seed's length, after an addVertex without
// initializeOptimization, under Levenberg)
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
  if (argc < 6) return 2;
  std::ifstream in(argv[1]);
  const int iters = std::atoi(argv[4]);
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
  std::vector<Ed> cands;
  {
    std::ifstream cin_(argv[2]);
    Ed c;
    c.closure = 1;
    while (cin_ >> c.i >> c.j) {
      for (double& v : c.z) cin_ >> v;
      for (double& v : c.o) cin_ >> v;
      if (!cin_) return 3;
      cands.push_back(c);
    }
  }
  std::vector<std::vector<int>> seeds;
  std::vector<double> chi2(41);
  int max_len = 0;
  {
    std::ifstream sin_(argv[5]);
    sin_ >> max_len;
    for (double& x : chi2) sin_ >> x;
    int cnt;
    while (sin_ >> cnt) {
      std::vector<int> idx((size_t)cnt);
      for (int& t : idx) sin_ >> t;
      if (!sin_) return 3;
      seeds.push_back(idx);
    }
  }
  dcs_kernel.setDelta(delta);

  std::deque<g2o::VertexSE2, Eigen::aligned_allocator<g2o::VertexSE2>> verts;
  std::deque<g2o::EdgeSE2, Eigen::aligned_allocator<g2o::EdgeSE2>> es, ces;
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
  for (const Ed& e : edges) {
    es.emplace_back();
    fill(&es.back(), e);
    if (e.closure) es.back().setRobustKernel(&dcs_kernel);
    opt.addEdge(&es.back());
  }
  opt.initializeOptimization();
  const int done = opt.optimize(iters);
  const std::string desc = opt.backendDescription();

  std::vector<g2o::EdgeSE2*> list;
  for (const Ed& c : cands) {
    ces.emplace_back();
    fill(&ces.back(), c);
    list.push_back(&ces.back());
  }
  using Path = g2o::SparseOptimizer::SgoJointPath;
  const std::vector<std::vector<bool>> all;
  std::vector<Path> paths, still;
  const int searches = opt.sgoJointGreedy(list, seeds, chi2, max_len, all, &paths);
  if (searches != (int)seeds.size() || paths.size() != seeds.size()) return 5;
  std::vector<std::vector<int>> orders;
  for (const Path& p : paths) orders.push_back(p.order);
  std::vector<double> xd2;
  std::vector<std::vector<double>> xext;
  if (opt.sgoJointExtend(list, orders, &xd2, &xext) != (int)seeds.size() || xd2.size() != seeds.size() || xext.size() != seeds.size()) return 5;
  const int nogrowth = opt.sgoJointGreedy(list, seeds, std::vector<double>(), max_len, all, &still);
  for (size_t b = 0; nogrowth >= 0 && b < seeds.size(); ++b)
    if (still[b].order != seeds[b]) return 5;
  const std::string desc2 = opt.backendDescription();

  // the refusals: none may touch the outputs
  std::vector<Path> keep(1);
  keep[0].stop = 7;
  const std::vector<std::vector<int>> one(1, std::vector<int>(1, 0));
  g2o::VertexSE2 stranger;
  stranger.setId(V);
  stranger.setEstimate(g2o::SE2(0.0, 0.0, 0.0));
  g2o::EdgeSE2 odd;
  odd.vertices()[0] = &verts[1];
  odd.vertices()[1] = &stranger;
  odd.setMeasurement(g2o::SE2(0.0, 0.0, 0.0));
  odd.information() = Eigen::Matrix3d::Identity();
  const int unknown = opt.sgoJointGreedy(std::vector<g2o::EdgeSE2*>(1, &odd), one, chi2, 40, all, &keep);
  const int bad_index = opt.sgoJointGreedy(list, std::vector<std::vector<int>>(1, std::vector<int>(1, (int)list.size())), chi2, 40, all, &keep);
  const int twice = opt.sgoJointGreedy(list, std::vector<std::vector<int>>(1, std::vector<int>(2, 1)), chi2, 40, all, &keep);
  const std::vector<int> three = {0, 1, 2};
  const int short_max_len = opt.sgoJointGreedy(list, std::vector<std::vector<int>>(1, three), chi2, 2, all, &keep);
  opt.addVertex(&stranger);
  const int stale = opt.sgoJointGreedy(list, one, chi2, 40, all, &keep);
  opt.removeVertex(&stranger);
  opt.initializeOptimization();
  g2o::OptimizationAlgorithm* gn = opt.algorithm();
  opt.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));
  const int lm = opt.sgoJointGreedy(list, one, chi2, 40, all, &keep);
  delete opt.algorithm();
  opt.setAlgorithm(gn);
  if (keep.size() != 1 || keep[0].stop != 7 || !keep[0].order.empty()) return 6;

  std::ofstream out(argv[3]);
  out << std::setprecision(17);
  out << done << "\n" << desc << "\n" << desc2 << "\n";
  for (auto& v : verts) out << v.estimate()[0] << " " << v.estimate()[1] << " " << v.estimate()[2] << "\n";
  for (size_t b = 0; b < seeds.size(); ++b) {
    const Path& p = paths[b];
    out << "path " << b << " " << p.stop << " " << p.order.size();
    for (int t : p.order) out << " " << t;
    out << " |";
    for (double v : p.d2Path) out << " " << v;
    out << " |";
    for (double v : p.d2Ext) out << " " << v;
    out << "\next " << b << " " << xd2[b] << " |";
    for (double v : xext[b]) out << " " << v;
    out << "\n";
  }
  out << "searches " << searches << "\nnogrowth " << nogrowth << "\nunknown_vertex " << unknown << "\nbad_index " << bad_index << "\ntwice " << twice
      << "\nshort_max_len " << short_max_len << "\nstale " << stale << "\nlevenberg " << lm << "\n";
  delete opt.algorithm();
  return out.good() ? 0 : 4;
}
