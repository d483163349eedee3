// replay_candidate_joint.cpp -- SparseOptimizer::sgoCandidateJoint through the g2o-compat shim: a pose graph is optimised, then a list
// of candidate closures -- EdgeSE2 objects as replay_candidate_gate.cpp builds them, never added to the graph -- and a list of subsets
// of them are put to the joint-compatibility test.  Records the estimates, d2 and the decision of every subset, and what the call
// returns when it must refuse, for tests/test_gpu_joint.py.  Public API only.
//
// build: the line of replay_marginals.cpp with this file's name (tests/test_gpu_joint.py builds it itself).
// usage: replay_candidate_joint graph.txt candidates.txt out.txt iters subsets.txt
//   graph.txt and candidates.txt as replay_candidate_gate.cpp reads them; subsets.txt: one line per subset,
//   chi2_max count t_0 ... t_{count-1}
//
// out.txt: "done", the backend's description after optimize() and again after the call (three lines), the V estimates, one line
// per subset:  sub b d2 pass,  then  npass N,  nodecision R (the same subsets without bounds),  unknown_vertex R,  bad_index R,
// oversize R,  stale R,  levenberg R  (R: what the call returned for a candidate whose vertex is not in the graph, a subset naming
// candidate n, a subset of 41 candidates, after an addVertex without initializeOptimization, under Levenberg)
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
  std::vector<std::vector<int>> subsets;
  std::vector<double> chi2;
  {
    std::ifstream sin_(argv[5]);
    double x;
    int cnt;
    while (sin_ >> x >> cnt) {
      std::vector<int> idx((size_t)cnt);
      for (int& t : idx) sin_ >> t;
      if (!sin_) return 3;
      chi2.push_back(x);
      subsets.push_back(idx);
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
  std::vector<double> d2, d2n;
  std::vector<bool> pass, passn(3, true);
  const int npass = opt.sgoCandidateJoint(list, subsets, chi2, &d2, &pass);
  if (npass < 0 || d2.size() != subsets.size() || pass.size() != subsets.size()) return 5;
  const int nodecision = opt.sgoCandidateJoint(list, subsets, std::vector<double>(), &d2n, &passn);
  if (nodecision != 0 || d2n != d2 || !passn.empty()) return 5;
  const std::string desc2 = opt.backendDescription();

  // the refusals: none may touch the outputs
  std::vector<double> d2r(1, 7.0);
  std::vector<bool> passr(1, true);
  const std::vector<std::vector<int>> one(1, std::vector<int>(1, 0));
  const std::vector<double> chi1(1, 1.0);
  g2o::VertexSE2 stranger;
  stranger.setId(V);
  stranger.setEstimate(g2o::SE2(0.0, 0.0, 0.0));
  g2o::EdgeSE2 odd;
  odd.vertices()[0] = &verts[1];
  odd.vertices()[1] = &stranger;
  odd.setMeasurement(g2o::SE2(0.0, 0.0, 0.0));
  odd.information() = Eigen::Matrix3d::Identity();
  const int unknown = opt.sgoCandidateJoint(std::vector<g2o::EdgeSE2*>(1, &odd), one, chi1, &d2r, &passr);
  const int bad_index = opt.sgoCandidateJoint(list, std::vector<std::vector<int>>(1, std::vector<int>(1, (int)list.size())), chi1, &d2r, &passr);
  std::vector<int> big;
  for (int t = 0; t < 41 && t < (int)list.size(); ++t) big.push_back(t);
  const int oversize = big.size() == 41 ? opt.sgoCandidateJoint(list, std::vector<std::vector<int>>(1, big), chi1, &d2r, &passr) : -1;
  opt.addVertex(&stranger);
  const int stale = opt.sgoCandidateJoint(list, one, chi1, &d2r, &passr);
  opt.removeVertex(&stranger);
  opt.initializeOptimization();
  g2o::OptimizationAlgorithm* gn = opt.algorithm();
  opt.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));
  const int lm = opt.sgoCandidateJoint(list, one, chi1, &d2r, &passr);
  delete opt.algorithm();
  opt.setAlgorithm(gn);
  if (d2r.size() != 1 || d2r[0] != 7.0 || passr.size() != 1 || !passr[0]) return 6;

  std::ofstream out(argv[3]);
  out << std::setprecision(17);
  out << done << "\n" << desc << "\n" << desc2 << "\n";
  for (auto& v : verts) out << v.estimate()[0] << " " << v.estimate()[1] << " " << v.estimate()[2] << "\n";
  for (size_t b = 0; b < subsets.size(); ++b) out << "sub " << b << " " << d2[b] << " " << (pass[b] ? 1 : 0) << "\n";
  out << "npass " << npass << "\nnodecision " << nodecision << "\nunknown_vertex " << unknown << "\nbad_index " << bad_index << "\noversize " << oversize
      << "\nstale " << stale << "\nlevenberg " << lm << "\n";
  delete opt.algorithm();
  return out.good() ? 0 : 4;
}
