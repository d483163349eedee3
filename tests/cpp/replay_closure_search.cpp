// replay_closure_search.cpp -- SparseOptimizer::sgoClosureSearch through the g2o-compat shim, in the place of the reference's
// shortlist filter (src/sparse_gslam/src/submap_loop_closer.cpp:147-155: every submap pose whose estimate lies within
// max_match_distance of the query pose is matched, with a fixed search window).  A pose graph is optimised, then every pose is
// offered as a submap pose for the last pose: once through the reference's Euclidean threshold, once through the covariance-aware
// search.  Records the estimates and both shortlists for tests/test_gpu_closure_search.py.  Public API only.
//
// build: the line of replay_edge_loo.cpp with this file's name (tests/test_gpu_closure_search.py builds it itself).
// usage: replay_closure_search graph.txt out.txt iters max_match_distance chi2_max min_sep
//   graph.txt as tests/test_shim_replay.py writes it (its phi is the kernel's delta)
//
// out.txt: "done", the backend's description after optimize() and again after the search (three lines), the V estimates, one line
// per pose:  pose j euclid m2 sigma_lin sigma_ang near,  then  count N,  by_pointer R,  not_active R,  stale R,  levenberg R,
// refused R  (R: what the call returned through the vertex-pointer overload, for an id that was never added, after an addVertex
// without initializeOptimization, under Levenberg, and for a negative radius)
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
  const double max_match_distance = std::atof(argv[4]), chi2_max = std::atof(argv[5]);
  const int min_sep = std::atoi(argv[6]);
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

  // the reference's filter: the submap poses within max_match_distance of the query pose's estimate
  const int c = V - 1;
  const g2o::SE2 query = verts[(size_t)c].estimate();
  std::vector<int> euclid((size_t)V, 0), all((size_t)V);
  for (int j = 0; j < V; ++j) {
    all[(size_t)j] = j;
    const g2o::SE2 map_pose = verts[(size_t)j].estimate();
    if ((query.translation() - map_pose.translation()).norm() >= max_match_distance) continue;
    euclid[(size_t)j] = 1;
  }
  // ... and the search in its place: the poses that cannot be excluded from lying that close, each with its own window
  std::vector<double> m2, rel, sigma;
  std::vector<bool> near;
  const int count = opt.sgoClosureSearch(std::vector<int>(1, c), all, max_match_distance, chi2_max, min_sep, &m2, &rel, &sigma, &near);
  if (count < 0 || m2.size() != (size_t)V || rel.size() != 3 * (size_t)V || sigma.size() != 2 * (size_t)V || near.size() != (size_t)V) return 5;
  const std::string desc2 = opt.backendDescription();

  // the vertex-pointer overload gives the same answer
  std::vector<const g2o::OptimizableGraph::Vertex*> qv(1, &verts[(size_t)c]), jv;
  for (auto& v : verts) jv.push_back(&v);
  std::vector<double> m2p;
  std::vector<bool> nearp;
  int by_pointer = opt.sgoClosureSearch(qv, jv, max_match_distance, chi2_max, min_sep, &m2p, nullptr, nullptr, &nearp);
  if (by_pointer != count || nearp != near || m2p.size() != m2.size()) by_pointer = -2;
  for (size_t t = 0; by_pointer >= 0 && t < m2.size(); ++t)
    if (!(m2p[t] == m2[t])) by_pointer = -2;

  // the refusals: none may touch the outputs
  std::vector<double> m2r(1, 7.0), sgr(1, 7.0);
  std::vector<bool> nearr(1, true);
  const int not_active = opt.sgoClosureSearch(std::vector<int>(1, c), std::vector<int>(1, V + 5), max_match_distance, chi2_max, min_sep, &m2r, nullptr, &sgr, &nearr);
  const int refused = opt.sgoClosureSearch(std::vector<int>(1, c), all, -1.0, chi2_max, min_sep, &m2r, nullptr, &sgr, &nearr);
  g2o::VertexSE2 stranger;
  stranger.setId(V);
  stranger.setEstimate(g2o::SE2(0.0, 0.0, 0.0));
  opt.addVertex(&stranger);
  const int stale = opt.sgoClosureSearch(std::vector<int>(1, c), all, max_match_distance, chi2_max, min_sep, &m2r, nullptr, &sgr, &nearr);
  opt.removeVertex(&stranger);
  opt.initializeOptimization();
  g2o::OptimizationAlgorithm* gn = opt.algorithm();
  opt.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));
  const int lm = opt.sgoClosureSearch(std::vector<int>(1, c), all, max_match_distance, chi2_max, min_sep, &m2r, nullptr, &sgr, &nearr);
  delete opt.algorithm();
  opt.setAlgorithm(gn);
  if (m2r.size() != 1 || m2r[0] != 7.0 || sgr.size() != 1 || sgr[0] != 7.0 || nearr.size() != 1 || !nearr[0]) return 6;

  std::ofstream out(argv[2]);
  out << std::setprecision(17);
  out << done << "\n" << desc << "\n" << desc2 << "\n";
  for (auto& v : verts) out << v.estimate()[0] << " " << v.estimate()[1] << " " << v.estimate()[2] << "\n";
  for (int j = 0; j < V; ++j)
    out << "pose " << j << " " << euclid[(size_t)j] << " " << m2[(size_t)j] << " " << sigma[2 * (size_t)j] << " " << sigma[2 * (size_t)j + 1] << " "
        << (near[(size_t)j] ? 1 : 0) << "\n";
  out << "count " << count << "\nby_pointer " << by_pointer << "\nnot_active " << not_active << "\nstale " << stale << "\nlevenberg " << lm
      << "\nrefused " << refused << "\n";
  delete opt.algorithm();
  return out.good() ? 0 : 4;
}
