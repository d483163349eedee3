// replay_dogleg.cpp -- a VertexSE2 / EdgeSE2 pose graph (no kernels) under OptimizationAlgorithmDogleg through the g2o-compatible
// header.  The shim sends the graph to the library's sgo_optimize_dogleg and, when the multifrontal analysis refuses it, to
// sgo_optimize_dogleg_pcg; the program then makes the same calls through the C-ABI on a context of its own, from the same arrays, and
// compares bit for bit: the iteration count, doglegTrace() against the call's stats, the estimates against sgo_get_poses.  For
// tests/test_shim_dogleg.py.
//
// usage: replay_dogleg graph.txt out.txt iterations     (graph.txt as tests/test_shim_replay.py writes it)
// out.txt: "<optimize()'s return> <sgo_optimize_dogleg's return> <the return of the call that ran> <trace equal> <estimates equal>",
//          the backend's description, the trace's length, one line "delta chi2 trials step" per iteration
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "g2o/core/block_solver.h"
#include "g2o/core/optimization_algorithm_dogleg.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam2d/edge_se2.h"
#include "g2o/types/slam2d/vertex_se2.h"
#include "sgo.h"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int iterations = std::atoi(argv[3]);
  std::ifstream in(argv[1]);
  int V, E;
  double phi;
  in >> V >> E >> phi;
  std::vector<double> poses(3 * (size_t)V), meas(3 * (size_t)E), info(6 * (size_t)E), none((size_t)E, -1.0);
  std::vector<int32_t> ei(E), ej(E);
  for (auto& v : poses) in >> v;
  for (int k = 0; k < E; ++k) {
    int closure;
    in >> ei[k] >> ej[k] >> closure;
    for (int q = 0; q < 3; ++q) in >> meas[3 * (size_t)k + q];
    for (int q = 0; q < 6; ++q) in >> info[6 * (size_t)k + q];
  }
  if (!in) return 3;

  std::deque<g2o::VertexSE2, Eigen::aligned_allocator<g2o::VertexSE2>> vs(V);
  std::deque<g2o::EdgeSE2, Eigen::aligned_allocator<g2o::EdgeSE2>> es(E);
  g2o::SparseOptimizer opt;
  using SlamBlockSolver = g2o::BlockSolver<g2o::BlockSolverTraits<3, 3>>;
  using SlamLinearSolver = g2o::LinearSolverEigen<SlamBlockSolver::PoseMatrixType>;
  std::unique_ptr<g2o::OptimizationAlgorithm> dl(
      new g2o::OptimizationAlgorithmDogleg(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));
  opt.setAlgorithm(dl.get());
  for (int k = 0; k < V; ++k) {
    vs[k].setId(k);
    vs[k].setEstimate(g2o::SE2(poses[3 * k], poses[3 * k + 1], poses[3 * k + 2]));
    vs[k].setFixed(k == 0);
    opt.addVertex(&vs[k]);
  }
  for (int k = 0; k < E; ++k) {
    const double* u = &info[6 * (size_t)k];
    Eigen::Matrix3d O;
    O << u[0], u[1], u[2], u[1], u[3], u[4], u[2], u[4], u[5];
    es[k].vertices()[0] = &vs[ei[k]];
    es[k].vertices()[1] = &vs[ej[k]];
    es[k].setMeasurement(g2o::SE2(meas[3 * k], meas[3 * k + 1], meas[3 * k + 2]));
    es[k].information() = O;
    opt.addEdge(&es[k]);
  }
  opt.initializeOptimization();
  const int its = opt.optimize(iterations);
  const std::string desc = opt.backendDescription();
  const auto& trace = opt.doglegTrace();

  std::vector<uint8_t> fixed((size_t)V, 0);
  fixed[0] = 1;
  sgo_ctx* c = sgo_create(-1, nullptr);
  if (!c) return 6;
  if (sgo_set_graph_se2(c, V, poses.data(), fixed.data(), E, ei.data(), ej.data(), meas.data(), info.data(), none.data()) != SGO_OK) return 7;
  std::unique_ptr<sgo_dogleg_stats> st(new sgo_dogleg_stats());
  const int factor = sgo_optimize_dogleg(c, iterations, 0.0, st.get());
  int abi = factor;
  if (factor == SGO_ENOTHING) abi = sgo_optimize_dogleg_pcg(c, iterations, 0.0, st.get());
  std::vector<double> P(3 * (size_t)V);
  if (sgo_get_poses(c, P.data()) != SGO_OK) return 8;
  int trace_equal = abi >= 0 && (size_t)st->iters_done == trace.size();
  for (size_t k = 0; trace_equal && k < trace.size(); ++k)
    trace_equal = std::memcmp(&trace[k].delta, &st->delta[k], 8) == 0 && std::memcmp(&trace[k].chi2, &st->robust_chi2[k + 1], 8) == 0 &&
                  trace[k].trials == st->trials[k] && trace[k].step == st->step_kind[k];
  int poses_equal = 1;
  for (int k = 0; k < V; ++k)
    for (int q = 0; q < 3; ++q) {
      const double v = vs[k].estimate()[q];
      poses_equal = poses_equal && std::memcmp(&v, &P[3 * (size_t)k + q], 8) == 0;
    }
  sgo_destroy(c);

  std::ofstream out(argv[2]);
  out << std::setprecision(17);
  out << its << " " << factor << " " << abi << " " << trace_equal << " " << poses_equal << "\n" << desc << "\n" << trace.size() << "\n";
  for (const auto& t : trace) out << t.delta << " " << t.chi2 << " " << t.trials << " " << t.step << "\n";
  return out.good() ? 0 : 4;
}
