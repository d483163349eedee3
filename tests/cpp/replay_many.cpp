// replay_many.cpp -- a back-end with several maps: each graph file becomes a SparseOptimizer of VertexSE2 / EdgeSE2 under
// Gauss-Newton, built as the reference builds its own (setup_pose_opt), and the loop
//     for (auto* o : optimisers) o->optimize(iters);
// is replaced by SparseOptimizer::sgoOptimizeMany(optimisers, iters).  With "loop" as the mode the program runs that loop instead,
// so that tests/test_gpu_many.py can compare the two.  Writes, per graph, the iterations returned, the backend's description and
// the estimates as bit patterns.  Public API only.
//
// usage: replay_many many|loop iters out.txt graph.txt...          (graph.txt as tests/test_shim_replay.py writes it)
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "g2o/core/block_solver.h"
#include "g2o/core/optimization_algorithm_gauss_newton.h"
#include "g2o/core/robust_kernel_impl.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam2d/edge_se2.h"
#include "g2o/types/slam2d/vertex_se2.h"

namespace {

Eigen::Matrix3d info_from(const double* u) {
  Eigen::Matrix3d O;
  O << u[0], u[1], u[2], u[1], u[3], u[4], u[2], u[4], u[5];
  return O;
}

struct Map {
  g2o::RobustKernelDCS kernel;
  std::deque<g2o::VertexSE2, Eigen::aligned_allocator<g2o::VertexSE2>> vs;
  std::deque<g2o::EdgeSE2, Eigen::aligned_allocator<g2o::EdgeSE2>> es;
  g2o::SparseOptimizer opt;

  bool load(const char* path) {
    std::ifstream in(path);
    int V, E;
    double phi;
    in >> V >> E >> phi;
    if (!in) return false;
    std::vector<double> poses(3 * (size_t)V);
    for (auto& v : poses) in >> v;
    kernel.setDelta(phi);
    using SlamBlockSolver = g2o::BlockSolver<g2o::BlockSolverTraits<3, 3>>;
    using SlamLinearSolver = g2o::LinearSolverEigen<SlamBlockSolver::PoseMatrixType>;
    opt.setAlgorithm(new g2o::OptimizationAlgorithmGaussNewton(g2o::make_unique<SlamBlockSolver>(g2o::make_unique<SlamLinearSolver>())));
    vs.resize(V);
    es.resize(E);
    for (int k = 0; k < V; ++k) {
      vs[k].setId(k);
      vs[k].setEstimate(g2o::SE2(poses[3 * k], poses[3 * k + 1], poses[3 * k + 2]));
      vs[k].setFixed(k == 0);
      opt.addVertex(&vs[k]);
    }
    for (int k = 0; k < E; ++k) {
      int i, j, closure;
      double z[3], o[6];
      in >> i >> j >> closure;
      for (double& v : z) in >> v;
      for (double& v : o) in >> v;
      es[k].vertices()[0] = &vs[i];
      es[k].vertices()[1] = &vs[j];
      es[k].setMeasurement(g2o::SE2(z[0], z[1], z[2]));
      es[k].information() = info_from(o);
      if (closure) es[k].setRobustKernel(&kernel);
      opt.addEdge(&es[k]);
    }
    return (bool)in && opt.initializeOptimization();
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const bool many = std::strcmp(argv[1], "many") == 0;
  const int iters = std::atoi(argv[2]);
  std::vector<std::unique_ptr<Map>> maps;
  std::vector<g2o::SparseOptimizer*> optimisers;
  for (int a = 4; a < argc; ++a) {
    maps.emplace_back(new Map());
    if (!maps.back()->load(argv[a])) return 3;
    optimisers.push_back(&maps.back()->opt);
  }
  std::vector<int> done;
  if (many) {
    done = g2o::SparseOptimizer::sgoOptimizeMany(optimisers, iters);
  } else {
    for (g2o::SparseOptimizer* o : optimisers) done.push_back(o->optimize(iters));
  }
  std::ofstream out(argv[3]);
  out << std::hex;
  for (size_t m = 0; m < maps.size(); ++m) {
    out << std::dec << done[m] << " " << maps[m]->vs.size() << "\n" << maps[m]->opt.backendDescription() << "\n" << std::hex;
    for (auto& v : maps[m]->vs) {
      for (int q = 0; q < 3; ++q) {
        const double x = v.estimate()[q];
        uint64_t u;
        std::memcpy(&u, &x, sizeof(u));
        out << u << (q < 2 ? " " : "\n");
      }
    }
    delete maps[m]->opt.algorithm();
  }
  return out.good() ? 0 : 4;
}
