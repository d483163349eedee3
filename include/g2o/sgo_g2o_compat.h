// sgo_g2o_compat.h -- header-only C++ mirror of the g2o API surface that sparse-gslam uses,
// implemented over the C-ABI of libsgo (include/sgo.h).  The individual g2o header paths
// (g2o/core/sparse_optimizer.h, g2o/types/slam2d/edge_se2.h, ...) include this file, so the
// reference's sources keep their #include lines (src/sparse_gslam/include/graphs.h:2-4,
// src/sparse_gslam/src/graphs.cpp:3-7, src/sparse_gslam/src/submap_loop_closer.cpp:8-9,
// src/sparse_gslam/include/delta_vector.h:2, include/g2o_bindings/*.h).
//
// Semantics mirrored (upstream g2o 2020.5.29):
//   * the caller owns vertices, edges, kernels and the algorithm object; nothing is deleted here
//     (README.md:22-23 G2O_DELETE_IMPLICITLY_OWNED_OBJECTS 0; graphs.cpp:29,36 delete the
//     algorithm before ~SparseOptimizer runs);
//   * add*/remove* return bool, optimize() returns the iteration count (0: solver failed,
//     -1: nothing to optimise); diagnostics go to std::cerr; no exceptions;
//   * initializeOptimization(): active vertices = graph vertices with at least one edge whose
//     vertices are all in the graph, sorted by id; active edges in insertion order; hessian
//     indices = non-fixed active vertices in ascending id;
//   * HyperGraph::clear() empties the graph's containers but not each vertex's own edges() set;
//   * activeChi2() is the un-robustified sum, activeRobustChi2() the robustified one.
//
// Backend: a graph whose active vertices are all VertexSE2 and whose active edges are all EdgeSE2
// (robust kernel: none, RobustKernelDCS or another kernel of robust_kernel_impl.h) optimised with OptimizationAlgorithmGaussNewton -- the
// reference's pose graph (graphs.cpp:17-23), the hot path -- ALWAYS runs on the GPU through
// sgo_optimize_gn; if the device or libsgo is unavailable optimize() fails loudly, there is no
// CPU fallback for it.  Every other combination (the reference's landmark graph: Levenberg,
// BlockSolverTraits<-1,2>, VertexRhoTheta / EdgeSE2RhoTheta with numeric Jacobians, graphs.cpp:9-15,
// drone.cpp:146-187) is a tiny, latency-bound problem (pruned to one pose at every loop closure,
// slc.cpp:257-262) and is solved by the small dense host solver at the end of this file
// ("CPU path of the new backend suffices").
#pragma once

#if defined(__has_include)
#if __has_include(<Eigen/Core>) && !defined(SGO_FORCE_EIGEN_MIN)
#include <Eigen/Core>
#include <Eigen/Geometry>
#include <Eigen/StdVector>
#else
#include "sgo_eigen_min.h"
#endif
#else
#include "sgo_eigen_min.h"
#endif

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <iomanip>
#include <sstream>
#include <string>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <typeinfo>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../sgo.h"

#ifndef G2O_REGISTER_TYPE
#define G2O_REGISTER_TYPE(name, classname)
#endif
#ifndef G2O_ATTRIBUTE_UNUSED
#define G2O_ATTRIBUTE_UNUSED __attribute__((unused))
#endif

namespace g2o {

using number_t = double;
using Vector2 = Eigen::Matrix<double, 2, 1>;
using Vector3 = Eigen::Matrix<double, 3, 1>;
using Matrix3 = Eigen::Matrix<double, 3, 3>;
using MatrixX = Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic>;
using Rotation2D = Eigen::Rotation2D<double>;

template <class T, class... A>
std::unique_ptr<T> make_unique(A&&... a) {
  return std::unique_ptr<T>(new T(std::forward<A>(a)...));
}

inline constexpr double const_pi() { return 3.14159265358979323846; }

// g2o/stuff/misc.h
inline double normalize_theta(double theta) {
  if (theta >= -const_pi() && theta < const_pi()) return theta;
  double multiplier = std::floor(theta / (2 * const_pi()));
  theta = theta - multiplier * 2 * const_pi();
  if (theta >= const_pi()) theta -= 2 * const_pi();
  if (theta < -const_pi()) theta += 2 * const_pi();
  return theta;
}

// ------------------------------------------------------------------------------- SE2
class SE2 {
 public:
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  SE2() : _R(0), _t(0, 0) {}
  SE2(double x, double y, double theta) : _R(theta), _t(x, y) {}
  const Vector2& translation() const { return _t; }
  void setTranslation(const Vector2& t) { _t = t; }
  const Rotation2D& rotation() const { return _R; }
  void setRotation(const Rotation2D& R) { _R = R; }

  SE2 operator*(const SE2& tr2) const {
    SE2 result(*this);
    result *= tr2;
    return result;
  }
  SE2& operator*=(const SE2& tr2) {
    _t = _t + _R * tr2._t;
    _R.angle() += tr2._R.angle();
    _R.angle() = normalize_theta(_R.angle());
    return *this;
  }
  Vector2 operator*(const Vector2& v) const { return _t + _R * v; }
  SE2 inverse() const {
    SE2 ret;
    ret._R = _R.inverse();
    ret._R.angle() = normalize_theta(ret._R.angle());
    ret._t = ret._R * (Vector2(-_t[0], -_t[1]));
    return ret;
  }
  double operator[](int i) const {
    assert(i >= 0 && i < 3);
    if (i < 2) return _t[i];
    return _R.angle();
  }
  void fromVector(const Vector3& v) { *this = SE2(v[0], v[1], v[2]); }
  Vector3 toVector() const { return Vector3(_t[0], _t[1], _R.angle()); }

 protected:
  Rotation2D _R;
  Vector2 _t;
};

// ------------------------------------------------------------------------------- graph
class SparseOptimizer;
class RobustKernel;

class HyperGraph {
 public:
  class Edge;
  class Vertex {
   public:
    explicit Vertex(int id = -1) : _id(id) {}
    virtual ~Vertex() {}
    int id() const { return _id; }
    virtual void setId(int id) { _id = id; }
    const std::set<Edge*>& edges() const { return _edges; }
    std::set<Edge*>& edges() { return _edges; }

   protected:
    int _id;
    std::set<Edge*> _edges;
  };
  class Edge {
   public:
    explicit Edge(int id = -1) : _id(id) {}
    virtual ~Edge() {}
    const std::vector<Vertex*>& vertices() const { return _vertices; }
    std::vector<Vertex*>& vertices() { return _vertices; }
    const Vertex* vertex(size_t i) const { return _vertices[i]; }
    Vertex* vertex(size_t i) { return _vertices[i]; }
    void setVertex(size_t i, Vertex* v) { _vertices[i] = v; }
    int id() const { return _id; }
    void setId(int id) { _id = id; }
    long long internalId() const { return _internalId; }

   protected:
    friend class HyperGraph;
    friend class SparseOptimizer;
    std::vector<Vertex*> _vertices;
    int _id;
    long long _internalId = -1;
  };
  using VertexSet = std::set<Vertex*>;
  using EdgeSet = std::set<Edge*>;
  using VertexIDMap = std::unordered_map<int, Vertex*>;
  using VertexContainer = std::vector<Vertex*>;
  using EdgeContainer = std::vector<Edge*>;
};

class OptimizableGraph : public HyperGraph {
 public:
  class Vertex : public HyperGraph::Vertex {
   public:
    virtual ~Vertex() {}
    bool fixed() const { return _fixed; }
    void setFixed(bool f) { _fixed = f; }
    int hessianIndex() const { return _hessianIndex; }
    void setHessianIndex(int i) { _hessianIndex = i; }
    int colInHessian() const { return _colInHessian; }
    void setColInHessian(int c) { _colInHessian = c; }
    int tempIndex() const { return _tempIndex; }
    void setTempIndex(int t) { _tempIndex = t; }
    virtual int dimension() const = 0;
    virtual void oplus(const double* v) = 0;
    virtual void push() = 0;
    virtual void pop() = 0;
    virtual void discardTop() = 0;
    virtual void setToOrigin() = 0;

   protected:
    bool _fixed = false;
    int _hessianIndex = -1;
    int _colInHessian = -1;
    int _tempIndex = -1;
  };
  class Edge : public HyperGraph::Edge {
   public:
    virtual ~Edge() {}
    virtual int dimension() const = 0;
    virtual void computeError() = 0;
    virtual double chi2() const = 0;
    virtual void linearizeOplus() = 0;
    // adds this edge's J^T W J / -J^T W e into the dense normal equations (row-major H, ld = n)
    virtual void constructQuadraticForm(double* H, int n, double* b) = 0;
    RobustKernel* robustKernel() const { return _robustKernel; }
    void setRobustKernel(RobustKernel* k) { _robustKernel = k; }
    int level() const { return _level; }
    void setLevel(int l) { _level = l; }

   protected:
    RobustKernel* _robustKernel = nullptr;
    int _level = 0;
  };
};

// g2o/core/robust_kernel.h / robust_kernel_impl.h
class RobustKernel {
 public:
  RobustKernel() : _delta(1.) {}
  virtual ~RobustKernel() {}
  virtual void robustify(double squaredError, Vector3& rho) const = 0;
  virtual void setDelta(double delta) { _delta = delta; }
  double delta() const { return _delta; }

 protected:
  double _delta;
};
class RobustKernelDCS : public RobustKernel {
 public:
  void robustify(double e2, Vector3& rho) const override {
    const double& phi = _delta;
    double scale = (2.0 * phi) / (phi + e2);
    if (scale >= 1.0) {
      rho[0] = e2;
      rho[1] = 1.;
      rho[2] = 0;
    } else {
      rho[0] = scale * e2 * scale;
      rho[1] = (scale * scale);
      rho[2] = 0;
    }
  }
};
// The other kernels of robust_kernel_impl.h that the GPU path evaluates (include/sgo.h lists the pairs rho[0], rho[1]; the
// SGO_KERNEL_* number of a class is sgoRobustKernelKind's).  rho[2] as g2o has it: nothing here reads it (robustInformation is
// rho[1] Omega, the second-order term is disabled upstream).
class RobustKernelHuber : public RobustKernel {
 public:
  void robustify(double e, Vector3& rho) const override {
    const double dsqr = _delta * _delta;
    if (e <= dsqr) {
      rho[0] = e;
      rho[1] = 1.;
      rho[2] = 0.;
    } else {
      const double sqrte = std::sqrt(e);
      rho[0] = 2 * sqrte * _delta - dsqr;
      rho[1] = _delta / sqrte;
      rho[2] = -0.5 * rho[1] / e;
    }
  }
};
class RobustKernelPseudoHuber : public RobustKernel {
 public:
  void robustify(double e2, Vector3& rho) const override {
    const double dsqr = _delta * _delta;
    const double aux = std::sqrt(1 + e2 / dsqr);
    rho[0] = 2 * dsqr * (aux - 1);
    rho[1] = 1. / aux;
    rho[2] = -0.5 / dsqr * rho[1] / (aux * aux);
  }
};
class RobustKernelCauchy : public RobustKernel {
 public:
  void robustify(double e2, Vector3& rho) const override {
    const double dsqr = _delta * _delta;
    const double aux = 1 + e2 / dsqr;
    rho[0] = dsqr * std::log(aux);
    rho[1] = 1. / aux;
    rho[2] = -1. / dsqr * rho[1] * rho[1];
  }
};
class RobustKernelGemanMcClure : public RobustKernel {
 public:
  void robustify(double e2, Vector3& rho) const override {
    const double aux = 1. / (1. + e2);
    rho[0] = e2 * aux;
    rho[1] = aux * aux;
    rho[2] = -2. * rho[1] * aux;
  }
};
class RobustKernelWelsch : public RobustKernel {
 public:
  void robustify(double e2, Vector3& rho) const override {
    const double dsqr = _delta * _delta;
    const double aux = std::exp(-e2 / dsqr);
    rho[0] = dsqr * (1. - aux);
    rho[1] = aux;
    rho[2] = -aux / dsqr;
  }
};
class RobustKernelFair : public RobustKernel {
 public:
  void robustify(double e2, Vector3& rho) const override {
    const double sqrte = std::sqrt(e2);
    const double aux = sqrte / _delta;
    rho[0] = 2. * _delta * _delta * (aux - std::log1p(aux));
    rho[1] = 1. / (1. + aux);
    rho[2] = sqrte > 0. ? -0.5 / (sqrte * (_delta + sqrte) * (1. + aux)) : 0.;
  }
};
class RobustKernelTukey : public RobustKernel {
 public:
  void robustify(double e2, Vector3& rho) const override {
    const double e = std::sqrt(e2);
    const double delta2 = _delta * _delta;
    if (e <= _delta) {
      const double aux = 1. - e2 / delta2;
      rho[0] = delta2 * (1. - aux * aux * aux) / 3.;
      rho[1] = aux * aux;
      rho[2] = -2. * aux / delta2;
    } else {
      rho[0] = delta2 / 3.;
      rho[1] = 0;
      rho[2] = 0;
    }
  }
};
class RobustKernelSaturated : public RobustKernel {
 public:
  void robustify(double e2, Vector3& rho) const override {
    const double dsqr = _delta * _delta;
    if (e2 <= dsqr) {
      rho[0] = e2;
      rho[1] = 1.;
      rho[2] = 0.;
    } else {
      rho[0] = dsqr;
      rho[1] = 0.;
      rho[2] = 0.;
    }
  }
};
// The SGO_KERNEL_* number of a kernel object (nullptr: SGO_KERNEL_NONE); -1 for a subclass the GPU path does not know.
inline int sgoRobustKernelKind(const RobustKernel* k) {
  if (!k) return SGO_KERNEL_NONE;
  const std::type_info& t = typeid(*k);
  if (t == typeid(RobustKernelDCS)) return SGO_KERNEL_DCS;
  if (t == typeid(RobustKernelHuber)) return SGO_KERNEL_HUBER;
  if (t == typeid(RobustKernelPseudoHuber)) return SGO_KERNEL_PSEUDO_HUBER;
  if (t == typeid(RobustKernelCauchy)) return SGO_KERNEL_CAUCHY;
  if (t == typeid(RobustKernelGemanMcClure)) return SGO_KERNEL_GEMAN_MCCLURE;
  if (t == typeid(RobustKernelWelsch)) return SGO_KERNEL_WELSCH;
  if (t == typeid(RobustKernelFair)) return SGO_KERNEL_FAIR;
  if (t == typeid(RobustKernelTukey)) return SGO_KERNEL_TUKEY;
  if (t == typeid(RobustKernelSaturated)) return SGO_KERNEL_SATURATED;
  return -1;
}

// g2o/core/base_vertex.h
template <int D, typename T>
class BaseVertex : public OptimizableGraph::Vertex {
 public:
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  using EstimateType = T;
  static const int Dimension = D;
  int dimension() const override { return D; }
  const EstimateType& estimate() const { return _estimate; }
  void setEstimate(const EstimateType& et) { _estimate = et; }
  void oplus(const double* v) override { oplusImpl(v); }
  void setToOrigin() override { setToOriginImpl(); }
  void push() override { _backup.push_back(_estimate); }
  void pop() override {
    assert(!_backup.empty());
    _estimate = _backup.back();
    _backup.pop_back();
  }
  void discardTop() override {
    assert(!_backup.empty());
    _backup.pop_back();
  }
  int stackSize() const { return (int)_backup.size(); }
  virtual void setToOriginImpl() = 0;
  virtual void oplusImpl(const double* v) = 0;
  virtual bool read(std::istream& is) = 0;
  virtual bool write(std::ostream& os) const = 0;

 protected:
  EstimateType _estimate;
  std::vector<EstimateType, Eigen::aligned_allocator<EstimateType>> _backup;
};

// g2o/core/base_binary_edge.h
template <int D, typename E, typename VertexXi, typename VertexXj>
class BaseBinaryEdge : public OptimizableGraph::Edge {
 public:
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  using Measurement = E;
  using VertexXiType = VertexXi;
  using VertexXjType = VertexXj;
  using ErrorVector = Eigen::Matrix<double, D, 1>;
  using InformationType = Eigen::Matrix<double, D, D>;
  using JacobianXiOplusType = Eigen::Matrix<double, D, VertexXi::Dimension>;
  using JacobianXjOplusType = Eigen::Matrix<double, D, VertexXj::Dimension>;
  static const int Dimension = D;

  BaseBinaryEdge() {
    _vertices.resize(2, nullptr);
    _information = InformationType::Identity();
  }
  int dimension() const override { return D; }
  const Measurement& measurement() const { return _measurement; }
  virtual void setMeasurement(const Measurement& m) { _measurement = m; }
  const InformationType& information() const { return _information; }
  InformationType& information() { return _information; }
  void setInformation(const InformationType& i) { _information = i; }
  const ErrorVector& error() const { return _error; }
  ErrorVector& error() { return _error; }
  double chi2() const override {
    double s = 0;
    for (int r = 0; r < D; ++r)
      for (int c = 0; c < D; ++c) s += _error[r] * _information(r, c) * _error[c];
    return s;
  }
  const JacobianXiOplusType& jacobianOplusXi() const { return _jacobianOplusXi; }
  const JacobianXjOplusType& jacobianOplusXj() const { return _jacobianOplusXj; }

  // numeric Jacobian by central differences (g2o's default when a subclass only defines
  // computeError, e.g. src/sparse_gslam/src/g2o_bindings/edge_se2_rhotheta.cpp:9-16)
  void linearizeOplus() override {
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    ErrorVector errorBak = _error;
    for (int side = 0; side < 2; ++side) {
      OptimizableGraph::Vertex* v = static_cast<OptimizableGraph::Vertex*>(_vertices[side]);
      if (v->fixed()) continue;
      const int dim = v->dimension();
      std::vector<double> add(dim, 0.0);
      for (int d = 0; d < dim; ++d) {
        v->push();
        add[d] = delta;
        v->oplus(add.data());
        computeError();
        ErrorVector e1 = _error;
        v->pop();
        v->push();
        add[d] = -delta;
        v->oplus(add.data());
        computeError();
        ErrorVector e2 = _error;
        v->pop();
        add[d] = 0.0;
        for (int r = 0; r < D; ++r) {
          const double val = scalar * (e1[r] - e2[r]);
          if (side == 0) _jacobianOplusXi(r, d) = val;
          else _jacobianOplusXj(r, d) = val;
        }
      }
    }
    _error = errorBak;
  }
  // BaseBinaryEdge::constructQuadraticForm (+ robustInformation with the second-order term
  // disabled, as upstream): b -= J^T (rho1 Omega) e ; H += J^T (rho1 Omega) J
  void constructQuadraticForm(double* H, int n, double* b) override {
    OptimizableGraph::Vertex* from = static_cast<OptimizableGraph::Vertex*>(_vertices[0]);
    OptimizableGraph::Vertex* to = static_cast<OptimizableGraph::Vertex*>(_vertices[1]);
    const bool fromNotFixed = !from->fixed(), toNotFixed = !to->fixed();
    if (!fromNotFixed && !toNotFixed) return;
    double w = 1.0;
    if (robustKernel()) {
      Vector3 rho;
      robustKernel()->robustify(chi2(), rho);
      w = rho[1];
    }
    const int Di = VertexXi::Dimension, Dj = VertexXj::Dimension;
    double Oe[D];
    for (int r = 0; r < D; ++r) {
      double s = 0;
      for (int c = 0; c < D; ++c) s += _information(r, c) * _error[c];
      Oe[r] = w * s;
    }
    const int ci = from->colInHessian(), cj = to->colInHessian();
    auto JtOJ = [&](auto& Ja, int da, int ca, auto& Jb, int db, int cb) {
      for (int p = 0; p < da; ++p)
        for (int q = 0; q < db; ++q) {
          double s = 0;
          for (int r = 0; r < D; ++r)
            for (int c = 0; c < D; ++c) s += Ja(r, p) * w * _information(r, c) * Jb(c, q);
          H[(size_t)(ca + p) * n + cb + q] += s;
        }
    };
    if (fromNotFixed) {
      for (int p = 0; p < Di; ++p) {
        double s = 0;
        for (int r = 0; r < D; ++r) s += _jacobianOplusXi(r, p) * Oe[r];
        b[ci + p] -= s;
      }
      JtOJ(_jacobianOplusXi, Di, ci, _jacobianOplusXi, Di, ci);
    }
    if (toNotFixed) {
      for (int p = 0; p < Dj; ++p) {
        double s = 0;
        for (int r = 0; r < D; ++r) s += _jacobianOplusXj(r, p) * Oe[r];
        b[cj + p] -= s;
      }
      JtOJ(_jacobianOplusXj, Dj, cj, _jacobianOplusXj, Dj, cj);
    }
    if (fromNotFixed && toNotFixed) {
      JtOJ(_jacobianOplusXi, Di, ci, _jacobianOplusXj, Dj, cj);
      JtOJ(_jacobianOplusXj, Dj, cj, _jacobianOplusXi, Di, ci);
    }
  }
  virtual bool read(std::istream& is) = 0;
  virtual bool write(std::ostream& os) const = 0;

 protected:
  Measurement _measurement;
  InformationType _information;
  ErrorVector _error;
  JacobianXiOplusType _jacobianOplusXi;
  JacobianXjOplusType _jacobianOplusXj;
};

// ------------------------------------------------------------------------------- slam2d types
class VertexSE2 : public BaseVertex<3, SE2> {
 public:
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  VertexSE2() {}
  void setToOriginImpl() override { _estimate = SE2(); }
  void oplusImpl(const double* update) override {
    Vector2 t = _estimate.translation();
    t[0] += update[0];
    t[1] += update[1];
    double angle = normalize_theta(_estimate.rotation().angle() + update[2]);
    _estimate.setTranslation(t);
    _estimate.setRotation(Rotation2D(angle));
  }
  bool read(std::istream& is) override {
    double x, y, t;
    is >> x >> y >> t;
    _estimate = SE2(x, y, t);
    return true;
  }
  bool write(std::ostream& os) const override {
    os << _estimate[0] << " " << _estimate[1] << " " << _estimate[2];
    return os.good();
  }
};

class EdgeSE2 : public BaseBinaryEdge<3, SE2, VertexSE2, VertexSE2> {
 public:
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  EdgeSE2() {}
  void computeError() override {
    const VertexSE2* v1 = static_cast<const VertexSE2*>(_vertices[0]);
    const VertexSE2* v2 = static_cast<const VertexSE2*>(_vertices[1]);
    SE2 delta = _inverseMeasurement * (v1->estimate().inverse() * v2->estimate());
    _error = delta.toVector();
  }
  void setMeasurement(const SE2& m) override {
    _measurement = m;
    _inverseMeasurement = m.inverse();
  }
  const SE2& inverseMeasurement() const { return _inverseMeasurement; }
  void linearizeOplus() override {
    const VertexSE2* vi = static_cast<const VertexSE2*>(_vertices[0]);
    const VertexSE2* vj = static_cast<const VertexSE2*>(_vertices[1]);
    double thetai = vi->estimate().rotation().angle();
    Vector2 dt = vj->estimate().translation() - vi->estimate().translation();
    double si = std::sin(thetai), ci = std::cos(thetai);
    Matrix3 a, b, z;
    a << -ci, -si, -si * dt[0] + ci * dt[1], si, -ci, -ci * dt[0] - si * dt[1], 0, 0, -1;
    b << ci, si, 0, -si, ci, 0, 0, 0, 1;
    const double tz = _inverseMeasurement.rotation().angle();
    z << std::cos(tz), -std::sin(tz), 0, std::sin(tz), std::cos(tz), 0, 0, 0, 1;
    _jacobianOplusXi = z * a;
    _jacobianOplusXj = z * b;
  }
  // g2o text format of EDGE_SE2 (after the tag and the two vertex ids): dx dy dtheta, then the upper triangle
  // of the information matrix row by row (o11 o12 o13 o22 o23 o33)
  bool read(std::istream& is) override {
    double x, y, t;
    is >> x >> y >> t;
    setMeasurement(SE2(x, y, t));
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j) {
        double v;
        is >> v;
        _information(i, j) = v;
        if (i != j) _information(j, i) = v;
      }
    return !is.fail();
  }
  bool write(std::ostream& os) const override {
    os << _measurement[0] << " " << _measurement[1] << " " << _measurement[2];
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j) os << " " << _information(i, j);
    return os.good();
  }

 protected:
  SE2 _inverseMeasurement;
};

// ------------------------------------------------------------------------------- solver stack
// Only the configuration chain of graphs.cpp:9-23 is mirrored; the objects carry no state.
template <typename MatrixType>
class LinearSolver {
 public:
  virtual ~LinearSolver() {}
};
template <typename MatrixType>
class LinearSolverEigen : public LinearSolver<MatrixType> {};
class Solver {
 public:
  virtual ~Solver() {}
};
template <int P, int L>
struct BlockSolverTraits {
  static const int PoseDim = P;
  static const int LandmarkDim = L;
  struct PoseMatrixType {};
  using LinearSolverType = LinearSolver<PoseMatrixType>;
};
template <typename Traits>
class BlockSolver : public Solver {
 public:
  using PoseMatrixType = typename Traits::PoseMatrixType;
  using LinearSolverType = typename Traits::LinearSolverType;
  explicit BlockSolver(std::unique_ptr<LinearSolverType> ls) : _ls(std::move(ls)) {}

 private:
  std::unique_ptr<LinearSolverType> _ls;
};
class OptimizationAlgorithm {
 public:
  enum Kind { GaussNewton, Levenberg, Dogleg };
  explicit OptimizationAlgorithm(Kind k, std::unique_ptr<Solver> s) : _kind(k), _solver(std::move(s)) {}
  virtual ~OptimizationAlgorithm() {}
  Kind kind() const { return _kind; }

 private:
  Kind _kind;
  std::unique_ptr<Solver> _solver;
};
class OptimizationAlgorithmGaussNewton : public OptimizationAlgorithm {
 public:
  explicit OptimizationAlgorithmGaussNewton(std::unique_ptr<Solver> s) : OptimizationAlgorithm(GaussNewton, std::move(s)) {}
};
class OptimizationAlgorithmLevenberg : public OptimizationAlgorithm {
 public:
  explicit OptimizationAlgorithmLevenberg(std::unique_ptr<Solver> s) : OptimizationAlgorithm(Levenberg, std::move(s)) {}
};
// Powell's dogleg: pose-only SE(2) graphs on the device (sgo_optimize_dogleg / sgo_optimize_dogleg_pcg); there is no host solver for it
class OptimizationAlgorithmDogleg : public OptimizationAlgorithm {
 public:
  explicit OptimizationAlgorithmDogleg(std::unique_ptr<Solver> s) : OptimizationAlgorithm(Dogleg, std::move(s)) {}
};

// g2o/core/sparse_block_matrix.h, as far as SparseOptimizer::computeMarginals' result needs it: the blocks asked for, by hessian
// block index; rows() / cols() count scalars, as upstream
template <class MatrixType = MatrixX>
class SparseBlockMatrix {
 public:
  using SparseMatrixBlock = MatrixType;
  SparseBlockMatrix() {}
  int rows() const { return _rows; }
  int cols() const { return _cols; }
  // the block at block row r, block column c; null when it is absent
  MatrixType* block(int r, int c) {
    auto it = _blocks.find(std::make_pair(r, c));
    return it == _blocks.end() ? nullptr : it->second.get();
  }
  const MatrixType* block(int r, int c) const {
    auto it = _blocks.find(std::make_pair(r, c));
    return it == _blocks.end() ? nullptr : it->second.get();
  }
  void clear(bool = false) { _blocks.clear(); }

 private:
  friend class SparseOptimizer;
  int _rows = 0, _cols = 0;
  std::map<std::pair<int, int>, std::unique_ptr<MatrixType>> _blocks;
};

// ------------------------------------------------------------------------------- actions
// g2o/core/hyper_graph_action.h and sparse_optimizer_terminate_action.h.  The device path does not come back to the host between
// its iterations, so the one post-iteration action there is is the one whose decision the device can take itself:
// SparseOptimizerTerminateAction, evaluated inside sgo_optimize_gn_until (include/sgo.h says the rule); SparseOptimizer refuses any
// other class at addPostIterationAction.
class HyperGraphAction {
 public:
  class Parameters {
   public:
    virtual ~Parameters() {}
  };
  class ParametersIteration : public Parameters {
   public:
    explicit ParametersIteration(int iter) : iteration(iter) {}
    int iteration;
  };
  virtual ~HyperGraphAction() {}
  virtual HyperGraphAction* operator()(const HyperGraph*, Parameters* = nullptr) { return nullptr; }
};

// Stops optimize() once the relative gain of the robust chi2 between two iterations is in [0, gainThreshold), and after the
// iteration with index maxIterations at the latest; the first iteration only records its chi2, so two always run.
class SparseOptimizerTerminateAction : public HyperGraphAction {
 public:
  double gainThreshold() const { return _gainThreshold; }
  void setGainThreshold(double g) { _gainThreshold = g; }
  int maxIterations() const { return _maxIterations; }
  void setMaxIterations(int m) { _maxIterations = m; }
  // how many iterations optimize(n) may run at most: upstream stops AFTER iteration index maxIterations
  int iterationCap(int n) const {
    const int cap = _maxIterations < 0 ? 1 : (_maxIterations < std::numeric_limits<int>::max() ? _maxIterations + 1 : _maxIterations);
    return std::min(n, cap);
  }

 private:
  double _gainThreshold = 1e-6;
  int _maxIterations = std::numeric_limits<int>::max();
};

// ------------------------------------------------------------------------------- optimiser
// What SparseOptimizer::sgoOptimizeHypotheses returns per hypothesis (extension; sgo_optimize_gn_hypotheses of include/sgo.h).
struct SgoHypothesis {
  int iterations = 0;        // updates applied
  int stopReason = 0;        // SGO_STOP_MAX_ITERS / SGO_STOP_GAIN / SGO_STOP_FAILED
  double chi2 = 0.0, robustChi2 = 0.0;                      // at the hypothesis' final poses
  std::map<const OptimizableGraph::Edge*, double> edgeChi2; // e^T Omega e of every active edge there, with the edge's own information
  std::map<int, SE2> poses;                                 // the final poses by vertex id
};

class SparseOptimizer : public OptimizableGraph {
 public:
  SparseOptimizer() {}
  ~SparseOptimizer() {
    if (_ctx) sgo_destroy(_ctx);  // never touches the algorithm, vertices or edges (caller-owned)
  }
  SparseOptimizer(const SparseOptimizer&) = delete;
  SparseOptimizer& operator=(const SparseOptimizer&) = delete;

  void setAlgorithm(OptimizationAlgorithm* a) { _algorithm = a; }
  OptimizationAlgorithm* algorithm() const { return _algorithm; }
  void setVerbose(bool v) { _verbose = v; }
  bool verbose() const { return _verbose; }
  void setComputeBatchStatistics(bool) {}

  // Post-iteration actions: a SparseOptimizerTerminateAction (one at a time; caller-owned, as upstream) makes optimize() end at
  // convergence -- on the device through sgo_optimize_gn_until, on the host solver by the same rule after every iteration.  Any
  // other class is refused: false and one line on std::cerr.
  bool addPostIterationAction(HyperGraphAction* a) {
    if (!a || typeid(*a) != typeid(SparseOptimizerTerminateAction)) {
      std::cerr << "SparseOptimizer::addPostIterationAction: only SparseOptimizerTerminateAction is supported (the device path does not return to the host between iterations); refused" << std::endl;
      return false;
    }
    if (_terminateAction == a) return false;   // (upstream: already in the set)
    if (_terminateAction) {
      std::cerr << "SparseOptimizer::addPostIterationAction: a SparseOptimizerTerminateAction is registered already; refused" << std::endl;
      return false;
    }
    _terminateAction = static_cast<SparseOptimizerTerminateAction*>(a);
    return true;
  }
  bool removePostIterationAction(HyperGraphAction* a) {
    if (!a || a != _terminateAction) return false;
    _terminateAction = nullptr;
    return true;
  }

  // ---- container (OptimizableGraph / HyperGraph)
  bool addVertex(HyperGraph::Vertex* v) {
    if (!v || v->id() < 0) return false;
    if (_vertices.find(v->id()) != _vertices.end()) return false;
    _vertices[v->id()] = v;
    ++_revision;
    return true;
  }
  bool addEdge(HyperGraph::Edge* e) {
    if (!e) return false;
    for (auto* v : e->vertices())
      if (!v) return false;
    if (!_edges.insert(e).second) return false;
    e->_internalId = _nextEdgeId++;
    for (auto* v : e->vertices()) v->edges().insert(e);
    ++_revision;
    return true;
  }
  bool removeEdge(HyperGraph::Edge* e) {
    auto it = _edges.find(e);
    if (it == _edges.end()) return false;
    _edges.erase(it);
    for (auto* v : e->vertices())
      if (v) v->edges().erase(e);
    ++_revision;
    return true;
  }
  bool removeVertex(HyperGraph::Vertex* v, bool = false) {
    auto it = _vertices.find(v->id());
    if (it == _vertices.end() || it->second != v) return false;
    std::set<HyperGraph::Edge*> tmp(v->edges());
    for (auto* e : tmp) removeEdge(e);
    _vertices.erase(it);
    ++_revision;
    return true;
  }
  OptimizableGraph::Vertex* vertex(int id) {
    auto it = _vertices.find(id);
    return it == _vertices.end() ? nullptr : static_cast<OptimizableGraph::Vertex*>(it->second);
  }
  const VertexIDMap& vertices() const { return _vertices; }
  VertexIDMap& vertices() { return _vertices; }
  const EdgeSet& edges() const { return _edges; }
  EdgeSet& edges() { return _edges; }
  void clear() {  // upstream semantics: the vertices' own edge sets are left alone
    _vertices.clear();
    _edges.clear();
    _activeVertices.clear();
    _activeEdges.clear();
    _graphOnDevice = false;
    ++_revision;
  }

  // ---- optimisation
  bool initializeOptimization(int level = 0) {
    (void)level;
    _activeVertices.clear();
    _activeEdges.clear();
    // upstream rule: walk the edge sets OF THE VERTICES that are in the graph (not the graph's own
    // edge container) and activate every edge all of whose vertices are in the graph.  After
    // clear() a re-added vertex still lists its old edges (slc.cpp:259-261); they come back to
    // life only if every endpoint is back in the graph too.
    std::set<HyperGraph::Vertex*> vs;
    std::set<HyperGraph::Edge*> seen;
    std::vector<HyperGraph::Edge*> es;
    for (auto& kv : _vertices) {
      for (auto* e : kv.second->edges()) {
        if (!seen.insert(e).second) continue;
        bool all = true;
        for (auto* v : e->vertices()) {
          auto it = v ? _vertices.find(v->id()) : _vertices.end();
          if (it == _vertices.end() || it->second != v) all = false;
        }
        if (!all) continue;
        // upstream: `allVerticesOK && !e->allVerticesFixed()` -- an edge between fixed vertices is not
        // active (it would count in activeChi2 / activeEdges, drone.cpp:162-165, and nowhere else)
        bool allFixed = true;
        for (auto* v : e->vertices()) allFixed = allFixed && static_cast<OptimizableGraph::Vertex*>(v)->fixed();
        if (allFixed) continue;
        es.push_back(e);
        for (auto* v : e->vertices()) vs.insert(v);
      }
    }
    std::sort(es.begin(), es.end(), [](HyperGraph::Edge* a, HyperGraph::Edge* b) { return a->internalId() < b->internalId(); });
    for (auto* e : es) _activeEdges.push_back(static_cast<OptimizableGraph::Edge*>(e));
    for (auto* v : vs) _activeVertices.push_back(static_cast<OptimizableGraph::Vertex*>(v));
    std::sort(_activeVertices.begin(), _activeVertices.end(),
              [](OptimizableGraph::Vertex* a, OptimizableGraph::Vertex* b) { return a->id() < b->id(); });
    int h = 0;
    for (auto* v : _activeVertices) v->setHessianIndex(v->fixed() ? -1 : h++);
    _activeRevision = _revision;
    // (what the device holds stays known: optimize() marshals the active sets again and compares -- an unchanged graph
    // uploads poses only, a graph that grew by a chain and a closure becomes an incremental update)
    return true;
  }
  // upstream appends the new vertices / edges to the active sets (new vertices get the next hessian indices)
  // and extends the solver's structure; vertices and edges already active keep their place
  bool updateInitialization(HyperGraph::VertexSet& vset, HyperGraph::EdgeSet& eset) {
    std::vector<OptimizableGraph::Vertex*> nv;
    for (auto* hv : vset) {
      auto* v = static_cast<OptimizableGraph::Vertex*>(hv);
      if (std::find(_activeVertices.begin(), _activeVertices.end(), v) == _activeVertices.end()) nv.push_back(v);
    }
    std::vector<OptimizableGraph::Edge*> ne;
    for (auto* he : eset) {
      auto* e = static_cast<OptimizableGraph::Edge*>(he);
      bool all = true, allFixed = true;
      for (auto* v : e->vertices()) {
        auto it = v ? _vertices.find(v->id()) : _vertices.end();
        if (it == _vertices.end() || it->second != v) all = false;
        else allFixed = allFixed && static_cast<OptimizableGraph::Vertex*>(v)->fixed();
      }
      if (!all || allFixed) continue;
      if (std::find(_activeEdges.begin(), _activeEdges.end(), e) == _activeEdges.end()) ne.push_back(e);
      for (auto* v : e->vertices()) {   // an edge activates its vertices (upstream asserts they are in vset)
        auto* ov = static_cast<OptimizableGraph::Vertex*>(v);
        if (std::find(_activeVertices.begin(), _activeVertices.end(), ov) == _activeVertices.end() &&
            std::find(nv.begin(), nv.end(), ov) == nv.end())
          nv.push_back(ov);
      }
    }
    std::sort(nv.begin(), nv.end(), [](OptimizableGraph::Vertex* a, OptimizableGraph::Vertex* b) { return a->id() < b->id(); });
    std::sort(ne.begin(), ne.end(), [](OptimizableGraph::Edge* a, OptimizableGraph::Edge* b) { return a->internalId() < b->internalId(); });
    int h = 0;
    for (auto* v : _activeVertices) h += v->fixed() ? 0 : 1;
    for (auto* v : nv) {
      v->setHessianIndex(v->fixed() ? -1 : h++);
      _activeVertices.push_back(v);
    }
    for (auto* e : ne) _activeEdges.push_back(e);
    _activeRevision = _revision;
    return true;
  }

  // `online` (drone.cpp:155 passes true after updateInitialization): upstream it only decides whether the block
  // structure is rebuilt (BlockSolver::init / buildStructure at iteration 0) or was already extended by
  // updateInitialization -> updateStructure; the numbers are the same either way -- lambda is re-initialised from
  // the diagonal at iteration 0 of every optimize() call in both modes (OptimizationAlgorithmLevenberg::solve).
  // This backend marshals / assembles from the active sets on every call, so the flag has nothing left to select.
  int optimize(int iterations, bool online = false) {
    (void)online;
    if (!_algorithm) {
      std::cerr << "SparseOptimizer::optimize: no algorithm set" << std::endl;
      return -1;
    }
    bool anyFree = false;
    for (auto* v : _activeVertices) anyFree = anyFree || !v->fixed();
    if (_activeVertices.empty() || !anyFree) return -1;
    if (_algorithm->kind() == OptimizationAlgorithm::Dogleg) return deviceDogleg(iterations);
    if (levenbergOnDevice()) return deviceLevenberg(iterations);
    if (!gpuEligible()) return hostOptimize(iterations, online);
    if (!uploadGraph()) return 0;
    sgo_stats* st = new sgo_stats();
    const int done = _terminateAction ? sgo_optimize_gn_until(_ctx, _terminateAction->iterationCap(iterations), _terminateAction->gainThreshold(), st, nullptr)
                                      : sgo_optimize_gn(_ctx, iterations, st);
    return finishDeviceCall(done, iterations, st);
  }
  // ---- many optimisers in one call (extension; sgo_optimize_gn_many of include/sgo.h): what the loop
  //     for (SparseOptimizer* o : optimisers) o->optimize(iters);
  // leaves -- every estimate, every return value (returned in the list's order) -- with the graphs of the single-launch path
  // sharing ONE kernel launch, a workgroup each, instead of taking a launch and a synchronisation each.  Each optimiser's pending
  // upload (its initializeOptimization, changed estimates) is done first, the estimates are written back after the call.  An
  // optimiser whose optimize() is not Gauss-Newton on the device (the landmark graph's host Levenberg, device Levenberg, dogleg),
  // one with a registered terminate action (its threshold is its own), one without a free active vertex and the second entry of
  // an optimiser listed twice run their own optimize(iters), in the list's order, after the shared call; a NULL entry gets -1.
  static std::vector<int> sgoOptimizeMany(const std::vector<SparseOptimizer*>& optimisers, int iters) {
    std::vector<int> done(optimisers.size(), -1);
    std::vector<size_t> shared;
    std::vector<sgo_ctx*> ctxs;
    for (size_t i = 0; i < optimisers.size(); ++i) {
      SparseOptimizer* o = optimisers[i];
      if (!o) continue;
      bool anyFree = false, twice = false;
      for (auto* v : o->_activeVertices) anyFree = anyFree || !v->fixed();
      for (size_t k : shared) twice = twice || optimisers[k] == o;
      if (twice || !o->_algorithm || !o->gpuEligible() || o->_terminateAction || !anyFree) continue;
      if (!o->uploadGraph()) {
        done[i] = 0;
        continue;
      }
      shared.push_back(i);
      ctxs.push_back(o->_ctx);
    }
    if (!shared.empty()) {
      std::vector<std::unique_ptr<sgo_stats>> st(shared.size());
      std::vector<sgo_stats*> stp(shared.size());
      for (size_t k = 0; k < shared.size(); ++k) stp[k] = (st[k] = std::unique_ptr<sgo_stats>(new sgo_stats())).get();
      std::vector<sgo_many_result> res(shared.size());
      const int rc = sgo_optimize_gn_many(ctxs.data(), (int32_t)ctxs.size(), iters, 0.0, stp.data(), res.data(), nullptr);
      if (rc < 0) std::cerr << "SparseOptimizer::sgoOptimizeMany: " << sgo_last_error(ctxs[0]) << std::endl;
      for (size_t k = 0; k < shared.size(); ++k)
        done[shared[k]] = rc < 0 ? 0 : optimisers[shared[k]]->finishDeviceCall(res[k].rc, iters, st[k].release());
    }
    for (size_t i = 0; i < optimisers.size(); ++i)
      if (optimisers[i] && done[i] == -1 && std::find(shared.begin(), shared.end(), i) == shared.end()) done[i] = optimisers[i]->optimize(iters);
    return done;
  }
  // ---- marginal covariances (SparseOptimizer::computeMarginals): the blocks (r, c) of H^-1 by HESSIAN index, as upstream, through
  // sgo_marginals -- three solves per distinct column index (include/sgo.h) --, or through sgo_marginals_selected when more than
  // kSelectedMinColumns distinct columns are asked for (a routing rule, not a measured crossover).  The current estimates are uploaded as optimize()
  // uploads them, and H is the system AT them (upstream inverts the system of its last iteration).  spinv holds the blocks asked
  // for and nothing else.  A graph that takes the host solver has no marginals here: false, with one line on std::cerr.
  static constexpr size_t kSelectedMinColumns = 8;
  bool computeMarginals(SparseBlockMatrix<MatrixX>& spinv, const std::vector<std::pair<int, int>>& blockIndices) {
    if (!_algorithm || !gpuEligible()) {
      std::cerr << "SparseOptimizer::computeMarginals: only the device path (VertexSE2 / EdgeSE2 under Gauss-Newton) computes marginals"
                << std::endl;
      return false;
    }
    std::vector<int32_t> ofHessian;   // hessian index -> compact vertex number (uploadGraph's numbering)
    for (size_t k = 0; k < _activeVertices.size(); ++k)
      if (_activeVertices[k]->hessianIndex() >= 0) ofHessian.push_back((int32_t)k);
    const int n = (int)ofHessian.size();
    std::vector<int32_t> vi, vj;
    for (const auto& rc : blockIndices) {
      if (rc.first < 0 || rc.first >= n || rc.second < 0 || rc.second >= n) {
        std::cerr << "SparseOptimizer::computeMarginals: block (" << rc.first << ", " << rc.second << ") outside the " << n
                  << " hessian blocks" << std::endl;
        return false;
      }
      vi.push_back(ofHessian[rc.first]);
      vj.push_back(ofHessian[rc.second]);
    }
    if (!uploadGraph()) return false;
    std::vector<double> cov(9 * vi.size());
    // Routing: a request with more than kSelectedMinColumns distinct column vertices asks the selected inversion of the
    // multifrontal factor first (sgo_marginals_selected: about one factorisation whatever the count) and comes back here when the
    // analysis refuses the graph (SGO_ENOTHING) or a pair lies outside the factor's pattern (SGO_EINVAL with nothing written);
    // smaller requests keep the column solves.
    bool answered = false;
    {
      std::vector<int32_t> cols(vj);
      std::sort(cols.begin(), cols.end());
      const size_t distinct = (size_t)(std::unique(cols.begin(), cols.end()) - cols.begin());
      if (distinct > kSelectedMinColumns)
        answered = sgo_marginals_selected(_ctx, nullptr, (int32_t)vi.size(), vi.data(), vj.data(), cov.data()) >= 0;
    }
    if (!answered && sgo_marginals(_ctx, (int32_t)vi.size(), vi.data(), vj.data(), cov.data()) < 0) {
      std::cerr << "SparseOptimizer::computeMarginals: " << sgo_last_error(_ctx) << std::endl;
      return false;
    }
    spinv.clear();
    spinv._rows = spinv._cols = 3 * n;
    for (size_t t = 0; t < blockIndices.size(); ++t) {
      std::unique_ptr<MatrixX> B(new MatrixX(3, 3));
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) (*B)(a, b) = cov[9 * t + 3 * a + b];
      spinv._blocks[blockIndices[t]] = std::move(B);
    }
    return true;
  }
  // upstream's convenience overloads: the diagonal block of one vertex, of every vertex of a container (fixed ones are skipped)
  bool computeMarginals(SparseBlockMatrix<MatrixX>& spinv, const OptimizableGraph::Vertex* vertex) {
    if (!vertex || vertex->hessianIndex() < 0) return false;
    return computeMarginals(spinv, std::vector<std::pair<int, int>>(1, std::make_pair(vertex->hessianIndex(), vertex->hessianIndex())));
  }
  bool computeMarginals(SparseBlockMatrix<MatrixX>& spinv, const VertexContainer& vertices) {
    std::vector<std::pair<int, int>> indices;
    for (const HyperGraph::Vertex* hv : vertices) {
      const int h = static_cast<const OptimizableGraph::Vertex*>(hv)->hessianIndex();
      if (h >= 0) indices.push_back(std::make_pair(h, h));
    }
    return computeMarginals(spinv, indices);
  }

  // ---- the innovation gate for candidate closures (extension; sgo_candidate_gate of include/sgo.h): is a candidate compatible with
  // the current estimates AND their uncertainty, before it is inserted?  The candidates are EdgeSE2 objects as the reference builds
  // them before addEdge (slc.cpp:273-280): both vertices set, measurement, information; they are not added to the graph.  (*d2)[t] =
  // e^T (Omega^-1 + J Sigma J^T)^-1 e at the current estimates, (*pass)[t] = d2 <= chi2Max; returns how many pass.  Returns -1 without
  // touching the outputs when the backend does not hold the graph as it stands (vertices or edges added or removed since the last
  // initializeOptimization / updateInitialization), when the graph takes the host solver (Levenberg, other types), when a
  // candidate's vertex is not an active vertex of the graph, or when the call itself refuses (one line on std::cerr).
  int sgoCandidateGate(const std::vector<EdgeSE2*>& candidates, double chi2Max, std::vector<double>* d2, std::vector<bool>* pass) {
    if (!_algorithm || _activeRevision != _revision || _activeVertices.empty() || !gpuEligible()) return -1;
    const size_t n = candidates.size();
    std::vector<int32_t> ci(n), cj(n);
    std::vector<double> meas(3 * n), info(6 * n);
    for (size_t t = 0; t < n; ++t) {
      const EdgeSE2* e = candidates[t];
      if (!e) return -1;
      for (int side = 0; side < 2; ++side) {
        const HyperGraph::Vertex* v = e->vertex(side);
        if (!v) return -1;
        // (the compact number uploadGraph gives: the vertex's place among the active vertices, which are sorted by id)
        auto it = std::lower_bound(_activeVertices.begin(), _activeVertices.end(), v->id(),
                                   [](const OptimizableGraph::Vertex* a, int id) { return a->id() < id; });
        if (it == _activeVertices.end() || *it != v) return -1;
        (side ? cj : ci)[t] = (int32_t)(it - _activeVertices.begin());
      }
      for (int q = 0; q < 3; ++q) meas[3 * t + q] = e->measurement()[q];
      const auto& O = e->information();
      double* o = &info[6 * t];
      o[0] = O(0, 0); o[1] = O(0, 1); o[2] = O(0, 2); o[3] = O(1, 1); o[4] = O(1, 2); o[5] = O(2, 2);
    }
    if (!uploadGraph()) return -1;
    std::vector<double> dd(n);
    std::vector<uint8_t> ok(n);
    const int rc = sgo_candidate_gate(_ctx, (int32_t)n, ci.data(), cj.data(), meas.data(), info.data(), chi2Max, dd.data(), nullptr, ok.data());
    if (rc < 0) {
      std::cerr << "SparseOptimizer::sgoCandidateGate: " << sgo_last_error(_ctx) << std::endl;
      return -1;
    }
    if (d2) d2->assign(dd.begin(), dd.end());
    if (pass) {
      pass->resize(n);
      for (size_t t = 0; t < n; ++t) (*pass)[t] = ok[t] != 0;
    }
    return rc;
  }

  // the listed edges as the device numbers them (sgoEdgeLeaveOneOut, sgoEdgeJoint); false with one line on std::cerr in the
  // situations sgoEdgeLeaveOneOut names
  bool residentEdgeIds(const char* who, const std::vector<OptimizableGraph::Edge*>& edges, std::vector<int32_t>& ids) {
    if (!_algorithm || !gpuEligible()) {
      std::cerr << "SparseOptimizer::" << who << ": only the device path (VertexSE2 / EdgeSE2 under Gauss-Newton) has this test" << std::endl;
      return false;
    }
    if (_activeRevision != _revision || _activeVertices.empty()) {
      std::cerr << "SparseOptimizer::" << who << ": the graph changed since the last initializeOptimization" << std::endl;
      return false;
    }
    std::vector<std::pair<const OptimizableGraph::Edge*, int32_t>> place(_activeEdges.size());   // active edge -> its place in _activeEdges
    for (size_t k = 0; k < _activeEdges.size(); ++k) place[k] = std::make_pair((const OptimizableGraph::Edge*)_activeEdges[k], (int32_t)k);
    std::sort(place.begin(), place.end());
    const size_t n = edges.size();
    ids.assign(n, 0);
    for (size_t t = 0; t < n; ++t) {
      auto it = std::lower_bound(place.begin(), place.end(), std::make_pair((const OptimizableGraph::Edge*)edges[t], (int32_t)0));
      if (!edges[t] || it == place.end() || it->first != edges[t]) {
        std::cerr << "SparseOptimizer::" << who << ": edge " << t << " of the list is not an active edge of the graph" << std::endl;
        return false;
      }
      ids[t] = it->second;
    }
    if (!uploadGraph()) return false;
    // the device's numbering: the records it was set up with, of which the edges that left since are deactivated, not renumbered
    if (_m.nDead > 0) {
      std::vector<int32_t> record;
      for (size_t r = 0; r < _m.dead.size(); ++r)
        if (!_m.dead[r]) record.push_back((int32_t)r);
      for (int32_t& id : ids) id = record[(size_t)id];
    }
    return true;
  }

  // ---- the leave-one-out test of edges that ARE in the graph (extension; sgo_edge_leave_one_out of include/sgo.h): (*d2)[t] is
  // what sgoCandidateGate would say about edges[t] had it never been inserted, at the current estimates, all edges from one selected
  // inversion; (*redundancy)[t] in [0, 1] is 0 for a bridge edge (removing it disconnects the graph), whose d2 is NaN and which
  // never fails; (*fail)[t] = redundancy >= minRedundancy && d2 > chi2Max.  Returns how many fail.  Returns -1 with one line on
  // std::cerr, the outputs untouched, when the graph takes the host solver (Levenberg, other types), when the backend does not hold
  // the graph as it stands (an addVertex / addEdge without initializeOptimization), for an edge that is not an active edge of the
  // graph, and when the call itself refuses (sgo_last_error's text).
  int sgoEdgeLeaveOneOut(const std::vector<OptimizableGraph::Edge*>& edges, double chi2Max, double minRedundancy, std::vector<double>* d2,
                         std::vector<double>* redundancy, std::vector<bool>* fail) {
    std::vector<int32_t> ids;
    if (!residentEdgeIds("sgoEdgeLeaveOneOut", edges, ids)) return -1;
    const size_t n = edges.size();
    std::vector<double> dd(n + 1), rr(n + 1);   // (never a null d2, whatever n)
    std::vector<uint8_t> ff(n + 1);
    const int rc = sgo_edge_leave_one_out(_ctx, (int32_t)n, ids.data(), chi2Max, minRedundancy, dd.data(), rr.data(), nullptr, ff.data());
    if (rc < 0) {
      std::cerr << "SparseOptimizer::sgoEdgeLeaveOneOut: " << sgo_last_error(_ctx) << std::endl;
      return -1;
    }
    if (d2) d2->assign(dd.begin(), dd.begin() + n);
    if (redundancy) redundancy->assign(rr.begin(), rr.begin() + n);
    if (fail) {
      fail->resize(n);
      for (size_t t = 0; t < n; ++t) (*fail)[t] = ff[t] != 0;
    }
    return rc;
  }

  // ---- the covariance-aware closure search (extension; sgo_closure_search of include/sgo.h): every listed vertex j against every
  // query vertex c at the current estimates, from one selected inversion and one panel solve.  With nq queries and n listed
  // vertices, pair (q, t) at q n + t: (*m2) is the squared Mahalanobis distance (1 degree of freedom) from c's position in j's frame
  // to the half-plane that contains the disc of `radius`, (*rel)[3 ..] the pose of c in j's frame, (*sigma)[2 ..] the 1-sigma linear
  // and angular half-widths of a matcher's window in j's frame, (*near) = m2 <= chi2Max && j != c && |j - c| >= minSep, counted in
  // the order of the active vertices (their ids where those are 0 .. V-1).  It replaces a Euclidean distance threshold on the
  // estimates and a fixed search window.  Returns the number of near pairs.  Returns -1 with one line on std::cerr, the outputs
  // untouched, where sgoEdgeLeaveOneOut does, for a vertex that is not an active vertex of the graph, and when the call itself
  // refuses (sgo_last_error's text).
  int sgoClosureSearch(const std::vector<int>& queryIds, const std::vector<int>& ids, double radius, double chi2Max, int minSep,
                       std::vector<double>* m2, std::vector<double>* rel, std::vector<double>* sigma, std::vector<bool>* near) {
    if (!_algorithm || !gpuEligible()) {
      std::cerr << "SparseOptimizer::sgoClosureSearch: only the device path (VertexSE2 / EdgeSE2 under Gauss-Newton) has this search" << std::endl;
      return -1;
    }
    if (_activeRevision != _revision || _activeVertices.empty()) {
      std::cerr << "SparseOptimizer::sgoClosureSearch: the graph changed since the last initializeOptimization" << std::endl;
      return -1;
    }
    const size_t nq = queryIds.size(), n = ids.size();
    std::vector<int32_t> qc(nq + 1), jc(n + 1);   // (never a null list, whatever the counts)
    for (size_t k = 0; k < nq + n; ++k) {
      const int id = k < nq ? queryIds[k] : ids[k - nq];
      // (the compact number uploadGraph gives: the vertex's place among the active vertices, which are sorted by id)
      auto it = std::lower_bound(_activeVertices.begin(), _activeVertices.end(), id,
                                 [](const OptimizableGraph::Vertex* a, int i) { return a->id() < i; });
      if (it == _activeVertices.end() || (*it)->id() != id) {
        std::cerr << "SparseOptimizer::sgoClosureSearch: vertex " << id << " is not an active vertex of the graph" << std::endl;
        return -1;
      }
      (k < nq ? qc[k] : jc[k - nq]) = (int32_t)(it - _activeVertices.begin());
    }
    if (!uploadGraph()) return -1;
    std::vector<double> mm(nq * n + 1), rr(3 * nq * n + 1), ss(2 * nq * n + 1);
    std::vector<uint8_t> nn(nq * n + 1);
    const int rc = sgo_closure_search(_ctx, (int32_t)nq, qc.data(), (int32_t)n, jc.data(), radius, chi2Max, (int32_t)minSep, mm.data(), rr.data(), nullptr,
                                      ss.data(), nn.data());
    if (rc < 0) {
      std::cerr << "SparseOptimizer::sgoClosureSearch: " << sgo_last_error(_ctx) << std::endl;
      return -1;
    }
    if (m2) m2->assign(mm.begin(), mm.begin() + nq * n);
    if (rel) rel->assign(rr.begin(), rr.begin() + 3 * nq * n);
    if (sigma) sigma->assign(ss.begin(), ss.begin() + 2 * nq * n);
    if (near) {
      near->resize(nq * n);
      for (size_t t = 0; t < nq * n; ++t) (*near)[t] = nn[t] != 0;
    }
    return rc;
  }
  // ... with the vertices themselves
  int sgoClosureSearch(const std::vector<const OptimizableGraph::Vertex*>& queries, const std::vector<const OptimizableGraph::Vertex*>& vertices,
                       double radius, double chi2Max, int minSep, std::vector<double>* m2, std::vector<double>* rel, std::vector<double>* sigma,
                       std::vector<bool>* near) {
    std::vector<int> q, j;
    for (size_t k = 0; k < queries.size() + vertices.size(); ++k) {
      const OptimizableGraph::Vertex* v = k < queries.size() ? queries[k] : vertices[k - queries.size()];
      if (!v) {
        std::cerr << "SparseOptimizer::sgoClosureSearch: a null vertex in the lists" << std::endl;
        return -1;
      }
      (k < queries.size() ? q : j).push_back(v->id());
    }
    return sgoClosureSearch(q, j, radius, chi2Max, minSep, m2, rel, sigma, near);
  }

  // ---- the leave-GROUP-out test of clusters of edges that are in the graph (extension; sgo_edge_joint / sgo_edge_groups of
  // include/sgo.h).  sgoEdgeJoint builds the table of the listed edges (at most SGO_JOINT_MAX_CANDIDATES, none twice) at the current
  // estimates and keeps it in the backend; returns their number.  sgoEdgeGroups: groups[b] lists the members of group b (indices
  // into the edges given to sgoEdgeJoint, any order, a repeated index counts once; at most SGO_JOINT_MAX_SUBSET); (*d2)[b] is what
  // sgoCandidateJoint would say about the cluster had it never been inserted, 3 |g| degrees of freedom; (*pivot)[b] in [0, 1] is 0 for a
  // cluster whose removal disconnects the graph, whose d2 is NaN and which never fails; chi2Max empty: no decisions (returns 0,
  // *fail is emptied), else one bound per group and (*fail)[b] = pivot >= minPivot && d2 > chi2Max[b]; returns how many fail.  Both
  // return -1 with one line on std::cerr, the outputs untouched, where sgoEdgeLeaveOneOut does, and sgoEdgeGroups also for an index
  // outside the table and a chi2Max of another length than groups.
  int sgoEdgeJoint(const std::vector<OptimizableGraph::Edge*>& edges) {
    std::vector<int32_t> ids;
    _edgeJointN = 0;
    if (!residentEdgeIds("sgoEdgeJoint", edges, ids)) return -1;
    ids.push_back(0);   // (never a null list, whatever n)
    const int rc = sgo_edge_joint(_ctx, (int32_t)edges.size(), ids.data(), nullptr, nullptr, nullptr);
    if (rc < 0) {
      std::cerr << "SparseOptimizer::sgoEdgeJoint: " << sgo_last_error(_ctx) << std::endl;
      return -1;
    }
    _edgeJointN = edges.size();
    return rc;
  }
  int sgoEdgeGroups(const std::vector<std::vector<int>>& groups, const std::vector<double>& chi2Max, double minPivot, std::vector<double>* d2,
                    std::vector<double>* pivot, std::vector<bool>* fail) {
    if (!_algorithm || !gpuEligible()) {
      std::cerr << "SparseOptimizer::sgoEdgeGroups: only the device path (VertexSE2 / EdgeSE2 under Gauss-Newton) has this test" << std::endl;
      return -1;
    }
    if (_activeRevision != _revision || _activeVertices.empty()) {
      std::cerr << "SparseOptimizer::sgoEdgeGroups: the graph changed since the last initializeOptimization" << std::endl;
      return -1;
    }
    const size_t n = _edgeJointN, B = groups.size();
    if (!chi2Max.empty() && chi2Max.size() != B) {
      std::cerr << "SparseOptimizer::sgoEdgeGroups: " << chi2Max.size() << " bounds for " << B << " groups" << std::endl;
      return -1;
    }
    std::vector<uint8_t> member(B * n + 1, 0);
    for (size_t b = 0; b < B; ++b)
      for (int t : groups[b]) {
        if (t < 0 || (size_t)t >= n) {
          std::cerr << "SparseOptimizer::sgoEdgeGroups: group " << b << " names row " << t << ", the table holds " << n << " edges" << std::endl;
          return -1;
        }
        member[b * n + (size_t)t] = 1;
      }
    std::vector<double> dd(B + 1), pp(B + 1);
    std::vector<uint8_t> ff(B + 1);
    const int rc = sgo_edge_groups(_ctx, (int32_t)n, (int32_t)B, member.data(), chi2Max.empty() ? nullptr : chi2Max.data(), minPivot, dd.data(), nullptr,
                                   pp.data(), ff.data());
    if (rc < 0) {
      std::cerr << "SparseOptimizer::sgoEdgeGroups: " << sgo_last_error(_ctx) << std::endl;
      return -1;
    }
    if (d2) d2->assign(dd.begin(), dd.begin() + B);
    if (pivot) pivot->assign(pp.begin(), pp.begin() + B);
    if (fail) {
      fail->assign(chi2Max.empty() ? 0 : B, false);
      for (size_t b = 0; b < fail->size(); ++b) (*fail)[b] = ff[b] != 0;
    }
    return rc;
  }

  // the candidates of sgoCandidateJoint / sgoJointGreedy / sgoJointExtend as the C-ABI takes them; false: a null edge or vertex, a vertex
  // that is not an active one
  bool jointCandidates(const std::vector<EdgeSE2*>& candidates, std::vector<int32_t>& ci, std::vector<int32_t>& cj, std::vector<double>& meas,
                       std::vector<double>& info) const {
    const size_t n = candidates.size();
    ci.assign(n, 0), cj.assign(n, 0);
    meas.assign(3 * n, 0.0), info.assign(6 * n, 0.0);
    for (size_t t = 0; t < n; ++t) {
      const EdgeSE2* e = candidates[t];
      if (!e) return false;
      for (int side = 0; side < 2; ++side) {
        const HyperGraph::Vertex* v = e->vertex(side);
        if (!v) return false;
        auto it = std::lower_bound(_activeVertices.begin(), _activeVertices.end(), v->id(),
                                   [](const OptimizableGraph::Vertex* a, int id) { return a->id() < id; });
        if (it == _activeVertices.end() || *it != v) return false;
        (side ? cj : ci)[t] = (int32_t)(it - _activeVertices.begin());
      }
      for (int q = 0; q < 3; ++q) meas[3 * t + q] = e->measurement()[q];
      const auto& O = e->information();
      double* o = &info[6 * t];
      o[0] = O(0, 0); o[1] = O(0, 1); o[2] = O(0, 2); o[3] = O(1, 1); o[4] = O(1, 2); o[5] = O(2, 2);
    }
    return true;
  }

  // ---- joint compatibility of a set of candidate closures (extension; sgo_candidate_joint / sgo_joint_subsets of include/sgo.h):
  // the candidates are EdgeSE2 objects as sgoCandidateGate takes them; subsets[b] lists the candidates (indices into `candidates`,
  // any order, a repeated index counts once) of subset b.  (*d2)[b] = e_s^T (S_ss)^-1 e_s with the candidates' cross-covariances at
  // the current estimates, 3 |s| degrees of freedom; chi2Max empty: no decisions (returns 0, *pass is emptied), else one bound per
  // subset and (*pass)[b] = d2 <= chi2Max[b]; returns how many pass.  Returns -1 without touching the outputs in the situations where
  // sgoCandidateGate does, for an index outside the candidates, for a chi2Max of another length than subsets, and when a call
  // itself refuses (more than SGO_JOINT_MAX_CANDIDATES candidates, a subset of more than SGO_JOINT_MAX_SUBSET; one line on std::cerr).
  int sgoCandidateJoint(const std::vector<EdgeSE2*>& candidates, const std::vector<std::vector<int>>& subsets, const std::vector<double>& chi2Max,
                        std::vector<double>* d2, std::vector<bool>* pass) {
    if (!_algorithm || _activeRevision != _revision || _activeVertices.empty() || !gpuEligible()) return -1;
    const size_t n = candidates.size(), B = subsets.size();
    if (!chi2Max.empty() && chi2Max.size() != B) return -1;
    std::vector<int32_t> ci, cj;
    std::vector<double> meas, info;
    if (!jointCandidates(candidates, ci, cj, meas, info)) return -1;
    std::vector<uint8_t> mask(std::max<size_t>(B * n, 1), 0);
    for (size_t b = 0; b < B; ++b)
      for (int t : subsets[b]) {
        if (t < 0 || (size_t)t >= n) return -1;
        mask[b * n + (size_t)t] = 1;
      }
    if (!uploadGraph()) return -1;
    int rc = sgo_candidate_joint(_ctx, (int32_t)n, ci.data(), cj.data(), meas.data(), info.data(), nullptr, nullptr);
    std::vector<double> dd(std::max<size_t>(B, 1));
    std::vector<uint8_t> ok(std::max<size_t>(B, 1), 0);
    if (rc >= 0 && n > 0)
      rc = sgo_joint_subsets(_ctx, (int32_t)n, (int32_t)B, mask.data(), chi2Max.empty() ? nullptr : chi2Max.data(), dd.data(), nullptr, ok.data());
    else if (rc >= 0) {   // (no candidates: every subset is the empty one, d2 = 0)
      rc = 0;
      for (size_t b = 0; b < B; ++b) {
        dd[b] = 0.0;
        ok[b] = !chi2Max.empty() && 0.0 <= chi2Max[b];
        rc += ok[b];
      }
    }
    if (rc < 0) {
      std::cerr << "SparseOptimizer::sgoCandidateJoint: " << sgo_last_error(_ctx) << std::endl;
      return -1;
    }
    if (d2) d2->assign(dd.begin(), dd.begin() + B);
    if (pass) {
      pass->resize(chi2Max.empty() ? 0 : B);
      for (size_t b = 0; b < pass->size(); ++b) (*pass)[b] = ok[b] != 0;
    }
    return rc;
  }

  // ---- greedy search for a large jointly compatible set (extension; sgo_joint_greedy / sgo_joint_extend of include/sgo.h): the
  // candidates are sgoCandidateJoint's; seeds[b] lists the candidates (indices into `candidates`, in this order) forced into search b,
  // chi2Max[k] bounds the d2 of a set of k candidates (SGO_JOINT_MAX_SUBSET + 1 entries, [0] ignored; empty: no growth), allow[b][t]
  // false keeps candidate t out of search b's growth (allow empty: all).  (*out)[b]: the order (seed, then the chosen ones), why the
  // search stopped (SGO_JSTOP_*), d2 after every pivot (order.size() + 1 entries) and d2 of the final set with each candidate added.
  // Returns how many searches ran; -1 without touching the outputs where sgoCandidateJoint returns it, for an allow of another shape
  // and when the call itself refuses (an index outside the candidates or listed twice, maxLen below a seed's length or above
  // SGO_JOINT_MAX_SUBSET, a chi2Max of another length; one line on std::cerr).
  struct SgoJointPath {
    std::vector<int> order;
    int stop = 0;
    std::vector<double> d2Path, d2Ext;
  };
  int sgoJointGreedy(const std::vector<EdgeSE2*>& candidates, const std::vector<std::vector<int>>& seeds, const std::vector<double>& chi2Max, int maxLen,
                     const std::vector<std::vector<bool>>& allow, std::vector<SgoJointPath>* out) {
    return jointSearch(candidates, seeds, &chi2Max, maxLen, allow, out, nullptr, nullptr);
  }
  // ... and its primitive without growth: (*d2)[b] of list b and (*d2Ext)[b][t] = d2 of the list with candidate t added
  int sgoJointExtend(const std::vector<EdgeSE2*>& candidates, const std::vector<std::vector<int>>& lists, std::vector<double>* d2,
                     std::vector<std::vector<double>>* d2Ext) {
    return jointSearch(candidates, lists, nullptr, -1, std::vector<std::vector<bool>>(), nullptr, d2, d2Ext);
  }

  int jointSearch(const std::vector<EdgeSE2*>& candidates, const std::vector<std::vector<int>>& seeds, const std::vector<double>* chi2Max, int maxLen,
                  const std::vector<std::vector<bool>>& allow, std::vector<SgoJointPath>* out, std::vector<double>* d2, std::vector<std::vector<double>>* d2Ext) {
    if (!_algorithm || _activeRevision != _revision || _activeVertices.empty() || !gpuEligible()) return -1;
    const size_t n = candidates.size(), B = seeds.size(), kS = SGO_JOINT_MAX_SUBSET;
    const char* who = chi2Max ? "SparseOptimizer::sgoJointGreedy: " : "SparseOptimizer::sgoJointExtend: ";
    if (chi2Max && !chi2Max->empty() && chi2Max->size() != kS + 1) {
      std::cerr << who << "chi2Max needs SGO_JOINT_MAX_SUBSET + 1 entries" << std::endl;
      return -1;
    }
    if (!allow.empty() && allow.size() != B) return -1;
    std::vector<int32_t> ci, cj;
    std::vector<double> meas, info;
    if (!jointCandidates(candidates, ci, cj, meas, info)) return -1;
    std::vector<int32_t> rows(std::max<size_t>(B, 1) * kS, -1);
    std::vector<uint8_t> mask(std::max<size_t>(B * n, 1), 1);
    for (size_t b = 0; b < B; ++b) {
      if (seeds[b].size() > kS) {
        std::cerr << who << "list " << b << " names more than SGO_JOINT_MAX_SUBSET candidates" << std::endl;
        return -1;
      }
      for (size_t k = 0; k < seeds[b].size(); ++k) {
        if (seeds[b][k] < 0 || (size_t)seeds[b][k] >= n) return -1;
        rows[b * kS + k] = seeds[b][k];
      }
      if (!allow.empty()) {
        if (allow[b].size() != n) return -1;
        for (size_t t = 0; t < n; ++t) mask[b * n + t] = allow[b][t] ? 1 : 0;
      }
    }
    if (n == 0) {
      std::cerr << who << "no candidates" << std::endl;
      return -1;
    }
    if (!uploadGraph()) return -1;
    int rc = sgo_candidate_joint(_ctx, (int32_t)n, ci.data(), cj.data(), meas.data(), info.data(), nullptr, nullptr);
    std::vector<int32_t> order(rows.size()), count(std::max<size_t>(B, 1)), stop(std::max<size_t>(B, 1));
    std::vector<double> path(std::max<size_t>(B, 1) * (kS + 1)), ext(std::max<size_t>(B * n, 1)), dd(std::max<size_t>(B, 1));
    if (rc >= 0)
      rc = chi2Max ? sgo_joint_greedy(_ctx, (int32_t)n, (int32_t)B, rows.data(), allow.empty() ? nullptr : mask.data(), chi2Max->empty() ? nullptr : chi2Max->data(),
                                      maxLen, order.data(), count.data(), stop.data(), path.data(), ext.data())
                   : sgo_joint_extend(_ctx, (int32_t)n, (int32_t)B, rows.data(), dd.data(), ext.data());
    if (rc < 0) {
      std::cerr << who << sgo_last_error(_ctx) << std::endl;
      return -1;
    }
    if (out) {
      out->assign(B, SgoJointPath());
      for (size_t b = 0; b < B; ++b) {
        SgoJointPath& p = (*out)[b];
        p.order.assign(order.begin() + b * kS, order.begin() + b * kS + count[b]);
        p.stop = stop[b];
        p.d2Path.assign(path.begin() + b * (kS + 1), path.begin() + b * (kS + 1) + count[b] + 1);
        p.d2Ext.assign(ext.begin() + b * n, ext.begin() + (b + 1) * n);
      }
    }
    if (d2) d2->assign(dd.begin(), dd.begin() + B);
    if (d2Ext) {
      d2Ext->assign(B, std::vector<double>());
      for (size_t b = 0; b < B; ++b) (*d2Ext)[b].assign(ext.begin() + b * n, ext.begin() + (b + 1) * n);
    }
    return rc;
  }

  // ---- many closure hypotheses of the graph in one call (extension; sgo_optimize_gn_hypotheses of include/sgo.h): hypothesis b is
  // the graph without the edges of off[b], optimised from the current estimates as optimize(iters) under a
  // SparseOptimizerTerminateAction of gain threshold gainTol would (gainTol <= 0: plain optimize(iters)).  Valid after
  // initializeOptimization() on a graph the device holds or can take; out[b] gets the iterations, the stop reason, both chi2, every
  // active edge's chi2 and the poses.  No vertex estimate changes.  false with one line on std::cerr for a graph that takes the host
  // solver (Levenberg, landmark types), for an edge that is not an active edge, and when the call itself refuses.
  bool sgoOptimizeHypotheses(const std::vector<std::vector<OptimizableGraph::Edge*>>& off, int iters, double gainTol,
                             std::vector<SgoHypothesis>& out) {
    if (!_algorithm || _activeRevision != _revision || _activeVertices.empty() || !gpuEligible()) {
      std::cerr << "SparseOptimizer::sgoOptimizeHypotheses: only the device path (VertexSE2 / EdgeSE2 under Gauss-Newton, after initializeOptimization) optimises hypotheses"
                << std::endl;
      return false;
    }
    if (!uploadGraph()) return false;
    // the device's record of every active edge (records of edges that left the graph since are deactivated there and stay so)
    const size_t dE = _m.ei.size(), V = _activeVertices.size(), B = off.size();
    std::unordered_map<const OptimizableGraph::Edge*, size_t> record;
    {
      size_t k = 0;
      for (size_t r = 0; r < dE && k < _activeEdges.size(); ++r)
        if (!_m.dead[r]) record[_activeEdges[k++]] = r;
    }
    std::vector<uint8_t> mask(std::max<size_t>(B * dE, 1), 0);
    for (size_t b = 0; b < B; ++b)
      for (const OptimizableGraph::Edge* e : off[b]) {
        const auto it = record.find(e);
        if (it == record.end()) {
          std::cerr << "SparseOptimizer::sgoOptimizeHypotheses: hypothesis " << b << " lists an edge that is not an active edge" << std::endl;
          return false;
        }
        mask[b * dE + it->second] = 1;
      }
    std::vector<sgo_hypothesis_result> res(std::max<size_t>(B, 1));
    std::vector<double> poses(std::max<size_t>(3 * B * V, 1)), e2(std::max<size_t>(B * dE, 1));
    if (sgo_optimize_gn_hypotheses(_ctx, (int32_t)B, iters, gainTol, mask.data(), nullptr, res.data(), nullptr, poses.data(), e2.data()) < 0) {
      std::cerr << "SparseOptimizer::sgoOptimizeHypotheses: " << sgo_last_error(_ctx) << std::endl;
      return false;
    }
    out.assign(B, SgoHypothesis());
    for (size_t b = 0; b < B; ++b) {
      SgoHypothesis& h = out[b];
      h.iterations = res[b].iters_done;
      h.stopReason = res[b].stop_reason;
      h.chi2 = res[b].chi2;
      h.robustChi2 = res[b].robust_chi2;
      for (const auto& er : record) h.edgeChi2[er.first] = e2[b * dE + er.second];
      for (size_t k = 0; k < V; ++k) {
        const double* p = &poses[3 * (b * V + k)];
        h.poses.emplace(_activeVertices[k]->id(), SE2(p[0], p[1], p[2]));
      }
    }
    return true;
  }

  // sgoSetHypothesesWorkspace(bytes): the device memory sgoOptimizeHypotheses may take for per-hypothesis copies on a graph of the
  // multifrontal path, where it then shares every launch among many hypotheses (sgo_set_hypotheses_workspace of include/sgo.h; 0,
  // the default: one hypothesis after the other; never more than `bytes` is allocated).  Kept by the optimiser and forwarded
  // whenever the graph goes to the device; false for a negative value.
  bool sgoSetHypothesesWorkspace(long long bytes) {
    if (bytes < 0) return false;
    _hypothesesWorkspace = bytes;
    return true;
  }

  // ---- graph files (OptimizableGraph::load / save of g2o, for the types of this backend's device path):
  //   VERTEX_SE2 id x y theta | EDGE_SE2 i j dx dy dtheta o11 o12 o13 o22 o23 o33 | FIX id...
  // load() creates the objects and keeps them alive for the optimiser's lifetime (everything the CALLER adds
  // stays caller-owned, README.md:22-23); records of other types are skipped with a note on std::cerr, as
  // upstream does for unregistered tags.  save() writes the vertices in ascending id, FIX lines, then the edges
  // in insertion order, with max_digits10 precision (a load / save / load round trip is exact).
  bool load(std::istream& is) {
    std::string line;
    int skipped = 0;
    while (std::getline(is, line)) {
      std::istringstream ls(line);
      std::string tag;
      if (!(ls >> tag) || tag[0] == '#') continue;
      if (tag == "VERTEX_SE2") {
        int id;
        if (!(ls >> id)) return false;
        _loadedVertices.emplace_back();
        VertexSE2& v = _loadedVertices.back();
        v.setId(id);
        if (!v.read(ls) || ls.fail() || !addVertex(&v)) return false;
      } else if (tag == "EDGE_SE2") {
        int i, j;
        if (!(ls >> i >> j)) return false;
        auto* vi = vertex(i);
        auto* vj = vertex(j);
        if (!vi || !vj) {
          std::cerr << "SparseOptimizer::load: EDGE_SE2 " << i << " " << j << " references an unknown vertex" << std::endl;
          return false;
        }
        _loadedEdges.emplace_back();
        EdgeSE2& e = _loadedEdges.back();
        e.vertices()[0] = vi;
        e.vertices()[1] = vj;
        if (!e.read(ls) || !addEdge(&e)) return false;
      } else if (tag == "FIX") {
        int id;
        while (ls >> id)
          if (auto* v = vertex(id)) v->setFixed(true);
      } else {
        ++skipped;
      }
    }
    if (skipped) std::cerr << "SparseOptimizer::load: skipped " << skipped << " records of types this backend does not read" << std::endl;
    return true;
  }
  bool load(const char* filename) {
    std::ifstream f(filename);
    return f.good() && load(f);
  }
  bool save(std::ostream& os, int level = 0) const {
    (void)level;
    os << std::setprecision(17);
    std::vector<const OptimizableGraph::Vertex*> vs;
    for (auto& kv : _vertices) vs.push_back(static_cast<const OptimizableGraph::Vertex*>(kv.second));
    std::sort(vs.begin(), vs.end(), [](const OptimizableGraph::Vertex* a, const OptimizableGraph::Vertex* b) { return a->id() < b->id(); });
    for (auto* v : vs) {
      if (typeid(*v) != typeid(VertexSE2)) continue;
      os << "VERTEX_SE2 " << v->id() << " ";
      static_cast<const VertexSE2*>(v)->write(os);
      os << "\n";
    }
    for (auto* v : vs)
      if (v->fixed()) os << "FIX " << v->id() << "\n";
    std::vector<const HyperGraph::Edge*> es(_edges.begin(), _edges.end());
    std::sort(es.begin(), es.end(), [](const HyperGraph::Edge* a, const HyperGraph::Edge* b) { return a->internalId() < b->internalId(); });
    for (auto* he : es) {
      auto* e = static_cast<const OptimizableGraph::Edge*>(he);
      if (typeid(*e) != typeid(EdgeSE2)) continue;
      os << "EDGE_SE2 " << e->vertices()[0]->id() << " " << e->vertices()[1]->id() << " ";
      static_cast<const EdgeSE2*>(e)->write(os);
      os << "\n";
    }
    return os.good();
  }
  bool save(const char* filename, int level = 0) const {
    std::ofstream f(filename);
    return f.good() && save(f, level);
  }

  const sgo_stats* lastStats() const { return _lastStats.get(); }
  // which solver / set-up the backend used for the graph it holds (extension for the tests: sgo_solver_description)
  std::string backendDescription() const { return _ctx ? std::string(sgo_solver_description(_ctx)) : std::string(); }
  // Levenberg-Marquardt bookkeeping of the last optimize() on the host solver (extension for the tests; g2o
  // exposes the same numbers through OptimizationAlgorithmLevenberg::currentLambda() / levenbergIterations()
  // and its verbose output): damping after the iteration, robust chi2 after it, trials it took.
  struct LmIteration {
    double lambda, chi2;
    int trials;
  };
  const std::vector<LmIteration>& lmTrace() const { return _lmTrace; }
  // ... and of the last optimize() under OptimizationAlgorithmDogleg (g2o: lastStep(), trustRegion() and the verbose output):
  // the trust region after the iteration, robust chi2 after it, its trials, the accepted step's kind (SGO_DL_STEP_*, -1: none)
  struct DoglegIteration {
    double delta, chi2;
    int trials, step;
  };
  const std::vector<DoglegIteration>& doglegTrace() const { return _dlTrace; }

  void computeActiveErrors() {
    for (auto* e : _activeEdges) e->computeError();
  }
  double activeChi2() const {
    double s = 0;
    for (auto* e : _activeEdges) s += e->chi2();
    return s;
  }
  double activeRobustChi2() const {
    double s = 0;
    Vector3 rho;
    for (auto* e : _activeEdges) {
      if (e->robustKernel()) {
        e->robustKernel()->robustify(e->chi2(), rho);
        s += rho[0];
      } else {
        s += e->chi2();
      }
    }
    return s;
  }
  const std::vector<OptimizableGraph::Edge*>& activeEdges() const { return _activeEdges; }
  const std::vector<OptimizableGraph::Vertex*>& activeVertices() const { return _activeVertices; }

  void push() {
    for (auto* v : _activeVertices) v->push();
  }
  void pop() {
    for (auto* v : _activeVertices) v->pop();
  }
  void discardTop() {
    for (auto* v : _activeVertices) v->discardTop();
  }

 private:
  // ---- small dense host solver for graphs that are not the SE(2) GN pose graph -----------------
  // OptimizationAlgorithmGaussNewton::solve / OptimizationAlgorithmLevenberg::solve of g2o
  // 2020.5.29 on dense normal equations (the landmark graph has <= a few hundred unknowns).
  bool hostBuildSystem(std::vector<double>& H, std::vector<double>& b, int n) {
    std::fill(H.begin(), H.end(), 0.0);
    std::fill(b.begin(), b.end(), 0.0);
    for (auto* e : _activeEdges) {
      e->linearizeOplus();
      e->constructQuadraticForm(H.data(), n, b.data());
    }
    return true;
  }
  static bool hostCholeskySolve(std::vector<double> A, const std::vector<double>& b, int n, std::vector<double>& x) {
    for (int j = 0; j < n; ++j) {                     // in-place lower Cholesky
      double d = A[(size_t)j * n + j];
      for (int k = 0; k < j; ++k) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
      if (!(d > 0.0) || !std::isfinite(d)) return false;
      d = std::sqrt(d);
      A[(size_t)j * n + j] = d;
      for (int i = j + 1; i < n; ++i) {
        double s = A[(size_t)i * n + j];
        for (int k = 0; k < j; ++k) s -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
        A[(size_t)i * n + j] = s / d;
      }
    }
    x = b;
    for (int i = 0; i < n; ++i) {
      double s = x[i];
      for (int k = 0; k < i; ++k) s -= A[(size_t)i * n + k] * x[k];
      x[i] = s / A[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
      double s = x[i];
      for (int k = i + 1; k < n; ++k) s -= A[(size_t)k * n + i] * x[k];
      x[i] = s / A[(size_t)i * n + i];
    }
    for (double v : x)
      if (!std::isfinite(v)) return false;
    return true;
  }
  void hostUpdate(const std::vector<double>& x) {
    for (auto* v : _activeVertices)
      if (!v->fixed()) v->oplus(x.data() + v->colInHessian());
  }
  int hostOptimize(int iterations, bool online) {
    (void)online;
    int n = 0;
    for (auto* v : _activeVertices) {
      v->setColInHessian(v->fixed() ? -1 : n);
      if (!v->fixed()) n += v->dimension();
    }
    if (n == 0) return -1;
    // This dense host solver exists for the landmark graph (<= a few hundred unknowns).  It is not a
    // fallback for pose graphs: a large graph that is not (VertexSE2, EdgeSE2, no kernel or one of robust_kernel_impl.h,
    // Gauss-Newton) is refused instead of being solved in O(n^3) on the host.
    if (n > kHostSolverMaxUnknowns) {
      std::cerr << "SparseOptimizer::optimize: " << n << " unknowns in a graph the device path does not cover "
                << "(only VertexSE2 / EdgeSE2 with no kernel or a kernel of robust_kernel_impl.h is); refusing"
                << std::endl;
      return 0;
    }
    const bool lm = _algorithm->kind() == OptimizationAlgorithm::Levenberg;
    _lmTrace.clear();
    std::vector<double> H((size_t)n * n), b(n), x(n);
    int cjIterations = 0;
    bool ok = true, failed = false;
    // a registered terminate action: sgo_optimize_gn_until's rule after every iteration (the first one only records its chi2)
    if (_terminateAction) iterations = _terminateAction->iterationCap(iterations);
    double lastChi = 0.0;
    auto converged = [&]() {
      if (!_terminateAction) return false;
      computeActiveErrors();
      const double chi = activeRobustChi2();
      const bool stop = cjIterations >= 2 && sgo_gain_stop(lastChi, chi, _terminateAction->gainThreshold()) != 0;
      lastChi = chi;
      return stop;
    };
    for (int it = 0; it < iterations && ok; ++it) {
      computeActiveErrors();
      double currentChi = activeRobustChi2();
      hostBuildSystem(H, b, n);
      if (!lm) {  // Gauss-Newton: one undamped step
        if (!hostCholeskySolve(H, b, n, x)) {
          std::cerr << "SparseOptimizer::optimize: Cholesky failure, solving failed" << std::endl;
          failed = true;
          break;
        }
        hostUpdate(x);
        ++cjIterations;
        if (converged()) break;
        continue;
      }
      if (it == 0) {  // computeLambdaInit: tau * max diagonal, tau = 1e-5
        double maxDiag = 0;
        for (int j = 0; j < n; ++j) maxDiag = std::max(std::fabs(H[(size_t)j * n + j]), maxDiag);
        _lmLambda = 1e-5 * maxDiag;
        _lmNi = 2.0;
      }
      double rho = 0;
      int qmax = 0;
      do {
        push();
        std::vector<double> Hl(H);
        for (int j = 0; j < n; ++j) Hl[(size_t)j * n + j] += _lmLambda;
        const bool ok2 = hostCholeskySolve(Hl, b, n, x);
        double tempChi = std::numeric_limits<double>::max();
        double scale = 1e-3;
        if (ok2) {
          hostUpdate(x);
          computeActiveErrors();
          tempChi = activeRobustChi2();
          for (int j = 0; j < n; ++j) scale += x[j] * (_lmLambda * x[j] + b[j]);
        }
        rho = (currentChi - tempChi) / scale;
        if (rho > 0 && std::isfinite(tempChi) && ok2) {  // accept
          double alpha = 1. - std::pow((2 * rho - 1), 3);
          alpha = std::min(alpha, 2. / 3.);
          const double scaleFactor = std::max(1. / 3., alpha);
          _lmLambda *= scaleFactor;
          _lmNi = 2;
          currentChi = tempChi;
          discardTop();
        } else {  // reject: restore and increase the damping
          _lmLambda *= _lmNi;
          _lmNi *= 2;
          pop();
          if (!std::isfinite(_lmLambda)) break;
        }
        qmax++;
      } while (rho < 0 && qmax < 10);
      ++cjIterations;
      _lmTrace.push_back({_lmLambda, currentChi, qmax});
      if (qmax == 10 || rho == 0 || !std::isfinite(_lmLambda)) ok = false;  // Terminate
      if (ok && converged()) break;
    }
    if (failed) return 0;
    return cjIterations;
  }
  double _lmLambda = 0.0, _lmNi = 2.0;
  std::vector<LmIteration> _lmTrace;
  static constexpr int kHostSolverMaxUnknowns = 3000;

  // Levenberg-Marquardt on a pose graph the dense host solver refuses for its size (more than kHostSolverMaxUnknowns unknowns): the
  // library's sgo_optimize_lm -- g2o's schedule on the multifrontal factor --, or, for a graph whose size or density the multifrontal
  // analysis refuses, sgo_optimize_lm_pcg -- the same schedule on the PCG --, with the marshalling of the Gauss-Newton route.
  // Everything the host solver solves stays there.
  bool levenbergOnDevice() const {
    if (_algorithm->kind() != OptimizationAlgorithm::Levenberg || !deviceTypes()) return false;
    int n = 0;
    for (auto* v : _activeVertices) n += v->fixed() ? 0 : v->dimension();
    return n > kHostSolverMaxUnknowns;
  }
  // Returns the iterations counted, as the host solver does; _lmTrace is the call's trace (lambda and robust chi2 after every
  // iteration, its trials).  0 with one line on std::cerr when a terminate action is registered (the decisions are taken on the
  // device, which knows g2o's own termination only).
  int deviceLevenberg(int iterations) {
    _lmTrace.clear();
    if (_terminateAction) {
      std::cerr << "SparseOptimizer::optimize: a graph of this size under Levenberg-Marquardt takes sgo_optimize_lm, which applies no "
                << "SparseOptimizerTerminateAction (remove the action, or use Gauss-Newton, whose device path applies it); refusing" << std::endl;
      return 0;
    }
    if (!uploadGraph()) return 0;
    // sgo_optimize_lm refuses a graph that carries an incremental overlay (a PCG context whose graph grew under Gauss-Newton, now
    // or in an earlier call): this route gives such a graph the full set-up
    if (std::strstr(sgo_solver_description(_ctx), "incremental overlay")) {
      _graphOnDevice = false;
      if (!uploadGraph()) return 0;
    }
    _lastStats.reset();   // (lastStats() is the last Gauss-Newton call's: none now)
    std::unique_ptr<sgo_lm_stats> st(new sgo_lm_stats());
    int done = sgo_optimize_lm(_ctx, iterations, 0.0, st.get());
    // (a graph the multifrontal analysis refuses for its size or density -- SGO_ENOTHING although there is a free active vertex --:
    // the same schedule with the trials solved by the context's PCG)
    if (done == SGO_ENOTHING && sgo_num_free(_ctx) > 0) done = sgo_optimize_lm_pcg(_ctx, iterations, 0.0, st.get());
    if (done < 0) {
      std::cerr << "SparseOptimizer::optimize: " << sgo_last_error(_ctx) << (done == SGO_ENOTHING ? "; refusing" : "") << std::endl;
      return 0;
    }
    for (int k = 0; k < st->iters_done; ++k) _lmTrace.push_back({st->lambda[k], st->robust_chi2[k + 1], st->trials[k]});
    if (st->iters_done > 0) _lmLambda = st->lambda[st->iters_done - 1];
    if (_verbose)
      for (int k = 0; k < st->iters_done; ++k)
        std::cerr << "iteration= " << k << "\t chi2= " << st->chi2[k + 1] << "\t lambda= " << st->lambda[k] << "\t trials= " << st->trials[k]
                  << std::endl;
    downloadEstimates();
    return done;
  }

  // Powell's dogleg, beside Levenberg's dispatch: sgo_optimize_dogleg -- g2o's schedule, one factorisation per iteration on the
  // multifrontal factor --, or, for a graph the multifrontal analysis refuses, sgo_optimize_dogleg_pcg.  The library has no host
  // solver for this algorithm: a graph the device path does not cover, or a registered terminate action, is refused with one line.
  std::vector<DoglegIteration> _dlTrace;
  int deviceDogleg(int iterations) {
    _dlTrace.clear();
    if (!deviceTypes()) {
      std::cerr << "SparseOptimizer::optimize: OptimizationAlgorithmDogleg covers VertexSE2 / EdgeSE2 graphs with no kernel or a kernel of "
                << "robust_kernel_impl.h only; refusing" << std::endl;
      return 0;
    }
    if (_terminateAction) {
      std::cerr << "SparseOptimizer::optimize: OptimizationAlgorithmDogleg takes sgo_optimize_dogleg, which applies no "
                << "SparseOptimizerTerminateAction (remove the action, or use Gauss-Newton, whose device path applies it); refusing" << std::endl;
      return 0;
    }
    if (!uploadGraph()) return 0;
    if (std::strstr(sgo_solver_description(_ctx), "incremental overlay")) {   // (refused by the call: the full set-up, as deviceLevenberg)
      _graphOnDevice = false;
      if (!uploadGraph()) return 0;
    }
    _lastStats.reset();   // (lastStats() is the last Gauss-Newton call's: none now)
    std::unique_ptr<sgo_dogleg_stats> st(new sgo_dogleg_stats());
    int done = sgo_optimize_dogleg(_ctx, iterations, 0.0, st.get());
    if (done == SGO_ENOTHING && sgo_num_free(_ctx) > 0) done = sgo_optimize_dogleg_pcg(_ctx, iterations, 0.0, st.get());
    if (done < 0) {
      std::cerr << "SparseOptimizer::optimize: " << sgo_last_error(_ctx) << (done == SGO_ENOTHING ? "; refusing" : "") << std::endl;
      return 0;
    }
    for (int k = 0; k < st->iters_done; ++k) _dlTrace.push_back({st->delta[k], st->robust_chi2[k + 1], st->trials[k], st->step_kind[k]});
    if (_verbose)
      for (int k = 0; k < st->iters_done; ++k)
        std::cerr << "iteration= " << k << "\t chi2= " << st->chi2[k + 1] << "\t delta= " << st->delta[k] << "\t trials= " << st->trials[k]
                  << std::endl;
    downloadEstimates();
    if (st->stop_reason == SGO_DL_STOP_DAMPING) return 0;   // (g2o: Fail)
    return done;
  }

  // what optimize() and sgoOptimizeMany do behind the device's Gauss-Newton call: the messages, the statistics, the estimates
  int finishDeviceCall(int done, int iterations, sgo_stats* st) {
    if (done < 0 && done != SGO_ENOTHING) {
      std::cerr << "SparseOptimizer::optimize: " << sgo_last_error(_ctx) << std::endl;
      done = 0;
    } else if (done == 0 && iterations > 0) {   // OptimizationAlgorithm::Fail: optimize() returns 0 upstream too
      std::cerr << "SparseOptimizer::optimize: linear solve failed after " << st->iters_done << " iterations: "
                << sgo_last_error(_ctx) << std::endl;
    }
    if (_verbose)
      for (int k = 0; k < st->iters_done; ++k)
        std::cerr << "iteration= " << k << "\t chi2= " << st->chi2[k + 1] << "\t time= " << st->seconds[k]
                  << "\t pcg= " << st->pcg_iters[k] << std::endl;
    _lastStats.reset(st);
    downloadEstimates();
    return done;
  }
  bool gpuEligible() const { return _algorithm->kind() == OptimizationAlgorithm::GaussNewton && deviceTypes(); }
  // every active vertex a VertexSE2 and every active edge an EdgeSE2 whose kernel, if any, the device evaluates
  bool deviceTypes() const {
    for (auto* v : _activeVertices)
      if (typeid(*v) != typeid(VertexSE2)) return false;
    for (auto* e : _activeEdges) {
      if (typeid(*e) != typeid(EdgeSE2)) return false;
      // (a kernel class the device does not evaluate, or a parameter sgo_set_robust_kernels would refuse: the host solver)
      const int kind = sgoRobustKernelKind(e->robustKernel());
      if (kind < 0) return false;
      const double delta = e->robustKernel() ? e->robustKernel()->delta() : 1.0;
      if (kind >= SGO_KERNEL_HUBER && kind != SGO_KERNEL_GEMAN_MCCLURE && !(std::isfinite(delta) && delta > 0.0)) return false;
      // (a multi-GPU context knows DCS only: decided here, before a set-up that sgo_set_robust_kernels would then refuse)
      if (kind >= SGO_KERNEL_HUBER && _ctx && sgo_comm_size(_ctx) > 1) return false;
    }
    return true;
  }
  // marshal the pointer graph into the flat arrays of sgo_set_graph_se2 (compact vertex numbering
  // in ascending id) and upload.  g2o rebuilds the system from the edge objects on every optimize(),
  // so measurement / information / fixed / kernel-delta changes made between two optimize() calls
  // without an initializeOptimization() must be seen: the arrays are marshalled every time and compared
  // with what the device holds.  Three outcomes:
  //   * identical graph: only the poses are uploaded (sgo_set_poses);
  //   * the device's graph is a PREFIX of the new one -- what the reference's loop closer produces: the graph it
  //     optimised before + a chain of new poses + one closure (slc.cpp:205-226, :272-287) -- : sgo_update_graph_se2,
  //     which keeps the resident structures when the appended part allows it (include/sgo.h);
  //   * same vertices, and the new edge records are the device's with some LEFT OUT, in order -- what removeEdge of EdgeSE2 edges
  //     followed by initializeOptimization() produces, the closure gate of log_runner.cpp:182-204 --: sgo_set_edge_information
  //     with zero rows for the missing edges (they are deactivated, every resident structure is kept), then sgo_set_poses.  _m
  //     keeps the device's records with a `dead` flag each, and later calls compare against the records that are not dead.
  //     SGO_INCREMENTAL=0 in the environment, or a refusal of that call, takes the full set-up;
  //   * anything else (growth or a re-added edge after a removal and a removed vertex included): sgo_set_graph_se2, which
  //     clears the flags.
  bool uploadGraph() {
    if (!_ctx) {
      _ctx = sgo_create(-1, nullptr);
      if (!_ctx) {
        std::cerr << "SparseOptimizer: " << sgo_last_error(nullptr) << std::endl;
        return false;
      }
    }
    sgo_set_hypotheses_workspace(_ctx, (int64_t)_hypothesesWorkspace);
    const int V = (int)_activeVertices.size(), E = (int)_activeEdges.size();
    std::vector<double> poses(3 * (size_t)V);
    for (int k = 0; k < V; ++k) {
      VertexSE2* v = static_cast<VertexSE2*>(_activeVertices[k]);
      poses[3 * k] = v->estimate()[0];
      poses[3 * k + 1] = v->estimate()[1];
      poses[3 * k + 2] = v->estimate()[2];
      v->setTempIndex(k);   // compact numbering in ascending id (the array index sgo uses)
    }
    std::vector<uint8_t> fixed(V);
    std::vector<int32_t> vid(V);
    for (int k = 0; k < V; ++k) {
      fixed[k] = _activeVertices[k]->fixed() ? 1 : 0;
      vid[k] = _activeVertices[k]->id();
    }
    std::vector<int32_t> ei(E), ej(E);
    std::vector<double> meas(3 * (size_t)E), info(6 * (size_t)E), phi(E);
    std::vector<int32_t> kind(E);   // SGO_KERNEL_* of the edge's kernel; phi carries its delta whatever the kind
    for (int k = 0; k < E; ++k) {
      const EdgeSE2* e = static_cast<const EdgeSE2*>(_activeEdges[k]);
      ei[k] = static_cast<const OptimizableGraph::Vertex*>(e->vertex(0))->tempIndex();
      ej[k] = static_cast<const OptimizableGraph::Vertex*>(e->vertex(1))->tempIndex();
      for (int q = 0; q < 3; ++q) meas[3 * k + q] = e->measurement()[q];
      const auto& O = e->information();
      double* o = &info[6 * (size_t)k];
      o[0] = O(0, 0); o[1] = O(0, 1); o[2] = O(0, 2); o[3] = O(1, 1); o[4] = O(1, 2); o[5] = O(2, 2);
      phi[k] = e->robustKernel() ? e->robustKernel()->delta() : -1.0;
      kind[k] = sgoRobustKernelKind(e->robustKernel());
      if (kind[k] == SGO_KERNEL_GEMAN_MCCLURE) phi[k] = 1.0;   // (the kernel has no parameter; the device wants a positive one)
    }
    // is the device's graph (the previous marshal) a prefix of this one?  Same vertex ids and fixed flags for its
    // vertices (compact numbers then agree), bit-identical edge records for its edges
    auto same = [](const void* a, const void* b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; };
    const int dV = (int)_m.vid.size(), dE = (int)_m.ei.size();
    const bool prefix = _graphOnDevice && _m.nDead == 0 && V >= dV && E >= dE && same(vid.data(), _m.vid.data(), sizeof(int32_t) * (size_t)dV) &&
                        same(fixed.data(), _m.fixed.data(), (size_t)dV) && same(ei.data(), _m.ei.data(), sizeof(int32_t) * (size_t)dE) &&
                        same(ej.data(), _m.ej.data(), sizeof(int32_t) * (size_t)dE) && same(meas.data(), _m.meas.data(), sizeof(double) * 3 * (size_t)dE) &&
                        same(info.data(), _m.info.data(), sizeof(double) * 6 * (size_t)dE) && same(phi.data(), _m.phi.data(), sizeof(double) * (size_t)dE) &&
                        same(kind.data(), _m.kind.data(), sizeof(int32_t) * (size_t)dE);
    if (prefix && V == dV && E == dE) {
      if (sgo_set_poses(_ctx, poses.data()) == SGO_OK) return true;
      std::cerr << "SparseOptimizer: " << sgo_last_error(_ctx) << std::endl;
      return false;
    }
    // the device's live records with some left out?  (greedy in-order match: of two identical records either may be the one that left)
    bool incremental = true;
    if (const char* env = std::getenv("SGO_INCREMENTAL")) incremental = std::atoi(env) != 0;
    if (_graphOnDevice && incremental && V == dV && E <= dE - _m.nDead && (E < dE - _m.nDead || _m.nDead > 0) &&
        same(vid.data(), _m.vid.data(), sizeof(int32_t) * (size_t)dV) && same(fixed.data(), _m.fixed.data(), (size_t)dV)) {
      std::vector<int32_t> missing;
      int k = 0;
      for (int r = 0; r < dE; ++r) {
        if (_m.dead[r]) continue;
        if (k < E && ei[k] == _m.ei[r] && ej[k] == _m.ej[r] && same(&meas[3 * (size_t)k], &_m.meas[3 * (size_t)r], sizeof(double) * 3) &&
            same(&info[6 * (size_t)k], &_m.info[6 * (size_t)r], sizeof(double) * 6) && same(&phi[k], &_m.phi[r], sizeof(double)) &&
            kind[k] == _m.kind[r])
          ++k;
        else
          missing.push_back(r);
      }
      if (k == E) {
        const std::vector<double> zero(6 * missing.size(), 0.0);
        if (missing.empty() || sgo_set_edge_information(_ctx, (int32_t)missing.size(), missing.data(), zero.data()) == SGO_OK) {
          for (int32_t r : missing) _m.dead[r] = 1;
          _m.nDead += (int)missing.size();
          if (sgo_set_poses(_ctx, poses.data()) == SGO_OK) return true;
          std::cerr << "SparseOptimizer: " << sgo_last_error(_ctx) << std::endl;
          return false;
        }
        // (refused -- a pose that would lose its last edge, a multi-GPU context --: the full set-up below)
      }
    }
    _graphOnDevice = false;
    const int rc = prefix ? sgo_update_graph_se2(_ctx, V, poses.data(), fixed.data(), E, ei.data(), ej.data(), meas.data(), info.data(),
                                                 phi.data(), dE)
                          : sgo_set_graph_se2(_ctx, V, poses.data(), fixed.data(), E, ei.data(), ej.data(), meas.data(), info.data(),
                                              phi.data());
    if (rc != SGO_OK) {
      std::cerr << "SparseOptimizer: " << sgo_last_error(_ctx) << std::endl;
      return false;
    }
    // The arrays describe every kernel as DCS with the edge's delta: the other kinds follow.  (After an update the resident
    // prefix keeps its kinds on either of the call's routes: only the appended edges are sent.)
    {
      std::vector<int32_t> kid, kk;
      std::vector<double> kd;
      for (int k = prefix ? dE : 0; k < E; ++k)
        if (kind[k] >= SGO_KERNEL_HUBER) {
          kid.push_back(k);
          kk.push_back(kind[k]);
          kd.push_back(phi[k]);
        }
      if (!kid.empty() && sgo_set_robust_kernels(_ctx, (int32_t)kid.size(), kid.data(), kk.data(), kd.data()) != SGO_OK) {
        std::cerr << "SparseOptimizer: " << sgo_last_error(_ctx) << std::endl;
        return false;
      }
    }
    _graphOnDevice = true;
    _m.vid.swap(vid);
    _m.fixed.swap(fixed);
    _m.ei.swap(ei);
    _m.ej.swap(ej);
    _m.meas.swap(meas);
    _m.info.swap(info);
    _m.phi.swap(phi);
    _m.kind.swap(kind);
    _m.dead.assign((size_t)E, 0);
    _m.nDead = 0;
    return true;
  }
  void downloadEstimates() {
    const int V = (int)_activeVertices.size();
    std::vector<double> poses(3 * (size_t)V);
    if (sgo_get_poses(_ctx, poses.data()) != SGO_OK) {
      std::cerr << "SparseOptimizer: " << sgo_last_error(_ctx) << std::endl;
      return;
    }
    for (int k = 0; k < V; ++k) {
      VertexSE2* v = static_cast<VertexSE2*>(_activeVertices[k]);
      if (!v->fixed()) v->setEstimate(SE2(poses[3 * k], poses[3 * k + 1], poses[3 * k + 2]));
    }
  }

  OptimizationAlgorithm* _algorithm = nullptr;
  bool _verbose = false;
  VertexIDMap _vertices;
  EdgeSet _edges;
  long long _nextEdgeId = 0;
  long long _revision = 0, _activeRevision = -1;   // container changes so far | ... when the active sets were last made
  size_t _edgeJointN = 0;                          // the edges of the table sgoEdgeJoint built last (0: none)
  std::vector<OptimizableGraph::Vertex*> _activeVertices;
  std::vector<OptimizableGraph::Edge*> _activeEdges;
  sgo_ctx* _ctx = nullptr;
  long long _hypothesesWorkspace = 0;   // sgoSetHypothesesWorkspace
  bool _graphOnDevice = false;
  struct Marshalled {   // what the device holds, as it was marshalled
    std::vector<int32_t> vid, ei, ej, kind;
    std::vector<uint8_t> fixed;
    std::vector<double> meas, info, phi;
    std::vector<uint8_t> dead;   // the record's edge left the graph since and is deactivated on the device (zero information)
    int nDead = 0;
  } _m;
  std::unique_ptr<sgo_stats> _lastStats;
  SparseOptimizerTerminateAction* _terminateAction = nullptr;
  std::deque<VertexSE2> _loadedVertices;   // objects created by load(): the optimiser's own
  std::deque<EdgeSE2> _loadedEdges;
};

// One line of the CARMEN-style trajectory file the reference writes for the external metricEvaluator
// (src/sparse_gslam/src/log_runner.cpp:18-23, :258-268; datasets/eval.sh:2-3):
//   FLASER 0 x y theta x y theta t myhost t
inline void write_carmen_result_line(std::ostream& os, const SE2& estimate, double time) {
  const double x = estimate[0], y = estimate[1], theta = estimate[2];
  os << "FLASER 0 " << x << ' ' << y << ' ' << theta << ' ' << x << ' ' << y << ' ' << theta << ' ' << time << " myhost " << time
     << '\n';
}

}  // namespace g2o
