// robust_kernels.cpp -- the host robustify of every robust-kernel class of the g2o-compat header, evaluated on the samples
// tests/test_robust_reference.py hands over, for comparison with the table of tests/robust_reference.py.  Also checks that
// sgoRobustKernelKind names every class with its SGO_KERNEL_* number and refuses a subclass it does not know.
//
// usage: robust_kernels samples.txt out.txt      (samples: lines "kind delta e2"; out: lines "rho0 rho1 rho2")
#include <fstream>
#include <iomanip>
#include <memory>

#include "g2o/core/robust_kernel_impl.h"

namespace {
struct Unknown : g2o::RobustKernel {
  void robustify(double e2, g2o::Vector3& rho) const override { rho[0] = e2; rho[1] = 1.; rho[2] = 0.; }
};
std::unique_ptr<g2o::RobustKernel> make(int kind) {
  switch (kind) {
    case SGO_KERNEL_DCS: return std::unique_ptr<g2o::RobustKernel>(new g2o::RobustKernelDCS);
    case SGO_KERNEL_HUBER: return std::unique_ptr<g2o::RobustKernel>(new g2o::RobustKernelHuber);
    case SGO_KERNEL_PSEUDO_HUBER: return std::unique_ptr<g2o::RobustKernel>(new g2o::RobustKernelPseudoHuber);
    case SGO_KERNEL_CAUCHY: return std::unique_ptr<g2o::RobustKernel>(new g2o::RobustKernelCauchy);
    case SGO_KERNEL_GEMAN_MCCLURE: return std::unique_ptr<g2o::RobustKernel>(new g2o::RobustKernelGemanMcClure);
    case SGO_KERNEL_WELSCH: return std::unique_ptr<g2o::RobustKernel>(new g2o::RobustKernelWelsch);
    case SGO_KERNEL_FAIR: return std::unique_ptr<g2o::RobustKernel>(new g2o::RobustKernelFair);
    case SGO_KERNEL_TUKEY: return std::unique_ptr<g2o::RobustKernel>(new g2o::RobustKernelTukey);
    case SGO_KERNEL_SATURATED: return std::unique_ptr<g2o::RobustKernel>(new g2o::RobustKernelSaturated);
    default: return nullptr;
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  if (g2o::sgoRobustKernelKind(nullptr) != SGO_KERNEL_NONE) return 5;
  for (int kind = SGO_KERNEL_DCS; kind <= SGO_KERNEL_SATURATED; ++kind)
    if (g2o::sgoRobustKernelKind(make(kind).get()) != kind) return 5;
  Unknown u;
  if (g2o::sgoRobustKernelKind(&u) != -1) return 6;
  std::ifstream in(argv[1]);
  std::ofstream out(argv[2]);
  out << std::setprecision(17);
  int kind;
  double delta, e2;
  while (in >> kind >> delta >> e2) {
    auto k = make(kind);
    if (!k) return 3;
    k->setDelta(delta);
    g2o::Vector3 rho;
    k->robustify(e2, rho);
    out << rho[0] << " " << rho[1] << " " << rho[2] << "\n";
  }
  return out.good() ? 0 : 4;
}
