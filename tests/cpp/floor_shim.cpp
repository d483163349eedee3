// A C entry point over sgo::rules::floor_backward_error (sgo_rules.h) for tests/test_floor_rule.py: the floor rule's measure,
// loaded with ctypes and checked against a numpy reference without a GPU or the product library.
#include "sgo_rules.h"

extern "C" double sgo_test_floor_backward_error(int n, const double* r, const double* x, const double* b, const double* dblk6) {
  return sgo::rules::floor_backward_error(n, r, x, b, dblk6);
}
