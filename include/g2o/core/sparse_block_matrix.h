// g2o/core/sparse_block_matrix.h -- include-path shim: the mirrored g2o surface (SparseBlockMatrix among it) lives in
// g2o/sgo_g2o_compat.h (see the header comment there).
#pragma once
#include "../sgo_g2o_compat.h"
