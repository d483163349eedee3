// g2o/core/optimization_algorithm_dogleg.h -- include-path shim: g2o's users include this path for OptimizationAlgorithmDogleg; the whole
// mirrored g2o surface lives in g2o/sgo_g2o_compat.h (see the header comment there).
#pragma once
#include "../sgo_g2o_compat.h"
