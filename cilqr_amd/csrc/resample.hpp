// Private to cilqr_amd/csrc: what resample_batch.hip (the two entry points) and kernels_resample.hip share -- the
// parameters of a launch and the launch function.  Every pointer of the launch is device memory; nothing here synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cilqr.h"

namespace cilqr {

struct ResampleParams {
  int batch, n_knots, n_queries;   // B, K (2 ... CILQR_DP_MAX_KNOTS), M
  int fields;                      // 9, 10 or 11: the layout (row_layouts.hpp)
  int key_col;                     // 0 or 1
  int per_problem;                 // queries [B][M] instead of [M]
};

// rows [B][K][fields], queries [M] or [B][M], out [B][M][fields]; aligned as doubles, no more is assumed
void launch_resample(const ResampleParams& P, const double* rows, const double* queries, double* out, hipStream_t st);

}  // namespace cilqr
