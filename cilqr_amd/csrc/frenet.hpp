// Private to cilqr_amd/csrc: what frenet_batch.hip (the entry points) and kernels_frenet.hip share -- the parameters of a
// launch and the launch functions.  Every pointer of a launch is device memory; nothing here synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cilqr.h"

namespace cilqr {

constexpr int kFrLanes = 256;    // lanes of a workgroup
constexpr int kFrTile = 512;     // centre points per LDS tile (tests/frenet_cases.py: TILE)
constexpr int kFrWide = 4;       // queries a lane owns in a large call
// below this many queries a lane owns one: 256 CUs x 4 SIMDs x 64 lanes x kFrWide, the first size at which the wide
// mapping gives every SIMD a wave
constexpr size_t kFrWideFrom = (size_t)256 * 4 * 64 * kFrWide;

struct FrenetParams {
  size_t n_queries;        // B K
  int n_center;            // >= 2
  int fields;              // doubles per row of `rows`: 2, 9, 10 or 11, which names the layout and so the column of x
  const double* center;    // [n_center][7] s x y theta kappa left_bound right_bound
  const double* xy;        // [n_center][2] the same x, y packed; 16-byte aligned
};

// rows [n_queries][fields] -> frenet [n_queries][8]; aligned as doubles, no more is assumed
void launch_frenet(const FrenetParams& P, const double* rows, double* frenet, hipStream_t st);
// sl [n][2] -> xyt [n][3]
void launch_cartesian(const double* center, int n_center, int n, const double* sl, double* xyt, hipStream_t st);

}  // namespace cilqr
