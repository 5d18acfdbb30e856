// Private to cilqr_amd/csrc: what cilqr_clearance_rows_batch (clearance_batch.hip) and kernels_clearance.hip share -- the
// parameters of a launch and the launch function.  The row layouts and the checks on the scalar arguments are the collision
// audit's (collision.hpp).  Every pointer of the launch is device memory; nothing here synchronises.
#pragma once
#include "collision.hpp"

namespace cilqr {

// what a launch shares between its scenes: the vehicle's discs (DpEnvironment's own numbers), the rows, the threshold of
// the count
struct ClearanceParams {
  double radius, r2x, f2x, threshold;
  int n_knots;
  int max_static, max_dynamic, max_vertices, max_samples;   // of the cilqr_scene_batch
  PoseColumns rows;
};

// One workgroup per scene of `dv`, the batch with its arrays on the device.  clearance [B][K][4] and nearest [B][K][4] may
// be null; n_below (one int, zeroed by the caller) += the scenes with min_clearance < threshold.
void launch_clearance(const ClearanceParams& P, const cilqr_scene_batch& dv, const double* rows, double* clearance,
                      int* nearest, double* min_clearance, int* min_knot, int* n_below, hipStream_t st);

}  // namespace cilqr
