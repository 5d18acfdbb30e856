// Private to cilqr_amd/csrc: what the audits of one scene (host_planner.hip), the batched ones (collision_batch.hip,
// clearance_batch.hip) and kernels_collision.hip share -- the checks on the scalar arguments, the parameters of a launch and
// the launch function.  Every pointer of the launch is device memory; nothing here synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/cilqr.h"
#include "../../include/cilqr/row_layouts.hpp"

namespace cilqr {

// layout, knot count and buffer of either audit: CILQR_ERR_ARG / CILQR_ERR_CAPACITY / CILQR_OK
inline int check_audit_arguments(int layout, int n_knots, double collision_buffer) {
  if (pose_columns(layout).fields == 0 || n_knots < 1) return CILQR_ERR_ARG;
  if (!(collision_buffer >= 0.0) || !std::isfinite(collision_buffer)) return CILQR_ERR_ARG;
  if (n_knots > CILQR_DP_MAX_KNOTS) return CILQR_ERR_CAPACITY;
  return CILQR_OK;
}

// what a launch shares between its scenes: the vehicle's discs with the buffer already in the half side (DpEnvironment:
// disc_radius() + collision_buffer, added on the host as CollisionMask adds it), the x-sorted barrier table, the rows
struct CollisionParams {
  double h, r2x, f2x;
  int n_knots, n_barrier;
  int max_static, max_dynamic, max_vertices, max_samples;   // of the cilqr_scene_batch
  PoseColumns rows;        // what the audits read of a row (row_layouts.hpp)
  const double* barrier;   // [n_barrier][2], read through L2
};

// One workgroup per scene of `dv`, the batch with its arrays on the device.  mask [B][K] and n_hit [B] may be null;
// n_colliding (one int, zeroed by the caller) += the scenes with first_hit >= 0.
void launch_check_collisions(const CollisionParams& P, const cilqr_scene_batch& dv, const double* rows, uint8_t* mask,
                             int* first_hit, int* n_hit, int* n_colliding, hipStream_t st);

}  // namespace cilqr
