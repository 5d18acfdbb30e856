// Private to cilqr_amd/csrc: what the host sides of the two batched audits (collision_batch.hip, clearance_batch.hip)
// have literally in common -- the checks around their own arguments and the limits of the batch as launch parameters.
#pragma once
#include "collision.hpp"
#include "scene_batch.hpp"

namespace cilqr {

// before an audit's own scalar checks: the batch, then layout, knot count and buffer
inline int check_audit_batch(const cilqr_scene_batch& sb, int layout, int n_knots, double collision_buffer) {
  if (int rc = check_scene_batch(sb)) return rc;
  return check_audit_arguments(layout, n_knots, collision_buffer);
}
// after them: the declared limits, the handle, the counts of HOST arrays
inline int check_audit_admissible(cilqr_solver* h, const cilqr_scene_batch& sb, int n_knots) {
  if (beyond_limits(sb, n_knots)) return CILQR_ERR_CAPACITY;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;
  if (sb.memory == CILQR_MEM_HOST && !host_counts_valid(sb)) return CILQR_ERR_ARG;
  return CILQR_OK;
}

// max_* of the batch into the parameters of a launch
template <class Params>
void scene_limits_into(Params* P, const cilqr_scene_batch& sb) {
  P->max_static = sb.max_static; P->max_dynamic = sb.max_dynamic; P->max_vertices = sb.max_vertices; P->max_samples = sb.max_samples;
}

}  // namespace cilqr
