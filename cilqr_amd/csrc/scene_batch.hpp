// Private to cilqr_amd/csrc: what the entry points that take a cilqr_scene_batch (planner_batch.hip, scene_pipeline.hip,
// collision_batch.hip, clearance_batch.hip; frenet_batch.hip and resample_batch.hip for the checks on the handle) share --
// the checks on the batch, in the order every one of them makes them -- and what they and the calls on one scene
// (host_planner.hip) hand to the host planner's classes: its configuration and its road.  The six arrays of a batch reach
// the device through staged_call::scenes (staging.hpp); SceneImage lays them out for the two pipelines, which keep them in
// a work block of their own beside their intermediates.
#pragma once
#include <array>
#include <vector>

#include "../../include/cilqr/dp_planner.hpp"
#include "staging.hpp"

namespace cilqr {

inline DpConfig dp_config_of(const cilqr_dp_config& c) {
  DpConfig d;
  d.tf = c.tf; d.delta_t = c.delta_t; d.dp_nominal_velocity = c.dp_nominal_velocity; d.dp_w_obstacle = c.dp_w_obstacle;
  d.dp_w_lateral = c.dp_w_lateral; d.dp_w_lateral_change = c.dp_w_lateral_change;
  d.dp_w_lateral_velocity_change = c.dp_w_lateral_velocity_change;
  d.dp_w_longitudinal_velocity_bias = c.dp_w_longitudinal_velocity_bias;
  d.dp_w_longitudinal_velocity_change = c.dp_w_longitudinal_velocity_change;
  d.front_hang_length = c.front_hang_length; d.wheel_base = c.wheel_base; d.rear_hang_length = c.rear_hang_length;
  d.width = c.width; d.max_velocity = c.max_velocity;
  return d;
}

// center [n][7]: s x y theta kappa left_bound right_bound
inline ReferenceLine reference_line_of(const double* center, int n) {
  std::vector<std::array<double, 7>> rows(n);
  for (int i = 0; i < n; ++i)
    for (int e = 0; e < 7; ++e) rows[i][e] = center[(size_t)i * 7 + e];
  return ReferenceLine(rows);
}

// shape, memory kind, the arrays the shape asks for
inline int check_scene_batch(const cilqr_scene_batch& sb) {
  if (sb.batch < 1 || sb.n_center < 2 || sb.max_static < 0 || sb.max_dynamic < 0 || sb.max_vertices < 0 || sb.max_samples < 0)
    return CILQR_ERR_ARG;
  if (sb.memory != CILQR_MEM_HOST && sb.memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  if ((sb.max_static > 0 && (sb.static_points == nullptr || sb.static_counts == nullptr)) ||
      (sb.max_dynamic > 0 && (sb.dynamic_polygon_points == nullptr || sb.dynamic_polygon_counts == nullptr ||
                              sb.dynamic_trajectories == nullptr || sb.dynamic_trajectory_counts == nullptr)))
    return CILQR_ERR_NULL;
  if ((sb.max_static > 0 || sb.max_dynamic > 0) && sb.max_vertices < 1) return CILQR_ERR_ARG;
  if (sb.max_dynamic > 0 && sb.max_samples < 1) return CILQR_ERR_ARG;
  return CILQR_OK;
}

inline bool beyond_limits(const cilqr_scene_batch& sb, int n_knots) {
  return sb.max_vertices > CILQR_DP_MAX_VERTICES || sb.max_static > CILQR_DP_MAX_STATIC ||
         sb.max_dynamic > CILQR_DP_MAX_DYNAMIC || sb.max_samples > CILQR_DP_MAX_SAMPLES || n_knots > CILQR_DP_MAX_KNOTS;
}

// counts of HOST arrays: negative, or above what the arrays store
inline bool host_counts_valid(const cilqr_scene_batch& sb) {
  const size_t B = (size_t)sb.batch;
  for (size_t i = 0; i < B * sb.max_static; ++i)
    if (sb.static_counts[i] < 0 || sb.static_counts[i] > sb.max_vertices) return false;
  for (size_t i = 0; i < B * sb.max_dynamic; ++i)
    if (sb.dynamic_polygon_counts[i] < 0 || sb.dynamic_polygon_counts[i] > sb.max_vertices ||
        sb.dynamic_trajectory_counts[i] < 0 || sb.dynamic_trajectory_counts[i] > sb.max_samples)
      return false;
  return true;
}

inline bool solves_in_flight(cilqr_solver* h) {
  std::lock_guard<std::mutex> lk(h->mu);
  return h->job_count != 0;   // submitted solves not collected yet (cilqr_wait)
}

// The six per-problem arrays of a scene batch as six slots of the caller's block (scene_pipeline.hip: a HOST batch on its
// way to the device; carry_pipeline.hip: the gathered scenes of a chunk).
struct SceneImage {
  slot sp, sc, dp, dpc, dt, dtc;   // named: carry_pipeline.hip gathers into each of them
  SceneImage(block_layout& L, const cilqr_scene_batch& sb) {
    slot* const s[] = {&sp, &sc, &dp, &dpc, &dt, &dtc};   // the order of scene_arrays, which states the sizes
    int i = 0;
    scene_arrays(sb, [&](auto member, size_t n) { *s[i++] = L.add(n * sizeof(*(sb.*member))); });
  }
  // the arrays of `sb` (HOST) into `block`; `view` = the batch with its arrays there
  int upload(const cilqr_scene_batch& sb, char* block, hipStream_t st, cilqr_scene_batch* view) const {
    if (int rc = copy_in(block, sp, sb.static_points, st)) return rc;
    if (int rc = copy_in(block, sc, sb.static_counts, st)) return rc;
    if (int rc = copy_in(block, dp, sb.dynamic_polygon_points, st)) return rc;
    if (int rc = copy_in(block, dpc, sb.dynamic_polygon_counts, st)) return rc;
    if (int rc = copy_in(block, dt, sb.dynamic_trajectories, st)) return rc;
    if (int rc = copy_in(block, dtc, sb.dynamic_trajectory_counts, st)) return rc;
    *view = sb;
    view->memory = CILQR_MEM_DEVICE;
    view->static_points = sp.in<const double>(block); view->static_counts = sc.in<const int32_t>(block);
    view->dynamic_polygon_points = dp.in<const double>(block); view->dynamic_polygon_counts = dpc.in<const int32_t>(block);
    view->dynamic_trajectories = dt.in<const double>(block); view->dynamic_trajectory_counts = dtc.in<const int32_t>(block);
    return CILQR_OK;
  }
};

}  // namespace cilqr
