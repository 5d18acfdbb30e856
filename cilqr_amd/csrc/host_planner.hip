// Host-side producers of the solve's inputs behind the C-ABI (include/cilqr.h, "coarse trajectory"):
// cilqr_dp_plan wraps the header-only planner of include/cilqr/dp_planner.hpp (DpPlanner::Plan,
// algorithm/planner/dp_planner.cpp:135-281 with ComputePathProfile, discrete_points_math.cc:27-176) for
// callers that are not C++ (the ctypes tests, the scene generator); cilqr_check_collisions asks DpEnvironment::CollisionMask
// about every knot of a trajectory (Environment::CheckOptimizationCollision, environment.cpp:92-111), cilqr_clearance_rows
// asks DpEnvironment::Clearance (Polygon2d::DistanceTo, polygon2d.cpp:43-52); cilqr_window_scene cuts the window of
// include/cilqr/scene_window.hpp out of a scene's trajectories, cilqr_predict_scene makes the prediction of
// include/cilqr/scene_predict.hpp from them.  No device code in this file.
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/cilqr/scene_window.hpp"
#include "collision.hpp"
#include "scene_batch.hpp"
#include "scene_predict.hpp"

namespace {

// what the two audits of one scene (cilqr_check_collisions, cilqr_clearance_rows) check about it, in this order around
// their own arguments: the shape and the arrays it asks for, then the counts
int check_scene_shape(const cilqr_scene& scene) {
  if (scene.n_center < 2 || scene.n_static < 0 || scene.n_dynamic < 0) return CILQR_ERR_ARG;
  if ((scene.n_static > 0 && (scene.static_points == nullptr || scene.static_counts == nullptr)) ||
      (scene.n_dynamic > 0 && (scene.dynamic_polygon_points == nullptr || scene.dynamic_polygon_counts == nullptr ||
                               scene.dynamic_trajectories == nullptr || scene.dynamic_trajectory_counts == nullptr)))
    return CILQR_ERR_NULL;
  return CILQR_OK;
}
int check_scene_counts(const cilqr_scene& scene) {
  if (scene.n_static > CILQR_DP_MAX_STATIC || scene.n_dynamic > CILQR_DP_MAX_DYNAMIC) return CILQR_ERR_CAPACITY;
  for (int o = 0; o < scene.n_static; ++o)
    if (scene.static_counts[o] < 0) return CILQR_ERR_ARG;
  for (int o = 0; o < scene.n_dynamic; ++o)
    if (scene.dynamic_polygon_counts[o] < 0 || scene.dynamic_trajectory_counts[o] < 0) return CILQR_ERR_ARG;
  for (int o = 0; o < scene.n_static; ++o)
    if (scene.static_counts[o] > CILQR_DP_MAX_VERTICES) return CILQR_ERR_CAPACITY;
  for (int o = 0; o < scene.n_dynamic; ++o)
    if (scene.dynamic_polygon_counts[o] > CILQR_DP_MAX_VERTICES || scene.dynamic_trajectory_counts[o] > CILQR_DP_MAX_SAMPLES)
      return CILQR_ERR_CAPACITY;
  return CILQR_OK;
}

// the environment of a checked scene, and the slot of every obstacle it kept
struct AuditScene {
  cilqr::DpEnvironment env;
  std::vector<int> static_slot, dynamic_slot;
  AuditScene(const cilqr_dp_config& cfg, const cilqr_scene& scene) {
    env = cilqr::DpEnvironment(cilqr::dp_config_of(cfg), cilqr::reference_line_of(scene.center, scene.n_center));
    size_t at = 0;
    for (int o = 0; o < scene.n_static; ++o) {
      std::vector<cilqr::DpPoint2> poly(scene.static_counts[o]);
      for (auto& p : poly) {
        p = cilqr::DpPoint2{scene.static_points[at * 2], scene.static_points[at * 2 + 1]};
        ++at;
      }
      if (!poly.empty()) {   // no vertices: the slot is unused
        env.AddStatic(poly);
        static_slot.push_back(o);
      }
    }
    size_t pa = 0, ta = 0;
    for (int o = 0; o < scene.n_dynamic; ++o) {
      const int m = scene.dynamic_polygon_counts[o], T = scene.dynamic_trajectory_counts[o];
      std::vector<cilqr::DpPoint2> poly(m);
      for (int k = 0; k < m; ++k) poly[k] = cilqr::DpPoint2{scene.dynamic_polygon_points[(pa + k) * 2], scene.dynamic_polygon_points[(pa + k) * 2 + 1]};
      std::vector<std::array<double, 4>> traj(T);
      for (int t = 0; t < T; ++t)
        for (int e = 0; e < 4; ++e) traj[t][e] = scene.dynamic_trajectories[(ta + t) * 4 + e];
      if (m > 0 && T > 0) {   // an obstacle without vertices or samples is never there
        env.AddDynamic(poly, traj);
        dynamic_slot.push_back(o);
      }
      pa += m;
      ta += T;
    }
  }
};

}  // namespace

extern "C" {

void cilqr_default_dp_config(cilqr_dp_config* c) {
  if (c == nullptr) return;
  const cilqr::DpConfig d;   // default member initialisers = planner_config.h:94-133, vehicle_param.h:26-46
  c->tf = d.tf; c->delta_t = d.delta_t; c->dp_nominal_velocity = d.dp_nominal_velocity; c->dp_w_obstacle = d.dp_w_obstacle;
  c->dp_w_lateral = d.dp_w_lateral; c->dp_w_lateral_change = d.dp_w_lateral_change;
  c->dp_w_lateral_velocity_change = d.dp_w_lateral_velocity_change;
  c->dp_w_longitudinal_velocity_bias = d.dp_w_longitudinal_velocity_bias;
  c->dp_w_longitudinal_velocity_change = d.dp_w_longitudinal_velocity_change;
  c->front_hang_length = d.front_hang_length; c->wheel_base = d.wheel_base; c->rear_hang_length = d.rear_hang_length;
  c->width = d.width; c->max_velocity = d.max_velocity;
}

int cilqr_road_barriers(const double* center, int32_t n_center, double* left, double* right, int32_t max_points) {
  if (center == nullptr || left == nullptr || right == nullptr) return CILQR_ERR_NULL;
  if (n_center < 2 || max_points < 1) return CILQR_ERR_ARG;
  const cilqr::ReferenceLine ref = cilqr::reference_line_of(center, n_center);
  constexpr double kSampleStep = 0.1;                                   // environment.cpp:18
  const double start_s = center[0], back_s = center[(size_t)(n_center - 1) * 7];
  const int sample_points = int((back_s - start_s) / kSampleStep);      // cpp:29-31
  if (sample_points + 1 > max_points) return CILQR_ERR_CAPACITY;
  for (int i = 0; i <= sample_points; ++i) {
    const double s = start_s + i * kSampleStep;
    const cilqr::RefPoint r = ref.EvaluateStation(s);
    const cilqr::DpPoint2 l = ref.GetCartesian(s, r.left_bound), q = ref.GetCartesian(s, -r.right_bound);   // cpp:38-39
    left[2 * i] = l.x; left[2 * i + 1] = l.y;
    right[2 * i] = q.x; right[2 * i + 1] = q.y;
  }
  return sample_points + 1;
}

int cilqr_dp_plan(const cilqr_dp_config* cfg, const cilqr_scene* scene, const double* start3, double* coarse,
                  int32_t n_knots) {
  if (cfg == nullptr || scene == nullptr || start3 == nullptr || coarse == nullptr || scene->center == nullptr)
    return CILQR_ERR_NULL;
  if (scene->n_center < 2 || scene->n_static < 0 || scene->n_dynamic < 0 || !(cfg->delta_t > 0.0) || !(cfg->tf > 0.0))
    return CILQR_ERR_ARG;
  if ((scene->n_static > 0 && (scene->static_points == nullptr || scene->static_counts == nullptr)) ||
      (scene->n_dynamic > 0 && (scene->dynamic_polygon_points == nullptr || scene->dynamic_polygon_counts == nullptr ||
                                scene->dynamic_trajectories == nullptr || scene->dynamic_trajectory_counts == nullptr)))
    return CILQR_ERR_NULL;
  const cilqr::DpConfig d = cilqr::dp_config_of(*cfg);
  if ((int32_t)(d.tf / d.delta_t + 1) != n_knots) return CILQR_ERR_KNOTS;
  cilqr::DpEnvironment env(d, cilqr::reference_line_of(scene->center, scene->n_center));
  size_t at = 0;
  for (int o = 0; o < scene->n_static; ++o) {
    if (scene->static_counts[o] < 1) return CILQR_ERR_ARG;
    std::vector<cilqr::DpPoint2> poly(scene->static_counts[o]);
    for (auto& p : poly) {
      p = cilqr::DpPoint2{scene->static_points[at * 2], scene->static_points[at * 2 + 1]};
      ++at;
    }
    env.AddStatic(poly);
  }
  size_t pa = 0, ta = 0;
  for (int o = 0; o < scene->n_dynamic; ++o) {
    const int m = scene->dynamic_polygon_counts[o], T = scene->dynamic_trajectory_counts[o];
    if (m < 1 || T < 0) return CILQR_ERR_ARG;
    std::vector<cilqr::DpPoint2> poly(m);
    for (int k = 0; k < m; ++k) poly[k] = cilqr::DpPoint2{scene->dynamic_polygon_points[(pa + k) * 2], scene->dynamic_polygon_points[(pa + k) * 2 + 1]};
    std::vector<std::array<double, 4>> traj(T);
    for (int t = 0; t < T; ++t)
      for (int e = 0; e < 4; ++e) traj[t][e] = scene->dynamic_trajectories[(ta + t) * 4 + e];
    env.AddDynamic(poly, traj);
    pa += m;
    ta += T;
  }
  cilqr::DpPlanner dp(d, &env);
  std::vector<cilqr::CoarsePoint> out;
  const bool ok = dp.Plan(start3[0], start3[1], start3[2], &out);
  if ((int32_t)out.size() != n_knots) return CILQR_ERR_KNOTS;
  constexpr cilqr::RowColumns C = cilqr::row_columns(CILQR_ROWS_COARSE);
  for (int i = 0; i < n_knots; ++i) {
    double* r = coarse + (size_t)i * C.fields;
    const cilqr::CoarsePoint& p = out[i];
    r[C.time] = p.time; r[C.station] = p.s; r[C.x] = p.x; r[C.y] = p.y; r[C.theta] = p.theta; r[C.kappa] = p.kappa;
    r[C.v] = p.velocity; r[C.a] = p.a; r[C.delta] = p.delta;
  }
  return ok ? CILQR_OK : CILQR_ERR_NO_PATH;
}

int cilqr_check_collisions(const cilqr_dp_config* cfg, const cilqr_scene* scene, int32_t layout, const double* rows,
                           int32_t n_knots, double collision_buffer, uint8_t* mask, int32_t* first_hit, int32_t* n_hit) {
  if (cfg == nullptr || scene == nullptr || rows == nullptr || first_hit == nullptr || scene->center == nullptr)
    return CILQR_ERR_NULL;
  if (int rc = check_scene_shape(*scene)) return rc;
  if (int rc = cilqr::check_audit_arguments(layout, n_knots, collision_buffer)) return rc;
  if (int rc = check_scene_counts(*scene)) return rc;

  const AuditScene audit(*cfg, *scene);
  const cilqr::PoseColumns L = cilqr::pose_columns(layout);
  int first = -1, count = 0;
  for (int k = 0; k < n_knots; ++k) {
    const double* r = rows + (size_t)k * L.fields;
    const unsigned bits = audit.env.CollisionMask(r[L.time], r[L.x], r[L.y], r[L.theta], collision_buffer);
    if (mask) mask[k] = (uint8_t)bits;
    if (bits != 0u) {
      if (first < 0) first = k;
      ++count;
    }
  }
  *first_hit = first;
  if (n_hit) *n_hit = count;
  return CILQR_OK;
}

int cilqr_clearance_rows(const cilqr_dp_config* cfg, const cilqr_scene* scene, int32_t layout, const double* rows,
                         int32_t n_knots, double* clearance, int32_t* nearest, double* min_clearance, int32_t* min_knot) {
  if (cfg == nullptr || scene == nullptr || rows == nullptr || clearance == nullptr || min_clearance == nullptr ||
      min_knot == nullptr || scene->center == nullptr)
    return CILQR_ERR_NULL;
  if (int rc = check_scene_shape(*scene)) return rc;
  if (int rc = cilqr::check_audit_arguments(layout, n_knots, 0.0)) return rc;
  if (int rc = check_scene_counts(*scene)) return rc;

  const AuditScene audit(*cfg, *scene);
  const cilqr::PoseColumns L = cilqr::pose_columns(layout);
  double lowest = std::numeric_limits<double>::infinity();
  int at = -1;
  for (int k = 0; k < n_knots; ++k) {
    const double* r = rows + (size_t)k * L.fields;
    const cilqr::DpEnvironment::ClearanceRow row = audit.env.Clearance(r[L.time], r[L.x], r[L.y], r[L.theta]);
    for (int c = 0; c < CILQR_CLEARANCE_FIELDS; ++c) {
      clearance[(size_t)k * CILQR_CLEARANCE_FIELDS + c] = row.clearance[c];
      if (nearest) {   // the environment counts the obstacles it kept; the caller counts slots
        const std::vector<int>& slot_of = (c & 1) ? audit.dynamic_slot : audit.static_slot;
        nearest[(size_t)k * CILQR_CLEARANCE_FIELDS + c] = row.nearest[c] < 0 ? -1 : slot_of[row.nearest[c]];
      }
      if (row.clearance[c] < lowest) {
        lowest = row.clearance[c];
        at = k;
      }
    }
  }
  *min_clearance = lowest;
  *min_knot = at;
  return CILQR_OK;
}

int cilqr_window_scene(const cilqr_scene* scene, double t0, double span, int32_t out_samples, double* trajectories,
                       int32_t* counts, int32_t* n_overflow) {
  if (scene == nullptr) return CILQR_ERR_NULL;
  if (scene->n_dynamic < 0) return CILQR_ERR_ARG;
  if (scene->n_dynamic > 0 && (scene->dynamic_trajectories == nullptr || scene->dynamic_trajectory_counts == nullptr ||
                               trajectories == nullptr || counts == nullptr))
    return CILQR_ERR_NULL;
  if (!std::isfinite(t0) || !std::isfinite(span) || span < 0.0 || out_samples < 1) return CILQR_ERR_ARG;
  for (int o = 0; o < scene->n_dynamic; ++o)
    if (scene->dynamic_trajectory_counts[o] < 0) return CILQR_ERR_ARG;
  size_t at = 0;
  int overflow = 0;
  for (int o = 0; o < scene->n_dynamic; ++o) {
    const int T = scene->dynamic_trajectory_counts[o];
    counts[o] = cilqr::scene_window::window_trajectory(scene->dynamic_trajectories + at * 4, T, t0, span, out_samples,
                                                       trajectories + (size_t)o * out_samples * 4);
    if (counts[o] < 0) ++overflow;
    at += T;
  }
  if (n_overflow) *n_overflow = overflow;
  return CILQR_OK;
}

int cilqr_predict_scene(const cilqr_scene* scene, double t0, double span, int32_t mode, double max_age, double sample_dt,
                        int32_t out_samples, double* trajectories, int32_t* counts, int32_t* n_refused) {
  if (scene == nullptr) return CILQR_ERR_NULL;
  if (scene->n_dynamic < 0) return CILQR_ERR_ARG;
  if (scene->n_dynamic > 0 && (scene->dynamic_trajectories == nullptr || scene->dynamic_trajectory_counts == nullptr ||
                               trajectories == nullptr || counts == nullptr))
    return CILQR_ERR_NULL;
  if (!std::isfinite(t0)) return CILQR_ERR_ARG;
  if (int rc = cilqr::check_prediction(span, mode, max_age, sample_dt, out_samples)) return rc;
  size_t at = 0;
  int refused = 0;
  for (int o = 0; o < scene->n_dynamic; ++o) {
    const int T = scene->dynamic_trajectory_counts[o];
    if (T < 0) {   // the rule's refusal: this obstacle alone, and no samples of the packed array are its
      counts[o] = -1;
      ++refused;
      continue;
    }
    counts[o] = cilqr::scene_predict::predict_trajectory(scene->dynamic_trajectories + at * 4, T, t0, mode, max_age, sample_dt,
                                                         out_samples, trajectories + (size_t)o * out_samples * 4);
    at += T;
  }
  if (n_refused) *n_refused = refused;
  return CILQR_OK;
}

}  // extern "C"
