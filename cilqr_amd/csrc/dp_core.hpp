// Device functions of the batched DP coarse planner (kernels_dp.hip; C-ABI: cilqr_dp_plan_batch).
//
// The arithmetic is include/cilqr/dp_planner.hpp, expression by expression and in that header's order (which is the
// reference's: algorithm/planner/dp_planner.cpp, algorithm/utils/discretized_trajectory.cpp, environment.cpp,
// algorithm/math/polygon2d.cpp, box2d.cpp): the DP decides with strict '<', so a sum in another order could pick another
// cell.  Built with -ffp-contract=off like everything else here.  std::min(a, b) / std::max(a, b) are written out as the
// selects they are ((b < a) ? b : a, (a < b) ? b : a): fmin / fmax treat a NaN differently.  What is NOT the host's
// arithmetic: sin / cos (lean_sincos, dev_model.hpp) and atan (the device library) -- they enter the positions of the
// collision discs, x / y and the headings, never a cost, a station or a time.  hypot is the libm-identical hypot_ref and
// NormalizeAngle the exact normalize_angle, so the Frenet coordinates of the start are the host's bits.
#pragma once

#include "../../include/cilqr.h"
#include "scene_core.hpp"

namespace cilqr {

constexpr int kDpLayers = 5, kDpStations = 7, kDpLaterals = 10;   // dp_planner.h:27-29
constexpr int kDpCells = kDpStations * kDpLaterals;                // cells of a layer, si-major / li-minor
constexpr int kDpMaxV = 8;                                         // CILQR_DP_MAX_VERTICES
constexpr int kDpRec = 4 + 2 * kDpMaxV;                            // a static polygon in LDS: min_x max_x min_y max_y, vertices
constexpr double kDpEps = 1e-3;                                    // dp_planner.cpp:25

// everything a call shares between its scenes: the lattice as DpPlanner's constructor lays it out, the vehicle's discs
// (DpEnvironment), and the two tables built on the host once per call and read through L2 by every workgroup
struct DpParams {
  double delta_t, unit_time, safe_margin, radius, r2x, f2x, wheel_base;
  double w_obstacle, w_lateral, w_lateral_change, w_lateral_velocity_change, w_velocity_bias, w_velocity_change;
  double nominal_velocity;
  double time[kDpLayers], station[kDpStations], lateral[kDpLaterals - 1];
  int nseg[kDpLayers];        // CountSegmentPoints per layer (a loop that accumulates t += delta_t: counted on the host)
  int qoff[kDpLayers + 1];    // first path sample of every layer among the nq samples of a path
  int nq;
  int n_center, n_barrier, n_knots;
  int max_static, max_dynamic, max_vertices, max_samples;
  const double* center;       // [n_center][7] s x y theta kappa left_bound right_bound
  const double* barrier;      // [n_barrier][2] both road barriers, sorted by x (Environment::set_reference)
};

// kernels_dp.hip.  `dv`: the batch with its arrays on the device; scenes [first, first + n_scenes) of them, the placed
// polygons start at the FIRST of these scenes
void launch_dp_place(const DpParams& P, const cilqr_scene_batch& dv, int first, int n_scenes, double* placed, int* placed_n,
                     hipStream_t st);
void launch_dp_plan(const DpParams& P, const cilqr_scene_batch& dv, int first, int n_scenes, const double* start3,
                    const double* placed, const int* placed_n, double* coarse9, double* coarse6, double* knots3,
                    double* station, int* found, int* n_not_found, hipStream_t st);

struct DpRef {
  double s, x, y, theta, kappa, left_bound, right_bound;
};

CILQR_DEV DpRef dp_center_point(const DpParams& P, int i) {
  const double* c = P.center + (size_t)i * 7;
  return DpRef{c[0], c[1], c[2], c[3], c[4], c[5], c[6]};
}

// The three functions below keep copies of their own of row_math.hpp's pair step (on a struct) and bracket_pair (the same
// halving written with lo / hi, without the upper clamp); slerp and the epsilon are the shared ones.  As calls of the shared
// functions they changed the code of k_dp_plan and k_cartesian, and each fell outside what the parent's own runs spread over
// in one of two sessions (profiles/row_math_parent_vs_branch.json).
CILQR_DEV DpRef dp_interpolate(const DpRef& p0, const DpRef& p1, double s) {   // discretized_trajectory.cpp:66-89
  const double s0 = p0.s, s1 = p1.s;
  if (fabs(s1 - s0) < kMathEps) return p0;
  DpRef pt;
  const double weight = (s - s0) / (s1 - s0);
  pt.s = s;
  pt.x = (1 - weight) * p0.x + weight * p1.x;
  pt.y = (1 - weight) * p0.y + weight * p1.y;
  pt.theta = slerp(p0.theta, p0.s, p1.theta, p1.s, s);
  pt.kappa = (1 - weight) * p0.kappa + weight * p1.kappa;
  pt.left_bound = (1 - weight) * p0.left_bound + weight * p1.left_bound;
  pt.right_bound = (1 - weight) * p0.right_bound + weight * p1.right_bound;
  return pt;
}

// discretized_trajectory.cpp:117-128: the pair of centre points a station lies between
CILQR_DEV int dp_station_index(const DpParams& P, double station) {
  const int n = P.n_center;
  int it;
  if (station >= P.center[(size_t)(n - 1) * 7]) {
    it = n - 1;
  } else if (station < P.center[0]) {
    it = 0;
  } else {
    int lo = 0, hi = n;   // first point with s >= station
    while (lo < hi) {
      const int mid = (lo + hi) / 2;
      if (P.center[(size_t)mid * 7] < station) lo = mid + 1;
      else hi = mid;
    }
    it = lo;
  }
  if (it == 0) it = 1;
  return it;
}
CILQR_DEV DpRef dp_evaluate_station(const DpParams& P, double station) {
  const int it = dp_station_index(P, station);
  return dp_interpolate(dp_center_point(P, it - 1), dp_center_point(P, it), station);
}
// the two bounds alone (LateralAt needs nothing else of the point)
CILQR_DEV void dp_bounds_at(const DpParams& P, double station, double* left_bound, double* right_bound) {
  const int it = dp_station_index(P, station);
  const double* p0 = P.center + (size_t)(it - 1) * 7;
  const double* p1 = p0 + 7;
  const double s0 = p0[0], s1 = p1[0];
  if (fabs(s1 - s0) < kMathEps) {
    *left_bound = p0[5];
    *right_bound = p0[6];
    return;
  }
  const double weight = (station - s0) / (s1 - s0);
  *left_bound = (1 - weight) * p0[5] + weight * p1[5];
  *right_bound = (1 - weight) * p0[6] + weight * p1[6];
}

CILQR_DEV double dp_lateral_at(const DpParams& P, double s, int l_ind) {   // dp_planner.h:84-92
  if (l_ind == kDpLaterals - 1) return 0.0;
  double left_bound, right_bound;
  dp_bounds_at(P, s, &left_bound, &right_bound);
  const double lb = -right_bound + P.safe_margin;
  const double ub = left_bound - P.safe_margin;
  return lb + (ub - lb) * P.lateral[l_ind];
}

// ---- collision tests (environment.cpp:45-130, polygon2d.cpp:120-164, box2d.cpp:93-129) ----
struct DpSquare {
  double cx, cy, h, min_x, max_x, min_y, max_y;
};
CILQR_DEV DpSquare dp_square(const DpParams& P, double cx, double cy) {
  return DpSquare{cx, cy, P.radius, cx - P.radius, cx + P.radius, cy - P.radius, cy + P.radius};
}
// the same square with its half side given (kernels_collision.hip: radius + collision_buffer)
CILQR_DEV DpSquare dp_square_of(double h, double cx, double cy) { return DpSquare{cx, cy, h, cx - h, cx + h, cy - h, cy + h}; }
CILQR_DEV bool dp_square_has_point(const DpSquare& b, double px, double py) {   // Box2d::IsPointIn, heading 0
  const double x0 = px - b.cx, y0 = py - b.cy;
  const double dx = fabs(x0 * 1.0 + y0 * 0.0);
  const double dy = fabs(-x0 * 0.0 + y0 * 1.0);
  return dx <= b.h + kMathEps && dy <= b.h + kMathEps;
}
// a placed polygon: box[4] = min_x max_x min_y max_y, pts[n][2]
CILQR_DEV bool dp_poly_has_point(const double* box, const double* pts, int n, double px, double py) {
  if (px < box[0] || px > box[1] || py < box[2] || py > box[3]) return false;
  int j = n - 1, c = 0;
  for (int i = 0; i < n; ++i) {
    const double xi = pts[2 * i], yi = pts[2 * i + 1], xj = pts[2 * j], yj = pts[2 * j + 1];
    if ((yi > py) != (yj > py)) {
      const double side = (xi - px) * (yj - py) - (xj - px) * (yi - py);
      if (yi < yj ? side > 0.0 : side < 0.0) ++c;
    }
    j = i;
  }
  return (c & 1) != 0;
}
CILQR_DEV bool dp_overlap(const double* box, const double* pts, int n, const DpSquare& b) {
  if (b.max_x < box[0] || b.min_x > box[1] || b.max_y < box[2] || b.min_y > box[3]) return false;
  for (int i = 0; i < n; ++i)
    if (dp_square_has_point(b, pts[2 * i], pts[2 * i + 1])) return true;
  return dp_poly_has_point(box, pts, n, b.cx + b.h, b.cy - b.h) || dp_poly_has_point(box, pts, n, b.cx + b.h, b.cy + b.h) ||
         dp_poly_has_point(box, pts, n, b.cx - b.h, b.cy + b.h) || dp_poly_has_point(box, pts, n, b.cx - b.h, b.cy - b.h);
}

// the obstacles of one scene as a workgroup sees them
struct DpScene {
  const double* statics;      // LDS: [max_static][kDpRec]
  const int* static_n;        // LDS: [max_static] vertices, 0 = unused
  const double* placed;       // global: [nq][max_dynamic][4 + 2 max_vertices] the polygon each obstacle shows at path sample q
  const int* placed_n;        // global: [nq][max_dynamic] vertices, 0 = not there at that time
};

CILQR_DEV bool dp_static_collision(const DpParams& P, const DpScene& S, double cx, double cy) {   // environment.cpp:45-80
  const DpSquare b = dp_square(P, cx, cy);
  for (int o = 0; o < P.max_static; ++o) {
    const int n = S.static_n[o];
    if (n > 0 && dp_overlap(S.statics + o * kDpRec, S.statics + o * kDpRec + 4, n, b)) return true;
  }
  // the window of scene_barrier_window (scene_core.hpp), written out: k_dp_plan measured 3 % slower with the call inlined
  const int nb = P.n_barrier;
  if (nb == 0) return false;
  if (b.max_x < P.barrier[0] || b.min_x > P.barrier[(size_t)(nb - 1) * 2]) return false;
  auto upper = [&](double val) {   // first barrier point with val < point.x
    int lo = 0, hi = nb;
    while (lo < hi) {
      const int mid = (lo + hi) / 2;
      if (val < P.barrier[(size_t)mid * 2]) hi = mid;
      else lo = mid + 1;
    }
    return lo;
  };
  int first = upper(b.min_x);
  const int last = upper(b.max_x);
  if (first > 0) --first;
  for (int i = first; i < last; ++i)
    if (dp_square_has_point(b, P.barrier[(size_t)i * 2], P.barrier[(size_t)i * 2 + 1])) return true;
  return false;
}
CILQR_DEV bool dp_dynamic_collision(const DpParams& P, const DpScene& S, int q, double cx, double cy) {   // environment.cpp:113-130
  const DpSquare b = dp_square(P, cx, cy);
  const int rec = 4 + 2 * P.max_vertices;
  for (int d = 0; d < P.max_dynamic; ++d) {
    const int n = S.placed_n[q * P.max_dynamic + d];
    if (n <= 0) continue;
    const double* r = S.placed + ((size_t)q * P.max_dynamic + d) * rec;
    if (dp_overlap(r, r + 4, n, b)) return true;
  }
  return false;
}
// environment.cpp:92-111 (collision_buffer = 0) at path sample q, whose time selected the placed polygons
CILQR_DEV bool dp_check_collision(const DpParams& P, const DpScene& S, int q, double x, double y, double theta) {
  double c[4];   // rear, front
  scene_discs_of_pose(x, y, theta, P.r2x, P.f2x, c);
  return dp_static_collision(P, S, c[0], c[1]) || dp_static_collision(P, S, c[2], c[3]) ||
         dp_dynamic_collision(P, S, q, c[0], c[1]) || dp_dynamic_collision(P, S, q, c[2], c[3]);
}

// ---- the lattice ----
// What a transition needs to know about the cell it starts from (dp_planner.hpp: Origin)
struct DpOrigin {
  double s, l, before_s, before_l, tail_s, tail_l, cost;
};

// Does the sampled segment from `from` to (.., end_l) leave the road or hit something (dp_planner.cpp:63-85)?
CILQR_DEV bool dp_segment_blocked(const DpParams& P, const DpScene& S, const DpOrigin& from, int layer, int si, double end_l) {
  const int n = P.nseg[layer];
  const double step_s = P.station[si] / n;
  const double step_l = (end_l - from.l) / n;
  double seen_s = from.tail_s, seen_l = from.tail_l;
  for (int i = 0; i < n; ++i) {
    const double at_s = from.s + i * step_s, at_l = from.l + i * step_l;
    const double rise = at_l - seen_l;
    const double run = dp_max(at_s - seen_s, kDpEps);
    seen_l = at_l;
    seen_s = at_s;
    const DpRef r = dp_evaluate_station(P, at_s);
    const double lo = dp_min(0.0, -r.right_bound + P.safe_margin);
    const double hi = dp_max(0.0, r.left_bound - P.safe_margin);
    if (at_l < lo - kDpEps || at_l > hi + kDpEps) return true;
    double sn, cs;
    lean_sincos(r.theta, &sn, &cs);
    const double cx = r.x - at_l * sn, cy = r.y + at_l * cs;
    const double heading = r.theta + atan((rise / run) / (1 - r.kappa * at_l));
    // the time of the sample, from.time + i * (unit_time / n), depends on (layer, i) alone: it chose the placed polygons
    // of path sample qoff[layer] + i in the pre-pass
    if (dp_check_collision(P, S, P.qoff[layer] + i, cx, cy, heading)) return true;
  }
  return false;
}

// cost of going from `from` to sample (si, li) of `layer` (dp_planner.cpp:88-133); the station reached is from.s + station[si]
CILQR_DEV double dp_transition(const DpParams& P, const DpScene& S, const DpOrigin& from, int layer, int si, int li) {
  const double to_s = from.s + P.station[si];
  const double to_l = dp_lateral_at(P, to_s, li);
  if (dp_segment_blocked(P, S, from, layer, si, to_l)) return P.w_obstacle;
  const double advance = to_s - from.s, advance_before = from.s - from.before_s;
  const double shift = to_l - from.l, shift_before = from.l - from.before_l;
  const double off_centre = fabs(to_l);
  const double slope = fabs(from.l - to_l) / (P.station[si] + kDpEps);
  const double lateral_rate_jump = fabs(shift - shift_before) / P.unit_time;
  const double speed_error = fabs(advance / P.unit_time - P.nominal_velocity);
  const double speed_jump = fabs((advance - advance_before) / P.unit_time);
  return (P.w_lateral * off_centre + P.w_lateral_change * slope + P.w_lateral_velocity_change * lateral_rate_jump +
          P.w_velocity_bias * speed_error + P.w_velocity_change * speed_jump);
}

}  // namespace cilqr
