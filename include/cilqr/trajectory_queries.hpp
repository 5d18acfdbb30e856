// include/cilqr/trajectory_queries.hpp -- DiscretizedTrajectory::EvaluateTime / EvaluateStation
// (algorithm/utils/discretized_trajectory.cpp:50-136, math::slerp math_utils.h:208-225) on rows in the layouts of
// include/cilqr.h: the host statement of cilqr_resample_rows, which cilqr_resample_rows_batch is held to bit for bit.
// Further down, GetProjection / GetCartesian (cpp:138-196) on a centre line: the host statement of cilqr_frenet_rows and
// cilqr_cartesian_points.  Between the two, the carry rule on top of EvaluateTime: the host statement of cilqr_carry_rows; and
// the stop rule on top of EvaluateStation: the host statement of cilqr_stop_rows.
// Header-only, C++14, no HIP.  The rules are stated once, in include/cilqr.h ("resample", "frenet"); this file follows
// them step by step.  NormalizeAngle, slerp, the bracket and the pair step are the functions of row_math.hpp, and
// stop_step is stated here: those the kernels RUN; the order of the steps around them a kernel follows on its own.
#ifndef CILQR_TRAJECTORY_QUERIES_HPP_
#define CILQR_TRAJECTORY_QUERIES_HPP_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "row_math.hpp"

namespace cilqr {
namespace trajectory_queries {

// the columns of a trajectory layout (CILQR_ROWS_TRAJ 0 / _PLAN 1 / _COARSE 2, row_layouts.hpp); fields = 0: no such layout
using Columns = RowColumns;
constexpr Columns columns_of(int layout) { return trajectory_columns(layout); }
// the key column of (layout, key) with key = CILQR_KEY_TIME 0 / CILQR_KEY_STATION 1; -1: no such pair
inline int key_column(int layout, int key) {
  const Columns c = columns_of(layout);
  if (c.fields == 0) return -1;
  if (key == 0) return c.time;
  if (key == 1) return c.station;
  return -1;
}

inline double NormalizeAngle(double angle) { return normalize_angle(angle); }
using cilqr::slerp;

// the row index i (1 <= i <= n_knots - 1) of p1; p0 is row i - 1.  rows [n_knots][fields], n_knots >= 2.
inline int bracket(const double* rows, int fields, int key_col, int n_knots, double q) {
  return bracket_pair(n_knots, q, [=](int r) { return rows[(size_t)r * fields + key_col]; });
}

// one output row from the pair (p0, p1) of a layout
inline void interpolate(const Columns& c, int key_col, const double* p0, const double* p1, double q, double* out) {
  pair_step(pair_all(c), key_col, p0[key_col], p1[key_col], q, p0, p1, out);
}

// rows [n_knots][fields] -> out [n_queries][fields]; the arguments are taken as checked (cilqr_resample_rows)
inline void resample_rows(int layout, const double* rows, int n_knots, int key, const double* queries, int n_queries,
                          double* out) {
  const Columns c = columns_of(layout);
  const int kc = key_column(layout, key);
  for (int m = 0; m < n_queries; ++m) {
    const int i = bracket(rows, c.fields, kc, n_knots, queries[m]);
    interpolate(c, kc, rows + (size_t)(i - 1) * c.fields, rows + (size_t)i * c.fields, queries[m],
                out + (size_t)m * c.fields);
  }
}

// ---- carry: a trajectory of the previous cycle as the coarse trajectory of the next: the host statement of cilqr_carry_rows
// and cilqr_carry_rows_batch.  The rule is stated in include/cilqr.h ("carry").
constexpr int kCoarseFields = 9;   // time s x y theta kappa velocity a delta
// what a coarse row takes from a row, in the order of its columns 2 ... 8
struct CarryColumns {
  int col[7];
};
constexpr CarryColumns carry_columns(const RowColumns& c) { return CarryColumns{{c.x, c.y, c.theta, c.kappa, c.v, c.a, c.delta}}; }
// ... as an instance of the pair step: out[0 ... 6]
constexpr PairColumns pair_carry(const RowColumns& c) {
  PairColumns L{};
  for (int e = 0; e < 7; ++e) L = pair_with(L, carry_columns(c).col[e], e, e == 2 ? kPairSlerp : kPairLerp);
  return L;
}

// rows [n_rows][fields] -> coarse9 [n_knots][9], coarse6 [n_knots][6], knots3 [n_knots][3], station [n_knots] (each may be
// null); returns the state (0 kept, 1 not asked, 2 refused).  The arguments are taken as checked (cilqr_carry_rows).
inline int carry_rows(int layout, const double* rows, int n_rows, double advance, double max_advance, int n_knots,
                      double delta_t, double* coarse9, double* coarse6, double* knots3, double* station) {
  const Columns c = columns_of(layout);
  const PairColumns seven = pair_carry(c);
  int state = 0;
  if (advance < 0.0) state = 1;
  else if (!(advance <= max_advance)) state = 2;                                          // a NaN, or above the limit
  else if (!(rows[(size_t)(n_rows - 1) * c.fields + c.time] - rows[c.time] > 0.0)) state = 2;
  double nine[256 * kCoarseFields];   // CILQR_DP_MAX_KNOTS rows
  if (state == 0) {
    const double first = rows[c.time] + advance;
    double s = 0.0;
    bool finite = true;
    for (int k = 0; k < n_knots; ++k) {
      const double q = first + k * delta_t;
      const int i = bracket(rows, c.fields, c.time, n_rows, q);
      const double *p0 = rows + (size_t)(i - 1) * c.fields, *p1 = p0 + c.fields;
      double* o = nine + (size_t)k * kCoarseFields;
      o[0] = delta_t * k;
      pair_step(seven, c.time, p0[c.time], p1[c.time], q, p0, p1, o + 2);
      if (k > 0) s = s + std::hypot(o[2] - o[2 - kCoarseFields], o[3] - o[3 - kCoarseFields]);
      o[1] = s;
      finite = finite && std::isfinite(o[2]) && std::isfinite(o[3]) && std::isfinite(o[4]) && std::isfinite(o[6]) &&
               std::isfinite(o[7]) && std::isfinite(o[8]);
    }
    if (!finite) state = 2;
  }
  if (state != 0) std::memset(nine, 0, sizeof(double) * (size_t)n_knots * kCoarseFields);
  static const int six[6] = {2, 3, 4, 6, 7, 8};
  for (int k = 0; k < n_knots; ++k) {
    const double* o = nine + (size_t)k * kCoarseFields;
    if (coarse9 != nullptr) std::memcpy(coarse9 + (size_t)k * kCoarseFields, o, sizeof(double) * kCoarseFields);
    if (coarse6 != nullptr)
      for (int e = 0; e < 6; ++e) std::memcpy(coarse6 + (size_t)k * 6 + e, o + six[e], sizeof(double));
    if (knots3 != nullptr) std::memcpy(knots3 + (size_t)k * 3, o + 2, sizeof(double) * 3);
    if (station != nullptr) station[k] = o[1];
  }
  return state;
}

// ---- stop: brake along the path: the host statement of cilqr_stop_rows and cilqr_stop_rows_batch.  The rule is stated in
// include/cilqr.h ("stop").
constexpr int kStopStopped = 0, kStopMoving = 1, kStopOverrun = 2, kStopRefused = 3;

// one state of the speed chain, and its step k -> k + 1 with jd = jerk * delta_t, hd = 0.5 * delta_t (constexpr: the kernel
// of cilqr_stop_rows_batch runs this very function)
struct StopState {
  double s, v, a;
};
constexpr StopState stop_step(const StopState& c, double a_target, double jd, double hd, double delta_t) {
  if (c.v == 0.0) return StopState{c.s, c.v, 0.0};
  double an = a_target;
  if (c.a > a_target) {
    an = c.a + jd;
    if (!(an > a_target)) an = a_target;   // max(a + jd, a_target)
  } else if (c.a < a_target) {
    an = c.a - jd;
    if (!(an < a_target)) an = a_target;   // min(a - jd, a_target)
  }
  const double vn = c.v + hd * (c.a + an);
  if (!(vn > 0.0)) {   // the stop lies inside the step
    const double f = c.v / (c.v - vn);
    return StopState{c.s + (0.5 * c.v) * (f * delta_t), 0.0, 0.0};
  }
  return StopState{c.s + hd * (c.v + vn), vn, an};
}

// what a stop row takes from the path, as an instance of the pair step: x y theta kappa delta of `from` to where `to` keeps them
constexpr PairColumns pair_stop(const RowColumns& from, const RowColumns& to) {
  const int f[5] = {from.x, from.y, from.theta, from.kappa, from.delta}, t[5] = {to.x, to.y, to.theta, to.kappa, to.delta};
  PairColumns L{};
  for (int e = 0; e < 5; ++e) L = pair_with(L, f[e], t[e], e == 2 ? kPairSlerp : kPairLerp);
  return L;
}

// rows [n_knots][fields] of `layout` as plan rows [n_knots][11] with the station key of the rule in the station column; a
// column the layout lacks is 0
inline void stop_plan_rows(int layout, const double* rows, int n_knots, double* plan) {
  const Columns c = columns_of(layout), P = columns_of(1);
  const ColumnMap from = column_map(P, c);
  double key = 0.0;
  for (int i = 0; i < n_knots; ++i) {
    const double* r = rows + (size_t)i * c.fields;
    double* o = plan + (size_t)i * P.fields;
    for (int f = 0; f < P.fields; ++f) {
      o[f] = 0.0;
      if (from.col[f] >= 0) std::memcpy(o + f, r + from.col[f], sizeof(double));
    }
    if (c.station < 0) {
      if (i > 0) key = key + std::hypot(r[c.x] - r[c.x - c.fields], r[c.y] - r[c.y - c.fields]);
      o[P.station] = key;
    }
  }
}

// rows [n_knots][fields] and ONE profile -> out_rows [n_out][11] (may be null); returns the status.  start_va: null, or
// (v0, a0).  The arguments are taken as checked (cilqr_stop_rows).
inline int stop_rows(int layout, const double* rows, int n_knots, double a_target, double jerk, const double* start_va,
                     double delta_t, int n_out, double* out_rows, int* stop_knot, double* travel) {
  const Columns P = columns_of(1);
  double plan[256 * 11], img[256 * 11];   // CILQR_DP_MAX_KNOTS rows
  stop_plan_rows(layout, rows, n_knots, plan);
  const double v0 = start_va ? start_va[0] : plan[P.v], a0 = start_va ? start_va[1] : plan[P.a];
  const double key0 = plan[P.station], s_end = plan[(size_t)(n_knots - 1) * P.fields + P.station];
  int status = kStopStopped, knot = -1;
  double went = 0.0;
  if (!std::isfinite(v0) || !std::isfinite(a0) || v0 < 0.0) {
    status = kStopRefused;
  } else {
    const double jd = jerk * delta_t, hd = 0.5 * delta_t;
    StopState c{key0, v0, a0};
    bool overrun = false, finite = true;
    const PairColumns five = pair_stop(P, P);
    for (int k = 0; k < n_out; ++k) {
      if (k > 0) c = stop_step(c, a_target, jd, hd, delta_t);
      if (c.s > s_end) overrun = true;
      if (knot < 0 && c.v == 0.0) knot = k;
      const double q = c.s > s_end ? s_end : c.s;
      const int i = bracket(plan, P.fields, P.station, n_knots, q);
      const double *p0 = plan + (size_t)(i - 1) * P.fields, *p1 = p0 + P.fields;
      double* o = img + (size_t)k * P.fields;
      o[P.time] = plan[P.time] + delta_t * k;
      o[P.station] = q;
      pair_step(five, P.station, p0[P.station], p1[P.station], q, p0, p1, o);
      o[P.v] = c.v;
      o[P.a] = c.a;
      o[P.jerk] = 0.0;
      o[P.rate] = 0.0;
      if (k > 0) {
        o[P.jerk - P.fields] = (o[P.a] - o[P.a - P.fields]) / delta_t;
        o[P.rate - P.fields] = (o[P.delta] - o[P.delta - P.fields]) / delta_t;
      }
    }
    for (int e = 0; e < n_out * P.fields; ++e) finite = finite && std::isfinite(img[e]);
    went = c.s - key0;
    if (!finite) status = kStopRefused;
    else if (overrun) status = kStopOverrun;
    else if (c.v > 0.0) status = kStopMoving;
  }
  if (status == kStopRefused) {
    std::memset(img, 0, sizeof(double) * (size_t)n_out * P.fields);
    knot = -1;
    went = 0.0;
  }
  if (out_rows != nullptr) std::memcpy(out_rows, img, sizeof(double) * (size_t)n_out * P.fields);
  if (stop_knot != nullptr) *stop_knot = knot;
  if (travel != nullptr) *travel = went;
  return status;
}

// ---- the Frenet frame of a centre line (DiscretizedTrajectory::GetProjection / GetCartesian, cpp:138-196): the host
// statement of cilqr_frenet_rows / cilqr_cartesian_points.  The rule is stated in include/cilqr.h ("frenet").
// center [n][7] = s x y theta kappa left_bound right_bound, n >= 2.
constexpr int kCenterFields = 7;
constexpr int kFrenetFields = 8;   // station, lateral, then x y theta kappa left_bound right_bound of the projected point

// where a layout keeps x (y follows it) and how many doubles a row has; CILQR_ROWS_POINTS too.  false: no such layout
inline bool point_columns(int layout, int* fields, int* x_col) {
  const RowColumns c = row_columns(layout);
  if (c.x < 0) return false;   // CILQR_ROWS_CONTROLS and every unknown layout
  *fields = c.fields;
  *x_col = c.x;
  return true;
}

// sin and cos of one angle as the reference's build evaluates them: g++ -O2 turns its std::sin / std::cos of one argument
// into ONE sincos call, and glibc's sincos differs from its sin / cos in the last bit for some angles
inline void sin_cos(double angle, double* sn, double* cs) {
#if defined(__GLIBC__)
  ::sincos(angle, sn, cs);
#else
  *sn = std::sin(angle);
  *cs = std::cos(angle);
#endif
}

// LinearInterpolateTrajectory (cpp:66-87) on centre rows: out[7]
inline void interpolate_center(const double* p0, const double* p1, double s, double* out) {
  pair_step(pair_center(), 0, p0[0], p1[0], s, p0, p1, out);
}

// QueryNearestPoint (cpp:138-157): the first index with the smallest squared distance; 0 when none is below DBL_MAX
inline int nearest_center_point(const double* center, int n_center, double px, double py) {
  int at = 0;
  double nearest = 1.7976931348623157e308;   // std::numeric_limits<double>::max()
  for (int i = 0; i < n_center; ++i) {
    const double dx = center[(size_t)i * kCenterFields + 1] - px, dy = center[(size_t)i * kCenterFields + 2] - py;
    const double d = dx * dx + dy * dy;
    if (d < nearest) {
      at = i;
      nearest = d;
    }
  }
  return at;
}

// GetProjection (cpp:159-190): out[8].  `cross` (optional) receives what the sign of the lateral offset was taken from.
inline void project_point(const double* center, int n_center, double px, double py, double* out, double* cross = nullptr) {
  const int at = nearest_center_point(center, n_center, px, py);
  const int i0 = at > 0 ? at - 1 : 0;
  const int i1 = at + 1 < n_center - 1 ? at + 1 : n_center - 1;
  double pp[kCenterFields];
  std::memcpy(pp, center + (size_t)at * kCenterFields, sizeof(pp));
  if (i0 < i1) {
    const double* c0 = center + (size_t)i0 * kCenterFields;
    const double* c1 = center + (size_t)i1 * kCenterFields;
    const double v0x = px - c0[1], v0y = py - c0[2];
    const double v1x = c1[1] - c0[1], v1y = c1[2] - c0[2];
    const double v1_norm = std::sqrt(v1x * v1x + v1y * v1y);
    const double dot = v0x * v1x + v0y * v1y;
    const double delta_s = dot / v1_norm;
    interpolate_center(c0, c1, c0[0] + delta_s, pp);
  }
  const double nr_x = px - pp[1], nr_y = py - pp[2];
  double sn, cs;
  sin_cos(pp[3], &sn, &cs);
  const double side = nr_y * cs - nr_x * sn;
  out[0] = pp[0];
  out[1] = std::copysign(std::hypot(nr_x, nr_y), side);
  std::memcpy(out + 2, pp + 1, sizeof(double) * (kCenterFields - 1));
  if (cross != nullptr) *cross = side;
}

// rows [n_rows][fields] of `layout` -> frenet [n_rows][8]; the arguments are taken as checked (cilqr_frenet_rows)
inline void project_rows(const double* center, int n_center, int layout, const double* rows, int n_rows, double* frenet) {
  int fields = 0, xc = 0;
  if (!point_columns(layout, &fields, &xc)) return;
  for (int r = 0; r < n_rows; ++r) {
    const double* p = rows + (size_t)r * fields + xc;
    project_point(center, n_center, p[0], p[1], frenet + (size_t)r * kFrenetFields);
  }
}

// GetCartesian (cpp:192-196) with the heading of the evaluated point: out[3] = x, y, theta
inline void cartesian_point(const double* center, int n_center, double station, double lateral, double* out) {
  const int i = bracket(center, kCenterFields, 0, n_center, station);
  double ref[kCenterFields];
  interpolate_center(center + (size_t)(i - 1) * kCenterFields, center + (size_t)i * kCenterFields, station, ref);
  double sn, cs;
  sin_cos(ref[3], &sn, &cs);
  out[0] = ref[1] - lateral * sn;
  out[1] = ref[2] + lateral * cs;
  out[2] = ref[3];
}

}  // namespace trajectory_queries
}  // namespace cilqr

#endif  // CILQR_TRAJECTORY_QUERIES_HPP_
