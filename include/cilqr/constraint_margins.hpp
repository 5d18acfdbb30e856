// include/cilqr/constraint_margins.hpp -- how far every knot of a trajectory stays inside the constraints its solve was
// given: the corridor half-planes, the nearest segment of the left and of the right lane table, the state and control
// bounds.  The host statement of cilqr_constraint_margins, which cilqr_constraint_margins_batch is held to.
// Header-only, C++14, no HIP, no Eigen.  The rule is stated once, in include/cilqr.h ("constraint margins"); this file
// follows it step by step.  Every product and sum is meant to be rounded once: build without FMA contraction
// (-ffp-contract=off) to get the bits the C call returns.
#ifndef CILQR_CONSTRAINT_MARGINS_HPP_
#define CILQR_CONSTRAINT_MARGINS_HPP_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "row_math.hpp"

namespace cilqr {
namespace constraint_margins {

constexpr int kFields = 8;        // corridor, left lane, right lane, velocity, acceleration, steering, jerk, steering rate
constexpr int kWhichFields = 6;   // corridor disc, corridor plane, left disc, left segment, right disc, right segment
constexpr int kLaneRowFields = 7; // a b c start_x start_y end_x end_y
constexpr int kMaxDiscs = 16;
constexpr double kInf = std::numeric_limits<double>::infinity();

// what the rule reads of a row (row_layouts.hpp); fields = 0: no such layout, jerk = -1: the layout has no control columns
using Columns = StateColumns;
constexpr Columns columns_of(int layout) { return state_columns(layout); }

// (hypot is row_math.hpp's hypot_ref: the value does not depend on the C library the caller links)

// what the rule takes from the configuration (any struct with cilqr_config's field names)
struct Vehicle {
  int n_disc = 0;
  double disc_off[kMaxDiscs] = {};
  double shrink_corridor = 0.0, shrink_lane = 0.0;
  double max_velocity = 0.0, min_acceleration = 0.0, max_acceleration = 0.0;
  double jerk_min = 0.0, jerk_max = 0.0, delta_min = 0.0, delta_max = 0.0, delta_rate_min = 0.0, delta_rate_max = 0.0;
};
template <class Config>
inline Vehicle vehicle_of(const Config& c) {
  Vehicle v;
  v.n_disc = c.num_of_disc < kMaxDiscs ? c.num_of_disc : kMaxDiscs;
  const double length = c.front_hang + c.wheel_base + c.rear_hang;
  const double disc_radius = std::hypot(c.width / 2.0, length / 2.0 / c.num_of_disc);   // CalculateDiscRadius cc:97-104
  const double L = (c.rear_hang + c.wheel_base + c.front_hang) / c.num_of_disc;
  for (int j = 0; j < v.n_disc; ++j) v.disc_off[j] = L * (j - 0.5) - c.rear_hang;          // cc:564
  v.shrink_corridor = disc_radius + c.safe_margin;                                         // cc:448
  v.shrink_lane = disc_radius;                                                             // cc:463
  v.max_velocity = c.max_velocity; v.min_acceleration = c.min_acceleration; v.max_acceleration = c.max_acceleration;
  v.jerk_min = c.jerk_min; v.jerk_max = c.jerk_max; v.delta_min = c.delta_min; v.delta_max = c.delta_max;
  v.delta_rate_min = c.delta_rate_min; v.delta_rate_max = c.delta_rate_max;
  return v;
}

// ShrinkConstraints + NormalizeHalfPlane (cc:438-495) on one plane.  `guard`: the corridor's rule for a non-finite result
struct Plane {
  double a, b, c;
};
inline Plane shrink_normalise(double a, double b, double c, double shrink, bool guard) {
  c = c - shrink * (a * a + b * b) / hypot_ref(a, b);
  const double nrm = hypot_ref(hypot_ref(a, b), c);
  Plane p{a / nrm, b / nrm, c / nrm};
  if (guard && !(std::isfinite(p.a) && std::isfinite(p.b) && std::isfinite(p.c))) p = Plane{0.0, 0.0, -kInf};
  return p;
}
inline double no_nan(double m) { return m != m ? -kInf : m; }
// metres by which (px, py) is inside the plane; h = hypot_ref(p.a, p.b)
inline double plane_margin(const Plane& p, double h, double px, double py) {
  const double g = p.a * px + p.b * py - p.c;
  return no_nan(-g / h);
}

// one lane row as the solver prepares it: the shrunk, normalised plane and LineSegment2d's constructor
// (line_segment2d.cpp:38-48)
struct Segment {
  Plane plane;
  double sx, sy, ux, uy, len, ex, ey;
};
inline void prepare_lane(const double* rows7, int n, double shrink, std::vector<Segment>* out) {
  out->resize((size_t)(n > 0 ? n : 0));
  for (int k = 0; k < n; ++k) {
    const double* r = rows7 + (size_t)k * kLaneRowFields;
    Segment& s = (*out)[(size_t)k];
    s.plane = shrink_normalise(r[0], r[1], r[2], shrink, false);
    s.sx = r[3]; s.sy = r[4]; s.ex = r[5]; s.ey = r[6];
    const double dx = s.ex - s.sx, dy = s.ey - s.sy;
    s.len = hypot_ref(dx, dy);
    s.ux = (s.len <= kMathEps) ? 0.0 : dx / s.len;
    s.uy = (s.len <= kMathEps) ? 0.0 : dy / s.len;
  }
}
// LineSegment2d::DistanceTo (line_segment2d.cpp:61-75)
inline double segment_distance(const Segment& s, double px, double py) {
  const double x0 = px - s.sx, y0 = py - s.sy;
  if (s.len <= kMathEps) return hypot_ref(x0, y0);
  const double proj = x0 * s.ux + y0 * s.uy;
  if (proj <= 0.0) return hypot_ref(x0, y0);
  if (proj >= s.len) return hypot_ref(px - s.ex, py - s.ey);
  return std::fabs(x0 * s.uy - y0 * s.ux);
}
// the same cases on squares alone: what CILQR_OPT_EXACT_LANE_TIES = 0 compares
inline double segment_distance2(const Segment& s, double px, double py) {
  const double x0 = px - s.sx, y0 = py - s.sy;
  const double d_start = x0 * x0 + y0 * y0;
  const double proj = x0 * s.ux + y0 * s.uy;
  const double x1 = px - s.ex, y1 = py - s.ey;
  const double d_end = x1 * x1 + y1 * y1;
  const double c = x0 * s.uy - y0 * s.ux;
  const double d_perp = c * c;
  return (s.len <= kMathEps || proj <= 0.0) ? d_start : (proj >= s.len ? d_end : d_perp);
}
// FindNeastLaneSegment (cc:605-618): strict `<`, the first index wins; 0 when no distance is below DBL_MAX
inline int nearest_segment(const std::vector<Segment>& tab, double px, double py, bool exact_ties) {
  double best = std::numeric_limits<double>::max();
  int at = 0;
  for (size_t k = 0; k < tab.size(); ++k) {
    const double d = exact_ties ? segment_distance(tab[k], px, py) : segment_distance2(tab[k], px, py);
    if (d < best) {
      best = d;
      at = (int)k;
    }
  }
  return at;
}

// min(-g1, -g2) of one bound family, the first of equals
inline double pair_margin(double g1, double g2) {
  const double m1 = no_nan(-g1), m2 = no_nan(-g2);
  return m2 < m1 ? m2 : m1;
}

// One knot.  planes [n][3] raw, n already clamped; m [8]; w [6]
inline void knot_margins(const Vehicle& V, bool exact_ties, const Columns& c, const double* row, bool last, const double* planes,
                         int n, const std::vector<Segment>& left, const std::vector<Segment>& right, double* m, int32_t* w) {
  const double x = row[c.x], y = row[c.y], theta = row[c.theta];
  const double cs = std::cos(theta), sn = std::sin(theta);
  double px[kMaxDiscs], py[kMaxDiscs];
  for (int j = 0; j < V.n_disc; ++j) {
    px[j] = x + V.disc_off[j] * cs;
    py[j] = y + V.disc_off[j] * sn;
  }
  for (int e = 0; e < kWhichFields; ++e) w[e] = -1;
  // corridor: discs outside, planes inside (cc:562-574)
  m[0] = kInf;
  std::vector<Plane> pl((size_t)n);
  std::vector<double> ph((size_t)n);
  for (int k = 0; k < n; ++k) {
    pl[(size_t)k] = shrink_normalise(planes[3 * k], planes[3 * k + 1], planes[3 * k + 2], V.shrink_corridor, true);
    ph[(size_t)k] = hypot_ref(pl[(size_t)k].a, pl[(size_t)k].b);
  }
  for (int j = 0; j < V.n_disc; ++j)
    for (int k = 0; k < n; ++k) {
      const double v = plane_margin(pl[(size_t)k], ph[(size_t)k], px[j], py[j]);
      if (v < m[0]) {
        m[0] = v;
        w[0] = j;
        w[1] = k;
      }
    }
  // lanes (cc:589-600)
  for (int side = 0; side < 2; ++side) {
    const std::vector<Segment>& tab = side ? right : left;
    double best = kInf;
    for (int j = 0; j < V.n_disc; ++j) {
      const int seg = nearest_segment(tab, px[j], py[j], exact_ties);
      const Plane& p = tab[(size_t)seg].plane;
      const double v = plane_margin(p, hypot_ref(p.a, p.b), px[j], py[j]);
      if (v < best) {
        best = v;
        w[2 + 2 * side] = j;
        w[3 + 2 * side] = seg;
      }
    }
    m[1 + side] = best;
  }
  // bounds (cc:523-528, 543-546)
  const double v = row[c.v], a = row[c.a], delta = row[c.delta];
  m[3] = pair_margin(-v, v - V.max_velocity);
  m[4] = pair_margin(a - V.max_acceleration, V.min_acceleration - a);
  m[5] = pair_margin(delta - V.delta_max, V.delta_min - delta);
  if (c.jerk >= 0 && !last) {
    const double jerk = row[c.jerk], rate = row[c.rate];
    m[6] = pair_margin(jerk - V.jerk_max, V.jerk_min - jerk);
    m[7] = pair_margin(rate - V.delta_rate_max, V.delta_rate_min - rate);
  } else {
    m[6] = kInf;
    m[7] = kInf;
  }
}

// One trajectory: rows [n_knots][fields], corridor [n_knots][cmax][3], count [n_knots] (clamped to 0 ... cmax here).
// margins [n_knots][8] and which [n_knots][6] may be null; min_margin [8], min_knot [8].
inline void problem_margins(const Vehicle& V, bool exact_ties, int layout, const double* rows, int n_knots, const double* corridor,
                            const int32_t* count, int cmax, const std::vector<Segment>& left, const std::vector<Segment>& right,
                            double* margins, int32_t* which, double* min_margin, int32_t* min_knot) {
  const Columns c = columns_of(layout);
  for (int f = 0; f < kFields; ++f) {
    min_margin[f] = kInf;
    min_knot[f] = -1;
  }
  for (int i = 0; i < n_knots; ++i) {
    int n = count[i] < cmax ? count[i] : cmax;
    if (n < 0) n = 0;
    double m[kFields];
    int32_t w[kWhichFields];
    knot_margins(V, exact_ties, c, rows + (size_t)i * c.fields, i == n_knots - 1, corridor + (size_t)i * cmax * 3, n, left, right, m, w);
    for (int f = 0; f < kFields; ++f) {
      if (margins) margins[(size_t)i * kFields + f] = m[f];
      if (m[f] < min_margin[f]) {
        min_margin[f] = m[f];
        min_knot[f] = i;
      }
    }
    if (which)
      for (int e = 0; e < kWhichFields; ++e) which[(size_t)i * kWhichFields + e] = w[e];
  }
}

// bit f: min_margin[f] < -tol[f]; tol == nullptr: zeros
inline uint32_t violated_mask(const double* min_margin, const double* tol) {
  uint32_t mask = 0;
  for (int f = 0; f < kFields; ++f)
    if (min_margin[f] < -(tol ? tol[f] : 0.0)) mask |= 1u << f;
  return mask;
}

}  // namespace constraint_margins
}  // namespace cilqr

#endif  // CILQR_CONSTRAINT_MARGINS_HPP_
