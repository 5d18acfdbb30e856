// include/cilqr/trajectory_queries.hpp -- DiscretizedTrajectory::EvaluateTime / EvaluateStation
// (algorithm/utils/discretized_trajectory.cpp:50-136, math::slerp math_utils.h:208-225) on rows in the layouts of
// include/cilqr.h: the host statement of cilqr_resample_rows, which cilqr_resample_rows_batch is held to bit for bit.
// Header-only, C++14, no HIP.  The rule is stated once, in include/cilqr.h ("resample"); this file follows it step by step.
#ifndef CILQR_TRAJECTORY_QUERIES_HPP_
#define CILQR_TRAJECTORY_QUERIES_HPP_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace cilqr {
namespace trajectory_queries {

constexpr double kPi = 3.14159265358979323846;   // M_PI
constexpr double kMathEpsilon = 1e-10;            // algorithm/math/vec2d.h:33

// where a row layout (CILQR_ROWS_TRAJ 0 / _PLAN 1 / _COARSE 2) keeps what the rule names; fields = 0: no such layout
struct Columns {
  int fields, time, station, theta, control;   // station / control = -1: the layout has none; the controls are two columns
};
inline Columns columns_of(int layout) {
  switch (layout) {
    case 0: return Columns{10, 0, -1, 3, 8};
    case 1: return Columns{11, 0, 1, 4, 9};
    case 2: return Columns{9, 0, 1, 4, -1};
  }
  return Columns{0, 0, -1, 0, -1};
}
// the key column of (layout, key) with key = CILQR_KEY_TIME 0 / CILQR_KEY_STATION 1; -1: no such pair
inline int key_column(int layout, int key) {
  const Columns c = columns_of(layout);
  if (c.fields == 0) return -1;
  if (key == 0) return c.time;
  if (key == 1) return c.station;
  return -1;
}

inline double NormalizeAngle(double angle) {   // math_utils.cpp:53-59
  double a = std::fmod(angle + kPi, 2.0 * kPi);
  if (a < 0.0) a += 2.0 * kPi;
  return a - kPi;
}

inline double slerp(double a0, double t0, double a1, double t1, double t) {   // math_utils.h:208-225
  if (std::fabs(t1 - t0) <= kMathEpsilon) return NormalizeAngle(a0);
  const double a0_n = NormalizeAngle(a0);
  const double a1_n = NormalizeAngle(a1);
  double d = a1_n - a0_n;
  if (d > kPi) d = d - 2 * kPi;
  else if (d < -kPi) d = d + 2 * kPi;
  const double r = (t - t0) / (t1 - t0);
  const double a = a0_n + d * r;
  return NormalizeAngle(a);
}

// the row index i (1 <= i <= n_knots - 1) of p1; p0 is row i - 1.  rows [n_knots][fields], n_knots >= 2.
inline int bracket(const double* rows, int fields, int key_col, int n_knots, double q) {
  int i;
  if (q >= rows[(size_t)(n_knots - 1) * fields + key_col]) {
    i = n_knots - 1;
  } else if (q < rows[key_col]) {
    i = 0;
  } else {   // std::lower_bound's halving, written out: defined for any input
    int first = 0, len = n_knots;
    while (len > 0) {
      const int half = len >> 1;
      if (rows[(size_t)(first + half) * fields + key_col] < q) {
        first += half + 1;
        len -= half + 1;
      } else {
        len = half;
      }
    }
    i = first;
  }
  if (i == 0) i = 1;
  if (i > n_knots - 1) i = n_knots - 1;   // not reached: q < key[K-1] here, so the halving stops at or before K - 1
  return i;
}

// one output row from the pair (p0, p1) of a layout
inline void interpolate(const Columns& c, int key_col, const double* p0, const double* p1, double q, double* out) {
  const double k0 = p0[key_col], k1 = p1[key_col];
  if (std::fabs(k1 - k0) < kMathEpsilon) {
    std::memcpy(out, p0, sizeof(double) * (size_t)c.fields);   // p0, its key column included, as bits
    return;
  }
  const double w = (q - k0) / (k1 - k0);
  for (int f = 0; f < c.fields; ++f) {
    if (f == key_col) {
      out[f] = q;
    } else if (f == c.theta) {
      out[f] = slerp(p0[f], k0, p1[f], k1, q);
    } else if (c.control >= 0 && (f == c.control || f == c.control + 1)) {
      std::memcpy(out + f, p0 + f, sizeof(double));   // a control holds over its step
    } else {
      out[f] = (1 - w) * p0[f] + w * p1[f];
    }
  }
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

}  // namespace trajectory_queries
}  // namespace cilqr

#endif  // CILQR_TRAJECTORY_QUERIES_HPP_
