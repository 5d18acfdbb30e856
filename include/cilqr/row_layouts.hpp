// include/cilqr/row_layouts.hpp -- where each row layout of include/cilqr.h (CILQR_ROWS_*) keeps what a rule names: the ONE
// statement of the column numbers.  The host statements (trajectory_queries.hpp, tracker.hpp, constraint_margins.hpp), the
// entry points and the kernels of cilqr_amd/csrc all take their numbers from here; a rule names fields, never numbers.
// C++14, constexpr, no HIP.  A new layout, or a new column of one, is added here and nowhere else ("row layouts").
#ifndef CILQR_ROW_LAYOUTS_HPP_
#define CILQR_ROW_LAYOUTS_HPP_

#include <cstdint>

namespace cilqr {

// doubles per row and the column of every named field; -1: the layout has no such column.  fields = 0: no such layout
struct RowColumns {
  int fields, time, station, x, y, theta, kappa, v, a, delta, jerk, rate;
};

constexpr RowColumns row_columns(int layout) {
  switch (layout) {   //                fields time  s   x   y  theta kappa v   a  delta jerk rate
    case 0: return RowColumns{10, 0, -1, 1, 2, 3, 7, 4, 5, 6, 8, 9};             // CILQR_ROWS_TRAJ
    case 1: return RowColumns{11, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10};             // CILQR_ROWS_PLAN
    case 2: return RowColumns{9, 0, 1, 2, 3, 4, 5, 6, 7, 8, -1, -1};             // CILQR_ROWS_COARSE
    case 3: return RowColumns{2, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 1};      // CILQR_ROWS_CONTROLS
    case 4: return RowColumns{2, -1, -1, 0, 1, -1, -1, -1, -1, -1, -1, -1};      // CILQR_ROWS_POINTS
  }
  return RowColumns{0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
}

// the three layouts whose rows are trajectory points (TRAJ, PLAN, COARSE); fields = 0 for every other value
constexpr RowColumns trajectory_columns(int layout) { return row_columns(layout >= 0 && layout <= 2 ? layout : -1); }

// Thin views for the two rules whose kernels carry their columns as launch parameters: what the rule reads, by name.
// the audits (collisions, clearance): time and the pose
struct PoseColumns {
  int fields, time, x, y, theta;
};
constexpr PoseColumns pose_columns(int layout) {
  const RowColumns c = trajectory_columns(layout);
  return PoseColumns{c.fields, c.time, c.x, c.y, c.theta};
}
// the constraint margins: the pose, the state and the controls (jerk = -1: the layout has none)
struct StateColumns {
  int fields, x, y, theta, v, a, delta, jerk, rate;
};
constexpr StateColumns state_columns(int layout) {
  const RowColumns c = trajectory_columns(layout);
  return StateColumns{c.fields, c.x, c.y, c.theta, c.v, c.a, c.delta, c.jerk, c.rate};
}

// the layout of rows `fields` doubles wide, for kernels templated on the width: 9, 10, 11, and POINTS for 2 (CONTROLS, as
// wide, is never dispatched by width); -1: no such width
constexpr int layout_of_fields(int fields) { return fields == 10 ? 0 : fields == 11 ? 1 : fields == 9 ? 2 : fields == 2 ? 4 : -1; }
constexpr RowColumns columns_of_fields(int fields) { return row_columns(layout_of_fields(fields)); }

// for every column of a row of `to`, the column of `from` that has the same name; -1: `from` has none (and past to.fields)
constexpr int kMaxRowFields = 11;
struct ColumnMap {
  int col[kMaxRowFields];
};
constexpr ColumnMap column_map(const RowColumns& to, const RowColumns& from) {
  const int t[] = {to.time, to.station, to.x, to.y, to.theta, to.kappa, to.v, to.a, to.delta, to.jerk, to.rate};
  const int f[] = {from.time, from.station, from.x, from.y, from.theta, from.kappa, from.v, from.a, from.delta, from.jerk, from.rate};
  ColumnMap m{};
  for (int c = 0; c < kMaxRowFields; ++c) m.col[c] = -1;
  for (int e = 0; e < 11; ++e)
    if (t[e] >= 0) m.col[t[e]] = f[e];
  return m;
}

}  // namespace cilqr

#endif  // CILQR_ROW_LAYOUTS_HPP_
