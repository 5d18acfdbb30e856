// Stand-alone host test of include/cilqr/row_layouts.hpp, the one statement of where a row layout keeps what a rule names,
// and of everything that takes its numbers from it.  Host and device read the same table, so a wrong table agrees with
// itself: here every number is written out a second time as a literal -- the layouts as include/cilqr.h documents them, and
// for every rule the tuple of columns it read before the table existed.  Built with g++ alone (-fsanitize=address,undefined)
// and run as a child process by tests/test_row_layouts.py.  The same facts on a GPU: tests/test_gpu_row_layouts.py.
// Prints "<n> checks, <f> failures"; the exit status is 0 only without failures.
#include <cstdint>
#include <cstdio>

#include "cilqr/constraint_margins.hpp"
#include "cilqr/row_layouts.hpp"
#include "cilqr/tracker.hpp"
#include "cilqr/trajectory_queries.hpp"
#include "solve_io.hpp"

using namespace cilqr;
namespace tq = cilqr::trajectory_queries;
namespace tk = cilqr::tracker;
namespace cm = cilqr::constraint_margins;

static int g_checks = 0, g_failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failures;                                                        \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

static bool same(const RowColumns& c, const int (&w)[12]) {
  const int got[12] = {c.fields, c.time, c.station, c.x, c.y, c.theta, c.kappa, c.v, c.a, c.delta, c.jerk, c.rate};
  for (int e = 0; e < 12; ++e)
    if (got[e] != w[e]) return false;
  return true;
}

// ---- the table against include/cilqr.h: fields, time, station, x, y, theta, kappa, v, a, delta, jerk, rate
static void check_table() {
  CHECK(same(row_columns(0), {10, 0, -1, 1, 2, 3, 7, 4, 5, 6, 8, 9}));
  CHECK(same(row_columns(1), {11, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}));
  CHECK(same(row_columns(2), {9, 0, 1, 2, 3, 4, 5, 6, 7, 8, -1, -1}));
  CHECK(same(row_columns(3), {2, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 1}));
  CHECK(same(row_columns(4), {2, -1, -1, 0, 1, -1, -1, -1, -1, -1, -1, -1}));
  CHECK(CILQR_ROWS_TRAJ == 0 && CILQR_ROWS_PLAN == 1 && CILQR_ROWS_COARSE == 2 && CILQR_ROWS_CONTROLS == 3 && CILQR_ROWS_POINTS == 4);
  CHECK(CILQR_TRAJ_FIELDS == 10 && CILQR_PLAN_FIELDS == 11 && CILQR_COARSE_FIELDS == 9 && CILQR_NU == 2);
  for (int bad : {-1, 5, 6, 1 << 20}) {
    CHECK(row_columns(bad).fields == 0);
    CHECK(trajectory_columns(bad).fields == 0);
  }
  CHECK(trajectory_columns(3).fields == 0 && trajectory_columns(4).fields == 0);
  for (int l = 0; l < 3; ++l) CHECK(trajectory_columns(l).fields == row_columns(l).fields);
  // the width back to the layout, for the kernels templated on it
  CHECK(layout_of_fields(10) == 0 && layout_of_fields(11) == 1 && layout_of_fields(9) == 2 && layout_of_fields(2) == 4);
  for (int bad : {-1, 0, 1, 3, 8, 12}) CHECK(layout_of_fields(bad) == -1 && columns_of_fields(bad).fields == 0);
}

// ---- every rule: what it reads now against the tuple it hard-coded before
static void check_rules() {
  // resample (trajectory_queries.hpp: Columns / columns_of): fields, time, station, theta, first control
  const int resample[3][5] = {{10, 0, -1, 3, 8}, {11, 0, 1, 4, 9}, {9, 0, 1, 4, -1}};
  // carry (carry_columns, which pair_carry and so k_carry take): x y theta kappa v a delta
  const int carry[3][7] = {{1, 2, 3, 7, 4, 5, 6}, {2, 3, 4, 5, 6, 7, 8}, {2, 3, 4, 5, 6, 7, 8}};
  // track (tracker.hpp: FollowColumns): fields, time, station, x, theta, v, a, delta; y follows x
  const int follow[3][8] = {{10, 0, -1, 1, 3, 4, 5, 6}, {11, 0, 1, 2, 4, 6, 7, 8}, {9, 0, 1, 2, 4, 6, 7, 8}};
  // margins (constraint_margins.hpp: Columns, margins.hpp: MarginRows): fields, x, y, theta, v, a, delta, jerk, rate
  const int margins[3][9] = {{10, 1, 2, 3, 4, 5, 6, 8, 9}, {11, 2, 3, 4, 6, 7, 8, 9, 10}, {9, 2, 3, 4, 6, 7, 8, -1, -1}};
  // the audits (collision.hpp: RowLayout): fields, time, x, y, theta
  const int audit[3][5] = {{10, 0, 1, 2, 3}, {11, 0, 2, 3, 4}, {9, 0, 2, 3, 4}};
  for (int l = 0; l < 3; ++l) {
    const tq::Columns r = tq::columns_of(l);
    CHECK(r.fields == resample[l][0] && r.time == resample[l][1] && r.station == resample[l][2] && r.theta == resample[l][3]);
    CHECK(r.jerk == resample[l][4] && r.rate == (resample[l][4] < 0 ? -1 : resample[l][4] + 1));
    const tq::CarryColumns c = tq::carry_columns(tq::columns_of(l));
    for (int e = 0; e < 7; ++e) CHECK(c.col[e] == carry[l][e]);
    const tk::FollowColumns f = tk::follow_columns(l);
    CHECK(f.fields == follow[l][0] && f.time == follow[l][1] && f.station == follow[l][2] && f.x == follow[l][3] &&
          f.y == follow[l][3] + 1 && f.theta == follow[l][4] && f.v == follow[l][5] && f.a == follow[l][6] && f.delta == follow[l][7]);
    const cm::Columns m = cm::columns_of(l);
    const StateColumns d = state_columns(l);   // what a margins launch carries
    const int got[9] = {m.fields, m.x, m.y, m.theta, m.v, m.a, m.delta, m.jerk, m.rate};
    const int dev[9] = {d.fields, d.x, d.y, d.theta, d.v, d.a, d.delta, d.jerk, d.rate};
    for (int e = 0; e < 9; ++e) CHECK(got[e] == margins[l][e] && dev[e] == margins[l][e]);
    const PoseColumns a = pose_columns(l);
    CHECK(a.fields == audit[l][0] && a.time == audit[l][1] && a.x == audit[l][2] && a.y == audit[l][3] && a.theta == audit[l][4]);
  }
  // the key column of (layout, key); station on CILQR_ROWS_TRAJ, an unknown key and the other layouts are refused
  CHECK(tq::key_column(0, 0) == 0 && tq::key_column(1, 0) == 0 && tq::key_column(2, 0) == 0);
  CHECK(tq::key_column(0, 1) == -1 && tq::key_column(1, 1) == 1 && tq::key_column(2, 1) == 1);
  for (int l = 0; l < 3; ++l) CHECK(tq::key_column(l, 2) == -1 && tq::key_column(l, -1) == -1);
  for (int bad : {-1, 3, 4, 5}) {
    CHECK(tq::columns_of(bad).fields == 0 && tq::key_column(bad, 0) == -1 && tq::key_column(bad, 1) == -1);
    CHECK(tk::follow_columns(bad).fields == 0);
    CHECK(cm::columns_of(bad).fields == 0 && state_columns(bad).fields == 0 && pose_columns(bad).fields == 0);
  }
  // frenet (point_columns, k_frenet): doubles per row and the column of x; CILQR_ROWS_POINTS included, CONTROLS not
  const int point[5][2] = {{10, 1}, {11, 2}, {9, 2}, {0, 0}, {2, 0}};
  for (int l = 0; l < 5; ++l) {
    int fields = -7, xc = -7;
    const bool ok = tq::point_columns(l, &fields, &xc);
    CHECK(ok == (l != 3));
    if (l != 3) CHECK(fields == point[l][0] && xc == point[l][1] && row_columns(l).y == xc + 1);
    else CHECK(fields == -7 && xc == -7);
  }
  for (int bad : {-1, 5}) {
    int fields = -7, xc = -7;
    CHECK(!tq::point_columns(bad, &fields, &xc) && fields == -7 && xc == -7);
  }
  // the kernels templated on the width F, against the ternaries they carried
  for (int F : {9, 10, 11}) {
    const RowColumns c = columns_of_fields(F);
    const bool traj = F == 10;
    CHECK(c.fields == F && c.time == 0);
    CHECK(c.x == (traj ? 1 : 2) && c.y == (traj ? 2 : 3) && c.theta == (traj ? 3 : 4) && c.v == (traj ? 4 : 6) &&
          c.a == (traj ? 5 : 7) && c.delta == (traj ? 6 : 8));                         // k_track_gather: XC TH VC AC DC
    CHECK(c.station == (traj ? -1 : 1));                                               // ... kChord, r[1]
    CHECK((c.jerk < 0 ? F : c.jerk) == (F == 9 ? F : F - 2));                          // pair_all: the held columns
    const int from[7] = {traj ? 1 : 2, traj ? 2 : 3, traj ? 3 : 4, traj ? 7 : 5, traj ? 4 : 6, traj ? 5 : 7, traj ? 6 : 8};
    const tq::CarryColumns k = tq::carry_columns(c);                                   // k_carry: pair_carry
    for (int e = 0; e < 7; ++e) CHECK(k.col[e] == from[e]);
  }
  for (int F : {2, 9, 10, 11}) CHECK(columns_of_fields(F).x == (F == 10 ? 1 : F == 2 ? 0 : 2));   // k_frenet: XC
  // k_plan_rows: every column of a plan row from the trajectory column of the same name, the station computed
  const int plan_from_traj[11] = {0, -1, 1, 2, 3, 7, 4, 5, 6, 8, 9};
  const ColumnMap map = column_map(row_columns(CILQR_ROWS_PLAN), row_columns(CILQR_ROWS_TRAJ));
  for (int c = 0; c < 11; ++c) CHECK(map.col[c] == plan_from_traj[c]);
  const ColumnMap self = column_map(row_columns(CILQR_ROWS_COARSE), row_columns(CILQR_ROWS_COARSE));
  for (int c = 0; c < 11; ++c) CHECK(self.col[c] == (c < 9 ? c : -1));
}

// ---- warm rows (solve_io.hpp): doubles per row, rows per problem, first control column
static void check_warm_geometry() {
  for (int K : {2, 3, 51, 256}) {
    int stride = -7, rows_per = -7, col = -7;
    CHECK(cilqr_warm_geometry(CILQR_ROWS_TRAJ, K, &stride, &rows_per, &col) && stride == 10 && rows_per == K && col == 8);
    CHECK(cilqr_warm_geometry(CILQR_ROWS_PLAN, K, &stride, &rows_per, &col) && stride == 11 && rows_per == K && col == 9);
    CHECK(cilqr_warm_geometry(CILQR_ROWS_CONTROLS, K, &stride, &rows_per, &col) && stride == 2 && rows_per == K - 1 && col == 0);
    for (int bad : {CILQR_ROWS_COARSE, CILQR_ROWS_POINTS, -1, 5}) {
      stride = rows_per = col = -7;
      CHECK(!cilqr_warm_geometry(bad, K, &stride, &rows_per, &col) && stride == -7 && rows_per == -7 && col == -7);
    }
  }
}

int main() {
  check_table();
  check_rules();
  check_warm_geometry();
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures == 0 ? 0 : 1;
}
