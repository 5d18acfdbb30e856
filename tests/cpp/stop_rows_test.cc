// Stand-alone host test of the stop rule as include/cilqr/trajectory_queries.hpp states it (stop_rows, stop_step,
// stop_plan_rows): the header alone, built with g++ -std=c++14 -fsanitize=address,undefined and run as a child process by
// tests/test_stop_cpp.py.  Every array is allocated at exactly its size, so that a read or write past an end is the
// sanitizer's to report: the shapes are n_knots = 2 and 256 with n_out = 1 and 256, every layout.  What is checked besides:
// the dyadic cases whose results are exact (16 m in 32 steps; 14.0625 m with the stop inside a step), the statuses, the zero
// rows of a refusal, and the pose against resample_rows at every row's station.
// Prints "<n> checks, <f> failures"; the exit status is 0 only without failures.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "cilqr/trajectory_queries.hpp"

using namespace cilqr;
namespace tq = cilqr::trajectory_queries;

static int g_checks = 0, g_failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failures;                                                        \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

// plan rows of a path along a gentle arc, ds between knots, then in `layout` through the column map
static std::vector<double> path(int layout, int n_knots, double ds, double kappa, double v, double a) {
  const RowColumns P = row_columns(1), c = tq::columns_of(layout);
  const ColumnMap from = column_map(c, P);
  std::vector<double> rows((size_t)n_knots * c.fields);
  for (int i = 0; i < n_knots; ++i) {
    double p[11];
    const double s = ds * i, th = kappa * s;
    p[P.time] = 0.5 + 0.1 * i;  p[P.station] = s;  p[P.theta] = th;  p[P.kappa] = kappa;  p[P.v] = v;  p[P.a] = a;
    p[P.x] = kappa == 0.0 ? s : std::sin(th) / kappa;
    p[P.y] = kappa == 0.0 ? 0.0 : (1.0 - std::cos(th)) / kappa;
    p[P.delta] = 0.01 * (i % 7);  p[P.jerk] = 0.3;  p[P.rate] = -0.2;
    for (int f = 0; f < c.fields; ++f) rows[(size_t)i * c.fields + f] = p[from.col[f]];
  }
  return rows;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

static void check_shapes() {
  const int knots[] = {2, 51, 256}, outs[] = {1, 2, 256};
  for (int layout = 0; layout < 3; ++layout)
    for (int K : knots)
      for (int N : outs) {
        const std::vector<double> rows = path(layout, K, 30.0 / (K - 1), 0.03, 7.0, -0.5);
        std::vector<double> out((size_t)N * 11, -7.0);
        int knot = -9;
        double travel = -7.0;
        const int st = tq::stop_rows(layout, rows.data(), K, -2.0, -4.0, nullptr, 0.05, N, out.data(), &knot, &travel);
        CHECK(st == (N == 256 ? tq::kStopStopped : tq::kStopMoving));
        CHECK((knot >= 0) == (st == tq::kStopStopped) && travel >= 0.0 && travel < 30.0);
        // the pose is EvaluateStation of the plan rows at the row's station
        std::vector<double> plan((size_t)K * 11), want((size_t)N * 11), q((size_t)N);
        tq::stop_plan_rows(layout, rows.data(), K, plan.data());
        for (int k = 0; k < N; ++k) q[k] = out[(size_t)k * 11 + 1];
        tq::resample_rows(1, plan.data(), K, 1, q.data(), N, want.data());
        bool pose = true, rest = true;
        for (int k = 0; k < N; ++k) {
          const double *o = &out[(size_t)k * 11], *w = &want[(size_t)k * 11];
          for (int f : {2, 3, 4, 5, 8}) pose = pose && same_bits(o[f], w[f]);
          rest = rest && o[0] == plan[0] + 0.05 * k && std::isfinite(o[9]) && std::isfinite(o[10]);
        }
        CHECK(pose);
        CHECK(rest);
        CHECK(out[(size_t)(N - 1) * 11 + 9] == 0.0 && out[(size_t)(N - 1) * 11 + 10] == 0.0);
        // the summaries alone, and the rows alone
        CHECK(tq::stop_rows(layout, rows.data(), K, -2.0, -4.0, nullptr, 0.05, N, nullptr, &knot, &travel) == st);
        CHECK(tq::stop_rows(layout, rows.data(), K, -2.0, -4.0, nullptr, 0.05, N, out.data(), nullptr, nullptr) == st);
      }
}

static void check_exact_cases() {
  const std::vector<double> rows = path(1, 41, 1.0, 0.0, 8.0, -2.0);
  std::vector<double> out((size_t)40 * 11);
  int knot = -9;
  double travel = -7.0;
  CHECK(tq::stop_rows(1, rows.data(), 41, -2.0, -4.0, nullptr, 0.125, 40, out.data(), &knot, &travel) == tq::kStopStopped);
  CHECK(travel == 16.0 && knot == 32);
  CHECK(out[32 * 11 + 1] == 16.0 && out[32 * 11 + 2] == 16.0 && out[32 * 11 + 6] == 0.0 && out[32 * 11 + 7] == 0.0);
  CHECK(out[31 * 11 + 9] == 16.0 && out[30 * 11 + 9] == 0.0);   // the jump of a to 0 at the stop shows in jerk
  const double va[2] = {7.5, -2.0};
  CHECK(tq::stop_rows(1, rows.data(), 41, -2.0, -4.0, va, 0.5, 12, out.data(), &knot, &travel) == tq::kStopStopped);
  CHECK(travel == 14.0625 && knot == 8);
  // the step itself: towards the target from either side, holding it, standing
  tq::StopState c = tq::stop_step(tq::StopState{0.0, 8.0, 0.0}, -2.0, -0.5, 0.0625, 0.125);
  CHECK(c.a == -0.5 && c.v == 7.96875 && c.s == 0.998046875);
  c = tq::stop_step(tq::StopState{0.0, 8.0, -4.0}, -2.0, -0.5, 0.0625, 0.125);
  CHECK(c.a == -3.5 && c.v == 7.53125);
  c = tq::stop_step(tq::StopState{0.0, 8.0, -1.75}, -2.0, -0.5, 0.0625, 0.125);
  CHECK(c.a == -2.0);
  c = tq::stop_step(tq::StopState{3.0, 0.0, -1.0}, -2.0, -0.5, 0.0625, 0.125);
  CHECK(c.s == 3.0 && c.v == 0.0 && c.a == 0.0);
}

static void check_statuses() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> out((size_t)40 * 11, -7.0);
  int knot = -9;
  double travel = -7.0;
  const std::vector<double> brief = path(0, 11, 1.0, 0.0, 8.0, -2.0);
  CHECK(tq::stop_rows(0, brief.data(), 11, -2.0, -4.0, nullptr, 0.125, 40, out.data(), &knot, &travel) == tq::kStopOverrun);
  CHECK(travel == 16.0 && out[39 * 11 + 1] == 10.0 && out[39 * 11 + 2] == 10.0);   // the rows stay on the path
  const double bad[][2] = {{nan, 0.0}, {8.0, nan}, {-1.0, 0.0}, {std::numeric_limits<double>::infinity(), 0.0}};
  for (const auto& va : bad) {
    std::fill(out.begin(), out.end(), -7.0);
    CHECK(tq::stop_rows(0, brief.data(), 11, -2.0, -4.0, va, 0.125, 40, out.data(), &knot, &travel) == tq::kStopRefused);
    bool zero = knot == -1 && travel == 0.0;
    for (double v : out) zero = zero && v == 0.0;
    CHECK(zero);
  }
  std::vector<double> holed = path(2, 51, 0.6, 0.05, 6.0, -1.0);
  holed[(size_t)4 * 9 + 5] = nan;   // a NaN curvature inside the stop distance
  CHECK(tq::stop_rows(2, holed.data(), 51, -2.0, -4.0, nullptr, 0.1, 40, out.data(), &knot, &travel) == tq::kStopRefused);
  holed[(size_t)4 * 9 + 5] = 0.05;
  holed[(size_t)45 * 9 + 5] = nan;  // ... beyond it
  CHECK(tq::stop_rows(2, holed.data(), 51, -2.0, -4.0, nullptr, 0.1, 40, out.data(), &knot, &travel) == tq::kStopStopped);
}

int main() {
  check_shapes();
  check_exact_cases();
  check_statuses();
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures == 0 ? 0 : 1;
}
