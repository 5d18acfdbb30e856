// Stand-alone check of include/cilqr/tracker.hpp on the crafted cases of tests/track_cases.py, meant to be built with
// -fsanitize=address,undefined:
//   tracker_test <cases file>
// The file is what track_cases.write_cases produces (little-endian): "TKCASE01", i32 n; per case i32 layout, i32 K,
// i32 n_drive, i32 has_start, 13 doubles of the tracker configuration, 9 of the vehicle, rows [K][F], start6 [6] if
// has_start, i32 ok, expected [n_drive][10].  Rows and results live in heap blocks of exactly their size, so a read or write
// past either end is the sanitizer's to report.  Two things are checked per case:
//   * cilqr::tracker::track_rows gives the expected flag and the expected rows bit for bit (a NaN matches any NaN);
//   * a case in CILQR_ROWS_COARSE layout with a start and n_drive = K also goes through the adapter with the reference's
//     call surface, Tracker(config, vehicle).Plan(start_state, trajectory, &out), against the types of reference_types.hpp
//     (the stand-ins lack the tracker's three configuration structs, which are declared below with the reference's member
//     names): the points it hands back are those rows.
// Exit status 0: all of it held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cilqr/tracker.hpp"
#include "reference_types.hpp"

#ifndef CILQR_TEST_REFERENCE_HEADERS
namespace planning {
struct LateralTrackerConfig {
  double weight_l = 1e-1, weight_theta = 1e-12, weight_delta = 1e-12, weight_delta_rate = 0.1, preview_time = 0.2;
};
struct LongitudinalTrackerConfig {
  double weight_s = 5.0 * 1e-1, weight_v = 1e-12, weight_a = 1e-12, weight_j = 0.1, preview_time = 0.0;
};
struct TrackerConfig {
  double sumulation_dt = 0.01, dt = 0.1, tolerance = 0.01;
  unsigned max_num_iteration = 150;
  LateralTrackerConfig lateral_config;
  LongitudinalTrackerConfig longitudinal_config;
};
}  // namespace planning
#endif

namespace {

using Tracker = cilqr::TrackerT<planning::TrackerConfig, planning::VehicleParam>;

bool read_exact(std::FILE* f, void* dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }

bool same(double a, double b) {
  if (std::isnan(a) && std::isnan(b)) return true;
  return std::memcmp(&a, &b, 8) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  char magic[8];
  int32_t n_cases = 0;
  if (!read_exact(f, magic, 8) || std::memcmp(magic, "TKCASE01", 8) != 0 || !read_exact(f, &n_cases, 4) || n_cases < 0 ||
      n_cases > (1 << 16)) {
    std::fprintf(stderr, "not a cases file\n");
    return 2;
  }
  namespace tk = cilqr::tracker;
  int failures = 0, through_adapter = 0;
  for (int32_t c = 0; c < n_cases; ++c) {
    int32_t head[4];
    double t[13], v[9];
    if (!read_exact(f, head, 16) || !read_exact(f, t, sizeof(t)) || !read_exact(f, v, sizeof(v))) return 2;
    const int32_t layout = head[0], K = head[1], D = head[2], has_start = head[3];
    const int F = tk::follow_columns(layout).fields;
    if (F == 0 || K < 2 || K > (1 << 16) || D < 1 || D > K) return 2;
    std::vector<double> rows((size_t)K * F), start(has_start ? 6 : 0), want((size_t)D * 10), got((size_t)D * 10, -7.0);
    int32_t want_ok = 0;
    if (!read_exact(f, rows.data(), rows.size() * 8) || !read_exact(f, start.data(), start.size() * 8) ||
        !read_exact(f, &want_ok, 4) || !read_exact(f, want.data(), want.size() * 8))
      return 2;
    tk::Config cfg;
    cfg.weight_l = t[0]; cfg.weight_theta = t[1]; cfg.weight_delta = t[2]; cfg.weight_delta_rate = t[3]; cfg.preview_time = t[4];
    cfg.weight_s = t[5]; cfg.weight_v = t[6]; cfg.weight_a = t[7]; cfg.weight_j = t[8];
    cfg.sumulation_dt = t[9]; cfg.dt = t[10]; cfg.tolerance = t[11]; cfg.max_num_iteration = (int)t[12];
    tk::Vehicle veh;
    veh.wheel_base = v[0]; veh.delta_min = v[1]; veh.delta_max = v[2]; veh.delta_rate_min = v[3]; veh.delta_rate_max = v[4];
    veh.jerk_min = v[5]; veh.jerk_max = v[6]; veh.min_acceleration = v[7]; veh.max_acceleration = v[8];
    const bool ok = tk::track_rows(cfg, veh, layout, rows.data(), K, has_start ? start.data() : nullptr, D, got.data());
    if (ok != (want_ok != 0)) {
      std::fprintf(stderr, "case %d: ok %d, expected %d\n", c, (int)ok, want_ok);
      ++failures;
    }
    for (size_t e = 0; e < got.size(); ++e)
      if (!same(got[e], want[e])) {
        std::fprintf(stderr, "case %d: element %zu is %.17g, expected %.17g\n", c, e, got[e], want[e]);
        ++failures;
        break;
      }
    if (layout != 2 || !has_start || D != K) continue;
    // ---- the same through the adapter
    planning::TrackerConfig tc;
    tc.lateral_config.weight_l = t[0]; tc.lateral_config.weight_theta = t[1]; tc.lateral_config.weight_delta = t[2];
    tc.lateral_config.weight_delta_rate = t[3]; tc.lateral_config.preview_time = t[4];
    tc.longitudinal_config.weight_s = t[5]; tc.longitudinal_config.weight_v = t[6]; tc.longitudinal_config.weight_a = t[7];
    tc.longitudinal_config.weight_j = t[8];
    tc.sumulation_dt = t[9]; tc.dt = t[10]; tc.tolerance = t[11]; tc.max_num_iteration = (unsigned)t[12];
    planning::VehicleParam vp;
    vp.wheel_base = v[0]; vp.delta_min = v[1]; vp.delta_max = v[2]; vp.delta_rate_min = v[3]; vp.delta_rate_max = v[4];
    vp.jerk_min = v[5]; vp.jerk_max = v[6]; vp.min_acceleration = v[7]; vp.max_acceleration = v[8];
    std::vector<planning::TrajectoryPoint> pts((size_t)K);
    for (int k = 0; k < K; ++k) {
      const double* r = rows.data() + (size_t)k * F;
      pts[k].time = r[0]; pts[k].s = r[1]; pts[k].x = r[2]; pts[k].y = r[3]; pts[k].theta = r[4]; pts[k].kappa = r[5];
      pts[k].velocity = r[6]; pts[k].a = r[7]; pts[k].delta = r[8];
    }
    planning::TrajectoryPoint s0;
    s0.x = start[0]; s0.y = start[1]; s0.theta = start[2]; s0.velocity = start[3]; s0.a = start[4]; s0.delta = start[5];
    Tracker by_constructor(tc, vp), by_init;
    by_init.Init(tc, vp);
    planning::DiscretizedTrajectory followed(pts), out_a, out_b;
    const bool ok_a = by_constructor.Plan(s0, followed, &out_a), ok_b = by_init.Plan(s0, followed, &out_b);
    ++through_adapter;
    if (ok_a != ok || ok_b != ok) {
      std::fprintf(stderr, "case %d: Plan returns %d / %d, track_rows %d\n", c, (int)ok_a, (int)ok_b, (int)ok);
      ++failures;
      continue;
    }
    if (!ok) {
      if (!out_a.trajectory().empty()) ++failures;   // untouched on failure
      continue;
    }
    for (const planning::DiscretizedTrajectory* o : {&out_a, &out_b}) {
      const std::vector<planning::TrajectoryPoint>& p = o->trajectory();
      if ((int)p.size() != K) {
        ++failures;
        continue;
      }
      for (int k = 0; k < K; ++k) {
        const double* d = got.data() + (size_t)k * 10;
        const double have[10] = {p[k].time, p[k].x, p[k].y, p[k].theta, p[k].velocity, p[k].a, p[k].delta, p[k].kappa, p[k].jerk,
                                 p[k].delta_rate};
        for (int e = 0; e < 10; ++e)
          if (!same(have[e], d[e])) {
            std::fprintf(stderr, "case %d: Plan's point %d differs in field %d\n", c, k, e);
            ++failures;
            k = K;
            break;
          }
      }
    }
  }
  std::fclose(f);
  std::printf("tracker_test (%s): %d cases, %d through the adapter, %d failures\n", CILQR_TEST_TYPES, n_cases, through_adapter,
              failures);
  return failures == 0 && n_cases > 0 && through_adapter > 0 ? 0 : 1;
}
