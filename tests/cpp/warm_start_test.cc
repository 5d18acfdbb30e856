// IlqrOptimizer::WarmStart of include/cilqr/ilqr_optimizer.hpp: Plan, WarmStart(previous), Plan, then a Plan without it.
// The reference's types come from tests/cpp/reference_types.hpp, as in adapter_test.cc (same scene file).
//
//   warm_start_test <scene.bin> <out.bin>
// scene.bin: int32 K, cmax, nl, nr | start[4] | coarse[K][6] | counts[K] (int32) |
//            corridor[K][cmax][3] | left[nl][7] | right[nr][7]
// out.bin:   int32 plans_ok, n_iter_trajs of the three plans | traj of plan 1 [K][10] | iter_trajs[0] of plan 2 [K][10] |
//            traj of plan 2 [K][10] | traj of plan 3 [K][10] | iter_trajs[0] of plan 1 and of plan 3 [K][10] each
#include <cstdio>
#include <cstdlib>

#include "cilqr/ilqr_optimizer.hpp"
#include "reference_types.hpp"

namespace planning {
using IlqrOptimizer = cilqr::IlqrOptimizerT<TrajectoryPoint, DiscretizedTrajectory, CorridorConstraints, LaneConstraints,
                                            IlqrConfig, VehicleParam, Cost>;
}

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  using namespace planning;
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hdr[4];
  if (!rd(f, hdr, 4)) return 4;
  const int K = hdr[0], cmax = hdr[1], nl = hdr[2], nr = hdr[3];
  std::vector<double> start(4), coarse((size_t)K * 6), cor((size_t)K * cmax * 3), left((size_t)nl * 7), right((size_t)nr * 7);
  std::vector<int32_t> counts(K);
  if (!rd(f, start.data(), 4) || !rd(f, coarse.data(), coarse.size()) || !rd(f, counts.data(), counts.size()) ||
      !rd(f, cor.data(), cor.size()) || !rd(f, left.data(), left.size()) || !rd(f, right.data(), right.size()))
    return 5;
  std::fclose(f);

  TrajectoryPoint st;
  st.x = start[0]; st.y = start[1]; st.theta = start[2]; st.velocity = start[3];
  std::vector<TrajectoryPoint> pts(K);
  for (int i = 0; i < K; ++i) {
    pts[i].time = 0.1 * i;
    pts[i].x = coarse[i * 6 + 0]; pts[i].y = coarse[i * 6 + 1]; pts[i].theta = coarse[i * 6 + 2];
    pts[i].velocity = coarse[i * 6 + 3]; pts[i].a = coarse[i * 6 + 4]; pts[i].delta = coarse[i * 6 + 5];
  }
  DiscretizedTrajectory coarse_traj(pts);
  CorridorConstraints corridor(K);
  for (int i = 0; i < K; ++i)
    for (int c = 0; c < counts[i]; ++c) {
      const double* p = &cor[((size_t)i * cmax + c) * 3];
      corridor[i].push_back(Vector3d(p[0], p[1], p[2]));
    }
  auto lanes = [](const std::vector<double>& t, int n) {
    LaneConstraints out;
    for (int k = 0; k < n; ++k) {
      const double* r = &t[(size_t)k * 7];
      out.push_back({Vector3d(r[0], r[1], r[2]), math::LineSegment2d(math::Vec2d(r[3], r[4]), math::Vec2d(r[5], r[6]))});
    }
    return out;
  };
  const LaneConstraints l = lanes(left, nl), r = lanes(right, nr);

  IlqrConfig config;
  VehicleParam vehicle;
  IlqrOptimizer opt(config, vehicle, 0.1 * (K - 1), 0.1);
  DiscretizedTrajectory first, second, third;
  std::vector<DiscretizedTrajectory> it1, it2, it3;
  const bool ok1 = opt.Plan(st, coarse_traj, corridor, l, r, &first, &it1);
  opt.WarmStart(first);
  const bool ok2 = opt.Plan(st, coarse_traj, corridor, l, r, &second, &it2);
  const bool ok3 = opt.Plan(st, coarse_traj, corridor, l, r, &third, &it3);   // armed for one Plan only
  const bool ok = ok1 && ok2 && ok3 && !it1.empty() && !it2.empty() && !it3.empty();

  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  int32_t oh[4] = {(int32_t)(ok ? 1 : 0), (int32_t)it1.size(), (int32_t)it2.size(), (int32_t)it3.size()};
  std::fwrite(oh, sizeof(int32_t), 4, o);
  auto dump = [&](const DiscretizedTrajectory& t) {
    for (const auto& p : t.trajectory()) {
      const double row[10] = {p.time, p.x, p.y, p.theta, p.velocity, p.a, p.delta, p.kappa, p.jerk, p.delta_rate};
      std::fwrite(row, sizeof(double), 10, o);
    }
  };
  if (ok) {
    dump(first);
    dump(it2[0]);
    dump(second);
    dump(third);
    dump(it1[0]);
    dump(it3[0]);
  }
  std::fclose(o);
  return ok ? 0 : 1;
}
